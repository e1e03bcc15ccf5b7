"""GPU: training the text-to-unit model on the device (parrot_tts_amd/tte_train.py over parrot_tte_train_forward /
parrot_tte_train_backward).

The yardstick is that of tests/test_gpu_aligner_train.py: the restatement (tests/tte_train_ref.py) run on the CPU in fp32 against its
fp64 run on the same inputs, both errors max-abs over the tensor.  Ours against fp64 must be within R x that, with a floor of what is
rounded once anyway: half an fp32 ulp of the tensor's largest magnitude.  R is twice the largest ratio measured on T1 - T4, rounded up
to a power of two (DESIGN.md has the table):
  R = 8      every tensor on T1 and T2, and on T3 and T4 the logits and the gradients of the embeddings, the FFT blocks and the head: the
             largest ratio measured is 4.56 (d duration_predictor.proj.bias on T2), 3.83 outside the duration predictor;
  R_DP = 256 on T3 and T4 ONLY (B S = 3 and 1 source rows), log_dur and the gradients of the duration predictor: 69.5 on T3 (d proj.bias
             under ModelLoss's upstream), 10.3 next, 8.0 on T4.  There the yardstick degenerates: proj.bias is a single number, log_dur
             has 3 or 1 elements, and the restatement's own fp32 error on so few values is a matter of chance: 8.7e-9, 0.07 ulp, where
             ours is 6.0e-7 -- which is log_dur's own rounding (7.4e-7, 3 ulps after two convs, two LayerNorms and a Linear), handed back
             by the loss as 2 (log_dur - target) / n.
With dropout the reference is handed the very masks the kernels apply
(parrot_tte_train_dropout_mask), so the rule is the same.

Trainer loop: the rule with the six losses as the compared tensor, and each loss held to R x its own fp32 error with a floor of
LOSS_FLOOR_ULPS ulps of that loss (derived below); the smaller of the two bounds counts, as in the aligner's file.

The whole file also passes under PARROT_POISON_WS=nan."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tte_train_ref as TR  # noqa: E402
from parrot_tts_amd import synth  # noqa: E402
from parrot_tts_amd import tte_train as TT  # noqa: E402
from parrot_tts_amd.loss import ModelLoss  # noqa: E402
from parrot_tts_amd.tte import Parrot  # noqa: E402

DEV = "cuda:0"
R = 8.0
R_DP = 256.0
# Floor of one loss of the trainer loop, in fp32 ulps of that loss (about 5: ulp = 4.8e-7) -- what is rounded once anyway on T1:
#   1    the loss itself, rounded to fp32 once;
#   1    the logits, rounded to fp32 once: |d nll / d logits[t]|_1 <= 2 per frame and the loss is their mean, so |d loss| <= 2 x half an
#        ulp of the largest logit (|logit| < 8: ulp 4.8e-7) = 4.8e-7;
#   0.5  log_dur, rounded once: |d dur_loss / d log_dur|_1 <= 2 max |log_dur - target| (< 4) x half an ulp of |log_dur| < 4 (1.2e-7);
#   1    from the second step on, every parameter as AdamW stored it in fp32, which moves the logits by about their own rounding again.
# 3.5, rounded up to 4.
LOSS_FLOOR_ULPS = 4
SEED = 42
_cases, _refs = {}, {}


def _case(shape):
    if shape not in _cases:
        _cases[shape] = TR.make_case(shape)
    return _cases[shape]


def _cfg(shape, p_zero):
    cfg = synth.clone_config(_case(shape)[0])
    if p_zero:
        cfg["transformer"]["encoder"]["dropout_p"] = cfg["transformer"]["decoder"]["dropout_p"] = 0.0
        cfg["duration_predictor"]["dropout_p"] = 0.0
    return cfg


def _upstream(shape):
    _, _, batch = _case(shape)
    B, S = batch["phones"].shape
    L, V = batch["tgt_mask"].shape[1], TR.SHAPES[shape][3]
    g = torch.Generator().manual_seed(17)
    return (torch.randn((B, L, V), generator=g, dtype=torch.float64).to(torch.float32),
            torch.randn((B, S), generator=g, dtype=torch.float64).to(torch.float32))


def _masks(shape, offset):
    """The masks of every site as the DEVICE generates them, as CPU tensors."""
    cfg, _, batch = _case(shape)
    B, S = batch["phones"].shape
    L = batch["tgt_mask"].shape[1]
    return [TT.dropout_mask(SEED, offset, site, n, p, DEV).cpu() for site, (n, p) in enumerate(zip(TR.site_sizes(cfg, B, S, L), TR.site_ps(cfg)))]


def _ref(shape, upstream, dropout):
    """(fp64, fp32) results of the restatement, computed once per (shape, upstream, dropout)."""
    key = (shape, upstream, dropout)
    if key not in _refs:
        cfg, sd, batch = _case(shape)
        masks = _masks(shape, 0) if dropout else None
        up = _upstream(shape) if upstream == "random" else None
        _refs[key] = tuple(TR.loss_and_grads(sd, cfg, batch, dt, upstream=up, masks=masks) for dt in (torch.float64, torch.float32))
    return _refs[key]


def _model(shape, dropout=False, sd=None):
    vocab = TR.SHAPES[shape][8]
    m = TT.TrainableParrot(_cfg(shape, not dropout), vocab, 0)
    m.load_state_dict(sd if sd is not None else _case(shape)[1])
    return m.to(DEV)


def _gpu_batch(shape):
    return {k: v.to(DEV) for k, v in _case(shape)[2].items()}


def _bound(ref32, ref64, r=R):
    ref64 = ref64.double()
    yard = float((ref32.double() - ref64).abs().max())
    floor = float(np.spacing(np.float32(ref64.abs().max().item()))) / 2
    return max(r * yard, floor), yard, floor


def _held(name, ours, ref32, ref64, r=R):
    bound, yard, floor = _bound(ref32, ref64, r)
    err = float((ours.detach().cpu().double() - ref64.double()).abs().max())
    ratio = err / yard if yard > 0 else float("inf") if err > 0 else 0.0
    print(f"{name}: err {err:.3e}  yardstick {yard:.3e}  ratio {ratio:.2f}  floor {floor:.3e}")
    assert np.isfinite(err) and err <= bound, (name, err, bound, yard, floor)
    return ratio


def _step(model, shape, upstream):
    """One training forward / backward of ours -> (logits, log_dur, {key -> grad})."""
    batch = _gpu_batch(shape)
    model.zero_grad()
    out, _, _, log_dur = model(batch)
    if upstream == "loss":
        _, gl, gld = ModelLoss(_case(shape)[0]).loss_and_grad(out.detach(), log_dur.detach(), batch)
    else:
        gl, gld = (t.to(DEV) for t in _upstream(shape))
    torch.autograd.backward([out, log_dur], [gl, gld])
    named = dict(model.named_parameters())
    return out.detach(), log_dur.detach(), {k: named[k].grad for k in TR.param_keys(_case(shape)[1])}


def _r_dp(shape):
    """R of log_dur and the duration predictor's gradients: R_DP where the batch has fewer than 8 source rows (T3, T4), R elsewhere."""
    B, S = _case(shape)[2]["phones"].shape
    return R_DP if B * S < 8 else R


def _check_all(shape, upstream, dropout):
    (l64, d64, g64, _), (l32, d32, g32, _) = _ref(shape, upstream, dropout)
    torch.manual_seed(SEED)
    model = _model(shape, dropout).train()
    logits, log_dur, grads = _step(model, shape, upstream)
    assert model._seed == SEED and model._offset == 1
    tag = f"{shape} {upstream} p={'cfg' if dropout else 0}"
    _held(f"{tag} logits", logits, l32, l64)
    _held(f"{tag} log_dur", log_dur, d32, d64, _r_dp(shape))
    assert set(grads) == set(g64) and len(grads) == len(list(model.parameters()))
    for k in g64:
        assert grads[k] is not None and grads[k].shape == g64[k].shape, k
        _held(f"{tag} d {k}", grads[k], g32[k], g64[k], _r_dp(shape) if k.startswith("duration_predictor.") else R)
    assert float(grads["tok_emb.weight"][0].abs().max()) == 0.0  # the padding_idx row, exactly


@pytest.mark.parametrize("upstream", ["loss", "random"])
@pytest.mark.parametrize("shape", ["T1", "T2", "T3", "T4"])
def test_outputs_and_every_gradient_without_dropout(shape, upstream):
    _check_all(shape, upstream, False)


@pytest.mark.parametrize("upstream", ["loss", "random"])
@pytest.mark.parametrize("shape", ["T1", "T2", "T3", "T4"])
def test_outputs_and_every_gradient_with_the_configs_dropout(shape, upstream):
    """p = 0.1 on the attention probabilities, 0.5 in the duration predictor; the reference gets the device's own masks."""
    _check_all(shape, upstream, True)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 70 * 70])
def test_device_mask_equals_the_numpy_restatement(n):
    for site, p, offset in ((0, 0.5, 0), (3, 0.1, 5), (255, 0.1, (1 << 40) + 3)):
        dev = TT.dropout_mask(SEED, offset, site, n, p, DEV).cpu().numpy()
        assert np.array_equal(dev, TR.dropout_mask(SEED, offset, site, n, p)), (site, p, offset)


def test_keep_rate_and_the_two_ends():
    n = 1 << 20
    for p in (0.1, 0.5):
        keep = float(TT.dropout_mask(SEED, 3, 1, n, p, DEV).float().mean())
        assert abs(keep - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / n), (p, keep)
    assert bool(TT.dropout_mask(SEED, 3, 1, 4096, 0.0, DEV).all()) and not bool(TT.dropout_mask(SEED, 3, 1, 4096, 1.0, DEV).any())
    assert not torch.equal(TT.dropout_mask(SEED, 3, 1, 4096, 0.5, DEV), TT.dropout_mask(SEED, 4, 1, 4096, 0.5, DEV))


def test_a_row_does_not_see_the_rows_beside_it_in_training_mode():
    """T2 at p = 0, in training mode: both rows have the batch's padded shape (S = 9; row 0 fills L), so row 0 alone is the same S and L.
    Its logits and log_dur are the batch's bits; and with an upstream gradient that is zero on row 1, every parameter gradient of the
    batch is row 0's alone, bit for bit: the other row contributes exact zeros to every fixed-order sum (products with 0 in the fp32
    chains, zero partials in the fp64 sums), so any data gradient leaking from one row into another would show here.  (Under dropout a
    row's mask depends on its index b in the batch, so only p = 0 can be compared; the dropout kernel's own p = 0 path is held to x's
    bits in tests/test_gpu_tte_train_kernels.py.)"""
    shape = "T2"
    batch = _gpu_batch(shape)
    row0 = {k: v[:1] for k, v in batch.items()}
    gl, gld = (t.to(DEV) for t in _upstream(shape))
    gl, gld = gl.clone(), gld.clone()
    gl[1:], gld[1:] = 0, 0
    res = []
    for b_, g0, g1 in ((batch, gl, gld), (row0, gl[:1], gld[:1])):
        model = _model(shape, False).train()
        out, _, _, log_dur = model(b_)
        assert out.requires_grad
        torch.autograd.backward([out, log_dur], [g0.contiguous(), g1.contiguous()])
        named = dict(model.named_parameters())
        res.append((out.detach(), log_dur.detach(), {k: named[k].grad for k in sorted(named)}))
    (o2, d2, g2), (o1, d1, g1) = res
    assert torch.equal(o2[:1], o1) and torch.equal(d2[:1], d1)
    for k in g1:
        assert torch.equal(g2[k], g1[k]), k


def test_same_seed_and_offset_agree_bit_for_bit():
    shape = "T2"
    runs = []
    for _ in range(2):
        torch.manual_seed(SEED)
        logits, log_dur, grads = _step(_model(shape, True).train(), shape, "random")
        runs.append([logits, log_dur] + [grads[k] for k in sorted(grads)])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    # the next step of the same model draws another mask
    torch.manual_seed(SEED)
    model = _model(shape, True).train()
    first = model(_gpu_batch(shape))[0].detach()
    second = model(_gpu_batch(shape))[0].detach()
    assert model._offset == 2 and not torch.equal(first, second)


@pytest.mark.parametrize("shape", ["T1", "T3"])
def test_eval_mode_against_the_restatement_and_the_inference_parrot(shape):
    cfg, sd, batch = _case(shape)
    with torch.no_grad():
        l64, d64 = TR.forward({k: v.double() for k, v in sd.items()}, cfg, batch)
        l32, d32 = TR.forward(sd, cfg, batch)
    model = _model(shape, True).eval()
    gpu = _gpu_batch(shape)
    out, src_mask, tgt_mask, log_dur = model(gpu)
    assert not out.requires_grad and src_mask is gpu["src_mask"] and tgt_mask is gpu["tgt_mask"] and model._offset == 0
    _held(f"{shape} eval logits", out, l32, l64)
    _held(f"{shape} eval log_dur", log_dur, d32, d64, _r_dp(shape))
    # the inference Parrot on the same state dict: its own bounds are those of tests/test_gpu_teacher_forced.py (1e-4 on the logits
    # of real frames, 2e-5 on log_dur of real tokens); the sum of both bounds
    inf = Parrot(cfg, TR.SHAPES[shape][8], 0)
    inf.load_state_dict(model.state_dict())
    inf = inf.to(DEV).eval()
    o2, _, _, d2 = inf(gpu)
    m, sm = batch["tgt_mask"], batch["src_mask"]
    assert float((out.cpu()[m] - o2.cpu()[m]).abs().max()) <= _bound(l32, l64)[0] + 1e-4
    assert float((log_dur.cpu()[sm] - d2.cpu()[sm]).abs().max()) <= _bound(d32, d64, _r_dp(shape))[0] + 2e-5
    model.load_state_dict(inf.state_dict())  # ... and back


def _ref_loop(cfg, sd, batch, dtype, steps, acc):
    params = {k: v.detach().to(dtype).clone() for k, v in sd.items()}
    keys = TR.param_keys(sd)
    leaves = [params[k].requires_grad_(True) for k in keys]
    optim = torch.optim.AdamW(leaves, lr=1e-3, weight_decay=0.01)
    V = cfg["preprocess"]["hubert_codes"]
    losses = []
    for _ in range(steps):
        optim.zero_grad()
        for _ in range(acc):
            logits, log_dur = TR.forward(params, cfg, batch)
            ld = log_dur.masked_select(batch["src_mask"])
            lt = torch.log(batch["duration"].to(dtype) + 1).masked_select(batch["src_mask"])
            loss = torch.nn.functional.cross_entropy(logits.reshape(-1, V), batch["codes"].reshape(-1), ignore_index=V) \
                + torch.nn.functional.mse_loss(ld, lt)
            (loss / acc).backward()
        torch.nn.utils.clip_grad_norm_(leaves, 1.0)
        optim.step()
        losses.append(float(loss.detach()))
    return losses


def test_trainer_loop_six_adamw_steps():
    """train.py:72-85, 99-103 on T1 at p = 0: AdamW, gradient accumulation 2, clip 1.0, under deterministic algorithms."""
    shape = "T1"
    cfg, sd, batch = _case(shape)
    l64 = _ref_loop(cfg, sd, batch, torch.float64, 6, 2)
    l32 = _ref_loop(cfg, sd, batch, torch.float32, 6, 2)
    print("fp64 losses", l64)
    model = _model(shape, False).train()
    optim = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=0.01)
    criterion = ModelLoss(cfg)
    gpu = _gpu_batch(shape)
    ours = []
    torch.use_deterministic_algorithms(True)
    try:
        for _ in range(6):
            optim.zero_grad()
            for _ in range(2):
                out, _, _, log_dur = model(gpu)
                loss, _, _ = criterion(out, log_dur, gpu)
                (loss / 2).backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
            optim.step()
            ours.append(float(loss.detach()))
    finally:
        torch.use_deterministic_algorithms(False)
    print("our losses", ours)
    assert ours[-1] < ours[0] and l64[-1] < l64[0]
    yard_vec = max(abs(a - b) for a, b in zip(l32, l64))
    for i in range(6):
        ulp = float(np.spacing(np.float32(l64[i])))
        yard = abs(l32[i] - l64[i])
        bound = min(R * yard_vec, max(R * yard, LOSS_FLOOR_ULPS * ulp))
        err = abs(ours[i] - l64[i])
        print(f"step {i}: err {err:.3e} ({err / ulp:.2f} ulp)  own yardstick {yard:.3e}  vector yardstick {yard_vec:.3e}  bound {bound:.3e}")
        assert err <= bound, (i, ours[i], l64[i], l32[i])


def test_error_paths_leave_the_module_usable():
    shape = "T3"
    cfg, sd, batch = _case(shape)
    model = _model(shape, False).train()
    gpu = _gpu_batch(shape)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        model(dict(gpu, phones=batch["phones"]))
    with pytest.raises(IndexError):
        model(dict(gpu, phones=torch.full_like(gpu["phones"], TR.SHAPES[shape][8])))
    with pytest.raises(AssertionError):
        model(dict(gpu, tgt_mask=torch.ones((1, 4), dtype=torch.bool, device=DEV)))
    max_len = cfg["transformer"]["max_len"]
    long = dict(gpu, duration=torch.tensor([[max_len, 0, 0]], device=DEV), tgt_mask=torch.ones((1, max_len), dtype=torch.bool, device=DEV))
    with pytest.raises(IndexError, match="out of bounds"):
        model(long)
    out, _, _, log_dur = model(gpu)
    (out.sum() + log_dur.sum()).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    frozen = _model(shape, False).train()
    frozen.get_parameter("head.weight").requires_grad_(False)
    out, _, _, log_dur = frozen(gpu)
    out.sum().backward()
    assert frozen.get_parameter("head.weight").grad is None and frozen.get_parameter("head.bias").grad is not None


def test_whole_file_under_poison():
    """This file once more in a child process under PARROT_POISON_WS=nan: a kernel reading a byte nobody wrote would turn a logit,
    a gradient or a loss into NaN there."""
    if os.environ.get("PARROT_POISON_WS"):
        return  # (already a poisoned run: the tests above were it)
    env = dict(os.environ, PARROT_POISON_WS="nan")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", os.path.abspath(__file__), "-k", "not whole_file"], cwd=ROOT,
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


def test_lit_parrot_training_step(tmp_path):
    """LitParrot(trainable=True).training_step logs the three losses and returns a loss with a graph; its state dict loads into
    LitParrot()."""
    from parrot_tts_amd.checkpoint import LitParrot
    shape = "T1"
    cfg, sd, _ = _case(shape)
    vocab = TR.SHAPES[shape][8]
    lit = LitParrot(cfg, vocab, 0, trainable=True)
    assert isinstance(lit.parrot, TT.TrainableParrot)
    lit.parrot.load_state_dict(sd)
    lit = lit.to(DEV).train()
    loss = lit.training_step(_gpu_batch(shape), 0)
    assert loss.requires_grad and set(lit.logged) == {"train_total_loss", "train_code_loss", "train_dur_loss"}
    loss.backward()
    assert all(p.grad is not None for p in lit.parrot.parameters())
    plain = LitParrot(cfg, vocab, 0)
    plain.load_state_dict(lit.state_dict())
    assert set(plain.state_dict()) == set(lit.state_dict())
    val = lit.eval().validation_step(_gpu_batch(shape), 0)
    assert not val.requires_grad and bool(torch.isfinite(val))
