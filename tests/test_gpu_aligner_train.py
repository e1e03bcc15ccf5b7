"""GPU: training the forced aligner on the device (parrot_tts_amd/aligner_train.py over parrot_aligner_train_forward /
parrot_aligner_train_backward).

The yardstick of every compared tensor is the reference's OWN fp32 error: the restatement (tests/aligner_train_ref.py) run on the
CPU in fp32 against its fp64 run on the same inputs, both errors max-abs over the tensor.  Ours against fp64 must be within
R x that, with a floor of what is rounded once anyway: half an fp32 ulp of the tensor's largest magnitude (logits, gradients,
buffers), one fp32 ulp of the loss (the trainer loop).  R = 8: twice the largest ratio measured on S1, S2 and S4 (2.49, DESIGN.md
section 4 has the table; 2.53 on S5 is the largest seen anywhere), rounded up to a power of two; it may not exceed 8, so there is no
room left.  In the trainer loop the rule is applied with the six losses as the compared tensor (R x the largest of the six fp32
errors), and on top of it each loss is held to R x its OWN fp32 error, with a floor of LOSS_FLOOR_ULPS = 4 ulps of that loss
(derived below from what is rounded once anyway): the smaller of the two bounds counts.  The floor is wider
than one ulp because a single loss's own fp32 error is a scalar that vanishes by chance, and differently on different hosts: at
step 2 it was 1.7e-8 (0.02 ulp) on one host and 9.4e-7 on another, where ours is 1.9e-6 = 2.0 ulps of 15.25 on both.

The whole file also passes under PARROT_POISON_WS=nan (workspace, saved buffer, logits and every gradient filled with NaN at the
top of both entry points)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import aligner_ref as R0  # noqa: E402
import aligner_train_ref as TR  # noqa: E402
from parrot_tts_amd import aligner as A  # noqa: E402

DEV = "cuda:0"
R = 8.0
# Floor of one loss of the trainer loop, in fp32 ulps of that loss -- what is rounded once anyway, on S1's batch:
#   1    the loss itself, rounded to fp32 once;
#   1.1  the logits, rounded to fp32 once: |d nll_b / d logits[t]|_1 <= 2 per frame, so |d loss| <= mean_b(2 T_b / N_b) x half an ulp of
#        the largest logit = 2 x 8.86 x 6.0e-8 = 1.06e-6 (T_b = 25, 37, 37; N_b = 5, 4, 3; |logit| < 2), against ulp(loss) = 9.5e-7;
#   1.1  from the second step on, every parameter as Adam stored it in fp32, which moves the logits by about their own rounding again.
# 3.2, rounded up to 4.
LOSS_FLOOR_ULPS = 4
_cases, _refs = {}, {}


def _case(shape):
    if shape not in _cases:
        _cases[shape] = TR.make_case(shape)
    return _cases[shape]


def _random_upstream(shape):
    B, T, _, V = TR.SHAPES[shape][:4]
    g = torch.Generator().manual_seed(17)
    return torch.randn((B, T, V), generator=g, dtype=torch.float64).to(torch.float32)


def _ref(shape, upstream):
    """(fp64, fp32) results of the restatement for one shape and upstream gradient ("ctc" / "random"), computed once."""
    key = (shape, upstream)
    if key not in _refs:
        sd, mel, tokens, ml, tl = _case(shape)
        g = _random_upstream(shape) if upstream == "random" else None
        _refs[key] = tuple(TR.loss_and_grads(sd, mel, tokens, ml, tl, dt, grad_logits=g) for dt in (torch.float64, torch.float32))
    return _refs[key]


def _model(shape, sd=None):
    B, T, n_mels, V, H, D, N = TR.SHAPES[shape]
    m = A.TrainableAligner(n_mels, V, H, D)
    m.load_state_dict(sd if sd is not None else _case(shape)[0])
    return m.to(DEV)


def _bound(ref32, ref64, r=R):
    ref64 = ref64.double()
    yard = float((ref32.double() - ref64).abs().max())
    floor = float(np.spacing(np.float32(ref64.abs().max().item()))) / 2
    return max(r * yard, floor), yard, floor


def _held(name, ours, ref32, ref64, r=R):
    """Print the figures, then hold ``ours`` to the rule above.  Returns ours / yardstick."""
    bound, yard, floor = _bound(ref32, ref64, r)
    err = float((ours.detach().cpu().double() - ref64.double()).abs().max())
    ratio = err / yard if yard > 0 else float("inf") if err > 0 else 0.0
    print(f"{name}: err {err:.3e}  yardstick {yard:.3e}  ratio {ratio:.2f}  floor {floor:.3e}")
    assert np.isfinite(err) and err <= bound, (name, err, bound, yard, floor)
    return ratio


def _step(model, shape, upstream):
    """One forward / backward of ours -> (logits, {param key -> grad})."""
    sd, mel, tokens, ml, tl = _case(shape)
    model.zero_grad()
    logits = model(mel.to(DEV))
    if upstream == "ctc":
        _, g = A.ctc_loss_and_grad(logits.detach(), tokens.to(DEV), ml, tl)
    else:
        g = _random_upstream(shape).to(DEV)
    logits.backward(g)
    named = dict(model.named_parameters())
    return logits.detach(), {k: named[k].grad for k in TR.PARAM_KEYS}


@pytest.mark.parametrize("shape", ["S1", "S2", "S4"])
def test_train_mode_logits(shape):
    (l64, _, _, _), (l32, _, _, _) = _ref(shape, "ctc")
    model = _model(shape).train()
    logits = model(_case(shape)[1].to(DEV))
    assert logits.requires_grad and logits.shape == l64.shape
    _held(f"{shape} logits", logits, l32, l64)


@pytest.mark.parametrize("upstream", ["ctc", "random"])
@pytest.mark.parametrize("shape", ["S1", "S2", "S4"])
def test_all_19_gradients(shape, upstream):
    (_, _, g64, _), (_, _, g32, _) = _ref(shape, upstream)
    model = _model(shape).train()
    _, grads = _step(model, shape, upstream)
    assert len(grads) == 19
    for k in TR.PARAM_KEYS:
        assert grads[k] is not None and grads[k].shape == g64[k].shape, k
        _held(f"{shape} {upstream} d {k}", grads[k], g32[k], g64[k])
    for sfx in ("", "_reverse"):
        assert torch.equal(grads["rnn.bias_ih_l0" + sfx], grads["rnn.bias_hh_l0" + sfx])


def test_more_rows_than_one_batch_pass_of_the_lstm_kernels():
    """S5, B = 17: both LSTM step kernels take 16 batch rows per pass; the 17th is a second pass of one row."""
    shape = "S5"
    (l64, _, g64, _), (l32, _, g32, _) = _ref(shape, "random")
    logits, grads = _step(_model(shape).train(), shape, "random")
    _held("S5 logits", logits, l32, l64)
    for k in TR.PARAM_KEYS:
        _held(f"S5 random d {k}", grads[k], g32[k], g64[k])


@pytest.mark.parametrize("shape, upstream", [("S6", "ctc"), ("S6", "random"), ("S7", "ctc"), ("S7", "random"), ("S8", "random")])
def test_shapes_that_reach_the_second_trips_and_tile_edges(shape, upstream):
    """S6: lstm_dim 144 and conv_dim 112 -- three trips of both LSTM k-loops with a partial last one, two block rows and a partial K
    pass in every conv; S7: T = 130 and V = 70 -- three column blocks, a reduction chunk ending inside a batch row, a second block
    of the Linear; S8: T = 1.  Logits and all 19 gradients under the rule of this file as it stands (the kernels on their own:
    tests/test_gpu_aligner_train_kernels.py)."""
    (l64, _, g64, _), (l32, _, g32, _) = _ref(shape, upstream)
    logits, grads = _step(_model(shape).train(), shape, upstream)
    assert logits.shape == l64.shape and len(grads) == 19
    ratios = {"logits": _held(f"{shape} logits", logits, l32, l64)}
    for k in TR.PARAM_KEYS:
        assert grads[k] is not None and grads[k].shape == g64[k].shape, k
        ratios[k] = _held(f"{shape} {upstream} d {k}", grads[k], g32[k], g64[k])
    worst = max(ratios, key=ratios.get)
    print(f"{shape} {upstream}: largest ratio {ratios[worst]:.2f} ({worst})")


def test_buffers_after_one_and_three_forwards():
    shape = "S1"
    sd, mel, tokens, ml, tl = _case(shape)
    model = _model(shape).train()
    P = {dt: {k: v.to(dt) for k, v in sd.items() if v.dim() > 0} for dt in (torch.float64, torch.float32)}
    x = mel.to(DEV)
    for n in (1, 2, 3):
        model(x)
        for dt in P:
            P[dt].update(TR.forward(P[dt], mel.to(dt), True)[1])
        if n == 2:
            continue
        got = model.state_dict()
        for k in TR.BUFFER_KEYS:
            _held(f"after {n}: {k}", got[k], P[torch.float32][k], P[torch.float64][k])
        for i in range(3):
            assert int(got[f"convs.{i}.bnorm.num_batches_tracked"]) == int(sd[f"convs.{i}.bnorm.num_batches_tracked"]) + n
        assert model.get_step() == int(sd["step"]) + n


@pytest.mark.parametrize("shape", ["S1", "S2"])
def test_eval_mode_agrees_with_the_inference_aligner(shape):
    sd, mel, *_ = _case(shape)
    B, T, n_mels, V, H, D, N = TR.SHAPES[shape]
    l64 = R0.aligner_forward(sd, mel.double())[0]
    l32 = R0.aligner_forward(sd, mel)[0]
    model = _model(shape).eval()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    logits = model(mel.to(DEV))
    assert not logits.requires_grad
    _held(f"{shape} eval logits", logits, l32, l64)
    inf = A.Aligner(n_mels, V, H, D, precision="f32")
    inf.load_state_dict(sd)
    theirs = inf.to(DEV)(mel.to(DEV))
    bound, yard, _ = _bound(l32, l64)
    gap = float((logits - theirs).abs().max())
    print(f"{shape} eval logits, ours - Aligner(f32): {gap:.3e}  yardstick {yard:.3e}  ratio {gap / yard:.2f}")
    assert gap <= bound  # (the bound of the train-mode logits, as it stands)
    after = model.state_dict()
    for k, v in before.items():
        if k == "step":
            assert int(after[k]) == int(v) + 1
        else:
            assert torch.equal(after[k], v), k
    model.train()
    with torch.no_grad():  # no_grad in train mode: the running statistics, no graph
        again = model(mel.to(DEV))
    assert not again.requires_grad and torch.equal(again, logits)


def test_two_runs_agree_bit_for_bit_and_an_in_place_update_is_seen():
    shape = "S2"
    sd, mel, tokens, ml, tl = _case(shape)
    runs = []
    for _ in range(2):
        model = _model(shape).train()
        logits, grads = _step(model, shape, "random")
        runs.append((logits, grads, {k: v.clone() for k, v in model.state_dict().items()}))
    assert torch.equal(runs[0][0], runs[1][0])
    for k in TR.PARAM_KEYS:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k
    # a parameter changed in place on the device is read by the next forward: nothing is cached
    model = _model(shape).train()
    model(mel.to(DEV))
    sd2 = {k: v.clone() for k, v in model.state_dict().items()}
    gen = torch.Generator().manual_seed(5)
    for k in TR.PARAM_KEYS:
        delta = 0.05 * torch.randn(sd2[k].shape, generator=gen)
        dict(model.named_parameters())[k].data.add_(delta.to(DEV))
        sd2[k] = sd2[k].cpu() + delta  # (the same fp32 addition)
    sd2 = {k: v.cpu() for k, v in sd2.items()}
    logits = model(mel.to(DEV))
    l64 = TR.forward({k: v.double() for k, v in sd2.items() if v.dim() > 0}, mel.double(), True)[0]
    l32 = TR.forward({k: v for k, v in sd2.items() if v.dim() > 0}, mel, True)[0]
    _held("S2 logits on the changed weights", logits, l32, l64)
    assert float((logits.detach().cpu() - runs[0][0].cpu()).abs().max()) > 100 * _bound(l32, l64)[0]


def _ref_loop(sd, mel, tokens, ml, tl, dtype, steps):
    P = TR.leaf_params(sd, dtype)
    params = [P[k] for k in TR.PARAM_KEYS]
    optim = torch.optim.Adam(params, lr=1e-3)
    losses = []
    for _ in range(steps):
        logits, bufs = TR.forward(P, mel.to(dtype), True)
        loss = TR.ctc(logits, tokens, ml, tl)
        optim.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        optim.step()
        P.update(bufs)
        losses.append(float(loss.detach()))
    return losses


def test_reference_trainer_loop_six_steps():
    shape = "S1"
    sd, mel, tokens, ml, tl = _case(shape)
    l64 = _ref_loop(sd, mel, tokens, ml, tl, torch.float64, 6)
    l32 = _ref_loop(sd, mel, tokens, ml, tl, torch.float32, 6)
    print("fp64 losses", l64)
    assert all(b < a for a, b in zip(l64, l64[1:])), l64
    model = _model(shape).train()
    optim = torch.optim.Adam(model.parameters(), lr=1e-3)
    ctc_loss = A.CTCLoss()
    x, tk, mlen, tlen = mel.to(DEV), tokens.to(DEV), ml.to(DEV), tl.to(DEV)
    ours = []
    torch.use_deterministic_algorithms(True)
    try:
        for _ in range(6):  # trainer.py:60-71, unchanged
            pred = model(x)
            pred = pred.transpose(0, 1).log_softmax(2)
            loss = ctc_loss(pred, tk, mlen, tlen)
            if not torch.isnan(loss) and not torch.isinf(loss):
                optim.zero_grad()
                loss.backward()
                torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
                optim.step()
            ours.append(float(loss.detach()))
    finally:
        torch.use_deterministic_algorithms(False)
    print("our losses", ours)
    assert all(b < a for a, b in zip(ours, ours[1:])), ours
    yard_vec = max(abs(a - b) for a, b in zip(l32, l64))  # (max-abs over the six losses taken as one tensor)
    for i in range(6):
        ulp = float(np.spacing(np.float32(l64[i])))
        yard = abs(l32[i] - l64[i])  # this loss's own fp32 error: a scalar, on some hosts a small fraction of an ulp by chance
        bound = min(R * yard_vec, max(R * yard, LOSS_FLOOR_ULPS * ulp))
        err = abs(ours[i] - l64[i])
        print(f"step {i}: err {err:.3e} ({err / ulp:.2f} ulp)  own yardstick {yard:.3e} ({yard / ulp:.2f} ulp)  vector yardstick {yard_vec:.3e}"
              f"  bound {bound:.3e}")
        assert err <= bound, (i, ours[i], l64[i], l32[i])
    assert model.get_step() == int(sd["step"]) + 6


def test_smallest_batch_and_its_error():
    shape = "S3"
    (l64, _, g64, _), (l32, _, g32, _) = _ref(shape, "ctc")
    model = _model(shape).train()
    logits, grads = _step(model, shape, "ctc")
    _held("S3 logits", logits, l32, l64)
    for k in TR.PARAM_KEYS:
        _held(f"S3 d {k}", grads[k], g32[k], g64[k])
    n_mels = TR.SHAPES[shape][2]
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        model(torch.zeros((1, 1, n_mels), device=DEV))
    model.eval()
    assert model(torch.zeros((1, 1, n_mels), device=DEV)).shape == (1, 1, TR.SHAPES[shape][3])  # (eval has no such limit)


def test_frozen_parameter_mel_gradient_nan_and_bad_shapes():
    shape = "S1"
    sd, mel, tokens, ml, tl = _case(shape)
    model = _model(shape).train()
    _, full = _step(model, shape, "random")
    frozen = _model(shape).train()
    named = dict(frozen.named_parameters())
    for k in ("convs.1.conv.weight", "rnn.bias_hh_l0", "lin.weight"):
        named[k].requires_grad_(False)
    x = mel.to(DEV).requires_grad_(True)
    logits = frozen(x)
    logits.backward(_random_upstream(shape).to(DEV))
    assert x.grad is None
    for k in TR.PARAM_KEYS:
        if named[k].requires_grad:
            assert torch.equal(named[k].grad, full[k]), k
        else:
            assert named[k].grad is None, k
    bad = mel.clone()
    bad[1, 7, 3] = float("nan")
    out = model(bad.to(DEV))  # the batch statistics spread it to every logit, and nothing is raised
    assert bool(torch.isnan(out).all())
    with pytest.raises(ValueError):
        model(torch.zeros((2, 9, TR.SHAPES[shape][2] + 1), device=DEV))
    with pytest.raises(RuntimeError, match="GPU"):
        model(mel)


def test_driver_end_to_end(tmp_path, capsys):
    """Twelve synthetic items, four steps from scratch: the driver writes latest_model.pt with the reference's keys, and both the
    inference ``Aligner`` and the align_durations driver (a fresh process) read it."""
    import json
    import pickle

    import yaml
    from parrot_tts_amd import synth
    from parrot_tts_amd.cli import aligner_train as CLI
    cfg = synth.small_aligner_config(str(tmp_path / "data"))
    cfg["training"] = {"learning_rate": 1e-3, "epochs": 2, "batch_size": 3, "checkpoint_steps": 3, "plot_steps": 1000}
    symbols = [chr(ord("a") + i) for i in range(12)]
    V = len(symbols) + 1
    data = tmp_path / "data"
    for d in ("mels", "tokens"):
        (data / d).mkdir(parents=True, exist_ok=True)
    rng = np.random.Generator(np.random.PCG64(6))
    dataset = []
    for i in range(12):
        T, N = int(rng.integers(20, 48)), int(rng.integers(3, 9))
        item = f"utt{i:02d}"
        np.save(data / "mels" / f"{item}.npy", synth.synth_aligner_mel(1, T, 16, seed=40 + i)[0].numpy(), allow_pickle=False)
        np.save(data / "tokens" / f"{item}.npy", rng.integers(1, V, size=N), allow_pickle=False)
        dataset.append({"item_id": item, "mel_len": T, "tokens_len": N})
    with open(data / "dataset.pkl", "wb") as f:
        pickle.dump(dataset, f)
    with open(data / "symbols.pkl", "wb") as f:
        pickle.dump(symbols, f)
    with open(tmp_path / "config.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    torch.manual_seed(11)
    CLI.main(["--config", str(tmp_path / "config.yaml"), "--max_steps", "4"])
    lines = [json.loads(s) for s in capsys.readouterr().out.strip().splitlines()]
    assert len(lines) == 1 and sorted(lines[0]) == ["epoch", "mean_loss", "n_skipped", "step"]
    assert lines[0]["epoch"] == 1 and lines[0]["step"] == 5 and lines[0]["n_skipped"] == 0 and np.isfinite(lines[0]["mean_loss"])
    assert sorted(os.listdir(data / "checkpoints")) == ["latest_model.pt", "model_step_0k.pt"]  # (step 3 of checkpoint_steps 3)
    ck = torch.load(data / "checkpoints" / "latest_model.pt", map_location="cpu", weights_only=False)
    assert sorted(ck) == ["config", "model", "optim", "symbols"] and ck["symbols"] == symbols
    model = A.Aligner.from_checkpoint(ck)
    assert model.get_step() == 5 and int(ck["model"]["convs.0.bnorm.num_batches_tracked"]) == 4
    CLI.main(["--config", str(tmp_path / "config.yaml"), "--max_steps", "1"])  # resumes from latest_model.pt
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["step"] == 6
    r = subprocess.run([sys.executable, "-m", "parrot_tts_amd.cli.align_durations", "--config", str(tmp_path / "config.yaml"), "--batch_size", "4"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["n_items"] == 12 and out["n_written"] == 12 and out["n_failed"] == 0 and out["step"] > 6
    os.remove(data / "mels" / "utt07.npy")  # an unreadable item ends the run: the corpus never shrinks silently
    with pytest.raises(RuntimeError, match="could not be loaded"):
        CLI.main(["--config", str(tmp_path / "config.yaml"), "--max_steps", "4"])


def test_whole_file_under_poison():
    """This file once more in a child process under PARROT_POISON_WS=nan: a kernel reading a byte nobody wrote would turn a logit,
    a gradient or a loss into NaN there."""
    if os.environ.get("PARROT_POISON_WS"):
        return  # (already a poisoned run: the tests above were it)
    env = dict(os.environ, PARROT_POISON_WS="nan")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", os.path.abspath(__file__), "-k", "not whole_file"], cwd=ROOT,
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
