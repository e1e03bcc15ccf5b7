"""GPU: training the vocoder's generator on the device (parrot_tts_amd/vocoder_train.py over parrot_voc_train_forward /
parrot_voc_train_backward).

The rule is that of tests/test_gpu_tte_train.py: the restatement (tests/voc_train_ref.py) run on the CPU in fp32 against its fp64 run
on the same inputs and the SAME device masks is the yardstick, both errors max-abs over the tensor; ours against fp64 must be within
R x that, with a floor of what is rounded once anyway, half an fp32 ulp of the tensor's largest magnitude.
  R = 8          tensors of 8 or more elements;
  R_SMALL = 256  tensors of fewer than 8 elements (conv_post.bias, conv_post.weight_g, the biases and gains of 2- and 4-channel
                 layers): on so few values the yardstick is a matter of chance.
These are the project's R and R_DP; DESIGN.md (section 3, "Vocoder generator training") has the table of the measured ratios: the
largest are 4.26 for a tensor of 8 or more elements (d resblocks.13.convs1.2.bias, V5) and 9.86 below (d resblocks.14.convs.0.bias, V4).
Masks: for every site the device mask equals x64 > 0 wherever |x64| > 8 e_site (e_site: the restatement's own fp32-vs-fp64 max error
on that site's input, from a single-threaded fp32 run: voc_train_ref.own_inputs); what lies inside that band is left out under the
caps of voc_train_ref.check_caps.

Trainer loop: four AdamW steps on V1 against an mse target; each loss is held to R x the restatement's own fp32 error with the floor
derived at _loss_floor below.

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

import voc_train_ref as VR  # noqa: E402
from parrot_tts_amd import vocoder_train as VT  # noqa: E402
from parrot_tts_amd.vocoder import CodeGenerator  # noqa: E402

DEV = "cuda:0"
R = 8.0
R_SMALL = 256.0
_cases, _runs, _refs = {}, {}, {}


def _case(name):
    if name not in _cases:
        _cases[name] = VR.make_case(name)
    return _cases[name]


def _model(name, sd=None, h=None):
    m = VT.TrainableCodeGenerator(h or _case(name)[0])
    m.load_state_dict(sd if sd is not None else _case(name)[1])
    return m.to(DEV)


def _gpu_batch(name):
    return {k: v.to(DEV) for k, v in _case(name)[2].items()}


def _upstream(name, kind):
    """"random": a seeded randn gradient at the waveform; "mse": ("mse", a seeded target)."""
    h, _, batch = _case(name)
    B, U = batch["code"].shape
    T = VT.TrainableCodeGenerator(h).out_samples(int(U))
    g = torch.Generator().manual_seed(17)
    t = torch.randn((B, 1, T), generator=g, dtype=torch.float64).to(torch.float32)
    return t if kind == "random" else ("mse", 0.3 * t)


def _step(model, name, kind, batch=None):
    """One training forward / backward of ours -> (wav, {key -> grad}, masks)."""
    model.zero_grad()
    wav = model(**(batch or _gpu_batch(name)))
    up = _upstream(name, kind)
    if kind == "mse":
        torch.nn.functional.mse_loss(wav, up[1].to(DEV)).backward()
    else:
        wav.backward(up.to(DEV))
    named = dict(model.named_parameters())
    return wav.detach(), {k: p.grad for k, p in named.items()}, model.lrelu_masks()


def _ours(name, kind):
    if (name, kind) not in _runs:
        _runs[(name, kind)] = _step(_model(name).train(), name, kind)
    return _runs[(name, kind)]


def _ref(name, kind):
    """(fp64, fp32) results of the restatement under the device's masks, computed once per (case, upstream)."""
    if (name, kind) not in _refs:
        h, sd, batch = _case(name)
        masks = [m.cpu() for m in _ours(name, kind)[2]]
        _refs[(name, kind)] = tuple(VR.loss_and_grads(sd, h, batch, dt, _upstream(name, kind), masks) for dt in (torch.float64, torch.float32))
    return _refs[(name, kind)]


def _bound(ref32, ref64, r):
    ref64 = ref64.double()
    yard = float((ref32.double() - ref64).abs().max())
    floor = float(np.spacing(np.float32(ref64.abs().max().item()))) / 2
    return max(r * yard, floor), yard, floor


def _held(name, ours, ref32, ref64, r=None):
    r = (R if ref64.numel() >= 8 else R_SMALL) if r is None else r
    bound, yard, floor = _bound(ref32, ref64, r)
    err = float((ours.detach().cpu().double() - ref64.double()).abs().max())
    ratio = err / yard if yard > 0 else float("inf") if err > 0 else 0.0
    print(f"{name}: n {ref64.numel()}  err {err:.3e}  yardstick {yard:.3e}  ratio {ratio:.2f}  floor {floor:.3e}  R {r:g}")
    ok = np.isfinite(err) and err <= bound
    return ok, (name, err, bound, yard, floor)


def _check_all(name, kind):
    (w64, g64, _, _), (w32, g32, _, _) = _ref(name, kind)
    wav, grads, _ = _ours(name, kind)
    tag = f"{name} {kind}"
    res = [_held(f"{tag} wav", wav, w32, w64)]
    assert set(grads) == set(g64)
    for k in g64:
        assert grads[k] is not None and grads[k].shape == g64[k].shape, k
        res.append(_held(f"{tag} d {k}", grads[k], g32[k], g64[k]))
    bad = [r[1] for r in res if not r[0]]
    assert not bad, bad


@pytest.mark.parametrize("name,kind", [(n, "random") for n in VR.CASES] + [("V1", "mse")])
def test_waveform_and_every_gradient(name, kind):
    _check_all(name, kind)


@pytest.mark.parametrize("name", VR.CASES)
def test_device_masks_are_the_fp64_signs_outside_the_band(name):
    """x64 and e_site are the restatement's own (VR.own_inputs: its fp64 run and its single-threaded fp32 run, each under its own
    signs, with no device value in them): the quantities tests/test_voc_train_cpu.py holds to the caps."""
    in64, in32 = VR.own_inputs(name)
    masks = _ours(name, "random")[2]
    h = _case(name)[0]
    assert len(masks) == VR.n_sites(h) == len(in64)
    for m, x in zip(masks, in64):
        assert m.shape == x.shape and m.dtype == torch.bool
    counts = VR.excluded(in64, in32, masks)
    print(f"{name}: sites {len(counts)}  elements {sum(c[1] for c in counts)}  inside the band {sum(c[0] for c in counts)}  "
          f"worst site {max(counts, key=lambda c: c[0] / c[1])[:2]}  mismatches outside the band {sum(c[2] for c in counts)}")
    share, worst = VR.check_caps(counts)
    print(f"{name}: excluded share {share:.2e}  worst site share {worst:.2e}")


def test_two_runs_agree_bit_for_bit_also_under_deterministic_algorithms():
    name = "V2"
    a = _ours(name, "random")
    torch.use_deterministic_algorithms(True)
    try:
        b = _step(_model(name).train(), name, "random")
    finally:
        torch.use_deterministic_algorithms(False)
    assert torch.equal(a[0], b[0])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
    assert all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


def test_a_row_does_not_see_the_rows_beside_it():
    name = "V2"
    wav = _ours(name, "random")[0]
    batch = _gpu_batch(name)
    model = _model(name).train()
    for b in range(wav.shape[0]):
        row = model(**{k: v[b:b + 1] for k, v in batch.items()})
        assert torch.equal(row.detach(), wav[b:b + 1]), b


@pytest.mark.parametrize("name", ["V1", "V5"])
def test_eval_and_no_grad_are_the_training_forward_and_agree_with_the_inference_generator(name):
    h, sd, batch = _case(name)
    wav = _ours(name, "random")[0]
    model = _model(name)
    gpu = _gpu_batch(name)
    out = model.eval()(**gpu)
    assert not out.requires_grad and torch.equal(out, wav)
    with torch.no_grad():
        assert torch.equal(model.train()(**gpu), wav)
    (w64, _, _, _), (w32, _, _, _) = _ref(name, "random")
    # the inference generator with exact-fp32 products, on the same state dict (and back): the same rule
    inf = CodeGenerator(h)
    inf.load_state_dict(model.state_dict())
    inf._precision_override = 0  # PARROT_PREC_F32
    inf = inf.to(DEV).eval()
    ok, info = _held(f"{name} inference generator (f32)", inf(**gpu), w32, w64)
    assert ok, info
    model.load_state_dict(inf.state_dict())
    assert torch.equal(model.eval()(**gpu), wav)


def test_remove_weight_norm_keeps_working_and_training():
    name = "V3"
    h, sd, batch = _case(name)
    model = _model(name).train()
    model.remove_weight_norm()
    keys = set(model.state_dict())
    assert not [k for k in keys if k.endswith("weight_g") or k.endswith("weight_v")] and "conv_pre.weight" in keys
    wav, grads, masks = _step(model, name, "random")
    plain = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    up = _upstream(name, "random")
    (w64, g64, _, _), (w32, g32, _, _) = (VR.loss_and_grads(plain, h, batch, dt, up, [m.cpu() for m in masks]) for dt in (torch.float64, torch.float32))
    res = [_held(f"{name} folded wav", wav, w32, w64)] + [_held(f"{name} folded d {k}", grads[k], g32[k], g64[k]) for k in g64]
    bad = [r[1] for r in res if not r[0]]
    assert not bad, bad
    # the fold itself against the fp64 fold rounded once: the norm, the quotient and the product are each rounded once (2^-24 relative
    # each) and so is the reference: 4 x 2^-24 |w| <= 4 ulps of the tensor's largest weight
    want = VR.folded(sd)
    for k, v in want.items():
        assert float((plain[k].double() - v.double()).abs().max()) <= 4 * float(np.spacing(np.float32(v.abs().max().item()))), k
    # a plain-weight state dict loads into a fresh module, which then holds no g
    fresh = VT.TrainableCodeGenerator(h)
    fresh.load_state_dict(plain)
    assert torch.equal(fresh.to(DEV).eval()(**_gpu_batch(name)), wav)
    with pytest.raises(ValueError):
        model.remove_weight_norm()


def test_a_frozen_parameter_gets_no_gradient_and_the_others_are_unchanged():
    name = "V4"
    _, grads, _ = _ours(name, "random")
    model = _model(name).train()
    frozen = ("ups.1.weight_v", "conv_post.weight_g", "resblocks.2.convs.1.bias", "dict.weight")
    for k in frozen:
        model.get_parameter(k).requires_grad_(False)
    _, g2, _ = _step(model, name, "random")
    for k in grads:
        if k in frozen:
            assert g2[k] is None, k
        else:
            assert torch.equal(g2[k], grads[k]), k


# Floor of one loss of the trainer loop, absolute.  loss = mean((wav - target)^2) over n samples.  What is rounded once anyway:
#   the loss itself: one ulp of it;
#   the waveform, rounded to fp32 once: |d loss / d wav[i]| = 2 |wav[i] - target[i]| / n, and |wav| < 1 so a sample moves by at most
#   half an ulp of 1 (2^-24): |d loss| <= 2 mean|wav - target| 2^-24;
#   from the second step on every parameter as AdamW stored it in fp32, which moves the waveform by about its own rounding again.
def _loss_floor(loss64, mean_abs_diff, step):
    return float(np.spacing(np.float32(loss64))) + (2 if step else 1) * 2 * mean_abs_diff * 2.0 ** -24


def test_four_adamw_steps_against_the_restatement():
    name, steps = "V1", 4
    h, sd, batch = _case(name)
    target = _upstream(name, "mse")[1]
    model = _model(name).train()
    optim = torch.optim.AdamW(model.parameters(), lr=2e-4, betas=(0.8, 0.99))
    gpu = _gpu_batch(name)
    ours, all_masks = [], []
    for _ in range(steps):
        optim.zero_grad()
        loss = torch.nn.functional.mse_loss(model(**gpu), target.to(DEV))
        loss.backward()
        all_masks.append([m.cpu() for m in model.lrelu_masks()])
        optim.step()
        ours.append(float(loss.detach()))
    final = {k: v.detach().cpu() for k, v in model.state_dict().items()}

    def loop(dtype):
        params = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
        opt = torch.optim.AdamW(list(params.values()), lr=2e-4, betas=(0.8, 0.99))
        losses, diffs = [], []
        for i in range(steps):
            opt.zero_grad()
            wav, _ = VR.forward(params, h, batch, all_masks[i])
            loss = torch.nn.functional.mse_loss(wav, target.to(dtype))
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
            diffs.append(float((wav.detach() - target.to(dtype)).abs().mean()))
        return losses, diffs, {k: v.detach() for k, v in params.items()}

    l64, d64, p64 = loop(torch.float64)
    l32, _, p32 = loop(torch.float32)
    # The final parameters take the larger of the restatement's fp32 errors on one thread and on the machine's threads.  AdamW divides
    # by sqrt(v): where a gradient is as small as its own rounding error the update is lr x noise, and the restatement's fp32 run
    # then moves with its summation order: on resblocks.4.convs2.2.weight_v two fp32 evaluations of the restatement (1 thread, 16
    # threads, the same masks) end 1.44e-5 and 1.3e-6 from fp64 and 1.3e-5 from each other, measured on the CPU alone.
    keep = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        _, _, p32_one = loop(torch.float32)
    finally:
        torch.set_num_threads(keep)
    p32 = {k: max((p32[k], p32_one[k]), key=lambda t: float((t.double() - p64[k]).abs().max())) for k in p64}
    print("fp64 losses", l64, "ours", ours)
    for i in range(steps):
        yard = abs(l32[i] - l64[i])
        bound = max(R * yard, _loss_floor(l64[i], d64[i], i))
        err = abs(ours[i] - l64[i])
        print(f"step {i}: err {err:.3e}  yardstick {yard:.3e}  bound {bound:.3e}")
        assert err <= bound, (i, ours[i], l64[i], l32[i])
    res = [_held(f"final {k}", final[k], p32[k], p64[k]) for k in p64]
    bad = [r[1] for r in res if not r[0]]
    assert not bad, bad


def test_composes_with_the_mel_loss():
    """train.py:151-157 on V1 at U = 4: MelL1Loss(h)(gen(**x), y_mel) * 45 then .backward()."""
    import mel_ref
    from parrot_tts_amd import mel as M
    from parrot_tts_amd import synth
    z, m = mel_ref.load_golden(os.path.join(ROOT, "tests", "golden"), "mel_noise")
    h = _case("V1")[0]
    batch = {k: v.to(DEV) for k, v in synth.synth_voc_batch(2, 4, h, seed=VR.SEED).items()}
    crit = M.MelL1Loss(precision=None, basis=z["basis"], window=torch.from_numpy(z["window"]), n_fft=m["n_fft"], num_mels=m["num_mels"],
                       sampling_rate=m["sampling_rate"], hop_size=m["hop_size"], win_size=m["win_size"], fmin=m["fmin"], fmax=m["fmax"])
    runs = []
    for _ in range(2):
        model = _model("V1").train()
        wav = model(**batch)
        g = torch.Generator().manual_seed(5)
        y_mel = torch.randn((2, m["num_mels"], wav.shape[-1] // m["hop_size"]), generator=g).to(DEV)
        loss = crit(wav, y_mel) * 45
        loss.backward()
        runs.append([loss.detach()] + [p.grad for p in model.parameters()])
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in runs[0])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_error_paths_leave_the_module_usable():
    name = "V1"
    h, sd, batch = _case(name)
    model = _model(name).train()
    gpu = _gpu_batch(name)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        model(code=batch["code"], spkr=gpu["spkr"])
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        model(code=gpu["code"], spkr=batch["spkr"])
    with pytest.raises(ValueError):
        model(code=gpu["code"].int(), spkr=gpu["spkr"])
    with pytest.raises(ValueError):
        model(code=gpu["code"][0], spkr=gpu["spkr"])
    with pytest.raises(ValueError):
        model(code=gpu["code"], spkr=gpu["spkr"].float())
    with pytest.raises(ValueError):
        model(code=gpu["code"], spkr=gpu["spkr"][:1])
    with pytest.raises(KeyError):
        model(code=gpu["code"])
    with pytest.raises(NotImplementedError):
        model(code=gpu["code"], spkr=gpu["spkr"], emo=torch.zeros((2, 4), device=DEV))
    with pytest.raises(IndexError):
        model(code=torch.full_like(gpu["code"], h["num_embeddings"]), spkr=gpu["spkr"])
    wav = model(**gpu, f0=None)  # (the reference skips the f0 keyword, models.py:163-164)
    wav.sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    from parrot_tts_amd import TrainableCodeGenerator
    assert TrainableCodeGenerator is VT.TrainableCodeGenerator


def test_whole_file_under_poison():
    """This file once more in a child process under PARROT_POISON_WS=nan: a kernel reading a byte nobody wrote would turn a sample or
    a gradient into NaN there."""
    if os.environ.get("PARROT_POISON_WS"):
        return  # (already a poisoned run: the tests above were it)
    env = dict(os.environ, PARROT_POISON_WS="nan")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", os.path.abspath(__file__), "-k", "not whole_file"], cwd=ROOT,
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
