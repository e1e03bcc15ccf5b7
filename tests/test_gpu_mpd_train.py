"""GPU: training the multi-period discriminator on the device (parrot_tts_amd/discriminator_train.py over parrot_mpd_train_forward /
parrot_mpd_train_backward).

The rule is that of tests/test_gpu_voc_train.py: the restatement (tests/mpd_ref.py) run on the CPU in fp32 against its fp64 run on the
same inputs and the SAME device masks (read off our maps as map > 0) is the yardstick, both errors max-abs over the tensor; ours
against fp64 must be within R x that, with a floor of what is rounded once anyway, half an fp32 ulp of the tensor's largest magnitude.
  R = 8          tensors of 8 or more elements;
  R_SMALL = 256  tensors of fewer than 8 elements: on so few values the yardstick is a matter of chance.
DESIGN.md (section 3, "Multi-period discriminator training") has the table of the measured ratios.
Masks: for every site the device mask equals x64 > 0 wherever |x64| > 8 e_site (mpd_ref.own_inputs); what lies inside that band is
left out under the caps of voc_train_ref.check_caps.

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

import mpd_ref as MR  # noqa: E402
from parrot_tts_amd import discriminator_train as DT  # noqa: E402
from parrot_tts_amd import gan_loss as GL  # noqa: E402

DEV = "cuda:0"
R = 8.0
R_SMALL = 256.0
_runs, _refs, _ups = {}, {}, {}


def _model(name, sd=None):
    cfg, sd0 = MR.make_case(name)[:2]
    m = DT.TrainableMultiPeriodDiscriminator(cfg["periods"], cfg["channels"], cfg["kernel_size"], cfg["stride"])
    m.load_state_dict(sd if sd is not None else sd0, strict=True)
    return m.to(DEV)


def _upstream(name, outs=None):
    if name not in _ups:
        _ups[name] = MR.random_upstream(outs)
    return _ups[name]


def _masks(res):
    """The device masks in site order: map > 0 on the five activated maps of every period, real rows first."""
    return [torch.cat([r, g], 0) > 0 for fr, fg in zip(res[2], res[3]) for r, g in zip(fr[:5], fg[:5])]


def _step(model, name, kind, rows=None):
    """One training forward / backward of ours -> (flat outputs, {key -> grad}, d y_hat or None, masks).  kind: "random" (a seeded
    gradient at every score and map), "d" / "g" (the two real steps through gan_loss).  rows: a slice of the batch."""
    _, _, y, y_hat = MR.make_case(name)
    if rows is not None:
        y, y_hat = y[rows], y_hat[rows]
    model.zero_grad()
    y, y_hat = y.to(DEV), y_hat.to(DEV).requires_grad_(kind != "d")
    res = model(y, y_hat)
    outs = MR.flat_outputs(*res)
    if kind == "random":
        up = _upstream(name, outs)
        torch.autograd.backward(outs, [(u if rows is None else u[rows]).to(DEV) for u in up])
    elif kind == "d":
        GL.discriminator_adversarial_loss(res[0], res[1], [], [])[0].backward()
    else:
        GL.generator_adversarial_loss(res[1], [], res[2], res[3], [], [])[0].backward()
    grads = {k: p.grad for k, p in model.named_parameters()}
    return [o.detach() for o in outs], grads, y_hat.grad, _masks(res)


def _ours(name, kind):
    if (name, kind) not in _runs:
        _runs[(name, kind)] = _step(_model(name), name, kind)
    return _runs[(name, kind)]


def _ref(name, kind):
    """(fp64, fp32) results of the restatement under the device's masks, computed once per (case, upstream)."""
    if (name, kind) not in _refs:
        cfg, sd, y, y_hat = MR.make_case(name)
        run = _ours(name, kind)
        masks = [m.cpu() for m in run[3]]
        up = _upstream(name, run[0]) if kind == "random" else kind
        _refs[(name, kind)] = tuple(MR.loss_and_grads(sd, cfg, y, y_hat, dt, up, masks) for dt in (torch.float64, torch.float32))
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
    (o64, g64, d64, _, _), (o32, g32, d32, _, _) = _ref(name, kind)
    outs, grads, dyh, _ = _ours(name, kind)
    cfg = MR.make_case(name)[0]
    tag = f"{name} {kind}"
    names = MR.output_names(cfg)
    assert len(outs) == len(o64) == len(names)
    res = []
    for n, a, b32, b64 in zip(names, outs, o32, o64):
        assert a.shape == b64.shape, (n, a.shape, b64.shape)
        res.append(_held(f"{tag} {n}", a, b32, b64))
    assert set(grads) == set(g64)
    for k in g64:
        assert grads[k] is not None and grads[k].shape == g64[k].shape, k
        res.append(_held(f"{tag} d {k}", grads[k], g32[k], g64[k]))
    if kind == "d":
        assert dyh is None and d64 is None
    else:
        assert dyh is not None and dyh.shape == d64.shape
        res.append(_held(f"{tag} d y_hat", dyh, d32, d64))
    bad = [r[1] for r in res if not r[0]]
    assert not bad, bad


@pytest.mark.parametrize("name", MR.CASES)
def test_scores_maps_and_every_gradient(name):
    _check_all(name, "random")


def test_the_discriminator_step_gives_parameter_gradients_only():
    """train.py:141-148 on M1: mpd(y, y_g_hat.detach()) into discriminator_adversarial_loss; y_hat gets no gradient."""
    _check_all("M1", "d")


def test_the_generator_step_gives_d_y_hat():
    """train.py:159-165 on M1: generator_adversarial_loss on the scores and the maps, y_hat a leaf."""
    _check_all("M1", "g")


@pytest.mark.parametrize("name", MR.CASES)
def test_device_masks_are_the_fp64_signs_outside_the_band(name):
    in64, in32 = MR.own_inputs(name)
    masks = _ours(name, "random")[3]
    cfg = MR.make_case(name)[0]
    assert len(masks) == MR.n_sites(cfg) == len(in64)
    for m, x in zip(masks, in64):
        assert m.shape == x.shape and m.dtype == torch.bool
    counts = MR.excluded(in64, in32, masks)
    print(f"{name}: sites {len(counts)}  elements {sum(c[1] for c in counts)}  inside the band {sum(c[0] for c in counts)}  "
          f"mismatches outside the band {sum(c[2] for c in counts)}")
    share, worst = MR.check_caps(counts)
    print(f"{name}: excluded share {share:.2e}  worst site share {worst:.2e}")


def _same(a, b):
    assert all(torch.equal(x, y) for x, y in zip(a[0], b[0]))
    for k in a[1]:
        assert (a[1][k] is None and b[1][k] is None) or torch.equal(a[1][k], b[1][k]), k
    assert (a[2] is None and b[2] is None) or torch.equal(a[2], b[2])
    assert all(torch.equal(x, y) for x, y in zip(a[3], b[3]))


def test_two_runs_agree_bit_for_bit_also_under_deterministic_algorithms():
    name = "M2"
    a = _ours(name, "random")
    torch.use_deterministic_algorithms(True)
    try:
        b = _step(_model(name), name, "random")
    finally:
        torch.use_deterministic_algorithms(False)
    _same(a, b)


def test_a_row_does_not_see_the_rows_beside_it():
    name = "M2"
    outs, _, dyh, _ = _ours(name, "random")
    model = _model(name)
    for b in range(dyh.shape[0]):
        o1, _, d1, _ = _step(model, name, "random", rows=slice(b, b + 1))
        for n, full, row in zip(MR.output_names(MR.make_case(name)[0]), outs, o1):
            assert torch.equal(full[b:b + 1], row), (b, n)
        assert torch.equal(dyh[b:b + 1], d1), b


def test_no_grad_is_the_training_forward_and_keeps_no_graph():
    name = "M1"
    outs = _ours(name, "random")[0]
    _, _, y, y_hat = MR.make_case(name)
    model = _model(name)
    with torch.no_grad():
        res = model(y.to(DEV), y_hat.to(DEV))
    got = MR.flat_outputs(*res)
    assert all(not t.requires_grad and t.grad_fn is None for t in got)
    assert all(torch.equal(a, b) for a, b in zip(got, outs))
    # shapes and nesting are the reference's: per period a score (B, H p) and six maps (B, C, H, p)
    cfg = MR.make_case(name)[0]
    assert [len(x) for x in res] == [len(cfg["periods"])] * 4 and all(len(f) == 6 for f in res[2] + res[3])
    for i, p in enumerate(cfg["periods"]):
        assert res[2][i][5].shape[1] == 1 and res[2][i][5].shape[3] == p
        assert res[0][i].shape == (y.shape[0], res[2][i][5].shape[2] * p)


def test_a_frozen_parameter_gets_no_gradient_and_the_others_are_unchanged():
    name = "M4"
    base = _ours(name, "random")
    model = _model(name)
    frozen = ("discriminators.1.convs.2.weight_v", "discriminators.0.conv_post.weight_g", "discriminators.4.convs.0.bias",
              "discriminators.3.convs.0.weight_v", "discriminators.3.convs.0.weight_g")
    for k in frozen:
        model.get_parameter(k).requires_grad_(False)
    _, g2, d2, _ = _step(model, name, "random")
    for k in base[1]:
        if k in frozen:
            assert g2[k] is None, k
        else:
            assert torch.equal(g2[k], base[1][k]), k
    assert torch.equal(d2, base[2])


def test_remove_weight_norm_keeps_working_and_training():
    name = "M4"
    cfg, sd, y, y_hat = MR.make_case(name)
    model = _model(name)
    model.remove_weight_norm()
    keys = set(model.state_dict())
    assert not [k for k in keys if k.endswith("weight_g") or k.endswith("weight_v")] and "discriminators.0.conv_post.weight" in keys
    outs, grads, dyh, masks = _step(model, name, "random")
    plain = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    up = _upstream(name, outs)
    (o64, g64, d64, _, _), (o32, g32, d32, _, _) = (MR.loss_and_grads(plain, cfg, y, y_hat, dt, up, [m.cpu() for m in masks])
                                                    for dt in (torch.float64, torch.float32))
    res = [_held(f"{name} folded {n}", a, b32, b64) for n, a, b32, b64 in zip(MR.output_names(cfg), outs, o32, o64)]
    res += [_held(f"{name} folded d {k}", grads[k], g32[k], g64[k]) for k in g64] + [_held(f"{name} folded d y_hat", dyh, d32, d64)]
    bad = [r[1] for r in res if not r[0]]
    assert not bad, bad
    # the fold itself against the fp64 fold rounded once: norm, quotient and product are each rounded once, and so is the reference:
    # 4 x 2^-24 |w| <= 4 ulps of the tensor's largest weight (tests/test_gpu_voc_train.py)
    for k, v in MR.folded(sd).items():
        assert float((plain[k].double() - v.double()).abs().max()) <= 4 * float(np.spacing(np.float32(v.abs().max().item()))), k
    with pytest.raises(ValueError):
        model.remove_weight_norm()


# Floor of one loss of the trainer loop, absolute.  loss = sum_k mean((1 - dr_k)^2) + mean(dg_k^2).  What is rounded once anyway:
#   the loss itself: one ulp of it;
#   every score, rounded to fp32 once, half an ulp of itself (2^-24 |s|): |d loss| <= sum_k 2 mean(|1 - dr| |dr|) 2^-24 + 2 mean(dg^2) 2^-24;
#   from the second step on every parameter as AdamW stored it in fp32, which moves the scores by about their own rounding again.
def _loss_floor(loss64, s, step):
    return float(np.spacing(np.float32(loss64))) + (2 if step else 1) * 2 * s * 2.0 ** -24


def test_four_adamw_steps_of_the_discriminator_loss_against_the_restatement():
    name, steps = "M1", 4
    cfg, sd, y, y_hat = MR.make_case(name)
    model = _model(name)
    optim = torch.optim.AdamW(model.parameters(), lr=2e-4, betas=(0.8, 0.99))
    yd, yhd = y.to(DEV), y_hat.to(DEV)
    ours, all_masks = [], []
    for _ in range(steps):
        optim.zero_grad()
        res = model(yd, yhd.detach())
        loss = GL.discriminator_adversarial_loss(res[0], res[1], [], [])[0]
        loss.backward()
        all_masks.append([m.cpu() for m in _masks(res)])
        optim.step()
        ours.append(float(loss.detach()))
    final = {k: v.detach().cpu() for k, v in model.state_dict().items()}

    def loop(dtype):
        params = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
        opt = torch.optim.AdamW(list(params.values()), lr=2e-4, betas=(0.8, 0.99))
        losses, ss = [], []
        for i in range(steps):
            opt.zero_grad()
            r, g = MR.forward(params, cfg, y.to(dtype), y_hat.to(dtype), all_masks[i])[:2]
            loss = MR.d_loss(r, g)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
            ss.append(float(sum(((1 - a).abs() * a.abs()).mean() + (b ** 2).mean() for a, b in zip(r, g)).detach()))
        return losses, ss, {k: v.detach() for k, v in params.items()}

    l64, s64, p64 = loop(torch.float64)
    l32, _, p32 = loop(torch.float32)
    # the final parameters take the larger of the restatement's fp32 errors on one thread and on the machine's threads, as
    # tests/test_gpu_voc_train.py does and for its reason: where a gradient is as small as its rounding error, AdamW's update is
    # lr x noise and the fp32 restatement moves with its summation order
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
        bound = max(R * yard, _loss_floor(l64[i], s64[i], i))
        err = abs(ours[i] - l64[i])
        print(f"step {i}: err {err:.3e}  yardstick {yard:.3e}  bound {bound:.3e}")
        assert err <= bound, (i, ours[i], l64[i], l32[i])
    res = [_held(f"final {k}", final[k], p32[k], p64[k]) for k in p64]
    bad = [r[1] for r in res if not r[0]]
    assert not bad, bad


def test_a_call_after_an_error_path_gives_the_bits_of_a_first_call():
    name = "M4"
    base = _ours(name, "random")
    _, _, y, y_hat = MR.make_case(name)
    model = _model(name)
    yd, yhd = y.to(DEV), y_hat.to(DEV)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        model(y, yhd)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        model(yd, y_hat)
    with pytest.raises(ValueError):
        model(yd[:, 0], yhd[:, 0])
    with pytest.raises(ValueError):
        model(yd, yhd[..., :-1])
    with pytest.raises(ValueError):
        model(yd.double(), yhd.double())
    with pytest.raises(RuntimeError, match="Padding size should be less"):
        model(yd[..., :5], yhd[..., :5])  # p = 11: n_pad = 6 > 5, what F.pad refuses
    from parrot_tts_amd import _lib
    with pytest.raises(_lib.ParrotHipError, match="limits"):
        bad = DT.TrainableMultiPeriodDiscriminator([2], [4, 8, 33, 65], kernel_size=4).to(DEV)
        bad(yd, yhd)
    _same(base, _step(model, name, "random"))
    from parrot_tts_amd import TrainableMultiPeriodDiscriminator
    assert TrainableMultiPeriodDiscriminator is DT.TrainableMultiPeriodDiscriminator


def test_whole_file_under_poison():
    """This file once more in a child process under PARROT_POISON_WS=nan: a kernel reading a byte nobody wrote would turn a score, a
    map or a gradient into NaN there."""
    if os.environ.get("PARROT_POISON_WS"):
        return  # (already a poisoned run: the tests above were it)
    env = dict(os.environ, PARROT_POISON_WS="nan")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", os.path.abspath(__file__), "-k", "not whole_file"], cwd=ROOT,
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
