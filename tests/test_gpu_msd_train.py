"""GPU: training the multi-scale discriminator on the device (parrot_tts_amd/msd_train.py over parrot_msd_train_forward /
parrot_msd_train_backward).

The rule is that of tests/test_gpu_mpd_train.py, unchanged: the restatement (tests/msd_ref.py) run on the CPU in fp32 against its fp64
run on the same inputs and the SAME device masks (read off our maps as map > 0) is the yardstick, both errors max-abs over the
tensor; ours against fp64 must be within R x that, with a floor of what is rounded once anyway, half an fp32 ulp of the tensor's
largest magnitude.
  R = 8          tensors of 8 or more elements;
  R_SMALL = 256  tensors of fewer than 8 elements: on so few values the yardstick is a matter of chance.
DESIGN.md (section 3, "Multi-scale discriminator training") has the table of the measured ratios.
Masks: for every site the device mask equals x64 > 0 wherever |x64| > 8 e_site (msd_ref.own_inputs); what lies inside that band is
left out under the caps of voc_train_ref.check_caps.
Everything runs in training mode unless a test says otherwise: discriminator 0's real rows on weight_orig / sigma after one power
iteration, its generated rows after two, the buffers two iterations on.

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

import msd_ref as MR  # noqa: E402
from parrot_tts_amd import gan_loss as GL  # noqa: E402
from parrot_tts_amd import msd_train as MT  # noqa: E402

DEV = "cuda:0"
R = 8.0
R_SMALL = 256.0
_runs, _refs, _ups = {}, {}, {}


def _model(name, sd=None):
    cfg, sd0 = MR.make_case(name)[:2]
    m = MT.TrainableMultiScaleDiscriminator(cfg["channels"], cfg["groups"], cfg["n_scales"])
    m.load_state_dict(sd if sd is not None else sd0, strict=True)
    return m.to(DEV)


def _upstream(name, outs=None):
    if name not in _ups:
        _ups[name] = MR.random_upstream(outs)
    return _ups[name]


def _masks(res):
    """The device masks in site order: map > 0 on the seven activated maps of every scale, real rows first."""
    return [torch.cat([r, g], 0) > 0 for fr, fg in zip(res[2], res[3]) for r, g in zip(fr[:7], fg[:7])]


def _buffers(model):
    return {k: v.detach().clone() for k, v in model.named_buffers()}


def _step(model, name, kind, rows=None, same=False):
    """One training forward / backward of ours -> (flat outputs, {key -> grad}, d y_hat or None, masks, the buffers afterwards).
    kind: "random" (a seeded gradient at every score and map), "d" / "g" (the two real steps through gan_loss).  rows: a slice of the
    batch.  same: y_hat = y."""
    _, _, y, y_hat = MR.make_case(name)
    if same:
        y_hat = y
    if rows is not None:
        y, y_hat = y[rows], y_hat[rows]
    model.zero_grad()
    y, y_hat = y.to(DEV), y_hat.to(DEV).clone().requires_grad_(kind != "d")
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
    return [o.detach() for o in outs], grads, y_hat.grad, _masks(res), _buffers(model)


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
    (o64, g64, d64, _, _, b64), (o32, g32, d32, _, _, b32) = _ref(name, kind)
    outs, grads, dyh, _, bufs = _ours(name, kind)
    cfg = MR.make_case(name)[0]
    tag = f"{name} {kind}"
    names = MR.output_names(cfg)
    assert len(outs) == len(o64) == len(names)
    res = []
    for n, a, b32_, b64_ in zip(names, outs, o32, o64):
        assert a.shape == b64_.shape, (n, a.shape, b64_.shape)
        res.append(_held(f"{tag} {n}", a, b32_, b64_))
    assert set(grads) == set(g64)
    for k in g64:
        assert grads[k] is not None and grads[k].shape == g64[k].shape, k
        res.append(_held(f"{tag} d {k}", grads[k], g32[k], g64[k]))
    if kind == "d":
        assert dyh is None and d64 is None
    else:
        assert dyh is not None and dyh.shape == d64.shape
        res.append(_held(f"{tag} d y_hat", dyh, d32, d64))
    assert set(bufs) == set(b64) and len(bufs) == 16
    for k in b64:  # weight_u and weight_v two power iterations on
        res.append(_held(f"{tag} buffer {k}", bufs[k], b32[k], b64[k]))
    bad = [r[1] for r in res if not r[0]]
    assert not bad, bad


@pytest.mark.parametrize("name", MR.CASES)
def test_scores_maps_every_gradient_and_the_buffers(name):
    _check_all(name, "random")


def test_the_discriminator_step_gives_parameter_gradients_only():
    """train.py:142-148 on S1: msd(y, y_g_hat.detach()) into discriminator_adversarial_loss; y_hat gets no gradient."""
    _check_all("S1", "d")


def test_the_generator_step_gives_d_y_hat():
    """train.py:160-165 on S1: generator_adversarial_loss on the scores and the maps, y_hat a leaf."""
    _check_all("S1", "g")


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


def test_eval_leaves_the_buffers_bit_for_bit_and_uses_one_sigma():
    """eval(): no power iteration.  With y == y_hat discriminator 0's halves are then bit-equal, and the buffers stay.  In train mode
    its halves differ (two sigmas) and the buffers move; the weight-normed scales' halves are bit-equal in both modes."""
    name = "S4"
    model = _model(name)
    model(*(t.to(DEV) for t in MR.make_case(name)[2:]))  # (one training forward: u and v leave their far-from-converged start)
    for train in (False, True):
        model.train(train)
        before = _buffers(model)
        outs, _, _, _, after = _step(model, name, "random", same=True)
        names = MR.output_names(MR.make_case(name)[0])
        for n, r, g in zip(names[0::2], outs[0::2], outs[1::2]):
            spectral = n.startswith("s0 ")
            assert torch.equal(r, g) != (spectral and train), (train, n)
        for k in before:
            if ".conv_post." in k:
                continue  # (one output row: v = +-W / ||W|| and u = +-1 are exact after the first iteration and stay)
            assert torch.equal(before[k], after[k]) != train, (train, k)
    # under no_grad a training-mode forward iterates too, as the reference's does
    before = _buffers(model)
    with torch.no_grad():
        model(*(t.to(DEV) for t in MR.make_case(name)[2:]))
    assert not torch.equal(before["discriminators.0.convs.3.weight_v"], model.discriminators[0].convs[3].weight_v)


def _same(a, b):
    assert all(torch.equal(x, y) for x, y in zip(a[0], b[0]))
    for k in a[1]:
        assert (a[1][k] is None and b[1][k] is None) or torch.equal(a[1][k], b[1][k]), k
    assert (a[2] is None and b[2] is None) or torch.equal(a[2], b[2])
    assert all(torch.equal(x, y) for x, y in zip(a[3], b[3]))
    assert all(torch.equal(a[4][k], b[4][k]) for k in a[4])


def test_two_runs_agree_bit_for_bit_also_under_deterministic_algorithms():
    name = "S2"
    a = _ours(name, "random")
    torch.use_deterministic_algorithms(True)
    try:
        b = _step(_model(name), name, "random")
    finally:
        torch.use_deterministic_algorithms(False)
    _same(a, b)


def test_a_row_does_not_see_the_rows_beside_it():
    """Rows [1:2] alone (a fresh module: the same buffers) reproduce their slice of every map, and of d y_hat, bit for bit."""
    name = "S2"
    outs, _, dyh, _, _ = _ours(name, "random")
    o1, _, d1, _, _ = _step(_model(name), name, "random", rows=slice(1, 2))
    for n, full, row in zip(MR.output_names(MR.make_case(name)[0]), outs, o1):
        assert torch.equal(full[1:2], row), n
    assert torch.equal(dyh[1:2], d1)


def test_no_grad_is_the_training_forward_and_keeps_no_graph():
    name = "S1"
    outs = _ours(name, "random")[0]
    _, _, y, y_hat = MR.make_case(name)
    model = _model(name)
    with torch.no_grad():
        res = model(y.to(DEV), y_hat.to(DEV))
    got = MR.flat_outputs(*res)
    assert all(not t.requires_grad and t.grad_fn is None for t in got)
    assert all(torch.equal(a, b) for a, b in zip(got, outs))
    # shapes and nesting are the reference's: per scale a score (B, L) and eight maps (B, C, L), the score the flattened eighth
    cfg = MR.make_case(name)[0]
    assert [len(x) for x in res] == [cfg["n_scales"]] * 4 and all(len(f) == 8 for f in res[2] + res[3])
    for i in range(cfg["n_scales"]):
        assert res[2][i][7].shape[:2] == (y.shape[0], 1) and res[0][i].shape == (y.shape[0], res[2][i][7].shape[2])
        assert torch.equal(res[0][i], res[2][i][7].flatten(1)) and torch.equal(res[1][i], res[3][i][7].flatten(1))


def test_one_sample_is_enough():
    """T = 1: every map of every scale has length 1, as the reference gives them; maps and d y_hat under the rule."""
    cfg, sd = MR.make_case("S4")[:2]
    y, y_hat = MR.synth.synth_msd_batch(2, 1, seed=9)
    model = _model("S4")
    yh = y_hat.to(DEV).requires_grad_(True)
    res = model(y.to(DEV), yh)
    outs = MR.flat_outputs(*res)
    up = [torch.ones(o.shape) for o in outs]
    torch.autograd.backward(outs, [u.to(DEV) for u in up])
    masks = [m.cpu() for m in _masks(res)]
    (o64, _, d64, _, _, _), (o32, _, d32, _, _, _) = (MR.loss_and_grads(sd, cfg, y, y_hat, dt, up, masks) for dt in (torch.float64, torch.float32))
    held = []
    for n, a, b32, b64 in zip(MR.output_names(cfg), outs, o32, o64):
        assert a.shape == b64.shape and a.shape[-1] == 1, n
        held.append(_held(f"T=1 {n}", a, b32, b64))
    held.append(_held("T=1 d y_hat", yh.grad, d32, d64))
    bad = [r[1] for r in held if not r[0]]
    assert not bad, bad


def test_a_frozen_parameter_gets_no_gradient_and_the_others_are_unchanged():
    name = "S4"
    base = _ours(name, "random")
    model = _model(name)
    frozen = ("discriminators.0.convs.2.weight_orig", "discriminators.0.conv_post.bias", "discriminators.1.convs.2.weight_v",
              "discriminators.1.conv_post.weight_g", "discriminators.2.convs.0.bias", "discriminators.2.convs.6.weight_v",
              "discriminators.2.convs.6.weight_g")
    for k in frozen:
        model.get_parameter(k).requires_grad_(False)
    _, g2, d2, _, _ = _step(model, name, "random")
    for k in base[1]:
        if k in frozen:
            assert g2[k] is None, k
        else:
            assert torch.equal(g2[k], base[1][k]), k
    assert torch.equal(d2, base[2])


def test_remove_weight_norm_keeps_working_and_training():
    name = "S4"
    cfg, sd, y, y_hat = MR.make_case(name)
    model = _model(name)
    model.remove_weight_norm()
    keys = set(model.state_dict())
    assert not [k for k in keys if k.endswith("weight_g")] and "discriminators.1.conv_post.weight" in keys
    assert "discriminators.0.convs.1.weight_orig" in keys and "discriminators.0.convs.1.weight_u" in keys  # (spectral norm stays)
    plain = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    assert list(plain) == list(MR.folded(sd))
    outs, grads, dyh, masks, bufs = _step(model, name, "random")
    up = _upstream(name, outs)
    (o64, g64, d64, _, _, b64), (o32, g32, d32, _, _, b32) = (MR.loss_and_grads(plain, cfg, y, y_hat, dt, up, [m.cpu() for m in masks])
                                                              for dt in (torch.float64, torch.float32))
    res = [_held(f"{name} folded {n}", a, b32_, b64_) for n, a, b32_, b64_ in zip(MR.output_names(cfg), outs, o32, o64)]
    res += [_held(f"{name} folded d {k}", grads[k], g32[k], g64[k]) for k in g64] + [_held(f"{name} folded d y_hat", dyh, d32, d64)]
    res += [_held(f"{name} folded buffer {k}", bufs[k], b32[k], b64[k]) for k in b64]
    bad = [r[1] for r in res if not r[0]]
    assert not bad, bad
    # the fold itself against the fp64 fold rounded once: norm, quotient and product are each rounded once, and so is the reference:
    # 4 x 2^-24 |w| <= 4 ulps of the tensor's largest weight (tests/test_gpu_voc_train.py)
    for k, v in MR.folded(sd).items():
        assert float((plain[k].double() - v.double()).abs().max()) <= 4 * float(np.spacing(np.float32(v.abs().max().item()))), k
    with pytest.raises(ValueError):
        model.remove_weight_norm()


def test_four_adamw_steps_of_the_discriminator_loss_against_the_restatement():
    """S2.  The restatement is stepped alike in fp64 and fp32 under the device's masks of every step, its buffers carried from step to
    step as ours are; the parameters and the buffers are held to the rule after EACH step."""
    name, steps = "S2", 4
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
        ours.append({k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
    keys = MR.param_keys(sd)

    def loop(dtype):
        state = {k: v.detach().to(dtype).clone().requires_grad_(k in keys) for k, v in sd.items()}
        opt = torch.optim.AdamW([state[k] for k in keys], lr=2e-4, betas=(0.8, 0.99))
        snaps = []
        for i in range(steps):
            opt.zero_grad()
            res = MR.forward(state, cfg, y.to(dtype), y_hat.to(dtype), all_masks[i])
            MR.d_loss(res[0], res[1]).backward()
            opt.step()
            state.update(res[5])
            snaps.append({k: v.detach().clone() for k, v in state.items()})
        return snaps

    s64, s32 = loop(torch.float64), loop(torch.float32)
    # the larger of the restatement's fp32 errors on one thread and on the machine's threads, as tests/test_gpu_mpd_train.py takes it
    # and for its reason: where a gradient is as small as its rounding error, AdamW's update is lr x noise
    keep = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        s32_one = loop(torch.float32)
    finally:
        torch.set_num_threads(keep)
    res = []
    for i in range(steps):
        for k in s64[i]:
            p32 = max((s32[i][k], s32_one[i][k]), key=lambda t: float((t.double() - s64[i][k]).abs().max()))
            res.append(_held(f"step {i} {k}", ours[i][k], p32, s64[i][k]))
    bad = [r[1] for r in res if not r[0]]
    assert not bad, bad


def test_an_in_place_write_to_a_returned_map_makes_backward_raise():
    name = "S4"
    _, _, y, y_hat = MR.make_case(name)
    model = _model(name)
    res = model(y.to(DEV), y_hat.to(DEV))
    with pytest.raises(RuntimeError, match="is a view and is being modified inplace"):
        res[2][1][3].mul_(2.0)  # (with grad enabled torch refuses the write itself: the maps are views of one node's outputs)
    with torch.no_grad():
        res[2][1][3].mul_(2.0)  # (without, the write goes through and the buffer the backward reads has changed)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        sum(s.sum() for s in res[0] + res[1]).backward()


def _torch_msd(cfg):
    """A torch module shaped like the reference's MultiScaleDiscriminator, from torch's own spectral_norm / weight_norm."""
    from torch import nn
    from torch.nn.utils import spectral_norm, weight_norm

    class S(nn.Module):
        def __init__(self, norm_f):
            super().__init__()
            c = [1] + list(cfg["channels"])
            self.convs = nn.ModuleList([norm_f(nn.Conv1d(c[l], c[l + 1], MR.KERNELS[l], MR.STRIDES[l], groups=cfg["groups"][l],
                                                         padding=(MR.KERNELS[l] - 1) // 2)) for l in range(7)])
            self.conv_post = norm_f(nn.Conv1d(c[7], 1, 3, 1, padding=1))

    class M(nn.Module):
        def __init__(self):
            super().__init__()
            self.discriminators = nn.ModuleList([S(spectral_norm if i == 0 else weight_norm) for i in range(cfg["n_scales"])])
            self.meanpools = nn.ModuleList([nn.AvgPool1d(4, 2, padding=2) for _ in range(cfg["n_scales"] - 1)])

    return M()


def test_a_state_dict_saved_from_a_reference_shaped_torch_module_loads_strictly(tmp_path):
    import warnings
    name = "S1"
    cfg, _, y, y_hat = MR.make_case(name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(11)
        ref = _torch_msd(cfg)
    path = tmp_path / "do_00000001"
    torch.save({"msd": ref.state_dict()}, path)
    sd = torch.load(path)["msd"]
    model = MT.TrainableMultiScaleDiscriminator(cfg["channels"], cfg["groups"], cfg["n_scales"])
    res = model.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys and list(model.state_dict()) == list(sd)
    model = model.to(DEV)
    outs, grads, dyh, masks, bufs = _step(model, name, "random")
    plain = {k: v.detach().clone() for k, v in sd.items()}
    up = _upstream(name, outs)
    (o64, g64, d64, _, _, b64), (o32, g32, d32, _, _, b32) = (MR.loss_and_grads(plain, cfg, y, y_hat, dt, up, [m.cpu() for m in masks])
                                                              for dt in (torch.float64, torch.float32))
    res = [_held(f"loaded {n}", a, b32_, b64_) for n, a, b32_, b64_ in zip(MR.output_names(cfg), outs, o32, o64)]
    res += [_held(f"loaded buffer {k}", bufs[k], b32[k], b64[k]) for k in b64]
    bad = [r[1] for r in res if not r[0]]
    assert not bad, bad


def test_a_call_after_an_error_path_gives_the_bits_of_a_first_call():
    name = "S4"
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
    with pytest.raises(ValueError):
        MT.TrainableMultiScaleDiscriminator(groups=(1, 4, 16, 16, 16, 16, 2))
    _same(base, _step(model, name, "random"))
    from parrot_tts_amd import TrainableMultiScaleDiscriminator
    assert TrainableMultiScaleDiscriminator is MT.TrainableMultiScaleDiscriminator


def test_whole_file_under_poison():
    """This file once more in a child process under PARROT_POISON_WS=nan: a kernel reading a byte nobody wrote would turn a score, a
    map, a gradient or a buffer into NaN there."""
    if os.environ.get("PARROT_POISON_WS"):
        return  # (already a poisoned run: the tests above were it)
    env = dict(os.environ, PARROT_POISON_WS="nan")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", os.path.abspath(__file__), "-k", "not whole_file"], cwd=ROOT,
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
