"""CPU: what the multi-scale discriminator's training path rests on and needs no device -- the restatement (tests/msd_ref.py) against
the golden recorded from the reference in train mode (tools/make_msd_goldens.py) and, in eval mode, against central differences; the
two-sigma rule; the pool; the share of lrelu inputs that the mask test leaves out; the new entry points in the headers, the export
list and the ctypes table; the refusals of the two calls; and the state dict's round trip."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from parrot_tts_amd import synth  # noqa: E402

synth.default_msd_config  # (the feature's first name: without it this file fails at import)
import msd_ref as MR  # noqa: E402

NEW = ("parrot_msd_train_forward", "parrot_msd_train_backward", "parrot_msd_train_saved_bytes", "parrot_msd_train_workspace_bytes",
       "parrot_msd_train_map_len")
NEW_DEBUG = ("parrot_debug_msd_gconv_fwd", "parrot_debug_msd_gconv_dx", "parrot_debug_msd_gconv_dw_workspace_bytes", "parrot_debug_msd_gconv_dw",
             "parrot_debug_msd_first_fwd", "parrot_debug_msd_first_dx", "parrot_debug_msd_first_dw_workspace_bytes", "parrot_debug_msd_first_dw",
             "parrot_debug_msd_pool_fwd", "parrot_debug_msd_pool_bwd", "parrot_debug_msd_sn_fold", "parrot_debug_msd_sn_bwd_workspace_bytes",
             "parrot_debug_msd_sn_bwd")
E_INVALID, E_NOMEM = -1, -4


def _one_thread(fn):
    keep = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        with torch.no_grad():
            return fn()
    finally:
        torch.set_num_threads(keep)


def test_restatement_in_train_mode_reproduces_the_reference_golden():
    """fp32 on one thread, the same torch calls in the same order.  Scores: to fp32 round-off, 4 ulps of the tensor's largest score
    (a conv's summation order is the library's own business).  Every map's fp64 sum within half an fp32 ulp of its sum of magnitudes
    plus 4 ulps of round-off per element's magnitude.  The buffers after the two power iterations: 4 ulps of one (unit vectors)."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "msd_default.npz"))
    cfg = synth.default_msd_config()
    sd = synth.synth_msd_state_dict(cfg, seed=int(z["seeds"][0]))
    assert synth.state_digest(sd) == str(z["digest"])
    assert list(sd) == [str(k) for k in z["keys"]]
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in z["shapes"]]
    y, y_hat = synth.synth_msd_batch(1, 400, seed=int(z["seeds"][1]))
    assert np.array_equal(y.numpy(), z["y"]) and np.array_equal(y_hat.numpy(), z["y_hat"])
    y_d_rs, y_d_gs, fmap_rs, fmap_gs, inputs, new = _one_thread(lambda: MR.forward(sd, cfg, y, y_hat))
    assert len(inputs) == MR.n_sites(cfg) == 21
    ulp = lambda a: float(np.spacing(np.float32(a)))  # noqa: E731
    for i in range(3):
        for got, want in ((y_d_rs[i].numpy(), z[f"score_r{i}"]), (y_d_gs[i].numpy(), z[f"score_g{i}"])):
            assert got.shape == want.shape and np.abs(got - want).max() <= 4 * ulp(np.abs(want).max()), i
        for l in range(8):
            for tag, m in (("r", fmap_rs[i][l]), ("g", fmap_gs[i][l])):
                assert tuple(m.shape) == tuple(z[f"map_{tag}{i}_{l}_shape"]), (i, l)
                s, a = z[f"map_{tag}{i}_{l}_sums"]
                assert abs(float(m.double().sum()) - s) <= ulp(a) / 2 + 4 * 2.0 ** -24 * a, (tag, i, l)
    after = [k[len("after:"):] for k in z.files if k.startswith("after:")]
    assert sorted(after) == sorted(new) and len(after) == 16
    for k in after:
        assert np.abs(new[k].numpy() - z["after:" + k]).max() <= 4 * ulp(1.0), k
        assert k.endswith("conv_post.weight_u") or not np.array_equal(z["after:" + k], sd[k].numpy()), k  # (train mode moved it)


def test_state_dict_keys_shapes_and_order_are_the_fixtures():
    from parrot_tts_amd.msd_train import TrainableMultiScaleDiscriminator
    z = np.load(os.path.join(ROOT, "tests", "golden", "msd_default.npz"))
    with torch.device("meta"):
        full = TrainableMultiScaleDiscriminator()
    got = full.state_dict()
    assert list(got) == [str(k) for k in z["keys"]]
    assert [",".join(str(d) for d in v.shape) for v in got.values()] == [str(s) for s in z["shapes"]]
    params, buffers = dict(full.named_parameters()), dict(full.named_buffers())
    for k in got:
        spectral_buffer = k.startswith("discriminators.0.") and (k.endswith("weight_u") or k.endswith("weight_v"))
        assert (k in buffers) == spectral_buffer and (k in params) != spectral_buffer, k


def test_fp64_eval_mode_gradients_agree_with_central_differences():
    """S5 in eval mode, where the output is a fixed function of weight_orig: sigma = u^T (W v) with u and v constants, so the spectral
    term of the backward is exercised.  u and v are first moved two iterations on (the seeded ones are far from converged: sigma
    would be near zero).  Along one random direction per parameter and for y_hat, masks fixed at the base point's: h = 1e-6, to 1e-6
    relative plus 1e-9."""
    cfg, sd, y, y_hat = MR.make_case("S5")
    sd64 = {k: v.double() for k, v in sd.items()}
    y64, yh64 = y.double(), y_hat.double()
    with torch.no_grad():
        sd64.update(MR.forward(sd64, cfg, y64, yh64)[5])
        res = MR.forward(sd64, cfg, y64, yh64, train=False)
    assert not res[5] or all(torch.equal(v, sd64[k]) for k, v in res[5].items())  # (eval: the buffers stay)
    masks = [x > 0 for x in res[4]]
    up = [u.double() for u in MR.random_upstream(MR.flat_outputs(*res[:4]), seed=3)]
    _, grads, dyh, _, _, _ = MR.loss_and_grads(sd64, cfg, y, y_hat, torch.float64, up, masks, train=False)
    assert set(grads) == set(MR.param_keys(sd)) and len(grads) == 8 * 2 + 16 * 3
    g = torch.Generator().manual_seed(3)
    eps = 1e-6

    def objective(p, yh):
        with torch.no_grad():
            outs = MR.flat_outputs(*MR.forward(p, cfg, y64, yh, masks, train=False)[:4])
        return float(sum((o * u).sum() for o, u in zip(outs, up)))

    for k in list(grads) + ["y_hat"]:
        base = yh64 if k == "y_hat" else sd64[k]
        d = torch.randn(base.shape, generator=g, dtype=torch.float64)
        vals = []
        for sign in (1, -1):
            p, yh = dict(sd64), yh64
            if k == "y_hat":
                yh = yh64 + sign * eps * d
            else:
                p[k] = sd64[k] + sign * eps * d
            vals.append(objective(p, yh))
        num, ana = (vals[0] - vals[1]) / (2 * eps), float(((dyh if k == "y_hat" else grads[k]) * d).sum())
        assert abs(num - ana) <= 1e-6 * abs(ana) + 1e-9, (k, num, ana)


def test_two_sigmas_in_train_mode_and_one_in_eval_mode():
    """With y == y_hat the reference's discriminator 0 still gives two different halves in train mode: the generated rows run one
    power iteration later.  In eval mode, and on the weight-normed scales in both modes, the halves are equal."""
    cfg, sd, y, _ = MR.make_case("S4")
    for train in (True, False):
        _, _, fr, fg, _, new = _one_thread(lambda: MR.forward(sd, cfg, y, y, train=train))
        for l in range(8):
            assert torch.equal(fr[0][l], fg[0][l]) != train, (train, l)
            assert torch.equal(fr[1][l], fg[1][l]) and torch.equal(fr[2][l], fg[2][l]), (train, l)
        for k, v in new.items():
            assert torch.equal(v, sd[k]) != (train and not k.endswith("conv_post.weight_u")), (train, k)


@pytest.mark.parametrize("T", [1, 2, 3, 5, 8])
def test_pool_restatement_is_avgpool1d(T):
    x = torch.randn(2, 1, T, generator=torch.Generator().manual_seed(T))
    want = torch.nn.AvgPool1d(4, 2, padding=2)(x)
    assert want.shape[-1] == T // 2 + 1
    assert torch.equal(MR.pool(x), want)
    # every window divides by 4, the padding counted
    xp = F.pad(x, (2, 2))
    hand = torch.stack([xp[..., 2 * i:2 * i + 4].sum(-1) / 4 for i in range(T // 2 + 1)], -1)
    assert torch.allclose(hand, want, rtol=0, atol=1e-6)


def test_any_length_works_down_to_one_sample():
    cfg, sd, _, _ = MR.make_case("S4")
    y, y_hat = synth.synth_msd_batch(1, 1, seed=5)
    res = _one_thread(lambda: MR.forward(sd, cfg, y, y_hat))
    assert all(m.shape[-1] == 1 for f in res[2] for m in f)


@pytest.mark.parametrize("name", MR.CASES)
def test_the_references_own_fp32_masks_stay_within_the_caps(name):
    in64, in32 = MR.own_inputs(name)
    counts = MR.excluded(in64, in32, None)
    share, worst = MR.check_caps(counts)
    print(f"{name}: inside the band {sum(c[0] for c in counts)} of {sum(c[1] for c in counts)}, share {share:.2e}, worst site {worst:.2e}")


def test_new_entry_points_are_declared_exported_and_bound():
    from parrot_tts_amd import _lib, build
    build.build()
    raw = C.CDLL(_lib.LIB_PATH)
    text = {}
    for header, names in (("parrot_hip.h", NEW), ("parrot_hip_debug.h", NEW_DEBUG)):
        text[header] = open(os.path.join(ROOT, "include", header)).read()
        src = re.sub(r"/\*.*?\*/", "", text[header], flags=re.S)
        for n in names:
            assert re.search(r"\b%s\s*\(" % n, src), f"{n} is not declared in {header}"
            assert hasattr(raw, n), f"{n} is not exported"
            assert n in _lib.SIGNATURES, f"{n} has no ctypes signature"
    S = int(re.search(r"#define PARROT_MSD_MAX_SCALES (\d+)", text["parrot_hip.h"]).group(1))
    L = int(re.search(r"#define PARROT_MSD_LAYERS (\d+)", text["parrot_hip.h"]).group(1))
    assert (S, L) == (_lib.MSD_MAX_SCALES, _lib.MSD_LAYERS) == (4, 8)
    assert C.sizeof(_lib.MsdCfg) == 4 * (1 + S + 7 + 7 + 1)
    assert C.sizeof(_lib.MsdPtrs) == S * L * C.sizeof(_lib.MsdLayerPtrs) == S * L * 40
    assert C.sizeof(_lib.MsdMaps) == S * L * 8
    assert _lib.lib().parrot_abi_version() == 7


def _model(name):
    from parrot_tts_amd.msd_train import TrainableMultiScaleDiscriminator
    cfg = MR.make_case(name)[0]
    return TrainableMultiScaleDiscriminator(cfg["channels"], cfg["groups"], cfg["n_scales"])


@pytest.mark.parametrize("name", ["S1", "S2", "S3"])
def test_map_lengths_and_saved_bytes(name):
    """The lengths of every map are torch's; the saved buffer holds at least every folded weight (two per spectral layer) and the
    pooled waveforms, and the workspace at least that."""
    from parrot_tts_amd import _lib, build
    build.build()
    cfg, sd, y, _ = MR.make_case(name)
    c = _model(name)._cfg()
    lib = _lib.lib()
    T = y.shape[-1]
    fmap = _one_thread(lambda: MR.forward(sd, cfg, y[:1, :, :min(T, 400)], y[:1, :, :min(T, 400)]))[2]
    for i in range(cfg["n_scales"]):
        for l in range(8):
            assert lib.parrot_msd_train_map_len(C.byref(c), min(T, 400), i, l) == fmap[i][l].shape[2], (i, l)
    per_scale = sum(cout * cin * k for _, cout, cin, k in synth.msd_layer_shapes(cfg)[:8])
    for N in (2, 32):
        pooled = N * ((T // 2 + 1) + ((T // 2 + 1) // 2 + 1))
        low = 4 * (per_scale * 4 + pooled)
        got = lib.parrot_msd_train_saved_bytes(C.byref(c), N, T)
        # (besides: row norms, u, v and sigma -- a few vectors per layer -- and each of some 110 buffers rounded up to 256 bytes)
        assert low <= got <= low + 4 * (24 * 4 * 1100) + 256 * 200, (N, got, low)
        assert lib.parrot_msd_train_workspace_bytes(C.byref(c), N, T) >= got
    assert lib.parrot_msd_train_saved_bytes(C.byref(c), 0, 400) == 0 and lib.parrot_msd_train_saved_bytes(C.byref(c), 2, 0) == 0
    assert lib.parrot_msd_train_saved_bytes(C.byref(c), 3, 400) == 0  # (N = 2 B)


def _call(lib, cfg, N, T, ptrs=None, ws_bytes=None, which="forward", iters=1):
    """One call on host memory that is never touched: every refusal happens before any launch."""
    from parrot_tts_amd import _lib
    dummy = (C.c_float * 4)()
    addr = C.addressof(dummy)
    if ptrs is None:
        ptrs = _lib.MsdPtrs()
        for i in range(_lib.MSD_MAX_SCALES):
            for l in range(_lib.MSD_LAYERS):
                p = ptrs.layer[i][l]
                p.v = p.bias = addr
                if cfg.spectral[i]:
                    p.u = p.sv = addr
                else:
                    p.g = addr
    maps = _lib.MsdMaps()
    for i in range(_lib.MSD_MAX_SCALES):
        for l in range(_lib.MSD_LAYERS):
            maps.map[i][l] = addr
    if ws_bytes is None:
        ws_bytes = 1 << 62
    if which == "forward":
        return lib.parrot_msd_train_forward(C.byref(cfg), C.byref(ptrs), addr, N, T, iters, C.byref(maps), addr, addr, ws_bytes, None)
    return lib.parrot_msd_train_backward(C.byref(cfg), C.byref(ptrs), addr, C.byref(maps), addr, C.byref(maps), N, T, C.byref(ptrs), addr, addr,
                                         ws_bytes, None)


@pytest.mark.parametrize("which", ["forward", "backward"])
def test_every_refusal_happens_before_any_launch(which):
    from parrot_tts_amd import _lib, build
    build.build()
    lib = _lib.lib()

    def cfg(**kw):
        c = _model("S1")._cfg()
        for k, v in kw.items():
            if k == "width":
                c.channels[v[0]] = v[1]
            elif k == "group":
                c.groups[v[0]] = v[1]
            else:
                setattr(c, k, v)
        return c

    bad = [("odd N", cfg(), 3, 400), ("N 0", cfg(), 0, 400), ("T 0", cfg(), 2, 0), ("no scale", cfg(n_scales=0), 2, 400),
           ("five scales", cfg(n_scales=5), 2, 400), ("width 0", cfg(width=(2, 0)), 2, 400),
           ("width not a multiple of its groups", cfg(width=(2, 33)), 2, 400), ("grouped first layer", cfg(group=(0, 2)), 2, 400),
           ("grouped last layer", cfg(group=(6, 5)), 2, 400), ("groups 0", cfg(group=(3, 0)), 2, 400)]
    for what, c, N, T in bad:
        assert _call(lib, c, N, T, which=which) == E_INVALID, what
        assert b"limits" in lib.parrot_last_error(), what
        assert lib.parrot_msd_train_workspace_bytes(C.byref(c), N, T) == 0, what
    ptrs = _lib.MsdPtrs()  # every field null
    assert _call(lib, cfg(), 2, 400, ptrs=ptrs, which=which) == E_INVALID
    assert b"null parameter" in lib.parrot_last_error()
    ok = cfg()
    ptrs = _lib.MsdPtrs()  # weight_g everywhere and no buffers: not what spectral scale 0 takes
    dummy = (C.c_float * 4)()
    for i in range(_lib.MSD_MAX_SCALES):
        for l in range(_lib.MSD_LAYERS):
            ptrs.layer[i][l].v = ptrs.layer[i][l].bias = ptrs.layer[i][l].g = C.addressof(dummy)
    assert _call(lib, ok, 2, 400, ptrs=ptrs, which=which) == E_INVALID
    assert b"spectral layer" in lib.parrot_last_error()
    need = lib.parrot_msd_train_workspace_bytes(C.byref(ok), 2, 400)
    assert need > 0
    assert _call(lib, ok, 2, 400, ws_bytes=need - 1, which=which) == E_NOMEM
    assert b"workspace too small" in lib.parrot_last_error()
    if which == "forward":
        assert _call(lib, ok, 2, 400, iters=2) == E_INVALID and b"power_iterations" in lib.parrot_last_error()
    assert lib.parrot_msd_train_forward(None, None, None, 2, 400, 1, None, None, None, 0, None) == E_INVALID
    assert b"null argument" in lib.parrot_last_error()
    assert lib.parrot_msd_train_map_len(C.byref(ok), 1, 2, 7) == 1  # (any T >= 1 works)


def test_debug_entry_points_refuse_their_limits_before_any_launch():
    from parrot_tts_amd import _lib, build
    build.build()
    lib = _lib.lib()
    dummy = (C.c_float * 4)()
    a = C.addressof(dummy)
    assert lib.parrot_debug_msd_gconv_fwd(a, a, a, a, 1, 4, 2, 1, 40, 2, 8, 1, 0.1, None) == E_INVALID    # even k
    assert lib.parrot_debug_msd_gconv_fwd(a, a, a, a, 1, 4, 2, 1, 43, 2, 64, 1, 0.1, None) == E_INVALID   # k > 41
    assert lib.parrot_debug_msd_gconv_fwd(a, a, a, a, 1, 4, 2, 1, 41, 5, 8, 1, 0.1, None) == E_INVALID    # stride > 4
    assert lib.parrot_debug_msd_gconv_fwd(a, a, a, a, 1, 4, 6, 4, 41, 2, 8, 1, 0.1, None) == E_INVALID    # c_out not a multiple of groups
    assert lib.parrot_debug_msd_gconv_dx(a, a, None, None, 0.1, a, 0, 4, 2, 1, 41, 2, 8, None) == E_INVALID  # Z = 0
    assert lib.parrot_debug_msd_gconv_dw(a, a, a, 1, 4, 2, 1, 41, 2, 8, a, 0, None) == E_INVALID          # workspace too small
    assert lib.parrot_debug_msd_gconv_dw_workspace_bytes(1, 4, 2, 1, 41, 2, 0) == 0
    assert lib.parrot_debug_msd_first_fwd(a, a, a, a, 1, 0, 4, 0.1, None) == E_INVALID                    # T = 0
    assert lib.parrot_debug_msd_first_dx(a, a, a, 1, 12, 0, None) == E_INVALID                            # no channel
    assert lib.parrot_debug_msd_first_dw(a, a, a, 1, 12, 4, a, 0, None) == E_INVALID                      # workspace too small
    assert lib.parrot_debug_msd_pool_fwd(a, a, 1, 0, None) == E_INVALID
    assert lib.parrot_debug_msd_pool_bwd(None, a, 1, 4, None) == E_INVALID
    assert lib.parrot_debug_msd_sn_fold(a, a, a, 2, 2, 0, a, a, a, 0, None) == E_INVALID                  # workspace too small
    assert lib.parrot_debug_msd_sn_bwd(a, a, a, a, a, a, None, a, a, a, 2, 2, a, 1 << 20, None) == E_INVALID  # gb without ub
    assert lib.parrot_debug_msd_sn_bwd_workspace_bytes(0, 2) == 0


def test_a_reference_shaped_state_dict_loads_strictly_and_saves_back_unchanged():
    from parrot_tts_amd.msd_train import TrainableMultiScaleDiscriminator
    from parrot_tts_amd.dropin.utils.vocoder import models
    import parrot_tts_amd
    assert models.MultiScaleDiscriminator is TrainableMultiScaleDiscriminator is parrot_tts_amd.TrainableMultiScaleDiscriminator
    cfg, sd = MR.make_case("S1")[:2]
    m = _model("S1")
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    back = m.state_dict()
    assert list(back) == list(sd)
    for k in sd:
        assert back[k].shape == sd[k].shape and torch.equal(back[k], sd[k]), k
    # a fresh module's buffers are unit vectors, as torch.nn.utils.spectral_norm leaves them
    fresh = _model("S1")
    for k, v in fresh.named_buffers():
        assert abs(float(v.double().norm()) - 1) < 1e-6, k
    # the multi-period module keeps refusing spectral norm, and says where it lives
    from parrot_tts_amd.discriminator_train import TrainableMultiPeriodDiscriminator
    with pytest.raises(NotImplementedError, match="TrainableMultiScaleDiscriminator"):
        TrainableMultiPeriodDiscriminator(use_spectral_norm=True)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        m(*MR.make_case("S1")[2:])
