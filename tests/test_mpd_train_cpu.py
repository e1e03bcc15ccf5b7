"""CPU: what the multi-period discriminator's training path rests on and needs no device -- the restatement (tests/mpd_ref.py) against
the golden recorded from the reference (tools/make_mpd_goldens.py) and against central differences, the share of lrelu inputs that
the mask test leaves out, the new entry points in the headers, the export list and the ctypes table, the size of the saved buffer
against the formula of DESIGN.md, every refusal of the two calls, and the state dict's round trip."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mpd_ref as MR  # noqa: E402
from parrot_tts_amd import synth  # noqa: E402

NEW = ("parrot_mpd_train_forward", "parrot_mpd_train_backward", "parrot_mpd_train_saved_bytes", "parrot_mpd_train_workspace_bytes",
       "parrot_mpd_train_map_rows")
NEW_DEBUG = ("parrot_debug_mpd_conv_fwd", "parrot_debug_mpd_conv_dx", "parrot_debug_mpd_conv_dw_workspace_bytes", "parrot_debug_mpd_conv_dw",
             "parrot_debug_mpd_first_fwd", "parrot_debug_mpd_first_dx", "parrot_debug_mpd_first_dw_workspace_bytes", "parrot_debug_mpd_first_dw",
             "parrot_debug_mpd_post_fwd", "parrot_debug_mpd_post_dx", "parrot_debug_mpd_post_dw_workspace_bytes", "parrot_debug_mpd_post_dw")
E_INVALID, E_NOMEM = -1, -4


def test_restatement_without_masks_reproduces_the_reference_golden():
    """fp32 on one thread, the same torch calls in the same order: the scores bit for bit, and every map's fp64 sum within half an
    fp32 ulp of its sum of magnitudes."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "mpd_default.npz"))
    cfg = synth.default_mpd_config()
    sd = synth.synth_mpd_state_dict(cfg, seed=int(z["seeds"][0]))
    assert synth.state_digest(sd) == str(z["digest"])
    y, y_hat = synth.synth_mpd_batch(1, 400, seed=int(z["seeds"][1]))
    assert np.array_equal(y.numpy(), z["y"]) and np.array_equal(y_hat.numpy(), z["y_hat"])
    keep = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        with torch.no_grad():
            y_d_rs, y_d_gs, fmap_rs, fmap_gs, inputs = MR.forward(sd, cfg, y, y_hat)
    finally:
        torch.set_num_threads(keep)
    assert len(inputs) == MR.n_sites(cfg) == 25
    for i in range(5):
        assert np.array_equal(y_d_rs[i].numpy(), z[f"score_r{i}"]), i
        assert np.array_equal(y_d_gs[i].numpy(), z[f"score_g{i}"]), i
        for l in range(6):
            for tag, m in (("r", fmap_rs[i][l]), ("g", fmap_gs[i][l])):
                assert tuple(m.shape) == tuple(z[f"map_{tag}{i}_{l}_shape"]), (i, l)
                s, a = z[f"map_{tag}{i}_{l}_sums"]
                assert abs(float(m.double().sum()) - s) <= float(np.spacing(np.float32(a))) / 2, (tag, i, l)


def test_fp64_gradients_agree_with_central_differences():
    """M5, along one random direction per parameter and for y_hat, masks fixed at the base point's: h = 1e-6, to 1e-6 relative plus 1e-9."""
    cfg, sd, y, y_hat = MR.make_case("M5")
    sd64 = {k: v.double() for k, v in sd.items()}
    y64, yh64 = y.double(), y_hat.double()
    with torch.no_grad():
        res = MR.forward(sd64, cfg, y64, yh64)
    masks = [x > 0 for x in res[4]]
    up = [u.double() for u in MR.random_upstream(MR.flat_outputs(*res[:4]), seed=3)]
    _, grads, dyh, _, _ = MR.loss_and_grads(sd, cfg, y, y_hat, torch.float64, up, masks)
    g = torch.Generator().manual_seed(3)
    eps = 1e-6

    def objective(p, yh):
        with torch.no_grad():
            outs = MR.flat_outputs(*MR.forward(p, cfg, y64, yh, masks)[:4])
        return float(sum((o * u).sum() for o, u in zip(outs, up)))

    for k in list(sd) + ["y_hat"]:
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
    P = int(re.search(r"#define PARROT_MPD_MAX_PERIODS (\d+)", text["parrot_hip.h"]).group(1))
    L = int(re.search(r"#define PARROT_MPD_LAYERS (\d+)", text["parrot_hip.h"]).group(1))
    assert (P, L) == (_lib.MPD_MAX_PERIODS, _lib.MPD_LAYERS) == (8, 6)
    assert C.sizeof(_lib.MpdCfg) == 4 * (1 + P + 4 + 2 + 1)
    assert C.sizeof(_lib.MpdPtrs) == P * L * C.sizeof(_lib.VocLayerPtrs) == P * L * 24
    assert C.sizeof(_lib.MpdMaps) == P * L * 8
    assert _lib.lib().parrot_abi_version() == 7


def _model(name):
    from parrot_tts_amd.discriminator_train import TrainableMultiPeriodDiscriminator
    cfg = MR.make_case(name)[0]
    return TrainableMultiPeriodDiscriminator(cfg["periods"], cfg["channels"], cfg["kernel_size"], cfg["stride"])


def saved_bytes_formula(cfg):
    """DESIGN.md section 3, "Multi-period discriminator training": per period and layer the row norms (cout floats) and the folded
    weight (cout cin k floats), every buffer at a multiple of 256 bytes; the maps are the caller's."""
    a256 = lambda n: (4 * n + 255) // 256 * 256  # noqa: E731
    return sum(a256(cout) + a256(cout * cin * k) for _, cout, cin, k in synth.mpd_layer_shapes(cfg))


@pytest.mark.parametrize("name", ["M1", "M3", "M5"])
def test_saved_bytes_follow_the_formula(name):
    from parrot_tts_amd import _lib, build
    build.build()
    cfg, sd, y, _ = MR.make_case(name)
    c = _model(name)._cfg()
    lib = _lib.lib()
    for N, T in ((2 * y.shape[0], y.shape[-1]), (32, 8960)):
        assert lib.parrot_mpd_train_saved_bytes(C.byref(c), N, T) == saved_bytes_formula(cfg), (N, T)
        assert lib.parrot_mpd_train_workspace_bytes(C.byref(c), N, T) >= saved_bytes_formula(cfg)
    assert lib.parrot_mpd_train_saved_bytes(C.byref(c), 0, 400) == 0 and lib.parrot_mpd_train_saved_bytes(C.byref(c), 2, 0) == 0
    # the rows of every map are torch's: the shapes of the restatement's maps
    with torch.no_grad():
        fmap = MR.forward(sd, cfg, y, y)[2]
    for i in range(len(cfg["periods"])):
        for l in range(6):
            assert lib.parrot_mpd_train_map_rows(C.byref(c), y.shape[-1], i, l) == fmap[i][l].shape[2], (i, l)


def _call(lib, cfg, N, T, ptrs=None, ws_bytes=None, which="forward"):
    """One call on host memory that is never touched: every refusal happens before any launch."""
    from parrot_tts_amd import _lib
    dummy = (C.c_float * 4)()
    addr = C.addressof(dummy)
    if ptrs is None:
        ptrs = _lib.MpdPtrs()
        for i in range(_lib.MPD_MAX_PERIODS):
            for l in range(_lib.MPD_LAYERS):
                ptrs.layer[i][l].v = ptrs.layer[i][l].g = ptrs.layer[i][l].bias = addr
    maps = _lib.MpdMaps()
    for i in range(_lib.MPD_MAX_PERIODS):
        for l in range(_lib.MPD_LAYERS):
            maps.map[i][l] = addr
    if ws_bytes is None:
        ws_bytes = 1 << 62
    if which == "forward":
        return lib.parrot_mpd_train_forward(C.byref(cfg), C.byref(ptrs), addr, N, T, C.byref(maps), addr, addr, ws_bytes, None)
    return lib.parrot_mpd_train_backward(C.byref(cfg), C.byref(ptrs), addr, C.byref(maps), addr, C.byref(maps), N, T, C.byref(ptrs), addr, addr,
                                         ws_bytes, None)


@pytest.mark.parametrize("which", ["forward", "backward"])
def test_every_refusal_happens_before_any_launch(which):
    from parrot_tts_amd import _lib, build
    build.build()
    lib = _lib.lib()

    def cfg(**kw):
        c = _model("M1")._cfg()
        for k, v in kw.items():
            if k == "periods":
                c.n_periods = len(v)
                for i, p in enumerate(v[:_lib.MPD_MAX_PERIODS]):
                    c.periods[i] = p
            elif k == "width0":
                c.channels[0] = v
            else:
                setattr(c, k, v)
        return c

    bad = [("T <= n_pad", cfg(), 2, 5),                        # p = 11: n_pad = 6 > 5
           ("T == n_pad", cfg(periods=[4]), 2, 2),             # n_pad = 2 = T
           ("even kernel", cfg(kernel_size=4), 2, 400),
           ("kernel above TG_MAX_TAPS", cfg(kernel_size=13), 2, 400),
           ("nine periods", cfg(periods=[2] * 9), 2, 400),
           ("no period", cfg(periods=[]), 2, 400),
           ("period 0", cfg(periods=[2, 0]), 2, 400),
           ("N 0", cfg(), 0, 400),
           ("T 0", cfg(), 2, 0),
           ("width 0", cfg(width0=0), 2, 400),
           ("stride 0", cfg(stride=0), 2, 400)]
    for what, c, N, T in bad:
        assert _call(lib, c, N, T, which=which) == E_INVALID, what
        assert b"limits" in lib.parrot_last_error(), what
        assert lib.parrot_mpd_train_workspace_bytes(C.byref(c), N, T) == 0, what
    ptrs = _lib.MpdPtrs()  # every field null
    assert _call(lib, cfg(), 2, 400, ptrs=ptrs, which=which) == E_INVALID
    assert b"null parameter" in lib.parrot_last_error()
    need = lib.parrot_mpd_train_workspace_bytes(C.byref(cfg()), 2, 400)
    assert need > 0
    assert _call(lib, cfg(), 2, 400, ws_bytes=need - 1, which=which) == E_NOMEM
    assert b"workspace too small" in lib.parrot_last_error()
    assert lib.parrot_mpd_train_forward(None, None, None, 2, 400, None, None, None, 0, None) == E_INVALID
    assert b"null argument" in lib.parrot_last_error()


def test_debug_entry_points_refuse_their_limits_before_any_launch():
    from parrot_tts_amd import _lib, build
    build.build()
    lib = _lib.lib()
    dummy = (C.c_float * 4)()
    a = C.addressof(dummy)
    assert lib.parrot_debug_mpd_conv_fwd(a, a, a, a, 1, 4, 2, 4, 3, 8, 1, 0.1, None) == E_INVALID    # even k
    assert lib.parrot_debug_mpd_conv_fwd(a, a, a, a, 1, 4, 2, 13, 3, 64, 1, 0.1, None) == E_INVALID  # k > 11
    assert lib.parrot_debug_mpd_conv_fwd(a, a, a, a, 1, 4, 2, 3, 5, 8, 1, 0.1, None) == E_INVALID    # stride > k
    assert lib.parrot_debug_mpd_conv_dx(a, a, None, None, 0.1, a, 0, 4, 2, 5, 3, 8, None) == E_INVALID  # Z = 0
    assert lib.parrot_debug_mpd_conv_dw(a, a, a, 1, 4, 2, 5, 3, 8, a, 0, None) == E_INVALID          # workspace too small
    assert lib.parrot_debug_mpd_conv_dw_workspace_bytes(1, 4, 2, 5, 3, 0) == 0
    assert lib.parrot_debug_mpd_first_fwd(a, a, a, a, 1, 5, 11, 4, 5, 3, 0.1, None) == E_INVALID     # T <= n_pad
    assert lib.parrot_debug_mpd_first_dx(a, a, a, 1, 12, 0, 4, 5, 3, None) == E_INVALID              # period 0
    assert lib.parrot_debug_mpd_first_dw(a, a, a, 1, 12, 11, 4, 5, 3, a, 0, None) == E_INVALID       # workspace too small
    assert lib.parrot_debug_mpd_first_dw_workspace_bytes(1, 5, 11, 4, 5, 3) == 0
    assert lib.parrot_debug_mpd_post_fwd(a, a, a, a, 1, 0, 4, None) == E_INVALID                     # C = 0
    assert lib.parrot_debug_mpd_post_dx(a, a, None, None, 0.1, a, 1, 4, 0, None) == E_INVALID        # H = 0
    assert lib.parrot_debug_mpd_post_dw(a, a, a, 1, 4, 4, a, 0, None) == E_INVALID                   # workspace too small
    assert lib.parrot_debug_mpd_post_fwd(None, a, a, a, 1, 4, 4, None) == E_INVALID                  # null argument


def test_a_reference_shaped_state_dict_loads_strictly_and_saves_back_unchanged():
    from parrot_tts_amd.discriminator_train import TrainableMultiPeriodDiscriminator
    from parrot_tts_amd.dropin.utils.vocoder import models
    assert models.MultiPeriodDiscriminator is TrainableMultiPeriodDiscriminator
    cfg = dict(synth.default_mpd_config(), channels=[4, 8, 16, 32])  # (the default widths' dict is 164 MB; its keys and ranks are these)
    sd = synth.synth_mpd_state_dict(cfg, seed=7)
    m = TrainableMultiPeriodDiscriminator(channels=cfg["channels"])
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    back = m.state_dict()
    assert list(back) == list(sd)
    for k in sd:
        assert back[k].shape == sd[k].shape and torch.equal(back[k], sd[k]), k
    # with no arguments: the reference's keys and shapes
    full = TrainableMultiPeriodDiscriminator()
    want = {name: (cout, cin, k) for name, cout, cin, k in synth.mpd_layer_shapes(synth.default_mpd_config())}
    got = {k: tuple(v.shape) for k, v in full.state_dict().items()}
    assert len(got) == 3 * len(want) == 90
    for name, (cout, cin, k) in want.items():
        assert got[name + ".weight_v"] == (cout, cin, k, 1) and got[name + ".weight_g"] == (cout, 1, 1, 1) and got[name + ".bias"] == (cout,)
    assert all(isinstance(p, torch.nn.Parameter) for p in full.parameters())
    with pytest.raises(NotImplementedError, match="MSD"):
        TrainableMultiPeriodDiscriminator(use_spectral_norm=True)
