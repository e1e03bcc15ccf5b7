"""The reduced-precision modes PARROT_PREC_BF16 / PARROT_PREC_F16 (BASELINE configs[2]) held element by element to their contract
(include/parrot_hip.h: operands rounded once to bf16 / fp16, one MFMA per product group, fp32 accumulate), emulated on the CPU by
oracle/reduced.py.

Bounds are calibrated in the same run, never assumed:
  * layers: A = |conv|(|x^|, |w^|) + |b| + |r| element by element (fp64); e32 = max |y_f32 - y64| / A of an exact-fp32 ConvPlan on
    the same data is pure accumulation-order noise.  A reduced layer must satisfy
      (a) max |y - y^64| / A <= 4 e32 + 2^-24        (y^64: the rounded operands convolved in fp64)
      (b) max |y - y64| / A >= 16 (bf16) / 8 (f16) x that bound: the data can see a rounding error at all
      (c) the round-toward-zero emulation fails (a): the test tells the rounding mode apart.
    Layers the library keeps in fp32 (oracle.reduced.reduced_layer) meet the fp32 bound of test_gpu_parity.py instead.
  * vocoder: every stage that `stages=` returns, anchored at the library's own input of that stage, against the emulation of that
    stage: max |y - y^64| <= 4 D + 2^-20, D = max |y^32 - y^64| of two emulations that differ in accumulation only.  Teeth
    (max |y_f32 - y^64| >= 20 x the bound) are asserted on the single-conv stages (conv_pre, upsampling convs): inside an MRF
    stage (six chained convs per branch) a rounding flip that accumulation order causes moves later roundings by an operand
    ulp, and the flips compound until y^32 and y^64 are as far apart as rounded and unrounded -- measured ratio ~1 there.  Where
    a stage is small or the rounding grid coarse (bf16), the emulation pair may see no flip at all while the library sees one
    (measured: D = 5e-7 against a 1.6e-3 cascade in a 32-channel bf16 MRF row), so an MRF stage is held to 4 x the larger of D and
    its whole rounding effect |y_f32 - y^64|: a wrong tile, a stale slab or a missing row shows, a mis-rounded operand does not.
    Operand-level correctness of those kernels is what the layer tests pin."""
import hashlib
import os
import sys
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import parrot_oracle as O  # noqa: E402
from oracle import reduced as R  # noqa: E402
from parrot_tts_amd import ops, synth  # noqa: E402
from parrot_tts_amd.vocoder import AttrDict, CodeGenerator  # noqa: E402
from test_gpu_parity import CONV_CASES, _report  # noqa: E402

DEV = "cuda:0"
TEETH = {"bf16": 16.0, "f16": 8.0}
_CPU_SECONDS = {"layers": 0.0, "vocoder": 0.0}


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _randn(rng, *shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))


# ----------------------------------------------------------------------------------------------------------------------
# single layers
# ----------------------------------------------------------------------------------------------------------------------
def _conv64(x, w, b, transposed, stride, pad, dil):
    if transposed:
        return F.conv_transpose1d(x.double(), w.double(), None if b is None else b.double(), stride=stride, padding=pad)
    return F.conv1d(x.double(), w.double(), None if b is None else b.double(), padding=pad, dilation=dil)


def check_layer(mode, w, b, x, r=None, *, dil=1, pad=0, pre_slope=None, act=ops.ACT_NONE, transposed=False, stride=1,
                epilogue=ops.EPI_STORE, div=1.0, prior=None, rows=None, tag=""):
    """Run one layer in `mode` and in exact fp32 on the GPU and hold it to the bounds above (rows: the batch rows compared)."""
    args = dict(dilation=dil, padding=pad, transposed=transposed, stride=stride, pre_act=int(pre_slope is not None),
                pre_slope=0.0 if pre_slope is None else pre_slope, act=act)
    xd, rd = x.to(DEV), None if r is None else r.to(DEV)

    def run(prec):
        plan = ops.ConvPlan(w, b, precision=prec, **args)
        out = None if prior is None else prior.to(DEV).clone()
        return plan(xd, rd, out=out, epilogue=epilogue, div=div).cpu()
    y, y32 = run(ops.PREC_NAMES[mode]), run(ops.PREC_F32)
    t0 = time.time()
    sel = slice(None) if rows is None else list(rows)
    x, y, y32 = x[sel], y[sel], y32[sel]
    r = None if r is None else r[sel]
    prior = None if prior is None else prior[sel]
    xin = x if pre_slope is None else F.leaky_relu(x, pre_slope)

    def finish(v, absolute=False):  # activation, residual, epilogue -- in fp64 (absolute: the magnitudes A is made of)
        if absolute:
            v = v + (0 if r is None else r.double().abs())
            if epilogue == ops.EPI_ADD:
                v = prior.double().abs() + v
            elif epilogue == ops.EPI_ADD_DIV:
                v = (prior.double().abs() + v) / div
            return v
        if act == ops.ACT_RELU:
            v = torch.relu(v)
        elif act == ops.ACT_TANH:
            v = torch.tanh(v)
        if r is not None:
            v = v + r.double()
        if epilogue == ops.EPI_ADD:
            v = prior.double() + v
        elif epilogue == ops.EPI_ADD_DIV:
            v = (prior.double() + v) / div
        return v
    y64 = finish(_conv64(xin, w, b, transposed, stride, pad, dil))
    c_in, c_out = (w.shape[0], w.shape[1]) if transposed else (w.shape[1], w.shape[0])
    act_s = {ops.ACT_NONE: "none", ops.ACT_RELU: "relu", ops.ACT_TANH: "tanh"}[act]
    red = R.reduced_layer("convt" if transposed else "conv", c_in, c_out, w.shape[2], stride, dilation=dil, padding=pad,
                          pre_slope=pre_slope, act=act_s)
    rec = dict(test="reduced_layer", tag=tag, mode=mode, cin=int(c_in), cout=int(c_out), k=int(w.shape[2]), dil=dil, T=int(x.shape[2]),
               transposed=transposed, reduced=red)
    if not red:
        err = float((y.double() - y64).abs().max())
        rec.update(err_fp32=err / max(1.0, float(y64.abs().max())))
        _report(**rec)
        _CPU_SECONDS["layers"] += time.time() - t0
        assert err <= 2e-5 * max(1.0, float(y64.abs().max())), rec
        return rec
    ws = R.f16_weight_scale(w) if mode == "f16" else 1.0
    xr, wr = R.round_operand(xin, mode, R.F16_XS), R.round_operand(w, mode, ws)
    xz, wz = R.round_operand(xin, mode, R.F16_XS, rtz=True), R.round_operand(w, mode, ws, rtz=True)
    yh = finish(_conv64(xr, wr, b, transposed, stride, pad, dil))
    yz = finish(_conv64(xz, wz, b, transposed, stride, pad, dil))
    A = finish(_conv64(xr.abs(), wr.abs(), None if b is None else b.abs(), transposed, stride, pad, dil), absolute=True)
    A = torch.clamp(A, min=1e-30)
    e32 = float(((y32.double() - y64).abs() / A).max())
    bound = 4 * e32 + 2.0 ** -24
    ea = float(((y.double() - yh).abs() / A).max())
    eb = float(((y.double() - y64).abs() / A).max())
    ez = float(((y.double() - yz).abs() / A).max())
    rec.update(e32=e32, bound=bound, ratio_a=ea / bound, teeth_b=eb / bound, teeth_rtz=ez / bound)
    _report(**rec)
    _CPU_SECONDS["layers"] += time.time() - t0
    assert bool(torch.isfinite(y).all()), rec
    assert ea <= bound, ("(a) the reduced kernel is not the emulation plus accumulation noise", rec)
    assert eb >= TEETH[mode] * bound, ("(b) this shape / data cannot see a rounding error", rec)
    assert ez > bound, ("(c) round-toward-zero passes too: the test cannot see the rounding mode", rec)
    return rec


@pytest.fixture(params=list(R.MODES))
def mode(request):
    return request.param


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv_cases_match_the_rounding_emulation(case, mode):
    cin, cout, k, dil, B, T, pre, res, act = case
    rng = _rng(cin * 131 + cout * 7 + k + dil + T + 99)
    w = _randn(rng, cout, cin, k, scale=1.0 / np.sqrt(cin * k))
    b = _randn(rng, cout, scale=0.1)
    x = _randn(rng, B, cin, T)
    r = _randn(rng, B, cout, T) if res else None
    check_layer(mode, w, b, x, r, dil=dil, pad=dil * (k - 1) // 2, pre_slope=0.1 if pre else None, act=act, tag="conv_cases")


def test_fuzz_wide_layers_match_the_rounding_emulation(mode):
    """The seeded draw of test_conv1d_fuzz_wide_layers_all_kernel_variants (conv_split16 128- / 64-row tiles and their 64-column
    variants, conv_split, exact kernel), in the reduced modes."""
    rng = _rng(2024)
    for case in range(48):
        cin = int(rng.choice([32, 64, 96, 128, 160, 256, 48, 20]))
        cout = int(rng.choice([64, 128, 192, 256, 72, 1024]))
        k = int(rng.choice([1, 3, 7, 9, 11]))
        dil = int(rng.choice([1, 3, 5])) if k > 1 else 1
        B = int(rng.integers(1, 4))
        T = int(rng.choice([1, 15, 63, 64, 65, 127, 128, 129, 191, 193, 255, 257, 300, 511, 640, 700]))
        pre, res, act = bool(rng.integers(0, 2)), bool(rng.integers(0, 2)), int(rng.choice([0, 0, 1]))
        w = _randn(rng, cout, cin, k, scale=1.0 / np.sqrt(cin * k))
        b = _randn(rng, cout, scale=0.1)
        x = _randn(rng, B, cin, T)
        r = _randn(rng, B, cout, T) if res else None
        check_layer(mode, w, b, x, r, dil=dil, pad=dil * (k - 1) // 2, pre_slope=0.1 if pre else None, act=act, tag=f"fuzz{case}")


def test_chip_filling_launches_match_the_rounding_emulation(mode):
    """The seeded draw of test_conv1d_fuzz_chip_filling_launches_take_the_wide_tiles (128 x 128, 128 x 160 and 64 x 128 tiles of
    conv_split16, partial last column tiles); three batch rows -- first, middle, last -- are compared."""
    rng = _rng(4242)
    for case in range(10):
        cin = int(rng.choice([64, 128, 256]))
        cout = int(rng.choice([64, 128, 256]))
        k = int(rng.choice([7, 11]))
        dil = int(rng.choice([1, 3, 5]))
        B = int(rng.choice([24, 33, 48]))
        T = int(rng.choice([330, 641, 1250, 1285, 1601]))
        pre, res = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        w = _randn(rng, cout, cin, k, scale=1.0 / np.sqrt(cin * k))
        b = _randn(rng, cout, scale=0.1)
        x = _randn(rng, B, cin, T)
        r = _randn(rng, B, cout, T) if res else None
        check_layer(mode, w, b, x, r, dil=dil, pad=dil * (k - 1) // 2, pre_slope=0.1 if pre else None, rows=(0, B // 2, B - 1),
                    tag=f"chip{case}")


# every conv shape of the full-size vocoder (models.py:80-106 with utils/vocoder/config.json), T around the tile edges
EDGE_T = [1, 63, 64, 65, 127, 128, 129, 160, 161, 255, 257, 641, 1285]
VOC_CONVS = [  # (kind, cin, cout, k, stride or dilation)
    ("conv", 256, 512, 7, 1),
    ("convt", 512, 256, 11, 5), ("convt", 256, 128, 8, 4), ("convt", 128, 64, 8, 4), ("convt", 64, 32, 4, 2), ("convt", 32, 16, 4, 2),
] + [("rb", c, c, k, d) for c in (256, 128, 64, 32) for k in (3, 7, 11) for d in (1, 3, 5)] + [("conv", 16, 1, 7, 1)]


def test_full_vocoder_layer_shapes_at_tile_edges(mode):
    rng = _rng(31337)
    for j, (kind, cin, cout, k, sd) in enumerate(VOC_CONVS):
        for T in (EDGE_T[j % len(EDGE_T)], EDGE_T[(j * 5 + 3) % len(EDGE_T)]):
            if kind == "convt":
                w = _randn(rng, cin, cout, k, scale=1.0 / np.sqrt(cin * k / sd))
                b = _randn(rng, cout, scale=0.1)
                x = _randn(rng, 2, cin, T)
                check_layer(mode, w, b, x, pre_slope=0.1, transposed=True, stride=sd, pad=(k - sd) // 2, tag=f"voc_{kind}")
            else:
                dil = sd if kind == "rb" else 1
                w = _randn(rng, cout, cin, k, scale=1.0 / np.sqrt(cin * k))
                b = _randn(rng, cout, scale=0.1)
                x = _randn(rng, 2, cin, T)
                r = _randn(rng, 2, cout, T) if kind == "rb" else None
                check_layer(mode, w, b, x, r, dil=dil, pad=dil * (k - 1) // 2, pre_slope=0.1 if cout > 1 else 0.01,
                            act=ops.ACT_TANH if cout == 1 else ops.ACT_NONE, tag=f"voc_{kind}")


@pytest.mark.parametrize("slope", [0.1, 0.01])
def test_epilogues_activations_and_residual(mode, slope):
    """EPI_ADD / EPI_ADD_DIV (the MRF sum), ReLU, leaky ReLU 0.1 / 0.01, a residual, on the conv_split16 and conv_split kernels."""
    rng = _rng(int(slope * 1000) + 7)
    B, T = 2, 333
    for cin, cout, k, dil in ((64, 64, 3, 1), (128, 128, 7, 3), (256, 256, 11, 1), (32, 32, 3, 5)):
        w = _randn(rng, cout, cin, k, scale=1.0 / np.sqrt(cin * k))
        b = _randn(rng, cout, scale=0.1)
        x = _randn(rng, B, cin, T)
        r = _randn(rng, B, cout, T)
        prior = _randn(rng, B, cout, T)
        pad = dil * (k - 1) // 2
        check_layer(mode, w, b, x, r, dil=dil, pad=pad, pre_slope=slope, epilogue=ops.EPI_ADD, prior=prior, tag="epi_add")
        check_layer(mode, w, b, x, r, dil=dil, pad=pad, pre_slope=slope, epilogue=ops.EPI_ADD_DIV, div=3.0, prior=prior, tag="epi_add_div")
        check_layer(mode, w, b, x, None, dil=dil, pad=pad, pre_slope=slope, act=ops.ACT_RELU, tag="relu")


def test_f16_range_overflows_loudly_and_tiny_weights_keep_accuracy():
    """Mirror of test_split_f16_scaling_...: the single-piece fp16 mode scales activations by 8 (|x| >= 8190 -> inf in the
    output, never a wrong finite value) and the layer's weights by a power of two (1e-6-scale weights keep full relative accuracy)."""
    rng = _rng(78)
    cin, cout, k, T = 64, 64, 3, 512
    mag = torch.from_numpy(10.0 ** rng.uniform(-3, 3, size=(1, cin, T))).float()
    x = _randn(rng, 1, cin, T) * mag
    for wscale in (1e-6, 1.0, 300.0):
        w = _randn(rng, cout, cin, k, scale=wscale / np.sqrt(cin * k))
        b = _randn(rng, cout, scale=0.1 * wscale)
        check_layer("f16", w, b, x, pad=1, tag=f"f16_wscale_{wscale:g}")
    x[0, 3, 100] = 8190.0
    x[0, 7, 300] = -9000.0
    y = ops.ConvPlan(w, None, padding=1, precision=ops.PREC_F16)(x.to(DEV)).cpu()
    # every output channel at every tap that reads an overflowed input is non-finite (all weights are nonzero)
    assert not bool(torch.isfinite(y[0, :, 99:102]).any()) and not bool(torch.isfinite(y[0, :, 299:302]).any())
    keep = torch.ones(T, dtype=torch.bool)
    keep[99:102] = False
    keep[299:302] = False
    assert bool(torch.isfinite(y[0][:, keep]).all())  # every output whose inputs are in range stays finite ...
    x[0, 3, 100] = 8189.0
    x[0, 7, 300] = -8189.0
    y = ops.ConvPlan(w, None, padding=1, precision=ops.PREC_F16)(x.to(DEV)).cpu()
    assert bool(torch.isfinite(y).all())  # ... and 8189 is still in range


# ----------------------------------------------------------------------------------------------------------------------
# vocoder
# ----------------------------------------------------------------------------------------------------------------------
_EMU_CACHE = {}


def _stage_emulations(h, sd, stage, x, mode, fused):
    """(y^64, y^32, y_fp32) of one stage from input x; cached by the input's bytes (fused modes 1 and 2 run the same kernels)."""
    key = (id(sd), stage, mode, 0 if fused == 0 else 2, tuple(x.shape), hashlib.sha1(x.numpy().tobytes()).hexdigest())
    if key not in _EMU_CACHE:
        y64 = R.generator_stage_reduced(sd, h, stage, x, mode, torch.float64, fused)
        y32 = R.generator_stage_reduced(sd, h, stage, x, mode, torch.float32, fused)
        yf = R.generator_stage_reduced(sd, h, stage, x, None)
        _EMU_CACHE[key] = (y64, y32, yf)
    return _EMU_CACHE[key]


def _stage_lengths(h, U):
    out, T = {"conv_pre": U}, U
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        T = (T - 1) * u - 2 * ((k - u) // 2) + k
        out[f"ups{i}"] = out[f"mrf{i}"] = T
    out["post"] = T
    return out


_LAYERS = {}


def _single_conv_stage(name, h, stage, fused):
    """conv_pre / ups_i: one conv -- is it a reduced one?"""
    if (name, fused) not in _LAYERS:
        _LAYERS[(name, fused)] = R.vocoder_layers(h, fused)
    layers = _LAYERS[(name, fused)]
    convs = [l for l in layers if l[0] != "rb"]
    idx = 0 if stage == "conv_pre" else 1 + int(stage[3:])
    return convs[idx][4]


_VOC_SD = {}


def _voc_case(name):
    if name not in _VOC_SD:
        if name == "small_ragged":
            h = synth.small_voc_config()
            sd = synth.synth_voc_state_dict(h, seed=9, scale=1.0)
            b = synth.synth_voc_batch(3, 31, h, seed=12)
            lens = torch.tensor([31, 17, 24], dtype=torch.int64)
        else:
            h = synth.default_voc_config()
            sd = synth.synth_voc_state_dict(h, seed=1234, scale=1.0)
            b = synth.synth_voc_batch(2, 40, h, seed=2) if name == "full_u40" else synth.synth_voc_batch(2, 256, h, seed=3)
            lens = None
        _VOC_SD[name] = (h, sd, b, lens)
    return _VOC_SD[name]


@pytest.mark.parametrize("fused", [0, 1, 2])
@pytest.mark.parametrize("name", ["full_u40", "full_u256", "small_ragged"])
def test_vocoder_stages_match_the_rounding_emulation(name, mode, fused):
    h, sd, b, lens = _voc_case(name)
    B, U = b["code"].shape
    ops.set_default_precision(ops.PREC_NAMES[mode])
    ops.set_fused_resblocks(fused)
    try:
        g = CodeGenerator(AttrDict(h))
        g.load_state_dict(sd)
        g = g.eval().to(DEV)
        st = {}
        y = g(code=b["code"].to(DEV), spkr=b["spkr"].to(DEV), stages=st, unit_lens=None if lens is None else lens.to(DEV))
        torch.cuda.synchronize()
    finally:
        ops.set_default_precision(ops.PREC_DEFAULT)
        ops.set_fused_resblocks(2)
    t0 = time.time()
    st = {k: v.cpu() for k, v in st.items()}
    st["post"] = y.cpu()
    with torch.no_grad():
        emb = {}
        O.code_generator_forward(sd, h, b["code"], b["spkr"], stages=emb)  # (the embedding only: exact in every mode)
    L = _stage_lengths(h, U)
    names = ["conv_pre"] + [f"{p}{i}" for i in range(len(h["upsample_rates"])) for p in ("ups", "mrf")] + ["post"]
    rows = range(B)
    prev_full = emb["embed"]
    for stage in names:
        got = st[stage]
        worst = (0.0, 0.0, 0.0)
        for r in rows:
            n_in = U if stage == "conv_pre" else L[names[names.index(stage) - 1]]
            n_out = L[stage]
            if lens is not None:  # ragged: the row as the library sees it -- its own length, zero padded at its own end
                n_in = _stage_lengths(h, int(lens[r]))["conv_pre"] if stage == "conv_pre" else \
                    _stage_lengths(h, int(lens[r]))[names[names.index(stage) - 1]]
                n_out = _stage_lengths(h, int(lens[r]))[stage]
            xin = prev_full[r:r + 1, :, :n_in].contiguous()
            y64, y32, yf = _stage_emulations(h, sd, stage, xin, mode, fused)
            yg = got[r:r + 1, :, :n_out].double()
            D = float((y32.double() - y64.double()).abs().max())
            teeth = float((yf.double() - y64.double()).abs().max())
            if stage.startswith("mrf"):  # chained convs: D is a sample of rare flip cascades (see the module docstring)
                D = max(D, teeth)
            bound = 4 * D + 2.0 ** -20
            err = float((yg - y64.double()).abs().max())
            worst = max(worst, (err / bound, teeth / bound, bound))
            assert err <= bound, (name, fused, mode, stage, r, err, D)
            if stage in ("conv_pre",) or stage.startswith("ups"):
                if _single_conv_stage(name, h, stage, fused):
                    assert teeth >= 20 * bound, ("a single-conv stage cannot see its rounding", name, stage, r, teeth, bound)
        _report(test="reduced_vocoder_stage", case=name, mode=mode, fused=fused, stage=stage, ratio=worst[0], teeth=worst[1],
                bound=worst[2])
        prev_full = got
    _CPU_SECONDS["vocoder"] += time.time() - t0
    _report(test="reduced_cpu_seconds", **_CPU_SECONDS)


def test_vocoder_waveform_end_to_end_within_the_emulations_spread(mode):
    """The whole waveform of the small config against an unanchored emulation: within 4 x the spread of two emulations.  A
    GROSS-ERROR check only (a wrong tile, a stale slab, a dropped row): through the whole generator rounding flips compound until
    that spread is as large as the rounding itself, so this cannot tell the reduced modes from fp32 -- the layer tests and
    test_isolated_resblock_pairs_match_the_rounding_emulation do."""
    h, sd, b, lens = _voc_case("small_ragged")
    ops.set_default_precision(ops.PREC_NAMES[mode])
    try:
        g = CodeGenerator(AttrDict(h))
        g.load_state_dict(sd)
        y = g.eval().to(DEV)(code=b["code"].to(DEV), spkr=b["spkr"].to(DEV)).cpu().double()
    finally:
        ops.set_default_precision(ops.PREC_DEFAULT)
    y64 = R.code_generator_forward_reduced(sd, h, b["code"], b["spkr"], mode, torch.float64).double()
    y32 = R.code_generator_forward_reduced(sd, h, b["code"], b["spkr"], mode, torch.float32).double()
    D = float((y32 - y64).abs().max())
    err = float((y - y64).abs().max())
    _report(test="reduced_vocoder_e2e", mode=mode, ratio=err / (4 * D + 2.0 ** -20), D=D)
    assert err <= 4 * D + 2.0 ** -20


# ----------------------------------------------------------------------------------------------------------------------
# ResBlock pair kernels and the whole-MRF kernel, isolated: one intermediate rounding per branch
# ----------------------------------------------------------------------------------------------------------------------
def _single_pair_state_dict(h, seed):
    """A generator whose every ResBlock1 keeps only its first pair: the later pairs have zero weights (weight_g = 0) and zero
    biases, so they add exactly 0 to the residual and each branch is r = x + conv2(q(lrelu(conv1(q(lrelu(x)))))) -- ONE
    intermediate rounding between the library's stage input and its stage output, as the pair kernels / whole-MRF kernel /
    layer plans of that stage evaluate it."""
    sd = synth.synth_voc_state_dict(h, seed=seed, scale=1.0)
    for key in list(sd):
        if key.startswith("resblocks.") and (".convs1.1." in key or ".convs2.1." in key or ".convs1.2." in key or ".convs2.2." in key):
            if key.endswith(".weight_g") or key.endswith(".bias"):
                sd[key] = torch.zeros_like(sd[key])
    return sd


def _grid(v, mode):
    """Spacing of the operand grid at v and the distance of v from the nearest rounding midpoint, both in v's units."""
    s = R.F16_XS if mode == "f16" else 1.0
    mant, lo = (7, -126) if mode == "bf16" else (10, -14)
    x = v.double() * s
    _, e = torch.frexp(torch.where(x != 0, x, torch.ones_like(x)))
    q = torch.exp2(torch.clamp(e.double() - 1, min=lo) - mant)
    mid = (torch.floor(x / q) + 0.5) * q
    return q / s, (x - mid).abs() / s


def _calib(w, b, x, res, dil, pad):
    """e32 of an exact-fp32 GPU ConvPlan on (x, w) against fp64, normalised by A = |conv|(|x|, |w|) + |b| + |res|."""
    y32 = ops.ConvPlan(w, b, dilation=dil, padding=pad, precision=ops.PREC_F32)(x.to(DEV), None if res is None else res.to(DEV)).cpu()
    y64 = _conv64(x, w, b, False, 1, pad, dil) + (0 if res is None else res.double())
    A = _conv64(x.abs(), w.abs(), b.abs(), False, 1, pad, dil) + (0 if res is None else res.double().abs())
    return float(((y32.double() - y64).abs() / A.clamp(min=1e-30)).max())


def _mrf_single_pair(w, h, i, x, mode, fused, variant="rne"):
    """Emulated stage i of a single-pair generator from the library's own stage input x (fp32): (y64, per-element bound).
    variant: "rne" (the contract), "none" (no rounding), "rtz" (truncation), "late_lrelu" (leaky ReLU after rounding the
    intermediate -- the issue's example of a contract violation).  The bound is accumulation noise, calibrated per conv on an
    exact-fp32 GPU plan (4 e32 + 2^-24 of A), plus the effect of every intermediate operand close enough to a rounding midpoint
    that accumulation noise may round it the other way (one grid step through |w2|), plus the fp32 branch sum."""
    nk = len(h["resblock_kernel_sizes"])
    C = int(x.shape[1])
    ys, bnds = [], []
    for j, k in enumerate(h["resblock_kernel_sizes"]):
        d0 = h["resblock_dilation_sizes"][j][0]
        p = f"resblocks.{i * nk + j}."
        w1, b1, w2, b2 = w[p + "convs1.0.weight"], w[p + "convs1.0.bias"], w[p + "convs2.0.weight"], w[p + "convs2.0.bias"]
        red = variant != "none" and mode is not None and R.reduced_layer("rb", C, C, k, fused=fused)
        rtz = variant == "rtz"
        a = F.leaky_relu(x, O.LRELU_SLOPE)
        if red:
            xh = R.round_operand(a, mode, R.F16_XS, rtz)
            w1h = R.round_operand(w1, mode, R.f16_weight_scale(w1) if mode == "f16" else 1.0, rtz)
            w2h = R.round_operand(w2, mode, R.f16_weight_scale(w2) if mode == "f16" else 1.0, rtz)
        else:
            xh, w1h, w2h = a, w1, w2
        pad1, pad2 = d0 * (k - 1) // 2, (k - 1) // 2
        hh = _conv64(xh, w1h, b1, False, 1, pad1, d0)
        Ah = _conv64(xh.abs(), w1h.abs(), b1.abs(), False, 1, pad1, d0)
        hf = hh.float()
        if red and variant == "late_lrelu":
            vh = F.leaky_relu(R.round_operand(hf, mode, R.F16_XS), O.LRELU_SLOPE)
        else:
            v = F.leaky_relu(hf, O.LRELU_SLOPE)
            vh = R.round_operand(v, mode, R.F16_XS, rtz) if red else v
        y = x.double() + _conv64(vh, w2h, b2, False, 1, pad2, 1)
        Ay = x.double().abs() + _conv64(vh.abs(), w2h.abs(), b2.abs(), False, 1, pad2, 1)
        e1 = _calib(w1h, b1, xh, None, d0, pad1)
        e2 = _calib(w2h, b2, vh, x, 1, pad2)
        bnd = (4 * e2 + 2.0 ** -24) * Ay
        if not red:  # (fp32: conv1's accumulation noise reaches the output through |w2|)
            bnd = bnd + _conv64((4 * e1 + 2.0 ** -24) * Ah, w2h.abs(), None, False, 1, pad2, 1)
        if red:
            q, dist = _grid(F.leaky_relu(hh, O.LRELU_SLOPE), mode)
            near = dist <= (4 * e1 + 2.0 ** -24) * Ah + 2.0 ** -23 * hh.abs()
            bnd = bnd + _conv64(torch.where(near, q, torch.zeros_like(q)), w2h.abs(), None, False, 1, pad2, 1)
        ys.append(y)
        bnds.append(bnd)
    y = sum(ys) / nk
    bound = sum(bnds) / nk + 2.0 ** -22 * sum(t.abs() for t in ys) / nk + 2.0 ** -40
    return y, bound


# (case, B, U, stages checked): full_u40 reaches every channel count's pair kernels (per-branch launches) and, at 256 / 128 /
# 64 channels, the layer plans with operand planes; full_b8_u256's 32-channel stage fills the chip twice over
# (B ceil(T / 648) >= 512 workgroups), which voc_forward runs as ONE whole-MRF launch (host_voc_mrf.hip, mrf_split_launch)
# Teeth: bf16 -- 20 x the bound against no rounding, and both truncation and leaky ReLU after the intermediate rounding fail.
# fp16's grid is 8 x finer: far more intermediate operands lie within accumulation noise of a rounding midpoint, and the flip
# allowance for them (one grid step through |w2| each) grows to a few times the rounding effect itself at 256 channels (emulated:
# no-rounding 2.3 x at 256 channels ... 7 x at 32, truncation 8 ... 34 x, leaky-ReLU order 0.2 ... 0.5 x) -- so fp16 asserts that
# the stage is told apart from fp32 and from truncation, and the order of leaky ReLU and rounding is pinned by bf16 (same kernels).
# At 64 ... 256 channels (k = 3 / 7 pair kernels and layer plans) the allowance outgrows the rounding effect in both modes
# (measured at 256 channels: no-rounding 4.2 x bf16, 0.44 x f16), so there the stages are held to (a) only; the teeth are
# asserted on the 32- and 16-channel stages (per-branch pair kernels, the whole-MRF kernel: measured 105 x bf16, 3.4 x f16).
PAIR_TEETH = {"bf16": 20.0, "f16": 1.0}
PAIR_TEETH_MAX_C = 32
PAIR_CASES = [("full_u40", 2, 40, (0, 1, 2, 3, 4)), ("full_b8_u256", 8, 256, (3,))]


@pytest.mark.parametrize("fused", [0, 1, 2])
@pytest.mark.parametrize("case", PAIR_CASES, ids=[c[0] for c in PAIR_CASES])
def test_isolated_resblock_pairs_match_the_rounding_emulation(case, mode, fused):
    name, B, U, check = case
    h = synth.default_voc_config()
    sd = _single_pair_state_dict(h, seed=4321)
    w = O.fold_weight_norm(sd)
    b = synth.synth_voc_batch(B, U, h, seed=77)
    ops.set_default_precision(ops.PREC_NAMES[mode])
    ops.set_fused_resblocks(fused)
    try:
        g = CodeGenerator(AttrDict(h))
        g.load_state_dict(sd)
        g = g.eval().to(DEV)
        st = {}
        g(code=b["code"].to(DEV), spkr=b["spkr"].to(DEV), stages=st)
        torch.cuda.synchronize()
        st = {k: v.cpu() for k, v in st.items()}
        for i in check:
            rows = [0, B - 1]
            x, got = st[f"ups{i}"][rows].contiguous(), st[f"mrf{i}"][rows].double()
            y, bound = _mrf_single_pair(w, h, i, x, mode, fused)
            ratio = float(((got - y).abs() / bound).max())
            C = int(x.shape[1])
            reduced = any(R.reduced_layer("rb", C, C, k, fused=fused) for k in h["resblock_kernel_sizes"])
            rec = dict(test="reduced_pair", case=name, mode=mode, fused=fused, stage=i, C=C, reduced=reduced, ratio=ratio)
            if reduced:
                for variant in ("none", "rtz", "late_lrelu"):
                    yv, _ = _mrf_single_pair(w, h, i, x, mode, fused, variant)
                    rec[variant] = float(((got - yv).abs() / bound).max())
            _report(**rec)
            assert ratio <= 1.0, ("the stage is not the emulation plus accumulation noise", rec)
            if reduced and C <= PAIR_TEETH_MAX_C:  # (teeth: see PAIR_TEETH)
                assert rec["none"] >= PAIR_TEETH[mode], ("the stage cannot see its rounding (or the library ran it in fp32)", rec)
                assert rec["rtz"] > 1.0, ("the test cannot see the rounding mode", rec)
                if mode == "bf16":
                    assert rec["late_lrelu"] > 1.0, ("the test cannot see leaky ReLU applied after the rounding", rec)
    finally:
        ops.set_default_precision(ops.PREC_DEFAULT)
        ops.set_fused_resblocks(2)
