"""GPU: the aligner's training kernels on their own (parrot_debug_tap_gemm / _wgrad / _colsum / _bn_train / _bn_relu_bwd: the launch
code of csrc/host_aligner_train.hip on caller-owned buffers), each against the numpy restatement of
tests/aligner_train_kernels_ref.py, which tests/test_aligner_train_kernels_cpu.py pins against torch.  The parameter sets are the
ones the host builds, at the sizes where a tile, a staging pass, a reduction chunk or an accumulator flush begins or ends.

  * Exact cases: integers in [-4, 4] stored as fp32.  Every product is at most 16 and every sum has at most 2000 terms, so every
    partial and final sum is an integer below 2^24 and every fp32 or fp64 operation on the way is exact in whatever order: the device
    must equal the int64 reference BIT FOR BIT.  Outputs live in buffers longer than needed, pre-filled with a sentinel, and the
    WHOLE buffer is compared: an element the strides do not address still holds the sentinel.
  * Real-valued cases (seeded normals): tap_gemm and wgrad per element within the forward bound of a sum of n products whose adds
    round to nearest, gamma(n + 4) sum |a||x| (+ |bias|), gamma(n) = n u / (1 - n u), u = 2^-24, n the products of that element
    (wgrad: n = min(R, 256), one fp32 chain per chunk, plus half an fp32 ulp of the result for the one rounding of the fp64 sum of the
    chunks).  The + 4: the flush add, tot + acc, the bias add and the bias pair's own add.  The largest observed fraction of the
    bound is printed per kernel (DESIGN.md section 4 records it).  colsum: within 1 fp32 ulp of math.fsum rounded to fp32.
  * A NaN in one operand of tap_gemm turns exactly the elements it is multiplied into to NaN and leaves every other bit alone.
  * The BatchNorm pair: statistics within 1 fp32 ulp of the fp64 value rounded once; the elementwise results against the documented
    fp32 formula evaluated from the DEVICE'S OWN statistics.
The refusals of tests/test_aligner_train_kernels_cpu.py are repeated on real buffers.  The whole file also passes under
PARROT_POISON_WS=nan (the partial-sum workspaces are filled with NaN first)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import aligner_train_kernels_ref as K  # noqa: E402
import test_aligner_train_kernels_cpu as CPU  # noqa: E402  (the refusal tables)
from parrot_tts_amd import _lib, ops  # noqa: E402

DEV = "cuda:0"
SENT, PAD = -7777.0, 37  # (an integer, so the exact references carry it too)
S6 = (2, 9, 24, 112, 144, 13)  # (B, T, n_mels, conv_dim, lstm_dim, V) of aligner_train_ref.SHAPES["S6"]
FRACTIONS = {}  # kernel -> largest |error| / bound seen in the real-valued cases


def _rng(*seed):
    return np.random.Generator(np.random.PCG64(list(seed)))


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _data(rng, n, real, nonzero=False):
    if real:
        v = rng.standard_normal(n).astype(np.float32)
        return np.where(v == 0, np.float32(1), v) if nonzero else v
    return rng.integers(-4, 5, size=n)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same_bits(got, want):
    return np.array_equal(_bits(got), _bits(want))


def _ulp(ref):
    return np.spacing(np.abs(np.asarray(ref, np.float32))).astype(np.float64)


def _note(kernel, frac):
    FRACTIONS[kernel] = max(FRACTIONS.get(kernel, 0.0), float(frac))


# =========================================================================================================================================
# tap_gemm
# =========================================================================================================================================
TG_PATTERNS = [("conv0", lambda M, N, Kk, Z, r: K.tg_conv(M, N, Kk, Z, True, r)), ("conv", lambda M, N, Kk, Z, r: K.tg_conv(M, N, Kk, Z, False, r)),
               ("xproj0", lambda M, N, Kk, Z, r: K.tg_xproj(M, N, Kk, Z, 0)), ("xproj1", lambda M, N, Kk, Z, r: K.tg_xproj(M, N, Kk, Z, 1)),
               ("linear", lambda M, N, Kk, Z, r: K.tg_linear(M, N, Kk, Z)), ("dlstm", lambda M, N, Kk, Z, r: K.tg_dlstm(M, N, Kk, Z)),
               ("dy2", lambda M, N, Kk, Z, r: K.tg_dy2(M, N, Kk, Z)), ("dgrad", lambda M, N, Kk, Z, r: K.tg_dgrad(M, N, Kk, Z))]


def _tg_cases():
    """name -> set.  (1) the seeded sample of (M, N, K) over the tile edges, stride patterns in turn (the sample is 40 long and
    there are 8 patterns: each pattern gets 5 triples), Z 1 or 3, the convs with and without their ReLU; (2) five taps on N = 1, 2, 3
    columns; (3) 8, 9, 16, 17 and 20 staging passes: zero, one and two accumulator flushes, on and just past the flush; (4) every
    launch of the model at S6's sizes (dy2: 36 passes)."""
    cases = {}
    for i, (M, N, Kk) in enumerate(K.sample_triples()):
        name, make = TG_PATTERNS[i % len(TG_PATTERNS)]
        Z, relu = (1, 3)[(i // len(TG_PATTERNS)) % 2], (i // len(TG_PATTERNS) + i) % 2
        cases[f"{name}-{M}x{N}x{Kk}-z{Z}" + ("-relu" if relu and name.startswith("conv") else "")] = make(M, N, Kk, Z, relu)
    for N in (1, 2, 3):
        cases[f"conv0-5taps-n{N}"] = K.tg_conv(33, N, 40, 3, True)
        cases[f"conv-5taps-n{N}"] = K.tg_conv(33, N, 40, 3, False, relu=0)
        cases[f"dgrad-5taps-n{N}"] = K.tg_dgrad(33, N, 40, 3)
    for n_pass, p in ((8, K.tg_linear(33, 70, 256, 1)), (9, K.tg_linear(33, 70, 272, 1)), (16, K.tg_dy2(33, 70, 256, 1)),
                      (17, K.tg_dlstm(33, 70, 520, 1)), (20, K.tg_conv(33, 70, 112, 1, False))):
        assert K.passes(p) == n_pass
        cases[f"passes{n_pass}"] = p
    for name, p in K.host_tap_gemm_sets(*S6).items():
        cases[f"S6-{name}"] = p
    for p in cases.values():
        assert p["ntaps"] * p["K"] <= 2000
    return cases


TG_CASES = _tg_cases()


def _tg_inputs(p, seed, real, nonzero=False):
    rng = _rng(11, seed, int(real))
    A, X = _data(rng, p["a_size"], real, nonzero), _data(rng, p["x_size"], real, nonzero)
    b0 = _data(rng, p["M"], real) if p["bias"] >= 1 else None
    b1 = _data(rng, p["M"], real) if p["bias"] == 2 else None
    return A, X, b0, b1


def _tg_index(p):
    """Flat index into C of every (z, m, n) the set addresses."""
    z, m, n = np.arange(p["Z"]), np.arange(p["M"]), np.arange(p["N"])
    return p["c_base"] + z[:, None, None] * p["c_sz"] + m[None, :, None] * p["c_sm"] + n[None, None, :] * p["c_sn"]


def _tg_run(p, A, X, b0, b1):
    c = torch.full((p["c_size"] + PAD,), SENT, dtype=torch.float32, device=DEV)
    ops.debug_tap_gemm(p, _dev(A), _dev(X), c, _dev(b0), _dev(b1))
    return c.cpu().numpy()


@pytest.mark.parametrize("name", list(TG_CASES))
def test_tap_gemm_exact(name):
    p = TG_CASES[name]
    A, X, b0, b1 = _tg_inputs(p, sorted(TG_CASES).index(name), False)
    want = K.tap_gemm(p, A, X, np.full(p["c_size"] + PAD, int(SENT), np.int64), b0, b1)
    assert np.abs(want).max() < 2 ** 24
    idx = _tg_index(p)
    assert np.unique(idx).size == idx.size
    if p["relu"] and idx.size >= 8:  # negative sums are there for the ReLU to act on
        pre = K.tap_gemm(dict(p, relu=0), A, X, np.zeros(p["c_size"] + PAD, np.int64), b0, b1)[idx]
        assert (pre < 0).any() and (want[idx] >= 0).all()
    got = _tg_run(p, A, X, b0, b1)
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, (name, bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("name", list(TG_CASES))
def test_tap_gemm_real_within_the_forward_bound(name):
    p = TG_CASES[name]
    A, X, b0, b1 = _tg_inputs(p, sorted(TG_CASES).index(name), True)
    init = np.full(p["c_size"] + PAD, SENT, np.float64)
    want, mag, cnt = K.tap_gemm(p, A, X, init, b0, b1, want_bound=True)
    got = _tg_run(p, A, X, b0, b1).astype(np.float64)
    idx = _tg_index(p)
    rest = np.ones(got.shape, bool)
    rest[idx] = False
    assert (got[rest] == SENT).all()  # sentinels
    bound = K.gamma_n(cnt + 4)[None, None, :] * mag
    err = np.abs(got[idx] - want[idx])
    frac = float((err / np.where(bound > 0, bound, 1.0))[bound > 0].max()) if (bound > 0).any() else 0.0
    print(f"tap_gemm {name}: largest |err| / bound = {frac:.4f}")
    _note("tap_gemm", frac)
    assert np.isfinite(got[idx]).all() and (err <= bound).all(), (name, frac)


NAN_SPOTS = {"first tile": dict(m0=0, k0=0, n0=0, z0=0, j0=1), "last, partial tile": dict(m0=32, k0=39, n0=69, z0=1, j0=4)}


@pytest.mark.parametrize("spot", list(NAN_SPOTS))
@pytest.mark.parametrize("first", [False, True], ids=["conv", "conv0"])
def test_tap_gemm_confines_a_nan(first, spot):
    """Partial tiles in every direction (M = 33, N = 70, K = 40), five taps, ReLU on, no zero in A or X.  A NaN in A_j[m0][k0]: exactly
    row m0 of every batch row is NaN (under a side tap that falls outside the NaN meets the zero that stands for the padding: NaN
    as well, so the whole row).  A NaN in X[z0][k0][n0]: exactly the columns n0 - shift_j inside [0, N) of batch row z0, every m.
    Everything else, sentinels included, has the bits of the run without the NaN: rows m >= M, columns n >= N and k >= K are
    staged as zeros on both sides, so no NaN leaks through the padding of a tile."""
    s = NAN_SPOTS[spot]
    p = K.tg_conv(33, 70, 40, 2, first, relu=1)
    A, X, _, _ = _tg_inputs(p, 99, True, nonzero=True)
    clean = _tg_run(p, A, X, None, None)
    assert np.isfinite(clean).all()
    idx = _tg_index(p)
    # in A
    A2 = A.copy()
    A2[p["a_off"][s["j0"]] + s["m0"] * p["a_sm"] + s["k0"] * p["a_sk"]] = np.nan
    got = _tg_run(p, A2, X, None, None)
    want_nan = np.zeros(got.shape, bool)
    want_nan[idx[:, s["m0"], :]] = True
    assert np.array_equal(np.isnan(got), want_nan)
    assert np.array_equal(_bits(got)[~want_nan], _bits(clean)[~want_nan])
    # in X
    X2 = X.copy()
    X2[p["x_base"] + s["z0"] * p["x_sz"] + s["k0"] * p["x_sk"] + s["n0"] * p["x_sn"]] = np.nan
    got = _tg_run(p, A, X2, None, None)
    cols = sorted({s["n0"] - sh for sh in p["shift"] if 0 <= s["n0"] - sh < 70})
    assert 3 <= len(cols) <= 5
    want_nan = np.zeros(got.shape, bool)
    want_nan[idx[s["z0"]][:, cols]] = True
    assert np.array_equal(np.isnan(got), want_nan)
    assert np.array_equal(_bits(got)[~want_nan], _bits(clean)[~want_nan])


# =========================================================================================================================================
# wgrad
# =========================================================================================================================================
WG_PATTERNS = [("linear", lambda M, Kk, B, T: K.wg_linear(M, Kk, B, T)), ("w_ih0", lambda M, Kk, B, T: K.wg_w_ih(M, Kk, B, T, 0)),
               ("w_ih1", lambda M, Kk, B, T: K.wg_w_ih(M, Kk, B, T, 1)), ("w_hh0", lambda M, Kk, B, T: K.wg_w_hh(M, Kk, B, T, 0)),
               ("w_hh1", lambda M, Kk, B, T: K.wg_w_hh(M, Kk, B, T, 1)), ("conv0", lambda M, Kk, B, T: K.wg_conv(M, Kk, B, T, True)),
               ("conv", lambda M, Kk, B, T: K.wg_conv(M, Kk, B, T, False))]
WG_BT = [(1, 1), (3, 85), (4, 64), (1, 257), (3, 200)]  # R = 1, 255, 256, 257, 600; (3, 200): chunks end at t = 56 of row 1 and t = 112 of row 2
WG_SIZES = (1, 33, 65, 130)


def _wg_cases():
    """Every pattern on every (B, T), (M, K) running through a seeded order of the 16 pairs of WG_SIZES (35 cases: each pair at
    least twice); T = 1 under five taps; every launch of the model at S6's sizes."""
    cases = {}
    pairs = [(a, b) for a in WG_SIZES for b in WG_SIZES]
    order = _rng(5).permutation(len(pairs))
    i = 0
    for B, T in WG_BT:
        for name, make in WG_PATTERNS:
            M, Kk = pairs[order[i % len(pairs)]]
            i += 1
            cases[f"{name}-{M}x{Kk}-b{B}t{T}"] = make(M, Kk, B, T)
    cases["conv0-5taps-t1"] = K.wg_conv(33, 65, 3, 1, True)
    cases["conv-5taps-t1"] = K.wg_conv(65, 33, 3, 1, False)
    for name, p in K.host_wgrad_sets(*S6).items():
        cases[f"S6-{name}"] = p
    for p in cases.values():
        assert p["R"] <= 2000
    return cases


WG_CASES = _wg_cases()


def _wg_run(p, dY, X):
    out = torch.full((p["o_size"] + PAD,), SENT, dtype=torch.float32, device=DEV)
    ops.debug_wgrad(p, _dev(dY), _dev(X), out)
    return out.cpu().numpy()


@pytest.mark.parametrize("name", list(WG_CASES))
def test_wgrad_exact(name):
    p = WG_CASES[name]
    rng = _rng(12, sorted(WG_CASES).index(name))
    dY, X = _data(rng, p["y_size"], False), _data(rng, p["x_size"], False)
    want = K.wgrad(p, dY, X, np.full(p["o_size"] + PAD, int(SENT), np.int64))
    assert np.abs(want).max() < 2 ** 24
    got = _wg_run(p, dY, X)
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, (name, bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("name", list(WG_CASES))
def test_wgrad_real_within_the_forward_bound(name):
    p = WG_CASES[name]
    rng = _rng(13, sorted(WG_CASES).index(name))
    dY, X = _data(rng, p["y_size"], True), _data(rng, p["x_size"], True)
    want, mags = K.wgrad(p, dY, X, np.full(p["o_size"] + PAD, SENT, np.float64), want_bound=True)
    got = _wg_run(p, dY, X).astype(np.float64)
    m, k = np.arange(p["M"]), np.arange(p["K"])
    seen = np.zeros(got.shape, bool)
    frac = 0.0
    for j in range(p["ntaps"]):
        idx = m[:, None] * p["o_sm"] + k[None, :] * p["o_sk"] + j * p["o_sj"]
        seen[idx] = True
        bound = K.gamma_n(min(p["R"], K.RCHUNK) + 4) * mags[j] + 0.5 * _ulp(want[idx])
        err = np.abs(got[idx] - want[idx])
        assert np.isfinite(got[idx]).all() and (err <= bound).all(), (name, j, float((err / bound).max()))
        frac = max(frac, float((err / bound).max()))
    assert np.array_equal(got[~seen], want[~seen])  # sentinels
    print(f"wgrad {name}: largest |err| / bound = {frac:.4f}")
    _note("wgrad", frac)


# =========================================================================================================================================
# colsum
# =========================================================================================================================================
@pytest.mark.parametrize("M", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("R", [1, 255, 256, 257, 1000])
def test_colsum(R, M):
    """Dense rows (ld = M) and the second half of rows twice as wide (ld = 2 M, offset M: the bias gradient of one direction out of
    dgates), on integer data exactly and on normals within 1 fp32 ulp of math.fsum rounded to fp32 (the device's own fp64 sum is off
    by less than R 2^-53 of sum |x|, which can move a result only where it sits on a rounding tie).  out1, when given, has
    out0's bits."""
    for ld, base, second in ((M, 0, False), (2 * M, M, True)):
        for real in (False, True):
            src = _data(_rng(14, R, M, ld, int(real)), R * ld, real)
            outs = [torch.full((M + PAD,), SENT, dtype=torch.float32, device=DEV) for _ in range(2)]
            ops.debug_colsum(_dev(src), R, M, ld, outs[0], outs[1] if second else None, base=base)
            got0, got1 = (o.cpu().numpy() for o in outs)
            assert (got0[M:] == SENT).all() and (got1[M if second else 0:] == SENT).all()
            if second:
                assert _same_bits(got0, got1)
            want = K.colsum(src, R, M, ld, base)
            if real:
                w32 = want.astype(np.float32)
                assert (np.abs(got0[:M].astype(np.float64) - w32) <= _ulp(w32)).all()
                _note("colsum (ulps)", float((np.abs(got0[:M].astype(np.float64) - w32) / _ulp(w32)).max()))
            else:
                assert _same_bits(got0[:M], want)


# =========================================================================================================================================
# BatchNorm forward and backward
# =========================================================================================================================================
BN_BT = [(2, 1), (3, 85), (4, 64), (257, 1), (5, 200)]  # n = B T = 2, 255, 256, 257, 1000
EPS = 1e-5
CONST = np.float32(0.3)


def _bn_inputs(B, T, seed=0):
    """x (B, 3, T): channel 0 a ReLU's output (exact zeros), channel 1 constant, channel 2 mean 1e4 and deviation 1e-2 (a variance
    formed in one pass, E x^2 - mean^2, would lose every digit there)."""
    rng = _rng(15, B, T, seed)
    x = np.empty((B, 3, T), np.float32)
    x[:, 0] = np.maximum(rng.standard_normal((B, T)), 0).astype(np.float32)
    x[:, 1] = CONST
    x[:, 2] = (1e4 + 1e-2 * rng.standard_normal((B, T))).astype(np.float32)
    gamma, beta = rng.standard_normal(3).astype(np.float32), rng.standard_normal(3).astype(np.float32)
    rm, rv = rng.standard_normal(3).astype(np.float32), rng.uniform(0.5, 2.0, 3).astype(np.float32)
    return x, gamma, beta, rm, rv


def _bn_run(x, gamma, beta, rm, rv, training):
    B, _, T = x.shape
    y = torch.full((x.size + PAD,), SENT, dtype=torch.float32, device=DEV)
    st = {k: torch.full((3 + PAD,), SENT, dtype=torch.float32, device=DEV) for k in ("mean", "invstd", "run_mean", "run_var")}
    st["run_mean"][:3], st["run_var"][:3] = _dev(rm), _dev(rv)
    ops.debug_bn_train(_dev(x), y, _dev(gamma), _dev(beta), st["run_mean"], st["run_var"], st["mean"], st["invstd"], training, EPS)
    out = {k: v.cpu().numpy() for k, v in st.items()}
    out["y"] = y.cpu().numpy()
    for k, v in out.items():
        n = x.size if k == "y" else 3
        assert (v[n:] == SENT).all(), k
        out[k] = v[:n].reshape(x.shape) if k == "y" else v[:n]
    return out


def _within_ulps(got, ref, ulps=1):
    ref = np.asarray(ref, np.float32)
    return bool((np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= ulps * _ulp(ref)).all())


@pytest.mark.parametrize("B, T", BN_BT)
def test_bn_train(B, T):
    x, gamma, beta, rm, rv = _bn_inputs(B, T)
    got = _bn_run(x, gamma, beta, rm, rv, True)
    mean, invstd, rm1, rv1 = K.bn_stats(x, rm, rv, EPS)
    for k, ref in (("mean", mean), ("invstd", invstd), ("run_mean", rm1), ("run_var", rv1)):
        assert _within_ulps(got[k], ref), (k, got[k], ref)
    # y from the device's own statistics: the fma emulated in fp64 is a double rounding, 1 ulp
    assert _within_ulps(got["y"], K.bn_apply(x, got["mean"], got["invstd"], gamma, beta))
    # the constant channel: sums of n <= 1000 copies of a 24-bit number are exact in fp64, so the mean is the constant itself,
    # every deviation is 0, and y = fma(0, gamma, beta) = beta
    assert _same_bits(got["mean"][1], CONST) and _same_bits(got["invstd"][1], np.float32(1.0 / np.sqrt(np.float64(np.float32(EPS)))))
    assert _same_bits(got["y"][:, 1], np.full((B, T), beta[1]))
    # the running statistics instead: no buffer changes, y comes from them
    ev = _bn_run(x, gamma, beta, rm, rv, False)
    assert _same_bits(ev["run_mean"], rm) and _same_bits(ev["run_var"], rv) and _same_bits(ev["mean"], rm)
    assert _within_ulps(ev["invstd"], K.bn_eval_stats(rm, rv, EPS)[1])
    assert _within_ulps(ev["y"], K.bn_apply(x, ev["mean"], ev["invstd"], gamma, beta))
    # a NaN in channel 0 stays in channel 0
    bad = x.copy()
    bad[B // 2, 0, T // 2] = np.nan
    nn = _bn_run(bad, gamma, beta, rm, rv, True)
    for k in got:
        assert np.isnan(nn[k][:, 0] if k == "y" else nn[k][0]).all(), k
        assert _same_bits(nn[k][:, 1:] if k == "y" else nn[k][1:], got[k][:, 1:] if k == "y" else got[k][1:]), k


def _bwd_run(dy, x, gamma, mean, invstd, alias=False, sums=True):
    B, _, T = x.shape
    t = {k: _dev(v) for k, v in dict(dy=dy, x=x, gamma=gamma, mean=mean, invstd=invstd).items()}
    dx = t["dy"] if alias else torch.full((x.size + PAD,), SENT, dtype=torch.float32, device=DEV)
    dg, db = (torch.full((3 + PAD,), SENT, dtype=torch.float32, device=DEV) for _ in range(2))
    d = _lib.DebugBnBwdDesc(*[ops.debug_buf(t[k]) for k in ("dy", "x")], ops.debug_buf(dx), *[ops.debug_buf(t[k]) for k in ("gamma", "mean", "invstd")],
                            ops.debug_buf(dg if sums else None), ops.debug_buf(db if sums else None), B, 3, T)
    with torch.cuda.device(DEV):
        _lib.check(_lib.lib().parrot_debug_bn_relu_bwd(C.byref(d), ops.stream_ptr(DEV)))
    dxn, dgn, dbn = dx.cpu().numpy().ravel(), dg.cpu().numpy(), db.cpu().numpy()
    assert (dxn[x.size:] == SENT).all() and (dgn[3 if sums else 0:] == SENT).all() and (dbn[3 if sums else 0:] == SENT).all()
    return dxn[:x.size].reshape(x.shape), dgn[:3], dbn[:3]


@pytest.mark.parametrize("B, T", BN_BT)
def test_bn_relu_bwd(B, T):
    """dbeta and dgamma: within 1 fp32 ulp of the fp64 sums (xh formed in fp32 single operations, as the kernel documents).

    dx = (gamma invstd) ((dy - m1) - xh m2) is a chain of single fp32 operations on m1 = fl32(s1 / n), m2 = fl32(s2 / n), where
    s1, s2 are the device's fp64 sums; the device stores dbeta = fl32(s1), dgamma = fl32(s2).  From those, m1' = fl32(dbeta / n):
    dbeta is within 2^-24 relative of s1, that is within one fp32 ulp of m1's magnitude, so the two roundings m1 and m1' are equal
    or neighbours (likewise m2).  Given m1 and m2 every further operation is determined, so the allowance is that one ulp on m1
    and on m2 and nothing else: per channel, dx must equal BIT FOR BIT the formula evaluated with some (m1, m2) out of the 3 x 3
    neighbours of (m1', m2') -- one pair for the whole channel."""
    n = B * T
    rng = _rng(16, B, T)
    x = np.maximum(rng.standard_normal((B, 3, T)), 0).astype(np.float32)
    assert (x == 0).any()
    dy = rng.standard_normal((B, 3, T)).astype(np.float32)
    gamma = rng.standard_normal(3).astype(np.float32)
    mean, invstd, _, _ = K.bn_stats(x, np.zeros(3, np.float32), np.ones(3, np.float32), EPS)
    dx, dgamma, dbeta = _bwd_run(dy, x, gamma, mean, invstd)
    s1, s2 = K.bn_bwd_sums(dy, x, mean, invstd)
    assert _within_ulps(dbeta, s1.astype(np.float32)) and _within_ulps(dgamma, s2.astype(np.float32))
    m1, m2 = ((v.astype(np.float64) / n).astype(np.float32) for v in (dbeta, dgamma))
    for c in range(3):
        cands = [(a, b) for a in (m1[c], np.nextafter(m1[c], np.float32(-np.inf)), np.nextafter(m1[c], np.float32(np.inf)))
                 for b in (m2[c], np.nextafter(m2[c], np.float32(-np.inf)), np.nextafter(m2[c], np.float32(np.inf)))]
        hits = [i for i, (a, b) in enumerate(cands)
                if _same_bits(dx[:, c], K.bn_bwd_apply(dy, x, gamma, mean, invstd, np.full(3, a), np.full(3, b))[:, c])]
        print(f"bn_relu_bwd n = {n} channel {c}: (m1, m2) candidates that reproduce dx bit for bit: {hits} (0 = the central pair)")
        assert hits, (c, m1[c], m2[c])
    assert (_bits(dx)[x == 0] == 0).all()  # +0.0 wherever the ReLU was off
    aliased, dg2, db2 = _bwd_run(dy, x, gamma, mean, invstd, alias=True)
    assert _same_bits(aliased, dx) and _same_bits(dg2, dgamma) and _same_bits(db2, dbeta)
    assert _same_bits(_bwd_run(dy, x, gamma, mean, invstd, sums=False)[0], dx)


# =========================================================================================================================================
# refusals, on real buffers: the tables of the CPU test.  Nothing is launched, so every buffer keeps its fill.
# =========================================================================================================================================
class _Real:
    def __init__(self):
        self.t = []

    def __call__(self, name, n):
        if n is None:
            return _lib.DebugBuf(None, 0)
        self.t.append(torch.full((max(int(n), 1),), SENT, dtype=torch.float32, device=DEV))
        return _lib.DebugBuf(self.t[-1].data_ptr(), n)

    def intact(self):
        torch.cuda.synchronize()
        return all(bool((t == SENT).all()) for t in self.t)


def test_refusals_on_real_buffers():
    lib = _lib.lib()
    for name, p, over, code in CPU.tap_gemm_refusals():
        mk = _Real()
        assert CPU.call_tap_gemm(lib, mk, p, over) == code and mk.intact(), name
    for name, p, over, code in CPU.wgrad_refusals():
        mk = _Real()
        assert CPU.call_wgrad(lib, mk, p, over) == code and mk.intact(), name
    for case in CPU.colsum_refusals():
        mk = _Real()
        assert CPU.call_colsum(lib, mk, *case[1:-1]) == case[-1] and mk.intact(), case[0]
    for case in CPU.bn_refusals():
        mk = _Real()
        assert CPU.call_bn(lib, mk, *case[1:-1]) == case[-1] and mk.intact(), case[0]


def test_report_fractions():
    for k in sorted(FRACTIONS):
        print(f"largest over this run, {k}: {FRACTIONS[k]:.4f}")
    if FRACTIONS:  # (empty when this test is selected alone)
        assert FRACTIONS.get("tap_gemm", 0.0) <= 1.0 and FRACTIONS.get("wgrad", 0.0) <= 1.0


def test_whole_file_under_poison():
    """This file once more in a child process under PARROT_POISON_WS=nan: a partial sum nobody wrote would turn a result into NaN."""
    if os.environ.get("PARROT_POISON_WS"):
        return  # (already a poisoned run: the tests above were it)
    env = dict(os.environ, PARROT_POISON_WS="nan")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", os.path.abspath(__file__), "-k", "not whole_file"], cwd=ROOT,
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
