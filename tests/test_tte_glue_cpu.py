"""CPU: the numpy restatements of tests/tte_glue_ref.py pinned against torch and the oracle, and the input design of
tests/test_gpu_tte_glue.py (the share of each seeded duration input inside the rounding band).  No library call, no GPU."""
import os
import sys
from fractions import Fraction

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tte_glue_ref as R  # noqa: E402
from oracle import parrot_oracle as O  # noqa: E402


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


# ---- durations -------------------------------------------------------------------------------------------------------------------------
def test_durations64_is_torch_round_and_clamp_in_fp64():
    v = np.concatenate([_rng(1).uniform(-3, 4.5, 5000), [-np.inf, 0.0, -0.0, np.log(1.5), np.log(2.5), np.log(3.5), 10.0, 22.18071, 43.0]])
    t = torch.from_numpy(v)
    want = torch.clamp(torch.round(torch.exp(t) - 1), min=0).to(torch.int64).numpy()
    assert np.array_equal(R.durations64(v), want)
    # half to even at exact halves; NaN -> 0; beyond int64 -> INT64_MAX; fp32 input is widened, not re-rounded
    assert np.rint(np.array([0.5, 1.5, 2.5])).tolist() == [0.0, 2.0, 2.0] and torch.round(torch.tensor([0.5, 1.5, 2.5])).tolist() == [0.0, 2.0, 2.0]
    assert R.durations64(np.array([np.nan, 60.0, np.inf], dtype=np.float32)).tolist() == [0, 2 ** 63 - 1, 2 ** 63 - 1]
    v32 = np.float32(22.18071)
    assert R.durations64(np.array([v32]))[0] == int(np.rint(np.exp(np.float64(v32)) - 1.0))


def test_fp32_durations_agree_with_fp64_outside_the_band():
    """The project's rule (tests/test_gpu_parity.py): the reference's fp32 arithmetic rounds as fp64 does wherever exp(v) - 1 is at
    least 1e-4 from k + 0.5.  Held here for the CPU's fp32 on every seeded input of the GPU file, and the band share recorded."""
    shares = {}
    for S in R.DUR_S:
        for mode in R.DUR_MODES:
            v, valid, src_len = R.duration_case(S, mode)
            ld, real = R.masked_log_dur(v, valid, src_len)
            band = R.in_band(ld)
            shares[(S, mode)] = float(band.mean())
            assert band.mean() <= 0.01, (S, mode, band.mean())
            d32 = O.durations_from_log(torch.from_numpy(ld)).numpy()
            ok, _ = R.durations_match(d32, ld)
            assert ok.all(), (S, mode)
            assert np.array_equal(d32[~band], R.durations64(ld)[~band])
            # the specials sit where the docstring says
            if S >= 6:
                assert np.isneginf(v[real]).any() and np.isneginf(v[~real]).any()
                assert (np.signbit(v) & (v == 0)).sum() == 2
            if mode == "src_len":
                assert src_len.tolist() == [S, 0, S // 2]
    draws = np.concatenate([R.duration_case(S, m)[0].ravel() for S in R.DUR_S for m in R.DUR_MODES])
    print("band share per case: max %.2e; over all %d draws: %.2e" % (max(shares.values()), draws.size, float(R.in_band(draws).mean())))
    assert R.in_band(draws).mean() <= 0.01


def test_faithful_durations_bracket_every_fp32_evaluation():
    """Beyond exp(v) ~ 2^24 the fp32 grid is coarser than 1: an fp32 evaluation returns rint(e - 1) for e one of the two fp32
    neighbours of exp64(v).  The CPU's own fp32 exp, evaluated element by element and as one array (its scalar and vector code
    paths), stays inside that pair -- and the two need not agree with each other."""
    v = np.concatenate([_rng(3).uniform(10, 43, 4000), [22.18071, np.log(2.0 ** 31 + 1)]]).astype(np.float32)
    lo, hi = R.faithful_durations(v)
    assert (hi >= lo).all() and (hi - lo <= np.maximum(np.exp(v.astype(np.float64)) * 2.0 ** -22, 1)).all()  # (a grid step, two across a binade edge)
    whole = O.durations_from_log(torch.from_numpy(v)).numpy()
    alone = np.array([int(O.durations_from_log(torch.from_numpy(v[i:i + 1]))[0]) for i in range(len(v))])
    for d in (whole, alone):
        assert ((d == lo) | (d == hi)).all()
    assert R.faithful_durations(np.array([22.18071], dtype=np.float32))[0][0] == 2 ** 32
    assert R.faithful_durations(np.array([22.18071], dtype=np.float32))[1][0] == 2 ** 32 + 512
    small = _rng(4).uniform(-3, 4.5, 2000).astype(np.float32)
    lo, hi = R.faithful_durations(small)
    ok, _ = R.durations_match(lo, small)
    assert ok.all() and R.durations_match(hi, small)[0].all()


def test_in_band_marks_the_boundaries():
    k = np.arange(0, 60, dtype=np.float64)
    assert R.in_band(np.log(k + 1.5)).all() and R.in_band(np.log(k + 1.5 + 5e-5)).all()
    assert not R.in_band(np.log(k + 1.5 + 2e-4)).any() and not R.in_band(np.log(k + 1.25)).any()
    assert not R.in_band(np.array([-np.inf, np.nan, np.inf, -3.0, np.log(0.5)])).any()
    ok, band = R.durations_match(np.array([1, 2, 0, 3]), np.log(np.array([2.5, 2.5, 2.5, 3.0 + 1.0])))
    assert band.tolist() == [True, True, True, False] and ok.tolist() == [True, True, False, True]


def test_masked_log_dur_keeps_bits_and_zeroes_pads():
    v = np.array([[np.nan, -0.0, 3.0, np.inf]], dtype=np.float32)
    ld, real = R.masked_log_dur(v, np.array([[1, 255, 0, 0]], dtype=np.uint8))
    assert real.tolist() == [[True, True, False, False]]
    assert ld.view(np.int32).tolist() == [[v.view(np.int32)[0, 0], v.view(np.int32)[0, 1], 0, 0]]
    ld, real = R.masked_log_dur(v, None, np.array([3], dtype=np.int32))
    assert real.tolist() == [[True, True, True, False]] and ld[0, 3] == 0 and ld[0, 2] == 3


# ---- prefix sums and the length regulator ---------------------------------------------------------------------------------------------
def test_length_regulate_is_repeat_interleave_with_both_mask_rules():
    rng = _rng(5)
    for S, D in [(1, 1), (7, 3), (129, 5), (300, 4)]:
        B = 3
        dur = rng.choice(np.array([0, 0, 1, 2, 7]), size=(B, S)).astype(np.int64)
        dur[0, 0] = max(dur[0, 0], 1)
        dur[1, : S // 3] = 0
        dur[2, S // 2:] = 0
        seq = rng.standard_normal((B, S, D)).astype(np.float32)  # channel-last, as the oracle takes it
        exp, mask, lens = O.length_regulator(torch.from_numpy(seq), torch.from_numpy(dur))
        L = exp.shape[1]
        pe = np.zeros((L + 2, D), dtype=np.float32)
        y, m, cum, out_len, status = R.length_regulate(seq.transpose(0, 2, 1), dur, pe, L)
        assert not status and out_len.tolist() == lens
        assert np.array_equal(cum, np.cumsum(dur, axis=1).astype(np.int32))
        assert np.array_equal(y.transpose(0, 2, 1), exp.numpy()) and np.array_equal(m.astype(bool), mask.numpy())
        for b in range(B):  # ... and row by row against repeat_interleave itself
            want = torch.from_numpy(seq[b]).repeat_interleave(torch.from_numpy(dur[b]), dim=0).numpy()
            assert np.array_equal(y[b].T[: lens[b]], want) and not y[b].T[lens[b]:].any()
        # a non-zero positional row: one fp32 add; row-exact: the row's own pe[len] and exactly max(len, 1) keys
        pe = rng.standard_normal((L + 2, D)).astype(np.float32)
        y2, _, _, _, _ = R.length_regulate(seq.transpose(0, 2, 1), dur, pe, L)
        assert np.array_equal(y2, y + pe[L][None, :, None])
        y3, m3, _, _, _ = R.length_regulate(seq.transpose(0, 2, 1), dur, pe, L, row_exact=True)
        for b in range(B):
            assert np.array_equal(y3[b], y[b] + pe[lens[b]][:, None])
            assert m3[b].tolist() == [1 if t < max(lens[b], 1) else 0 for t in range(L)]


def test_sat_prefix_saturates_and_flags():
    cum, out_len, st = R.sat_prefix(np.array([[1, 2 ** 31, 5], [2 ** 40, 0, 1], [3, -4, 2]], dtype=np.int64))
    assert cum.tolist() == [[1, R.INT32_MAX, R.INT32_MAX], [R.INT32_MAX] * 3, [3, 3, 5]]
    assert out_len.tolist() == [R.INT32_MAX, R.INT32_MAX, 5] and st == {R.ST_NEGATIVE}
    cum, out_len, st = R.sat_prefix(np.array([[1, 2, 3]], dtype=np.int64), np.array([2], dtype=np.int32))
    assert cum.tolist() == [[1, 3, 3]] and out_len.tolist() == [3] and st == {R.ST_PADDED}
    assert R.sat_prefix(np.array([[1, 2, 0]], dtype=np.int64), np.array([2], dtype=np.int32))[2] == set()


# ---- argmax and the guard -------------------------------------------------------------------------------------------------------------
def test_argmax_guard_is_torch_argmax_and_topk():
    rng = _rng(9)
    for V in (1, 2, 15, 17, 33, 1000):
        x = rng.standard_normal((2, V, 40)).astype(np.float32)
        x = np.round(x * 4) / 4  # coarse values: duplicates of the maximum occur by themselves
        if V >= 2:
            x[0, :, 0] = 1.0                         # all equal
            x[0, 0, 1], x[0, 1, 1] = -0.0, 0.0       # signed zeros tie
            x[0, 2:, 1] = -1.0
        r = R.argmax_guard(x, 2.0 ** -13, row0=3)
        t = torch.from_numpy(x)
        # first maximum: torch.argmax picks one maximal index, the FIRST is what the kernel documents -- take it from the values
        first = (t == t.max(dim=1, keepdim=True).values).to(torch.int8).argmax(dim=1)
        assert np.array_equal(r["ids"], first.numpy())
        assert bool((t.gather(1, torch.argmax(t, 1, keepdim=True)) == t.gather(1, first[:, None])).all())
        if V >= 2:
            top = torch.topk(t, 2, dim=1).values
            assert np.array_equal(r["margin"], (top[:, 0] - top[:, 1]).numpy())
            assert r["margin"][0, 0] == 0 and r["margin"][0, 1] == 0 and r["ids"][0, 0] == 0 and r["ids"][0, 1] == 0
        else:
            assert np.isposinf(r["margin"]).all()
        want = {(3 + b, tt) for b in range(2) for tt in range(40) if not r["margin"][b, tt] >= 2.0 ** -13}
        assert r["guarded"] == want and r["count"] == len(want)
        assert r["min_bits"] == int(r["margin"].view(np.int32).min())
    # the threshold itself is not guarded; non-finite columns are, whatever their margin
    x = np.zeros((1, 4, 5), dtype=np.float32)
    x[0, 0] = [1.0, 1.0, np.inf, -np.inf, 1.0]
    x[0, 1] = [1.0 - 2.0 ** -13, 1.0 - 2.0 ** -14, 0.0, -np.inf, np.nan]
    x[0, 2:, 3] = -np.inf
    r = R.argmax_guard(x, 2.0 ** -13)
    assert r["margin"][0, 0] == np.float32(2.0 ** -13) and r["margin"][0, 1] == np.float32(2.0 ** -14)
    assert r["guarded"] == {(0, 1), (0, 2), (0, 3), (0, 4)} and r["nonfinite"][0].tolist() == [False, False, True, True, True]
    assert [R.wave_ranges(V)[:3] for V in (1, 17, 33)] == [[(0, 1), (1, 1), (1, 1)], [(0, 2), (2, 4), (4, 6)], [(0, 3), (3, 6), (6, 9)]]
    assert R.wave_ranges(17)[8:10] == [(16, 17), (17, 17)]


# ---- the fp64 re-evaluation -------------------------------------------------------------------------------------------------------------
def _fma_exact(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))  # (Fraction -> float rounds to nearest even, once)


def test_fma64_rounds_once():
    rng = _rng(2)
    n = 3000
    a = rng.standard_normal(n).astype(np.float32).astype(np.float64)
    b = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)
    c = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)
    c[::3] = -(a[::3] * b[::3])            # cancellation: the result is the product's rounding error
    c[1::7] = 0.0
    b[2::11] = np.ldexp(1.0 + 2.0 ** -30, rng.integers(-5, 5, len(b[2::11])))
    got = R.fma64(a, b, c)
    want = np.array([_fma_exact(x, y, z) for x, y, z in zip(a, b, c)])
    assert np.array_equal(got, want)
    assert (got != a * b + c).any()        # ... which a product rounded first does not give
    # halfway cases of the final rounding: a b = 1 + 2^-53 exactly (a tie without c, broken by a tiny c)
    a1, b1 = np.float64(1.0 + 2.0 ** -26), np.float64(1.0 + 2.0 ** -27)
    for cc in (0.0, 2.0 ** -90, -2.0 ** -90, 2.0 ** -53, -2.0 ** -53):
        assert R.fma64(a1, b1, cc) == _fma_exact(a1, b1, cc), cc
    # fp32-valued operands: the product is exact and fma is `a b + c`
    x = rng.standard_normal(n).astype(np.float32).astype(np.float64)
    assert np.array_equal(R.fma64(a, x, c), a * x + c)


def test_refine64_is_the_sequential_fp64_loop():
    rng = _rng(4)
    B, D, V, L, F = 2, 9, 7, 5, 11
    x, h = (rng.standard_normal((B, D, L)).astype(np.float32) for _ in range(2))
    f = np.maximum(rng.standard_normal((B, F, L)), 0).astype(np.float32)
    hwt, w2t = rng.standard_normal((D, V)).astype(np.float32), rng.standard_normal((F, D)).astype(np.float32)
    hb, b2 = rng.standard_normal(V).astype(np.float32), rng.standard_normal(D).astype(np.float32)
    pos = [(1, 4), (0, 0), (1, 2)]
    for use_hb in (True, False):
        got = R.refine64(pos, x, hwt, hb if use_hb else None)
        for i, (b, t) in enumerate(pos):
            for v in range(V):
                a = 0.0
                for c in range(D):
                    a = a + float(hwt[c, v]) * float(x[b, c, t])
                assert got[i, v] == a + (float(hb[v]) if use_hb else 0.0)
        assert float(np.abs(got - (np.einsum("cv,nc->nv", hwt.astype(np.float64), x[[1, 0, 1], :, [4, 0, 2]].astype(np.float64))
                                   + (hb if use_hb else 0.0))).max()) < 1e-13
    for use_b2 in (True, False):
        got = R.refine64(pos, None, hwt, hb, f=f, h=h, w2t=w2t, b2=b2 if use_b2 else None)
        for i, (b, t) in enumerate(pos):
            xs = []
            for c in range(D):
                a = 0.0
                for j in range(F):
                    a = a + float(w2t[j, c]) * float(f[b, j, t])
                xs.append((a + (float(b2[c]) if use_b2 else 0.0)) + float(h[b, c, t]))
            for v in range(V):
                a = 0.0
                for c in range(D):
                    a = _fma_exact(float(hwt[c, v]), xs[c], a)
                assert got[i, v] == a + float(hb[v])
