"""GPU: the TTE's integer and gather kernels on their own (parrot_debug_durations / parrot_debug_length_regulate /
parrot_debug_argmax_guard: the launchers of csrc/tte_glue.h that the model itself calls; the embedding kernels through the
parrot_tte_debug_stages taps), each against the plain numpy restatement of tests/tte_glue_ref.py, which tests/test_tte_glue_cpu.py
pins against torch and the oracle.

Every comparison is exact:
  * durations: log_dur bit-equal to the masked input; dur equal to the fp64 evaluation wherever exp64(v) - 1 is at least 1e-4 from
    k + 0.5 (the project's rule, tests/test_gpu_parity.py), either neighbour inside that band (share printed, capped at 1 %); cum the
    exact inclusive sum of the device's OWN dur; sums saturate at INT32_MAX; a NaN / +inf log-duration of a real token raises status 5.
  * length regulator: y bit-equal to pe_row + gather (one fp32 add), both mask rules, exact cum / out_len, statuses 6 and 7.
  * argmax: first-maximum ids, the fp32 top-2 margin (minimum bitwise), the guarded set, at V below / at / above the 16 wave ranges
    with the designed columns placed on the range boundaries.
  * refinement: gref bit-equal to float32 of the sequential fp64 evaluation.  Shallow form and the deep form's sum over F: products of
    two fp32 values, exact in fp64, so `a + w x` is the kernel's fma.  The deep form's head multiplies a weight with a full fp64
    activation: there the kernel's fma rounds once, which tte_glue_ref.fma64 restates.
Outputs sit between sentinel regions that must stay intact, and every call is repeated and must come out bit-identical (the guard
list as a set: its order is the order in which the atomics land).  The whole file also passes under PARROT_POISON_WS=nan."""
import ctypes as C
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tte_glue_ref as R  # noqa: E402
from oracle import parrot_oracle as O  # noqa: E402
from parrot_tts_amd import _lib, ops, synth  # noqa: E402
from parrot_tts_amd.tte import Parrot  # noqa: E402
from test_gpu_parity import _report  # noqa: E402

DEV = "cuda:0"
GUARD_ELEMS, SENTINEL = 4096, 77
INT32_MAX = R.INT32_MAX
INF_BITS = 0x7F800000
TG = 2.0 ** -13  # the guard of the argmax tests: margins of exactly 2^-13 stay, 2^-14 are guarded


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


class Fenced:
    """Output tensors carved out of sentinel-filled buffers; intact() after a call."""

    def __init__(self):
        self.bufs = []

    def new(self, shape, dtype, fill=SENTINEL):
        n = math.prod(shape)
        buf = torch.full((GUARD_ELEMS + n + GUARD_ELEMS,), fill, dtype=dtype, device=DEV)
        self.bufs.append((buf, n, fill))
        return buf[GUARD_ELEMS:GUARD_ELEMS + n].view(shape)

    def intact(self):
        return all(bool((b[:GUARD_ELEMS] == f).all()) and bool((b[GUARD_ELEMS + n:] == f).all()) for b, n, f in self.bufs)


def _np(d):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in d.items()}


# =========================================================================================================================================
# durations
# =========================================================================================================================================
def _dur_out(fence, B, S):
    return {"log_dur": fence.new((B, S), torch.float32), "dur": fence.new((B, S), torch.int64), "cum": fence.new((B, S), torch.int32),
            "out_len": fence.new((B,), torch.int32), "status": torch.zeros((1,), dtype=torch.int32, device=DEV)}


def _run_durations(v, valid, src_len):
    B, S = v.shape
    fence = Fenced()
    args = (_dev(v), _dev(valid), _dev(src_len))
    got = _np(ops.debug_durations(*args, out=_dur_out(fence, B, S)))
    assert fence.intact()
    again = _np(ops.debug_durations(*args))
    for k in got:
        assert np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)), k  # (bytes: a NaN log-duration compares too)
    return got


def _exact_cum(dur):
    """Inclusive sums of the device's own durations in exact integers, saturated."""
    cum = np.zeros(dur.shape, dtype=np.int64)
    for b in range(dur.shape[0]):
        run = 0
        for s in range(dur.shape[1]):
            run += int(dur[b, s])
            cum[b, s] = min(run, INT32_MAX)
    return cum


@pytest.mark.parametrize("mode", R.DUR_MODES)
@pytest.mark.parametrize("S", R.DUR_S)
def test_durations_exact(S, mode):
    v, valid, src_len = R.duration_case(S, mode)
    got = _run_durations(v, valid, src_len)
    ld, real = R.masked_log_dur(v, valid, src_len)
    assert np.array_equal(got["log_dur"].view(np.int32), ld.view(np.int32))
    ok, band = R.durations_match(got["dur"], ld)
    share = float(band.mean())
    print(json.dumps(dict(S=S, mode=mode, band_share=share, mismatches=int((~ok).sum()))))
    _report(test="tte_glue_durations", S=S, mode=mode, band_share=share, mismatches=int((~ok).sum()))
    assert share <= 0.01
    assert ok.all(), np.argwhere(~ok)[:5]
    assert (got["dur"][~real] == 0).all()
    cum = _exact_cum(got["dur"])
    assert np.array_equal(got["cum"].astype(np.int64), cum)
    assert np.array_equal(got["out_len"].astype(np.int64), cum[:, -1])
    assert int(got["status"][0]) == 0


def _overflow_rows(S):
    """Three rows of small log-durations with (0) one token of 2^32 + 512 j, (1) two tokens of ln(2^31 + 1), (2) one token of exp(60)."""
    rng = _rng(23 + S)
    v = rng.uniform(-3.0, 1.5, size=(3, S)).astype(np.float32)
    v[0, S // 2] = 22.18071
    v[1, 0] = v[1, S - 1] = np.float32(math.log(2.0 ** 31 + 1))
    v[2, (2 * S) // 3] = 60.0
    return v


@pytest.mark.parametrize("S", [3, 300])
def test_durations_overflow_saturates(S):
    """The defect this file was written for: int32 partial sums wrapped (three tokens of 2^32 + 512 j beside normal ones gave a
    plausible out_len of 1536).  Sums are int64 now and stored saturated."""
    v = _overflow_rows(S)
    valid = np.ones((3, S), dtype=np.uint8)
    got = _run_durations(v, valid, None)
    print(json.dumps(dict(S=S, out_len=got["out_len"].tolist(), big=[int(got["dur"][0, S // 2]), int(got["dur"][1, 0]), int(got["dur"][2, (2 * S) // 3])])))
    assert got["out_len"].tolist() == [INT32_MAX] * 3
    assert (np.diff(got["cum"].astype(np.int64), axis=1) >= 0).all() and (got["cum"][:, -1] == INT32_MAX).all()
    assert np.array_equal(got["cum"].astype(np.int64), _exact_cum(got["dur"]))
    # dur itself.  Small ones by the fp64 rule.  The huge ones, wherever exp(v) - 1 < 2^62: the fp32 grid is 256 / 512 wide there, so
    # no fp32 evaluation can give the fp64 integer, and the reference's own fp32 exp is not one number either -- exp64(22.18071f) lies
    # 0.511 grid steps above 2^32, and torch.exp on the CPU returns 2^32 for that element alone and 2^32 + 512 inside this (3, S)
    # array (scalar and vector code paths of an expf of <= 1 ulp error; measured).  What every such evaluation
    # satisfies, and what is asserted: dur is rint(e - 1) for one of the two fp32 neighbours e of exp64(v).
    ref32 = O.durations_from_log(torch.from_numpy(v)).numpy()
    small = v < 10
    ok, _ = R.durations_match(got["dur"], np.where(small, v, 0))
    assert ok[small].all()
    mid = ~small & (np.exp(v.astype(np.float64)) - 1 < 2.0 ** 62)
    lo, hi = R.faithful_durations(np.where(mid, v, 0))
    print(json.dumps(dict(device=got["dur"][mid].tolist(), cpu_fp32=ref32[mid].tolist(), lo=lo[mid].tolist(), hi=hi[mid].tolist())))
    assert mid.sum() == 3 and ((got["dur"][mid] == lo[mid]) | (got["dur"][mid] == hi[mid])).all(), (got["dur"][mid], lo[mid], hi[mid])
    assert ((ref32[mid] == lo[mid]) | (ref32[mid] == hi[mid])).all()  # (... the reference's own evaluation on this host included)
    assert (got["dur"][mid] >= 2 ** 30).all() and int(got["dur"][2, (2 * S) // 3]) >= 2 ** 62
    assert int(got["status"][0]) == 0  # (finite log-durations: the length check of the decode is what fails, as pe[L] does in the reference)


@pytest.mark.parametrize("S", [2, 300])
def test_durations_nonfinite_raise_status_for_real_tokens_only(S):
    """NaN is a silent duration 0 by the clamp, +inf a saturated one: for a real token both raise status 5 (the reference fails on
    them).  At padded positions the value is masked first and changes nothing."""
    rng = _rng(29 + S)
    v = rng.uniform(-3.0, 3.0, size=(3, S)).astype(np.float32)
    valid = np.ones((3, S), dtype=np.uint8)
    valid[1, S - 1] = 0
    valid[2, 0] = 0
    base = _run_durations(v, valid, None)
    assert int(base["status"][0]) == 0
    for bad in (np.nan, np.inf):
        for (b, s) in [(1, S - 1), (2, 0)]:  # padded
            w = v.copy()
            w[b, s] = bad
            got = _run_durations(w, valid, None)
            for k in base:
                assert np.array_equal(got[k], base[k]), (bad, b, s, k)
        for (b, s) in [(0, S - 1), (1, 0)]:  # real
            w = v.copy()
            w[b, s] = bad
            got = _run_durations(w, valid, None)
            assert int(got["status"][0]) == R.ST_NONFINITE, (bad, b, s)
            assert np.array_equal(got["log_dur"].view(np.int32), R.masked_log_dur(w, valid)[0].view(np.int32))
            assert np.array_equal(got["cum"].astype(np.int64), _exact_cum(got["dur"]))
            others = np.ones_like(valid, dtype=bool)
            others[b, s] = False
            assert np.array_equal(got["dur"][others], base["dur"][others])
    # the row-exact mode decides by src_len, not by the key mask: key 0 of an empty row is attendable and still padded
    src_len = np.array([S, 0, S - 1], dtype=np.int32)
    key = (np.arange(S)[None, :] < np.maximum(src_len, 1)[:, None]).astype(np.uint8)
    w = v.copy()
    w[1, 0] = np.nan
    w[2, S - 1] = np.inf
    got = _run_durations(w, key, src_len)
    assert int(got["status"][0]) == 0 and got["out_len"][1] == 0 and (got["log_dur"][1] == 0).all()


# =========================================================================================================================================
# prefix sums and the length regulator
# =========================================================================================================================================
LR_S = (1, 129, 256, 257, 600, 1025)
LR_D = (1, 3, 4, 5, 64, 300)
LR_ENDS = (63, 64, 65, 0)  # rows 1 .. 4 end there; row 0 is the longest


@functools.lru_cache(maxsize=None)
def _lr_durations(S):
    rng = _rng(41 + S)
    dur = rng.choice(np.array([0, 0, 1, 2, 7]), size=(5, S)).astype(np.int64)
    if S >= 12:  # runs of zeros at the start, in the middle and at the end
        dur[0, :3] = 0
        dur[0, S // 2:S // 2 + 4] = 0
        dur[0, -3:] = 0
    dur[0, S // 3] = 70  # the long token
    for b, end in enumerate(LR_ENDS, start=1):
        run = 0
        for s in range(S):
            d = int(dur[b, s]) if s < S - 1 or S == 1 else 0
            d = min(d, end - run) if S > 1 else end
            dur[b, s] = d
            run += d
        if run < end:
            dur[b, S // 2] += end - run
    assert dur.sum(1)[1:].tolist() == list(LR_ENDS) and dur.sum(1)[0] > 65
    last = [int(np.flatnonzero(r)[-1]) + 1 if r.any() else 0 for r in dur]
    src_len = np.array([S, last[1], S, last[3], 0], dtype=np.int32)
    return dur, src_len


def _run_lr(enc, dur, pe, L, row_exact, src_len, want_mask=True):
    B, D, S = enc.shape
    fence = Fenced()
    out = {"y": fence.new((B, D, L), torch.float32), "tgt_mask": fence.new((B, L), torch.uint8) if want_mask else None,
           "cum": fence.new((B, S), torch.int32), "out_len": fence.new((B,), torch.int32),
           "status": torch.zeros((1,), dtype=torch.int32, device=DEV)}
    args = (_dev(enc), _dev(dur), _dev(pe), L)
    kw = dict(row_exact=row_exact, src_len=_dev(src_len))
    got = _np(ops.debug_length_regulate(*args, out=out, **kw))
    assert fence.intact()
    again = _np(ops.debug_length_regulate(*args, want_mask=want_mask, **kw))
    for k in got:
        assert (got[k] is None and again[k] is None) or np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)), k
    return got


def _check_lr(got, enc, dur, pe, L, row_exact, src_len, status=0):
    y, mask, cum, out_len, st = R.length_regulate(enc, dur, pe, L, row_exact=row_exact, src_len=src_len)
    assert st == ({status} if status else set())
    assert np.array_equal(got["cum"], cum) and np.array_equal(got["out_len"], out_len)
    assert np.array_equal(got["y"].view(np.int32), y.view(np.int32))
    if got["tgt_mask"] is not None:
        assert np.array_equal(got["tgt_mask"], mask)
    assert int(got["status"][0]) == status


@pytest.mark.parametrize("D", LR_D)
@pytest.mark.parametrize("S", LR_S)
def test_length_regulator_exact(S, D):
    dur, src_len = _lr_durations(S)
    L = int(dur.sum(1).max())
    rng = _rng(1000 * S + D)
    enc = rng.standard_normal((5, D, S)).astype(np.float32)
    pe = rng.standard_normal((L + 2, D)).astype(np.float32)
    for row_exact in (0, 1):
        for sl in (None, src_len):
            got = _run_lr(enc, dur, pe, L, row_exact, sl)
            _check_lr(got, enc, dur, pe, L, row_exact, sl)
            assert got["out_len"].tolist() == [L] + list(LR_ENDS)
    # a caller that supplies the key mask itself passes no tgt_mask
    got = _run_lr(enc, dur, pe, L, 0, None, want_mask=False)
    _check_lr(got, enc, dur, pe, L, 0, None)


@pytest.mark.parametrize("S", [2, 300])
def test_length_regulator_bad_and_huge_durations(S):
    rng = _rng(53 + S)
    D, L = 5, 70
    enc = rng.standard_normal((3, D, S)).astype(np.float32)
    pe = rng.standard_normal((L + 1, D)).astype(np.float32)
    base = np.zeros((3, S), dtype=np.int64)
    base[:, 0] = [L, 3, 1]
    # a negative duration: status 6, counts as 0
    dur = base.copy()
    dur[1, S - 1] = -5
    _check_lr(_run_lr(enc, dur, pe, L, 0, None), enc, dur, pe, L, 0, None, status=R.ST_NEGATIVE)
    # a duration at s >= src_len: status 7, counts as 0; the same durations without src_len count
    dur = base.copy()
    dur[2, S - 1] = 4
    src_len = np.array([S, S, S - 1], dtype=np.int32)
    got = _run_lr(enc, dur, pe, L, 1, src_len)
    _check_lr(got, enc, dur, pe, L, 1, src_len, status=R.ST_PADDED)
    assert got["out_len"][2] == 1
    got = _run_lr(enc, dur, pe, L, 1, None)
    _check_lr(got, enc, dur, pe, L, 1, None)
    assert got["out_len"][2] == 5
    # 2^31 and 2^40 saturate: cum stays at INT32_MAX, the L frames read come from that token
    dur = base.copy()
    dur[1, S - 1] = 2 ** 31
    dur[2, 0] = 2 ** 40
    for row_exact in (0, 1):
        got = _run_lr(enc, dur, pe, L, row_exact, None)
        _check_lr(got, enc, dur, pe, L, row_exact, None)
        assert got["out_len"].tolist() == [L, INT32_MAX, INT32_MAX] and (got["cum"][2] == INT32_MAX).all()
        assert np.array_equal(got["y"][2], (pe[L][:, None] + enc[2][:, :1]).astype(np.float32).repeat(L, axis=1))


# =========================================================================================================================================
# argmax and the tie guard
# =========================================================================================================================================
AG_V = (1, 2, 15, 16, 17, 31, 33, 1000, 1030)
AG_L = (1, 63, 64, 65, 130)
N_DESIGNS = 14


def _design(kind, V, rng):
    """One designed column (V,), placed from the kernel's wave ranges; a design that V is too small for falls back to a plain one."""
    col = rng.uniform(-2.0, -1.0, size=V).astype(np.float32)
    ranges = [r for r in R.wave_ranges(V) if r[1] > r[0]]
    w = int(rng.integers(0, len(ranges)))
    w2 = (w + 1 + int(rng.integers(0, max(len(ranges) - 1, 1)))) % len(ranges)
    (a0, a1), (b0, b1) = ranges[w], ranges[w2]
    wide = [r for r in ranges if r[1] - r[0] >= 2]
    if kind == 0:       # the maximum at the first index of a range
        col[a0] = 1.0
    elif kind == 1:     # ... at the last
        col[a1 - 1] = 1.0
    elif kind == 2:     # duplicate maxima inside one range
        if wide:
            c0, c1 = wide[w % len(wide)]
            col[c0] = col[c1 - 1] = 1.0
        else:
            col[a0] = col[b0] = 1.0
    elif kind == 3:     # duplicate maxima in two ranges
        col[a1 - 1] = col[b0] = 1.0
    elif kind in (4, 5):  # the runner-up before / after the maximum, same range
        if wide:
            c0, c1 = wide[w % len(wide)]
            col[c0], col[c1 - 1] = (0.5, 1.0) if kind == 4 else (1.0, 0.5)
        else:
            col[a0] = 1.0
    elif kind in (6, 7):  # the runner-up in another range, before / after
        lo, hi = sorted((a0, b1 - 1))
        col[lo], col[hi] = (0.5, 1.0) if kind == 6 else (1.0, 0.5)
        if lo == hi:
            col[lo] = 1.0
    elif kind == 8:     # all equal
        col[:] = 0.25
    elif kind == 9:     # -0.0 everywhere, +0.0 later: equal, the first wins
        col[:] = -0.0
        col[V - 1] = 0.0
    elif kind == 10:    # +0.0 first, -0.0 after
        col[:] = -0.0
        col[0] = 0.0
    elif kind == 11:    # a margin of exactly the guard: not guarded
        col[a1 - 1] = 1.0
        if V > 1:
            col[b0 if b0 != a1 - 1 else a0] = np.float32(1.0 - TG)
    elif kind == 12:    # half the guard: guarded
        col[a0] = 1.0
        if V > 1:
            col[b1 - 1 if b1 - 1 != a0 else a1 - 1] = np.float32(1.0 - TG / 2)
    else:               # the maximum last of all, the runner-up first of all
        col[V - 1], col[0] = 1.0, 0.5
        if V == 1:
            col[0] = 1.0
    return col


@functools.lru_cache(maxsize=None)
def _ag_logits(B, V, L):
    rng = _rng(7919 * V + 31 * L + B)
    x = rng.standard_normal((B, V, L)).astype(np.float32)
    for b in range(B):
        for t in range(L):
            i = b * L + t
            if i % 2 == 0:
                x[b, :, t] = _design((i // 2 + L + V) % N_DESIGNS, V, rng)
    x.setflags(write=False)
    return x


def _ag_out(fence, B, V, L, fill=0):
    return {"ids": fence.new((B, L), torch.int64), "glist": fence.new((R.TIE_GUARD_MAX, 2), torch.int32, fill),
            "gstat": fence.new((4,), torch.int32, fill), "gref": fence.new((R.TIE_GUARD_MAX, V), torch.float32, fill),
            "status": torch.zeros((1,), dtype=torch.int32, device=DEV)}


def _listed(got):
    n = min(int(got["gstat"][0]), R.TIE_GUARD_MAX)
    return [tuple(int(v) for v in p) for p in got["glist"][:n]]


def _run_ag(x, guard, row0=0, refine=None, gstat_start=None, fill=0, prefill=None):
    B, V, L = x.shape
    outs = []
    for _ in range(2):  # every call twice, into fresh fenced buffers
        fence = Fenced()
        out = _ag_out(fence, B, V, L, fill)
        if prefill is not None:
            prefill(out)
        got = _np(ops.debug_argmax_guard(_dev(x), guard, row0=row0, refine=refine, gstat_start=gstat_start, out=out))
        assert fence.intact()
        outs.append(got)
    a, b = outs
    assert np.array_equal(a["ids"], b["ids"]) and np.array_equal(a["gstat"], b["gstat"]) and np.array_equal(a["status"], b["status"])
    if guard > 0:
        assert sorted(_listed(a)) == sorted(_listed(b)) or int(a["gstat"][0]) > R.TIE_GUARD_MAX
    return a


def _check_ag(got, x, guard, row0):
    ref = R.argmax_guard(x, guard, row0=row0)
    assert np.array_equal(got["ids"], ref["ids"])
    assert int(got["gstat"][2]) == ref["min_bits"], (hex(int(got["gstat"][2])), hex(ref["min_bits"]))
    assert int(got["gstat"][0]) == ref["count"]
    lst = _listed(got)
    assert len(set(lst)) == len(lst) == min(ref["count"], R.TIE_GUARD_MAX)
    assert set(lst) == ref["guarded"] if ref["count"] <= R.TIE_GUARD_MAX else set(lst) <= ref["guarded"]
    assert int(got["gstat"][1]) == 0 and int(got["gstat"][3]) == 0 and int(got["status"][0]) == 0
    return ref


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V", AG_V)
def test_argmax_and_guard_exact(V, B):
    row0 = 2 if B == 1 else 0
    worst = 0
    for L in AG_L:
        x = _ag_logits(B, V, L)
        ref = _check_ag(_run_ag(x, TG, row0=row0), x, TG, row0)
        worst = max(worst, ref["count"])
        # the designs did land: exact ties and the two threshold margins are present (V = 1 has no second element)
        if V > 1 and L >= 63:
            m = ref["margin"]
            assert (m == 0).any() and (m == np.float32(TG)).any() and (m == np.float32(TG / 2)).any()
            assert not any((row0 + int(b), int(t)) in ref["guarded"] for b, t in zip(*np.nonzero(m == np.float32(TG))))
    _report(test="tte_glue_argmax", V=V, B=B, max_guarded=worst, mismatches=0)


def test_argmax_more_guarded_positions_than_the_list_holds():
    x = np.full((3, 33, 130), 0.5, dtype=np.float32)  # 390 ties
    x[1, 7, 5] = 3.0                                    # ... but one
    got = _run_ag(x, TG)
    ref = _check_ag(got, x, TG, 0)
    assert ref["count"] == 389 and int(got["gstat"][0]) == 389 and len(set(_listed(got))) == R.TIE_GUARD_MAX
    assert (got["ids"] == 0).sum() == 389 and got["ids"][1, 5] == 7


@pytest.mark.parametrize("V", [17, 1000])
def test_argmax_nonfinite_columns_are_flagged_and_guarded(V):
    L = 65
    rng = _rng(61 + V)
    x = rng.standard_normal((2, V, L)).astype(np.float32) * 4  # (random columns with a wide margin)
    r3 = R.wave_ranges(V)[3][0]
    cases = {}
    x[0, :, 3] = -np.inf
    cases[(0, 3)] = 0
    x[1, V // 2, 64] = np.inf
    cases[(1, 64)] = V // 2
    x[0, 0, 10] = np.nan
    cases[(0, 10)] = None   # (ids are not asserted where the column holds a NaN)
    x[1, r3, 0] = np.nan
    cases[(1, 0)] = None
    got = _run_ag(x, TG, row0=4)
    assert int(got["status"][0]) == R.ST_NONFINITE
    ref = R.argmax_guard(x, TG, row0=4)
    lst = set(_listed(got))
    assert lst == ref["guarded"] and int(got["gstat"][0]) == ref["count"]
    for (b, t), want in cases.items():
        assert (4 + b, t) in lst
        if want is not None:
            assert got["ids"][b, t] == want
    clean = ~np.isnan(x).any(axis=1)
    assert np.array_equal(got["ids"][clean], ref["ids"][clean])


def test_argmax_guard_off_touches_neither_list_nor_statistics():
    x = _ag_logits(3, 33, 65)
    got = _run_ag(x, 0.0, fill=SENTINEL)
    assert np.array_equal(got["ids"], R.argmax_guard(x, TG)["ids"]) and int(got["status"][0]) == 0
    assert (got["glist"] == SENTINEL).all() and (got["gstat"] == SENTINEL).all() and (got["gref"] == SENTINEL).all()


# =========================================================================================================================================
# the fp64 re-evaluation
# =========================================================================================================================================
RF_D = (8, 256, 300)
RF_V = (5, 256, 257, 1000, 1025, 1030)
RF_B, RF_L = 2, 20
RF_GUARDED = [(0, 0), (0, 7), (0, 19), (1, 1), (1, 2), (1, 13), (1, 19)]  # positions whose logits are ties
RF_P0, RF_P1 = (0, 7), (1, 13)  # the positions whose maximum sits on duplicated head columns


@functools.lru_cache(maxsize=None)
def _rf_case(D, V, F):
    rng = _rng(104729 * D + 17 * V + F)
    h = rng.standard_normal((RF_B, D, RF_L)).astype(np.float32)
    hwt = rng.standard_normal((D, V)).astype(np.float32)
    hb = (rng.standard_normal(V) * 0.05).astype(np.float32)
    # two identical head columns at v, v + 1 (two threads) that win at P0, and at v2, v2 + 256 (one thread's two codes) that win at P1
    v = min(2, V - 2)
    hwt[:, v] = hwt[:, v + 1] = 3 * np.sign(h[RF_P0[0], :, RF_P0[1]])
    hb[v + 1] = hb[v]
    dup2 = V > 300
    if dup2:
        hwt[:, 40] = hwt[:, 40 + 256] = 3 * np.sign(h[RF_P1[0], :, RF_P1[1]])
        hb[40 + 256] = hb[40]
    f = w2t = b2 = None
    if F:
        f = np.maximum(rng.standard_normal((RF_B, F, RF_L)), 0).astype(np.float32)
        w2t = (rng.standard_normal((F, D)) * (0.05 / math.sqrt(F))).astype(np.float32)  # (small: h decides where the maximum is)
        b2 = (rng.standard_normal(D) * 0.01).astype(np.float32)
    logits = rng.standard_normal((RF_B, V, RF_L)).astype(np.float32) * 4
    for b, t in RF_GUARDED:
        logits[b, :, t] = 0.125
    return dict(h=h, hwt=hwt, hb=hb, f=f, w2t=w2t, b2=b2, logits=logits, v=v, dup2=dup2)


def _refine_args(c, use_bias):
    r = {"x": _dev(c["h"]), "hwt": _dev(c["hwt"]), "hb": _dev(c["hb"]) if use_bias else None}
    if c["f"] is not None:
        r.update(f=_dev(c["f"]), h=_dev(c["h"]), w2t=_dev(c["w2t"]), b2=_dev(c["b2"]) if use_bias else None)
    return r


def _check_refine(got, c, use_bias, row0, first=0, ids_plain=None):
    """Entries [first, n) of the list against refine64, bit for bit; ids the first maximum of the fp64 values."""
    lst = _listed(got)[first:]
    pos = [(b - row0, t) for b, t in lst]
    assert sorted(pos) == sorted(RF_GUARDED)
    a = R.refine64(pos, c["h"], c["hwt"], c["hb"] if use_bias else None, f=c["f"], h=c["h"], w2t=c["w2t"], b2=c["b2"] if use_bias else None)
    want32 = a.astype(np.float32)
    got32 = got["gref"][first:first + len(pos)]
    bad = int((got32.view(np.int32) != want32.view(np.int32)).sum())
    assert bad == 0, (bad, got32.size)
    best = np.argmax(a, axis=1)  # (numpy: the first maximum)
    changed = 0
    for i, (b, t) in enumerate(pos):
        assert got["ids"][b, t] == best[i], (b, t)
        changed += int(ids_plain[b, t] != best[i])
    assert int(got["gstat"][1]) == changed
    return dict(zip(pos, best)), a


@pytest.mark.parametrize("V", RF_V)
@pytest.mark.parametrize("D", RF_D)
def test_refinement_is_the_sequential_fp64_loop_bit_for_bit(D, V):
    elems = 0
    for F in (0, 40, 1024):
        c = _rf_case(D, V, F)
        plain = R.argmax_guard(c["logits"], TG)
        assert plain["guarded"] == set(RF_GUARDED)
        for use_bias in (True, False):
            got = _run_ag(c["logits"], TG, refine=_refine_args(c, use_bias))
            best, a = _check_refine(got, c, use_bias, 0, ids_plain=plain["ids"])
            elems += a.size
            # duplicated columns: the lower index wins, across two threads and inside one thread
            assert best[RF_P0] == c["v"] and a[list(best).index(RF_P0), c["v"]] == a[list(best).index(RF_P0), c["v"] + 1]
            if c["dup2"]:
                i = list(best).index(RF_P1)
                assert best[RF_P1] == 40 and a[i, 40] == a[i, 296]
            # everything the guard did not list keeps its plain argmax
            keep = np.ones((RF_B, RF_L), dtype=bool)
            for b, t in RF_GUARDED:
                keep[b, t] = False
            assert np.array_equal(got["ids"][keep], plain["ids"][keep])
            assert int(got["gstat"][0]) == len(RF_GUARDED) and int(got["gstat"][2]) == 0 and int(got["status"][0]) == 0
    _report(test="tte_glue_refine", D=D, V=V, elements=elems, mismatches=0)


@pytest.mark.parametrize("F", [0, 40])
def test_refinement_of_a_second_row_group_leaves_the_first_alone(F):
    """gstat_start = {k, ., ., k}: a lane's second row group.  Entries below k belong to the first group (other buffers, rows below
    row0): neither they, their refined rows nor any id are touched; this group's entries start at k and index its own rows."""
    D, V, k, row0 = 256, 257, 5, 3
    c = _rf_case(D, V, F)
    plain = R.argmax_guard(c["logits"], TG)
    earlier = np.array([[0, 2 + i] for i in range(k)], dtype=np.int32)  # (rows of the first group: below row0)

    def prefill(out):
        out["glist"][:k] = torch.from_numpy(earlier).to(DEV)
        out["gref"][:k] = float(SENTINEL)

    got = _run_ag(c["logits"], TG, row0=row0, refine=_refine_args(c, True), gstat_start=[k, 2, INF_BITS, k], prefill=prefill)
    assert int(got["gstat"][0]) == k + len(RF_GUARDED) and int(got["gstat"][3]) == k
    assert np.array_equal(got["glist"][:k], earlier) and (got["gref"][:k] == SENTINEL).all()
    best, _ = _check_refine(dict(got, gstat=np.array([got["gstat"][0], got["gstat"][1] - 2, 0, k])), c, True, row0, first=k, ids_plain=plain["ids"])
    # positions (b, 2 + i) of THIS group are not in its list: their ids are the plain argmax although the list names (0, 2 + i)
    for i in range(k):
        assert got["ids"][0, 2 + i] == plain["ids"][0, 2 + i]
    assert (got["gref"][k + len(RF_GUARDED):] == 0).all()


# =========================================================================================================================================
# the embedding kernels, through the stage taps of the model
# =========================================================================================================================================
VOCAB, NSPK = 30, 3


@pytest.fixture(scope="module")
def small_model(tmp_path_factory):
    cfg = synth.small_tte_config()
    tmp = str(tmp_path_factory.mktemp("tte_glue"))
    cfg["path"]["root_path"] = tmp
    with open(os.path.join(tmp, "speakers.json"), "w") as f:
        json.dump({f"s{i}": i for i in range(NSPK)}, f)
    sd = synth.synth_tte_state_dict(cfg, VOCAB, NSPK, seed=5, forced_duration=1)  # (L = the number of real tokens: S <= 130 stays below max_len)
    m = Parrot(cfg, VOCAB, 0)
    m.load_state_dict(sd)
    return m.eval().to(DEV), sd, cfg


def _encoder_taps(model, batch, row_exact):
    ne = model.data_config["transformer"]["encoder"]["n_layer"]
    B, S = batch["phones"].shape
    model._current_handle(torch.device(DEV))
    fence = Fenced()
    enc = [fence.new((B, model.d_model, S), torch.float32) for _ in range(ne + 2)]
    ptrs = (C.c_void_p * (ne + 2))(*[C.c_void_p(t.data_ptr()) for t in enc])
    lib = _lib.lib()
    _lib.check(lib.parrot_tte_debug_stages(model._handle, ptrs, None))
    try:
        model._run(batch, want_logits=False, row_exact=row_exact)
        torch.cuda.synchronize()
    finally:
        _lib.check(lib.parrot_tte_debug_stages(model._handle, None, None))
    assert fence.intact()
    return [t.cpu().numpy() for t in enc]


def _emb_batch(S, seed):
    b = synth.synth_tte_batch(3, S, VOCAB, NSPK, seed=seed, ragged=S > 1)
    b["speaker"] = torch.tensor([2, 0, 1])
    return b


@pytest.mark.parametrize("row_exact", [False, True])
@pytest.mark.parametrize("S", [1, 63, 64, 65, 130])
def test_embedding_and_speaker_add_exact(small_model, S, row_exact):
    model, sd, _ = small_model
    batch = _emb_batch(S, 70 + S)
    taps = _encoder_taps(model, {k: v.to(DEV) for k, v in batch.items()}, row_exact)
    assert all(np.array_equal(a, b) for a, b in zip(taps, _encoder_taps(model, {k: v.to(DEV) for k, v in batch.items()}, row_exact)))
    pe, emb, spk = sd["pos_emb.pe"].numpy(), sd["tok_emb.weight"].numpy(), sd["speaker_emb.weight"].numpy()
    phones, lens = batch["phones"].numpy(), batch["src_mask"].sum(1).numpy()
    for b in range(3):
        row = pe[int(lens[b]) if row_exact else S]
        want = (row[None, :] + emb[phones[b]]).T  # (D, S): pe[S or len_b] + emb[id], pads (id 0) included
        assert np.array_equal(taps[0][b].view(np.int32), np.ascontiguousarray(want).view(np.int32)), b
        want = taps[-2][b] + spk[int(batch["speaker"][b])][:, None]
        assert np.array_equal(taps[-1][b].view(np.int32), want.view(np.int32)), b


def test_embedding_ids_out_of_range_raise(small_model):
    model, _, _ = small_model
    for key, bad, code in (("phones", VOCAB, 3), ("speaker", NSPK, 4)):
        batch = _emb_batch(9, 3)
        batch[key] = batch[key].clone()
        batch[key].view(-1)[1] = bad
        with pytest.raises(IndexError, match=f"code {code}"):
            model.infer({k: v.to(DEV) for k, v in batch.items()})
    batch = _emb_batch(9, 3)
    assert len(model.infer({k: v.to(DEV) for k, v in batch.items()})) == 3  # ... and the handle is fine afterwards


def test_a_runaway_duration_prediction_raises_instead_of_returning_ids(small_model):
    """duration_predictor.proj: weight 0, bias 60 -- every real token lasts exp(60) frames.  The reference fails (pe[T] out of range,
    fft.py:18).  With int32 sums the expanded length wrapped to whatever the low bits gave and ids came back."""
    _, sd, cfg = small_model
    sd = {k: v.clone() for k, v in sd.items()}
    sd["duration_predictor.proj.weight"].zero_()
    sd["duration_predictor.proj.bias"].fill_(60.0)
    m = Parrot(cfg, VOCAB, 0)
    m.load_state_dict(sd)
    m = m.eval().to(DEV)
    for S in (3, 11):
        batch = {k: v.to(DEV) for k, v in _emb_batch(S, 5).items()}
        for row_exact in (False, True):
            with pytest.raises(IndexError):
                m.infer(batch, row_exact=row_exact)


# =========================================================================================================================================
# refusals (every one before a launch) and poison
# =========================================================================================================================================
def test_refusals():
    lib = _lib.lib()
    p, st = ops.dptr, ops.stream_ptr
    B, S, D, L, V = 2, 4, 3, 6, 5
    z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=DEV)  # noqa: E731
    t = dict(ld=z((B, S)), valid=z((B, S), torch.uint8), log_dur=z((B, S)), dur=z((B, S), torch.int64), cum=z((B, S), torch.int32),
             out_len=z((B,), torch.int32), status=z((1,), torch.int32), enc=z((B, D, S)), pe=z((L + 1, D)), y=z((B, D, L)),
             mask=z((B, L), torch.uint8), logits=z((B, V, L)), ids=z((B, L), torch.int64), glist=z((256, 2), torch.int32),
             gstat=z((4,), torch.int32), gref=z((256, V)), x=z((B, D, L)), hwt=z((D, V)), f=z((B, 7, L)), w2t=z((7, D)))

    def durations(Bc=B, Sc=S, null=()):
        a = {k: (None if k in null else p(t[k])) for k in ("ld", "valid", "log_dur", "dur", "cum", "out_len", "status")}
        return lib.parrot_debug_durations(a["ld"], a["valid"], None, Bc, Sc, a["log_dur"], a["dur"], a["cum"], a["out_len"], a["status"], st())

    def regulate(Bc=B, Sc=S, Dc=D, Lc=L, P=L + 1, null=()):
        a = {k: (None if k in null else p(t[k])) for k in ("enc", "dur", "pe", "y", "mask", "cum", "out_len", "status")}
        return lib.parrot_debug_length_regulate(a["enc"], a["dur"], None, a["pe"], Bc, Sc, Dc, Lc, P, 0, a["y"], a["mask"], a["cum"], a["out_len"],
                                                a["status"], st())

    def argmax(Bc=B, Vc=V, Lc=L, guard=TG, row0=0, Dc=D, Fc=7, null=(), refine=False, deep=False, start=None):
        names = ("logits", "ids", "glist", "gstat", "gref", "status", "x", "hwt", "f", "w2t")
        a = {k: (None if k in null else p(t[k])) for k in names}
        if not refine:
            a["x"] = None
        if not deep:
            a["f"] = None
        s4 = None if start is None else (C.c_int32 * 4)(*start)
        return lib.parrot_debug_argmax_guard(a["logits"], Bc, Vc, Lc, guard, row0, a["x"], Dc, a["hwt"], None, a["f"], a["x"] if deep else None,
                                             a["w2t"], None, Fc, s4, a["ids"], a["glist"], a["gstat"], a["gref"], a["status"], st())

    big = (1 << 20) + 1
    assert durations() == 0 and regulate() == 0 and argmax() == 0 and argmax(refine=True) == 0 and argmax(refine=True, deep=True) == 0
    for n in ("ld", "valid", "log_dur", "dur", "cum", "out_len", "status"):
        assert durations(null=(n,)) == -1, n
    assert b"debug_durations" in lib.parrot_last_error()
    assert durations(Bc=0) == -1 and durations(Sc=0) == -1 and durations(Sc=-3) == -1
    assert durations(Sc=big) == -5 and durations(Bc=65536) == -5
    for n in ("enc", "dur", "pe", "y", "cum", "out_len", "status"):
        assert regulate(null=(n,)) == -1, n
    assert regulate(null=("mask",)) == 0  # (the caller's own key mask: no tgt_mask)
    assert regulate(Bc=0) == -1 and regulate(Sc=0) == -1 and regulate(Dc=0) == -1 and regulate(Lc=0) == -1 and regulate(Lc=-1) == -1
    assert regulate(P=L) == -2 and regulate(P=L - 1) == -2 and regulate(P=0) == -2
    assert b"pe[L]" in lib.parrot_last_error()
    assert regulate(Sc=big) == -5 and regulate(Dc=big) == -5
    for n in ("logits", "ids", "glist", "gstat", "status"):
        assert argmax(null=(n,)) == -1, n
    assert argmax(Bc=0) == -1 and argmax(Vc=0) == -1 and argmax(Lc=0) == -1 and argmax(guard=-1.0) == -1 and argmax(guard=float("nan")) == -1
    assert argmax(row0=-1) == -1 and argmax(Vc=big) == -5 and argmax(Lc=big) == -5
    assert argmax(refine=True, null=("hwt",)) == -1 and argmax(refine=True, null=("gref",)) == -1 and argmax(refine=True, Dc=0) == -1
    assert argmax(refine=True, deep=True, null=("w2t",)) == -1 and argmax(refine=True, deep=True, Fc=0) == -1
    assert argmax(refine=True, deep=True, Fc=8000) == -5  # (D + F doubles beyond the workgroup's LDS)
    assert argmax(start=(3, 0, 0, 4)) == -1 and argmax(start=(-1, 0, 0, 0)) == -1 and argmax(start=(300, 0, 0, 257)) == -1
    assert argmax(start=(3, 0, INF_BITS, 3)) == 0
    torch.cuda.synchronize()
    with pytest.raises(_lib.ParrotHipError) as e:
        ops.debug_length_regulate(t["enc"], t["dur"], t["pe"], L + 1)
    assert e.value.code == _lib.E_RANGE
    # and the library is fine afterwards
    v, valid, src_len = R.duration_case(257, "hole")
    got = _run_durations(v, valid, src_len)
    assert R.durations_match(got["dur"], R.masked_log_dur(v, valid, src_len)[0])[0].all()


def test_whole_file_under_poison():
    """This file once more in a child process under PARROT_POISON_WS=nan: an output element that a kernel leaves unwritten, or a read
    of one before it is written, shows as the poison word in an exact comparison."""
    if os.environ.get("PARROT_POISON_WS"):
        return  # (already a poisoned run: the tests above were it)
    env = dict(os.environ, PARROT_POISON_WS="nan")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", os.path.abspath(__file__), "-k", "not whole_file"], cwd=ROOT,
                       capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
