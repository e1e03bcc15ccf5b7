"""Plain numpy restatements of the TTE's glue kernels (csrc/tte_glue.h: duration_kernel, dur_prefix_kernel,
length_regulate_kernel, argmax_cf_kernel, tie_guard_refine_kernel), pinned on the CPU by tests/test_tte_glue_cpu.py against torch
and the oracle, and held against the device by tests/test_gpu_tte_glue.py.  Nothing here imports the library."""
import numpy as np

INT32_MAX = 2 ** 31 - 1
TIE_GUARD_MAX = 256
ARGMAX_WAVES = 16
BAND = 1e-4  # durations are exact where |frac(exp64(v) - 1) - 0.5| >= BAND (tests/test_gpu_parity.py: the project's rule)
ST_NONFINITE, ST_NEGATIVE, ST_PADDED = 5, 6, 7


# ---- durations -------------------------------------------------------------------------------------------------------------------------
def masked_log_dur(ld_raw, src_valid=None, src_len=None):
    """What the kernel stores as log_dur: the input where the token is real, +0.0 elsewhere (bit pattern kept where real)."""
    ld_raw = np.asarray(ld_raw, dtype=np.float32)
    B, S = ld_raw.shape
    real = np.arange(S)[None, :] < np.asarray(src_len)[:, None] if src_len is not None else np.asarray(src_valid) != 0
    return np.where(real, ld_raw, np.float32(0.0)).astype(np.float32), real


def durations64(v):
    """max(rint(exp(v) - 1), 0) evaluated in fp64 (rint: round half to even), as int64; NaN -> 0, beyond int64 -> INT64_MAX."""
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(np.asarray(v, dtype=np.float64)) - 1.0
        r = np.rint(e)
    r = np.where(r > 0, r, 0.0)
    big = r >= 2.0 ** 63
    return np.where(big, np.iinfo(np.int64).max, np.where(big, 0.0, r).astype(np.int64))


def in_band(v, band=BAND):
    """Elements whose exact exp(v) - 1 lies within `band` of a rounding boundary k + 0.5 (k >= 0): either neighbour is accepted there."""
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(np.asarray(v, dtype=np.float64)) - 1.0
        frac = e - np.floor(e)
    return np.isfinite(e) & (e > 0) & (np.abs(frac - 0.5) < band)


def durations_match(got, v):
    """got == durations64(v) outside the band; inside it floor or ceil of exp64(v) - 1 (clamped at 0)."""
    got = np.asarray(got, dtype=np.int64)
    ref = durations64(v)
    band = in_band(v)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(np.asarray(v, dtype=np.float64)) - 1.0
    lo = np.maximum(np.floor(np.where(band, e, 0.0)), 0).astype(np.int64)
    ok = np.where(band, (got == lo) | (got == lo + 1), got == ref)
    return ok, band


DUR_S = (1, 2, 255, 256, 257, 511, 513, 1025)  # per = ceil(S / 256) in {1, 2, 3, 5}, rows that end inside a thread's slice
DUR_MODES = ("hole", "left_pad", "src_len")
DUR_B = 3


def faithful_durations(v):
    """The two values max(rint(e - 1), 0) can take in fp32 arithmetic when e is a FAITHFUL fp32 rounding of exp(v) -- one of the two
    fp32 neighbours of the exact value, which is what an expf of at most 1 ulp error returns: (lo, hi) int64 arrays (equal where
    exp64(v) is an fp32 number).  For log-durations beyond ~16 the fp32 grid is coarser than 1 and this, not the fp64 integer, is
    what any fp32 evaluation -- the reference's included -- can be held to."""
    e = np.exp(np.asarray(v, dtype=np.float64))
    near = e.astype(np.float32)
    other = np.where(near.astype(np.float64) > e, np.nextafter(near, np.float32(-np.inf)), np.nextafter(near, np.float32(np.inf)))
    other = np.where(near.astype(np.float64) == e, near, other).astype(np.float32)
    vals = [np.maximum(np.rint(x - np.float32(1.0)), 0).astype(np.float64).astype(np.int64) for x in (near, other)]
    return np.minimum(*vals), np.maximum(*vals)


def duration_case(S, mode, seed=11):
    """The seeded input of the duration tests: v (3, S) uniform in [-3, 4.5] with -inf, 0 and -0.0 at real and at padded positions;
    "hole": row 1 has a pad inside, row 2 is right-padded; "left_pad": rows 1 and 2 start with pads; "src_len": lengths (S, 0,
    S // 2) with the key mask the model passes beside them (the prefix of max(len, 1)).  -> v, src_valid u8, src_len or None."""
    rng = np.random.Generator(np.random.PCG64(seed * 100003 + S * 7 + DUR_MODES.index(mode)))
    v = rng.uniform(-3.0, 4.5, size=(DUR_B, S)).astype(np.float32)
    valid = np.ones((DUR_B, S), dtype=np.uint8)
    src_len = None
    if mode == "hole":
        valid[1, S // 2] = 0
        valid[2, S - S // 3:] = 0
        valid[0, ::2] *= 255  # (any non-zero byte is a real token)
    elif mode == "left_pad":
        valid[1, :S // 2] = 0
        valid[2, :S - 1] = 0
    else:
        src_len = np.array([S, 0, S // 2], dtype=np.int32)
        valid = (np.arange(S)[None, :] < np.maximum(src_len, 1)[:, None]).astype(np.uint8)
    real = np.arange(S)[None, :] < src_len[:, None] if src_len is not None else valid != 0
    for idx in (np.flatnonzero(real), np.flatnonzero(~real)):
        for i, val in enumerate((-np.inf, 0.0, -0.0)):
            if len(idx) > i:
                v.reshape(-1)[idx[(len(idx) * (2 * i + 1)) // 6]] = val
    return v, valid, src_len


# ---- saturating prefix sums and the length regulator -------------------------------------------------------------------------------------
def sat_prefix(dur, src_len=None):
    """dur (B, S) int64 -> (cum (B, S) int32, out_len (B) int32, status): inclusive sums in exact integers, stored saturated at
    INT32_MAX; a negative duration counts as 0 (status 6), a nonzero one at s >= src_len[b] counts as 0 (status 7)."""
    dur = np.asarray(dur, dtype=np.int64)
    B, S = dur.shape
    cum = np.zeros((B, S), dtype=np.int32)
    out_len = np.zeros((B,), dtype=np.int32)
    status = set()
    for b in range(B):
        real = S if src_len is None else int(src_len[b])
        run = 0
        for s in range(S):
            d = int(dur[b, s])
            if d < 0:
                status.add(ST_NEGATIVE)
                d = 0
            elif s >= real and d != 0:
                status.add(ST_PADDED)
                d = 0
            run += min(d, INT32_MAX)
            cum[b, s] = min(run, INT32_MAX)
        out_len[b] = min(run, INT32_MAX)
    return cum, out_len, status


def length_regulate(enc, dur, pe, L, row_exact=False, src_len=None):
    """enc (B, D, S) f32 channel-first, dur (B, S) i64, pe (P, D) f32 -> y (B, D, L) = pe_row + (enc[:, :, src(t)] for t < len_b, else 0)
    in ONE fp32 add, src(t) = first s with cum[b, s] > t; pe_row = pe[L], or pe[min(len_b, L)] in the row-exact mode;
    tgt_mask = t <= len_b (quirk Q2), or t < max(len_b, 1) in the row-exact mode."""
    enc, pe = np.asarray(enc, dtype=np.float32), np.asarray(pe, dtype=np.float32)
    B, D, S = enc.shape
    cum, out_len, status = sat_prefix(dur, src_len)
    y = np.zeros((B, D, L), dtype=np.float32)
    mask = np.zeros((B, L), dtype=np.uint8)
    t = np.arange(L)
    for b in range(B):
        n = int(out_len[b])
        row = pe[min(n, L) if row_exact else L]
        src = np.searchsorted(cum[b], t, side="right")  # smallest s with cum[s] > t
        live = t < n
        g = np.where(live[None, :], enc[b][:, np.minimum(src, S - 1)], np.float32(0.0)).astype(np.float32)
        y[b] = row[:, None] + g
        mask[b] = (t < max(n, 1)) if row_exact else (t <= n)
    return y, mask, cum, out_len, status


# ---- argmax and the tie guard ------------------------------------------------------------------------------------------------------------
def wave_ranges(V):
    """[v0, v1) of each of the kernel's 16 waves (empty beyond V): where a test places its designed columns."""
    per = (V + ARGMAX_WAVES - 1) // ARGMAX_WAVES
    return [(min(V, w * per), min(V, w * per + per)) for w in range(ARGMAX_WAVES)]


def argmax_guard(logits, guard, row0=0):
    """logits (B, V, L) f32 -> dict: ids (B, L) first maximum; margin (B, L) f32 = largest - second largest element (duplicates
    count: two equal maxima give 0; V = 1 gives +inf), the subtraction in fp32; nonfinite (B, L): the column holds NaN / inf;
    guarded: the set of (row0 + b, t) with not (margin >= guard) or a non-finite column; count; min_bits: the smallest margin >= 0
    as int32 float bits (+inf bits when there is none).  ids / margin of a column that holds a NaN are not defined here."""
    x = np.asarray(logits, dtype=np.float32)
    B, V, L = x.shape
    nonfinite = ~np.isfinite(x).all(axis=1)
    xs = np.where(np.isnan(x), -np.inf, x).astype(np.float32)
    ids = np.argmax(xs, axis=1).astype(np.int64)
    if V > 1:
        top = np.sort(xs, axis=1)[:, -2:, :]
        with np.errstate(invalid="ignore"):
            margin = (top[:, 1] - top[:, 0]).astype(np.float32)
    else:
        with np.errstate(invalid="ignore"):
            margin = (xs[:, 0] - np.float32(-np.inf)).astype(np.float32)
    margin = np.where(margin == 0, np.float32(0.0), margin).astype(np.float32)  # (a tie of -0.0 and +0.0: +0.0, whichever came first)
    with np.errstate(invalid="ignore"):
        guarded_mask = ~(margin >= np.float32(guard)) | nonfinite
        ge0 = margin >= 0
    bits = margin.view(np.int32)
    min_bits = int(bits[ge0].min()) if ge0.any() else 0x7F800000
    guarded = {(row0 + int(b), int(t)) for b, t in zip(*np.nonzero(guarded_mask))}
    return dict(ids=ids, margin=margin, nonfinite=nonfinite, guarded=guarded, count=len(guarded), min_bits=min(min_bits, 0x7F800000))


# ---- the fp64 re-evaluation ----------------------------------------------------------------------------------------------------------------
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a  # 2^27 + 1 (Veltkamp)
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma64(a, b, c):
    """round(a b + c) with ONE rounding, on fp64 arrays: the device's fma.  (Boldo and Melquiond, "Emulation of FMA and correctly
    rounded sums": exact product and sum by error-free transformations, the two error terms added with rounding to odd, then one
    rounding to nearest.)  No overflow / underflow handling: operands of ordinary magnitude only."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    uh, ul = _two_prod(a, b)
    th, tl = _two_sum(c, uh)
    vh, vl = _two_sum(tl, ul)
    even = (vh.view(np.int64) & 1) == 0
    fix = (vl != 0) & even
    vh = np.where(fix, np.nextafter(vh, np.where(vl > 0, np.inf, -np.inf)), vh)
    return th + vh


def refine64(pos, x, hwt, hb=None, f=None, h=None, w2t=None, b2=None):
    """The kernel's evaluation, sequentially in its order, for the positions pos = [(b, t), ...] -> (n, V) fp64.
    Shallow (f None): xs[c] = float64(x[b, c, t]).  Deep: xs[c] = (sum_j float64(w2t[j, c]) float64(f[b, j, t]) + b2[c]) + h[b, c, t],
    j ascending.  Then a[v] = sum_c float64(hwt[c, v]) xs[c], c ascending, + hb[v].
    Every product of two fp32 values is exact in fp64, so `a + w x` with the sum rounded IS the device's fma there: the deep sum
    over j and the whole shallow form.  The deep form's xs is a full fp64 value: its product with a weight needs up to 77 bits,
    and the device's fma rounds a + w xs once where `a + w * xs` would round twice -- fma64 restates that."""
    n = len(pos)
    bs, ts = np.array([p[0] for p in pos], dtype=np.int64), np.array([p[1] for p in pos], dtype=np.int64)
    hwt = np.asarray(hwt, dtype=np.float32)
    D, V = hwt.shape
    deep = f is not None
    if deep:
        fs = np.asarray(f, np.float32)[bs, :, ts].astype(np.float64)             # (n, F)
        w2 = np.asarray(w2t, np.float32).astype(np.float64)                      # (F, D)
        a = np.zeros((n, D), dtype=np.float64)
        for j in range(w2.shape[0]):
            a = a + w2[j][None, :] * fs[:, j][:, None]
        bias = np.asarray(b2, np.float32).astype(np.float64)[None, :] if b2 is not None else 0.0
        xs = (a + bias) + np.asarray(h, np.float32)[bs, :, ts].astype(np.float64)
    else:
        xs = np.asarray(x, np.float32)[bs, :, ts].astype(np.float64)             # (n, D)
    w = hwt.astype(np.float64)
    acc = np.zeros((n, V), dtype=np.float64)
    for c in range(D):
        if deep:
            acc = fma64(w[c][None, :], xs[:, c][:, None], acc)
        else:
            acc = acc + w[c][None, :] * xs[:, c][:, None]
    return acc + (np.asarray(hb, np.float32).astype(np.float64)[None, :] if hb is not None else 0.0)
