"""Plain numpy restatement of the aligner's training kernels (parrot_tts_amd/csrc/train_gemm.h, aligner_train.h), one function per kernel, each
evaluating the kernel's documented formula on the strided buffers a descriptor names -- and the descriptors themselves: the
parameter sets parrot_tts_amd/csrc/host_aligner_train.hip builds, written once as functions of the problem sizes.

A tap-GEMM or weight-gradient set is a dict of the kernel's sizes, strides, shifts and offsets (the names of TapGemmParams /
WgradParams) plus the element counts of the buffers of the model it stands for (``a_size`` ...) and the element offsets at which
the model hands a buffer in (``x_base``, ``c_base``, ``y_base``; per tap ``a_off``).  Buffers are flat arrays.  Sums are int64 on
integer data (exact) and fp64 otherwise; the BatchNorm pair uses the documented mix: fp64 sums, each rounded once to ``ft``
(np.float32: what the kernels do; np.float64: the form tests/test_aligner_train_kernels_cpu.py pins against torch), then the
elementwise formula in single ``ft`` operations."""
import math

import numpy as np

MAX_TAPS = 5
RCHUNK = 256     # TG_RCHUNK: (b, t) pairs per fp32 partial of wgrad_kernel
PASS_K = 32      # k per staging pass of tap_gemm_kernel
ACC_FLUSH = 8    # TG_ACC_FLUSH
U32 = 2.0 ** -24


# =========================================================================================================================================
# the layouts of host_aligner_train.hip, in the GEMM's own sizes (M x K times K x N, Z batch rows) ...
# =========================================================================================================================================
def tg_conv(M, N, K, Z, first: bool, relu=1):
    """Conv forward, k = 5, pad 2 (the conv blocks of parrot_aligner_train_forward, host_aligner_train.hip): weight (M, K, 5), tap j at w + j, shift j - 2; input the mel
    (Z, N, K) read transposed (``first``) or channel-first (Z, K, N); output channel-first (Z, M, N), ReLU."""
    x = dict(x_sz=N * K, x_sk=1, x_sn=K) if first else dict(x_sz=K * N, x_sk=N, x_sn=1)
    return dict(ntaps=5, a_off=list(range(5)), x_off=[0] * 5, shift=[j - 2 for j in range(5)], M=M, N=N, K=K, Z=Z, a_sm=K * 5, a_sk=5,
                c_sz=M * N, c_sm=N, c_sn=1, bias=0, relu=relu, x_base=0, c_base=0, a_size=M * K * 5, x_size=Z * K * N, c_size=Z * M * N, **x)


def tg_xproj(M, N, K, Z, d: int):
    """LSTM input projection of direction d (:174-179): W_ih (M, K) on the channel-first (Z, K, N), + (b_ih + b_hh), written as the
    d-th half of the rows of (Z, N, 2M)."""
    return dict(ntaps=1, a_off=[0], x_off=[0], shift=[0], M=M, N=N, K=K, Z=Z, a_sm=K, a_sk=1, x_sz=K * N, x_sk=N, x_sn=1, c_sz=N * 2 * M,
                c_sm=1, c_sn=2 * M, bias=2, relu=0, x_base=0, c_base=d * M, a_size=M * K, x_size=Z * K * N, c_size=Z * N * 2 * M)


def tg_linear(M, N, K, Z):
    """Linear (:193-195): lin_w (M, K) on (Z, N, K), + lin_b, written (Z, N, M)."""
    return dict(ntaps=1, a_off=[0], x_off=[0], shift=[0], M=M, N=N, K=K, Z=Z, a_sm=K, a_sk=1, x_sz=N * K, x_sk=1, x_sn=K, c_sz=N * M,
                c_sm=1, c_sn=M, bias=1, relu=0, x_base=0, c_base=0, a_size=M * K, x_size=Z * N * K, c_size=Z * N * M)


def tg_dlstm(M, N, K, Z):
    """Linear data gradient (:241): lin_w (K, M) read transposed on grad_logits (Z, N, K), written (Z, N, M)."""
    return dict(ntaps=1, a_off=[0], x_off=[0], shift=[0], M=M, N=N, K=K, Z=Z, a_sm=1, a_sk=M, x_sz=N * K, x_sk=1, x_sn=K, c_sz=N * M,
                c_sm=1, c_sn=M, bias=0, relu=0, x_base=0, c_base=0, a_size=K * M, x_size=Z * N * K, c_size=Z * N * M)


def tg_dy2(M, N, K, Z):
    """Gradient at the third block's output (:270-276): two taps without a shift, W_ih and W_ih_reverse (K, M each, here one after
    the other in one buffer) read transposed, each on its half (x_off K) of the rows of dgates (Z, N, 2K); written (Z, M, N)."""
    return dict(ntaps=2, a_off=[0, K * M], x_off=[0, K], shift=[0, 0], M=M, N=N, K=K, Z=Z, a_sm=1, a_sk=M, x_sz=N * 2 * K, x_sk=1,
                x_sn=2 * K, c_sz=M * N, c_sm=N, c_sn=1, bias=0, relu=0, x_base=0, c_base=0, a_size=2 * K * M, x_size=Z * N * 2 * K,
                c_size=Z * M * N)


def tg_dgrad(M, N, K, Z):
    """Conv data gradient (:296-306): weight (K, M, 5) read transposed, tap j at w + j with the flipped shift 2 - j, on the
    channel-first (Z, K, N); written (Z, M, N)."""
    return dict(ntaps=5, a_off=list(range(5)), x_off=[0] * 5, shift=[2 - j for j in range(5)], M=M, N=N, K=K, Z=Z, a_sm=5, a_sk=M * 5,
                x_sz=K * N, x_sk=N, x_sn=1, c_sz=M * N, c_sm=N, c_sn=1, bias=0, relu=0, x_base=0, c_base=0, a_size=K * M * 5,
                x_size=Z * K * N, c_size=Z * M * N)


def wg_linear(M, K, B, T):
    """lin_w gradient (:233-239): dY = grad_logits (B, T, M), X = the LSTM output (B, T, K); out (M, K)."""
    return dict(ntaps=1, shift=[0], M=M, K=K, T=T, R=B * T, y_sz=T * M, y_sm=1, y_st=M, x_sz=T * K, x_sk=1, x_st=K, o_sm=K, o_sk=1, o_sj=0,
                y_base=0, x_base=0, y_size=B * T * M, x_size=B * T * K, o_size=M * K)


def wg_w_ih(M, K, B, T, d: int):
    """W_ih gradient of direction d (:257-263): dY = the d-th half of the rows of dgates (B, T, 2M), X channel-first (B, K, T)."""
    return dict(ntaps=1, shift=[0], M=M, K=K, T=T, R=B * T, y_sz=T * 2 * M, y_sm=1, y_st=2 * M, x_sz=K * T, x_sk=T, x_st=1, o_sm=K, o_sk=1,
                o_sj=0, y_base=d * M, x_base=0, y_size=B * T * 2 * M, x_size=B * K * T, o_size=M * K)


def wg_w_hh(M, K, B, T, d: int):
    """W_hh gradient of direction d (:264-268): X = the d-th half of the LSTM output (B, T, 2K) at the step before t: shift -1
    forward, +1 backward; the zero fill is h_0 = 0."""
    return dict(ntaps=1, shift=[1 if d else -1], M=M, K=K, T=T, R=B * T, y_sz=T * 2 * M, y_sm=1, y_st=2 * M, x_sz=T * 2 * K, x_sk=1,
                x_st=2 * K, o_sm=K, o_sk=1, o_sj=0, y_base=d * M, x_base=d * K, y_size=B * T * 2 * M, x_size=B * T * 2 * K, o_size=M * K)


def wg_conv(M, K, B, T, first: bool):
    """Conv weight gradient (:286-294): dY channel-first (B, M, T); X the mel (B, T, K) (``first``) or channel-first (B, K, T);
    five taps, shift j - 2, out (M, K, 5)."""
    x = dict(x_sz=T * K, x_sk=1, x_st=K) if first else dict(x_sz=K * T, x_sk=T, x_st=1)
    return dict(ntaps=5, shift=[j - 2 for j in range(5)], M=M, K=K, T=T, R=B * T, y_sz=M * T, y_sm=T, y_st=1, o_sm=K * 5, o_sk=5, o_sj=1,
                y_base=0, x_base=0, y_size=B * M * T, x_size=B * K * T, o_size=M * K * 5, **x)


# ... and at the model's sizes: every launch of the two entry points
def host_tap_gemm_sets(B, T, F, D, H, V):
    s = {"conv0": tg_conv(D, T, F, B, True), "conv1": tg_conv(D, T, D, B, False)}
    for d in (0, 1):
        s[f"xproj{d}"] = tg_xproj(4 * H, T, D, B, d)
    s["linear"] = tg_linear(V, T, 2 * H, B)
    s["dlstm"] = tg_dlstm(2 * H, T, V, B)
    s["dy2"] = tg_dy2(D, T, 4 * H, B)
    s["dgrad"] = tg_dgrad(D, T, D, B)
    return s


def host_wgrad_sets(B, T, F, D, H, V):
    s = {"linear": wg_linear(V, 2 * H, B, T)}
    for d in (0, 1):
        s[f"w_ih{d}"] = wg_w_ih(4 * H, D, B, T, d)
        s[f"w_hh{d}"] = wg_w_hh(4 * H, H, B, T, d)
    s["conv0"] = wg_conv(D, F, B, T, True)
    s["conv1"] = wg_conv(D, D, B, T, False)
    return s


def passes(p) -> int:
    """32-wide staging passes of tap_gemm_kernel: the accumulator is flushed after every ACC_FLUSH of them."""
    return p["ntaps"] * ((p["K"] + PASS_K - 1) // PASS_K)


# =========================================================================================================================================
# the kernels
# =========================================================================================================================================
def _acc_type(*arrays):
    return np.int64 if all(np.issubdtype(a.dtype, np.integer) for a in arrays if a is not None) else np.float64


def tap_gemm(p, A, X, c_init, bias0=None, bias1=None, want_bound=False):
    """C[z][m][n] = act(sum_j sum_k A_j[m][k] X[z][k][n + shift_j] + bias0[m] + bias1[m]) scattered into a copy of the flat
    ``c_init``; X is zero outside 0 <= n + shift_j < N.  ``want_bound``: also (sum |a||x| + |bias|, number of products) per
    (z, m, n), shaped (Z, M, N) and (N,)."""
    dt = _acc_type(A, X, bias0, bias1)
    M, N, K, Z = p["M"], p["N"], p["K"], p["Z"]
    m, k, n, z = np.arange(M), np.arange(K), np.arange(N), np.arange(Z)
    acc = np.zeros((Z, M, N), dt)
    mag = np.zeros((Z, M, N), np.float64)
    cnt = np.zeros((N,), np.int64)
    for j in range(p["ntaps"]):
        Aj = A[p["a_off"][j] + m[:, None] * p["a_sm"] + k[None, :] * p["a_sk"]].astype(dt)
        tn = n + p["shift"][j]
        ok = (tn >= 0) & (tn < N)
        idx = p["x_base"] + p["x_off"][j] + z[:, None, None] * p["x_sz"] + k[None, :, None] * p["x_sk"] + np.where(ok, tn, 0)[None, None, :] * p["x_sn"]
        Xj = np.where(ok[None, None, :], X[idx], 0).astype(dt)
        acc += np.matmul(Aj, Xj)
        if want_bound:
            mag += np.matmul(np.abs(Aj).astype(np.float64), np.abs(Xj).astype(np.float64))
            cnt += ok * K
    if bias0 is not None:
        if bias1 is not None:  # (added to bias0 first, in the data's own precision: b_ih + b_hh)
            b = bias0[:M] + bias1[:M]
        else:
            b = bias0[:M]
        acc = acc + b.astype(dt)[None, :, None]
        mag += np.abs(b.astype(np.float64))[None, :, None]
    if p["relu"]:
        acc = np.where(acc < 0, 0, acc)  # (a NaN stays a NaN)
    out = c_init.copy()
    out[p["c_base"] + z[:, None, None] * p["c_sz"] + m[None, :, None] * p["c_sm"] + n[None, None, :] * p["c_sn"]] = acc
    return (out, mag, cnt) if want_bound else out


def wgrad(p, dY, X, o_init, want_bound=False):
    """out[m o_sm + k o_sk + j o_sj] = sum_(b, t) dY[b][m][t] X[b][k][t + shift_j]; X is zero outside 0 <= t + shift_j < T."""
    dt = _acc_type(dY, X)
    M, K, T = p["M"], p["K"], p["T"]
    B = p["R"] // T
    assert B * T == p["R"]
    m, k, t, b = np.arange(M), np.arange(K), np.arange(T), np.arange(B)
    Y = dY[p["y_base"] + b[:, None, None] * p["y_sz"] + m[None, :, None] * p["y_sm"] + t[None, None, :] * p["y_st"]].astype(dt)
    out = o_init.copy()
    mags = []
    for j in range(p["ntaps"]):
        tt = t + p["shift"][j]
        ok = (tt >= 0) & (tt < T)
        idx = p["x_base"] + b[:, None, None] * p["x_sz"] + k[None, :, None] * p["x_sk"] + np.where(ok, tt, 0)[None, None, :] * p["x_st"]
        Xj = np.where(ok[None, None, :], X[idx], 0).astype(dt)
        out[m[:, None] * p["o_sm"] + k[None, :] * p["o_sk"] + j * p["o_sj"]] = np.einsum("bmt,bkt->mk", Y, Xj)
        if want_bound:
            mags.append(np.einsum("bmt,bkt->mk", np.abs(Y).astype(np.float64), np.abs(Xj).astype(np.float64)))
    return (out, mags) if want_bound else out


def colsum(src, R, M, ld, base=0):
    """out[m] = sum_r src[base + r ld + m]: int64 on integer data, else the correctly rounded sum (math.fsum) as fp64."""
    S = src[base + np.arange(R)[:, None] * ld + np.arange(M)[None, :]]
    if np.issubdtype(S.dtype, np.integer):
        return S.astype(np.int64).sum(axis=0)
    return np.array([math.fsum(S[:, i].astype(np.float64)) for i in range(M)], np.float64)


def bn_stats(x, run_mean, run_var, eps, ft=np.float32):
    """Batch statistics of x (B, C, T) as bn_train_kernel documents them: fp64 sums over the n = B T values of a channel, biased
    variance about the fp64 mean; mean and 1 / sqrt(var + eps) rounded once to ``ft``; the running buffers' update formed in fp64
    (unbiased variance) and rounded once.  -> mean, invstd, new run_mean, new run_var."""
    B, C, T = x.shape
    n = B * T
    x64 = x.astype(np.float64).transpose(1, 0, 2).reshape(C, n)
    mean = x64.sum(axis=1) / n
    var = ((x64 - mean[:, None]) ** 2).sum(axis=1) / n
    invstd = 1.0 / np.sqrt(var + np.float64(ft(eps)))
    rm = 0.9 * run_mean.astype(np.float64) + 0.1 * mean
    rv = 0.9 * run_var.astype(np.float64) + 0.1 * (var * n / (n - 1))
    return mean.astype(ft), invstd.astype(ft), rm.astype(ft), rv.astype(ft)


def bn_eval_stats(run_mean, run_var, eps, ft=np.float32):
    """training = 0: the running mean as it stands and fl(1 / sqrt(var + eps)) formed in fp64."""
    return run_mean.astype(ft), (1.0 / np.sqrt(run_var.astype(np.float64) + np.float64(ft(eps)))).astype(ft)


def bn_apply(x, mean, invstd, gamma, beta, ft=np.float32):
    """y = fma(fl(fl(x - mean) invstd), gamma, beta) in ``ft``.  The product of two fp32 numbers is exact in fp64, so the fma is the
    fp64 sum rounded to fp32: a double rounding, within 1 ulp of the fused result (and equal to it but on a tie of the second)."""
    c = (None, slice(None), None)
    xh = ((x.astype(ft) - mean.astype(ft)[c]).astype(ft) * invstd.astype(ft)[c]).astype(ft)
    return (xh.astype(np.float64) * gamma.astype(np.float64)[c] + beta.astype(np.float64)[c]).astype(ft)


def bn_train(x, gamma, beta, run_mean, run_var, eps, training=True, ft=np.float32):
    """-> dict(y, mean, invstd, run_mean, run_var) of bn_train_kernel."""
    if training:
        mean, invstd, rm, rv = bn_stats(x, run_mean, run_var, eps, ft)
    else:
        mean, invstd = bn_eval_stats(run_mean, run_var, eps, ft)
        rm, rv = run_mean.astype(ft), run_var.astype(ft)
    return dict(y=bn_apply(x, mean, invstd, gamma, beta, ft), mean=mean, invstd=invstd, run_mean=rm, run_var=rv)


def bn_xhat(x, mean, invstd, ft=np.float32):
    c = (None, slice(None), None)
    return ((x.astype(ft) - mean.astype(ft)[c]).astype(ft) * invstd.astype(ft)[c]).astype(ft)


def bn_bwd_sums(dy, x, mean, invstd, ft=np.float32):
    """(sum dy, sum dy xh) per channel in fp64, xh in single ``ft`` operations."""
    xh = bn_xhat(x, mean, invstd, ft)
    d = dy.astype(np.float64)
    return d.sum(axis=(0, 2)), (d * xh.astype(np.float64)).sum(axis=(0, 2))


def bn_bwd_apply(dy, x, gamma, mean, invstd, m1, m2, ft=np.float32):
    """dx = (gamma invstd) ((dy - m1) - xh m2) where x > 0, +0 elsewhere; every operation a single ``ft`` one.  m1, m2 (C)."""
    c = (None, slice(None), None)
    xh = bn_xhat(x, mean, invstd, ft)
    k = (gamma.astype(ft) * invstd.astype(ft)).astype(ft)
    a = (dy.astype(ft) - m1.astype(ft)[c]).astype(ft)
    v = (k[c] * (a - (xh * m2.astype(ft)[c]).astype(ft)).astype(ft)).astype(ft)
    return np.where(x > 0, v, ft(0))


def bn_relu_bwd(dy, x, gamma, mean, invstd, ft=np.float32):
    """-> dict(dx, dgamma, dbeta) of bn_relu_bwd_kernel: the two sums rounded once to ``ft``, and once more after the division by n."""
    n = x.shape[0] * x.shape[2]
    s1, s2 = bn_bwd_sums(dy, x, mean, invstd, ft)
    return dict(dx=bn_bwd_apply(dy, x, gamma, mean, invstd, (s1 / n).astype(ft), (s2 / n).astype(ft), ft), dgamma=s2.astype(ft), dbeta=s1.astype(ft))


# =========================================================================================================================================
# bounds and shape samples shared by the CPU and GPU tests
# =========================================================================================================================================
def gamma_n(n, u=U32):
    """Higham's gamma_n = n u / (1 - n u): the forward bound of n roundings to nearest of unit roundoff u."""
    n = np.asarray(n, np.float64)
    return n * u / (1.0 - n * u)


SIZES = (1, 31, 32, 33, 63, 64, 65, 130)


def sample_triples(count=40, seed=7):
    """``count`` (M, N, K) triples over SIZES, seeded, every value in every position: the first len(SIZES) rows are three
    independent permutations side by side, the rest are drawn freely."""
    rng = np.random.Generator(np.random.PCG64(seed))
    cols = [rng.permutation(len(SIZES)) for _ in range(3)]
    rows = [tuple(SIZES[c[i]] for c in cols) for i in range(len(SIZES))]
    while len(rows) < count:
        t = tuple(int(SIZES[i]) for i in rng.integers(0, len(SIZES), size=3))
        if t not in rows:
            rows.append(t)
    return rows
