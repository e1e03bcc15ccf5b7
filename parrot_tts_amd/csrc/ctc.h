// ctc.h -- the aligner's validation loss (reference utils/aligner/trainer.py:60-63): torch.nn.CTCLoss() of the log-softmax of the
// logits, and its gradient with respect to the logits (trainer.py:69, loss.backward()).  The loss is two kernels and a reduction:
//   ctc_lse_kernel    one wave per real frame: the fp32 max-shifted log-sum-exp over V
//   ctc_alpha_kernel  one workgroup per utterance: the forward (alpha) recursion over the blank-interleaved states, in fp64
//   ctc_mean_kernel   mean_b(nll[b] / tokens_len[b]) in fp64, in row order
// the gradient reruns the first two with alpha kept (ctc_alpha_kernel<true>) and adds three:
//   ctc_index_kernel  one workgroup per utterance: the token positions sorted by (label, position), and each label's segment
//   ctc_beta_kernel   one workgroup per utterance: the backward (beta) recursion; alpha becomes the log-occupancy in place
//   ctc_grad_kernel   one wave per frame: w (softmax - occupancy per label), fp32, every element of the output
// The launchers below are defined in tu_ctc.hip, which alone sees the kernel bodies (PARROT_CTC_TU).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aligner.h"  // (ALIGN_ST_*, ALIGN_MAX_T, ALIGN_MAX_N)

namespace parrot {

constexpr int CTC_BLOCK = 1024;  // threads of ctc_alpha_kernel at most
constexpr int CTC_KMAX = 5;      // states a thread owns at most: ceil((2 ALIGN_MAX_N + 1) / CTC_BLOCK)
static_assert((2 * ALIGN_MAX_N + 1 + CTC_BLOCK - 1) / CTC_BLOCK <= CTC_KMAX, "a thread's states fit its registers");

// logits (B, T, V) -> lse (B, T) fp64 for t < mel_len[b]; nothing is read or written at or beyond mel_len[b]
hipError_t launch_ctc_lse(const float* logits, const int32_t* mel_len, double* lse, int B, int T, int V, int* status, hipStream_t s);
// -> nll (B) fp64, and mean (1) fp32 when it is not null; alpha (B, T, 2 N + 1) fp64 when it is not null (the same nll bits)
hipError_t launch_ctc_alpha(const float* logits, const int64_t* tokens, const int32_t* mel_len, const int32_t* tokens_len, const double* lse, int B,
                            int T, int V, int N, double* nll, float* mean, double* alpha, int* status, hipStream_t s);
// The gradient's workspace behind the status word and lse: alpha / log-occupancy (B, T, 2 N + 1) fp64, order (B, N), seg_lo and
// seg_hi (B, V) int32.
struct CtcGradWs {
    double* occ;
    int32_t *order, *seg_lo, *seg_hi;
};
// after launch_ctc_lse and launch_ctc_alpha (alpha = ws.occ): -> grad (B, T, V) fp32, every element written
hipError_t launch_ctc_grad(const float* logits, const int64_t* tokens, const int32_t* mel_len, const int32_t* tokens_len, const double* lse,
                           const double* nll, const double* row_weight, int zero_infinity, int B, int T, int V, int N, CtcGradWs ws, float* grad,
                           hipStream_t s);

#ifdef PARROT_CTC_TU

// ---------------------------------------------------------------------------------------------
// ctc_lse_kernel: lse[b][t] = m + logf(sum_v expf(x[v] - m)), m = max_v x[v], the two terms of the reference's fp32 log_softmax
// (trainer.py:61), for the frames t < mel_len[b]: one wave per frame as align_softmax_kernel, the maximum and the sum by a fixed
// lane stride and a fixed xor tree, in fp32.  The two fp32 terms are added in fp64 (exactly) and stored so: the recursion
// subtracts the sum from the fp64 widening of a logit, which leaves logf's rounding as the only error of a log-probability.
// A row whose mel_len is outside [1, T] is skipped whole (ctc_alpha_kernel raises ALIGN_ST_BAD_INPUT for it); a non-finite logit
// of a real frame raises ALIGN_ST_NONFINITE.  grid ceil(B T / 4), 4 waves per workgroup.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ctc_lse_kernel(const float* __restrict__ logits, const int32_t* __restrict__ mel_len, double* __restrict__ lse, int B,
                                                      int T, int V, int* __restrict__ status) {
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (size_t)B * T) return;
    const int b = (int)(row / T), t = (int)(row % T);
    const int len = mel_len[b];
    if (len < 1 || len > T || t >= len) return;
    const float* __restrict__ x = logits + row * V;
    float m = -INFINITY;
    bool bad = false;
    for (int v = lane; v < V; v += 64) {
        const float a = x[v];
        bad |= !(fabsf(a) < INFINITY);
        m = fmaxf(m, a);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    float s = 0.f;
    for (int v = lane; v < V; v += 64) s += expf(x[v] - m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) lse[row] = (double)m + (double)logf(s);
    if (bad) atomicMax(status, ALIGN_ST_NONFINITE);
}

// log(exp(a) + exp(b) [+ exp(c)]) in fp64, shifted by the largest term m: m + log(1 + exp(lo - m) [+ exp(mid - m)]), so the
// largest term's own exp is never formed (two exps, not three).  All terms -inf -> -inf, never NaN: -inf - -inf is not formed.
__device__ __forceinline__ double ctc_logaddexp(double a, double b, double c, bool with_c) {
    const double ninf = __longlong_as_double(0xfff0000000000000LL);
    double m = fmax(a, b);
    const double lo = fmin(a, b);
    double mid = ninf;
    if (with_c) {
        mid = fmin(m, c);
        m = fmax(m, c);
    }
    if (m == ninf) return ninf;
    double sum = 1.0 + exp(lo - m);
    if (with_c) sum += exp(mid - m);
    return m + log(sum);
}

// ---------------------------------------------------------------------------------------------
// ctc_alpha_kernel: -log p(tokens | logits) of utterance b = blockIdx.x with T_b = mel_len[b], N_b = tokens_len[b], as torch's
// CTCLoss computes it (blank = 0, no zero_infinity), over the S = 2 N_b + 1 states blank, tok_0, blank, tok_1, ..., blank:
//   lp[t][c]    = (double)logits[b][t][c] - lse[b][t]
//   alpha_0[0]  = lp[0][blank], alpha_0[1] = lp[0][tok_0], -inf elsewhere
//   alpha_t[s]  = logaddexp(alpha_{t-1}[s], alpha_{t-1}[s-1], alpha_{t-1}[s-2] if s is odd and its token differs from the
//                 previous token) + lp[t][label_s]
//   nll         = -logaddexp(alpha_{T_b-1}[S-1], alpha_{T_b-1}[S-2])          (+inf when no path exists: T_b < N_b + repeats)
// in fp64.  A blank (0) among the tokens is a label like any other, as in torch.
// LDS plan: no state vector in LDS at all (two fp64 vectors of 4097 states would be 65 552 B).  Thread i owns the K =
// ceil(S / blockDim) <= 5 CONTIGUOUS states [i K, i K + K) in registers; per frame it needs two values it does not own, the last
// two states of the thread before it (K == 1: the states of the two threads before it).  Every thread publishes its last two
// states in a double-buffered LDS array (2 x 1024 x 2 fp64 = 32 KiB), so the frame loop has ONE barrier per frame: frame t
// writes half t & 1 while the slowest wave may still read half (t - 1) & 1.  The next frame's logits (one gather per owned state)
// and lse are loaded before the frame's arithmetic and first used after its barrier.
// Every state is computed by the same expression whatever K and blockDim are, so a row's bits do not depend on its batch.
// A token outside [0, V) among the first N_b, or a length outside [1, T] / [1, N], sets ALIGN_ST_BAD_INPUT: nll[b] is NaN and
// nothing is read through the bad value.  blockDim: a multiple of 64, >= min(CTC_BLOCK, 2 N + 1).
// STORE: alpha_t[s] of every real frame and state also goes to alpha[b][t][s] (frame stride 2 N + 1), for ctc_beta_kernel; the
// arithmetic, and so nll, is that of STORE = false.  A bad row stores nothing.
// ---------------------------------------------------------------------------------------------
template <bool STORE>
__global__ __launch_bounds__(CTC_BLOCK) void ctc_alpha_kernel(const float* __restrict__ logits, const int64_t* __restrict__ tokens,
                                                              const int32_t* __restrict__ mel_len, const int32_t* __restrict__ tokens_len,
                                                              const double* __restrict__ lse, int T, int V, int N, double* __restrict__ nll,
                                                              double* __restrict__ alpha, int* __restrict__ status) {
    __shared__ double edge[2][CTC_BLOCK][2];  // [frame parity][thread]{its last state, the one before}
    __shared__ double fin[2];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int Tb = mel_len[b], Nb = tokens_len[b];
    int bad = (Tb < 1 || Tb > T || Nb < 1 || Nb > N) ? 1 : 0;
    const int64_t* __restrict__ tok = tokens + (size_t)b * N;
    if (!bad)
        for (int j = tid; j < Nb; j += nt) {
            const int64_t v = tok[j];
            if (v < 0 || v >= V) bad = 1;
        }
    if (__syncthreads_or(bad)) {
        if (tid == 0) {
            nll[b] = __longlong_as_double(0x7ff8000000000000LL);
            atomicMax(status, ALIGN_ST_BAD_INPUT);
        }
        return;
    }
    const double ninf = __longlong_as_double(0xfff0000000000000LL);
    const int S = 2 * Nb + 1;
    const int K = (S + nt - 1) / nt;
    const int s0 = tid * K;
    int lab[CTC_KMAX];
    bool live[CTC_KMAX], skip[CTC_KMAX];
#pragma unroll
    for (int k = 0; k < CTC_KMAX; ++k) {
        const int s = s0 + k;
        live[k] = k < K && s < S;
        lab[k] = 0;
        skip[k] = false;
        if (live[k] && (s & 1)) {
            const int j = s >> 1;
            lab[k] = (int)tok[j];
            skip[k] = j > 0 && tok[j] != tok[j - 1];
        }
    }
    const float* __restrict__ lb = logits + (size_t)b * T * V;
    const double* __restrict__ lseb = lse + (size_t)b * T;
    float xn[CTC_KMAX];
    double ln;
    auto fetch = [&](int t) {
        ln = lseb[t];
#pragma unroll
        for (int k = 0; k < CTC_KMAX; ++k) xn[k] = live[k] ? lb[(size_t)t * V + lab[k]] : 0.f;
    };
    auto publish = [&](const double* a, int half) {
        double e0 = ninf, e1 = ninf;
#pragma unroll
        for (int k = 0; k < CTC_KMAX; ++k) {
            if (k == K - 1) e0 = a[k];
            if (k == K - 2) e1 = a[k];
        }
        edge[half][tid][0] = e0;
        edge[half][tid][1] = e1;
    };
    const size_t SN = (size_t)2 * N + 1;
    auto store = [&](const double* a, int t) {
        if (!STORE) return;
        double* __restrict__ row = alpha + ((size_t)b * T + t) * SN + s0;
#pragma unroll
        for (int k = 0; k < CTC_KMAX; ++k)
            if (live[k]) row[k] = a[k];
    };
    double a[CTC_KMAX];
    fetch(0);
#pragma unroll
    for (int k = 0; k < CTC_KMAX; ++k) a[k] = (live[k] && s0 + k < 2) ? (double)xn[k] - ln : ninf;
    publish(a, 0);
    store(a, 0);
    if (Tb > 1) fetch(1);
    __syncthreads();
    for (int t = 1; t < Tb; ++t) {
        float xc[CTC_KMAX];
#pragma unroll
        for (int k = 0; k < CTC_KMAX; ++k) xc[k] = xn[k];
        const double lc = ln;
        if (t + 1 < Tb) fetch(t + 1);
        const double(*e)[2] = edge[(t - 1) & 1];
        double p1 = ninf, p2 = ninf;  // alpha_{t-1}[s0 - 1], alpha_{t-1}[s0 - 2]
        if (K == 1) {
            if (tid >= 1) p1 = e[tid - 1][0];
            if (tid >= 2) p2 = e[tid - 2][0];
        } else if (tid >= 1) {
            p1 = e[tid - 1][0];
            p2 = e[tid - 1][1];
        }
#pragma unroll
        for (int k = 0; k < CTC_KMAX; ++k) {
            if (live[k]) {
                const double old = a[k];
                a[k] = ctc_logaddexp(old, p1, p2, skip[k]) + ((double)xc[k] - lc);
                p2 = p1;
                p1 = old;
            }
        }
        publish(a, t & 1);
        store(a, t);
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < CTC_KMAX; ++k) {
        if (live[k] && s0 + k == S - 1) fin[0] = a[k];
        if (live[k] && s0 + k == S - 2) fin[1] = a[k];
    }
    __syncthreads();
    if (tid == 0) nll[b] = -ctc_logaddexp(fin[0], fin[1], ninf, false);  // (-(-inf) = +inf: no path)
}

// ---------------------------------------------------------------------------------------------
// The gradient (trainer.py:69).  With beta the mirror image of alpha,
//   beta_{T_b-1}[S-1] = lp[T_b-1][blank], beta_{T_b-1}[S-2] = lp[T_b-1][label_{S-2}], -inf elsewhere
//   beta_t[s]   = logaddexp(beta_{t+1}[s], beta_{t+1}[s+1], beta_{t+1}[s+2] if state s+2 may be entered by a skip) + lp[t][label_s]
//   gamma_t(v)  = sum_{s : label_s = v} exp(alpha_t[s] + beta_t[s] - lp[t][v] + nll)        (the occupancy of label v at frame t)
//   grad[t][v]  = (float)(w (exp(lp[t][v]) - gamma_t(v)))  for t < T_b,  0 for T_b <= t < T
// is d(w nll) / d logits[t][v], the log-softmax folded in.  A row without a path (nll = +inf) is NaN on its real frames, or zero
// throughout under zero_infinity; a bad row (nll = NaN, ctc_alpha_kernel) is NaN throughout and none of its lengths or tokens is
// used.  No floating-point atomics anywhere: every gamma_t(v) is one lane's sum in a fixed order.
// ---------------------------------------------------------------------------------------------

// ctc_index_kernel: order[b][r], r < N_b: the token positions j stably sorted by (tokens[j], j), by a rank count over the row in
// LDS (N_b <= 2048: 4 Mi comparisons at most); seg_lo / seg_hi[b][v], v < V: the ranks [lo, hi) that hold label v, by bisection
// of the sorted labels.  A bad row is skipped as in ctc_alpha_kernel (the same test), before a token indexes anything.
__global__ __launch_bounds__(CTC_BLOCK) void ctc_index_kernel(const int64_t* __restrict__ tokens, const int32_t* __restrict__ mel_len,
                                                              const int32_t* __restrict__ tokens_len, int T, int V, int N,
                                                              int32_t* __restrict__ order, int32_t* __restrict__ seg_lo,
                                                              int32_t* __restrict__ seg_hi) {
    __shared__ int tk[ALIGN_MAX_N], sorted[ALIGN_MAX_N];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int Tb = mel_len[b], Nb = tokens_len[b];
    int bad = (Tb < 1 || Tb > T || Nb < 1 || Nb > N) ? 1 : 0;
    const int64_t* __restrict__ tok = tokens + (size_t)b * N;
    if (!bad)
        for (int j = tid; j < Nb; j += nt) {
            const int64_t v = tok[j];
            if (v < 0 || v >= V) bad = 1;
            else tk[j] = (int)v;
        }
    if (__syncthreads_or(bad)) return;
    for (int j = tid; j < Nb; j += nt) {
        const int v = tk[j];
        int rank = 0;
        for (int i = 0; i < Nb; ++i) rank += (tk[i] < v || (tk[i] == v && i < j)) ? 1 : 0;
        order[(size_t)b * N + rank] = j;
        sorted[rank] = v;
    }
    __syncthreads();
    for (int v = tid; v < V; v += nt) {
        int lo = 0, hi = Nb;  // the first rank whose label is >= v
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (sorted[mid] < v) lo = mid + 1;
            else hi = mid;
        }
        int end = lo;
        while (end < Nb && sorted[end] == v) ++end;
        seg_lo[(size_t)b * V + v] = lo;
        seg_hi[(size_t)b * V + v] = end;
    }
}

// ctc_beta_kernel: the beta recursion of utterance b = blockIdx.x from frame T_b - 1 down to 0, the mirror image of
// ctc_alpha_kernel: the same ownership of K contiguous states per thread, but a thread needs the FIRST two states of the thread
// after it (K == 1: the states of the two threads after it), published in the same double-buffered LDS array, one barrier per
// frame.  Per frame and owned state it replaces the stored alpha_t[s] by the log-occupancy alpha_t[s] + beta_t[s] - lp[t][label_s]
// + nll (each thread reads and writes its own elements only); alpha, the logits and lse of the next frame down are loaded before
// the frame's arithmetic.  Rows whose nll is NaN (bad) or +inf (no path) are skipped whole: ctc_grad_kernel does not read them.
__global__ __launch_bounds__(CTC_BLOCK) void ctc_beta_kernel(const float* __restrict__ logits, const int64_t* __restrict__ tokens,
                                                             const int32_t* __restrict__ mel_len, const int32_t* __restrict__ tokens_len,
                                                             const double* __restrict__ lse, const double* __restrict__ nll, int T, int V, int N,
                                                             double* __restrict__ occ) {
    __shared__ double edge[2][CTC_BLOCK][2];  // [frame parity][thread]{its first state, the one after}
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const double z = nll[b];
    if (!(fabs(z) < (double)INFINITY)) return;
    const int Tb = mel_len[b], Nb = tokens_len[b];
    const int64_t* __restrict__ tok = tokens + (size_t)b * N;
    const double ninf = __longlong_as_double(0xfff0000000000000LL);
    const int S = 2 * Nb + 1;
    const int K = (S + nt - 1) / nt;
    const int s0 = tid * K;
    int lab[CTC_KMAX];
    bool live[CTC_KMAX], skipn[CTC_KMAX];  // skipn: state s + 2 exists and may be entered from s
#pragma unroll
    for (int k = 0; k < CTC_KMAX; ++k) {
        const int s = s0 + k;
        live[k] = k < K && s < S;
        lab[k] = 0;
        skipn[k] = false;
        if (live[k] && (s & 1)) {
            const int j = s >> 1;
            lab[k] = (int)tok[j];
            skipn[k] = j + 1 < Nb && tok[j + 1] != tok[j];
        }
    }
    const size_t SN = (size_t)2 * N + 1;
    const float* __restrict__ lb = logits + (size_t)b * T * V;
    const double* __restrict__ lseb = lse + (size_t)b * T;
    double* __restrict__ ob = occ + (size_t)b * T * SN + s0;
    float xn[CTC_KMAX];
    double an[CTC_KMAX], ln;
    auto fetch = [&](int t) {
        ln = lseb[t];
#pragma unroll
        for (int k = 0; k < CTC_KMAX; ++k) {
            xn[k] = live[k] ? lb[(size_t)t * V + lab[k]] : 0.f;
            an[k] = live[k] ? ob[(size_t)t * SN + k] : 0.0;
        }
    };
    double bt[CTC_KMAX];
    auto publish = [&](int half) {
        edge[half][tid][0] = bt[0];
        edge[half][tid][1] = bt[1];  // (-inf when the thread owns one state: bt[k] stays -inf for k >= K)
    };
    auto occupancy = [&](int t, const float* x, const double* al, double l) {
#pragma unroll
        for (int k = 0; k < CTC_KMAX; ++k)
            if (live[k]) ob[(size_t)t * SN + k] = al[k] + bt[k] - ((double)x[k] - l) + z;
    };
    fetch(Tb - 1);
#pragma unroll
    for (int k = 0; k < CTC_KMAX; ++k) bt[k] = (live[k] && s0 + k >= S - 2) ? (double)xn[k] - ln : ninf;
    publish((Tb - 1) & 1);
    occupancy(Tb - 1, xn, an, ln);
    if (Tb > 1) fetch(Tb - 2);
    __syncthreads();
    for (int t = Tb - 2; t >= 0; --t) {
        float xc[CTC_KMAX];
        double ac[CTC_KMAX];
#pragma unroll
        for (int k = 0; k < CTC_KMAX; ++k) {
            xc[k] = xn[k];
            ac[k] = an[k];
        }
        const double lc = ln;
        if (t > 0) fetch(t - 1);
        const double(*e)[2] = edge[(t + 1) & 1];
        double n1 = ninf, n2 = ninf;  // beta_{t+1}[s + 1], beta_{t+1}[s + 2] of the thread's last state s
        if (K == 1) {
            if (tid + 1 < nt) n1 = e[tid + 1][0];
            if (tid + 2 < nt) n2 = e[tid + 2][0];
        } else if (tid + 1 < nt) {
            n1 = e[tid + 1][0];
            n2 = e[tid + 1][1];
        }
#pragma unroll
        for (int k = CTC_KMAX - 1; k >= 0; --k) {
            if (live[k]) {
                const double old = bt[k];
                bt[k] = ctc_logaddexp(old, n1, n2, skipn[k]) + ((double)xc[k] - lc);
                n2 = n1;
                n1 = old;
            }
        }
        publish(t & 1);
        occupancy(t, xc, ac, lc);
        __syncthreads();
    }
}

// ctc_grad_kernel: one wave per (b, t) as ctc_lse_kernel, every element of grad[b][t][:] written once.  gamma_t(blank) starts
// from the N_b + 1 even states, summed by the wave with a fixed lane stride and a fixed xor tree (every lane holds the same
// bits); then lane v % 64 adds the states of label v in the order of ctc_index_kernel, one after the other, in fp64.  The order
// depends on the row's tokens alone, so a row's bits depend on that row, T and V only.  grid ceil(B T / 4), 4 waves per workgroup.
__global__ __launch_bounds__(256) void ctc_grad_kernel(const float* __restrict__ logits, const int32_t* __restrict__ mel_len,
                                                       const int32_t* __restrict__ tokens_len, const double* __restrict__ lse,
                                                       const double* __restrict__ nll, const double* __restrict__ occ,
                                                       const int32_t* __restrict__ order, const int32_t* __restrict__ seg_lo,
                                                       const int32_t* __restrict__ seg_hi, const double* __restrict__ row_weight, int zero_infinity,
                                                       int B, int T, int V, int N, float* __restrict__ grad) {
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (size_t)B * T) return;
    const int b = (int)(row / T), t = (int)(row % T);
    float* __restrict__ g = grad + row * V;
    const double z = nll[b];
    float fill = 0.f;
    bool plain = false;
    if (z != z) {
        fill = __int_as_float(0x7fc00000);  // a bad row: NaN throughout, its lengths are not used
    } else if (t < mel_len[b]) {
        if (z < (double)INFINITY) plain = true;
        else if (!zero_infinity) fill = __int_as_float(0x7fc00000);  // no path: NaN on the real frames
    }
    if (!plain) {
        for (int v = lane; v < V; v += 64) g[v] = fill;
        return;
    }
    const int Nb = tokens_len[b];
    const double w = row_weight ? row_weight[b] : 1.0;
    const double* __restrict__ o = occ + row * ((size_t)2 * N + 1);
    double gb = 0.0;
    for (int j = lane; j <= Nb; j += 64) gb += exp(o[2 * j]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) gb += __shfl_xor(gb, off);
    const float* __restrict__ x = logits + row * V;
    const double l = lse[row];
    const int32_t* __restrict__ ord = order + (size_t)b * N;
    for (int v = lane; v < V; v += 64) {
        double gam = v == 0 ? gb : 0.0;
        const int hi = seg_hi[(size_t)b * V + v];
        for (int r = seg_lo[(size_t)b * V + v]; r < hi; ++r) gam += exp(o[2 * ord[r] + 1]);
        g[v] = (float)(w * (exp((double)x[v] - l) - gam));
    }
}

// ---------------------------------------------------------------------------------------------
// ctc_mean_kernel: torch's reduction='mean', mean_b(nll[b] / tokens_len[b]), one thread, fp64, in row order, rounded to fp32 once.
// (A bad row's nll is NaN whatever its tokens_len is, and so is the mean.)
// ---------------------------------------------------------------------------------------------
__global__ void ctc_mean_kernel(const double* __restrict__ nll, const int32_t* __restrict__ tokens_len, int B, float* __restrict__ mean) {
    if (blockIdx.x || threadIdx.x) return;
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += nll[b] / (double)tokens_len[b];
    *mean = (float)(s / (double)B);
}

#endif  // PARROT_CTC_TU

}  // namespace parrot
