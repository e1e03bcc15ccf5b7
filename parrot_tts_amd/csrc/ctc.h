// ctc.h -- the aligner's validation loss (reference utils/aligner/trainer.py:60-63): torch.nn.CTCLoss() of the log-softmax of the
// logits, forward pass only.  Two kernels and a reduction:
//   ctc_lse_kernel    one wave per real frame: the fp32 max-shifted log-sum-exp over V
//   ctc_alpha_kernel  one workgroup per utterance: the forward (alpha) recursion over the blank-interleaved states, in fp64
//   ctc_mean_kernel   mean_b(nll[b] / tokens_len[b]) in fp64, in row order
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
// -> nll (B) fp64, and mean (1) fp32 when it is not null
hipError_t launch_ctc_alpha(const float* logits, const int64_t* tokens, const int32_t* mel_len, const int32_t* tokens_len, const double* lse, int B,
                            int T, int V, int N, double* nll, float* mean, int* status, hipStream_t s);

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
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CTC_BLOCK) void ctc_alpha_kernel(const float* __restrict__ logits, const int64_t* __restrict__ tokens,
                                                              const int32_t* __restrict__ mel_len, const int32_t* __restrict__ tokens_len,
                                                              const double* __restrict__ lse, int T, int V, int N, double* __restrict__ nll,
                                                              int* __restrict__ status) {
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
    double a[CTC_KMAX];
    fetch(0);
#pragma unroll
    for (int k = 0; k < CTC_KMAX; ++k) a[k] = (live[k] && s0 + k < 2) ? (double)xn[k] - ln : ninf;
    publish(a, 0);
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
