// tte_train.h -- the kernels that TRAIN the text-to-unit model (reference modules/parrot.py:90-110 with inference=False under
// model.train(), and the backward of that graph): parrot_tte_train_forward / _backward (host_tte_train.hip).  Everything is
// channel-last, (rows, C) with rows = b T + t, as torch holds it.  The matrix products are not here: the Linear layers and the convs
// go through train_gemm.h, QK^T, PV and their five gradient products through bgemm_mfma_kernel (attn.h), all on
// v_mfma_f32_32x32x2_f32.  This file holds what lies between them:
//   ln_fwd_kernel            LayerNorm over C keeping the row's mean and rstd
//   ln_bwd_kernel            its data gradient (+ a residual, x an optional ReLU mask) and dy xhat, whose column sums are dgamma
//   softmax_drop_fwd_kernel  key-masked row softmax P, and P with dropout
//   softmax_drop_bwd_kernel  dS = P (dP - sum_k dP_k P_k), dP the dropout's backward of the incoming gradient
//   dropout_kernel           y = keep ? x / (1 - p) : 0 (forward, and backward on the gradient); relu_bwd_kernel; add / mask kernels
//   tt_embed_kernel, tt_add_speaker_kernel, dur_cum_kernel, lr_fwd_kernel, lr_bwd_kernel, embed_grad_kernel
// Rules, as in train_gemm.h: no floating-point atomics; every sum over rows that ends in one number is fp64 in a fixed order;
// nothing clamps with fmaxf, so a NaN stays a NaN.
//
// DROPOUT BITS.  Element i of dropout site `site` under (seed, offset) is kept iff
//     philox4x32_10(counter = {lo32(i), hi32(i), lo32(offset), (hi32(offset) & 0xffffff) | site << 24}, key = {lo32(seed), hi32(seed)})[0] >> 8
//         >= floor(p 2^24 + 0.5)                                                  (p 2^24 formed in fp64 from the fp32 p)
// so p = 0 keeps everything and p = 1 nothing; a survivor is multiplied by the fp32 quotient 1 / (1 - p).  Sites: 0 and 1 are the
// duration predictor's two dropouts (i = (b S + s) NF + c), 2 + l the attention of encoder block l, 2 + enc_layers + l of decoder
// block l (i = ((b H + h) T + tq) T + tk).  The mask depends on nothing else, and the backward regenerates it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wave_reduce.h"

namespace parrot {

struct DropArgs {
    float p;          // 0 <= p <= 1; p == 0 generates nothing
    uint64_t seed, offset;
    int site;
};

struct BgemmTrainParams {  // BgemmParams of attn.h, declared here for the host unit
    const float* A;
    const float* B;
    float* C;
    int M, N, K;
    long a_sk, a_sm, b_sk, b_sn, a_zb, a_zh, b_zb, b_zh, c_zb, c_zh, ldc;
    int H;
    float alpha;
};
// C[b, h](m, n) = sum_k (alpha A[b, h](k, m)) B[b, h](k, n); Z = batch x heads
hipError_t tt_launch_bgemm(const BgemmTrainParams& p, int Z, hipStream_t s);
hipError_t tt_launch_ln_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, long rows, int C, hipStream_t s);
// dx = rstd (g - mean(g) - xhat mean(g xhat)) with g = dy gamma, + res (nullable), zeroed where relu_mask and x <= 0; dyxh = dy xhat
hipError_t tt_launch_ln_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, const float* res, float* dx,
                            float* dyxh, long rows, int C, int relu_mask, hipStream_t s);
// s (rows, T) scores in, P out in place; pd (nullable): P after dropout.  key_valid (B, T), row r belongs to batch r / HT
hipError_t tt_launch_softmax_fwd(float* s, float* pd, const uint8_t* key_valid, long rows, int T, int HT, DropArgs d, hipStream_t s_);
hipError_t tt_launch_softmax_bwd(const float* P, float* dP, long rows, int T, DropArgs d, hipStream_t s);
hipError_t tt_launch_dropout(const float* x, float* y, size_t n, DropArgs d, hipStream_t s);
hipError_t tt_launch_dropout_mask(uint8_t* out, size_t n, DropArgs d, hipStream_t s);
hipError_t tt_launch_relu_bwd(const float* y, const float* dy, float* dx, size_t n, hipStream_t s);  // dx = y > 0 ? dy : 0
hipError_t tt_launch_add(const float* a, const float* b, float* y, size_t n, hipStream_t s);
hipError_t tt_launch_mask(const float* x, const uint8_t* valid, float* y, size_t n, hipStream_t s);  // y = valid ? x : 0
// x[r][c] = tok_emb[phones[r]][c] + pe_row[c]; an id outside [0, vocab) gives NaN (nothing is indexed through it)
hipError_t tt_launch_embed(const int64_t* phones, const float* tok_emb, const float* pe_row, float* x, long rows, int D, int vocab, hipStream_t s);
hipError_t tt_launch_add_speaker(const float* x, const int64_t* speaker, const float* tab, float* y, int B, int S, int D, int n_speaker, hipStream_t s);
// cum (B, S + 1): prefix sums of the durations, every term and every sum saturated into [0, L]
hipError_t tt_launch_dur_cum(const int64_t* dur, int32_t* cum, int B, int S, int L, hipStream_t s);
// y[b][t] = (t < cum[b][S] ? enc[b][s(t)] : 0) + pe_row, s(t) the position whose segment [cum[s], cum[s + 1]) holds t
hipError_t tt_launch_lr_fwd(const float* enc, const int32_t* cum, const float* pe_row, float* y, int B, int S, int L, int D, hipStream_t s);
// denc[b][s] = fl32(sum of dy[b][t] over the segment, ascending t, fp64) + add (nullable); an empty segment gives exactly 0 (+ add)
hipError_t tt_launch_lr_bwd(const float* dy, const int32_t* cum, const float* add, float* denc, int B, int S, int L, int D, hipStream_t s);
// dtab[v][c] = fl32(sum over r, ascending, of [ids[r / per] == v] dx[r][c], fp64); row pad_idx (if >= 0) is exactly 0
hipError_t tt_launch_embed_grad(const int64_t* ids, const float* dx, float* dtab, long rows, int per, int D, int V, int pad_idx, hipStream_t s);

#ifdef PARROT_TTE_TRAIN_TU

__device__ __forceinline__ uint32_t philox4x32_10_word0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}
__device__ __forceinline__ uint32_t drop_threshold(float p) { return (uint32_t)floor((double)p * 16777216.0 + 0.5); }
__device__ __forceinline__ bool drop_keep(const DropArgs& d, uint32_t thr, uint64_t i) {
    const uint32_t w = philox4x32_10_word0((uint32_t)i, (uint32_t)(i >> 32), (uint32_t)d.offset,
                                           ((uint32_t)(d.offset >> 32) & 0xffffffu) | ((uint32_t)d.site << 24), (uint32_t)d.seed,
                                           (uint32_t)(d.seed >> 32));
    return (w >> 8) >= thr;
}
// max that keeps a NaN (fmaxf would drop it)
__device__ __forceinline__ float nan_max(float a, float b) { return (b > a || b != b) ? b : a; }

// One wave per row, four rows per workgroup.  mean and the biased variance in two passes, summed in fp64 (lane l adds c = l, l + 64,
// ... then the xor tree); both and rstd = 1 / sqrt(var + 1e-5) are rounded to fp32 once and kept for the backward.
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     float* __restrict__ y, float* __restrict__ mean, float* __restrict__ rstd, long rows, int C) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + row * C;
    double s = 0.0;
    for (int c = lane; c < C; c += 64) s += (double)xr[c];
    const double md = wave_sum(s) / (double)C;
    s = 0.0;
    for (int c = lane; c < C; c += 64) {
        const double d = (double)xr[c] - md;
        s += d * d;
    }
    const float m = (float)md, r = (float)(1.0 / sqrt(wave_sum(s) / (double)C + 1e-5));
    if (lane == 0) {
        mean[row] = m;
        rstd[row] = r;
    }
    float* yr = y + row * C;
    for (int c = lane; c < C; c += 64) yr[c] = fmaf((xr[c] - m) * r, gamma[c], beta[c]);
}

__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ gamma,
                                                     const float* __restrict__ mean, const float* __restrict__ rstd, const float* res, float* dx,
                                                     float* __restrict__ dyxh, long rows, int C, int relu_mask) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + row * C;
    const float* dr = dy + row * C;
    const float m = mean[row], r = rstd[row];
    double a1 = 0.0, a2 = 0.0;  // the two row means, summed in fp64 and rounded once
    for (int c = lane; c < C; c += 64) {
        const float xh = (xr[c] - m) * r, g = dr[c] * gamma[c];
        a1 += (double)g;
        a2 += (double)g * (double)xh;
    }
    const float s1 = (float)(wave_sum(a1) / (double)C), s2 = (float)(wave_sum(a2) / (double)C);
    for (int c = lane; c < C; c += 64) {
        const float xv = xr[c], xh = (xv - m) * r, d = dr[c], g = d * gamma[c];
        float v = r * ((g - s1) - xh * s2);
        if (res) v += res[row * C + c];
        if (relu_mask && !(xv > 0.f)) v = 0.f;
        dyxh[row * C + c] = d * xh;
        dx[row * C + c] = v;
    }
}

__global__ __launch_bounds__(256) void softmax_drop_fwd_kernel(float* __restrict__ s, float* __restrict__ pd, const uint8_t* __restrict__ key_valid,
                                                               long rows, int T, int HT, DropArgs d) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float* sr = s + row * T;
    const uint8_t* kv = key_valid + (row / HT) * T;
    float mx = -INFINITY;
    for (int t = lane; t < T; t += 64)
        if (kv[t]) mx = nan_max(mx, sr[t]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = nan_max(mx, __shfl_xor(mx, o));
    float sum = 0.f;
    for (int t = lane; t < T; t += 64) {
        const float e = kv[t] ? expf(sr[t] - mx) : 0.f;
        sr[t] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    const uint32_t thr = drop_threshold(d.p);
    const float scale = 1.f / (1.f - d.p);
    for (int t = lane; t < T; t += 64) {
        const float pv = sr[t] / sum;
        sr[t] = pv;
        if (pd) pd[row * T + t] = (d.p > 0.f) ? (drop_keep(d, thr, (uint64_t)(row * T + t)) ? pv * scale : 0.f) : pv;
    }
}

__global__ __launch_bounds__(256) void softmax_drop_bwd_kernel(const float* __restrict__ P, float* __restrict__ dP, long rows, int T, DropArgs d) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* pr = P + row * T;
    float* dr = dP + row * T;
    const uint32_t thr = drop_threshold(d.p);
    const float scale = 1.f / (1.f - d.p);
    float sum = 0.f;
    for (int t = lane; t < T; t += 64) {
        float g = dr[t];
        if (d.p > 0.f) g = drop_keep(d, thr, (uint64_t)(row * T + t)) ? g * scale : 0.f;
        dr[t] = g;
        sum = fmaf(g, pr[t], sum);
    }
    sum = wave_sum(sum);
    for (int t = lane; t < T; t += 64) dr[t] = pr[t] * (dr[t] - sum);
}

__global__ __launch_bounds__(256) void dropout_kernel(const float* x, float* y, size_t n, DropArgs d) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = x[i];
    if (d.p > 0.f) y[i] = drop_keep(d, drop_threshold(d.p), i) ? v * (1.f / (1.f - d.p)) : 0.f;
    else y[i] = v;
}
__global__ __launch_bounds__(256) void dropout_mask_kernel(uint8_t* __restrict__ out, size_t n, DropArgs d) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = drop_keep(d, drop_threshold(d.p), i) ? 1 : 0;
}
__global__ __launch_bounds__(256) void relu_bwd_kernel(const float* __restrict__ y, const float* dy, float* dx, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dx[i] = y[i] > 0.f ? dy[i] : 0.f;
}
__global__ __launch_bounds__(256) void tt_add_kernel(const float* a, const float* b, float* y, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = a[i] + b[i];
}
__global__ __launch_bounds__(256) void tt_mask_kernel(const float* x, const uint8_t* __restrict__ valid, float* y, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = valid[i] ? x[i] : 0.f;
}
__global__ __launch_bounds__(256) void tt_embed_kernel(const int64_t* __restrict__ phones, const float* __restrict__ tok_emb,
                                                       const float* __restrict__ pe_row, float* __restrict__ x, long rows, int D, int vocab) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)rows * D) return;
    const long r = (long)(i / D);
    const int c = (int)(i - (size_t)r * D);
    const int64_t id = phones[r];
    x[i] = (id >= 0 && id < vocab) ? pe_row[c] + tok_emb[id * D + c] : NAN;
}
__global__ __launch_bounds__(256) void tt_add_speaker_kernel(const float* x, const int64_t* __restrict__ speaker, const float* __restrict__ tab, float* y,
                                                             int S, int D, int n_speaker, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % D);
    const int64_t id = speaker[i / ((size_t)S * D)];
    y[i] = (id >= 0 && id < n_speaker) ? x[i] + tab[id * D + c] : NAN;
}
__global__ void dur_cum_kernel(const int64_t* __restrict__ dur, int32_t* __restrict__ cum, int B, int S, int L) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int32_t acc = 0;
    cum[(size_t)b * (S + 1)] = 0;
    for (int s = 0; s < S; ++s) {
        int64_t d = dur[(size_t)b * S + s];
        d = d < 0 ? 0 : (d > L ? L : d);
        acc = (int32_t)((int64_t)acc + d > L ? L : acc + d);
        cum[(size_t)b * (S + 1) + s + 1] = acc;
    }
}
// the position s with cum[s] <= t < cum[s + 1] (t < cum[S]): the last s with cum[s] <= t
__device__ __forceinline__ int lr_find(const int32_t* __restrict__ cum, int S, int t) {
    int lo = 0, hi = S;  // cum[lo] <= t < cum[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}
__global__ __launch_bounds__(256) void lr_fwd_kernel(const float* __restrict__ enc, const int32_t* __restrict__ cum, const float* __restrict__ pe_row,
                                                     float* __restrict__ y, int S, int L, int D) {
    const int t = blockIdx.x, b = blockIdx.y;
    const int32_t* cb = cum + (size_t)b * (S + 1);
    const bool real = t < cb[S];
    const int s = real ? lr_find(cb, S, t) : 0;
    const float* er = enc + ((size_t)b * S + s) * D;
    float* yr = y + ((size_t)b * L + t) * D;
    for (int c = threadIdx.x; c < D; c += 256) yr[c] = pe_row[c] + (real ? er[c] : 0.f);
}
__global__ __launch_bounds__(256) void lr_bwd_kernel(const float* __restrict__ dy, const int32_t* __restrict__ cum, const float* add, float* denc, int S,
                                                     int L, int D) {
    const int s = blockIdx.x, b = blockIdx.y;
    const int t0 = cum[(size_t)b * (S + 1) + s], t1 = cum[(size_t)b * (S + 1) + s + 1];
    for (int c = threadIdx.x; c < D; c += 256) {
        double acc = 0.0;
        for (int t = t0; t < t1; ++t) acc += (double)dy[((size_t)b * L + t) * D + c];
        const size_t o = ((size_t)b * S + s) * D + c;
        const float v = (float)acc;
        denc[o] = add ? add[o] + v : v;
    }
}
__global__ __launch_bounds__(256) void embed_grad_kernel(const int64_t* __restrict__ ids, const float* __restrict__ dx, float* __restrict__ dtab,
                                                         long rows, int per, int D, int pad_idx) {
    const int v = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x;
    if (c >= D) return;
    double acc = 0.0;
    if (v != pad_idx)
        for (long r = 0; r < rows; ++r)
            if (ids[r / per] == v) acc += (double)dx[r * D + c];
    dtab[(size_t)v * D + c] = (float)acc;
}

#endif  // PARROT_TTE_TRAIN_TU

}  // namespace parrot
