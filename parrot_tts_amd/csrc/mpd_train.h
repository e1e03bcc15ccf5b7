// mpd_train.h -- the kernels that TRAIN the multi-period discriminator (reference utils/vocoder/models.py:171-225 with weight norm
// attached, and the backward of that graph): parrot_mpd_train_forward / _backward (host_mpd_train.hip).  Activations are kept
// period-major: the map of a layer with C channels and H rows at period p is (N, p, C, H), so the (k, 1) convs of DiscriminatorP are
// plain 1-D convs over H on N p independent rows, and torch's (N, C, H, p) is a permuted view of the same memory.  The four convs
// between the ends go through train_gemm.h (host_mpd_train.hip fills the structs); the weight norm and the bias gradients are
// voc_train.h's.  This file holds the two ends of the stack, where a 64 x 64 MFMA tile would be almost all padding:
//   md_first_fwd_kernel   convs[0] (1 -> C1, k taps, stride s, padding 2) fused with the reflect pad and the fold: reads the
//                         waveform (N, T), writes the activated map (N, p, C1, H1)
//   md_first_dw_kernel    its weight gradient, fp64 partials per MD_CHUNK (row, column) pairs;  md_reduce_kernel adds them in order
//   md_first_dx_kernel    its data gradient fused with the fold's and the reflect pad's backward: d wav (N, T)
//   md_post_fwd_kernel    conv_post (C -> 1, 3 taps, padding 1): a per-column reduction over the channels
//   md_post_dx_kernel     its data gradient, an outer product, plus the upstream gradient, through the leaky ReLU's mask
//   md_post_dw_kernel     its weight gradient, fp64 partials per MD_CHUNK pairs
// Rules, as in train_gemm.h: exact fp32 products, fp32 accumulation in chains of at most MD_FLUSH channels; no floating-point
// atomics; every sum that ends in one number is fp64 in a fixed order; nothing clamps with fmaxf, so a NaN stays a NaN.  The
// launchers are defined in tu_mpd_train.hip, which alone sees the kernel bodies.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "train_gemm.h"
#include "wave_reduce.h"

namespace parrot {

constexpr int MD_PAD = 2;        // get_padding(5, 1): the reference pads by 2 whatever kernel_size is (models.py:177-181)
constexpr int MD_POST_K = 3;     // conv_post: (3, 1), padding (1, 0)
constexpr int MD_CHUNK = 2048;   // (row, column) pairs per fp64 partial of the two weight gradients
constexpr int MD_FLUSH = 64;     // channels per fp32 chain of md_first_dx_kernel and md_post_fwd_kernel

// The first layer.  H = (T + n_pad) / p rows of the folded waveform, H1 = (H + 2 MD_PAD - k) / s + 1 output rows.
struct MdFirst {
    int N, T, p, H, H1, C1, k, s;
};
inline int md_chunks(long R) { return (int)((R + MD_CHUNK - 1) / MD_CHUNK); }

hipError_t md_launch_first_fwd(const MdFirst& d, const float* wav, const float* w, const float* bias, float* y, float slope, hipStream_t s);
// part: md_chunks(N p H1) x C1 x k doubles
hipError_t md_launch_first_dw(const MdFirst& d, const float* dy, const float* wav, double* part, float* dw, hipStream_t s);
// dwav = (accumulate ? dwav : 0) + the period's gradient
hipError_t md_launch_first_dx(const MdFirst& d, const float* dy, const float* w, float* dwav, int accumulate, hipStream_t s);
// x (Z, C, H) -> y (Z, H)
hipError_t md_launch_post_fwd(const float* x, const float* w, const float* bias, float* y, int Z, int C, int H, hipStream_t s);
// dx (Z, C, H) = mask(pre + w (x) dy): pre, mask nullable
hipError_t md_launch_post_dx(const float* dy, const float* w, const float* pre, const float* mask, float mslope, float* dx, int Z, int C, int H,
                             hipStream_t s);
// part: md_chunks(Z H) x C x 3 doubles
hipError_t md_launch_post_dw(const float* dy, const float* x, double* part, float* dw, int Z, int C, int H, hipStream_t s);

#ifdef PARROT_MPD_TRAIN_TU

// Sample (row hh, column q) of the folded, reflect-padded waveform of one batch row; zero outside [0, H) (the conv's padding).
// Position t >= T is the reflection of 2 (T - 1) - t (F.pad(..., "reflect") on the tail; n_pad < T, so that index is never negative).
__device__ __forceinline__ float md_fold_at(const float* __restrict__ row, int hh, int q, int p, int H, int T) {
    if (hh < 0 || hh >= H) return 0.f;
    int t = hh * p + q;
    if (t >= T) t = 2 * (T - 1) - t;
    return row[t];
}

// grid (ceil(H1 / 256), p, N): thread = output row h1 of column q of batch row n; the k input samples are read once and every
// channel is then k FMAs and one store, coalesced along h1.  The weights and the bias are uniform over the wave.
__global__ __launch_bounds__(256) void md_first_fwd_kernel(const MdFirst d, const float* __restrict__ wav, const float* __restrict__ w,
                                                           const float* __restrict__ bias, float* __restrict__ y, float slope) {
    const int h1 = blockIdx.x * 256 + threadIdx.x, q = blockIdx.y, n = blockIdx.z;
    if (h1 >= d.H1) return;
    const float* row = wav + (size_t)n * d.T;
    float x[TG_MAX_TAPS];
#pragma unroll
    for (int j = 0; j < TG_MAX_TAPS; ++j) x[j] = j < d.k ? md_fold_at(row, h1 * d.s + j - MD_PAD, q, d.p, d.H, d.T) : 0.f;
    float* out = y + ((size_t)n * d.p + q) * d.C1 * d.H1 + h1;
    for (int c = 0; c < d.C1; ++c) {
        const float* wc = w + (size_t)c * d.k;
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < TG_MAX_TAPS; ++j)
            if (j < d.k) acc = fmaf(wc[j], x[j], acc);
        acc += bias[c];
        out[(size_t)c * d.H1] = acc > 0.f ? acc : acc * slope;
    }
}

// grid (chunks, C1): block (chunk, c) adds dy[n][q][c][h1] x[n][q][h1 s + j - 2] over its MD_CHUNK pairs r = (n p + q) H1 + h1, thread
// tid taking r_lo + tid, r_lo + tid + 256, ... in fp64, then the fixed tree, per tap.
__global__ __launch_bounds__(256) void md_first_dw_kernel(const MdFirst d, const float* __restrict__ dy, const float* __restrict__ wav,
                                                          double* __restrict__ part) {
    __shared__ double sm[256];
    const int c = blockIdx.y, tid = threadIdx.x;
    const long R = (long)d.N * d.p * d.H1, r_lo = (long)blockIdx.x * MD_CHUNK, r_hi = min(R, r_lo + MD_CHUNK);
    double acc[TG_MAX_TAPS];
#pragma unroll
    for (int j = 0; j < TG_MAX_TAPS; ++j) acc[j] = 0.0;
    for (long r = r_lo + tid; r < r_hi; r += 256) {
        const long zq = r / d.H1;
        const int h1 = (int)(r - zq * d.H1), n = (int)(zq / d.p), q = (int)(zq - (long)n * d.p);
        const double g = (double)dy[((size_t)zq * d.C1 + c) * d.H1 + h1];
        const float* row = wav + (size_t)n * d.T;
#pragma unroll
        for (int j = 0; j < TG_MAX_TAPS; ++j)
            if (j < d.k) acc[j] += g * (double)md_fold_at(row, h1 * d.s + j - MD_PAD, q, d.p, d.H, d.T);
    }
#pragma unroll
    for (int j = 0; j < TG_MAX_TAPS; ++j)
        if (j < d.k) {
            const double sum = block_sum(acc[j], sm);
            if (tid == 0) part[((size_t)blockIdx.x * d.C1 + c) * d.k + j] = sum;
        }
}
// out[i] = fl32(sum_c part[c][i]) in chunk order
__global__ __launch_bounds__(256) void md_reduce_kernel(const double* __restrict__ part, int nchunks, int n, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int c = 0; c < nchunks; ++c) s += part[(size_t)c * n + i];
    out[i] = (float)s;
}

// The gradient at sample (hh, q) of the padded, folded waveform of row n: sum over channels and over the taps j with
// hh + 2 - j = h1 s, 0 <= h1 < H1, of w[c][j] dy[n][q][c][h1]; the fp32 chain is moved into a second sum every MD_FLUSH channels.
__device__ __forceinline__ float md_first_dxp(const MdFirst& d, const float* __restrict__ dy, const float* __restrict__ w, int n, int q, int hh) {
    int h1[TG_MAX_TAPS];
#pragma unroll
    for (int j = 0; j < TG_MAX_TAPS; ++j) {
        const int num = hh + MD_PAD - j, o = num / d.s;
        h1[j] = (j < d.k && num >= 0 && o * d.s == num && o < d.H1) ? o : -1;
    }
    const float* g = dy + ((size_t)n * d.p + q) * d.C1 * d.H1;
    float acc = 0.f, tot = 0.f;
    for (int c = 0; c < d.C1; ++c) {
        const float* wc = w + (size_t)c * d.k;
        const float* gc = g + (size_t)c * d.H1;
#pragma unroll
        for (int j = 0; j < TG_MAX_TAPS; ++j)
            if (h1[j] >= 0) acc = fmaf(wc[j], gc[h1[j]], acc);
        if ((c + 1) % MD_FLUSH == 0) {
            tot += acc;
            acc = 0.f;
        }
    }
    return tot + acc;
}
// grid (ceil(H / 256), p, N): thread = sample t = hh p + q < T of row n (hh along the lanes, so dy is read along its rows).  The
// reflect pad's backward: padded position t' = 2 (T - 1) - t, when T <= t' < T + n_pad, is a second reader of sample t, and its
// gradient is added to the sample's own, once, after it.
__global__ __launch_bounds__(256) void md_first_dx_kernel(const MdFirst d, const float* __restrict__ dy, const float* __restrict__ w,
                                                          float* __restrict__ dwav, int accumulate) {
    const int hh = blockIdx.x * 256 + threadIdx.x, q = blockIdx.y, n = blockIdx.z;
    if (hh >= d.H) return;
    const int t = hh * d.p + q;
    if (t >= d.T) return;
    float v = md_first_dxp(d, dy, w, n, q, hh);
    const int tr = 2 * (d.T - 1) - t;
    if (tr >= d.T && tr < d.H * d.p) v = __fadd_rn(v, md_first_dxp(d, dy, w, n, tr % d.p, tr / d.p));
    float* o = dwav + (size_t)n * d.T + t;
    *o = accumulate ? __fadd_rn(*o, v) : v;
}

// grid ceil(Z H / 64): thread (g, l) = (tid / 64, tid % 64) adds channels g, g + 4, ... of column r = 64 blockIdx.x + l = z H + h, three
// taps each, in fp32 chains of at most MD_FLUSH channels; the four g are then added in order, then the bias.
__global__ __launch_bounds__(256) void md_post_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                          float* __restrict__ y, long R, int C, int H) {
    __shared__ float sm[4][64];
    const int g = threadIdx.x >> 6, l = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 64 + l;
    float acc = 0.f, tot = 0.f;
    if (r < R) {
        const long z = r / H;
        const int h = (int)(r - z * H);
        const float* xz = x + (size_t)z * C * H;
        int n = 0;
        for (int c = g; c < C; c += 4) {
            const float* xc = xz + (size_t)c * H;
            const float* wc = w + (size_t)c * MD_POST_K;
#pragma unroll
            for (int j = 0; j < MD_POST_K; ++j) {
                const int hh = h + j - 1;
                if (hh >= 0 && hh < H) acc = fmaf(wc[j], xc[hh], acc);
            }
            if (++n == MD_FLUSH) {
                n = 0;
                tot += acc;
                acc = 0.f;
            }
        }
    }
    sm[g][l] = tot + acc;
    __syncthreads();
    if (g == 0 && r < R) y[r] = (((sm[0][l] + sm[1][l]) + sm[2][l]) + sm[3][l]) + bias[0];
}
// thread = element (z, c, h): v = sum_j w[c][j] dy[z][h + 1 - j]; then + pre and the mask, rounded one after the other as in
// tap_gemm_kernel's epilogue
__global__ __launch_bounds__(256) void md_post_dx_kernel(const float* __restrict__ dy, const float* __restrict__ w, const float* __restrict__ pre,
                                                         const float* __restrict__ mask, float mslope, float* __restrict__ dx, size_t n, int C, int H) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int h = (int)(i % H), c = (int)(i / H % C);
    const size_t z = i / ((size_t)H * C);
    const float* g = dy + z * H;
    const float* wc = w + (size_t)c * MD_POST_K;
    float v = 0.f;
#pragma unroll
    for (int j = 0; j < MD_POST_K; ++j) {
        const int ho = h + 1 - j;
        if (ho >= 0 && ho < H) v = fmaf(wc[j], g[ho], v);
    }
    {
#pragma clang fp contract(off)
        if (pre) v = v + pre[i];
        if (mask && !(mask[i] > 0.f)) v = v * mslope;
    }
    dx[i] = v;
}
// grid (chunks, C): block (chunk, c) adds dy[z][h] x[z][c][h + j - 1] over its MD_CHUNK pairs r = z H + h, as md_first_dw_kernel does
__global__ __launch_bounds__(256) void md_post_dw_kernel(const float* __restrict__ dy, const float* __restrict__ x, double* __restrict__ part, long R,
                                                         int C, int H) {
    __shared__ double sm[256];
    const int c = blockIdx.y, tid = threadIdx.x;
    const long r_lo = (long)blockIdx.x * MD_CHUNK, r_hi = min(R, r_lo + MD_CHUNK);
    double acc[MD_POST_K];
#pragma unroll
    for (int j = 0; j < MD_POST_K; ++j) acc[j] = 0.0;
    for (long r = r_lo + tid; r < r_hi; r += 256) {
        const long z = r / H;
        const int h = (int)(r - z * H);
        const double g = (double)dy[r];
        const float* xc = x + ((size_t)z * C + c) * H;
#pragma unroll
        for (int j = 0; j < MD_POST_K; ++j) {
            const int hh = h + j - 1;
            if (hh >= 0 && hh < H) acc[j] += g * (double)xc[hh];
        }
    }
#pragma unroll
    for (int j = 0; j < MD_POST_K; ++j) {
        const double sum = block_sum(acc[j], sm);
        if (tid == 0) part[((size_t)blockIdx.x * C + c) * MD_POST_K + j] = sum;
    }
}

#endif  // PARROT_MPD_TRAIN_TU

}  // namespace parrot
