// msd_train.h -- the kernels that TRAIN the multi-scale discriminator (reference utils/vocoder/models.py:228-276: spectral norm on
// the first scale, weight norm on the others, and the backward of that graph): parrot_msd_train_forward / _backward
// (host_msd_train.hip).  Maps are torch's own, (N, C, L).  convs[6] (dense, 5 taps) goes through train_gemm_host.h, conv_post through
// mpd_train.h's md_launch_post_*, the weight norm and the bias gradients are voc_train.h's.  This file holds the rest:
//   ms_gconv_kernel         the grouped, strided convs[1 .. 5] (41 taps): forward (mode 0) and data gradient (mode 1, phase-split by
//                           t mod s), ONE launch per layer and direction, the group a grid dimension.  A block stages its input
//                           window in LDS once per 32 channels and forms the B operand of every tap from LDS
//   ms_gwgrad_kernel        their weight gradient, train_gemm.h's scheme: fp32 partials per TG_RCHUNK (b, t) pairs,
//   ms_gwgrad_reduce_kernel added in chunk order in fp64 and rounded once
//   ms_first_*_kernel       convs[0] (1 -> C, 15 taps, padding 7) on the VALU: forward, fp64 weight gradient, data gradient
//   ms_pool_*_kernel        AvgPool1d(4, 2, padding=2), count_include_pad: forward and backward
//   ms_sn_*_kernel          spectral norm: the two mat-vecs of a power iteration, the normalisation, sigma = u^T (W v), the fold
//                           W / sigma (a true fp32 division) and the backward through sigma with u and v as constants
// Rules, as in train_gemm.h: exact fp32 products (v_mfma_f32_32x32x2_f32), fp32 accumulation in chains of at most TG_ACC_FLUSH x 32
// products; no floating-point atomics; every sum that ends in one number is fp64 in a fixed order; nothing clamps with fmaxf, so a
// NaN stays a NaN.  A scale under spectral norm runs rows [0, zsplit) on one folded weight and rows [zsplit, Z) on another (the
// reference folds once per call of the discriminator, and iterates before each): every kernel that reads a weight takes both.
// The launchers are defined in tu_msd_train.hip, which alone sees the kernel bodies.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "train_gemm.h"
#include "wave_reduce.h"

namespace parrot {

constexpr int MS_K = 41;            // convs[1 .. 5]; padding 20
constexpr int MS_MAX_STRIDE = 4;    // the widest window a block stages: 64 s + 40 columns
constexpr int MS_CCH = 32;          // channels per staged window
constexpr int MS_XS_FLOATS = MS_CCH * MS_MAX_STRIDE * (64 + (MS_K - 1) / MS_MAX_STRIDE + 1);  // 32 x 300 floats = 37.5 KiB
constexpr int MS_FIRST_K = 15;      // convs[0]; padding 7
constexpr int MS_FIRST_PAD = 7;
constexpr int MS_FIRST_FLUSH = 16;  // channels per fp32 chain of ms_first_dx_kernel (16 x 15 products)
constexpr int MS_CHUNK = 2048;      // (row, column) pairs per fp64 partial of convs[0]'s weight gradient; elements per partial of <G, W>
constexpr float MS_SN_EPS = 1e-12f; // torch.nn.utils.spectral_norm's eps

// One grouped conv, x (Z, cin, Tin) -> y (Z, cout, Tout), Tout = (Tin + 2 pad - k) / s + 1, weight (cout, cin / G, k) as torch holds
// it.  w1 serves rows z >= zsplit (zsplit = Z: w0 alone).
struct MsGconv {
    int cin, cout, G, k, s, pad, Tin, Tout;
};
// forward: y = lrelu(conv + bias) when act.  bias nullable.
hipError_t ms_launch_gconv_fwd(const MsGconv& d, const float* x, const float* w0, const float* w1, int zsplit, const float* bias, float* y, int Z,
                               int act, float slope, hipStream_t s);
// dx (Z, cin, Tin) = mask(pre + the data gradient of dy): pre, mask (dx's shape) nullable
hipError_t ms_launch_gconv_dx(const MsGconv& d, const float* dy, const float* w0, const float* w1, int zsplit, const float* pre, const float* mask,
                              float mslope, float* dx, int Z, hipStream_t s);
// dw (cout, cin / G, k) over the Z rows given; part: ms_gwgrad_part_floats floats
size_t ms_gwgrad_part_floats(const MsGconv& d, int Z);
hipError_t ms_launch_gconv_dw(const MsGconv& d, const float* dy, const float* x, float* dw, int Z, float* part, size_t part_floats, hipStream_t s);

inline int ms_chunks(long R) { return (int)((R + MS_CHUNK - 1) / MS_CHUNK); }
// convs[0]: wav (Z, T), w (C, 15), y (Z, C, T)
hipError_t ms_launch_first_fwd(const float* wav, const float* w0, const float* w1, int zsplit, const float* bias, float* y, int Z, int T, int C,
                               float slope, hipStream_t s);
// part: ms_chunks(Z T) x C x 15 doubles
hipError_t ms_launch_first_dw(const float* dy, const float* wav, double* part, float* dw, int Z, int T, int C, hipStream_t s);
hipError_t ms_launch_first_dx(const float* dy, const float* w0, const float* w1, int zsplit, float* dwav, int Z, int T, int C, hipStream_t s);
// x (Z, T) -> y (Z, T / 2 + 1);  dx = (accumulate ? dx : 0) + the pool's backward of dy
hipError_t ms_launch_pool_fwd(const float* x, float* y, int Z, int T, hipStream_t s);
hipError_t ms_launch_pool_bwd(const float* dy, float* dx, int Z, int T, int accumulate, hipStream_t s);
// Spectral norm of w (rows, cols).  iterate: v = normalize(W^T u), u = normalize(W v), both in place; then sigma[0] = u^T (W v) and
// wf = w / sigma.  tmp: rows + cols floats.
hipError_t ms_launch_sn_fold(const float* w, float* u, float* v, int rows, int cols, int iterate, float* wf, float* sigma, float* tmp, hipStream_t s);
// dw = ga / sa - (<ga, w> / sa^2) ua va^T + gb / sb - (<gb, w> / sb^2) ub vb^T  (gb null: the first two terms alone)
// part: 2 x (ms_chunks(rows cols) + 1) doubles
hipError_t ms_launch_sn_bwd(const float* ga, const float* gb, const float* w, const float* ua, const float* va, const float* sa, const float* ub,
                            const float* vb, const float* sb, float* dw, int rows, int cols, double* part, hipStream_t s);

#ifdef PARROT_MSD_TRAIN_TU

typedef float ms_f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------------
// ms_gconv_kernel: out[z][g Mg + m][n c_mul + c_off] = epi(sum over kc < Kg and taps i < nt of A(g, m, kc, i) X[z][g Kg + kc][win(n, i)]).
//   mode 0 (forward):  rows m = output channels, kc = input channels, nt = k, win = n s + i - pad
//   mode 1 (data gradient, phase r = t mod s of dx, t = n s + r): rows m = input channels, kc = output channels, the taps
//           j = j0 + s i with j0 = (r + pad) mod s, win = n + (r + pad - j0) / s - i in dy
// grid (tiles x phases, G x ceil(Mg / 64), Z), four waves, each one 32 x 32 tile of the 64 x 64 block, as tap_gemm_kernel.  For every
// MS_CCH channels the block stages the window of its 64 columns ONCE, 63 xs + nt columns a channel (xs = s forward, 1 backward),
// stored de-interleaved by column mod xs so that the 32 lanes of a half-wave read consecutive words for every tap (ds_read_b32 banks
// modulo 32 within a half-wave: conflict-free at any stride).  The A operand is staged 32 reduction indices q = kc nt + i at a time
// ([q][m], row stride 65); forward, q is contiguous in torch's weight row, so A is a plain row-major (cout / G, cin / G k) matrix.
// Qo[q] is where tap q's window row starts in Xs, or -1 past the end, where both operands are zero.
// ---------------------------------------------------------------------------------------------
struct MsGconvParams {
    MsGconv d;
    int mode, tiles, mtiles, zsplit;
    const float *w0, *w1;
    const float* X;   // forward: x; backward: dy
    float* C;         // forward: y; backward: dx
    const float *bias, *pre, *mask;
    int lrelu;
    float lslope, mslope;
};
__global__ __launch_bounds__(256) void ms_gconv_kernel(const MsGconvParams p) {
    __shared__ float Xs[MS_XS_FLOATS];
    __shared__ float As[32][65];
    __shared__ int Qo[32];
    const MsGconv& d = p.d;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, half = lane >> 5, l31 = lane & 31;
    const int g = blockIdx.y / p.mtiles, m0 = (blockIdx.y - g * p.mtiles) * 64, z = blockIdx.z;
    const int cing = d.cin / d.G, coutg = d.cout / d.G;
    int Mg, Kg, nt, xs, N, c_mul, c_off, a_si, n0, win0, x_len, c_len;
    long a_sm, a_sk, a_off;
    if (p.mode == 0) {
        n0 = blockIdx.x * 64;
        Mg = coutg; Kg = cing; nt = d.k; xs = d.s; N = d.Tout; c_mul = 1; c_off = 0;
        a_sm = (long)cing * d.k; a_sk = d.k; a_si = 1; a_off = 0;
        win0 = n0 * d.s - d.pad; x_len = d.Tin; c_len = d.Tout;
    } else {
        const int r = blockIdx.x / p.tiles, j0 = (r + d.pad) % d.s;
        n0 = (blockIdx.x - r * p.tiles) * 64;
        Mg = cing; Kg = coutg; nt = (d.k - 1 - j0) / d.s + 1; xs = 1; N = (d.Tin - r + d.s - 1) / d.s; c_mul = d.s; c_off = r;
        a_sm = d.k; a_sk = (long)cing * d.k; a_si = d.s; a_off = j0;
        win0 = n0 + (r + d.pad - j0) / d.s - (nt - 1); x_len = d.Tout; c_len = d.Tin;
    }
    if (n0 >= N) return;  // (the whole block: a short phase has fewer tiles)
    const int PL = 64 + (nt - 1) / xs + 1, RS = xs * PL, Wc = 63 * xs + nt;
    const float* __restrict__ A = (z < p.zsplit ? p.w0 : p.w1) + (long)g * coutg * cing * d.k + a_off;
    const float* __restrict__ X = p.X + ((long)z * (p.mode == 0 ? d.cin : d.cout) + (long)g * Kg) * x_len;
    const bool a_qfast = (p.mode == 0);
    const bool live = m0 + wm * 32 < Mg;  // (a wave whose 32 rows are all padding stages and waits but issues no MFMA)
    ms_f32x16 acc, tot;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = tot[r] = 0.f;
    int since = 0;
    for (int kc0 = 0; kc0 < Kg; kc0 += MS_CCH) {
        const int kcn = min(MS_CCH, Kg - kc0), Q = kcn * nt;
        for (int idx = tid; idx < kcn * Wc; idx += 256) {
            const int kl = idx / Wc, xl = idx - kl * Wc, x = win0 + xl;
            float v = 0.f;
            if (x >= 0 && x < x_len) v = X[(long)(kc0 + kl) * x_len + x];
            Xs[kl * RS + (xl % xs) * PL + xl / xs] = v;
        }
        for (int q0 = 0; q0 < Q; q0 += 32) {
#pragma unroll
            for (int i = 0; i < (32 * 64) / 256; ++i) {
                const int idx = i * 256 + tid;
                int kk, mm;
                if (a_qfast) { mm = idx / 32; kk = idx % 32; } else { kk = idx / 64; mm = idx % 64; }
                const int q = q0 + kk;
                float v = 0.f;
                if (q < Q && m0 + mm < Mg) {
                    const int kl = q / nt, ti = q - kl * nt;
                    v = A[(long)(m0 + mm) * a_sm + (long)(kc0 + kl) * a_sk + (long)ti * a_si];
                }
                As[kk][mm] = v;
            }
            if (tid < 32) {
                const int q = q0 + tid;
                int o = -1;
                if (q < Q) {
                    const int kl = q / nt, ti = q - kl * nt;
                    o = kl * RS + (p.mode == 0 ? (ti % xs) * PL + ti / xs : nt - 1 - ti);
                }
                Qo[tid] = o;
            }
            __syncthreads();
            if (live) {
#pragma unroll
                for (int ks = 0; ks < 32; ks += 2) {
                    const float a = As[ks + half][wm * 32 + l31];
                    const int o = Qo[ks + half];
                    const float b = o >= 0 ? Xs[o + wn * 32 + l31] : 0.f;
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
                }
            }
            __syncthreads();
            if (++since == TG_ACC_FLUSH) {
                since = 0;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    tot[r] += acc[r];
                    acc[r] = 0.f;
                }
            }
        }
    }
    const int n = n0 + wn * 32 + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (m < Mg && n < N) {
            float v = tot[r] + acc[r];
            const int ch = g * Mg + m;
            if (p.bias) v += p.bias[ch];
            const long o = ((long)z * (p.mode == 0 ? d.cout : d.cin) + ch) * c_len + (long)n * c_mul + c_off;
            if (p.mask || p.pre) {
#pragma clang fp contract(off)  // (the product and the sum are rounded one after the other, as tap_gemm_kernel's epilogue rounds them)
                if (p.pre) v = v + p.pre[o];
                if (p.mask && !(p.mask[o] > 0.f)) v = v * p.mslope;
            }
            if (p.lrelu) v = v > 0.f ? v : v * p.lslope;
            p.C[o] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// ms_gwgrad_kernel: part[chunk][co][ci ntg + jj] = sum over the chunk's pairs r = z Tout + t of dy[z][co][t] x[z][ci][t s + j0 + jj - pad],
// for the ntg taps from j0.  grid (ceil(cin / G ntg / 64), G x ceil(cout / G / 64), chunks); the tile and the staging are
// wgrad_kernel's, the 256 pairs of a chunk one accumulation chain.  Every element of part is written.
// ---------------------------------------------------------------------------------------------
struct MsGwgradParams {
    MsGconv d;
    const float *dy, *x;
    float* part;
    int R, j0, ntg, mtiles;
};
__global__ __launch_bounds__(256) void ms_gwgrad_kernel(const MsGwgradParams p) {
    __shared__ float As[32][65];
    __shared__ float Bs[32][65];
    const MsGconv& d = p.d;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, half = lane >> 5, l31 = lane & 31;
    const int cing = d.cin / d.G, coutg = d.cout / d.G, ncol = cing * p.ntg;
    const int g = blockIdx.y / p.mtiles, m0 = (blockIdx.y - g * p.mtiles) * 64, n0 = blockIdx.x * 64;
    const int r_lo = blockIdx.z * TG_RCHUNK, r_hi = min(p.R, r_lo + TG_RCHUNK);
    const bool live = m0 + wm * 32 < coutg && n0 + wn * 32 < ncol;
    ms_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int r0 = r_lo; r0 < r_hi; r0 += 32) {
#pragma unroll
        for (int i = 0; i < (32 * 64) / 256; ++i) {
            const int idx = i * 256 + tid, mm = idx / 32, kk = idx % 32, r = r0 + kk;
            float v = 0.f, w = 0.f;
            if (r < r_hi) {
                const int z = r / d.Tout, t = r - z * d.Tout;
                if (m0 + mm < coutg) v = p.dy[((long)z * d.cout + g * coutg + m0 + mm) * d.Tout + t];
                const int col = n0 + mm;
                if (col < ncol) {
                    const int ci = col / p.ntg, x = t * d.s + p.j0 + (col - ci * p.ntg) - d.pad;
                    if (x >= 0 && x < d.Tin) w = p.x[((long)z * d.cin + g * cing + ci) * d.Tin + x];
                }
            }
            As[kk][mm] = v;
            Bs[kk][mm] = w;
        }
        __syncthreads();
        if (live) {
#pragma unroll
            for (int ks = 0; ks < 32; ks += 2) {
                const float a = As[ks + half][wm * 32 + l31];
                const float b = Bs[ks + half][wn * 32 + l31];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
            }
        }
        __syncthreads();
    }
    float* __restrict__ out = p.part + (size_t)blockIdx.z * d.cout * ncol;
    const int n = n0 + wn * 32 + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (m < coutg && n < ncol) out[(size_t)(g * coutg + m) * ncol + n] = acc[r];
    }
}
// dw[co][ci][j0 + jj] = fl32(sum_c part[c][co][ci ntg + jj]) in chunk order
__global__ __launch_bounds__(256) void ms_gwgrad_reduce_kernel(const float* __restrict__ part, int nchunks, int cout, int cing, int ntg, int j0, int k,
                                                               float* __restrict__ dw) {
    const size_t per = (size_t)cout * cing * ntg;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= per) return;
    double s = 0.0;
    for (int c = 0; c < nchunks; ++c) s += (double)part[(size_t)c * per + i];
    const int jj = (int)(i % ntg);
    const size_t row = i / ntg;  // co cing + ci
    dw[row * k + j0 + jj] = (float)s;
}

// ---------------------------------------------------------------------------------------------
// convs[0].  ms_first_fwd_kernel: grid (ceil(T / 256), Z), thread = sample t: the 15 inputs are read once, every channel is then 15
// FMAs and one store, coalesced along t.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ms_first_fwd_kernel(const float* __restrict__ wav, const float* __restrict__ w0, const float* __restrict__ w1,
                                                           int zsplit, const float* __restrict__ bias, float* __restrict__ y, int T, int C, float slope) {
    const int t = blockIdx.x * 256 + threadIdx.x, z = blockIdx.y;
    if (t >= T) return;
    const float* row = wav + (size_t)z * T;
    const float* w = z < zsplit ? w0 : w1;
    float x[MS_FIRST_K];
#pragma unroll
    for (int j = 0; j < MS_FIRST_K; ++j) {
        const int tt = t + j - MS_FIRST_PAD;
        x[j] = (tt >= 0 && tt < T) ? row[tt] : 0.f;
    }
    float* out = y + (size_t)z * C * T + t;
    for (int c = 0; c < C; ++c) {
        const float* wc = w + (size_t)c * MS_FIRST_K;
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < MS_FIRST_K; ++j) acc = fmaf(wc[j], x[j], acc);
        acc += bias[c];
        out[(size_t)c * T] = acc > 0.f ? acc : acc * slope;
    }
}
// grid (chunks, C): block (chunk, c) adds dy[z][c][t] wav[z][t + j - 7] over its MS_CHUNK pairs r = z T + t in fp64, then the fixed tree
__global__ __launch_bounds__(256) void ms_first_dw_kernel(const float* __restrict__ dy, const float* __restrict__ wav, double* __restrict__ part, long R,
                                                          int T, int C) {
    __shared__ double sm[256];
    const int c = blockIdx.y, tid = threadIdx.x;
    const long r_lo = (long)blockIdx.x * MS_CHUNK, r_hi = min(R, r_lo + MS_CHUNK);
    double acc[MS_FIRST_K];
#pragma unroll
    for (int j = 0; j < MS_FIRST_K; ++j) acc[j] = 0.0;
    for (long r = r_lo + tid; r < r_hi; r += 256) {
        const long z = r / T;
        const int t = (int)(r - z * T);
        const double g = (double)dy[((size_t)z * C + c) * T + t];
        const float* row = wav + (size_t)z * T;
#pragma unroll
        for (int j = 0; j < MS_FIRST_K; ++j) {
            const int tt = t + j - MS_FIRST_PAD;
            if (tt >= 0 && tt < T) acc[j] += g * (double)row[tt];
        }
    }
#pragma unroll
    for (int j = 0; j < MS_FIRST_K; ++j) {
        const double sum = block_sum(acc[j], sm);
        if (tid == 0) part[((size_t)blockIdx.x * C + c) * MS_FIRST_K + j] = sum;
    }
}
// out[i] = fl32(sum_c part[c][i]) in chunk order
__global__ __launch_bounds__(256) void ms_reduce_kernel(const double* __restrict__ part, int nchunks, int n, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int c = 0; c < nchunks; ++c) s += part[(size_t)c * n + i];
    out[i] = (float)s;
}
// thread = sample (z, t): dwav = sum_c sum_j w[c][j] dy[z][c][t + 7 - j], the fp32 chain moved into a second sum every MS_FIRST_FLUSH channels
__global__ __launch_bounds__(256) void ms_first_dx_kernel(const float* __restrict__ dy, const float* __restrict__ w0, const float* __restrict__ w1,
                                                          int zsplit, float* __restrict__ dwav, int T, int C) {
    const int t = blockIdx.x * 256 + threadIdx.x, z = blockIdx.y;
    if (t >= T) return;
    const float* w = z < zsplit ? w0 : w1;
    const float* g = dy + (size_t)z * C * T;
    float acc = 0.f, tot = 0.f;
    for (int c = 0; c < C; ++c) {
        const float* wc = w + (size_t)c * MS_FIRST_K;
        const float* gc = g + (size_t)c * T;
#pragma unroll
        for (int j = 0; j < MS_FIRST_K; ++j) {
            const int to = t + MS_FIRST_PAD - j;
            if (to >= 0 && to < T) acc = fmaf(wc[j], gc[to], acc);
        }
        if ((c + 1) % MS_FIRST_FLUSH == 0) {
            tot += acc;
            acc = 0.f;
        }
    }
    dwav[(size_t)z * T + t] = tot + acc;
}

// ---------------------------------------------------------------------------------------------
// The pool: y[i] = (x[2 i - 2] + x[2 i - 1] + x[2 i] + x[2 i + 1]) / 4, zero outside [0, T), i < T / 2 + 1; sample t feeds outputs
// t / 2 and t / 2 + 1.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ms_pool_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int T, int To) {
    const int i = blockIdx.x * 256 + threadIdx.x, z = blockIdx.y;
    if (i >= To) return;
    const float* row = x + (size_t)z * T;
    float s = 0.f;
#pragma unroll
    for (int dd = 0; dd < 4; ++dd) {
        const int t = 2 * i - 2 + dd;
        if (t >= 0 && t < T) s += row[t];
    }
    y[(size_t)z * To + i] = s * 0.25f;
}
__global__ __launch_bounds__(256) void ms_pool_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int T, int To, int accumulate) {
    const int t = blockIdx.x * 256 + threadIdx.x, z = blockIdx.y;
    if (t >= T) return;
    const float* g = dy + (size_t)z * To;
    const int ia = t >> 1, ib = ia + 1;
    float s = g[ia];  // (ia <= (T - 1) / 2 < To)
    if (ib < To) s += g[ib];
    float* o = dx + (size_t)z * T + t;
    const float v = s * 0.25f;
    *o = accumulate ? __fadd_rn(*o, v) : v;
}

// ---------------------------------------------------------------------------------------------
// Spectral norm.  W is (rows, cols) row-major.
// ---------------------------------------------------------------------------------------------
// out[c] = fl32(sum_r W[r][c] u[r]): grid ceil(cols / 64); thread (g, l) adds rows g, g + 4, ... of column 64 x + l in fp64, then the four g in order
__global__ __launch_bounds__(256) void ms_sn_mvt_kernel(const float* __restrict__ w, const float* __restrict__ u, float* __restrict__ out, int rows, int cols) {
    __shared__ double sm[4][64];
    const int g = threadIdx.x >> 6, l = threadIdx.x & 63, c = blockIdx.x * 64 + l;
    double s = 0.0;
    if (c < cols)
        for (int r = g; r < rows; r += 4) s += (double)w[(size_t)r * cols + c] * (double)u[r];
    sm[g][l] = s;
    __syncthreads();
    if (g == 0 && c < cols) out[c] = (float)(((sm[0][l] + sm[1][l]) + sm[2][l]) + sm[3][l]);
}
// out[r] = fl32(sum_c W[r][c] v[c]): one block per row
__global__ __launch_bounds__(256) void ms_sn_mv_kernel(const float* __restrict__ w, const float* __restrict__ v, float* __restrict__ out, int cols) {
    __shared__ double sm[256];
    const int r = blockIdx.x, tid = threadIdx.x;
    const float* wr = w + (size_t)r * cols;
    double s = 0.0;
    for (int c = tid; c < cols; c += 256) s += (double)wr[c] * (double)v[c];
    s = block_sum(s, sm);
    if (tid == 0) out[r] = (float)s;
}
// one block: x[i] = t[i] / max(||t||, eps), the norm an fp64 sum rounded to fp32 (a NaN norm stays a NaN)
__device__ __forceinline__ void ms_sn_normalize(const float* __restrict__ t, float* __restrict__ x, int n, double* sm) {
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int i = tid; i < n; i += 256) s += (double)t[i] * (double)t[i];
    const float nf = (float)sqrt(block_sum(s, sm));
    const float den = nf < MS_SN_EPS ? MS_SN_EPS : nf;
    for (int i = tid; i < n; i += 256) x[i] = __fdiv_rn(t[i], den);
}
__global__ __launch_bounds__(256) void ms_sn_normalize_kernel(const float* __restrict__ t, float* __restrict__ x, int n) {
    __shared__ double sm[256];
    ms_sn_normalize(t, x, n, sm);
}
// one block: t = W v.  iterate: u = normalize(t) (a thread reads back only what it wrote).  sigma = fl32(sum_r u[r] t[r])
__global__ __launch_bounds__(256) void ms_sn_sigma_kernel(const float* __restrict__ t, float* __restrict__ u, int rows, int iterate, float* __restrict__ sigma) {
    __shared__ double sm[256];
    const int tid = threadIdx.x;
    if (iterate) ms_sn_normalize(t, u, rows, sm);
    double s = 0.0;
    for (int i = tid; i < rows; i += 256) s += (double)u[i] * (double)t[i];
    s = block_sum(s, sm);
    if (tid == 0) sigma[0] = (float)s;
}
__global__ __launch_bounds__(256) void ms_sn_fold_kernel(const float* __restrict__ w, const float* __restrict__ sigma, float* __restrict__ wf, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) wf[i] = __fdiv_rn(w[i], sigma[0]);
}
// part[h][chunk] = sum over the chunk's MS_CHUNK elements of g_h[i] w[i] (fp64, thread-strided, the fixed tree): grid (chunks, halves)
__global__ __launch_bounds__(256) void ms_sn_dot_kernel(const float* __restrict__ ga, const float* __restrict__ gb, const float* __restrict__ w,
                                                        double* __restrict__ part, size_t n, int nchunks) {
    __shared__ double sm[256];
    const float* g = blockIdx.y ? gb : ga;
    const size_t lo = (size_t)blockIdx.x * MS_CHUNK, hi = min(n, lo + MS_CHUNK);
    double s = 0.0;
    for (size_t i = lo + threadIdx.x; i < hi; i += 256) s += (double)g[i] * (double)w[i];
    s = block_sum(s, sm);
    if (threadIdx.x == 0) part[(size_t)blockIdx.y * (nchunks + 1) + blockIdx.x] = s;
}
// part[h][nchunks] = (the chunks of half h, added in order) / sigma_h^2: one thread per half
__global__ void ms_sn_coef_kernel(double* __restrict__ part, int nchunks, const float* __restrict__ sa, const float* __restrict__ sb) {
    const int h = threadIdx.x;
    double* p = part + (size_t)h * (nchunks + 1);
    double s = 0.0;
    for (int c = 0; c < nchunks; ++c) s += p[c];
    const double sg = (double)(h ? sb : sa)[0];
    p[nchunks] = s / (sg * sg);
}
__global__ __launch_bounds__(256) void ms_sn_bwd_kernel(const float* __restrict__ ga, const float* __restrict__ gb, const float* __restrict__ ua,
                                                        const float* __restrict__ va, const float* __restrict__ sa, const float* __restrict__ ub,
                                                        const float* __restrict__ vb, const float* __restrict__ sb, const double* __restrict__ part,
                                                        int nchunks, float* __restrict__ dw, int rows, int cols) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)rows * cols) return;
    const int r = (int)(i / cols), c = (int)(i - (size_t)r * cols);
    double v = (double)ga[i] / (double)sa[0] - part[nchunks] * (double)ua[r] * (double)va[c];
    if (gb) v += (double)gb[i] / (double)sb[0] - part[2 * nchunks + 1] * (double)ub[r] * (double)vb[c];
    dw[i] = (float)v;
}

#endif  // PARROT_MSD_TRAIN_TU

}  // namespace parrot
