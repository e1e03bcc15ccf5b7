// train_gemm.h -- the exact-fp32 matrix products of the three training paths (aligner_train.h, tte_train.h, voc_train.h): every
// conv, Linear and transposed-conv phase, their data gradients, weight gradients and bias gradients.  Weights are read where torch
// holds them and activations where the caller keeps them, both through strides, so one kernel serves channel-first and channel-last
// arrays and a transposed operand costs nothing (the host wrappers that fill the structs: train_gemm_host.h).
//   tap_gemm_kernel      Y[z] (M x N) = sum_j A_j (M x K) shift_j(X[z]) (K x N), any strides: a conv (one tap per kernel column), a
//                        Linear (one tap) and every data gradient (A transposed through its strides, taps flipped)
//   wgrad_kernel         dA_j (M x K) = sum_(b, t) dY[b][m][t] X[b][k][t + shift_j] as fp32 partials over fixed blocks of B T,
//   wgrad_reduce_kernel  which adds the partials in block order in fp64 and rounds once
//   colsum_*             bias gradients: the same two-level fixed-order scheme over the rows of a (B T, M) array
// The base contract, which is all the aligner and the TTE use: exact fp32 products (v_mfma_f32_32x32x2_f32), fp32 accumulation in
// chains of at most TG_ACC_FLUSH x 32 products, X zero outside [0, N); every sum over B T that ends in one number is fp64 in a fixed
// order.  No floating-point atomics: two calls on the same inputs agree bit for bit.  Nothing clamps with fmaxf, so a NaN stays a NaN
// (the ReLU is `v < 0 ? 0 : v`).
// The vocoder's extra fields: x_mul / x_n (TapGemmParams) and x_mul / x_T (WgradParams) read X at a stride with its own bound, for
// the phases of a transposed conv and its gradients; mask / mslope, res and lrelu / lslope extend the epilogue by a leaky ReLU's
// backward, a residual add and the next conv's activation; pre (the discriminator's training, mpd_train.h) is added before the mask:
// the gradient that arrives at a saved map from outside joins the data gradient, and the sum passes the mask.  A zero in every extra
// field is the base behaviour bit for bit, so a caller that value-initialises the struct and fills the base fields need not know of them.
// The launchers are defined in tu_train_gemm.hip, which alone sees the kernel bodies (PARROT_TRAIN_GEMM_TU).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace parrot {

constexpr int TG_MAX_TAPS = 11;   // the widest conv that goes through tap_gemm_kernel: the vocoder's k = 11 (the TTE's FFN has 9, the aligner 5)
constexpr int TG_RCHUNK = 256;    // (b, t) pairs per weight-gradient / column-sum partial: the fixed block of the two-level sums
constexpr int TG_ACC_FLUSH = 8;   // tap_gemm_kernel moves its accumulator into a second one every 8 x 32 products

// Y[z][m][n] = act(sum_j sum_k A_j[m][k] X[z][k][n + shift_j] + bias0[m] + bias1[m]); X is zero outside 0 <= n + shift_j < N.
// The fields after `relu` serve the vocoder's training (voc_train.h); zero in each of them is the line above, bit for bit:
//   X is read at column n x_mul + shift_j and is zero outside [0, x_n)  (x_mul = 0: 1; x_n = 0: N): a transposed conv's phases and its
//   data gradient;  then, after the bias:  v += pre[z][m][n],  v = mask[z][m][n] > 0 ? v : v mslope  (a leaky ReLU's backward on its
//   saved output),  v += res[z][m][n]  (a residual), all three at C's strides;  and after `relu`:  v = v > 0 ? v : v lslope  when lrelu.
struct TapGemmParams {
    const float* A[TG_MAX_TAPS];  // tap j: A_j[m][k] at A[j] + m a_sm + k a_sk
    long x_off[TG_MAX_TAPS];      // tap j reads X[z] + x_off[j] (a column block of a wider array)
    int shift[TG_MAX_TAPS];
    int ntaps;
    const float* X;               // X[z][k][n] at X + z x_sz + k x_sk + n x_sn
    float* C;                     // Y[z][m][n] at C + z c_sz + m c_sm + n c_sn
    int M, N, K;
    long a_sm, a_sk, x_sz, x_sk, x_sn, c_sz, c_sm, c_sn;
    const float* bias0;           // nullable; bias1 (nullable) is added to bias0 first, in fp32 (b_ih + b_hh)
    const float* bias1;
    int relu;
    int x_mul, x_n;
    const float* mask;
    float mslope;
    const float* res;
    int lrelu;
    float lslope;
    const float* pre;
};
// part[chunk][j][m][k] = sum over the chunk's (b, t) of dY[b][m][t] X[b][k][t + shift_j]; chunk c covers r = b T + t in
// [c TG_RCHUNK, (c + 1) TG_RCHUNK).  X is zero outside 0 <= t + shift_j < T.
// x_mul, x_T (zero: 1 and T, the line above): X is read at t x_mul + shift_j and is zero outside [0, x_T): the weight gradient of a
// transposed conv, whose input is in dY's role and whose output gradient, u times as long, in X's.
struct WgradParams {
    const float* dY;  // dY[b][m][t] at dY + b y_sz + m y_sm + t y_st
    const float* X;   // X[b][k][t] at X + b x_sz + k x_sk + t x_st
    float* part;
    int M, K, T, R, ntaps;
    int shift[TG_MAX_TAPS];
    long y_sz, y_sm, y_st, x_sz, x_sk, x_st;
    int x_mul, x_T;
};

hipError_t launch_tap_gemm(const TapGemmParams& p, int Z, hipStream_t s);
int wgrad_chunks(int R);
hipError_t launch_wgrad(const WgradParams& p, hipStream_t s);
// out[m o_sm + k o_sk + j o_sj] = fl32(sum_c part[c][j][m][k]) in chunk order, fp64
hipError_t launch_wgrad_reduce(const float* part, int nchunks, int ntaps, int M, int K, float* out, long o_sm, long o_sk, long o_sj, hipStream_t s);
// out0[m] (and out1[m], nullable) = fl32(sum_r src[r ld + m]), r < R: fp64 partials per TG_RCHUNK rows (part: chunks x M doubles)
hipError_t launch_colsum(const float* src, int R, int M, long ld, double* part, float* out0, float* out1, hipStream_t s);

#ifdef PARROT_TRAIN_GEMM_TU

typedef float tg_f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------------
// tap_gemm_kernel: grid (ceil(N / 64), ceil(M / 64), Z), four waves, each one 32 x 32 tile of the 64 x 64 block on
// v_mfma_f32_32x32x2_f32.  Both operands are staged K-major in LDS ([k][m], [k][n], row stride 65) through their strides, 32 k per
// pass; whichever index has stride 1 runs along the lanes of the staging loads.  Rows m >= M, columns n >= N and k >= K are staged
// as zeros on BOTH sides, so a NaN never meets a padding zero in a stored element.  The fp32 chain of one accumulator is at most
// TG_ACC_FLUSH x 32 products long: it is then added into a second accumulator and cleared.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tap_gemm_kernel(const TapGemmParams p) {
    constexpr int KC = 32, RS = 65;
    __shared__ float As[KC][RS];
    __shared__ float Bs[KC][RS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, half = lane >> 5, l31 = lane & 31;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const float* __restrict__ X = p.X + (long)blockIdx.z * p.x_sz;
    tg_f32x16 acc, tot;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = tot[r] = 0.f;
    int since = 0;
    const bool a_kfast = (p.a_sk == 1), x_kfast = (p.x_sn != 1);
    const int x_mul = p.x_mul ? p.x_mul : 1, x_n = p.x_n ? p.x_n : p.N;
    for (int j = 0; j < p.ntaps; ++j) {
        const float* __restrict__ A = p.A[j];
        const float* __restrict__ Xj = X + p.x_off[j];
        const int sh = p.shift[j];
        for (int k0 = 0; k0 < p.K; k0 += KC) {
#pragma unroll
            for (int i = 0; i < (KC * 64) / 256; ++i) {
                const int idx = i * 256 + tid;
                int kk, mm;
                if (a_kfast) { mm = idx / KC; kk = idx % KC; } else { kk = idx / 64; mm = idx % 64; }
                float v = 0.f;
                if (k0 + kk < p.K && m0 + mm < p.M) v = A[(long)(m0 + mm) * p.a_sm + (long)(k0 + kk) * p.a_sk];
                As[kk][mm] = v;
                int kb, nn;
                if (x_kfast) { nn = idx / KC; kb = idx % KC; } else { kb = idx / 64; nn = idx % 64; }
                const int tn = (n0 + nn) * x_mul + sh;
                float w = 0.f;
                if (k0 + kb < p.K && n0 + nn < p.N && tn >= 0 && tn < x_n) w = Xj[(long)(k0 + kb) * p.x_sk + (long)tn * p.x_sn];
                Bs[kb][nn] = w;
            }
            __syncthreads();
#pragma unroll
            for (int ks = 0; ks < KC; ks += 2) {
                const float a = As[ks + half][wm * 32 + l31];
                const float b = Bs[ks + half][wn * 32 + l31];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
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
    float* __restrict__ C = p.C + (long)blockIdx.z * p.c_sz;
    const int n = n0 + wn * 32 + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (m < p.M && n < p.N) {
            float v = tot[r] + acc[r];
            if (p.bias0) v += p.bias1 ? __fadd_rn(p.bias0[m], p.bias1[m]) : p.bias0[m];
            const long o = (long)m * p.c_sm + (long)n * p.c_sn;
            if (p.mask || p.res || p.pre) {
#pragma clang fp contract(off)  // (the product and the sum are rounded one after the other, as torch rounds them)
                const long oz = (long)blockIdx.z * p.c_sz + o;
                if (p.pre) v = v + p.pre[oz];
                if (p.mask && !(p.mask[oz] > 0.f)) v = v * p.mslope;
                if (p.res) v = v + p.res[oz];
            }
            if (p.relu) v = v < 0.f ? 0.f : v;  // (a NaN stays a NaN, as torch's relu keeps it)
            if (p.lrelu) v = v > 0.f ? v : v * p.lslope;
            C[o] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// wgrad_kernel: the same tile on the transposed problem: the reduction runs over r = b T + t inside one fixed chunk of TG_RCHUNK
// pairs, rows are dY's channels, columns X's.  grid (ceil(K / 64), ceil(M / 64), chunks x ntaps); blockIdx.z = chunk ntaps + j.
// Every element of part is written (a chunk is never empty: chunks = ceil(R / TG_RCHUNK)).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wgrad_kernel(const WgradParams p) {
    constexpr int KC = 32, RS = 65;
    __shared__ float As[KC][RS];
    __shared__ float Bs[KC][RS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, half = lane >> 5, l31 = lane & 31;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const int chunk = blockIdx.z / p.ntaps, j = blockIdx.z - chunk * p.ntaps;
    const int sh = p.shift[j];
    const int r_lo = chunk * TG_RCHUNK, r_hi = min(p.R, r_lo + TG_RCHUNK);
    tg_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const bool y_rfast = (p.y_st == 1), x_rfast = (p.x_st == 1);
    const int x_mul = p.x_mul ? p.x_mul : 1, x_T = p.x_T ? p.x_T : p.T;
    for (int r0 = r_lo; r0 < r_hi; r0 += KC) {
#pragma unroll
        for (int i = 0; i < (KC * 64) / 256; ++i) {
            const int idx = i * 256 + tid;
            int kk, mm;
            if (y_rfast) { mm = idx / KC; kk = idx % KC; } else { kk = idx / 64; mm = idx % 64; }
            float v = 0.f;
            if (r0 + kk < r_hi && m0 + mm < p.M) {
                const int b = (r0 + kk) / p.T, t = (r0 + kk) - b * p.T;
                v = p.dY[(long)b * p.y_sz + (long)(m0 + mm) * p.y_sm + (long)t * p.y_st];
            }
            As[kk][mm] = v;
            int kb, nn;
            if (x_rfast) { nn = idx / KC; kb = idx % KC; } else { kb = idx / 64; nn = idx % 64; }
            float w = 0.f;
            if (r0 + kb < r_hi && n0 + nn < p.K) {
                const int b = (r0 + kb) / p.T, t = ((r0 + kb) - b * p.T) * x_mul + sh;
                if (t >= 0 && t < x_T) w = p.X[(long)b * p.x_sz + (long)(n0 + nn) * p.x_sk + (long)t * p.x_st];
            }
            Bs[kb][nn] = w;
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < KC; ks += 2) {
            const float a = As[ks + half][wm * 32 + l31];
            const float b = Bs[ks + half][wn * 32 + l31];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    float* __restrict__ out = p.part + (size_t)blockIdx.z * p.M * p.K;
    const int n = n0 + wn * 32 + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (m < p.M && n < p.K) out[(size_t)m * p.K + n] = acc[r];
    }
}

__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part, int nchunks, int ntaps, int M, int K, float* __restrict__ out,
                                                           long o_sm, long o_sk, long o_sj) {
    const size_t per = (size_t)ntaps * M * K;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= per) return;
    double s = 0.0;
    for (int c = 0; c < nchunks; ++c) s += (double)part[(size_t)c * per + i];
    const int k = (int)(i % K), m = (int)(i / K % M), j = (int)(i / ((size_t)K * M));
    out[(long)m * o_sm + (long)k * o_sk + (long)j * o_sj] = (float)s;
}

// ---------------------------------------------------------------------------------------------
// Column sums of src (R rows of stride ld, M columns of stride 1).  colsum_part_kernel: grid (ceil(M / 64), chunks); thread
// (g, l) = (tid / 64, tid % 64) adds rows g, g + 4, ... of its chunk for column 64 x + l in fp64, then the four g are added in
// order.  colsum_final_kernel adds the chunks in order and rounds once.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void colsum_part_kernel(const float* __restrict__ src, int R, int M, long ld, double* __restrict__ part) {
    __shared__ double sm[4][64];
    const int g = threadIdx.x >> 6, l = threadIdx.x & 63, m = blockIdx.x * 64 + l;
    const int r_lo = blockIdx.y * TG_RCHUNK, r_hi = min(R, r_lo + TG_RCHUNK);
    double s = 0.0;
    if (m < M)
        for (int r = r_lo + g; r < r_hi; r += 4) s += (double)src[(long)r * ld + m];
    sm[g][l] = s;
    __syncthreads();
    if (g == 0 && m < M) part[(size_t)blockIdx.y * M + m] = ((sm[0][l] + sm[1][l]) + sm[2][l]) + sm[3][l];
}
__global__ __launch_bounds__(256) void colsum_final_kernel(const double* __restrict__ part, int nchunks, int M, float* __restrict__ out0, float* __restrict__ out1) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    double s = 0.0;
    for (int c = 0; c < nchunks; ++c) s += part[(size_t)c * M + m];
    out0[m] = (float)s;
    if (out1) out1[m] = (float)s;
}

#endif  // PARROT_TRAIN_GEMM_TU

}  // namespace parrot
