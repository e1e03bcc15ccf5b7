// aligner_train.h -- the kernels that TRAIN the forced aligner (reference utils/aligner/model.py:5-48 under model.train(), and the
// backward of that stack): parrot_aligner_train_forward / _backward (host_aligner_train.hip).  Unlike the inference handle nothing
// here is packed, cached or folded: every weight is read from the device pointer the caller gives, in torch's layout, through
// strides, so an optimiser's in-place update is seen by the next call.
//   tap_gemm_kernel      Y[z] (M x N) = sum_j A_j (M x K) shift_j(X[z]) (K x N), any strides: the three k = 5 convs, the LSTM input
//                        projection, the Linear, and every data gradient (A transposed through its strides, taps flipped)
//   wgrad_kernel         dA_j (M x K) = sum_(b, t) dY[b][m][t] X[b][k][t + shift_j] as fp32 partials over fixed blocks of B T,
//   wgrad_reduce_kernel  which adds the partials in block order in fp64 and rounds once
//   colsum_*             bias gradients: the same two-level fixed-order scheme over the rows of a (B T, M) array
//   bn_train_kernel      BatchNorm1d forward on batch statistics (fp64, fixed order) or on the running ones; running-buffer update
//   bn_relu_bwd_kernel   BatchNorm backward on the batch statistics, fused with the ReLU backward
//   lstm_train_step / lstm_bwd_step   the recurrence keeping its gate activations and cell states, and its backward through time
// All products are exact fp32 (v_mfma_f32_32x32x2_f32, fp32 FMA), accumulated in fp32; every sum over B T that ends in one number
// is fp64.  No floating-point atomics: two calls on the same inputs agree bit for bit.  Nothing here clamps with fmaxf, so a NaN
// stays a NaN through every kernel (the ReLU is `v < 0 ? 0 : v`).
// The launchers are defined in tu_aligner_train.hip, which alone sees the kernel bodies (PARROT_ALIGNER_TRAIN_TU).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace parrot {

constexpr int AT_MAX_TAPS = 11;    // the widest conv that goes through tap_gemm_kernel: the vocoder's k = 11 (the TTE's FFN has 9, the aligner 5)
constexpr int AT_RCHUNK = 256;    // (b, t) pairs per weight-gradient / column-sum partial: the fixed block of the two-level sums
constexpr int AT_ACC_FLUSH = 8;   // tap_gemm_kernel moves its accumulator into a second one every 8 x 32 products
constexpr int AT_BT = 16;         // batch rows per pass of the LSTM step kernels: their sums live in registers, nothing is staged in LDS
constexpr int AT_UNITS = 4;       // hidden units per workgroup of the LSTM step kernels (as LSTM_UNITS)

// Y[z][m][n] = act(sum_j sum_k A_j[m][k] X[z][k][n + shift_j] + bias0[m] + bias1[m]); X is zero outside 0 <= n + shift_j < N.
// The fields after `relu` serve the vocoder's training (voc_train.h); zero in each of them is the line above, bit for bit:
//   X is read at column n x_mul + shift_j and is zero outside [0, x_n)  (x_mul = 0: 1; x_n = 0: N): a transposed conv's phases and its
//   data gradient;  then, after the bias:  v = mask[z][m][n] > 0 ? v : v mslope  (a leaky ReLU's backward on its saved output),
//   v += res[z][m][n]  (a residual), both at C's strides;  and after `relu`:  v = v > 0 ? v : v lslope  when lrelu.
struct TapGemmParams {
    const float* A[AT_MAX_TAPS];  // tap j: A_j[m][k] at A[j] + m a_sm + k a_sk
    long x_off[AT_MAX_TAPS];      // tap j reads X[z] + x_off[j] (a column block of a wider array)
    int shift[AT_MAX_TAPS];
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
};
// part[chunk][j][m][k] = sum over the chunk's (b, t) of dY[b][m][t] X[b][k][t + shift_j]; chunk c covers r = b T + t in
// [c AT_RCHUNK, (c + 1) AT_RCHUNK).  X is zero outside 0 <= t + shift_j < T.
// x_mul, x_T (zero: 1 and T, the line above): X is read at t x_mul + shift_j and is zero outside [0, x_T): the weight gradient of a
// transposed conv, whose input is in dY's role and whose output gradient, u times as long, in X's.
struct WgradParams {
    const float* dY;  // dY[b][m][t] at dY + b y_sz + m y_sm + t y_st
    const float* X;   // X[b][k][t] at X + b x_sz + k x_sk + t x_st
    float* part;
    int M, K, T, R, ntaps;
    int shift[AT_MAX_TAPS];
    long y_sz, y_sm, y_st, x_sz, x_sk, x_st;
    int x_mul, x_T;
};
struct BnTrainParams {
    const float* x;   // (B, C, T): the ReLU's output
    float* y;         // (B, C, T)
    const float *gamma, *beta;
    float *run_mean, *run_var;  // read when !training; updated in place when training
    float *mean, *invstd;       // (C) out: the statistics the apply used
    int B, C, T, training;
    float eps;
};
struct BnBwdParams {
    const float* dy;  // (B, C, T)
    const float* x;   // (B, C, T): the ReLU's output, which is the BatchNorm's input
    float* dx;        // (B, C, T): gradient at the conv's output (may be dy)
    const float *gamma, *mean, *invstd;
    float *dgamma, *dbeta;  // nullable
    int B, C, T;
};
struct LstmTrainParams {
    const float* w_hh[2];  // (4H, H) each, torch layout
    const float* xproj;    // (B, T, 8H)
    const float* h_prev;   // [2][B][H]
    float* h_next;
    float* c;              // [2][B][H]
    float* out;            // (B, T, 2H)
    float* gates;          // (B, T, 8H): sigmoid(i), sigmoid(f), tanh(g), sigmoid(o) per direction
    float* c_all;          // (B, T, 2H)
    int B, T, H, step;
};
struct LstmBwdParams {
    const float* w_hh_t;  // [2][H][4H]: W_hh transposed
    const float* gates;   // (B, T, 8H)
    const float* c_all;   // (B, T, 2H)
    const float* dout;    // (B, T, 2H)
    float* dgates;        // (B, T, 8H): gradient at the gate pre-activations
    float* dc;            // [2][B][H], zero before step 0
    int B, T, H, step;    // forward direction at t = T - 1 - step, backward at t = step
};

hipError_t launch_tap_gemm(const TapGemmParams& p, int Z, hipStream_t s);
int wgrad_chunks(int R);
hipError_t launch_wgrad(const WgradParams& p, hipStream_t s);
// out[m o_sm + k o_sk + j o_sj] = fl32(sum_c part[c][j][m][k]) in chunk order, fp64
hipError_t launch_wgrad_reduce(const float* part, int nchunks, int ntaps, int M, int K, float* out, long o_sm, long o_sk, long o_sj, hipStream_t s);
// out0[m] (and out1[m], nullable) = fl32(sum_r src[r ld + m]), r < R: fp64 partials per AT_RCHUNK rows (part: chunks x M doubles)
hipError_t launch_colsum(const float* src, int R, int M, long ld, double* part, float* out0, float* out1, hipStream_t s);
hipError_t launch_bn_train(const BnTrainParams& p, hipStream_t s);
hipError_t launch_bn_relu_bwd(const BnBwdParams& p, hipStream_t s);
hipError_t launch_lstm_train_step(const LstmTrainParams& p, hipStream_t s);
hipError_t launch_lstm_bwd_step(const LstmBwdParams& p, hipStream_t s);

#ifdef PARROT_ALIGNER_TRAIN_TU

typedef float at_f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------------
// tap_gemm_kernel: grid (ceil(N / 64), ceil(M / 64), Z), four waves, each one 32 x 32 tile of the 64 x 64 block on
// v_mfma_f32_32x32x2_f32.  Both operands are staged K-major in LDS ([k][m], [k][n], row stride 65) through their strides, 32 k per
// pass; whichever index has stride 1 runs along the lanes of the staging loads.  Rows m >= M, columns n >= N and k >= K are staged
// as zeros on BOTH sides, so a NaN never meets a padding zero in a stored element.  The fp32 chain of one accumulator is at most
// AT_ACC_FLUSH x 32 products long: it is then added into a second accumulator and cleared.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tap_gemm_kernel(const TapGemmParams p) {
    constexpr int KC = 32, RS = 65;
    __shared__ float As[KC][RS];
    __shared__ float Bs[KC][RS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, half = lane >> 5, l31 = lane & 31;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const float* __restrict__ X = p.X + (long)blockIdx.z * p.x_sz;
    at_f32x16 acc, tot;
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
            if (++since == AT_ACC_FLUSH) {
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
            if (p.mask || p.res) {
#pragma clang fp contract(off)  // (the product and the sum are rounded one after the other, as torch rounds them)
                const long oz = (long)blockIdx.z * p.c_sz + o;
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
// wgrad_kernel: the same tile on the transposed problem: the reduction runs over r = b T + t inside one fixed chunk of AT_RCHUNK
// pairs, rows are dY's channels, columns X's.  grid (ceil(K / 64), ceil(M / 64), chunks x ntaps); blockIdx.z = chunk ntaps + j.
// Every element of part is written (a chunk is never empty: chunks = ceil(R / AT_RCHUNK)).
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
    const int r_lo = chunk * AT_RCHUNK, r_hi = min(p.R, r_lo + AT_RCHUNK);
    at_f32x16 acc;
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
    const int r_lo = blockIdx.y * AT_RCHUNK, r_hi = min(R, r_lo + AT_RCHUNK);
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

// fp64 sum over the 256 threads of a workgroup in a fixed tree; every thread gets the result
__device__ __forceinline__ double at_block_sum(double v, double* sm) {
    const int tid = threadIdx.x;
    sm[tid] = v;
    __syncthreads();
#pragma unroll
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) sm[tid] += sm[tid + o];
        __syncthreads();
    }
    const double r = sm[0];
    __syncthreads();
    return r;
}

// ---------------------------------------------------------------------------------------------
// bn_train_kernel: one workgroup per channel c over its n = B T values (padded frames included: the reference masks nothing).
// training: mean = sum x / n, var = sum (x - mean)^2 / n (biased), both fp64 with thread tid adding elements tid, tid + 256, ... and
// the fixed tree of at_block_sum; mean and rsqrt(var + eps) are rounded to fp32 once and kept for the backward;
// running_mean <- 0.9 running_mean + 0.1 mean, running_var <- 0.9 running_var + 0.1 var n / (n - 1), formed in fp64 and rounded once.
// Otherwise: the running statistics, and no buffer is written.
// Then y = (x - mean) rsqrt(var + eps) gamma + beta in fp32.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bn_train_kernel(const BnTrainParams p) {
    __shared__ double sm[256];
    const int c = blockIdx.x, tid = threadIdx.x, T = p.T;
    const int n = p.B * T;
    const float* __restrict__ x = p.x + (size_t)c * T;
    const size_t bs = (size_t)p.C * T;
    float mean_f, invstd_f;
    if (p.training) {
        double s = 0.0;
        for (int i = tid; i < n; i += 256) {
            const int b = i / T, t = i - b * T;
            s += (double)x[b * bs + t];
        }
        const double mean = at_block_sum(s, sm) / (double)n;
        s = 0.0;
        for (int i = tid; i < n; i += 256) {
            const int b = i / T, t = i - b * T;
            const double d = (double)x[b * bs + t] - mean;
            s += d * d;
        }
        const double var = at_block_sum(s, sm) / (double)n;
        mean_f = (float)mean;
        invstd_f = (float)(1.0 / sqrt(var + (double)p.eps));
        if (tid == 0) {
            p.run_mean[c] = (float)(0.9 * (double)p.run_mean[c] + 0.1 * mean);
            p.run_var[c] = (float)(0.9 * (double)p.run_var[c] + 0.1 * (var * (double)n / (double)(n - 1)));
        }
    } else {
        mean_f = p.run_mean[c];
        invstd_f = (float)(1.0 / sqrt((double)p.run_var[c] + (double)p.eps));
    }
    if (tid == 0) {
        p.mean[c] = mean_f;
        p.invstd[c] = invstd_f;
    }
    const float g = p.gamma[c], be = p.beta[c];
    float* __restrict__ y = p.y + (size_t)c * T;
    for (int i = tid; i < n; i += 256) {
        const int b = i / T, t = i - b * T;
        y[b * bs + t] = fmaf(__fmul_rn(__fsub_rn(x[b * bs + t], mean_f), invstd_f), g, be);
    }
}

// ---------------------------------------------------------------------------------------------
// bn_relu_bwd_kernel: one workgroup per channel.  With xh = (x - mean) invstd:  dbeta = sum dy, dgamma = sum dy xh (fp64, the
// order of bn_train_kernel), then dx = gamma invstd (dy - dbeta / n - xh dgamma / n) where the conv's output was > 0 (x > 0: x is
// the ReLU's output) and 0 elsewhere.  dx may be dy.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bn_relu_bwd_kernel(const BnBwdParams p) {
    __shared__ double sm[256];
    const int c = blockIdx.x, tid = threadIdx.x, T = p.T;
    const int n = p.B * T;
    const size_t bs = (size_t)p.C * T, co = (size_t)c * T;
    const float* __restrict__ x = p.x + co;
    const float* dy = p.dy + co;
    float* dx = p.dx + co;
    const float mean = p.mean[c], invstd = p.invstd[c];
    double s1 = 0.0, s2 = 0.0;
    for (int i = tid; i < n; i += 256) {
        const int b = i / T, t = i - b * T;
        const float xh = __fmul_rn(__fsub_rn(x[b * bs + t], mean), invstd);
        const double d = (double)dy[b * bs + t];
        s1 += d;
        s2 += d * (double)xh;
    }
    s1 = at_block_sum(s1, sm);
    s2 = at_block_sum(s2, sm);
    if (tid == 0) {
        if (p.dbeta) p.dbeta[c] = (float)s1;
        if (p.dgamma) p.dgamma[c] = (float)s2;
    }
    const float m1 = (float)(s1 / (double)n), m2 = (float)(s2 / (double)n);
    const float k = __fmul_rn(p.gamma[c], invstd);
    for (int i = tid; i < n; i += 256) {
        const int b = i / T, t = i - b * T;
        const float xv = x[b * bs + t];
        const float xh = __fmul_rn(__fsub_rn(xv, mean), invstd);
        float v;
        {
            // (HIP's __fmul_rn / __fsub_rn are a plain `*` and `-` compiled under the default -ffp-contract=fast, so nested as
            // a - xh m2 they fuse into one FMA and dx is not the chain of single roundings documented above: plain operators
            // under the pragma stay apart)
#pragma clang fp contract(off)
            v = k * ((dy[b * bs + t] - m1) - xh * m2);
        }
        dx[b * bs + t] = xv > 0.f ? v : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------
// lstm_train_step_kernel: lstm_step_kernel (aligner.h) reading each direction's W_hh where torch holds it, and keeping what the
// backward needs: the four gate activations and c_t of every step.  Same thread layout and the same order of every sum, but h_prev
// (B x H floats) is read straight from global memory as float4, AT_BT batch rows per pass, instead of through LDS.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lstm_train_step_kernel(const LstmTrainParams p) {
    __shared__ float gates[16 * AT_BT];
    const int H = p.H, B = p.B, T = p.T;
    const int dir = blockIdx.y, u0 = blockIdx.x * AT_UNITS, tid = threadIdx.x;
    const int t = dir ? T - 1 - p.step : p.step;
    const int r = tid >> 4, q = tid & 15;
    const float* __restrict__ wrow = p.w_hh[dir] + ((size_t)(r >> 2) * H + u0 + (r & 3)) * H;
    for (int b0 = 0; b0 < B; b0 += AT_BT) {
        const int nb = min(AT_BT, B - b0);
        // (rows bb >= nb re-read row nb - 1, so the loads stay unconditional; their sums are never used)
        const float* __restrict__ hp = p.h_prev + ((size_t)dir * B + b0) * H;
        float acc[AT_BT];
#pragma unroll
        for (int bb = 0; bb < AT_BT; ++bb) acc[bb] = 0.f;
#pragma unroll 2
        for (int k0 = 4 * q; k0 < H; k0 += 64) {  // (H % 16 == 0: k0 + 3 < H)
            const float4 w4 = *reinterpret_cast<const float4*>(wrow + k0);
#pragma unroll
            for (int bb = 0; bb < AT_BT; ++bb) {
                const float4 h4 = *reinterpret_cast<const float4*>(hp + (size_t)min(bb, nb - 1) * H + k0);
                acc[bb] = fmaf(w4.x, h4.x, acc[bb]);
                acc[bb] = fmaf(w4.y, h4.y, acc[bb]);
                acc[bb] = fmaf(w4.z, h4.z, acc[bb]);
                acc[bb] = fmaf(w4.w, h4.w, acc[bb]);
            }
        }
#pragma unroll
        for (int bb = 0; bb < AT_BT; ++bb) {
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) acc[bb] += __shfl_xor(acc[bb], o);  // (stays inside the row's 16 lanes)
            if (q == 0) gates[r * AT_BT + bb] = acc[bb];
        }
        __syncthreads();
        if (tid < AT_UNITS * AT_BT) {
            const int uu = tid & (AT_UNITS - 1), bb = tid / AT_UNITS;
            if (bb < nb) {
                const int b = b0 + bb, unit = u0 + uu;
                const size_t go8 = ((size_t)b * T + t) * 8 * H + (size_t)dir * 4 * H + unit;
                const float* __restrict__ xp = p.xproj + go8;
                const float gi = xp[0] + gates[(0 * AT_UNITS + uu) * AT_BT + bb];
                const float gf = xp[H] + gates[(1 * AT_UNITS + uu) * AT_BT + bb];
                const float gg = xp[2 * H] + gates[(2 * AT_UNITS + uu) * AT_BT + bb];
                const float go = xp[3 * H] + gates[(3 * AT_UNITS + uu) * AT_BT + bb];
                const float i_ = 1.f / (1.f + expf(-gi)), f_ = 1.f / (1.f + expf(-gf)), g_ = tanhf(gg), o_ = 1.f / (1.f + expf(-go));
                const size_t ci = ((size_t)dir * B + b) * H + unit;
                const float cn = fmaf(f_, p.c[ci], i_ * g_);  // (lstm_step_kernel's own FMA: see the note there)
                const float hn = o_ * tanhf(cn);
                p.c[ci] = cn;
                p.h_next[ci] = hn;
                const size_t o2 = ((size_t)b * T + t) * 2 * H + (size_t)dir * H + unit;
                p.out[o2] = hn;
                p.c_all[o2] = cn;
                float* __restrict__ ga = p.gates + go8;
                ga[0] = i_;
                ga[H] = f_;
                ga[2 * H] = g_;
                ga[3 * H] = o_;
            }
        }
        __syncthreads();  // (gates is rewritten by the next pass)
    }
}

// ---------------------------------------------------------------------------------------------
// lstm_bwd_step_kernel: one launch takes both directions one step back through time.  grid (H / AT_UNITS, 2): workgroup (x, dir)
// owns hidden units [4x, 4x + 4) of direction dir.  The forward direction runs t = T - 1 .. 0, the backward one t = 0 .. T - 1, and
// the step before this one was t' = t + 1 resp. t - 1.
//   dh_rec[b][u] = sum_r W_hh[r][u] dgates[b][t'][r]  (r over the 4H gate rows; 0 at step 0): wave w of the workgroup owns unit
//   4x + w; its lane q adds rows 4q .. 4q + 3, 4q + 256 .. of W_hh^T's row u in fp32 FMA, then a fixed xor tree over the 64 lanes;
//   AT_BT batch rows per pass.  dgates[t'] (B x 4H floats) is read straight from global memory as float4: the four waves of a
//   workgroup read the same lines, and staging it in LDS first cost two barriers per 1024 rows and more time than the products.
// Then one thread per (unit, batch row):  dh = dout[t] + dh_rec;  do = dh tanh(c);  dc += dh o (1 - tanh(c)^2);
//   di = dc g, df = dc c_prev, dg = dc i;  dgates[t] = (di i (1 - i), df f (1 - f), dg (1 - g^2), do o (1 - o));  dc <- dc f.
// c_prev is c at the step the FORWARD pass took before t (0 at its first).  Stream order is the only synchronisation.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lstm_bwd_step_kernel(const LstmBwdParams p) {
    __shared__ float rec[AT_UNITS][AT_BT];
    const int H = p.H, B = p.B, T = p.T, H4 = 4 * p.H;
    const int dir = blockIdx.y, u0 = blockIdx.x * AT_UNITS, tid = threadIdx.x;
    const int t = dir ? p.step : T - 1 - p.step;
    const int t_done = dir ? t - 1 : t + 1;  // the step this pass took before t
    const int t_cprev = dir ? t + 1 : t - 1;  // the step the forward pass took before t
    const int r = tid >> 6, q = tid & 63;
    const float* __restrict__ wrow = p.w_hh_t + ((size_t)dir * H + u0 + r) * H4;
    const size_t row8 = (size_t)T * 8 * H;  // one batch row of dgates
    for (int b0 = 0; b0 < B; b0 += AT_BT) {
        const int nb = min(AT_BT, B - b0);
        float acc[AT_BT];
#pragma unroll
        for (int bb = 0; bb < AT_BT; ++bb) acc[bb] = 0.f;
        if (p.step > 0) {
            // (rows bb >= nb re-read row nb - 1, so the loads stay unconditional; their sums are never used)
            const float* __restrict__ dg = p.dgates + ((size_t)b0 * T + t_done) * 8 * H + (size_t)dir * H4;
#pragma unroll 2
            for (int k0 = 4 * q; k0 < H4; k0 += 256) {  // (4H % 64 == 0: k0 + 3 < 4H)
                const float4 w4 = *reinterpret_cast<const float4*>(wrow + k0);
#pragma unroll
                for (int bb = 0; bb < AT_BT; ++bb) {
                    const float4 d4 = *reinterpret_cast<const float4*>(dg + (size_t)min(bb, nb - 1) * row8 + k0);
                    acc[bb] = fmaf(w4.x, d4.x, acc[bb]);
                    acc[bb] = fmaf(w4.y, d4.y, acc[bb]);
                    acc[bb] = fmaf(w4.z, d4.z, acc[bb]);
                    acc[bb] = fmaf(w4.w, d4.w, acc[bb]);
                }
            }
        }
#pragma unroll
        for (int bb = 0; bb < AT_BT; ++bb) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc[bb] += __shfl_xor(acc[bb], o);
            if (q == 0) rec[r][bb] = acc[bb];
        }
        __syncthreads();
        if (tid < AT_UNITS * AT_BT) {
            const int uu = tid & (AT_UNITS - 1), bb = tid / AT_UNITS;
            if (bb < nb) {
                const int b = b0 + bb, unit = u0 + uu;
                const size_t o2 = ((size_t)b * T + t) * 2 * H + (size_t)dir * H + unit;
                const size_t o8 = ((size_t)b * T + t) * 8 * H + (size_t)dir * H4 + unit;
                const float i_ = p.gates[o8], f_ = p.gates[o8 + H], g_ = p.gates[o8 + 2 * H], o_ = p.gates[o8 + 3 * H];
                const float cp = (t_cprev >= 0 && t_cprev < T) ? p.c_all[((size_t)b * T + t_cprev) * 2 * H + (size_t)dir * H + unit] : 0.f;
                const float tc = tanhf(p.c_all[o2]);
                const float dh = p.dout[o2] + rec[uu][bb];
                const size_t ci = ((size_t)dir * B + b) * H + unit;
                const float dct = fmaf(dh * o_, 1.f - tc * tc, p.dc[ci]);
                float* __restrict__ dgo = p.dgates + o8;
                dgo[0] = dct * g_ * (i_ * (1.f - i_));
                dgo[H] = dct * cp * (f_ * (1.f - f_));
                dgo[2 * H] = dct * i_ * (1.f - g_ * g_);
                dgo[3 * H] = dh * tc * (o_ * (1.f - o_));
                p.dc[ci] = dct * f_;
            }
        }
        __syncthreads();  // (rec is rewritten by the next pass)
    }
}

#endif  // PARROT_ALIGNER_TRAIN_TU

}  // namespace parrot
