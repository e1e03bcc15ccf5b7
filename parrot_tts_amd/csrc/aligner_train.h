// aligner_train.h -- the kernels that TRAIN the forced aligner (reference utils/aligner/model.py:5-48 under model.train(), and the
// backward of that stack): parrot_aligner_train_forward / _backward (host_aligner_train.hip).  Unlike the inference handle nothing
// here is packed, cached or folded: every weight is read from the device pointer the caller gives, in torch's layout, through
// strides, so an optimiser's in-place update is seen by the next call.  The matrix products are not here: the three k = 5 convs, the
// LSTM input projection, the Linear and all their gradients go through train_gemm.h.  This file holds what lies between them:
//   bn_train_kernel      BatchNorm1d forward on batch statistics (fp64, fixed order) or on the running ones; running-buffer update
//   bn_relu_bwd_kernel   BatchNorm backward on the batch statistics, fused with the ReLU backward
//   lstm_train_step / lstm_bwd_step   the recurrence keeping its gate activations and cell states, and its backward through time
// Rules, as in train_gemm.h: no floating-point atomics; every sum over B T that ends in one number is fp64 in a fixed order; nothing
// clamps with fmaxf, so a NaN stays a NaN.
// The launchers are defined in tu_aligner_train.hip, which alone sees the kernel bodies (PARROT_ALIGNER_TRAIN_TU).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wave_reduce.h"

namespace parrot {

constexpr int AT_BT = 16;         // batch rows per pass of the LSTM step kernels: their sums live in registers, nothing is staged in LDS
constexpr int AT_UNITS = 4;       // hidden units per workgroup of the LSTM step kernels (as LSTM_UNITS)

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

hipError_t launch_bn_train(const BnTrainParams& p, hipStream_t s);
hipError_t launch_bn_relu_bwd(const BnBwdParams& p, hipStream_t s);
hipError_t launch_lstm_train_step(const LstmTrainParams& p, hipStream_t s);
hipError_t launch_lstm_bwd_step(const LstmBwdParams& p, hipStream_t s);

#ifdef PARROT_ALIGNER_TRAIN_TU

// ---------------------------------------------------------------------------------------------
// bn_train_kernel: one workgroup per channel c over its n = B T values (padded frames included: the reference masks nothing).
// training: mean = sum x / n, var = sum (x - mean)^2 / n (biased), both fp64 with thread tid adding elements tid, tid + 256, ... and
// the fixed tree of block_sum; mean and rsqrt(var + eps) are rounded to fp32 once and kept for the backward;
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
        const double mean = block_sum(s, sm) / (double)n;
        s = 0.0;
        for (int i = tid; i < n; i += 256) {
            const int b = i / T, t = i - b * T;
            const double d = (double)x[b * bs + t] - mean;
            s += d * d;
        }
        const double var = block_sum(s, sm) / (double)n;
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
    s1 = block_sum(s1, sm);
    s2 = block_sum(s2, sm);
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
