// tte_loss.h -- ModelLoss of the text-to-unit model and its gradient (reference modules/loss.py:5-21, train.py:72-85).
// The launchers below are defined in tu_tte.hip, which alone sees the kernel bodies (PARROT_TTE_TU); host_tte_loss.hip validates
// and lays out the workspace.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace parrot {

// ---------------------------------------------------------------------------------------------
// ModelLoss (modules/loss.py:5-21): CrossEntropyLoss(ignore_index) over (N, V) channel-last fp32 logits + MSELoss of the
// log-durations over src_mask.  Stage 1: one wave per position -- max-shifted log-sum-exp in fp32, nll = log(sum) - (x[t] - max)
// (log_softmax's order), and whether the first-max argmax is the target; each block's 16 positions are added in fp64 in row
// order.  Stage 2 (one block): the block partials and the duration term, each thread a fixed strided slice, then a fixed LDS
// tree.  No atomics on values: two calls agree bit for bit.  Reads the logits once (V <= 1024 and 16-byte rows: from registers).
// The gradient (train.py:72-85, loss.backward()): loss_count_kernel counts the valid targets and the set mask bytes first (the
// scales w_code / n_valid and 2 w_dur / n_src must be known before a scaled element can be written) and writes the duration
// gradient; loss_rows_kernel<true> is stage 1 with one more step per row, g_code (softmax - onehot) from the registers that hold
// the row (an ignored row: zeros, a bad target: NaN); stage 2 is unchanged.  Every output element is written exactly once.
// ---------------------------------------------------------------------------------------------
constexpr int LOSS_WAVES = 16;      // positions per stage-1 block
constexpr int LOSS_CHUNKS = 4;      // float4 per lane held in registers: V <= 1024 on the vector path
constexpr int LOSS_REDUCE = 1024;   // stage-2 threads (and loss_count_kernel's)
struct LossCounts { int32_t n_valid, n_correct, n_bad, first_bad_row; };
struct LossScale { float g_code, g_dur; int32_t n_valid, n_src; };  // g_code = w_code / n_valid, g_dur = 2 w_dur / n_src: fp64, rounded once

// nll / cnt / bad: one entry per stage-1 block, ceil(N / LOSS_WAVES) of them.
// loss_rows_kernel + loss_reduce_kernel
hipError_t launch_tte_loss(const float* logits, const int64_t* targets, int N, int V, int64_t ignore_index, const float* log_dur, const int64_t* dur,
                           const uint8_t* src_mask, int n_src, double* nll, LossCounts* cnt, int64_t* bad, double* out, float* losses, hipStream_t s);
// The same with the gradient: count + duration gradient, rows + logit gradient (grad_logits nullable), the forward's reduction
hipError_t launch_tte_loss_grad(const float* logits, const int64_t* targets, int N, int V, int64_t ignore_index, const float* log_dur,
                                const int64_t* dur, const uint8_t* src_mask, int n_src, const double* weights, double* nll, LossCounts* cnt,
                                int64_t* bad, LossScale* scale, double* out, float* losses, float* grad_logits, float* grad_log_dur, hipStream_t s);

}  // namespace parrot

#ifdef PARROT_TTE_TU
#include "wave_reduce.h"

namespace parrot {

// weights (nullable: {1, 1}) = {w_code, w_dur} fp64; grad_log_dur (nullable) (n_src) <- g_dur (log_dur - log(dur + 1)) under the mask, 0 elsewhere
static __global__ __launch_bounds__(LOSS_REDUCE) void loss_count_kernel(const int64_t* __restrict__ tgt, int N, int V, int64_t ignore,
                                                                        const float* __restrict__ log_dur, const int64_t* __restrict__ dur,
                                                                        const uint8_t* __restrict__ src_mask, int n_src,
                                                                        const double* __restrict__ weights, LossScale* __restrict__ scale,
                                                                        float* __restrict__ grad_log_dur) {
    __shared__ int s_valid[LOSS_REDUCE], s_src[LOSS_REDUCE];
    const int tid = threadIdx.x;
    int nv = 0, ns = 0;
    for (int i = tid; i < N; i += LOSS_REDUCE) {
        const int64_t t = tgt[i];
        nv += t != ignore && t >= 0 && t < V;  // loss_rows_kernel's states 1 and 2
    }
    for (int i = tid; i < n_src; i += LOSS_REDUCE) ns += src_mask[i] != 0;
    s_valid[tid] = nv; s_src[tid] = ns;
    __syncthreads();
    for (int h = LOSS_REDUCE / 2; h > 0; h >>= 1) {
        if (tid < h) {
            s_valid[tid] += s_valid[tid + h];
            s_src[tid] += s_src[tid + h];
        }
        __syncthreads();
    }
    nv = s_valid[0]; ns = s_src[0];
    const double w_code = weights ? weights[0] : 1.0, w_dur = weights ? weights[1] : 1.0;
    // (nothing valid: the quotient is inf or NaN and multiplies nothing -- every row is ignored, every mask byte clear)
    const float g_code = (float)(w_code / (double)nv), g_dur = (float)(2.0 * w_dur / (double)ns);
    if (tid == 0) *scale = LossScale{g_code, g_dur, nv, ns};
    if (grad_log_dur)
        for (int i = tid; i < n_src; i += LOSS_REDUCE)
            grad_log_dur[i] = src_mask[i] ? g_dur * (log_dur[i] - logf((float)dur[i] + 1.0f)) : 0.f;  // the forward's difference
}

// GRAD: also grad (N, V) <- scale->g_code (softmax(x) - onehot(target)) per valid row, 0 for an ignored one, NaN for a bad target
template <bool GRAD>
static __global__ __launch_bounds__(64 * LOSS_WAVES) void loss_rows_kernel(const float* __restrict__ logits, const int64_t* __restrict__ tgt,
                                                                         int N, int V, int64_t ignore, double* __restrict__ part_nll,
                                                                         LossCounts* __restrict__ part_cnt, int64_t* __restrict__ part_bad,
                                                                         const LossScale* __restrict__ scale, float* __restrict__ grad) {
    __shared__ double s_nll[LOSS_WAVES];
    __shared__ int s_st[LOSS_WAVES];  // 0 skipped, 1 valid, 2 valid and argmax == target, 3 target out of range
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * LOSS_WAVES + wave;  // wave-uniform: every branch below is uniform
    int st = 0;
    double nll = 0.0;
    if (row < N) {
        const float* __restrict__ x = logits + (size_t)row * V;
        const bool vec = (V & 3) == 0 && V <= 256 * LOSS_CHUNKS && ((uintptr_t)logits & 15) == 0;
        // (vector path: the row's loads are issued together with the target's, not behind it -- an ignored row reads its logits too)
        float4 r[LOSS_CHUNKS];
        if (vec) {
#pragma unroll
            for (int k = 0; k < LOSS_CHUNKS; ++k) {
                const int i = (k * 64 + lane) * 4;
                r[k] = i < V ? *reinterpret_cast<const float4*>(x + i) : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
            }
        }
        const int64_t tg = tgt[row];
        float* __restrict__ g = GRAD ? grad + (size_t)row * V : nullptr;
        const bool gvec = ((uintptr_t)grad & 15) == 0;  // (V % 4 == 0 on the vector path: every row of an aligned base is aligned)
        auto put4 = [&](int i, float a, float b, float c, float d) {
            if (gvec) {
                *reinterpret_cast<float4*>(g + i) = make_float4(a, b, c, d);
            } else {
                g[i] = a; g[i + 1] = b; g[i + 2] = c; g[i + 3] = d;
            }
        };
        if (tg == ignore || tg < 0 || tg >= V) {
            st = tg == ignore ? 0 : 3;
            if constexpr (GRAD) {  // an ignored row is 0 throughout; nothing is indexed through a bad target: its row is NaN
                const float fill = st == 0 ? 0.f : NAN;
                if (vec) {
#pragma unroll
                    for (int k = 0; k < LOSS_CHUNKS; ++k) {
                        const int i = (k * 64 + lane) * 4;
                        if (i < V) put4(i, fill, fill, fill, fill);
                    }
                } else {
                    for (int i = lane; i < V; i += 64) g[i] = fill;
                }
            }
        } else {
            const float xt = x[tg];
            float m = -INFINITY, s = 0.f;
            int mi = V;
            if (vec) {
#pragma unroll
                for (int k = 0; k < LOSS_CHUNKS; ++k) {
                    const int i = (k * 64 + lane) * 4;
                    const float e[4] = {r[k].x, r[k].y, r[k].z, r[k].w};
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (i + j < V && e[j] > m) { m = e[j]; mi = i + j; }
                }
                for (int o = 32; o > 0; o >>= 1) {  // (value, index): larger value, then smaller index -- torch.argmax's first maximum
                    const float om = __shfl_xor(m, o);
                    const int oi = __shfl_xor(mi, o);
                    if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
                }
#pragma unroll
                for (int k = 0; k < LOSS_CHUNKS; ++k) {
                    const int i = (k * 64 + lane) * 4;
                    const float e[4] = {r[k].x, r[k].y, r[k].z, r[k].w};
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (i + j < V) s += expf(e[j] - m);
                }
            } else {  // any V / alignment: two passes over the row (the second from cache)
                for (int i = lane; i < V; i += 64)
                    if (x[i] > m) { m = x[i]; mi = i; }
                for (int o = 32; o > 0; o >>= 1) {
                    const float om = __shfl_xor(m, o);
                    const int oi = __shfl_xor(mi, o);
                    if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
                }
                for (int i = lane; i < V; i += 64) s += expf(x[i] - m);
            }
            s = wave_sum(s);
            nll = (double)(logf(s) - (xt - m));
            st = mi == (int)tg ? 2 : 1;
            if constexpr (GRAD) {
                const float gc = scale->g_code, inv = 1.0f / s;
                const int t = (int)tg;
                if (vec) {  // from the registers that hold the row
#pragma unroll
                    for (int k = 0; k < LOSS_CHUNKS; ++k) {
                        const int i = (k * 64 + lane) * 4;
                        if (i < V)
                            put4(i, gc * (expf(r[k].x - m) * inv - (i == t ? 1.f : 0.f)), gc * (expf(r[k].y - m) * inv - (i + 1 == t ? 1.f : 0.f)),
                                 gc * (expf(r[k].z - m) * inv - (i + 2 == t ? 1.f : 0.f)), gc * (expf(r[k].w - m) * inv - (i + 3 == t ? 1.f : 0.f)));
                    }
                } else {  // a third pass, from cache
                    for (int i = lane; i < V; i += 64) g[i] = gc * (expf(x[i] - m) * inv - (i == t ? 1.f : 0.f));
                }
            }
        }
    }
    if (lane == 0) {
        s_nll[wave] = nll;
        s_st[wave] = st;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0;
        LossCounts c{0, 0, 0, -1};
        int64_t bad_t = 0;
        for (int w = 0; w < LOSS_WAVES; ++w) {
            a += s_nll[w];
            c.n_valid += s_st[w] == 1 || s_st[w] == 2;
            c.n_correct += s_st[w] == 2;
            if (s_st[w] == 3 && c.n_bad++ == 0) {
                c.first_bad_row = blockIdx.x * LOSS_WAVES + w;
                bad_t = tgt[c.first_bad_row];
            }
        }
        part_nll[blockIdx.x] = a;
        part_cnt[blockIdx.x] = c;
        part_bad[blockIdx.x] = bad_t;
    }
}

// out[0..7] = {sum nll, n_valid, n_correct, sum sq, n_src, n_bad, first bad target, 0}; losses (nullable) = {total, code, dur} fp32
static __global__ __launch_bounds__(LOSS_REDUCE) void loss_reduce_kernel(const double* __restrict__ part_nll, const LossCounts* __restrict__ part_cnt,
                                                                         const int64_t* __restrict__ part_bad, int nblk,
                                                                         const float* __restrict__ log_dur, const int64_t* __restrict__ dur,
                                                                         const uint8_t* __restrict__ src_mask, int n_src, double* __restrict__ out,
                                                                         float* __restrict__ losses) {
    __shared__ double s_nll[LOSS_REDUCE], s_sq[LOSS_REDUCE];
    __shared__ int s_valid[LOSS_REDUCE], s_correct[LOSS_REDUCE], s_bad[LOSS_REDUCE], s_src[LOSS_REDUCE];
    __shared__ int s_first[LOSS_REDUCE];  // lowest-numbered block with an out-of-range target (nblk: none)
    const int tid = threadIdx.x;
    double a = 0.0, q = 0.0;
    int nv = 0, nc = 0, nb = 0, ns = 0, first = nblk;
    for (int i = tid; i < nblk; i += LOSS_REDUCE) {
        const LossCounts c = part_cnt[i];
        a += part_nll[i];
        nv += c.n_valid;
        nc += c.n_correct;
        nb += c.n_bad;
        if (c.n_bad && i < first) first = i;
    }
    for (int i = tid; i < n_src; i += LOSS_REDUCE) {
        if (!src_mask[i]) continue;
        const float d = log_dur[i] - logf((float)dur[i] + 1.0f);  // log(duration.float() + 1), loss.py:14
        q += (double)(d * d);
        ++ns;
    }
    s_nll[tid] = a; s_sq[tid] = q; s_valid[tid] = nv; s_correct[tid] = nc; s_bad[tid] = nb; s_src[tid] = ns; s_first[tid] = first;
    __syncthreads();
    for (int h = LOSS_REDUCE / 2; h > 0; h >>= 1) {
        if (tid < h) {
            s_nll[tid] += s_nll[tid + h];
            s_sq[tid] += s_sq[tid + h];
            s_valid[tid] += s_valid[tid + h];
            s_correct[tid] += s_correct[tid + h];
            s_bad[tid] += s_bad[tid + h];
            s_src[tid] += s_src[tid + h];
            s_first[tid] = min(s_first[tid], s_first[tid + h]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        out[0] = s_nll[0];
        out[1] = (double)s_valid[0];
        out[2] = (double)s_correct[0];
        out[3] = s_sq[0];
        out[4] = (double)s_src[0];
        out[5] = (double)s_bad[0];
        out[6] = s_first[0] < nblk ? (double)part_bad[s_first[0]] : 0.0;
        out[7] = 0.0;
        if (losses) {
            const float code = (float)(s_nll[0] / (double)s_valid[0]);  // 0 / 0 = NaN: an all-ignored batch, as torch gives
            const float durl = (float)(s_sq[0] / (double)s_src[0]);
            losses[0] = code + durl;  // loss.py:19, in fp32
            losses[1] = code;
            losses[2] = durl;
        }
    }
}

}  // namespace parrot

#endif  // PARROT_TTE_TU
