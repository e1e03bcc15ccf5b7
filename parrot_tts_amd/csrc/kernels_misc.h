// kernels_misc.h -- the HBM-bound glue kernels of the Parrot-TTS path (gathers, LayerNorm, softmax,
// duration rounding, length regulator, argmax).  All activations are channel-first (B, C, T).
// Include it from ONE unit only (the one that launches these): a `static __global__` kernel is emitted by every unit that sees it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "conv_mfma.h"  // (f32x16)
#include "wave_reduce.h"

namespace parrot {

// ---------------------------------------------------------------------------------------------
// TTE input: x[b, c, s] = tok_emb[phones[b,s]][c] + pe[S][c]   (parrot.py:94-95, fft.py:17-19, Q1)
// row_len (nullable): row-exact mode, pe[row_len[b]] -- the single row the reference adds when it runs that utterance alone.
// ---------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void tte_embed_kernel(const int64_t* __restrict__ phones, const float* __restrict__ emb,
                                                        const float* __restrict__ pe, const int32_t* __restrict__ row_len,
                                                        float* __restrict__ x, int S, int D, int vocab, int* __restrict__ err) {
    __shared__ float tile[64][65];
    const int s0 = blockIdx.x * 64, c0 = blockIdx.y * 64, b = blockIdx.z;
    const float* __restrict__ pe_row = pe + (size_t)(row_len ? min(max(row_len[b], 0), S) : S) * D;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int r = ty; r < 64; r += 4) {
        const int s = s0 + r, c = c0 + tx;
        float v = 0.f;
        if (s < S && c < D) {
            int64_t id = phones[(size_t)b * S + s];
            if (id < 0 || id >= vocab) { atomicExch(err, 3); id = 0; }
            v = pe_row[c] + emb[(size_t)id * D + c];
        }
        tile[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int c = c0 + r, s = s0 + tx;
        if (c < D && s < S) x[((size_t)b * D + c) * S + s] = tile[tx][r];
    }
}

// x[b, c, t] += tab[id[b]][c]      (speaker embedding add, parrot.py:98-99, Q6: all positions incl. pads)
static __global__ void add_channel_vec_kernel(float* __restrict__ x, const int64_t* __restrict__ id, const float* __restrict__ tab,
                                       int C, int T, int n_rows, size_t total, int* __restrict__ err) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = (int)((i / T) % C);
    const int b = (int)(i / ((size_t)T * C));
    int64_t s = id[b];
    if (s < 0 || s >= n_rows) { atomicExch(err, 4); s = 0; }
    x[i] = x[i] + tab[(size_t)s * C + c];
}

// ---------------------------------------------------------------------------------------------
// LayerNorm over channels of a channel-first tensor (fft.py:91-92,98-99; duration.py:32,36):
// biased variance, eps inside the sqrt, affine.  Optional ReLU on the input (duration predictor:
// Conv -> ReLU -> LayerNorm).  Two passes (mean, then centred variance), cross-wave combine through LDS.
// ---------------------------------------------------------------------------------------------
// NW waves per block split the channels (c = wave, wave + NW, ...); lane = time step, so every load / store is a
// coalesced 256-byte row segment.  For C <= NW * 16 a thread's channel values stay in registers (one global read);
// wider layers re-read them per pass.  (NW = 16: 16 waves per (batch row, 64 steps) keep a CU busy where 4 left it
// latency-bound.)
template <int NW>
__global__ __launch_bounds__(NW * 64) void layernorm_cf_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, float* __restrict__ y, int C, int T,
                                                                float eps, int relu_in) {
    __shared__ float red[NW][64];
    constexpr int MAXV = 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = blockIdx.x * 64 + lane, b = blockIdx.y;
    const bool ok = t < T;
    const float* xb = x + (size_t)b * C * T + (ok ? t : 0);
    const bool in_regs = C <= NW * MAXV;
    float vals[MAXV];
    float s = 0.f;
    if (in_regs) {
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = wave + NW * i;
            float v = (c < C) ? xb[(size_t)c * T] : 0.f;
            if (relu_in) v = v > 0.f ? v : 0.f;
            vals[i] = v;
        }
#pragma unroll
        for (int i = 0; i < MAXV; ++i) s += (wave + NW * i < C) ? vals[i] : 0.f;
    } else {
        for (int c = wave; c < C; c += NW) {
            float v = xb[(size_t)c * T];
            if (relu_in) v = v > 0.f ? v : 0.f;
            s += v;
        }
    }
    red[wave][lane] = s;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) tot += red[w][lane];
    const float mean = tot / (float)C;
    __syncthreads();
    float q = 0.f;
    if (in_regs) {
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const float d = vals[i] - mean;
            q += (wave + NW * i < C) ? d * d : 0.f;
        }
    } else {
        for (int c = wave; c < C; c += NW) {
            float v = xb[(size_t)c * T];
            if (relu_in) v = v > 0.f ? v : 0.f;
            const float d = v - mean;
            q += d * d;
        }
    }
    red[wave][lane] = q;
    __syncthreads();
    float qt = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) qt += red[w][lane];
    const float var = qt / (float)C;
    const float rstd = 1.0f / sqrtf(var + eps);
    if (ok) {
        float* yb = y + (size_t)b * C * T + t;
        if (in_regs) {
#pragma unroll
            for (int i = 0; i < MAXV; ++i) {
                const int c = wave + NW * i;
                if (c < C) yb[(size_t)c * T] = (vals[i] - mean) * rstd * gamma[c] + beta[c];
            }
        } else {
            for (int c = wave; c < C; c += NW) {
                float v = xb[(size_t)c * T];
                if (relu_in) v = v > 0.f ? v : 0.f;
                yb[(size_t)c * T] = (v - mean) * rstd * gamma[c] + beta[c];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Row softmax of attention scores with a key-padding mask (torch MHA math path, Q3):
// P[r, :] = softmax(S[r, :] + (-inf where key masked)).  One wave per row, wave-shuffle reductions.
// rows = B*H*T, row r belongs to batch r / (H*T).  key_valid (B,T) u8 1 = attend.
// ---------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void softmax_mask_kernel(float* __restrict__ s, const uint8_t* __restrict__ key_valid, int rows,
                                                           int T, int HT) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int b = row / HT;
    float* sr = s + (size_t)row * T;
    const uint8_t* kv = key_valid + (size_t)b * T;
    float mx = -INFINITY;
    for (int t = lane; t < T; t += 64) {
        const float v = kv[t] ? sr[t] : -INFINITY;
        mx = fmaxf(mx, v);
    }
    mx = wave_max(mx);
    float sum = 0.f;
    for (int t = lane; t < T; t += 64) {
        const float e = kv[t] ? expf(sr[t] - mx) : 0.f;
        sr[t] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    for (int t = lane; t < T; t += 64) sr[t] = sr[t] / sum;
}

// ---------------------------------------------------------------------------------------------
// Row sums of durations, shared by duration_kernel and dur_prefix_kernel: int64 sums, stored saturated at INT32_MAX (a single
// duration is capped at INT32_MAX first, so S of them cannot overflow int64).  A row longer than max_len keeps a length the
// host's checks see: the decode's L < max_len check then fails as pe[L] does in the reference (fft.py:18).
// ---------------------------------------------------------------------------------------------
static __device__ __forceinline__ int32_t sat_i32(int64_t v) { return (int32_t)min(v, (int64_t)INT32_MAX); }
// The 256 threads' partial sums -> each thread's exclusive prefix (returned); thread 0 stores the row total.  Two barriers.
static __device__ __forceinline__ int64_t row_prefix_256(int64_t local, int64_t* __restrict__ part, int32_t* __restrict__ row_total) {
    const int tid = threadIdx.x;
    part[tid] = local;
    __syncthreads();
    if (tid == 0) {
        int64_t run = 0;
        for (int i = 0; i < 256; ++i) {
            const int64_t v = part[i];
            part[i] = run;
            run += v;
        }
        *row_total = sat_i32(run);
    }
    __syncthreads();
    return part[tid];
}

// ---------------------------------------------------------------------------------------------
// Durations (parrot.py:82-86, duration.py:46-47): ld = masked_fill(ld, pad, 0);
// dur = max(rint(exp(ld) - 1), 0) as int64 (torch.round = round-half-even = rintf);
// one block per batch row also produces out_len[b] = sum(dur) and the inclusive prefix sums (row_prefix_256: saturated).
// A log-duration beyond ln(2^31) is one token longer than any max_len: the int32 sums this kernel once kept wrapped (three
// tokens of 2^32 + 512 j beside normal ones came out as a plausible short row).  dur itself saturates at INT64_MAX.
// err (nullable): a REAL token whose log-duration is NaN or +inf raises device status 5 (the reference fails there:
// "repeats can not be negative" / pe[T] out of range); at a padded position the value is masked to 0 first and changes nothing.
// ---------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void duration_kernel(const float* __restrict__ ld_raw, const uint8_t* __restrict__ src_valid,
                                                       float* __restrict__ log_dur, int64_t* __restrict__ dur,
                                                       int32_t* __restrict__ cum /* (B,S) inclusive */, int32_t* __restrict__ out_len,
                                                       int S, const int32_t* __restrict__ src_len = nullptr, int* __restrict__ err = nullptr) {
    __shared__ int64_t part[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int per = (S + 255) / 256;
    const int s_begin = min(S, tid * per), s_end = min(S, s_begin + per);
    int64_t local = 0;
    for (int s = s_begin; s < s_end; ++s) {
        // (row-exact: the row's own token count decides, not the key mask -- a row of NO tokens keeps key 0 attendable so that its
        //  softmax is defined, and must still expand to nothing)
        const bool real = src_len ? s < src_len[b] : src_valid[(size_t)b * S + s] != 0;
        float v = real ? ld_raw[(size_t)b * S + s] : 0.0f;
        log_dur[(size_t)b * S + s] = v;
        if (err && !(v < INFINITY)) atomicExch(err, 5);  // NaN or +inf (-inf is a duration of 0)
        float d = rintf(expf(v) - 1.0f);
        d = d > 0.f ? d : 0.f;
        const int64_t di = d < 9.2233720e18f ? (int64_t)d : INT64_MAX;
        dur[(size_t)b * S + s] = di;
        local += min(di, (int64_t)INT32_MAX);
    }
    int64_t run = row_prefix_256(local, part, out_len + b);
    for (int s = s_begin; s < s_end; ++s) {
        run += min(dur[(size_t)b * S + s], (int64_t)INT32_MAX);
        cum[(size_t)b * S + s] = sat_i32(run);
    }
}

// inclusive prefix sums + totals of given (B,S) durations: parrot_length_regulator (the standalone entry point) and teacher
// forcing (parrot_tte_set_durations: parrot.py:104, forward_duration(..., dur_target), duration.py:6-24).  Every position counts,
// padded ones included (repeat_interleave expands whatever it is given, duration.py:13-14); a negative duration counts as 0.
// Sums are int64, stored saturated at INT32_MAX (row_prefix_256): a row longer than max_len keeps its true length for the host's
// tgt_mask width check (duration.py:12).
// err (nullable): a negative duration raises device status 6 (torch: "repeats can not be negative"); with src_len (row-exact
// encode) a nonzero duration at s >= src_len[b] raises 7 (the row alone has no such token) and counts as 0.
static __global__ __launch_bounds__(256) void dur_prefix_kernel(const int64_t* __restrict__ dur, int32_t* __restrict__ cum, int32_t* __restrict__ out_len, int S,
                                                                int* __restrict__ err = nullptr, const int32_t* __restrict__ src_len = nullptr) {
    __shared__ int64_t part[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int per = (S + 255) / 256;
    const int s_begin = min(S, tid * per), s_end = min(S, s_begin + per);
    const int real = src_len ? src_len[b] : S;
    auto take = [&](int s) -> int64_t {
        const int64_t d = dur[(size_t)b * S + s];
        if (d < 0) {
            if (err) atomicExch(err, 6);
            return 0;
        }
        if (s >= real && d != 0) {
            if (err) atomicExch(err, 7);
            return 0;
        }
        return min(d, (int64_t)INT32_MAX);  // (S * 2^31 cannot overflow int64)
    };
    int64_t local = 0;
    for (int s = s_begin; s < s_end; ++s) local += take(s);
    int64_t run = row_prefix_256(local, part, out_len + b);
    for (int s = s_begin; s < s_end; ++s) {
        run += take(s);
        cum[(size_t)b * S + s] = sat_i32(run);
    }
}

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

constexpr int TIE_GUARD_MAX = 256;  // guarded positions per batch (argmax_cf_kernel / tie_guard_refine_kernel below)

// ---------------------------------------------------------------------------------------------
// Length regulator + positional row (duration.py:6-24, parrot.py:106, data.py:8-20):
// y[b, c, t] = (t < len_b ? enc[b, c, src(t)] : 0) + pe[L][c], src(t) = first s with cum[b,s] > t;
// tgt_mask[b,t] = t <= len_b (Q2).   grid (ceil(L/64), B).  idx is recomputed per (b,t) once and
// reused over channels.
// ---------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void length_regulate_kernel(const float* __restrict__ enc, const int32_t* __restrict__ cum,
                                                              const int32_t* __restrict__ out_len, const float* __restrict__ pe,
                                                              float* __restrict__ y, uint8_t* __restrict__ tgt_mask, int S, int L, int D,
                                                              int* __restrict__ gstat = nullptr, int gstat_reset = 1, int row_exact = 0, int pe_stride = -1) {
    const int b = blockIdx.y;
    const int wave = threadIdx.x >> 6;  // lane = frame, the four waves split the channels
    const int t = blockIdx.x * 64 + (threadIdx.x & 63);
    // (first kernel of a decode: restart the tie-guard statistics {count, ids changed, min margin bits = +inf, first list entry of
    //  this row group} of argmax_cf_kernel; a later row group of the same batch keeps them and notes where its entries start)
    if (gstat && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 4) {
        if (gstat_reset) gstat[threadIdx.x] = threadIdx.x == 2 ? 0x7f800000 : 0;
        else if (threadIdx.x == 3) gstat[3] = min(gstat[0], TIE_GUARD_MAX);
    }
    if (t >= L) return;
    const int len = out_len[b];
    // padded batch: pe[L] of the batch-max length and the `<=` mask (one extra frame per shorter row, quirk Q2); row-exact: what the
    // row's own B = 1 run sees -- pe[len] and exactly len frames (get_mask_from_lengths(len, max_len = len) is all True)
    const float* __restrict__ pe_row = pe + (size_t)(row_exact ? min(len, L) : L) * (pe_stride < 0 ? D : pe_stride);  // (pe_stride 0: one row for every length)
    // (row-exact rows of length 0 keep key 0 valid: a softmax over no keys at all is 0 / 0, and its NaN would raise the batch's
    //  non-finite flag for a row that emits nothing -- the host recomputes the returned mask from the lengths)
    // (tgt_mask NULL: the caller supplies the decoder's key mask -- parrot_tte_decode_masked, teacher forcing)
    if (wave == 0 && tgt_mask) tgt_mask[(size_t)b * L + t] = (row_exact ? t < max(len, 1) : t <= len) ? 1 : 0;
    int src = -1;
    if (t < len) {
        const int32_t* cb = cum + (size_t)b * S;
        int lo = 0, hi = S - 1;  // smallest s with cum[s] > t
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cb[mid] > t) hi = mid; else lo = mid + 1;
        }
        src = lo;
    }
    const float* eb = enc + (size_t)b * D * S;
    float* yb = y + (size_t)b * D * L + t;
    for (int c = wave; c < D; c += 4) {
        const float v = (src >= 0) ? eb[(size_t)c * S + src] : 0.0f;
        yb[(size_t)c * L] = pe_row[c] + v;
    }
}

// argmax over channels of (B, V, L) logits -> ids (B, L); first maximal index wins (torch.argmax).
// Tie guard (reference modules/parrot.py:115 takes the argmax of 1000 fp32 logits): every position also yields its top-2
// margin; positions whose margin is below `guard` are appended to `glist` ((b, t) pairs, at most TIE_GUARD_MAX) and counted in
// gstat[0], the smallest margin of the call lands in gstat[2] (float bits; positive floats order like ints) --
// tie_guard_refine_kernel then re-evaluates the head for exactly those positions in fp64.
constexpr int ARGMAX_WAVES = 16;  // waves per 64 positions: 62-63 codes each at V = 1000 (sixteen loads in flight per position)
static __global__ __launch_bounds__(64 * ARGMAX_WAVES) void argmax_cf_kernel(const float* __restrict__ logits, int64_t* __restrict__ ids, int V, int L,
                                                               int* __restrict__ err, float guard, int* __restrict__ glist,
                                                               int* __restrict__ gstat, int row0 = 0) {
    // lane = time step; the waves scan a slice of the vocabulary each, then the first maximum wins
    // (strict > inside a range, lower range first on ties: torch.argmax's first-occurrence rule)
    __shared__ float bv[ARGMAX_WAVES][64], sv[ARGMAX_WAVES][64];
    __shared__ int bix[ARGMAX_WAVES][64], bad[ARGMAX_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int t = blockIdx.x * 64 + lane;
    const bool ok = t < L;
    const int per = (V + ARGMAX_WAVES - 1) / ARGMAX_WAVES, v0 = wave * per, v1 = min(V, v0 + per);
    const float* lb = logits + (size_t)b * V * L + (ok ? t : 0);
    float best = -INFINITY, second = -INFINITY;  // second: the largest value of the range that is not `best`'s element
    int bi = v0 < V ? v0 : 0, nonfinite = 0;
    auto take = [&](float x, int v) {
        nonfinite |= !(fabsf(x) < INFINITY);  // NaN / inf anywhere in the column (a NaN never wins a `>` comparison)
        if (x > best) { second = best; best = x; bi = v; }
        else if (x > second) second = x;
    };
    if (v0 < V) {
        best = lb[(size_t)v0 * L];
        nonfinite |= !(fabsf(best) < INFINITY);
    }
    int v = v0 + 1;
    for (; v + 3 < v1; v += 4) {
        const float x0 = lb[(size_t)v * L], x1 = lb[(size_t)(v + 1) * L], x2 = lb[(size_t)(v + 2) * L], x3 = lb[(size_t)(v + 3) * L];
        take(x0, v); take(x1, v + 1); take(x2, v + 2); take(x3, v + 3);
    }
    for (; v < v1; ++v) take(lb[(size_t)v * L], v);
    bv[wave][lane] = best;
    sv[wave][lane] = second;
    bix[wave][lane] = bi;
    bad[wave][lane] = nonfinite;
    __syncthreads();
    if (wave == 0 && ok) {
        float m = bv[0][lane], s2 = sv[0][lane];
        int mi = bix[0][lane], nf = bad[0][lane];
#pragma unroll
        for (int w = 1; w < ARGMAX_WAVES; ++w) {
            const float bw = bv[w][lane];
            nf |= bad[w][lane];
            if (bw > m) { s2 = fmaxf(fmaxf(s2, m), sv[w][lane]); m = bw; mi = bix[w][lane]; }
            else s2 = fmaxf(s2, fmaxf(bw, sv[w][lane]));
        }
        ids[(size_t)b * L + t] = mi;
        if (err && nf) atomicExch(err, 5);  // NaN / inf logits (an activation left the fp16 split range)
        if (gstat) {
            const float margin = m - s2;  // >= 0, or NaN when the column holds non-finite logits (flagged above)
            // (sign bit cleared: -0.0 against +0.0 is a tie whose difference can come out as -0.0, which would order below every margin)
            if (margin >= 0.f) atomicMin(gstat + 2, __float_as_int(margin) & 0x7fffffff);
            if (!(margin >= guard) || nf) {  // (a NaN margin and a column with any non-finite logit are guarded too: one +inf gives margin +inf)
                const int slot = atomicAdd(gstat, 1);
                if (slot < TIE_GUARD_MAX) { glist[2 * slot] = row0 + b; glist[2 * slot + 1] = t; }  // (batch row; b is the row inside this group)
            }
        }
    }
}

// One workgroup per guarded position: logits[v] = head_b[v] + sum_c head_w[v][c] * x[b][c][t] in fp64 (exact products, fp64
// sums in channel order: the argmax no longer depends on the accumulation order of the fp32 head), first maximum wins.
// `hwt` is the head weight TRANSPOSED to (D, V): thread v reads hwt[c][v], coalesced across the workgroup.
// Deep form (f != NULL; round 4): the position's activation is first re-evaluated one layer earlier, from the last decoder block's
// own fp32 intermediates -- x[c] = h[c] + b2[c] + sum_j w2t[j][c] * f[j] in fp64 (f = relu(conv1) (B, F, L), h = x + attn (B, D, L),
// w2t the 1x1 conv2's weight as (F, D): reference modules/fft.py:81,99) -- which removes the fp32 accumulation error of that
// K = F sum and of the residual add from the refined logits.  `gref` (TIE_GUARD_MAX x V) receives the refined logits.
static __global__ __launch_bounds__(256) void tie_guard_refine_kernel(const float* __restrict__ x, const float* __restrict__ hwt,
                                                                      const float* __restrict__ hb, int64_t* __restrict__ ids, int D, int V,
                                                                      int L, const int* __restrict__ glist, int* __restrict__ gstat,
                                                                      const float* __restrict__ f, const float* __restrict__ h,
                                                                      const float* __restrict__ w2t, const float* __restrict__ b2, int F,
                                                                      float* __restrict__ gref, int row0 = 0) {
    // this row group's entries are [gstat[3], gstat[0]) of the lane's list; x / f / h / ids are the group's own buffers (row b - row0)
    const int n = min(gstat[0], TIE_GUARD_MAX), entry = gstat[3] + (int)blockIdx.x;
    if (entry >= n) return;
    extern __shared__ double xs[];  // D activations of the position (+ F intermediates in the deep form)
    __shared__ double rv[256];
    __shared__ int ri[256];
    const int b = glist[2 * entry] - row0, t = glist[2 * entry + 1];
    if (f) {
        double* fs = xs + D;
        for (int j = threadIdx.x; j < F; j += 256) fs[j] = (double)f[((size_t)b * F + j) * L + t];
        __syncthreads();
        for (int c = threadIdx.x; c < D; c += 256) {
            // (a thread walks F = 1024 weights with one dependent fp64 chain: what bounds it is the number of loads in flight, not
            //  the arithmetic -- 8 per thread took 96 us for a full list, one position per workgroup; 32 at a time keep the sum's order)
            double a = 0.0;
#pragma unroll 32
            for (int j = 0; j < F; ++j) a = fma((double)w2t[(size_t)j * D + c], fs[j], a);
            xs[c] = (a + (b2 ? (double)b2[c] : 0.0)) + (double)h[((size_t)b * D + c) * L + t];  // (conv + bias) + residual, fft.py:99
        }
    } else {
        for (int c = threadIdx.x; c < D; c += 256) xs[c] = (double)x[((size_t)b * D + c) * L + t];
    }
    __syncthreads();
    double best = -INFINITY;
    int bi = 0x7fffffff;
    for (int v0 = 0; v0 < V; v0 += 1024) {  // four codes per thread and pass: v0 + threadIdx.x + {0, 256, 512, 768}
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        int vv[4];
        bool ok[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            vv[q] = v0 + threadIdx.x + 256 * q;
            ok[q] = vv[q] < V;
            vv[q] = min(vv[q], V - 1);  // (unconditional loads: a predicated load per element would serialise them; the surplus is ignored below)
        }
#pragma unroll 8
        for (int c = 0; c < D; ++c) {
            const float* w = hwt + (size_t)c * V;
            const double xc = xs[c];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = fma((double)w[vv[q]], xc, acc[q]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double a = acc[q] + (hb ? (double)hb[vv[q]] : 0.0);
            if (ok[q] && gref) gref[(size_t)entry * V + vv[q]] = (float)a;
            if (ok[q] && a > best) { best = a; bi = vv[q]; }  // (codes ascending per thread: the first maximum is kept)
        }
    }
    rv[threadIdx.x] = best;
    ri[threadIdx.x] = bi;
    __syncthreads();
    for (int sft = 128; sft > 0; sft >>= 1) {
        if ((int)threadIdx.x < sft) {
            const double o = rv[threadIdx.x + sft];
            const int oi = ri[threadIdx.x + sft];
            if (o > rv[threadIdx.x] || (o == rv[threadIdx.x] && oi < ri[threadIdx.x])) { rv[threadIdx.x] = o; ri[threadIdx.x] = oi; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (ids[(size_t)b * L + t] != ri[0]) atomicAdd(gstat + 1, 1);  // positions whose id the refinement changed
        ids[(size_t)b * L + t] = ri[0];
    }
}

// (B, C, T) -> (B, T, C) transpose (tests / optional logits export)
static __global__ __launch_bounds__(256) void transpose_cf_to_cl_kernel(const float* __restrict__ x, float* __restrict__ y, int C, int T) {
    __shared__ float tile[64][65];
    const int t0 = blockIdx.x * 64, c0 = blockIdx.y * 64, b = blockIdx.z;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int r = ty; r < 64; r += 4) {
        const int c = c0 + r, t = t0 + tx;
        tile[r][tx] = (c < C && t < T) ? x[((size_t)b * C + c) * T + t] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int t = t0 + r, c = c0 + tx;
        if (t < T && c < C) y[((size_t)b * T + t) * C + c] = tile[tx][r];
    }
}


// the batched fp32 MFMA GEMM of the three-kernel attention path (operand addressing: attn.h)
struct BgemmParams {
    const float* A;
    const float* B;
    float* C;
    int M, N, K;
    long a_sk, a_sm, b_sk, b_sn;      // element strides
    long a_zb, a_zh, b_zb, b_zh;      // batch / head offsets
    long c_zb, c_zh, ldc;
    int H;
    float alpha;
};

static __global__ __launch_bounds__(256) void bgemm_mfma_kernel(const BgemmParams p) {
    constexpr int KC = 32, RS = 65;
    __shared__ float As[KC][RS];
    __shared__ float Bs[KC][RS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, half = lane >> 5, l31 = lane & 31;
    const int z = blockIdx.z, zb = z / p.H, zh = z - zb * p.H;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const float* __restrict__ A = p.A + zb * p.a_zb + zh * p.a_zh;
    const float* __restrict__ B = p.B + zb * p.b_zb + zh * p.b_zh;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    const bool a_kfast = (p.a_sk == 1), b_kfast = (p.b_sk == 1);
    for (int k0 = 0; k0 < p.K; k0 += KC) {
#pragma unroll
        for (int i = 0; i < (KC * 64) / 256; ++i) {
            const int idx = i * 256 + tid;
            int kk, mm;
            if (a_kfast) { mm = idx / KC; kk = idx % KC; } else { kk = idx / 64; mm = idx % 64; }
            float v = 0.f;
            if (k0 + kk < p.K && m0 + mm < p.M) v = A[(long)(k0 + kk) * p.a_sk + (long)(m0 + mm) * p.a_sm] * p.alpha;
            As[kk][mm] = v;
            int kb, nn;
            if (b_kfast) { nn = idx / KC; kb = idx % KC; } else { kb = idx / 64; nn = idx % 64; }
            float w = 0.f;
            if (k0 + kb < p.K && n0 + nn < p.N) w = B[(long)(k0 + kb) * p.b_sk + (long)(n0 + nn) * p.b_sn];
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
    float* __restrict__ C = p.C + zb * p.c_zb + zh * p.c_zh;
    const int n = n0 + wn * 32 + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (m < p.M && n < p.N) C[(long)m * p.ldc + n] = acc[r];
    }
}

}  // namespace parrot
