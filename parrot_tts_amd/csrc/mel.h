// mel.h -- the HBM-bound kernels of the vocoder's validation metric: the log-mel spectrogram of reference
// utils/vocoder/dataset.py:43-69 (reflect pad, framed DFT, magnitude, mel projection, log-clamp) and the L1 distance of two such
// spectrograms (utils/vocoder/train.py:213).  The two GEMMs -- the framed DFT as a Conv1d over a polyphase view of the padded
// signal, the mel projection as a 1x1 conv -- are parrot_conv plans (conv_split.h / conv_mfma.h); what is here only moves data.
// Include it from ONE unit only (the one that launches these).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace parrot {

constexpr int MEL_ST_NONFINITE = 5;  // device status values of a mel handle (5: as the vocoder / TTE handles use it)
constexpr int MEL_ST_SHORT_ROW = 8;  // a row no longer than the reflect pad (torch F.pad: "Padding size should be less than ...")
constexpr int MEL_BWD_GROUPS = 8;    // channel groups of the transposed DFT (parrot_mel_l1_grad); mel_frame_adjoint_kernel adds the partial sums

// ---------------------------------------------------------------------------------------------
// Frame kernel: reflect padding + polyphase transpose, wav (B, N) -> x (B, hop, Tc), Tc = N / hop + k - 1:
//   x[b][c][j] = padded_b[j * hop + c],  padded_b = reflect-pad of wav[b, :n_b] by pad_r = (n_fft - hop) / 2 on both sides
// (dataset.py:55), so that frame t of the STFT (center = False) is columns t .. t + k - 1: a Conv1d with hop input channels
// and k = ceil(n_fft / hop) taps.  The view is a transpose of the padded signal read as (Tc, hop): a 64 x 64 tile through LDS,
// so that the reads (contiguous in c; backwards inside the reflected ends) and the writes (contiguous in j) both coalesce.
// n_samples (nullable): row b holds n_b = n_samples[b] real samples (clamped to [0, N]); the reflection happens at the row's OWN
// end, the row yields n_b / hop frames and every column beyond the n_b / hop + k - 1 those frames read is zero -- the tail of the
// padded row is never read -- so a row of a padded batch equals that utterance run alone.  A row with n_b <= pad_r raises
// MEL_ST_SHORT_ROW and is written as zeros.  grid (ceil(Tc / 64), ceil(hop / 64), B).
// ---------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void mel_frame_kernel(const float* __restrict__ wav, long row_stride, const int32_t* __restrict__ n_samples,
                                                               int N, int hop, int k, int pad_r, int Tc, float* __restrict__ x,
                                                               int* __restrict__ err) {
    __shared__ float tile[64][65];
    const int j0 = blockIdx.x * 64, c0 = blockIdx.y * 64, b = blockIdx.z;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;  // 4 rows of 64
    const int n_b = n_samples ? min(max(n_samples[b], 0), N) : N;
    const bool too_short = n_b <= pad_r;
    if (too_short && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) atomicExch(err, MEL_ST_SHORT_ROW);
    const int frames = n_b / hop;
    const int cols = (too_short || frames == 0) ? 0 : frames + k - 1;
    const long plen = (long)n_b + 2 * pad_r;
    const float* __restrict__ wb = wav + (size_t)b * row_stride;
    for (int r = ty; r < 64; r += 4) {  // rows = column j of the view, cols = channel c: contiguous in the signal
        const int j = j0 + r, c = c0 + tx;
        float v = 0.f;
        if (j < cols && c < hop) {
            const long p = (long)j * hop + c;
            if (p < plen) {
                long i = p - pad_r;
                if (i < 0) i = -i;                                  // (pad_r < n_b: both reflections land inside the row)
                else if (i >= n_b) i = 2 * ((long)n_b - 1) - i;
                v = wb[i];
            }
        }
        tile[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int c = c0 + r, j = j0 + tx;
        if (c < hop && j < Tc) x[((size_t)b * hop + c) * Tc + j] = tile[tx][r];
    }
}

// ---------------------------------------------------------------------------------------------
// Magnitude kernel: spec (B, G Mg, T) -> (B, Fp, T), sqrt(re^2 + im^2 + 1e-9) in the reference's order of roundings
// (dataset.py:63: pow, pow, add, add, sqrt -- no contraction).  Group g of the spec holds the partial DFT sums over the g-th G-th
// of the input channels in its rows [g Mg, g Mg + F) (real parts) and [g Mg + F, g Mg + 2F) (imaginary parts); the partials are
// added in group order.  G = 1, Mg = 2F: the plain (B, 2F, T) spec of the split schemes; G > 1: the exact-fp32 handle, whose
// conv would otherwise round n_fft times along one accumulator chain (parrot_mel_create).  The pad channels F .. Fp - 1 (Fp = F
// rounded up to the mel conv's 16-channel chunks) are written as zero.  V consecutive frames per thread (V = 4: 16-byte loads
// and stores, for T % 4 = 0 and 16-byte aligned buffers; V = 1 otherwise), consecutive threads along t.
// ---------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(256) void mel_magnitude_kernel(const float* __restrict__ spec, float* __restrict__ mag, int F, int Fp, int T,
                                                            int G, int Mg, size_t groups) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= groups) return;
    const int Tg = T / V;
    const int t = (int)(g % Tg) * V;
    const int f = (int)((g / Tg) % Fp);
    const size_t b = g / ((size_t)Tg * Fp);
    float re[V], im[V], v[V];
    if (f < F) {
#pragma unroll
        for (int q = 0; q < V; ++q) re[q] = im[q] = 0.f;
        for (int gi = 0; gi < G; ++gi) {  // (0 + x = x: one group is the plain sum)
            const float* __restrict__ pr = spec + ((b * G + gi) * Mg + f) * T + t;
            const float* __restrict__ pi = pr + (size_t)F * T;
            if constexpr (V == 4) {
                const float4 r4 = *reinterpret_cast<const float4*>(pr), i4 = *reinterpret_cast<const float4*>(pi);
                re[0] = __fadd_rn(re[0], r4.x); re[1] = __fadd_rn(re[1], r4.y); re[2] = __fadd_rn(re[2], r4.z); re[3] = __fadd_rn(re[3], r4.w);
                im[0] = __fadd_rn(im[0], i4.x); im[1] = __fadd_rn(im[1], i4.y); im[2] = __fadd_rn(im[2], i4.z); im[3] = __fadd_rn(im[3], i4.w);
            } else {
                re[0] = __fadd_rn(re[0], pr[0]);
                im[0] = __fadd_rn(im[0], pi[0]);
            }
        }
#pragma unroll
        for (int q = 0; q < V; ++q) v[q] = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(re[q], re[q]), __fmul_rn(im[q], im[q])), 1e-9f));
    } else {
#pragma unroll
        for (int q = 0; q < V; ++q) v[q] = 0.f;
    }
    float* __restrict__ po = mag + (b * Fp + f) * T + t;
    if constexpr (V == 4) *reinterpret_cast<float4*>(po) = make_float4(v[0], v[1], v[2], v[3]);
    else po[0] = v[0];
}

// ---------------------------------------------------------------------------------------------
// Log-clamp kernel, in place on the mel conv's output (B, n_mels, T): log(clamp(x, min = 1e-5)) (dataset.py:85-86).  A NaN
// passes through the clamp as torch's does; a non-finite mel of a real frame raises MEL_ST_NONFINITE.  With n_samples, frames
// t >= n_samples[b] / hop of row b are written as zero and not examined.
// ---------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void mel_log_kernel(float* __restrict__ mel, const int32_t* __restrict__ n_samples, int N, int hop,
                                                             int n_mels, int T, size_t total, int* __restrict__ err) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int t = (int)(i % T);
    const size_t b = i / ((size_t)T * n_mels);
    const int frames = n_samples ? min(max(n_samples[b], 0), N) / hop : T;
    float out = 0.f;
    if (t < frames) {
        const float v = mel[i];
        if (!(fabsf(v) < INFINITY)) atomicExch(err, MEL_ST_NONFINITE);
        out = logf(v < 1e-5f ? 1e-5f : v);
    }
    mel[i] = out;
}

// ---------------------------------------------------------------------------------------------
// L1 kernel pair (patterned on loss_rows_kernel / loss_reduce_kernel): per row b, sum |a - b| over n_mels x n_frames[b] elements
// of two (B, n_mels, T) tensors.  Stage 1: block (x, b) owns [x * MEL_L1_CHUNK, + MEL_L1_CHUNK) of the row's n_mels * n_frames[b]
// REAL elements, counted bin-major without the padding frames -- so a row's sum does not depend on the T it is padded to;
// each thread adds its fixed strided slice in fp64 (the difference of two floats is exact in fp64), then a fixed LDS tree.
// Stage 2 (one block): thread r adds the partials of rows r, r + 256, ... in block order; the batch sums by a fixed tree.  No
// atomics on values: two calls agree bit for bit.
// out (2B doubles) <- row sums, then row counts n_mels * n_frames[b]; mean (nullable, 1 float) <- sum of sums / sum of counts
// (F.l1_loss's mean for equal-length rows; 0 / 0 = NaN for an empty batch).
// ---------------------------------------------------------------------------------------------
constexpr int MEL_L1_CHUNK = 4096;  // elements per stage-1 block: 16 per thread

static __global__ __launch_bounds__(256) void mel_l1_rows_kernel(const float* __restrict__ a, const float* __restrict__ bb, const int32_t* __restrict__ n_frames,
                                                                 int n_mels, int T, double* __restrict__ part) {
    __shared__ double red[256];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int nf = n_frames ? min(max(n_frames[b], 0), T) : T;
    const long row = (long)n_mels * T, real = (long)n_mels * nf;
    const float* __restrict__ ar = a + (size_t)b * row;
    const float* __restrict__ br = bb + (size_t)b * row;
    double s = 0.0;
    const long i0 = (long)blockIdx.x * MEL_L1_CHUNK;
#pragma unroll 4
    for (int q = 0; q < MEL_L1_CHUNK / 256; ++q) {
        const long i = i0 + q * 256 + tid;  // position among the row's REAL elements: (mel bin i / nf, frame i % nf)
        if (i < real) {
            const long at = i / nf * T + i % nf;
            s += fabs((double)ar[at] - (double)br[at]);
        }
    }
    red[tid] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    if (tid == 0) part[(size_t)b * gridDim.x + blockIdx.x] = red[0];
}

static __global__ __launch_bounds__(256) void mel_l1_reduce_kernel(const double* __restrict__ part, int nblk, const int32_t* __restrict__ n_frames, int B,
                                                                   int n_mels, int T, double* __restrict__ out, float* __restrict__ mean) {
    __shared__ double s_sum[256], s_cnt[256];
    const int tid = threadIdx.x;
    double tot = 0.0, cnt = 0.0;
    for (int b = tid; b < B; b += 256) {
        double s = 0.0;
        for (int x = 0; x < nblk; ++x) s += part[(size_t)b * nblk + x];
        const int nf = n_frames ? min(max(n_frames[b], 0), T) : T;
        const double c = (double)n_mels * (double)nf;
        out[b] = s;
        out[B + b] = c;
        tot += s;
        cnt += c;
    }
    s_sum[tid] = tot;
    s_cnt[tid] = cnt;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) {
            s_sum[tid] += s_sum[tid + h];
            s_cnt[tid] += s_cnt[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0 && mean) mean[0] = (float)(s_sum[0] / s_cnt[0]);
}

// ---------------------------------------------------------------------------------------------
// The gradient of the mel L1 with respect to the waveform (parrot_mel_l1_grad; train.py:157 and loss_gen_all.backward()): the
// forward above with the log-clamp out of place, the L1 pair, then five stages backwards.  The two transposed GEMMs are conv plans
// (host_mel.hip); what is here moves data.  All operands are of unit weight: scale / count enters once, in the last kernel.
// Every kernel writes each element of its output exactly once; nothing is accumulated atomically.
// ---------------------------------------------------------------------------------------------

// mel_log_kernel out of place: the gradient needs the pre-log mel, so `mel` stays and the log-clamp goes to `logmel` -- the same
// expression, so the loss equals the forward's bit for bit.
static __global__ __launch_bounds__(256) void mel_log_keep_kernel(const float* __restrict__ mel, float* __restrict__ logmel, const int32_t* __restrict__ n_samples,
                                                                  int N, int hop, int n_mels, int T, size_t total, int* __restrict__ err) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int t = (int)(i % T);
    const size_t b = i / ((size_t)T * n_mels);
    const int frames = n_samples ? min(max(n_samples[b], 0), N) / hop : T;
    float out = 0.f;
    if (t < frames) {
        const float v = mel[i];
        if (!(fabsf(v) < INFINITY)) atomicExch(err, MEL_ST_NONFINITE);
        out = logf(v < 1e-5f ? 1e-5f : v);
    }
    logmel[i] = out;
}

// n_frames[b] = n_samples[b] / hop (clamped as everywhere) for the L1 pair
static __global__ void mel_frames_kernel(const int32_t* __restrict__ n_samples, int N, int hop, int B, int32_t* __restrict__ n_frames) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) n_frames[b] = min(max(n_samples[b], 0), N) / hop;
}

// After the L1 pair (one block): factor <- what the last kernel multiplies by -- scale / (sum of the row counts) for the mean,
// scale for the sum -- and, for the sum, loss_sum <- the row sums added in row order.  The counts are integers: their fp64 sum is
// exact in any order.
static __global__ __launch_bounds__(256) void mel_l1_scale_kernel(const double* __restrict__ out, int B, int mean, double scale, float* __restrict__ factor,
                                                                  double* __restrict__ loss_sum) {
    __shared__ double s_cnt[256];
    const int tid = threadIdx.x;
    double cnt = 0.0;
    for (int b = tid; b < B; b += 256) cnt += out[B + b];
    s_cnt[tid] = cnt;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) s_cnt[tid] += s_cnt[tid + h];
        __syncthreads();
    }
    if (tid == 0) {
        factor[0] = (float)(mean ? scale / s_cnt[0] : scale);
        if (loss_sum) {
            double s = 0.0;
            for (int b = 0; b < B; ++b) s += out[b];
            loss_sum[0] = s;
        }
    }
}

// Stage 1, the head: g_mel (B, Mp, T) = sgn(logmel - target) [mel >= 1e-5] / mel -- d|x| = sgn(x), 0 at 0; the clamp passes the
// gradient where it did not act; d log = 1 / mel, from the PRE-log value the forward kept -- and 0 for the frames beyond
// n_samples[b] / hop and for the pad channels n_mels .. Mp - 1 (Mp: n_mels rounded up to the conv's 16-channel chunks).
static __global__ __launch_bounds__(256) void mel_l1_head_kernel(const float* __restrict__ mel, const float* __restrict__ logmel, const float* __restrict__ target,
                                                                 const int32_t* __restrict__ n_samples, int N, int hop, int n_mels, int Mp, int T,
                                                                 size_t total, float* __restrict__ g_mel) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int t = (int)(i % T);
    const int o = (int)((i / T) % Mp);
    const size_t b = i / ((size_t)T * Mp);
    const int frames = n_samples ? min(max(n_samples[b], 0), N) / hop : T;
    float g = 0.f;
    if (o < n_mels && t < frames) {
        const size_t at = (b * n_mels + o) * T + t;
        const float d = logmel[at] - target[at], v = mel[at];
        const float s = d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f;
        if (v >= 1e-5f) g = s / v;
    }
    g_mel[i] = g;
}

// Stage 3, the magnitude backwards: g_spec (B, C2p, T), rows [0, F) = g_mag re / mag, rows [F, 2F) = g_mag im / mag, the pad rows
// 2F .. C2p - 1 zero.  re / im: the G group partials the forward left in `spec`, added in group order as mel_magnitude_kernel
// does (every partial has the gradient of the sum); mag: the forward's, >= sqrt(1e-9), so re = im = 0 gives 0 and not 0 / 0.
static __global__ __launch_bounds__(256) void mel_magnitude_bwd_kernel(const float* __restrict__ spec, const float* __restrict__ mag, const float* __restrict__ g_mag,
                                                                       int F, int Fp, int C2p, int T, int G, int Mg, size_t total,
                                                                       float* __restrict__ g_spec) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int t = (int)(i % T);
    const int r = (int)((i / T) % C2p);
    const size_t b = i / ((size_t)T * C2p);
    float v = 0.f;
    if (r < 2 * F) {
        float x = 0.f;
        for (int gi = 0; gi < G; ++gi) x = __fadd_rn(x, spec[((b * G + gi) * Mg + r) * T + t]);
        const size_t at = (b * Fp + (r < F ? r : r - F)) * T + t;
        v = __fmul_rn(__fdiv_rn(g_mag[at], mag[at]), x);
    }
    g_spec[i] = v;
}

// Stage 5, the adjoint of mel_frame_kernel: g_poly (B, hop, Tc) -> grad (B, N), un-polyphase + reflect adjoint in GATHER form.
// g_poly arrives as the G group partials of the transposed DFT, (B, G Mg, Tc) with channel c of group g in row g Mg + c: every
// read adds them in group order.
// Sample i < n_b of row b was read at up to three padded positions p = j hop + c: its own, i + pad_r; the left mirror pad_r - i
// (1 <= i <= pad_r); the right mirror about n_b - 1, 2 (n_b - 1) - i + pad_r (n_b - 1 - pad_r <= i <= n_b - 2).  They are added
// in that order, multiplied by factor[0] and written; positions no frame reads (p >= (frames - 1) hop + n_fft, or beyond the
// padded row) give nothing, samples at and beyond n_b are written as zero.  The view is transposed through a 64 x 64 LDS tile as
// in the forward: the reads of the own position run along j, the writes along i.  The mirrors -- at most 2 pad_r samples of a
// row -- are read from g_poly directly.  grid (ceil(((N + pad_r - 1) / hop + 1) / 64), ceil(hop / 64), B): every i in [0, N)
// is some block's p - pad_r exactly once.  A non-finite gradient raises MEL_ST_NONFINITE.
static __global__ __launch_bounds__(256) void mel_frame_adjoint_kernel(const float* __restrict__ g_poly, const int32_t* __restrict__ n_samples, int N, int hop,
                                                                       int k, int n_fft, int pad_r, int Tc, int G, int Mg,
                                                                       const float* __restrict__ factor, float* __restrict__ grad,
                                                                       int* __restrict__ err) {
    __shared__ float tile[64][65];
    const int j0 = blockIdx.x * 64, c0 = blockIdx.y * 64, b = blockIdx.z;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int n_b = n_samples ? min(max(n_samples[b], 0), N) : N;
    const int frames = n_b / hop;
    // padded positions some frame of the row reads: [0, plim)
    const long plim = (n_b <= pad_r || frames == 0) ? 0 : min((long)n_b + 2 * pad_r, (long)(frames - 1) * hop + n_fft);
    const float* __restrict__ gp = g_poly + (size_t)b * G * Mg * Tc;
    auto at = [&](int c, long j) {  // the G partials of g_poly[c][j], in group order
        float s = 0.f;
        for (int g = 0; g < G; ++g) s = __fadd_rn(s, gp[((size_t)g * Mg + c) * Tc + j]);
        return s;
    };
    for (int r = ty; r < 64; r += 4) {  // rows = channel c, cols = column j: contiguous in g_poly
        const int c = c0 + r, j = j0 + tx;
        tile[r][tx] = (c < hop && j < Tc) ? at(c, j) : 0.f;
    }
    __syncthreads();
    const float f = factor[0];
    for (int r = ty; r < 64; r += 4) {
        const int j = j0 + r, c = c0 + tx;
        const long p = (long)j * hop + c, i = p - pad_r;
        if (c >= hop || i < 0 || i >= N) continue;
        float v = 0.f;
        if (i < n_b && plim > 0) {
            if (p < plim) v = tile[tx][r];
            if (i >= 1 && i <= pad_r) {
                const long q = pad_r - i;
                if (q < plim) v = __fadd_rn(v, at((int)(q % hop), q / hop));
            }
            if (i <= (long)n_b - 2 && i >= (long)n_b - 1 - pad_r) {
                const long q = 2 * ((long)n_b - 1) - i + pad_r;
                if (q < plim) v = __fadd_rn(v, at((int)(q % hop), q / hop));
            }
            v = __fmul_rn(v, f);
            if (!(fabsf(v) < INFINITY)) atomicExch(err, MEL_ST_NONFINITE);
        }
        grad[(size_t)b * N + i] = v;
    }
}

}  // namespace parrot
