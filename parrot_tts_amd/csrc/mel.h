// mel.h -- the HBM-bound kernels of the vocoder's validation metric: the log-mel spectrogram of reference
// utils/vocoder/dataset.py:43-69 (reflect pad, framed DFT, magnitude, mel projection, log-clamp) and the L1 distance of two such
// spectrograms (utils/vocoder/train.py:213).  The two GEMMs -- the framed DFT as a Conv1d over a polyphase view of the padded
// signal, the mel projection as a 1x1 conv -- are parrot_conv plans (conv_split.h / conv_mfma.h); what is here only moves data.
// Include it from ONE unit only (the one that launches these), like kernels_misc.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace parrot {

constexpr int MEL_ST_NONFINITE = 5;  // device status values of a mel handle (5: as the vocoder / TTE handles use it)
constexpr int MEL_ST_SHORT_ROW = 8;  // a row no longer than the reflect pad (torch F.pad: "Padding size should be less than ...")

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

}  // namespace parrot
