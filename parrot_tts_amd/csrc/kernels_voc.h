// kernels_voc.h -- the glue kernels of the vocoder handle (host_voc.hip): the input gather, chunk lengths, int16 output, the range probe.
// Include it from ONE unit only (the one that launches these): a `static __global__` kernel is emitted by every unit that sees it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace parrot {

// ---------------------------------------------------------------------------------------------
// vocoder input: x[b, c, t] = c < E ? dict[code[b,t]][c] : spkr[spkr_id[b]][c - E]
// (utils/vocoder/models.py:155-160 + _upsample :132-151: the speaker vector is repeated over time)
// grid (ceil(U/64), C/?, B): each block = 64 time steps x 64 channels via an LDS transpose so that
// both the embedding-row reads (contiguous in c) and the (B,C,U) writes (contiguous in t) coalesce.
// ---------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void voc_embed_kernel(const int64_t* __restrict__ code, const int64_t* __restrict__ spkr,
                                                        const float* __restrict__ dict, const float* __restrict__ spk_tab,
                                                        float* __restrict__ x, int U, int E, int C, int Cx, int n_emb, int n_spk,
                                                        int* __restrict__ err, int code_stride) {  // C embedding channels of the Cx input channels; code rows code_stride apart
    __shared__ float tile[64][65];
    const int t0 = blockIdx.x * 64, c0 = blockIdx.y * 64, b = blockIdx.z;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;  // 4 rows of 64
    // load: rows = time, cols = channel (contiguous reads along the embedding row)
    for (int r = ty; r < 64; r += 4) {
        const int t = t0 + r, c = c0 + tx;
        float v = 0.f;
        if (t < U && c < C) {
            if (c < E) {
                int64_t id = code[(size_t)b * code_stride + t];
                if (id < 0 || id >= n_emb) { atomicExch(err, 1); id = 0; }
                v = dict[(size_t)id * E + c];
            } else {
                int64_t s = spkr[b];
                if (s < 0 || s >= n_spk) { atomicExch(err, 2); s = 0; }
                v = spk_tab[(size_t)s * E + (c - E)];
            }
        }
        tile[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int c = c0 + r, t = t0 + tx;
        if (c < C && t < U) x[((size_t)b * Cx + c) * U + t] = tile[tx][r];
    }
}

// per-row unit counts re-based to a chunk [lo, lo + n): clamp(len - lo, 0, n)   (parrot_voc_forward_chunked)
static __global__ void rebase_lens_kernel(const int32_t* __restrict__ lens, int32_t* __restrict__ out, int B, int lo, int n) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) out[b] = min(max(lens[b] - lo, 0), n);
}

// wav fp32 -> int16 exactly like numpy's `(x * 32768).astype('int16')` for in-range values
// (C cast: truncation toward zero; utils/vocoder/inference.py:71-73).
static __global__ void wav_to_int16_kernel(const float* __restrict__ w, int16_t* __restrict__ o, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) o[i] = (int16_t)(int32_t)(w[i] * 32768.0f);
}

// max |x[i]| -> atomic max into dst[0] (non-negative floats order like their bit patterns); NaN / inf count as +inf
static __global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ x, size_t n, float* __restrict__ dst) {
    float m = 0.f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float v = fabsf(x[i]);
        m = (v > m || !(v == v)) ? (v == v ? v : INFINITY) : m;
    }
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0) atomicMax(reinterpret_cast<int*>(dst), __float_as_int(m));
}

}  // namespace parrot
