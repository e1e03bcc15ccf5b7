// voc_train.h -- the kernels that TRAIN the vocoder's generator (reference utils/vocoder/models.py:69-169 with weight norm attached,
// and the backward of that graph): parrot_voc_train_forward / _backward (host_voc_train.hip).  Activations are channel-first,
// (B, C, T), as torch holds them.  The matrix products are not here: every Conv1d, every phase of a ConvTranspose1d, their data
// gradients and their weight gradients go through train_gemm.h, with the leaky ReLU's backward, the residual add and the activation
// of the next conv in tap_gemm_kernel's epilogue.  This file holds what lies between them:
//   vt_wn_fwd_kernel     weight norm, old style, dim 0: w = v (g / ||v||), the norm per row over everything else (fp64, fixed order)
//   vt_wn_bwd_kernel     dg = s / ||v||, dv = (g / ||v||) dw - (g s / ||v||^3) v with s = sum dw v (fp64, fixed order)
//   vt_embed_kernel      x (B, E (1 + multispkr), U) = dict[code] transposed, spkr[spkr] broadcast over the frames below it
//   vt_lrelu_kernel      a = x > 0 ? x : x slope;  vt_mask_kernel: a > 0 as bytes (the predicate the backward applies)
//   vt_mrf_kernel        ((r0 + r1) + r2 ...) / n_kernels, a true division;  vt_div_kernel its backward
//   vt_tanh_kernel, vt_tanh_bwd_kernel (from the saved output), vt_add_kernel
//   vt_chansum_kernel    bias gradients: out[c] = sum over (b, t), ascending per thread then a fixed tree, fp64
// Rules, as in train_gemm.h: no floating-point atomics; every sum that ends in one number is fp64 in a fixed order; nothing clamps
// with fmaxf, so a NaN stays a NaN.  The launchers are defined in tu_voc_train.hip, which alone sees the kernel bodies.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wave_reduce.h"

namespace parrot {

constexpr int VT_MAX_KERNELS = 4;  // PARROT_MAX_KERNELS

hipError_t vt_launch_wn_fwd(const float* v, const float* g, float* w, float* norm, int rows, int len, hipStream_t s);
// dv, dg: nullable
hipError_t vt_launch_wn_bwd(const float* dw, const float* v, const float* g, const float* norm, float* dv, float* dg, int rows, int len, hipStream_t s);
// an id outside its table gives NaN (nothing is indexed through it)
hipError_t vt_launch_embed(const int64_t* code, const int64_t* spkr, const float* dict, const float* spk_tab, float* x, int B, int U, int E, int n_emb,
                           int n_spkr, int multispkr, hipStream_t s);
hipError_t vt_launch_lrelu(const float* x, float* a, float slope, size_t n, hipStream_t s);
hipError_t vt_launch_mask(const float* a, uint8_t* out, size_t n, hipStream_t s);
// out = ((r[0] + r[1]) + ...) / nk, r[j] = r0 + j stride
hipError_t vt_launch_mrf(const float* r0, size_t stride, int nk, float* out, size_t n, hipStream_t s);
hipError_t vt_launch_div(const float* g, int nk, float* out, size_t n, hipStream_t s);
hipError_t vt_launch_add(const float* a, const float* b, float* y, size_t n, hipStream_t s);
hipError_t vt_launch_tanh(const float* z, float* y, float* keep, size_t n, hipStream_t s);
hipError_t vt_launch_tanh_bwd(const float* y, const float* dy, float* dz, size_t n, hipStream_t s);  // dz = dy (1 - y^2)
hipError_t vt_launch_chansum(const float* g, float* out, int B, int C, int T, hipStream_t s);

#ifdef PARROT_VOC_TRAIN_TU

// One workgroup per row.  ||v|| = sqrt(sum v^2): thread tid adds elements tid, tid + 256, ... in fp64, then the fixed tree; rounded to
// fp32 once and kept for the backward.  w = v (g / ||v||), the quotient formed once in fp32 (torch._weight_norm's own order).  A zero
// row divides by zero as torch does: nothing is clamped.
__global__ __launch_bounds__(256) void vt_wn_fwd_kernel(const float* __restrict__ v, const float* __restrict__ g, float* __restrict__ w,
                                                        float* __restrict__ norm, int len) {
    __shared__ double sm[256];
    const int row = blockIdx.x, tid = threadIdx.x;
    const float* vr = v + (size_t)row * len;
    double s = 0.0;
    for (int i = tid; i < len; i += 256) s += (double)vr[i] * (double)vr[i];
    const float nf = (float)sqrt(block_sum(s, sm));
    if (tid == 0) norm[row] = nf;
    const float ratio = g[row] / nf;
    float* wr = w + (size_t)row * len;
    for (int i = tid; i < len; i += 256) wr[i] = vr[i] * ratio;
}

__global__ __launch_bounds__(256) void vt_wn_bwd_kernel(const float* __restrict__ dw, const float* __restrict__ v, const float* __restrict__ g,
                                                        const float* __restrict__ norm, float* __restrict__ dv, float* __restrict__ dg, int len) {
    __shared__ double sm[256];
    const int row = blockIdx.x, tid = threadIdx.x;
    const float* vr = v + (size_t)row * len;
    const float* dr = dw + (size_t)row * len;
    double s = 0.0;
    for (int i = tid; i < len; i += 256) s += (double)dr[i] * (double)vr[i];
    s = block_sum(s, sm);
    const double n = (double)norm[row], gg = (double)g[row];
    if (dg && tid == 0) dg[row] = (float)(s / n);
    if (dv) {
        const double ratio = (double)(g[row] / norm[row]), c = gg * s / (n * n * n);
        float* o = dv + (size_t)row * len;
        for (int i = tid; i < len; i += 256) o[i] = (float)(ratio * (double)dr[i] - c * (double)vr[i]);
    }
}

__global__ __launch_bounds__(256) void vt_embed_kernel(const int64_t* __restrict__ code, const int64_t* __restrict__ spkr, const float* __restrict__ dict,
                                                       const float* __restrict__ spk_tab, float* __restrict__ x, int U, int E, int Cin, int n_emb,
                                                       int n_spkr, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int u = (int)(i % U), c = (int)(i / U % Cin);
    const size_t b = i / ((size_t)U * Cin);
    if (c < E) {
        const int64_t id = code[b * U + u];
        x[i] = (id >= 0 && id < n_emb) ? dict[id * E + c] : NAN;
    } else {
        const int64_t id = spkr[b];
        x[i] = (id >= 0 && id < n_spkr) ? spk_tab[id * E + (c - E)] : NAN;
    }
}
__global__ __launch_bounds__(256) void vt_lrelu_kernel(const float* __restrict__ x, float* __restrict__ a, float slope, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const float v = x[i];
        a[i] = v > 0.f ? v : v * slope;
    }
}
__global__ __launch_bounds__(256) void vt_mask_kernel(const float* __restrict__ a, uint8_t* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = a[i] > 0.f ? 1 : 0;
}
__global__ __launch_bounds__(256) void vt_mrf_kernel(const float* __restrict__ r0, size_t stride, int nk, float* out, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v = r0[i];
    for (int j = 1; j < nk; ++j) v += r0[(size_t)j * stride + i];
    out[i] = v / (float)nk;
}
__global__ __launch_bounds__(256) void vt_div_kernel(const float* g, float nk, float* out, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = g[i] / nk;
}
__global__ __launch_bounds__(256) void vt_add_kernel(const float* a, const float* b, float* y, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = a[i] + b[i];
}
__global__ __launch_bounds__(256) void vt_tanh_kernel(const float* __restrict__ z, float* __restrict__ y, float* __restrict__ keep, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const float v = tanhf(z[i]);
        y[i] = v;
        if (keep) keep[i] = v;
    }
}
__global__ __launch_bounds__(256) void vt_tanh_bwd_kernel(const float* __restrict__ y, const float* __restrict__ dy, float* __restrict__ dz, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const float v = y[i];
        dz[i] = dy[i] * (1.f - v * v);
    }
}
// One workgroup per channel c over its n = B T values: thread tid adds elements tid, tid + 256, ... (element i = b T + t) in fp64,
// then the fixed tree.
__global__ __launch_bounds__(256) void vt_chansum_kernel(const float* __restrict__ g, float* __restrict__ out, int B, int C, int T) {
    __shared__ double sm[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    const long n = (long)B * T;
    double s = 0.0;
    for (long i = tid; i < n; i += 256) {
        const long b = i / T, t = i - b * T;
        s += (double)g[((size_t)b * C + c) * T + t];
    }
    s = block_sum(s, sm);
    if (tid == 0) out[c] = (float)s;
}

#endif  // PARROT_VOC_TRAIN_TU

}  // namespace parrot
