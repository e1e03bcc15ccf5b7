// kernels_conv.h -- the two kernels beside the conv plans (host_conv.hip): conv_post's tanh and the MFMA layout probe.
// Include it from ONE unit only (the one that launches these): a `static __global__` kernel is emitted by every unit that sees it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "conv_mfma.h"  // (f32x16)

namespace parrot {

// MFMA fragment-layout probe: D = A(32x2) * B(2x32) with A[i][k] = i + 100k, B[k][j] = (k ? 1000 : 1) * (j+1)
// dumps the 16 accumulator registers of every lane so the host can check the assumed C/D mapping.
static __global__ void mfma_probe_kernel(float* out) {
    const int lane = threadIdx.x;
    const int i = lane & 31, k = lane >> 5;
    const float a = (float)(i + 100 * k);
    const float b = (k ? 1000.f : 1.f) * (float)(i + 1);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) out[lane * 16 + r] = acc[r];
}

// ACT_TANH (conv_post only): applied right after the conv launch (apply_act, conv_mfma.h)
static __global__ void tanh_inplace_kernel(float* __restrict__ y, size_t n, int* __restrict__ err) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const float v = y[i];
        y[i] = tanhf(v);
        // NaN / inf reached the waveform (fp16 split range exceeded).  The PRE-activation is tested: tanhf(+-inf) = +-1 would pass
        if (err && !(fabsf(v) < INFINITY)) atomicExch(err, 5);
    }
}

}  // namespace parrot
