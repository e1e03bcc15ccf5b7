// optim.h -- AdamW (torch.optim.AdamW, decoupled weight decay, no amsgrad) over a whole parameter group in one launch: the two
// optimiser steps of the vocoder's trainer (reference utils/vocoder/train.py:80-82, 151, 168).
//
// A tensor is (p, g, m, v, n, step) over dense fp32 arrays.  The work is cut into chunks of ADAMW_CHUNK elements; a chunk belongs
// to one tensor and a tensor's chunks start at its element 0.  The tensor table, the two per-tensor scalars and the per-tensor
// chunk prefix travel BY VALUE in the kernel arguments (AdamwLaunch, under the 4 KB limit): the entry point allocates nothing and
// copies nothing.  A workgroup is one chunk and finds its tensor by bisecting the prefix.
//
// The update of one element, every line one correctly rounded fp32 operation, nothing contracted (tests/adamw_ref.py states the
// same lines in numpy float32):
//     p <- p * decay
//     m <- m + (g - m) * w1
//     v <- v * b2 + (g * w2) * g
//     d <- sqrt(v) / rs + e
//     p <- p + ns * (m / d)
// decay = 1 - lr wd, w1 = 1 - beta1, b2 = beta2, w2 = 1 - beta2, e = eps, and per tensor ns = -lr / (1 - beta1^step),
// rs = sqrt(1 - beta2^step): formed on the host in double and rounded to fp32 once (host_optim.hip).
// Inside a chunk, thread t owns the quads 4 (t + 256 i) .. + 3, i = 0 .. 3: 16-byte loads and stores when all four bases are
// 16-byte aligned (a chunk starts at a multiple of 4 elements, so the bases decide), scalar ones otherwise and in the quad that
// crosses n.  An element's result does not depend on the path.  g is read only; nothing outside [0, n) is touched.
// The launcher is defined in tu_optim.hip, which alone sees the kernel body (PARROT_OPTIM_TU).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/parrot_hip.h"

namespace parrot {

constexpr int ADAMW_BLOCK = 256;
constexpr int ADAMW_CHUNK = 4096;  // elements per workgroup: 256 threads x 4 quads
constexpr int ADAMW_MAX_TENSORS = 76;
static_assert(ADAMW_CHUNK == ADAMW_BLOCK * 16, "four quads per thread");

struct AdamwSlot {
    float* p;
    const float* g;
    float* m;
    float* v;
    int64_t n;
    float ns, rs;
};

// One launch's tensors.  chunk0[k]: the first chunk of tensor k, chunk0[K]: the launch's chunk count.  3980 bytes.
struct AdamwLaunch {
    AdamwSlot t[ADAMW_MAX_TENSORS];
    int32_t chunk0[ADAMW_MAX_TENSORS + 1];
    int32_t K;
    float decay, w1, b2, w2, e;
};
static_assert(sizeof(AdamwSlot) == 48 && sizeof(AdamwLaunch) + 64 <= 4096, "the tensor table travels in the kernel arguments");
static_assert(sizeof(AdamwLaunch) + 64 + sizeof(AdamwSlot) + 4 >= 4096, "... and one more tensor would leave no spare byte below it");

hipError_t launch_adamw(const AdamwLaunch& L, hipStream_t s);

}  // namespace parrot

#ifdef PARROT_OPTIM_TU
namespace parrot {

// (no contraction: an element is the same bits on the 16-byte and on the scalar path, and the bits of tests/adamw_ref.py)
#pragma clang fp contract(off)

__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, float decay, float w1, float b2, float w2, float e, float ns,
                                           float rs) {
    p = p * decay;
    m = m + (g - m) * w1;
    v = v * b2 + (g * w2) * g;
    const float d = sqrtf(v) / rs + e;
    p = p + ns * (m / d);
}

static __global__ __launch_bounds__(ADAMW_BLOCK) void adamw_kernel(const AdamwLaunch L) {
    const int chunk = blockIdx.x;
    // the last k with chunk0[k] <= chunk (tensors without a chunk share their successor's first chunk and are passed over)
    int lo = 0, hi = L.K - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (L.chunk0[mid] <= chunk) lo = mid;
        else hi = mid - 1;
    }
    const AdamwSlot t = L.t[lo];
    const int64_t e0 = (int64_t)(chunk - L.chunk0[lo]) * ADAMW_CHUNK;
    float* __restrict__ p = t.p;
    const float* __restrict__ g = t.g;
    float* __restrict__ m = t.m;
    float* __restrict__ v = t.v;
    const float decay = L.decay, w1 = L.w1, b2 = L.b2, w2 = L.w2, eps = L.e, ns = t.ns, rs = t.rs;
    const bool vec = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v)) & 15) == 0;
    if (vec && e0 + ADAMW_CHUNK <= t.n) {  // a whole chunk, 16-byte accesses: all loads first
        float4 vp[4], vg[4], vm[4], vv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t e = e0 + 4 * (threadIdx.x + ADAMW_BLOCK * i);
            vp[i] = *reinterpret_cast<const float4*>(p + e);
            vg[i] = *reinterpret_cast<const float4*>(g + e);
            vm[i] = *reinterpret_cast<const float4*>(m + e);
            vv[i] = *reinterpret_cast<const float4*>(v + e);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t e = e0 + 4 * (threadIdx.x + ADAMW_BLOCK * i);
            adamw_elem(vp[i].x, vg[i].x, vm[i].x, vv[i].x, decay, w1, b2, w2, eps, ns, rs);
            adamw_elem(vp[i].y, vg[i].y, vm[i].y, vv[i].y, decay, w1, b2, w2, eps, ns, rs);
            adamw_elem(vp[i].z, vg[i].z, vm[i].z, vv[i].z, decay, w1, b2, w2, eps, ns, rs);
            adamw_elem(vp[i].w, vg[i].w, vm[i].w, vv[i].w, decay, w1, b2, w2, eps, ns, rs);
            *reinterpret_cast<float4*>(p + e) = vp[i];
            *reinterpret_cast<float4*>(m + e) = vm[i];
            *reinterpret_cast<float4*>(v + e) = vv[i];
        }
        return;
    }
    // the tensor's last chunk, or a misaligned base: the same elements per thread
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t e = e0 + 4 * (threadIdx.x + ADAMW_BLOCK * i);
        if (e >= t.n) break;
        if (vec && e + 4 <= t.n) {
            float4 vp = *reinterpret_cast<const float4*>(p + e);
            const float4 vg = *reinterpret_cast<const float4*>(g + e);
            float4 vm = *reinterpret_cast<const float4*>(m + e);
            float4 vv = *reinterpret_cast<const float4*>(v + e);
            adamw_elem(vp.x, vg.x, vm.x, vv.x, decay, w1, b2, w2, eps, ns, rs);
            adamw_elem(vp.y, vg.y, vm.y, vv.y, decay, w1, b2, w2, eps, ns, rs);
            adamw_elem(vp.z, vg.z, vm.z, vv.z, decay, w1, b2, w2, eps, ns, rs);
            adamw_elem(vp.w, vg.w, vm.w, vv.w, decay, w1, b2, w2, eps, ns, rs);
            *reinterpret_cast<float4*>(p + e) = vp;
            *reinterpret_cast<float4*>(m + e) = vm;
            *reinterpret_cast<float4*>(v + e) = vv;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (e + j >= t.n) break;
                float xp = p[e + j], xm = m[e + j], xv = v[e + j];
                adamw_elem(xp, g[e + j], xm, xv, decay, w1, b2, w2, eps, ns, rs);
                p[e + j] = xp;
                m[e + j] = xm;
                v[e + j] = xv;
            }
        }
    }
}

}  // namespace parrot
#endif  // PARROT_OPTIM_TU
