// gan_loss.h -- the vocoder's adversarial losses with their gradients (reference utils/vocoder/models.py:279-310: feature_loss,
// generator_loss, discriminator_loss; train.py:141-148, 159-165), every term of a training step in one launch.
//
// A term is (op, a, b, n) over dense fp32 arrays: PARROT_GAN_L1 mean |a - b|, PARROT_GAN_SQ1 mean (1 - a)^2, PARROT_GAN_SQ0 mean a^2.
// The work is cut into tiles of GAN_TILE elements; a tile belongs to one term and a term's tiling starts at its element 0.  The
// term table and the per-term tile prefix travel BY VALUE in the kernel arguments (GanLaunch, under the 4 KB limit): the entry
// point allocates nothing and copies nothing.  A workgroup strides over tiles and finds a tile's term by bisecting the prefix.
//
// Determinism: inside a tile, thread t owns the quads 4 (t + 256 i) .. + 3, i = 0 .. 3, whatever the alignment (16-byte loads and
// stores when every pointer of the term is 16-byte aligned, scalar ones otherwise and in the quad that crosses n); it adds its
// contributions, formed in fp64 from the fp32 inputs, in element order; the wave adds by a fixed butterfly (wave_reduce.h), the
// workgroup in wave order.  The sum is stored PER TILE, so neither the grid size nor the term's position enters a bit of it.
// gan_reduce_kernel then adds a term's tile sums in an order that depends on the term's tile count alone.  No atomics.
// The launchers are defined in tu_gan_loss.hip, which alone sees the kernel bodies (PARROT_GAN_TU).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/parrot_hip.h"

namespace parrot {

constexpr int GAN_TILE = 4096;                 // elements per tile: 256 threads x 4 quads
constexpr int GAN_BLOCK = 256;
constexpr int GAN_GRID_CAP = PARROT_GAN_GRID_CAP;  // workgroups per launch; the rest of the tiles by stride
constexpr int GAN_REDUCE_BLOCK = 1024;         // gan_reduce_kernel: 16 waves, one term per wave at a time
static_assert(GAN_TILE == GAN_BLOCK * 16, "four quads per thread");

// One launch's terms.  tile0[k]: the first tile of term k, tile0[K]: the launch's tile count.  3344 bytes.
struct GanLaunch {
    parrot_gan_term_t t[PARROT_GAN_MAX_TERMS];
    int32_t tile0[PARROT_GAN_MAX_TERMS + 1];
    int32_t K;
};
static_assert(sizeof(parrot_gan_term_t) == 48 && sizeof(GanLaunch) + 64 <= 4096, "the term table travels in the kernel arguments");

// part (the launch's tiles, fp64) <- per-tile sums, when `values`; the gradients of every term that asks for one.
// weights: device, this launch's K doubles, or null (ones).
hipError_t launch_gan_tiles(const GanLaunch& L, const double* weights, double* part, bool values, hipStream_t s);
// mean[k] (and term_out[k], nullable) <- sum of term k's tiles / n_k for this launch's terms; total (nullable) <-
// (float)(scale * sum of mean_all[0 .. K_all)) in table order: pass it with the LAST launch of a call.
hipError_t launch_gan_reduce(const GanLaunch& L, const double* part, double* mean, double* term_out, const double* mean_all, int K_all, double scale,
                             float* total, hipStream_t s);

}  // namespace parrot

#ifdef PARROT_GAN_TU
#include "wave_reduce.h"

namespace parrot {

// (no contraction: a contribution is the same bits in every instantiation)
#pragma clang fp contract(off)

// One element: its contribution (fp64) and, where asked for, its gradient(s).  gmag: (float)(w / n) for L1; c2: 2 w / n for the squares.
template <int OP>
__device__ __forceinline__ double gan_elem(float a, float b, float gmag, double c2, float& ga, float& gb) {
    if (OP == PARROT_GAN_L1) {
        // the sign from the comparison (a difference could be flushed to zero); a == b, or either NaN: 0, as torch's sgn
        gb = a < b ? gmag : (a > b ? -gmag : 0.f);
        ga = -gb;
        return fabs((double)a - (double)b);
    }
    if (OP == PARROT_GAN_SQ1) {
        const double d = 1.0 - (double)a;
        ga = (float)(-c2 * d);
        gb = 0.f;
        return d * d;
    }
    ga = (float)(c2 * (double)a);
    gb = 0.f;
    return (double)a * (double)a;
}

// One tile of one term -> this thread's sum of contributions (0 when !VALUES).
template <int OP, bool VALUES>
__device__ __forceinline__ double gan_tile(const parrot_gan_term_t& t, int64_t e_tile, float gmag, double c2) {
    const float* __restrict__ a = t.a;
    const float* __restrict__ b = t.b;
    float* __restrict__ grad_a = t.grad_a;
    float* __restrict__ grad_b = OP == PARROT_GAN_L1 ? t.grad_b : nullptr;
    const uintptr_t bits = (uintptr_t)a | (OP == PARROT_GAN_L1 ? (uintptr_t)b : 0) | (uintptr_t)grad_a | (uintptr_t)grad_b;
    const bool vec = (bits & 15) == 0;  // (the tile's first element is a multiple of 4: the bases decide)
    double sum = 0.0;
    if (vec && e_tile + GAN_TILE <= t.n) {  // a whole tile, 16-byte accesses: all loads first
        float4 va[4], vb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t e = e_tile + 4 * (threadIdx.x + GAN_BLOCK * i);
            va[i] = *reinterpret_cast<const float4*>(a + e);
            if (OP == PARROT_GAN_L1) vb[i] = *reinterpret_cast<const float4*>(b + e);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t e = e_tile + 4 * (threadIdx.x + GAN_BLOCK * i);
            const float xa[4] = {va[i].x, va[i].y, va[i].z, va[i].w};
            const float xb[4] = {OP == PARROT_GAN_L1 ? vb[i].x : 0.f, OP == PARROT_GAN_L1 ? vb[i].y : 0.f, OP == PARROT_GAN_L1 ? vb[i].z : 0.f,
                                 OP == PARROT_GAN_L1 ? vb[i].w : 0.f};
            float ga[4], gb[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double c = gan_elem<OP>(xa[j], xb[j], gmag, c2, ga[j], gb[j]);
                if (VALUES) sum += c;
            }
            if (grad_a) *reinterpret_cast<float4*>(grad_a + e) = make_float4(ga[0], ga[1], ga[2], ga[3]);
            if (OP == PARROT_GAN_L1 && grad_b) *reinterpret_cast<float4*>(grad_b + e) = make_float4(gb[0], gb[1], gb[2], gb[3]);
        }
        return sum;
    }
    // the term's last tile, or a misaligned base: the same elements per thread in the same order
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t e = e_tile + 4 * (threadIdx.x + GAN_BLOCK * i);
        if (e >= t.n) break;
        if (vec && e + 4 <= t.n) {
            const float4 va = *reinterpret_cast<const float4*>(a + e);
            float4 vb = make_float4(0.f, 0.f, 0.f, 0.f);
            if (OP == PARROT_GAN_L1) vb = *reinterpret_cast<const float4*>(b + e);
            const float xa[4] = {va.x, va.y, va.z, va.w}, xb[4] = {vb.x, vb.y, vb.z, vb.w};
            float ga[4], gb[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double c = gan_elem<OP>(xa[j], xb[j], gmag, c2, ga[j], gb[j]);
                if (VALUES) sum += c;
            }
            if (grad_a) *reinterpret_cast<float4*>(grad_a + e) = make_float4(ga[0], ga[1], ga[2], ga[3]);
            if (OP == PARROT_GAN_L1 && grad_b) *reinterpret_cast<float4*>(grad_b + e) = make_float4(gb[0], gb[1], gb[2], gb[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (e + j >= t.n) break;
                float ga, gb;
                const double c = gan_elem<OP>(a[e + j], OP == PARROT_GAN_L1 ? b[e + j] : 0.f, gmag, c2, ga, gb);
                if (VALUES) sum += c;
                if (grad_a) grad_a[e + j] = ga;
                if (OP == PARROT_GAN_L1 && grad_b) grad_b[e + j] = gb;
            }
        }
    }
    return sum;
}

template <bool VALUES>
static __global__ __launch_bounds__(GAN_BLOCK) void gan_tiles_kernel(const GanLaunch L, const double* __restrict__ weights, double* __restrict__ part) {
    __shared__ double wave_part[GAN_BLOCK / 64];
    const int n_tiles = L.tile0[L.K];
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        // the last k with tile0[k] <= tile (terms without a tile share their successor's first tile and are passed over)
        int lo = 0, hi = L.K - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (L.tile0[mid] <= tile) lo = mid;
            else hi = mid - 1;
        }
        const int k = lo;
        const parrot_gan_term_t t = L.t[k];
        const int64_t e_tile = (int64_t)(tile - L.tile0[k]) * GAN_TILE;
        float gmag = 0.f;
        double c2 = 0.0;
        if (t.grad_a || t.grad_b) {  // the magnitude once per term and tile, in fp64
            const double w = weights ? weights[k] : 1.0;
            const double q = w / (double)t.n;
            gmag = (float)q;
            c2 = 2.0 * w / (double)t.n;
        }
        double sum;
        if (t.op == PARROT_GAN_L1) sum = gan_tile<PARROT_GAN_L1, VALUES>(t, e_tile, gmag, c2);
        else if (t.op == PARROT_GAN_SQ1) sum = gan_tile<PARROT_GAN_SQ1, VALUES>(t, e_tile, gmag, c2);
        else sum = gan_tile<PARROT_GAN_SQ0, VALUES>(t, e_tile, gmag, c2);
        if (VALUES) {
            sum = wave_sum(sum);
            if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = sum;
            __syncthreads();
            if (threadIdx.x == 0) {
                double s = wave_part[0];
#pragma unroll
                for (int w = 1; w < GAN_BLOCK / 64; ++w) s += wave_part[w];
                part[tile] = s;
            }
            __syncthreads();  // (wave_part is reused by the next tile)
        }
    }
}

// One workgroup.  Wave w takes terms w, w + 16, ...: lane l adds the term's tiles l, l + 64, ... in that order, the wave by the
// butterfly -- an order fixed by the term's tile count.  mean = sum / n (n = 0: 0 / 0 = NaN, torch's mean of nothing).
static __global__ __launch_bounds__(GAN_REDUCE_BLOCK) void gan_reduce_kernel(const GanLaunch L, const double* __restrict__ part, double* mean,
                                                                               double* __restrict__ term_out, const double* mean_all, int K_all,
                                                                               double scale, float* __restrict__ total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = wave; k < L.K; k += GAN_REDUCE_BLOCK / 64) {
        const int t0 = L.tile0[k], t1 = L.tile0[k + 1];
        double s = 0.0;
        for (int i = t0 + lane; i < t1; i += 64) s += part[i];
        s = wave_sum(s);
        if (lane == 0) {
            const double m = s / (double)L.t[k].n;
            mean[k] = m;
            if (term_out) term_out[k] = m;
        }
    }
    if (!total) return;
    __syncthreads();  // (this launch's means are visible to thread 0; the earlier launches' came with the stream order)
    if (threadIdx.x == 0) {
        double acc = 0.0;
        for (int k = 0; k < K_all; ++k) acc += mean_all[k];
        *total = (float)(scale * acc);
    }
}

}  // namespace parrot
#endif  // PARROT_GAN_TU
