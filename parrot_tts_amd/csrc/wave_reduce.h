// wave_reduce.h -- wave-wide (64 lanes) max / sum by shuffles; every lane gets the result.
#pragma once
#include <hip/hip_runtime.h>

namespace parrot {

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// (fp64: the butterfly adds the same pairs in every lane, so the order is fixed and every lane holds the same bits)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

}  // namespace parrot
