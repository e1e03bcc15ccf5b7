// wave_reduce.h -- wave-wide (64 lanes) max / sum by shuffles, and the sum over a workgroup of 256; every lane gets the result.
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
// fp64 sum over the 256 threads of a workgroup in a fixed tree (sm: 256 doubles of LDS); every thread gets the result
__device__ __forceinline__ double block_sum(double v, double* sm) {
    const int tid = threadIdx.x;
    sm[tid] = v;
    __syncthreads();
#pragma unroll
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) sm[tid] += sm[tid + o];
        __syncthreads();
    }
    const double r = sm[0];
    __syncthreads();
    return r;
}

}  // namespace parrot
