// tu_train_gemm.hip -- one translation unit of libparrot_hip.so: the fp32 tap-GEMM kernels of the three training paths
// (train_gemm.h) and their launchers.  A launcher refuses (hipErrorInvalidValue, before any launch) what its kernel cannot take:
// sizes below 1, too many taps, a grid beyond the limits.  What a model's shapes need beyond that is validated by the callers in
// host_aligner_train.hip, host_tte_train.hip and host_voc_train.hip.
#define PARROT_TRAIN_GEMM_TU
#include "train_gemm.h"
namespace parrot {
hipError_t launch_tap_gemm(const TapGemmParams& p, int Z, hipStream_t s) {
    if (p.ntaps < 1 || p.ntaps > TG_MAX_TAPS || p.M < 1 || p.N < 1 || p.K < 1 || Z < 1 || Z > 65535 || (p.M + 63) / 64 > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tap_gemm_kernel, dim3((p.N + 63) / 64, (p.M + 63) / 64, Z), dim3(256), 0, s, p);
    return hipGetLastError();
}
int wgrad_chunks(int R) { return (R + TG_RCHUNK - 1) / TG_RCHUNK; }
hipError_t launch_wgrad(const WgradParams& p, hipStream_t s) {
    const long z = (long)wgrad_chunks(p.R) * p.ntaps;
    if (p.ntaps < 1 || p.ntaps > TG_MAX_TAPS || p.M < 1 || p.K < 1 || p.R < 1 || z > 65535 || (p.M + 63) / 64 > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wgrad_kernel, dim3((p.K + 63) / 64, (p.M + 63) / 64, (unsigned)z), dim3(256), 0, s, p);
    return hipGetLastError();
}
hipError_t launch_wgrad_reduce(const float* part, int nchunks, int ntaps, int M, int K, float* out, long o_sm, long o_sk, long o_sj, hipStream_t s) {
    const size_t per = (size_t)ntaps * M * K;
    if (nchunks < 1 || ntaps < 1 || ntaps > TG_MAX_TAPS || M < 1 || K < 1 || (per + 255) / 256 > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, s, part, nchunks, ntaps, M, K, out, o_sm, o_sk, o_sj);
    return hipGetLastError();
}
hipError_t launch_colsum(const float* src, int R, int M, long ld, double* part, float* out0, float* out1, hipStream_t s) {
    const int nchunks = wgrad_chunks(R);
    if (R < 1 || M < 1 || nchunks > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(colsum_part_kernel, dim3((M + 63) / 64, nchunks), dim3(256), 0, s, src, R, M, ld, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(colsum_final_kernel, dim3((M + 255) / 256), dim3(256), 0, s, part, nchunks, M, out0, out1);
    return hipGetLastError();
}
}  // namespace parrot
