// tu_aligner_train.hip -- one translation unit of libparrot_hip.so: the aligner's training kernels (aligner_train.h) and their
// launchers.  A launcher refuses (hipErrorInvalidValue, before any launch) what its kernel cannot take: sizes below 1, too many taps,
// a grid beyond the limits.  What the model's shapes need beyond that is validated by the callers in host_aligner_train.hip.
#define PARROT_ALIGNER_TRAIN_TU
#include "aligner_train.h"
namespace parrot {
hipError_t launch_tap_gemm(const TapGemmParams& p, int Z, hipStream_t s) {
    if (p.ntaps < 1 || p.ntaps > AT_MAX_TAPS || p.M < 1 || p.N < 1 || p.K < 1 || Z < 1 || Z > 65535 || (p.M + 63) / 64 > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tap_gemm_kernel, dim3((p.N + 63) / 64, (p.M + 63) / 64, Z), dim3(256), 0, s, p);
    return hipGetLastError();
}
int wgrad_chunks(int R) { return (R + AT_RCHUNK - 1) / AT_RCHUNK; }
hipError_t launch_wgrad(const WgradParams& p, hipStream_t s) {
    const long z = (long)wgrad_chunks(p.R) * p.ntaps;
    if (p.ntaps < 1 || p.ntaps > AT_MAX_TAPS || p.M < 1 || p.K < 1 || p.R < 1 || z > 65535 || (p.M + 63) / 64 > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wgrad_kernel, dim3((p.K + 63) / 64, (p.M + 63) / 64, (unsigned)z), dim3(256), 0, s, p);
    return hipGetLastError();
}
hipError_t launch_wgrad_reduce(const float* part, int nchunks, int ntaps, int M, int K, float* out, long o_sm, long o_sk, long o_sj, hipStream_t s) {
    const size_t per = (size_t)ntaps * M * K;
    if (nchunks < 1 || ntaps < 1 || ntaps > AT_MAX_TAPS || M < 1 || K < 1 || (per + 255) / 256 > 0x7fffffffu) return hipErrorInvalidValue;
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
// (one workgroup per channel; n = B T is an int inside the kernels, and the unbiased running variance divides by n - 1)
hipError_t launch_bn_train(const BnTrainParams& p, hipStream_t s) {
    if (p.C < 1 || p.B < 1 || p.T < 1 || (long)p.B * p.T > 0x7fffffffL || (p.training && (long)p.B * p.T < 2)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bn_train_kernel, dim3(p.C), dim3(256), 0, s, p);
    return hipGetLastError();
}
hipError_t launch_bn_relu_bwd(const BnBwdParams& p, hipStream_t s) {
    if (p.C < 1 || p.B < 1 || p.T < 1 || (long)p.B * p.T > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bn_relu_bwd_kernel, dim3(p.C), dim3(256), 0, s, p);
    return hipGetLastError();
}
hipError_t launch_lstm_train_step(const LstmTrainParams& p, hipStream_t s) {
    if (p.H % 16 || p.H > 1024 || p.B <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lstm_train_step_kernel, dim3(p.H / AT_UNITS, 2), dim3(256), 0, s, p);
    return hipGetLastError();
}
hipError_t launch_lstm_bwd_step(const LstmBwdParams& p, hipStream_t s) {
    if (p.H % 16 || p.H > 1024 || p.B <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lstm_bwd_step_kernel, dim3(p.H / AT_UNITS, 2), dim3(256), 0, s, p);
    return hipGetLastError();
}
}  // namespace parrot
