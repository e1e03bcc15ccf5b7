// tu_aligner_train.hip -- one translation unit of libparrot_hip.so: the aligner's training kernels (aligner_train.h) and their
// launchers.  A launcher refuses (hipErrorInvalidValue, before any launch) what its kernel cannot take: sizes below 1, a grid beyond
// the limits.  What the model's shapes need beyond that is validated by the callers in host_aligner_train.hip.
#define PARROT_ALIGNER_TRAIN_TU
#include "aligner_train.h"
namespace parrot {
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
