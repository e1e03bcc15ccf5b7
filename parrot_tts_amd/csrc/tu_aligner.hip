// tu_aligner.hip -- one translation unit of libparrot_hip.so (parrot_tts_amd/build.py compiles them in parallel): the aligner's
// kernels (aligner.h) and their launchers.  Shapes are validated by the callers in host_aligner.hip.
#define PARROT_ALIGNER_TU
#include "aligner.h"
namespace parrot {
hipError_t launch_lstm_step(const LstmStepParams& p, hipStream_t s) {
    if (p.H % 16 || p.H > LSTM_MAX_DIM || p.B <= 0) return hipErrorInvalidValue;
    const size_t lds = ((size_t)LSTM_BT * p.H + 16 * LSTM_BT) * sizeof(float);
    hipLaunchKernelGGL(lstm_step_kernel, dim3(p.H / LSTM_UNITS, 2), dim3(256), lds, s, p);
    return hipGetLastError();
}
hipError_t launch_align_transpose(const float* in, float* out, int B, int R, int C, hipStream_t s) {
    if (B > 65535 || (R + 31) / 32 > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(align_transpose_kernel, dim3((C + 31) / 32, (R + 31) / 32, B), dim3(256), 0, s, in, out, R, C);
    return hipGetLastError();
}
hipError_t launch_align_epilogue(const float* in, float* out, const float* scale, const float* shift, int B, int C, int T, int G, int Mg,
                                 int relu, hipStream_t s) {
    const size_t total = (size_t)B * C * T;
    if ((total + 255) / 256 > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(align_epilogue_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, in, out, scale, shift, C, T, G, Mg, relu, total);
    return hipGetLastError();
}
hipError_t launch_align_softmax(const float* logits, const int32_t* mel_len, float* pred, int B, int T, int V, int* err, hipStream_t s) {
    const size_t rows = (size_t)B * T;
    if ((rows + 3) / 4 > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(align_softmax_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, logits, mel_len, pred, B, T, V, err);
    return hipGetLastError();
}
hipError_t launch_align_dp(const float* pred, const int64_t* tokens, const int32_t* mel_len, const int32_t* tokens_len, int B, int T, int V,
                           int N, uint8_t* bp, int32_t* dur, double* cost, int* status, hipStream_t s) {
    if (N > ALIGN_MAX_N || T > ALIGN_MAX_T) return hipErrorInvalidValue;
    const size_t lds = (size_t)N * (3 * sizeof(double) + sizeof(int));
    hipLaunchKernelGGL(align_dp_kernel, dim3(B), dim3(256), lds, s, pred, tokens, mel_len, tokens_len, T, V, N, bp, dur, cost, status);
    return hipGetLastError();
}
}  // namespace parrot
