// tu_ctc.hip -- one translation unit of libparrot_hip.so: the CTC loss and gradient kernels (ctc.h) and their launchers.  Shapes
// are validated by the caller in host_aligner.hip.
#define PARROT_CTC_TU
#include "ctc.h"
namespace parrot {
hipError_t launch_ctc_lse(const float* logits, const int32_t* mel_len, double* lse, int B, int T, int V, int* status, hipStream_t s) {
    const size_t rows = (size_t)B * T;
    if ((rows + 3) / 4 > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ctc_lse_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, logits, mel_len, lse, B, T, V, status);
    return hipGetLastError();
}
static int ctc_block(int N) { return ((2 * N + 1 < CTC_BLOCK ? 2 * N + 1 : CTC_BLOCK) + 63) / 64 * 64; }  // one state per thread up to 1024 states
hipError_t launch_ctc_alpha(const float* logits, const int64_t* tokens, const int32_t* mel_len, const int32_t* tokens_len, const double* lse, int B,
                            int T, int V, int N, double* nll, float* mean, double* alpha, int* status, hipStream_t s) {
    if (N < 1 || N > ALIGN_MAX_N || T > ALIGN_MAX_T) return hipErrorInvalidValue;
    const int nt = ctc_block(N);
    if (alpha)
        hipLaunchKernelGGL(ctc_alpha_kernel<true>, dim3(B), dim3(nt), 0, s, logits, tokens, mel_len, tokens_len, lse, T, V, N, nll, alpha, status);
    else
        hipLaunchKernelGGL(ctc_alpha_kernel<false>, dim3(B), dim3(nt), 0, s, logits, tokens, mel_len, tokens_len, lse, T, V, N, nll, alpha, status);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !mean) return e;
    hipLaunchKernelGGL(ctc_mean_kernel, dim3(1), dim3(64), 0, s, nll, tokens_len, B, mean);
    return hipGetLastError();
}
hipError_t launch_ctc_grad(const float* logits, const int64_t* tokens, const int32_t* mel_len, const int32_t* tokens_len, const double* lse,
                           const double* nll, const double* row_weight, int zero_infinity, int B, int T, int V, int N, CtcGradWs ws, float* grad,
                           hipStream_t s) {
    const size_t rows = (size_t)B * T;
    if (N < 1 || N > ALIGN_MAX_N || T > ALIGN_MAX_T || (rows + 3) / 4 > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ctc_index_kernel, dim3(B), dim3(CTC_BLOCK), 0, s, tokens, mel_len, tokens_len, T, V, N, ws.order, ws.seg_lo, ws.seg_hi);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ctc_beta_kernel, dim3(B), dim3(ctc_block(N)), 0, s, logits, tokens, mel_len, tokens_len, lse, nll, T, V, N, ws.occ);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ctc_grad_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, logits, mel_len, tokens_len, lse, nll, ws.occ, ws.order,
                       ws.seg_lo, ws.seg_hi, row_weight, zero_infinity, B, T, V, N, grad);
    return hipGetLastError();
}
}  // namespace parrot
