// tu_voc_train.hip -- one translation unit of libparrot_hip.so: the vocoder's training kernels (voc_train.h) and their launchers.  A
// launcher refuses (hipErrorInvalidValue, before any launch) sizes below 1 and grids beyond the limits; the model's shapes are
// validated by the callers in host_voc_train.hip.
#define PARROT_VOC_TRAIN_TU
#include "voc_train.h"

#define LAUNCH(...)                     \
    do {                                \
        hipLaunchKernelGGL(__VA_ARGS__); \
        return hipGetLastError();       \
    } while (0)

namespace parrot {

static inline bool grid_ok(size_t n) { return n >= 1 && (n + 255) / 256 <= 0x7fffffffu; }
static inline unsigned blocks256(size_t n) { return (unsigned)((n + 255) / 256); }

hipError_t vt_launch_wn_fwd(const float* v, const float* g, float* w, float* norm, int rows, int len, hipStream_t s) {
    if (rows < 1 || len < 1) return hipErrorInvalidValue;
    LAUNCH(vt_wn_fwd_kernel, dim3(rows), dim3(256), 0, s, v, g, w, norm, len);
}
hipError_t vt_launch_wn_bwd(const float* dw, const float* v, const float* g, const float* norm, float* dv, float* dg, int rows, int len, hipStream_t s) {
    if (rows < 1 || len < 1) return hipErrorInvalidValue;
    LAUNCH(vt_wn_bwd_kernel, dim3(rows), dim3(256), 0, s, dw, v, g, norm, dv, dg, len);
}
hipError_t vt_launch_embed(const int64_t* code, const int64_t* spkr, const float* dict, const float* spk_tab, float* x, int B, int U, int E, int n_emb,
                           int n_spkr, int multispkr, hipStream_t s) {
    if (B < 1 || U < 1 || E < 1) return hipErrorInvalidValue;
    const int Cin = multispkr ? 2 * E : E;
    const size_t n = (size_t)B * Cin * U;
    if (!grid_ok(n)) return hipErrorInvalidValue;
    LAUNCH(vt_embed_kernel, dim3(blocks256(n)), dim3(256), 0, s, code, spkr, dict, spk_tab, x, U, E, Cin, n_emb, n_spkr, n);
}
hipError_t vt_launch_lrelu(const float* x, float* a, float slope, size_t n, hipStream_t s) {
    if (!grid_ok(n)) return hipErrorInvalidValue;
    LAUNCH(vt_lrelu_kernel, dim3(blocks256(n)), dim3(256), 0, s, x, a, slope, n);
}
hipError_t vt_launch_mask(const float* a, uint8_t* out, size_t n, hipStream_t s) {
    if (!grid_ok(n)) return hipErrorInvalidValue;
    LAUNCH(vt_mask_kernel, dim3(blocks256(n)), dim3(256), 0, s, a, out, n);
}
hipError_t vt_launch_mrf(const float* r0, size_t stride, int nk, float* out, size_t n, hipStream_t s) {
    if (!grid_ok(n) || nk < 1 || nk > VT_MAX_KERNELS) return hipErrorInvalidValue;
    LAUNCH(vt_mrf_kernel, dim3(blocks256(n)), dim3(256), 0, s, r0, stride, nk, out, n);
}
hipError_t vt_launch_div(const float* g, int nk, float* out, size_t n, hipStream_t s) {
    if (!grid_ok(n) || nk < 1) return hipErrorInvalidValue;
    LAUNCH(vt_div_kernel, dim3(blocks256(n)), dim3(256), 0, s, g, (float)nk, out, n);
}
hipError_t vt_launch_add(const float* a, const float* b, float* y, size_t n, hipStream_t s) {
    if (!grid_ok(n)) return hipErrorInvalidValue;
    LAUNCH(vt_add_kernel, dim3(blocks256(n)), dim3(256), 0, s, a, b, y, n);
}
hipError_t vt_launch_tanh(const float* z, float* y, float* keep, size_t n, hipStream_t s) {
    if (!grid_ok(n)) return hipErrorInvalidValue;
    LAUNCH(vt_tanh_kernel, dim3(blocks256(n)), dim3(256), 0, s, z, y, keep, n);
}
hipError_t vt_launch_tanh_bwd(const float* y, const float* dy, float* dz, size_t n, hipStream_t s) {
    if (!grid_ok(n)) return hipErrorInvalidValue;
    LAUNCH(vt_tanh_bwd_kernel, dim3(blocks256(n)), dim3(256), 0, s, y, dy, dz, n);
}
hipError_t vt_launch_chansum(const float* g, float* out, int B, int C, int T, hipStream_t s) {
    if (B < 1 || C < 1 || T < 1) return hipErrorInvalidValue;
    LAUNCH(vt_chansum_kernel, dim3(C), dim3(256), 0, s, g, out, B, C, T);
}

}  // namespace parrot
