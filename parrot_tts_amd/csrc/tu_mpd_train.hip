// tu_mpd_train.hip -- one translation unit of libparrot_hip.so: the multi-period discriminator's training kernels (mpd_train.h) and
// their launchers.  A launcher refuses (hipErrorInvalidValue, before any launch) sizes below 1 and grids beyond the limits; the
// model's shapes are validated by the callers in host_mpd_train.hip.
#define PARROT_MPD_TRAIN_TU
#include "mpd_train.h"

#define LAUNCH(...)                     \
    do {                                \
        hipLaunchKernelGGL(__VA_ARGS__); \
        return hipGetLastError();       \
    } while (0)

namespace parrot {

static inline unsigned blocks(long n, int per) { return (unsigned)((n + per - 1) / per); }
static inline bool first_ok(const MdFirst& d) {
    if (d.N < 1 || d.N > 65535 || d.T < 1 || d.p < 1 || d.p > 65535 || d.H < 1 || d.H1 < 1 || d.C1 < 1 || d.C1 > 65535) return false;
    if (d.k < 1 || d.k > TG_MAX_TAPS || d.s < 1) return false;
    // the fold: H p = T + n_pad with n_pad < min(p, T); the conv: H1 rows, the last of which starts inside the padded input
    const long Tp = (long)d.H * d.p;
    if (Tp < d.T || Tp - d.T >= d.p || Tp - d.T >= d.T || Tp > 0x3fffffffL) return false;
    if ((long)(d.H1 - 1) * d.s + d.k > (long)d.H + 2 * MD_PAD) return false;
    return (long)d.N * d.p * d.H1 * d.C1 <= 0x3fffffffL;
}

hipError_t md_launch_first_fwd(const MdFirst& d, const float* wav, const float* w, const float* bias, float* y, float slope, hipStream_t s) {
    if (!first_ok(d)) return hipErrorInvalidValue;
    LAUNCH(md_first_fwd_kernel, dim3(blocks(d.H1, 256), d.p, d.N), dim3(256), 0, s, d, wav, w, bias, y, slope);
}
hipError_t md_launch_first_dw(const MdFirst& d, const float* dy, const float* wav, double* part, float* dw, hipStream_t s) {
    if (!first_ok(d)) return hipErrorInvalidValue;
    const int chunks = md_chunks((long)d.N * d.p * d.H1), n = d.C1 * d.k;
    hipLaunchKernelGGL(md_first_dw_kernel, dim3(chunks, d.C1), dim3(256), 0, s, d, dy, wav, part);
    LAUNCH(md_reduce_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, part, chunks, n, dw);
}
hipError_t md_launch_first_dx(const MdFirst& d, const float* dy, const float* w, float* dwav, int accumulate, hipStream_t s) {
    if (!first_ok(d)) return hipErrorInvalidValue;
    LAUNCH(md_first_dx_kernel, dim3(blocks(d.H, 256), d.p, d.N), dim3(256), 0, s, d, dy, w, dwav, accumulate);
}
static inline bool post_ok(int Z, int C, int H) { return Z >= 1 && C >= 1 && C <= 65535 && H >= 1 && (long)Z * C * H <= 0x3fffffffL; }
hipError_t md_launch_post_fwd(const float* x, const float* w, const float* bias, float* y, int Z, int C, int H, hipStream_t s) {
    if (!post_ok(Z, C, H)) return hipErrorInvalidValue;
    const long R = (long)Z * H;
    LAUNCH(md_post_fwd_kernel, dim3(blocks(R, 64)), dim3(256), 0, s, x, w, bias, y, R, C, H);
}
hipError_t md_launch_post_dx(const float* dy, const float* w, const float* pre, const float* mask, float mslope, float* dx, int Z, int C, int H,
                             hipStream_t s) {
    if (!post_ok(Z, C, H)) return hipErrorInvalidValue;
    const size_t n = (size_t)Z * C * H;
    LAUNCH(md_post_dx_kernel, dim3(blocks((long)n, 256)), dim3(256), 0, s, dy, w, pre, mask, mslope, dx, n, C, H);
}
hipError_t md_launch_post_dw(const float* dy, const float* x, double* part, float* dw, int Z, int C, int H, hipStream_t s) {
    if (!post_ok(Z, C, H)) return hipErrorInvalidValue;
    const long R = (long)Z * H;
    const int chunks = md_chunks(R), n = C * MD_POST_K;
    hipLaunchKernelGGL(md_post_dw_kernel, dim3(chunks, C), dim3(256), 0, s, dy, x, part, R, C, H);
    LAUNCH(md_reduce_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, part, chunks, n, dw);
}

}  // namespace parrot
