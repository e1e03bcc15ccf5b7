// tu_msd_train.hip -- one translation unit of libparrot_hip.so: the multi-scale discriminator's training kernels (msd_train.h) and
// their launchers.  A launcher refuses (hipErrorInvalidValue, before any launch) sizes below 1, grids beyond the limits and a window
// wider than the kernel's LDS; the model's shapes are validated by the callers in host_msd_train.hip.
#define PARROT_MSD_TRAIN_TU
#include "msd_train.h"

#include <algorithm>

#define LAUNCH(...)                     \
    do {                                \
        hipLaunchKernelGGL(__VA_ARGS__); \
        return hipGetLastError();       \
    } while (0)

namespace parrot {

static inline unsigned blocks(long n, int per) { return (unsigned)((n + per - 1) / per); }
constexpr long MS_LIM = 0x3fffffffL;
constexpr size_t MS_WG_BUDGET = (size_t)64 << 20;  // (train_gemm_host.h's WG_BUDGET: the partials of as many taps as fit, at least one)

static inline bool gconv_ok(const MsGconv& d, int Z) {
    if (Z < 1 || Z > 65535 || d.G < 1 || d.cin < 1 || d.cout < 1 || d.cin % d.G || d.cout % d.G) return false;
    if (d.k < 1 || d.k > MS_K || d.s < 1 || d.s > MS_MAX_STRIDE || d.s > d.k || d.pad < 0 || d.pad >= d.k || d.Tin < 1 || d.Tout < 1) return false;
    if ((long)d.Tin + 2 * d.pad < d.k || (long)d.Tout != ((long)d.Tin + 2 * d.pad - d.k) / d.s + 1) return false;
    const long mt_f = (d.cout / d.G + 63) / 64, mt_b = (d.cin / d.G + 63) / 64;
    if (d.G * mt_f > 65535 || d.G * mt_b > 65535) return false;
    return (long)Z * d.cin * d.Tin <= MS_LIM && (long)Z * d.cout * d.Tout <= MS_LIM && (long)d.cout * (d.cin / d.G) * d.k <= MS_LIM;
}

hipError_t ms_launch_gconv_fwd(const MsGconv& d, const float* x, const float* w0, const float* w1, int zsplit, const float* bias, float* y, int Z,
                               int act, float slope, hipStream_t s) {
    if (!gconv_ok(d, Z)) return hipErrorInvalidValue;
    MsGconvParams p{};
    p.d = d; p.mode = 0; p.tiles = (int)blocks(d.Tout, 64); p.mtiles = (d.cout / d.G + 63) / 64; p.zsplit = zsplit;
    p.w0 = w0; p.w1 = w1; p.X = x; p.C = y; p.bias = bias; p.lrelu = act; p.lslope = slope;
    LAUNCH(ms_gconv_kernel, dim3(p.tiles, d.G * p.mtiles, Z), dim3(256), 0, s, p);
}
hipError_t ms_launch_gconv_dx(const MsGconv& d, const float* dy, const float* w0, const float* w1, int zsplit, const float* pre, const float* mask,
                              float mslope, float* dx, int Z, hipStream_t s) {
    if (!gconv_ok(d, Z)) return hipErrorInvalidValue;
    MsGconvParams p{};
    p.d = d; p.mode = 1; p.tiles = (int)blocks((d.Tin + d.s - 1) / d.s, 64); p.mtiles = (d.cin / d.G + 63) / 64; p.zsplit = zsplit;
    p.w0 = w0; p.w1 = w1; p.X = dy; p.C = dx; p.pre = pre; p.mask = mask; p.mslope = mslope;
    LAUNCH(ms_gconv_kernel, dim3(p.tiles * d.s, d.G * p.mtiles, Z), dim3(256), 0, s, p);
}
static inline long gw_chunks(const MsGconv& d, int Z) { return ((long)Z * d.Tout + TG_RCHUNK - 1) / TG_RCHUNK; }
size_t ms_gwgrad_part_floats(const MsGconv& d, int Z) {
    if (!gconv_ok(d, Z)) return 0;
    const size_t chunks = (size_t)gw_chunks(d, Z), mk = (size_t)d.cout * (d.cin / d.G);
    return chunks * std::max(mk, std::min(mk * d.k, MS_WG_BUDGET / sizeof(float) / chunks));
}
hipError_t ms_launch_gconv_dw(const MsGconv& d, const float* dy, const float* x, float* dw, int Z, float* part, size_t part_floats, hipStream_t s) {
    if (!gconv_ok(d, Z)) return hipErrorInvalidValue;
    const long chunks = gw_chunks(d, Z);
    const size_t mk = (size_t)d.cout * (d.cin / d.G);
    if (chunks > 65535 || part_floats < (size_t)chunks * mk) return hipErrorInvalidValue;
    const int cing = d.cin / d.G, G = (int)std::min<size_t>((size_t)d.k, part_floats / ((size_t)chunks * mk));
    MsGwgradParams p{};
    p.d = d; p.dy = dy; p.x = x; p.part = part; p.R = Z * d.Tout; p.mtiles = (d.cout / d.G + 63) / 64;
    for (int j0 = 0; j0 < d.k; j0 += G) {
        p.j0 = j0; p.ntg = std::min(G, d.k - j0);
        hipLaunchKernelGGL(ms_gwgrad_kernel, dim3(blocks((long)cing * p.ntg, 64), d.G * p.mtiles, (unsigned)chunks), dim3(256), 0, s, p);
        hipLaunchKernelGGL(ms_gwgrad_reduce_kernel, dim3(blocks((long)mk * p.ntg, 256)), dim3(256), 0, s, part, (int)chunks, d.cout, cing, p.ntg, j0,
                           d.k, dw);
    }
    return hipGetLastError();
}

static inline bool first_ok(int Z, int T, int C) { return Z >= 1 && Z <= 65535 && T >= 1 && C >= 1 && C <= 65535 && (long)Z * T * C <= MS_LIM; }
hipError_t ms_launch_first_fwd(const float* wav, const float* w0, const float* w1, int zsplit, const float* bias, float* y, int Z, int T, int C,
                               float slope, hipStream_t s) {
    if (!first_ok(Z, T, C)) return hipErrorInvalidValue;
    LAUNCH(ms_first_fwd_kernel, dim3(blocks(T, 256), Z), dim3(256), 0, s, wav, w0, w1, zsplit, bias, y, T, C, slope);
}
hipError_t ms_launch_first_dw(const float* dy, const float* wav, double* part, float* dw, int Z, int T, int C, hipStream_t s) {
    if (!first_ok(Z, T, C)) return hipErrorInvalidValue;
    const long R = (long)Z * T;
    const int chunks = ms_chunks(R), n = C * MS_FIRST_K;
    hipLaunchKernelGGL(ms_first_dw_kernel, dim3(chunks, C), dim3(256), 0, s, dy, wav, part, R, T, C);
    LAUNCH(ms_reduce_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, part, chunks, n, dw);
}
hipError_t ms_launch_first_dx(const float* dy, const float* w0, const float* w1, int zsplit, float* dwav, int Z, int T, int C, hipStream_t s) {
    if (!first_ok(Z, T, C)) return hipErrorInvalidValue;
    LAUNCH(ms_first_dx_kernel, dim3(blocks(T, 256), Z), dim3(256), 0, s, dy, w0, w1, zsplit, dwav, T, C);
}

static inline bool pool_ok(int Z, int T) { return Z >= 1 && Z <= 65535 && T >= 1 && (long)Z * T <= MS_LIM; }
hipError_t ms_launch_pool_fwd(const float* x, float* y, int Z, int T, hipStream_t s) {
    if (!pool_ok(Z, T)) return hipErrorInvalidValue;
    const int To = T / 2 + 1;
    LAUNCH(ms_pool_fwd_kernel, dim3(blocks(To, 256), Z), dim3(256), 0, s, x, y, T, To);
}
hipError_t ms_launch_pool_bwd(const float* dy, float* dx, int Z, int T, int accumulate, hipStream_t s) {
    if (!pool_ok(Z, T)) return hipErrorInvalidValue;
    LAUNCH(ms_pool_bwd_kernel, dim3(blocks(T, 256), Z), dim3(256), 0, s, dy, dx, T, T / 2 + 1, accumulate);
}

static inline bool sn_ok(int rows, int cols) { return rows >= 1 && cols >= 1 && (long)rows * cols <= MS_LIM; }
hipError_t ms_launch_sn_fold(const float* w, float* u, float* v, int rows, int cols, int iterate, float* wf, float* sigma, float* tmp, hipStream_t s) {
    if (!sn_ok(rows, cols)) return hipErrorInvalidValue;
    float *tu = tmp, *tv = tmp + rows;
    if (iterate) {
        hipLaunchKernelGGL(ms_sn_mvt_kernel, dim3(blocks(cols, 64)), dim3(256), 0, s, w, u, tv, rows, cols);
        hipLaunchKernelGGL(ms_sn_normalize_kernel, dim3(1), dim3(256), 0, s, tv, v, cols);
    }
    hipLaunchKernelGGL(ms_sn_mv_kernel, dim3(rows), dim3(256), 0, s, w, v, tu, cols);
    hipLaunchKernelGGL(ms_sn_sigma_kernel, dim3(1), dim3(256), 0, s, tu, u, rows, iterate, sigma);
    const size_t n = (size_t)rows * cols;
    LAUNCH(ms_sn_fold_kernel, dim3(blocks((long)n, 256)), dim3(256), 0, s, w, sigma, wf, n);
}
hipError_t ms_launch_sn_bwd(const float* ga, const float* gb, const float* w, const float* ua, const float* va, const float* sa, const float* ub,
                            const float* vb, const float* sb, float* dw, int rows, int cols, double* part, hipStream_t s) {
    if (!sn_ok(rows, cols)) return hipErrorInvalidValue;
    const size_t n = (size_t)rows * cols;
    const int chunks = ms_chunks((long)n), halves = gb ? 2 : 1;
    hipLaunchKernelGGL(ms_sn_dot_kernel, dim3(chunks, halves), dim3(256), 0, s, ga, gb, w, part, n, chunks);
    hipLaunchKernelGGL(ms_sn_coef_kernel, dim3(1), dim3(halves), 0, s, part, chunks, sa, sb);
    LAUNCH(ms_sn_bwd_kernel, dim3(blocks((long)n, 256)), dim3(256), 0, s, ga, gb, ua, va, sa, ub, vb, sb, part, chunks, dw, rows, cols);
}

}  // namespace parrot
