// tu_gan_loss.hip -- one translation unit of libparrot_hip.so: the GAN loss kernels (gan_loss.h) and their launchers.  Terms are
// validated by the caller in host_gan_loss.hip.
#define PARROT_GAN_TU
#include "gan_loss.h"
namespace parrot {
hipError_t launch_gan_tiles(const GanLaunch& L, const double* weights, double* part, bool values, hipStream_t s) {
    const int n_tiles = L.tile0[L.K];
    if (n_tiles <= 0) return hipSuccess;  // (nothing but empty terms)
    const dim3 grid((unsigned)(n_tiles < GAN_GRID_CAP ? n_tiles : GAN_GRID_CAP));
    if (values)
        hipLaunchKernelGGL(gan_tiles_kernel<true>, grid, dim3(GAN_BLOCK), 0, s, L, weights, part);
    else
        hipLaunchKernelGGL(gan_tiles_kernel<false>, grid, dim3(GAN_BLOCK), 0, s, L, weights, part);
    return hipGetLastError();
}
hipError_t launch_gan_reduce(const GanLaunch& L, const double* part, double* mean, double* term_out, const double* mean_all, int K_all, double scale,
                             float* total, hipStream_t s) {
    hipLaunchKernelGGL(gan_reduce_kernel, dim3(1), dim3(GAN_REDUCE_BLOCK), 0, s, L, part, mean, term_out, mean_all, K_all, scale, total);
    return hipGetLastError();
}
}  // namespace parrot
