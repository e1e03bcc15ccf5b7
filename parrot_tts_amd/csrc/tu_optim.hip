// tu_optim.hip -- one translation unit of libparrot_hip.so: the fused AdamW kernel (optim.h) and its launcher.  Tensors are
// validated by the caller in host_optim.hip.  No fast-math flag on this unit: division and square root are the correctly rounded
// ones and subnormals are kept.
#define PARROT_OPTIM_TU
#include "optim.h"
namespace parrot {
hipError_t launch_adamw(const AdamwLaunch& L, hipStream_t s) {
    const int n_chunks = L.chunk0[L.K];
    if (n_chunks <= 0) return hipSuccess;  // (nothing but empty tensors)
    hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)n_chunks), dim3(ADAMW_BLOCK), 0, s, L);
    return hipGetLastError();
}
}  // namespace parrot
