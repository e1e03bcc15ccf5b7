// host_optim.hip -- the fused multi-tensor AdamW step (torch.optim.AdamW; reference utils/vocoder/train.py:80-82, 151, 168):
// validation, the host half of the update rule and the launches of optim.h.  Stateless: no handle, no device allocation, no copy,
// no host synchronisation.
#include "host_common.h"

#include <cmath>

#include "optim.h"

using namespace parrot;

// n <= 2^40 per tensor, and a launch is closed before its chunks pass 2^30: the chunk prefix stays an int32
static constexpr int64_t ADAMW_MAX_N = (int64_t)1 << 40;
static constexpr int64_t ADAMW_MAX_LAUNCH_CHUNKS = (int64_t)1 << 30;
static int64_t adamw_chunks(int64_t n) { return (n + ADAMW_CHUNK - 1) / ADAMW_CHUNK; }

extern "C" int32_t parrot_adamw_chunk(void) { return ADAMW_CHUNK; }
extern "C" int32_t parrot_adamw_max_tensors(void) { return ADAMW_MAX_TENSORS; }

extern "C" int parrot_adamw_step(const parrot_adamw_tensor_t* t, int32_t K, double lr, double beta1, double beta2, double eps, double weight_decay,
                                 void* stream) {
    if (K < 0 || (K > 0 && !t)) return fail(PARROT_E_INVALID, "adamw_step: null tensor table or negative K");
    if (!(lr >= 0.0)) return fail(PARROT_E_INVALID, "adamw_step: negative lr");
    if (!(eps >= 0.0)) return fail(PARROT_E_INVALID, "adamw_step: negative eps");
    if (!(weight_decay >= 0.0)) return fail(PARROT_E_INVALID, "adamw_step: negative weight_decay");
    if (!(beta1 >= 0.0 && beta1 < 1.0)) return fail(PARROT_E_INVALID, "adamw_step: beta1 outside [0, 1)");
    if (!(beta2 >= 0.0 && beta2 < 1.0)) return fail(PARROT_E_INVALID, "adamw_step: beta2 outside [0, 1)");
    for (int32_t k = 0; k < K; ++k) {
        const parrot_adamw_tensor_t& x = t[k];
        const std::string who = "adamw_step: tensor " + std::to_string(k);
        if (!x.p || !x.g || !x.m || !x.v) return fail(PARROT_E_INVALID, who + ": null pointer");
        if (x.n < 0) return fail(PARROT_E_INVALID, who + ": negative n");
        if (x.n > ADAMW_MAX_N) return fail(PARROT_E_UNSUPPORTED, who + ": more than 2^40 elements");
        if (x.step < 1) return fail(PARROT_E_INVALID, who + ": step below 1 (the count AFTER this update)");
        const void* q[4] = {x.p, x.g, x.m, x.v};
        for (int i = 0; i < 4; ++i)
            for (int j = i + 1; j < 4; ++j)
                if (q[i] == q[j]) return fail(PARROT_E_INVALID, who + ": two of p, g, m, v alias");
    }
    hipStream_t s = (hipStream_t)stream;
    AdamwLaunch L{};
    // the host half of the rule: double, each rounded to fp32 once
    L.decay = (float)(1.0 - lr * weight_decay);
    L.w1 = (float)(1.0 - beta1);
    L.b2 = (float)beta2;
    L.w2 = (float)(1.0 - beta2);
    L.e = (float)eps;
    for (int32_t k = 0; k < K; ++k) {
        const parrot_adamw_tensor_t& x = t[k];
        if (x.n == 0) continue;
        const int64_t c = adamw_chunks(x.n);
        if (L.K == ADAMW_MAX_TENSORS || L.chunk0[L.K] + c > ADAMW_MAX_LAUNCH_CHUNKS) {
            HIP_TRY(launch_adamw(L, s));
            L.K = 0;
        }
        AdamwSlot& d = L.t[L.K];
        d.p = x.p, d.g = x.g, d.m = x.m, d.v = x.v, d.n = x.n;
        d.ns = (float)(-lr / (1.0 - std::pow(beta1, (double)x.step)));
        d.rs = (float)std::sqrt(1.0 - std::pow(beta2, (double)x.step));
        L.chunk0[L.K + 1] = L.chunk0[L.K] + (int32_t)c;
        ++L.K;
    }
    if (L.K > 0) HIP_TRY(launch_adamw(L, s));
    return PARROT_OK;
}
