// host_tte_loss.hip -- ModelLoss of the text-to-unit model (modules/loss.py:5-21) and its gradient (train.py:72-85): validation and
// the workspace layout around the launchers of tte_loss.h.
#include "host_common.h"

#include <algorithm>

#include "tte_loss.h"

using namespace parrot;

// The workspace of both entry points: one partial {nll, counts, first bad target} per stage-1 block; the gradient adds its scales.
struct LossWs {
    double* nll;
    LossCounts* cnt;
    int64_t* bad;
    LossScale* scale;
};
static LossWs loss_ws(Arena& a, int32_t N, bool grad) {
    const size_t nblk = (size_t)std::max((N + LOSS_WAVES - 1) / LOSS_WAVES, 1);
    LossWs w{};
    w.nll = a.take<double>(nblk);
    w.cnt = a.take<LossCounts>(nblk);
    w.bad = a.take<int64_t>(nblk);
    if (grad) w.scale = a.take<LossScale>(1);
    return w;
}
static size_t loss_ws_bytes(int32_t N, bool grad) {
    if (N < 0) return 0;
    Arena a(nullptr, 0);
    (void)loss_ws(a, N, grad);
    return align_up(a.off, 256);
}
extern "C" size_t parrot_tte_loss_workspace_bytes(int32_t N) { return loss_ws_bytes(N, false); }
extern "C" size_t parrot_tte_loss_grad_workspace_bytes(int32_t N) { return loss_ws_bytes(N, true); }

extern "C" int parrot_tte_loss(const float* logits, const int64_t* targets, int32_t N, int32_t V, int64_t ignore_index, const float* log_dur,
                               const int64_t* dur, const uint8_t* src_mask, int32_t n_src, double* out, float* losses, void* ws, size_t ws_bytes,
                               void* stream) {
    if (!logits || !targets || !log_dur || !dur || !src_mask || !out || !ws) return fail(PARROT_E_INVALID, "tte_loss: null argument");
    if (N <= 0 || V <= 0 || n_src < 0) return fail(PARROT_E_INVALID, "tte_loss: empty logits or negative size");
    hipStream_t s = (hipStream_t)stream;
    Arena a(ws, ws_bytes);
    const LossWs w = loss_ws(a, N, false);
    if (!a.ok) return fail(PARROT_E_NOMEM, "tte_loss: workspace too small");
    if (poison_word()) {
        TRY(poison(ws, ws_bytes, s));
        TRY(poison(out, 8 * sizeof(double), s));
        TRY(poison(losses, 3 * sizeof(float), s));
    }
    HIP_TRY(launch_tte_loss(logits, targets, N, V, ignore_index, log_dur, dur, src_mask, n_src, w.nll, w.cnt, w.bad, out, losses, s));
    return PARROT_OK;
}

extern "C" int parrot_tte_loss_grad(const float* logits, const int64_t* targets, int32_t N, int32_t V, int64_t ignore_index, const float* log_dur,
                                    const int64_t* dur, const uint8_t* src_mask, int32_t n_src, const double* weights, double* out, float* losses,
                                    float* grad_logits, float* grad_log_dur, void* ws, size_t ws_bytes, void* stream) {
    if (!logits || !targets || !log_dur || !dur || !src_mask || !out || !ws) return fail(PARROT_E_INVALID, "tte_loss_grad: null argument");
    if (N <= 0 || V <= 0 || n_src < 0) return fail(PARROT_E_INVALID, "tte_loss_grad: empty logits or negative size");
    if (!grad_logits && !grad_log_dur) return fail(PARROT_E_INVALID, "tte_loss_grad: both gradients null (parrot_tte_loss is the forward alone)");
    if (grad_logits == logits || grad_log_dur == log_dur) return fail(PARROT_E_INVALID, "tte_loss_grad: a gradient must not alias its input");
    hipStream_t s = (hipStream_t)stream;
    Arena a(ws, ws_bytes);
    const LossWs w = loss_ws(a, N, true);
    if (!a.ok) return fail(PARROT_E_NOMEM, "tte_loss_grad: workspace too small");
    if (poison_word()) {
        TRY(poison(ws, ws_bytes, s));
        TRY(poison(out, 8 * sizeof(double), s));
        TRY(poison(losses, 3 * sizeof(float), s));
        TRY(poison(grad_logits, (size_t)N * V * sizeof(float), s));
        TRY(poison(grad_log_dur, (size_t)n_src * sizeof(float), s));
    }
    HIP_TRY(launch_tte_loss_grad(logits, targets, N, V, ignore_index, log_dur, dur, src_mask, n_src, weights, w.nll, w.cnt, w.bad, w.scale, out,
                                 losses, grad_logits, grad_log_dur, s));
    return PARROT_OK;
}
