// host_aligner_train.hip -- training the forced aligner: the batch-statistics forward and the full backward as two stateless calls
// (kernels and launchers: aligner_train.h / tu_aligner_train.hip; the matrix products: train_gemm_host.h).  No handle, no packed
// weights, no host copy and no synchronisation: every weight is read from the device pointer it is given.
#include "host_common.h"

#include <algorithm>
#include <string>

#include "aligner.h"
#include "aligner_train.h"
#include "train_gemm_host.h"

using namespace parrot;

namespace {

constexpr int ALIGNER_TAPS = 5;  // the aligner's convs; also the slots of the debug descriptors
constexpr long AT_MAX_BT = (long)(65535 / ALIGNER_TAPS) * TG_RCHUNK;  // wgrad_kernel's grid.z = chunks x taps: every weight gradient is one launch

// What the forward keeps for the backward.  Activations are channel-first (B, C, T) around the convs, (B, T, C) around the LSTM.
struct TrainSaved {
    float *r[3], *y[3];        // (B, conv_dim, T): ReLU output (the BatchNorm's input) and BatchNorm output of block i
    float *mean[3], *invstd[3];  // (conv_dim): the statistics block i normalised with
    float *gates, *c_all, *h;  // (B, T, 8H) gate activations; (B, T, 2H) cell states; (B, T, 2H) LSTM output
};
TrainSaved train_saved(const parrot_aligner_cfg& cfg, Arena& ar, int B, int T) {
    const size_t BT = (size_t)B * T, H = (size_t)cfg.lstm_dim, D = (size_t)cfg.conv_dim;
    TrainSaved sv{};
    for (int i = 0; i < 3; ++i) {
        sv.r[i] = ar.take<float>(BT * D);
        sv.y[i] = ar.take<float>(BT * D);
        sv.mean[i] = ar.take<float>(D);
        sv.invstd[i] = ar.take<float>(D);
    }
    sv.gates = ar.take<float>(BT * 8 * H);
    sv.c_all = ar.take<float>(BT * 2 * H);
    sv.h = ar.take<float>(BT * 2 * H);
    return sv;
}
size_t saved_bytes(const parrot_aligner_cfg& cfg, int B, int T) {
    Arena ar(nullptr, 0);
    (void)train_saved(cfg, ar, B, T);
    return align_up(ar.off, 256);
}
// One workspace layout for both calls.  The forward uses xproj, hbuf, cbuf and -- when the caller keeps nothing (training = 0,
// saved = NULL) -- `saved`; the backward uses the rest.
struct TrainScratch {
    float *xproj;          // (B, T, 8H)
    float *hbuf, *cbuf;    // [2][2][B][H], [2][B][H]
    char* saved;           // saved_bytes
    float *dlstm, *dgates; // (B, T, 2H), (B, T, 8H)
    float *dc, *w_hh_t;    // [2][B][H], [2][H][4H]
    float *da, *db;        // (B, conv_dim, T) each: gradient at a block's output / at its conv's output
    float* part;           // chunks x the largest weight gradient, all its taps: with B T <= AT_MAX_BT wgrad_group never splits one
    size_t part_floats;
    double* colpart;       // chunks x max(8H, V)
};
TrainScratch train_scratch(const parrot_aligner_cfg& cfg, Arena& ar, int B, int T) {
    const size_t BT = (size_t)B * T, H = (size_t)cfg.lstm_dim, D = (size_t)cfg.conv_dim, V = (size_t)cfg.num_symbols, F = (size_t)cfg.n_mels;
    const size_t chunks = (size_t)wgrad_chunks((int)BT);
    TrainScratch w{};
    w.xproj = ar.take<float>(BT * 8 * H);
    w.hbuf = ar.take<float>((size_t)2 * 2 * B * H);
    w.cbuf = ar.take<float>((size_t)2 * B * H);
    w.saved = ar.take<char>(saved_bytes(cfg, B, T));
    w.dlstm = ar.take<float>(BT * 2 * H);
    w.dgates = ar.take<float>(BT * 8 * H);
    w.dc = ar.take<float>((size_t)2 * B * H);
    w.w_hh_t = ar.take<float>((size_t)2 * H * 4 * H);
    w.da = ar.take<float>(BT * D);
    w.db = ar.take<float>(BT * D);
    size_t wmax = std::max(std::max(D * D * 5, D * F * 5), std::max(std::max(4 * H * D, 4 * H * H), V * 2 * H));
    w.part_floats = chunks * wmax;
    w.part = ar.take<float>(w.part_floats);
    w.colpart = ar.take<double>(chunks * std::max(8 * H, V));
    return w;
}
int train_cfg_ok(const parrot_aligner_cfg* cfg, int B, int T, const char* who) {
    const std::string w(who);
    if (cfg->n_mels < 1 || cfg->num_symbols < 1 || cfg->lstm_dim < 1 || cfg->conv_dim < 1) return fail(PARROT_E_INVALID, w + ": dimensions must be positive");
    if (cfg->lstm_dim % 16 || cfg->conv_dim % 16) return fail(PARROT_E_UNSUPPORTED, w + ": conv_dim and lstm_dim must be multiples of 16");
    if (cfg->lstm_dim > LSTM_MAX_DIM) return fail(PARROT_E_UNSUPPORTED, w + ": lstm_dim > 1024");
    if (B <= 0 || B > 65535 || T <= 0) return fail(PARROT_E_INVALID, w + ": need 1 <= B <= 65535 and T >= 1");
    if (T > ALIGN_MAX_T) return fail(PARROT_E_UNSUPPORTED, w + ": T > 32768 frames");
    if ((long)B * T > AT_MAX_BT) return fail(PARROT_E_UNSUPPORTED, w + ": B T beyond " + std::to_string(AT_MAX_BT) + " frames per batch");
    return PARROT_OK;
}
bool train_cfg_quiet_ok(const parrot_aligner_cfg* cfg, int B, int T) {
    return cfg && cfg->n_mels >= 1 && cfg->num_symbols >= 1 && cfg->lstm_dim >= 1 && cfg->conv_dim >= 1 && cfg->lstm_dim % 16 == 0 &&
           cfg->conv_dim % 16 == 0 && cfg->lstm_dim <= LSTM_MAX_DIM && B > 0 && B <= 65535 && T > 0 && T <= ALIGN_MAX_T && (long)B * T <= AT_MAX_BT;
}
int weights_ok(const parrot_aligner_dev_weights* w, const char* who) {
    bool ok = w->lin_w && w->lin_b;
    for (int i = 0; i < 3; ++i) ok = ok && w->conv_w[i] && w->bn_weight[i] && w->bn_bias[i] && w->bn_mean[i] && w->bn_var[i];
    for (int d = 0; d < 2; ++d) ok = ok && w->w_ih[d] && w->w_hh[d] && w->b_ih[d] && w->b_hh[d];
    return ok ? PARROT_OK : fail(PARROT_E_INVALID, std::string(who) + ": null weight");
}

// The training recurrence as the forward runs it: lstm_run_steps (host_aligner.hip) over lstm_train_step_kernel.  The initial state
// into half 0 of hbuf [2][2][B][H] and into q.c (zeros when h0 / c0 are null), one launch per step; afterwards h of the last step is
// half n_steps & 1 of hbuf and c is q.c.  Also behind parrot_debug_lstm.
int lstm_train_run_steps(LstmTrainParams q, float* hbuf, const float* h0, const float* c0, int n_steps, hipStream_t s) {
    const size_t hn = (size_t)2 * q.B * q.H;
    if (h0) HIP_TRY(hipMemcpyAsync(hbuf, h0, hn * sizeof(float), hipMemcpyDeviceToDevice, s));
    else HIP_TRY(hipMemsetAsync(hbuf, 0, hn * sizeof(float), s));
    if (c0) HIP_TRY(hipMemcpyAsync(q.c, c0, hn * sizeof(float), hipMemcpyDeviceToDevice, s));
    else HIP_TRY(hipMemsetAsync(q.c, 0, hn * sizeof(float), s));
    for (int step = 0; step < n_steps; ++step) {
        q.step = step;
        q.h_prev = hbuf + (size_t)(step & 1) * hn;
        q.h_next = hbuf + (size_t)((step + 1) & 1) * hn;
        HIP_TRY(launch_lstm_train_step(q, s));
    }
    return PARROT_OK;
}

}  // namespace

extern "C" size_t parrot_aligner_train_saved_bytes(const parrot_aligner_cfg* cfg, int32_t B, int32_t T) {
    return train_cfg_quiet_ok(cfg, B, T) ? saved_bytes(*cfg, B, T) : 0;
}
extern "C" size_t parrot_aligner_train_workspace_bytes(const parrot_aligner_cfg* cfg, int32_t B, int32_t T) {
    if (!train_cfg_quiet_ok(cfg, B, T)) return 0;
    Arena ar(nullptr, 0);
    (void)train_scratch(*cfg, ar, B, T);
    return align_up(ar.off, 256);
}

extern "C" int parrot_aligner_train_forward(const parrot_aligner_cfg* cfg, const parrot_aligner_dev_weights* wt, const float* mel, int32_t B, int32_t T,
                                            int32_t training, float* logits, void* saved, void* ws, size_t ws_bytes, void* stream) {
    if (!cfg || !wt || !mel || !logits || !ws) return fail(PARROT_E_INVALID, "aligner_train_forward: null argument");
    TRY(train_cfg_ok(cfg, B, T, "aligner_train_forward"));
    TRY(weights_ok(wt, "aligner_train_forward"));
    if (training && !saved) return fail(PARROT_E_INVALID, "aligner_train_forward: training needs the saved buffer");
    if (training && (long)B * T == 1) return fail(PARROT_E_INVALID, "aligner_train_forward: Expected more than 1 value per channel when training");
    hipStream_t s = (hipStream_t)stream;
    const int H = cfg->lstm_dim, D = cfg->conv_dim, V = cfg->num_symbols, F = cfg->n_mels;
    Arena ar(ws, ws_bytes);
    const TrainScratch w = train_scratch(*cfg, ar, B, T);
    if (!ar.ok) return fail(PARROT_E_NOMEM, "aligner_train_forward: workspace too small");
    const size_t sv_bytes = saved_bytes(*cfg, B, T);
    if (poison_word()) {
        TRY(poison(ws, ws_bytes, s));
        if (saved) TRY(poison(saved, sv_bytes, s));
        TRY(poison(logits, (size_t)B * T * V * sizeof(float), s));
    }
    Arena sa(saved ? saved : (void*)w.saved, sv_bytes);
    const TrainSaved sv = train_saved(*cfg, sa, B, T);
    // 3 x [conv(k = 5, pad 2) -> ReLU -> BatchNorm] on the padded batch as it stands (model.py:16-19, 41-45)
    for (int i = 0; i < 3; ++i) {
        Epi relu;
        relu.relu = 1;
        const Lay lx = i ? chan_first(D, T) : chan_last(T, F);  // mel (B, T, n_mels) read transposed
        TRY(conv_fwd(ConvW{wt->conv_w[i], D, i ? D : F, 5, 1, 2}, i ? sv.y[i - 1] : mel, lx, sv.r[i], chan_first(D, T), B, T, relu, s));
        BnTrainParams bn{};
        bn.x = sv.r[i]; bn.y = sv.y[i];
        bn.gamma = wt->bn_weight[i]; bn.beta = wt->bn_bias[i];
        bn.run_mean = wt->bn_mean[i]; bn.run_var = wt->bn_var[i];
        bn.mean = sv.mean[i]; bn.invstd = sv.invstd[i];
        bn.B = B; bn.C = D; bn.T = T; bn.training = training ? 1 : 0;
        bn.eps = cfg->bn_eps;
        HIP_TRY(launch_bn_train(bn, s));
    }
    // W_ih x + (b_ih + b_hh) of both directions for all frames, written as (B, T, 8H)
    for (int d = 0; d < 2; ++d) {
        Epi bias;
        bias.bias0 = wt->b_ih[d]; bias.bias1 = wt->b_hh[d];
        TRY(conv_fwd(ConvW{wt->w_ih[d], 4 * H, D, 1, 1, 0}, sv.y[2], chan_first(D, T), w.xproj + (size_t)d * 4 * H, chan_last(T, 8 * H), B, T, bias, s));
    }
    LstmTrainParams q{};
    q.w_hh[0] = wt->w_hh[0]; q.w_hh[1] = wt->w_hh[1];
    q.xproj = w.xproj; q.c = w.cbuf; q.out = sv.h; q.gates = sv.gates; q.c_all = sv.c_all;
    q.B = B; q.T = T; q.H = H;
    TRY(lstm_train_run_steps(q, w.hbuf, nullptr, nullptr, T, s));  // h_0 = c_0 = 0
    Epi bias;
    bias.bias0 = wt->lin_b;
    return conv_fwd(ConvW{wt->lin_w, V, 2 * H, 1, 1, 0}, sv.h, chan_last(T, 2 * H), logits, chan_last(T, V), B, T, bias, s);
}

extern "C" int parrot_aligner_train_backward(const parrot_aligner_cfg* cfg, const parrot_aligner_dev_weights* wt, const float* mel, const void* saved,
                                             const float* grad_logits, int32_t B, int32_t T, const parrot_aligner_grads* gr, void* ws, size_t ws_bytes,
                                             void* stream) {
    if (!cfg || !wt || !mel || !saved || !grad_logits || !gr || !ws) return fail(PARROT_E_INVALID, "aligner_train_backward: null argument");
    TRY(train_cfg_ok(cfg, B, T, "aligner_train_backward"));
    TRY(weights_ok(wt, "aligner_train_backward"));
    if ((long)B * T == 1) return fail(PARROT_E_INVALID, "aligner_train_backward: Expected more than 1 value per channel when training");
    hipStream_t s = (hipStream_t)stream;
    const int H = cfg->lstm_dim, D = cfg->conv_dim, V = cfg->num_symbols, F = cfg->n_mels, BT = B * T;
    Arena ar(ws, ws_bytes);
    const TrainScratch w = train_scratch(*cfg, ar, B, T);
    if (!ar.ok) return fail(PARROT_E_NOMEM, "aligner_train_backward: workspace too small");
    if (poison_word()) {
        TRY(poison(ws, ws_bytes, s));
        for (int i = 0; i < 3; ++i) {
            TRY(poison(gr->conv_w[i], (size_t)D * (i ? D : F) * 5 * sizeof(float), s));
            TRY(poison(gr->bn_weight[i], (size_t)D * sizeof(float), s));
            TRY(poison(gr->bn_bias[i], (size_t)D * sizeof(float), s));
        }
        for (int d = 0; d < 2; ++d) {
            TRY(poison(gr->w_ih[d], (size_t)4 * H * D * sizeof(float), s));
            TRY(poison(gr->w_hh[d], (size_t)4 * H * H * sizeof(float), s));
            TRY(poison(gr->b_ih[d], (size_t)4 * H * sizeof(float), s));
            TRY(poison(gr->b_hh[d], (size_t)4 * H * sizeof(float), s));
        }
        TRY(poison(gr->lin_w, (size_t)V * 2 * H * sizeof(float), s));
        TRY(poison(gr->lin_b, (size_t)V * sizeof(float), s));
    }
    Arena sa(const_cast<void*>(saved), saved_bytes(*cfg, B, T));
    const TrainSaved sv = train_saved(*cfg, sa, B, T);
    const Lay lh = chan_last(T, 2 * H), lg = chan_last(T, 8 * H), lv = chan_last(T, V), lc = chan_first(D, T);  // h / dlstm, gates, logits, conv blocks
    const ConvW lin{wt->lin_w, V, 2 * H, 1, 1, 0};

    // ---- Linear(2H -> V): db, dW, dX -------------------------------------------------------------
    if (gr->lin_b) TRY(colsum(grad_logits, BT, V, V, w.colpart, gr->lin_b, nullptr, s));
    if (gr->lin_w) TRY(conv_dw(lin, grad_logits, lv, sv.h, lh, gr->lin_w, B, T, w.part, w.part_floats, s));
    TRY(conv_dx(lin, grad_logits, lv, w.dlstm, lh, B, T, Epi(), s));  // dlstm (B, T, 2H) = grad_logits lin_w

    // ---- the LSTM back through time, both directions per launch ----------------------------------
    for (int d = 0; d < 2; ++d) HIP_TRY(launch_align_transpose(wt->w_hh[d], w.w_hh_t + (size_t)d * H * 4 * H, 1, 4 * H, H, s));
    HIP_TRY(hipMemsetAsync(w.dc, 0, (size_t)2 * B * H * sizeof(float), s));
    LstmBwdParams lb{};
    lb.w_hh_t = w.w_hh_t; lb.gates = sv.gates; lb.c_all = sv.c_all; lb.dout = w.dlstm; lb.dgates = w.dgates; lb.dc = w.dc;
    lb.B = B; lb.T = T; lb.H = H;
    for (int step = 0; step < T; ++step) {
        lb.step = step;
        HIP_TRY(launch_lstm_bwd_step(lb, s));
    }
    for (int d = 0; d < 2; ++d) {
        const float* dg = w.dgates + (size_t)d * 4 * H;
        if (gr->b_ih[d] || gr->b_hh[d])  // db_ih = db_hh = sum dgates: one sum, written twice
            TRY(colsum(dg, BT, 4 * H, 8 * H, w.colpart, gr->b_ih[d] ? gr->b_ih[d] : gr->b_hh[d], gr->b_ih[d] ? gr->b_hh[d] : nullptr, s));
        if (gr->w_ih[d]) TRY(conv_dw(ConvW{nullptr, 4 * H, D, 1, 1, 0}, dg, lg, sv.y[2], lc, gr->w_ih[d], B, T, w.part, w.part_floats, s));
        // dW_hh = sum_t dgates_t^T h at the step before t: one tap at t - 1 forward (pad 1), t + 1 backward (pad -1); the zero fill is h_0 = 0
        if (gr->w_hh[d]) TRY(conv_dw(ConvW{nullptr, 4 * H, H, 1, 1, d ? -1 : 1}, dg, lg, sv.h + (size_t)d * H, lh, gr->w_hh[d], B, T, w.part, w.part_floats, s));
    }
    {   // dy_2 (B, conv_dim, T) = W_ih^T dgates + W_ih_reverse^T dgates_reverse: two taps without a shift.  (A raw struct: two weights
        // and a per-tap column offset into X are no conv, and nobody else wants them.)
        TapGemmParams g{};
        g.ntaps = 2;
        g.A[0] = wt->w_ih[0]; g.A[1] = wt->w_ih[1];
        g.x_off[1] = 4 * H;
        g.a_sm = 1; g.a_sk = D;
        g.X = w.dgates; g.x_sz = lg.sz; g.x_sk = lg.sc; g.x_sn = lg.st;
        g.C = w.da; g.c_sz = lc.sz; g.c_sm = lc.sc; g.c_sn = lc.st;
        g.M = D; g.N = T; g.K = 4 * H;
        HIP_TRY(launch_tap_gemm(g, B, s));
    }
    // ---- the conv blocks, last to first: BatchNorm + ReLU backward, conv weight gradient, conv data gradient -----
    for (int i = 2; i >= 0; --i) {
        const int cin = i ? D : F;
        BnBwdParams bb{};
        bb.dy = w.da; bb.x = sv.r[i]; bb.dx = w.db;
        bb.gamma = wt->bn_weight[i]; bb.mean = sv.mean[i]; bb.invstd = sv.invstd[i];
        bb.dgamma = gr->bn_weight[i]; bb.dbeta = gr->bn_bias[i];
        bb.B = B; bb.C = D; bb.T = T;
        HIP_TRY(launch_bn_relu_bwd(bb, s));
        const ConvW cw{wt->conv_w[i], D, cin, 5, 1, 2};
        if (gr->conv_w[i]) TRY(conv_dw(cw, w.db, lc, i ? sv.y[i - 1] : mel, i ? lc : chan_last(T, F), gr->conv_w[i], B, T, w.part, w.part_floats, s));
        if (i == 0) break;  // mel gets no gradient
        TRY(conv_dx(cw, w.db, lc, w.da, lc, B, T, Epi(), s));
    }
    return PARROT_OK;
}

// ---------------------------------------------------------------------------------------------
// Debug entry points (include/parrot_hip_debug.h): the kernels above on caller-owned buffers, through wgrad_taps() / the launch_*
// helpers; the descriptors mirror the kernels' own parameter structs, so they are filled field by field.  Nothing is launched before every index the descriptor can reach has been bounded on the host.
// ---------------------------------------------------------------------------------------------
namespace {

static_assert(PARROT_DEBUG_MAX_TAPS == ALIGNER_TAPS && ALIGNER_TAPS <= TG_MAX_TAPS, "the debug descriptors hold one slot per tap");

// smallest and largest element index of sum_i idx_i stride_i + offset, idx_i in [lo_i, hi_i]
struct Reach {
    __int128 lo = 0, hi = 0;
    Reach& off(long o) { lo += o; hi += o; return *this; }
    Reach& dim(long first, long last, long stride) {
        const __int128 a = (__int128)first * stride, b = (__int128)last * stride;
        lo += a < b ? a : b;
        hi += a < b ? b : a;
        return *this;
    }
    Reach& dim(long n, long stride) { return dim(0, n - 1, stride); }
};
int reach_ok(const Reach& r, const parrot_debug_buf& b, const std::string& who, const char* name) {
    if (!b.p || b.n < 1) return fail(PARROT_E_INVALID, who + ": " + name + " is null or empty");
    if (r.lo < 0) return fail(PARROT_E_INVALID, who + ": the strides reach below element 0 of " + name);
    if (r.hi >= b.n) return fail(PARROT_E_INVALID, who + ": the strides reach beyond the " + std::to_string(b.n) + " elements of " + name);
    return PARROT_OK;
}
// what a launcher refused before launching anything is a limit of the kernels, not a fault of the device
int launched(hipError_t e, const std::string& who) {
    if (e == hipErrorInvalidValue) return fail(PARROT_E_UNSUPPORTED, who + ": beyond the launcher's limits (taps, grid size)");
    if (e != hipSuccess) return fail(PARROT_E_HIP, who + ": " + hipGetErrorString(e));
    return PARROT_OK;
}
bool wgrad_sizes_ok(long R, long ntaps, long M, long K) { return R >= 1 && ntaps >= 1 && ntaps <= PARROT_DEBUG_MAX_TAPS && M >= 1 && K >= 1; }

}  // namespace

extern "C" int parrot_debug_tap_gemm(const parrot_debug_tap_gemm_desc* d, void* stream) {
    const std::string who = "debug_tap_gemm";
    if (!d) return fail(PARROT_E_INVALID, who + ": null argument");
    if (d->ntaps < 1 || d->M < 1 || d->N < 1 || d->K < 1 || d->Z < 1) return fail(PARROT_E_INVALID, who + ": ntaps, M, N, K and Z must be positive");
    if (d->ntaps > PARROT_DEBUG_MAX_TAPS) return fail(PARROT_E_UNSUPPORTED, who + ": more than 5 taps");
    if (d->bias1.p && !d->bias0.p) return fail(PARROT_E_INVALID, who + ": bias1 without bias0");
    for (int j = 0; j < d->ntaps; ++j) {
        TRY(reach_ok(Reach().dim(d->M, d->a_sm).dim(d->K, d->a_sk), d->A[j], who, "A"));
        const long lo = std::max<long>(0, d->shift[j]), hi = std::min<long>(d->N - 1, (long)d->N - 1 + d->shift[j]);  // the columns of X tap j reads
        if (!d->X.p || d->X.n < 1) return fail(PARROT_E_INVALID, who + ": X is null or empty");
        if (lo <= hi) TRY(reach_ok(Reach().off(d->x_off[j]).dim(d->Z, d->x_sz).dim(d->K, d->x_sk).dim(lo, hi, d->x_sn), d->X, who, "X"));
    }
    TRY(reach_ok(Reach().dim(d->Z, d->c_sz).dim(d->M, d->c_sm).dim(d->N, d->c_sn), d->C, who, "C"));
    if (d->bias0.p) TRY(reach_ok(Reach().dim(d->M, 1), d->bias0, who, "bias0"));
    if (d->bias1.p) TRY(reach_ok(Reach().dim(d->M, 1), d->bias1, who, "bias1"));
    TapGemmParams g{};
    g.X = d->X.p; g.x_sz = d->x_sz; g.x_sk = d->x_sk; g.x_sn = d->x_sn;
    g.C = d->C.p; g.c_sz = d->c_sz; g.c_sm = d->c_sm; g.c_sn = d->c_sn;
    g.a_sm = d->a_sm; g.a_sk = d->a_sk;
    g.M = d->M; g.N = d->N; g.K = d->K;
    g.ntaps = d->ntaps;
    for (int j = 0; j < d->ntaps; ++j) {
        g.A[j] = d->A[j].p;
        g.x_off[j] = d->x_off[j];
        g.shift[j] = d->shift[j];
    }
    g.bias0 = d->bias0.p;
    g.bias1 = d->bias1.p;
    g.relu = d->relu ? 1 : 0;
    return launched(launch_tap_gemm(g, d->Z, (hipStream_t)stream), who);
}

extern "C" size_t parrot_debug_wgrad_workspace_bytes(int32_t R, int32_t ntaps, int32_t M, int32_t K) {
    return wgrad_sizes_ok(R, ntaps, M, K) ? (size_t)wgrad_chunks(R) * ntaps * M * K * sizeof(float) : 0;
}
extern "C" int parrot_debug_wgrad(const parrot_debug_wgrad_desc* d, void* ws, size_t ws_bytes, void* stream) {
    const std::string who = "debug_wgrad";
    if (!d || !ws) return fail(PARROT_E_INVALID, who + ": null argument");
    if (d->ntaps < 1 || d->M < 1 || d->K < 1 || d->T < 1 || d->R < 1) return fail(PARROT_E_INVALID, who + ": ntaps, M, K, T and R must be positive");
    if (d->ntaps > PARROT_DEBUG_MAX_TAPS) return fail(PARROT_E_UNSUPPORTED, who + ": more than 5 taps");
    if (d->R % d->T) return fail(PARROT_E_INVALID, who + ": R must be a multiple of T");
    const int B = d->R / d->T;
    TRY(reach_ok(Reach().dim(B, d->y_sz).dim(d->M, d->y_sm).dim(d->T, d->y_st), d->dY, who, "dY"));
    if (!d->X.p || d->X.n < 1) return fail(PARROT_E_INVALID, who + ": X is null or empty");
    for (int j = 0; j < d->ntaps; ++j) {
        const long lo = std::max<long>(0, d->shift[j]), hi = std::min<long>(d->T - 1, (long)d->T - 1 + d->shift[j]);  // the frames of X tap j reads
        if (lo <= hi) TRY(reach_ok(Reach().dim(B, d->x_sz).dim(d->K, d->x_sk).dim(lo, hi, d->x_st), d->X, who, "X"));
    }
    TRY(reach_ok(Reach().dim(d->M, d->o_sm).dim(d->K, d->o_sk).dim(d->ntaps, d->o_sj), d->out, who, "out"));
    if (ws_bytes < parrot_debug_wgrad_workspace_bytes(d->R, d->ntaps, d->M, d->K)) return fail(PARROT_E_INVALID, who + ": workspace too small");
    if ((long)wgrad_chunks(d->R) * d->ntaps > 65535 || (d->M + 63) / 64 > 65535)  // (launch_wgrad's own limits, before the workspace is touched)
        return fail(PARROT_E_UNSUPPORTED, who + ": beyond the launcher's limits (taps, grid size)");
    hipStream_t s = (hipStream_t)stream;
    if (poison_word()) TRY(poison(ws, parrot_debug_wgrad_workspace_bytes(d->R, d->ntaps, d->M, d->K), s));
    WgradParams q{};
    q.dY = d->dY.p; q.y_sz = d->y_sz; q.y_sm = d->y_sm; q.y_st = d->y_st;
    q.X = d->X.p; q.x_sz = d->x_sz; q.x_sk = d->x_sk; q.x_st = d->x_st;
    q.M = d->M; q.K = d->K; q.T = d->T; q.R = d->R;
    return wgrad_taps(q, d->shift, d->ntaps, d->out.p, d->o_sm, d->o_sk, d->o_sj, (float*)ws, ws_bytes / sizeof(float), s);  // (one group: checked above)
}

extern "C" size_t parrot_debug_colsum_workspace_bytes(int32_t R, int32_t M) {
    return R >= 1 && M >= 1 ? (size_t)wgrad_chunks(R) * M * sizeof(double) : 0;
}
extern "C" int parrot_debug_colsum(const parrot_debug_colsum_desc* d, void* ws, size_t ws_bytes, void* stream) {
    const std::string who = "debug_colsum";
    if (!d || !ws) return fail(PARROT_E_INVALID, who + ": null argument");
    if (d->R < 1 || d->M < 1) return fail(PARROT_E_INVALID, who + ": R and M must be positive");
    TRY(reach_ok(Reach().dim(d->R, d->ld).dim(d->M, 1), d->src, who, "src"));
    TRY(reach_ok(Reach().dim(d->M, 1), d->out0, who, "out0"));
    if (d->out1.p) TRY(reach_ok(Reach().dim(d->M, 1), d->out1, who, "out1"));
    const size_t need = parrot_debug_colsum_workspace_bytes(d->R, d->M);
    if (ws_bytes < need) return fail(PARROT_E_INVALID, who + ": workspace too small");
    if (wgrad_chunks(d->R) > 65535)  // (launch_colsum's own limit, before the workspace is touched)
        return fail(PARROT_E_UNSUPPORTED, who + ": beyond the launcher's limits (grid size)");
    hipStream_t s = (hipStream_t)stream;
    if (poison_word()) TRY(poison(ws, need, s));
    return launched(launch_colsum(d->src.p, d->R, d->M, d->ld, (double*)ws, d->out0.p, d->out1.p, s), who);
}

extern "C" int parrot_debug_bn_train(const parrot_debug_bn_train_desc* d, void* stream) {
    const std::string who = "debug_bn_train";
    if (!d) return fail(PARROT_E_INVALID, who + ": null argument");
    if (d->B < 1 || d->C < 1 || d->T < 1) return fail(PARROT_E_INVALID, who + ": B, C and T must be positive");
    if (d->training && (long)d->B * d->T < 2) return fail(PARROT_E_INVALID, who + ": Expected more than 1 value per channel when training");
    const Reach all = Reach().dim(d->B, (long)d->C * d->T).dim(d->C, d->T).dim(d->T, 1), chan = Reach().dim(d->C, 1);
    TRY(reach_ok(all, d->x, who, "x"));
    TRY(reach_ok(all, d->y, who, "y"));
    TRY(reach_ok(chan, d->gamma, who, "gamma"));
    TRY(reach_ok(chan, d->beta, who, "beta"));
    TRY(reach_ok(chan, d->run_mean, who, "run_mean"));
    TRY(reach_ok(chan, d->run_var, who, "run_var"));
    TRY(reach_ok(chan, d->mean, who, "mean"));
    TRY(reach_ok(chan, d->invstd, who, "invstd"));
    BnTrainParams bn{};
    bn.x = d->x.p; bn.y = d->y.p;
    bn.gamma = d->gamma.p; bn.beta = d->beta.p;
    bn.run_mean = d->run_mean.p; bn.run_var = d->run_var.p;
    bn.mean = d->mean.p; bn.invstd = d->invstd.p;
    bn.B = d->B; bn.C = d->C; bn.T = d->T; bn.training = d->training ? 1 : 0;
    bn.eps = d->eps;
    return launched(launch_bn_train(bn, (hipStream_t)stream), who);
}

extern "C" int parrot_debug_bn_relu_bwd(const parrot_debug_bn_bwd_desc* d, void* stream) {
    const std::string who = "debug_bn_relu_bwd";
    if (!d) return fail(PARROT_E_INVALID, who + ": null argument");
    if (d->B < 1 || d->C < 1 || d->T < 1) return fail(PARROT_E_INVALID, who + ": B, C and T must be positive");
    const Reach all = Reach().dim(d->B, (long)d->C * d->T).dim(d->C, d->T).dim(d->T, 1), chan = Reach().dim(d->C, 1);
    TRY(reach_ok(all, d->dy, who, "dy"));
    TRY(reach_ok(all, d->x, who, "x"));
    TRY(reach_ok(all, d->dx, who, "dx"));
    TRY(reach_ok(chan, d->gamma, who, "gamma"));
    TRY(reach_ok(chan, d->mean, who, "mean"));
    TRY(reach_ok(chan, d->invstd, who, "invstd"));
    if (d->dgamma.p) TRY(reach_ok(chan, d->dgamma, who, "dgamma"));
    if (d->dbeta.p) TRY(reach_ok(chan, d->dbeta, who, "dbeta"));
    BnBwdParams bb{};
    bb.dy = d->dy.p; bb.x = d->x.p; bb.dx = d->dx.p;
    bb.gamma = d->gamma.p; bb.mean = d->mean.p; bb.invstd = d->invstd.p;
    bb.dgamma = d->dgamma.p; bb.dbeta = d->dbeta.p;
    bb.B = d->B; bb.C = d->C; bb.T = d->T;
    return launched(launch_bn_relu_bwd(bb, (hipStream_t)stream), who);
}

// parrot_debug_lstm: the recurrence alone, through lstm_run_steps (kernel 0, host_aligner.hip) or lstm_train_run_steps (kernel 1):
// the loops parrot_aligner_forward and parrot_aligner_train_forward run.  Workspace: the h double buffer and c.
namespace {
struct LstmDebugScratch {
    float *hbuf, *cbuf;  // [2][2][B][H], [2][B][H]
};
LstmDebugScratch lstm_debug_scratch(Arena& ar, int B, int H) {
    LstmDebugScratch w{};
    w.hbuf = ar.take<float>((size_t)2 * 2 * B * H);
    w.cbuf = ar.take<float>((size_t)2 * B * H);
    return w;
}
bool lstm_debug_sizes_ok(int B, int T, int H, int kernel) {
    return B >= 1 && B <= 65535 && T >= 1 && T <= ALIGN_MAX_T && H >= 1 && H % 16 == 0 && H <= LSTM_MAX_DIM && (kernel == 0 || kernel == 1);
}
}  // namespace

extern "C" size_t parrot_debug_lstm_workspace_bytes(int32_t B, int32_t T, int32_t H, int32_t kernel) {
    if (!lstm_debug_sizes_ok(B, T, H, kernel)) return 0;
    Arena ar(nullptr, 0);
    (void)lstm_debug_scratch(ar, B, H);
    return align_up(ar.off, 256);
}
extern "C" int parrot_debug_lstm(const float* w_hh, const float* xproj, const float* h0, const float* c0, int32_t B, int32_t T, int32_t H,
                                 int32_t n_steps, int32_t kernel, float* out, float* h_n, float* c_n, float* gates, float* c_all, void* ws,
                                 size_t ws_bytes, void* stream) {
    const std::string who = "debug_lstm";
    if (!w_hh || !xproj || !out || !h_n || !c_n || !ws) return fail(PARROT_E_INVALID, who + ": null argument");
    if ((h0 == nullptr) != (c0 == nullptr)) return fail(PARROT_E_INVALID, who + ": h0 and c0 are given together or not at all");
    if (kernel != 0 && kernel != 1) return fail(PARROT_E_INVALID, who + ": kernel must be 0 (lstm_step_kernel) or 1 (lstm_train_step_kernel)");
    if (kernel == 1 && (!gates || !c_all)) return fail(PARROT_E_INVALID, who + ": kernel 1 writes gates and c_all");
    if (kernel == 0 && (gates || c_all)) return fail(PARROT_E_INVALID, who + ": kernel 0 keeps no gates or c_all: pass NULL");
    if (B < 1 || T < 1 || H < 1) return fail(PARROT_E_INVALID, who + ": B, T and H must be positive");
    if (n_steps < 1 || n_steps > T) return fail(PARROT_E_INVALID, who + ": n_steps outside [1, T]");
    if (H % 16) return fail(PARROT_E_UNSUPPORTED, who + ": H must be a multiple of 16");
    if (H > LSTM_MAX_DIM) return fail(PARROT_E_UNSUPPORTED, who + ": H > 1024");
    if (B > 65535) return fail(PARROT_E_UNSUPPORTED, who + ": B > 65535");
    if (T > ALIGN_MAX_T) return fail(PARROT_E_UNSUPPORTED, who + ": T > 32768 frames");
    Arena ar(ws, ws_bytes);
    const LstmDebugScratch w = lstm_debug_scratch(ar, B, H);
    if (!ar.ok) return fail(PARROT_E_UNSUPPORTED, who + ": workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const size_t hn = (size_t)2 * B * H;
    if (poison_word()) {  // (out, gates and c_all keep what the caller gave them outside the steps' own frames)
        TRY(poison(ws, ws_bytes, s));
        TRY(poison(h_n, hn * sizeof(float), s));
        TRY(poison(c_n, hn * sizeof(float), s));
    }
    if (kernel == 0) {
        LstmStepParams q{};
        q.w_hh = w_hh; q.xproj = xproj; q.c = w.cbuf; q.out = out;
        q.B = B; q.T = T; q.H = H;
        TRY(lstm_run_steps(q, w.hbuf, h0, c0, n_steps, s));
    } else {
        LstmTrainParams q{};
        q.w_hh[0] = w_hh; q.w_hh[1] = w_hh + (size_t)4 * H * H;
        q.xproj = xproj; q.c = w.cbuf; q.out = out; q.gates = gates; q.c_all = c_all;
        q.B = B; q.T = T; q.H = H;
        TRY(lstm_train_run_steps(q, w.hbuf, h0, c0, n_steps, s));
    }
    HIP_TRY(hipMemcpyAsync(h_n, w.hbuf + (size_t)(n_steps & 1) * hn, hn * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(c_n, w.cbuf, hn * sizeof(float), hipMemcpyDeviceToDevice, s));
    return PARROT_OK;
}
