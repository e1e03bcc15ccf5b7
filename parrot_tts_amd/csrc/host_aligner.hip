// host_aligner.hip -- the forced-aligner handle (kernels and launchers: aligner.h / tu_aligner.hip).
#include "host_common.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "aligner.h"
#include "ctc.h"
#include "weight_pack.h"

using namespace parrot;

// ---------------------------------------------------------------------------------------------
// Forced aligner (reference utils/aligner/model.py:24-48, extract_durations.py:86-96, duration_extraction.py:52-85): the five
// GEMMs as parrot_conv plans owned by the handle, everything else in aligner.h.
// ---------------------------------------------------------------------------------------------
struct AlignPlan {
    std::unique_ptr<parrot_conv> conv;
    int C = 0, G = 1, Mg = 0, relu = 0;      // real output channels; channel groups of the plan and rows per group
    float *scale = nullptr, *shift = nullptr;  // BatchNorm affine (scale, shift) or bias (shift only)
    ~AlignPlan() {
        if (scale) (void)hipFree(scale);
        if (shift) (void)hipFree(shift);
    }
};
struct parrot_aligner {
    parrot_aligner_cfg cfg{};
    int scheme = PARROT_PREC_F16X3;
    AlignPlan plan[5];  // conv 0..2, LSTM input projection (both directions), lin
    float* w_hh = nullptr;
    DevFlag err;
    float *dbg_bn3 = nullptr, *dbg_lstm = nullptr;  // parrot_aligner_debug_stages (tests only)
    ~parrot_aligner() {
        if (w_hh) (void)hipFree(w_hh);
    }
};

// One plan: y = affine(relu?(W x)).  PARROT_PREC_F32 runs the plan as a GROUPED conv (chain_groups, weight_pack.h) -- group g sums the
// g-th G-th of the input channels into its own rows -- and align_epilogue_kernel adds the G partials before the ReLU.
static int align_plan(AlignPlan& p, int scheme, int cin, int cout, int k, const float* w, const float* scale, const float* shift, int relu) {
    const ChainGroups cgr = chain_groups(scheme, cin, cout);
    const int G = cgr.G, Mg = cgr.Mg, cg = cin / G;
    p.C = cout;
    p.G = G;
    p.Mg = Mg;
    p.relu = relu;
    if (G > 1) {
        std::vector<float> W((size_t)G * Mg * cg * k, 0.f);  // (G Mg, c_in / G, k): torch's grouped layout
        for (int g = 0; g < G; ++g)
            for (int o = 0; o < cout; ++o)
                memcpy(&W[((size_t)g * Mg + o) * cg * k], &w[((size_t)o * cin + (size_t)g * cg) * k], (size_t)cg * k * sizeof(float));
        TRY(make_conv(p.conv, cin, G * Mg, k, 1, k / 2, 0, 1, PRE_NONE, 0.f, ACT_NONE, W.data(), nullptr, G));
    } else {
        TRY(make_conv(p.conv, cin, cout, k, 1, k / 2, 0, 1, PRE_NONE, 0.f, ACT_NONE, w, nullptr));
    }
    if (scale) TRY(upload(&p.scale, scale, (size_t)cout));
    if (shift) TRY(upload(&p.shift, shift, (size_t)cout));
    return PARROT_OK;
}

static int aligner_create(parrot_aligner_t** out, const parrot_aligner_cfg* cfg, const parrot_aligner_weights* w, int prec) {
    if (!out || !cfg || !w) return fail(PARROT_E_INVALID, "aligner_create: null argument");
    const int n_mels = cfg->n_mels, V = cfg->num_symbols, H = cfg->lstm_dim, D = cfg->conv_dim;
    if (n_mels < 1 || V < 1 || H < 1 || D < 1) return fail(PARROT_E_INVALID, "aligner_create: dimensions must be positive");
    if (H % 16 || D % 16) return fail(PARROT_E_UNSUPPORTED, "aligner_create: conv_dim and lstm_dim must be multiples of 16");
    if (H > LSTM_MAX_DIM) return fail(PARROT_E_UNSUPPORTED, "aligner_create: lstm_dim > 1024");
    if (!w->lin_w || !w->lin_b) return fail(PARROT_E_INVALID, "aligner_create: null weight");
    for (int i = 0; i < 3; ++i)
        if (!w->conv_w[i] || !w->bn_weight[i] || !w->bn_bias[i] || !w->bn_mean[i] || !w->bn_var[i]) return fail(PARROT_E_INVALID, "aligner_create: null weight");
    for (int d = 0; d < 2; ++d)
        if (!w->w_ih[d] || !w->w_hh[d] || !w->b_ih[d] || !w->b_hh[d]) return fail(PARROT_E_INVALID, "aligner_create: null weight");
    int scheme;  // (as the mel handle: durations do not move with the operating point)
    TRY(resolve_parity_prec(prec, "aligner_create", &scheme));
    CreateScope scope(scheme, -1, -1);
    query_device();
    std::unique_ptr<parrot_aligner> a(new parrot_aligner());
    a->cfg = *cfg;
    a->scheme = scheme;
    for (int i = 0; i < 3; ++i) {  // eval-mode BatchNorm1d after the ReLU (model.py:16-19) as scale / shift, formed in fp64, rounded once
        std::vector<float> sc((size_t)D), sh((size_t)D);
        for (int c = 0; c < D; ++c) {
            const double s = (double)w->bn_weight[i][c] / std::sqrt((double)w->bn_var[i][c] + (double)cfg->bn_eps);
            sc[c] = (float)s;
            sh[c] = (float)((double)w->bn_bias[i][c] - (double)w->bn_mean[i][c] * s);
        }
        TRY(align_plan(a->plan[i], scheme, i ? D : n_mels, D, 5, w->conv_w[i], sc.data(), sh.data(), 1));
    }
    {   // W_ih of both directions as one 1x1 plan conv_dim -> 8 lstm_dim, bias b_ih + b_hh (fp32 sum)
        std::vector<float> W((size_t)8 * H * D), bsum((size_t)8 * H);
        for (int d = 0; d < 2; ++d) {
            memcpy(&W[(size_t)d * 4 * H * D], w->w_ih[d], (size_t)4 * H * D * sizeof(float));
            for (int r = 0; r < 4 * H; ++r) bsum[(size_t)d * 4 * H + r] = w->b_ih[d][r] + w->b_hh[d][r];
        }
        TRY(align_plan(a->plan[3], scheme, D, 8 * H, 1, W.data(), nullptr, bsum.data(), 0));
    }
    TRY(align_plan(a->plan[4], scheme, 2 * H, V, 1, w->lin_w, nullptr, w->lin_b, 0));
    HIP_TRY(hipMalloc((void**)&a->w_hh, (size_t)2 * 4 * H * H * sizeof(float)));
    for (int d = 0; d < 2; ++d)
        HIP_TRY(hipMemcpy(a->w_hh + (size_t)d * 4 * H * H, w->w_hh[d], (size_t)4 * H * H * sizeof(float), hipMemcpyHostToDevice));
    TRY(a->err.init());
    *out = a.release();
    return PARROT_OK;
}
extern "C" int parrot_aligner_create(parrot_aligner_t** out, const parrot_aligner_cfg* cfg, const parrot_aligner_weights* w) {
    return aligner_create(out, cfg, w, -1);
}
extern "C" int parrot_aligner_create_ex(parrot_aligner_t** out, const parrot_aligner_cfg* cfg, const parrot_aligner_weights* w, int32_t precision) {
    return aligner_create(out, cfg, w, precision);
}
extern "C" void parrot_aligner_destroy(parrot_aligner_t* a) { delete a; }
extern "C" int parrot_aligner_precision(const parrot_aligner_t* a) { return a ? a->scheme : PARROT_E_INVALID; }
extern "C" int parrot_aligner_debug_stages(parrot_aligner_t* a, float* bn3_dev, float* lstm_dev) {
    if (!a) return fail(PARROT_E_INVALID, "aligner_debug_stages: null handle");
    a->dbg_bn3 = bn3_dev;
    a->dbg_lstm = lstm_dev;
    return PARROT_OK;
}

struct AlignScratch {
    float *x0, *a, *b, *part, *xp_cf, *xp, *lstm, *lstm_cf, *logits_cf, *h, *c;
};
static AlignScratch align_scratch(const parrot_aligner* al, Arena& ar, int B, int T) {
    const size_t BT = (size_t)B * T, H = (size_t)al->cfg.lstm_dim, D = (size_t)al->cfg.conv_dim;
    size_t part = 0;
    for (const AlignPlan& p : al->plan) part = std::max(part, (size_t)p.G * p.Mg);
    AlignScratch w{};
    w.x0 = ar.take<float>(BT * al->cfg.n_mels);
    w.a = ar.take<float>(BT * D);
    w.b = ar.take<float>(BT * D);
    w.part = ar.take<float>(BT * part);
    w.xp_cf = ar.take<float>(BT * 8 * H);
    w.xp = ar.take<float>(BT * 8 * H);
    w.lstm = ar.take<float>(BT * 2 * H);
    w.lstm_cf = ar.take<float>(BT * 2 * H);
    w.logits_cf = ar.take<float>(BT * al->cfg.num_symbols);
    w.h = ar.take<float>((size_t)2 * 2 * B * H);
    w.c = ar.take<float>((size_t)2 * B * H);
    return w;
}
static int align_shape_ok(int B, int T, const char* who) {
    if (B <= 0 || B > 65535 || T <= 0) return fail(PARROT_E_INVALID, std::string(who) + ": need 1 <= B <= 65535 and T >= 1");
    if (T > ALIGN_MAX_T) return fail(PARROT_E_UNSUPPORTED, std::string(who) + ": T > 32768 frames");
    return PARROT_OK;
}
extern "C" size_t parrot_aligner_workspace_bytes(const parrot_aligner_t* al, int32_t B, int32_t T) {
    if (!al || B <= 0 || B > 65535 || T <= 0 || T > ALIGN_MAX_T) return 0;
    Arena ar(nullptr, 0);
    (void)align_scratch(al, ar, B, T);
    return align_up(ar.off, 256);
}
static int align_run_plan(const AlignPlan& p, const float* x, float* part, float* y, int B, int T, hipStream_t s) {
    TRY(conv_launch(p.conv.get(), x, nullptr, part, B, T, EPI_STORE, 1.f, s));
    HIP_TRY(launch_align_epilogue(part, y, p.scale, p.shift, B, p.C, T, p.G, p.Mg, p.relu, s));
    return PARROT_OK;
}
// The recurrence as the forward runs it: the initial state into half 0 of the h double buffer hbuf [2][2][B][H] and into q.c (zeros
// when h0 / c0 are null, else device copies), then one launch per step, each reading the half the step before wrote.  Afterwards h
// of the last step is half n_steps & 1 of hbuf and c is q.c.  Also behind parrot_debug_lstm (host_aligner_train.hip).
int parrot::lstm_run_steps(LstmStepParams q, float* hbuf, const float* h0, const float* c0, int n_steps, hipStream_t s) {
    const size_t hn = (size_t)2 * q.B * q.H;
    if (h0) HIP_TRY(hipMemcpyAsync(hbuf, h0, hn * sizeof(float), hipMemcpyDeviceToDevice, s));
    else HIP_TRY(hipMemsetAsync(hbuf, 0, hn * sizeof(float), s));
    if (c0) HIP_TRY(hipMemcpyAsync(q.c, c0, hn * sizeof(float), hipMemcpyDeviceToDevice, s));
    else HIP_TRY(hipMemsetAsync(q.c, 0, hn * sizeof(float), s));
    for (int step = 0; step < n_steps; ++step) {
        q.step = step;
        q.h_prev = hbuf + (size_t)(step & 1) * hn;
        q.h_next = hbuf + (size_t)((step + 1) & 1) * hn;
        HIP_TRY(launch_lstm_step(q, s));
    }
    return PARROT_OK;
}
extern "C" int parrot_aligner_forward(parrot_aligner_t* al, const float* mel, int32_t B, int32_t T, float* logits, void* ws, size_t ws_bytes,
                                      void* stream) {
    if (!al || !mel || !logits || !ws) return fail(PARROT_E_INVALID, "aligner_forward: null argument");
    TRY(align_shape_ok(B, T, "aligner_forward"));
    hipStream_t s = (hipStream_t)stream;
    const int H = al->cfg.lstm_dim, D = al->cfg.conv_dim, V = al->cfg.num_symbols, n_mels = al->cfg.n_mels;
    Arena ar(ws, ws_bytes);
    const AlignScratch w = align_scratch(al, ar, B, T);
    if (!ar.ok) return fail(PARROT_E_NOMEM, "aligner_forward: workspace too small");
    if (poison_word()) {
        TRY(poison(ws, ws_bytes, s));
        TRY(poison(logits, (size_t)B * T * V * sizeof(float), s));
    }
    // the padded batch as it stands (dataset.py:66-75, model.py:41-48): no row lengths before the softmax
    HIP_TRY(launch_align_transpose(mel, w.x0, B, T, n_mels, s));
    TRY(align_run_plan(al->plan[0], w.x0, w.part, w.a, B, T, s));
    TRY(align_run_plan(al->plan[1], w.a, w.part, w.b, B, T, s));
    TRY(align_run_plan(al->plan[2], w.b, w.part, w.a, B, T, s));
    if (al->dbg_bn3) HIP_TRY(hipMemcpyAsync(al->dbg_bn3, w.a, (size_t)B * D * T * sizeof(float), hipMemcpyDeviceToDevice, s));
    TRY(align_run_plan(al->plan[3], w.a, w.part, w.xp_cf, B, T, s));
    HIP_TRY(launch_align_transpose(w.xp_cf, w.xp, B, 8 * H, T, s));
    LstmStepParams q{};
    q.w_hh = al->w_hh; q.xproj = w.xp; q.c = w.c; q.out = w.lstm;
    q.B = B; q.T = T; q.H = H;
    TRY(lstm_run_steps(q, w.h, nullptr, nullptr, T, s));  // h_0 = c_0 = 0 (nn.LSTM without an initial state)
    if (al->dbg_lstm) HIP_TRY(hipMemcpyAsync(al->dbg_lstm, w.lstm, (size_t)B * T * 2 * H * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIP_TRY(launch_align_transpose(w.lstm, w.lstm_cf, B, T, 2 * H, s));
    TRY(align_run_plan(al->plan[4], w.lstm_cf, w.part, w.logits_cf, B, T, s));
    HIP_TRY(launch_align_transpose(w.logits_cf, logits, B, V, T, s));
    return PARROT_OK;
}
extern "C" int parrot_align_softmax(parrot_aligner_t* al, const float* logits, const int32_t* mel_len, int32_t B, int32_t T, float* pred,
                                    void* stream) {
    if (!al || !logits || !pred) return fail(PARROT_E_INVALID, "align_softmax: null argument");
    TRY(align_shape_ok(B, T, "align_softmax"));
    hipStream_t s = (hipStream_t)stream;
    if (poison_word() && pred != logits) TRY(poison(pred, (size_t)B * T * al->cfg.num_symbols * sizeof(float), s));
    HIP_TRY(launch_align_softmax(logits, mel_len, pred, B, T, al->cfg.num_symbols, al->err, s));
    return PARROT_OK;
}
extern "C" size_t parrot_align_workspace_bytes(int32_t B, int32_t T, int32_t N) {
    if (B <= 0 || B > 65535 || T <= 0 || T > ALIGN_MAX_T || N <= 0 || N > ALIGN_MAX_N) return 0;
    return 256 + align_up((size_t)B * T * N, 256);  // the status word, then one back-pointer byte per cell
}
extern "C" int parrot_align_durations(const float* pred, const int64_t* tokens, const int32_t* mel_len, const int32_t* tokens_len, int32_t B,
                                      int32_t T, int32_t V, int32_t N, int32_t* dur_out, double* cost_out, void* ws, size_t ws_bytes, void* stream) {
    if (!pred || !tokens || !mel_len || !tokens_len || !dur_out || !cost_out || !ws) return fail(PARROT_E_INVALID, "align_durations: null argument");
    if (B <= 0 || B > 65535 || T <= 0 || N <= 0 || V <= 0) return fail(PARROT_E_INVALID, "align_durations: need 1 <= B <= 65535 and T, N, V >= 1");
    if (T > ALIGN_MAX_T || N > ALIGN_MAX_N) return fail(PARROT_E_UNSUPPORTED, "align_durations: at most 32768 frames and 2048 tokens per utterance");
    if (ws_bytes < parrot_align_workspace_bytes(B, T, N)) return fail(PARROT_E_NOMEM, "align_durations: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    if (poison_word()) {
        TRY(poison(ws, ws_bytes, s));
        TRY(poison(dur_out, (size_t)B * N * sizeof(int32_t), s));
        TRY(poison(cost_out, (size_t)B * sizeof(double), s));
    }
    HIP_TRY(hipMemsetAsync(ws, 0, sizeof(int), s));
    HIP_TRY(launch_align_dp(pred, tokens, mel_len, tokens_len, B, T, V, N, (uint8_t*)ws + 256, dur_out, cost_out, (int*)ws, s));
    return PARROT_OK;
}
extern "C" size_t parrot_ctc_workspace_bytes(int32_t B, int32_t T, int32_t N) {
    if (B <= 0 || B > 65535 || T <= 0 || T > ALIGN_MAX_T || N <= 0 || N > ALIGN_MAX_N) return 0;
    return 256 + align_up((size_t)B * T * sizeof(double), 256);  // the status word, then lse (B, T) fp64
}
extern "C" int parrot_ctc_loss(const float* logits, const int64_t* tokens, const int32_t* mel_len, const int32_t* tokens_len, int32_t B, int32_t T,
                               int32_t V, int32_t N, double* nll_out, float* mean_out, void* ws, size_t ws_bytes, void* stream) {
    if (!logits || !tokens || !mel_len || !tokens_len || !nll_out || !ws) return fail(PARROT_E_INVALID, "ctc_loss: null argument");
    if (B <= 0 || B > 65535 || T <= 0 || N <= 0 || V <= 0) return fail(PARROT_E_INVALID, "ctc_loss: need 1 <= B <= 65535 and T, N, V >= 1");
    if (T > ALIGN_MAX_T || N > ALIGN_MAX_N) return fail(PARROT_E_UNSUPPORTED, "ctc_loss: at most 32768 frames and 2048 tokens per utterance");
    if (ws_bytes < parrot_ctc_workspace_bytes(B, T, N)) return fail(PARROT_E_NOMEM, "ctc_loss: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    if (poison_word()) {
        TRY(poison(ws, ws_bytes, s));
        TRY(poison(nll_out, (size_t)B * sizeof(double), s));
        if (mean_out) TRY(poison(mean_out, sizeof(float), s));
    }
    HIP_TRY(hipMemsetAsync(ws, 0, sizeof(int), s));
    double* lse = (double*)((char*)ws + 256);
    HIP_TRY(launch_ctc_lse(logits, mel_len, lse, B, T, V, (int*)ws, s));
    HIP_TRY(launch_ctc_alpha(logits, tokens, mel_len, tokens_len, lse, B, T, V, N, nll_out, mean_out, nullptr, (int*)ws, s));
    return PARROT_OK;
}
// the gradient's workspace: the status word, lse (B, T) fp64, alpha / log-occupancy (B, T, 2 N + 1) fp64, then the sorted token
// positions (B, N) and each label's segment of them, seg_lo and seg_hi (B, V) int32
struct CtcGradLayout {
    size_t lse, occ, order, seg_lo, seg_hi, total;
};
static CtcGradLayout ctc_grad_layout(int32_t B, int32_t T, int32_t V, int32_t N) {
    CtcGradLayout l{};
    l.lse = 256;
    l.occ = l.lse + align_up((size_t)B * T * sizeof(double), 256);
    l.order = l.occ + align_up((size_t)B * T * ((size_t)2 * N + 1) * sizeof(double), 256);
    l.seg_lo = l.order + align_up((size_t)B * N * sizeof(int32_t), 256);
    l.seg_hi = l.seg_lo + align_up((size_t)B * V * sizeof(int32_t), 256);
    l.total = l.seg_hi + align_up((size_t)B * V * sizeof(int32_t), 256);
    return l;
}
extern "C" size_t parrot_ctc_grad_workspace_bytes(int32_t B, int32_t T, int32_t V, int32_t N) {
    if (B <= 0 || B > 65535 || T <= 0 || T > ALIGN_MAX_T || N <= 0 || N > ALIGN_MAX_N || V <= 0) return 0;
    return ctc_grad_layout(B, T, V, N).total;
}
extern "C" int parrot_ctc_loss_grad(const float* logits, const int64_t* tokens, const int32_t* mel_len, const int32_t* tokens_len, int32_t B,
                                    int32_t T, int32_t V, int32_t N, const double* row_weight, int32_t zero_infinity, double* nll_out,
                                    float* grad_out, void* ws, size_t ws_bytes, void* stream) {
    if (!logits || !tokens || !mel_len || !tokens_len || !nll_out || !grad_out || !ws) return fail(PARROT_E_INVALID, "ctc_loss_grad: null argument");
    if (B <= 0 || B > 65535 || T <= 0 || N <= 0 || V <= 0) return fail(PARROT_E_INVALID, "ctc_loss_grad: need 1 <= B <= 65535 and T, N, V >= 1");
    if (T > ALIGN_MAX_T || N > ALIGN_MAX_N) return fail(PARROT_E_UNSUPPORTED, "ctc_loss_grad: at most 32768 frames and 2048 tokens per utterance");
    const CtcGradLayout l = ctc_grad_layout(B, T, V, N);
    if (ws_bytes < l.total) return fail(PARROT_E_NOMEM, "ctc_loss_grad: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    if (poison_word()) {
        TRY(poison(ws, ws_bytes, s));
        TRY(poison(nll_out, (size_t)B * sizeof(double), s));
        TRY(poison(grad_out, (size_t)B * T * V * sizeof(float), s));
    }
    HIP_TRY(hipMemsetAsync(ws, 0, sizeof(int), s));
    char* base = (char*)ws;
    double* lse = (double*)(base + l.lse);
    CtcGradWs g{(double*)(base + l.occ), (int32_t*)(base + l.order), (int32_t*)(base + l.seg_lo), (int32_t*)(base + l.seg_hi)};
    HIP_TRY(launch_ctc_lse(logits, mel_len, lse, B, T, V, (int*)ws, s));
    HIP_TRY(launch_ctc_alpha(logits, tokens, mel_len, tokens_len, lse, B, T, V, N, nll_out, nullptr, g.occ, (int*)ws, s));
    HIP_TRY(launch_ctc_grad(logits, tokens, mel_len, tokens_len, lse, nll_out, row_weight, zero_infinity ? 1 : 0, B, T, V, N, g, grad_out, s));
    return PARROT_OK;
}
static int aligner_status(int h) {
    if (h == ALIGN_ST_BAD_INPUT) return fail(PARROT_E_INVALID, "aligner: a mel_len outside [1, T] (status 9)");
    return fail(PARROT_E_NONFINITE, "aligner: non-finite logit (a NaN / inf mel value, or an activation beyond the fp16 split scheme's range: use PARROT_PREC_BF16X6 or PARROT_PREC_F32)");
}
extern "C" int parrot_aligner_check(parrot_aligner_t* al, void* stream) { return al ? check_flag(al->err, (hipStream_t)stream, aligner_status) : PARROT_E_INVALID; }
extern "C" int parrot_aligner_status_async(parrot_aligner_t* al, int32_t* dst_dev, void* stream) {
    return al ? status_async(al->err, dst_dev, (hipStream_t)stream) : PARROT_E_INVALID;
}
