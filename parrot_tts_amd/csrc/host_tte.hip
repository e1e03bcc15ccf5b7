// host_tte.hip -- the text-to-unit model: create, the FFT block, encode / decode with the tie guard, the loss and the stand-alone
// length regulator.
#include "host_common.h"

#include <algorithm>
#include <cmath>
#include <vector>

#include "attn.h"
#include "kernels_misc.h"

using namespace parrot;

// ---------------------------------------------------------------------------------------------
// TTE
// ---------------------------------------------------------------------------------------------
struct FftLayer {
    std::unique_ptr<parrot_conv> qkv, in_proj, out_proj, wo, conv1, conv2;
    float *an_w = nullptr, *an_b = nullptr, *cn_w = nullptr, *cn_b = nullptr;
    int heads = 1;
    bool merged = false;  // qkv holds in_proj * qkv, wo holds wo * out_proj (in_proj / out_proj unused)
    ~FftLayer() {
        for (float* p : {an_w, an_b, cn_w, cn_b})
            if (p) (void)hipFree(p);
    }
};

struct parrot_tte {
    parrot_tte_cfg cfg{};
    float *pe = nullptr, *tok = nullptr, *spk = nullptr;
    float *ln0_w = nullptr, *ln0_b = nullptr, *ln1_w = nullptr, *ln1_b = nullptr;
    DevFlag err;
    std::unique_ptr<parrot_conv> dp0, dp1, dp_proj, head;
    std::vector<std::unique_ptr<FftLayer>> enc, dec;
    std::vector<float*> dbg_enc, dbg_dec;  // parrot_tte_debug_stages (tests only)
    int scheme = 0;                        // PARROT_PREC_* captured at create
    bool flash = false;                    // attention core on attn_flash_kernel (any T, no score tensor)
    // tie guard (argmax_cf_kernel / tie_guard_refine_kernel): fp32 head weights (transposed to (D, V)) for the fp64 re-evaluation, the (b, t) list of
    // the last decode's low-margin positions and its statistics {count, min margin bits, ids changed}
    float *head_w = nullptr, *head_b = nullptr;
    // (one set per decoder lane -- parrot_tte_decode_rows: row groups of one batch may decode concurrently on several streams --
    //  laid out back to back: lane l's list / statistics / refined logits start at l x the per-lane size)
    static constexpr int LANES = 1;
    int *glist = nullptr, *gstat = nullptr;
    int lanes_used = 1;  // bit l: lane l took part in the last decoded batch (host-side bookkeeping of the statistics readers)
    float guard = 1e-4f;
    // ... extended to the last decoder block's FFN output (round 4): for a guarded position the block's conv2 (1x1) + bias +
    // residual are re-evaluated in fp64 from the fp32 activations the block itself produced (relu(conv1) and x + attn), then the
    // head: last_w2t = that conv2's weight transposed to (F, D), last_b2 its bias; gref = the refined logits of the guarded
    // positions of the last decode (TIE_GUARD_MAX x V floats, parrot_tte_guard_logits)
    float *last_w2t = nullptr, *last_b2 = nullptr, *gref = nullptr;
    bool merged = true;
    ~parrot_tte() {
        for (float* p : {pe, tok, spk, ln0_w, ln0_b, ln1_w, ln1_b, head_w, head_b, last_w2t, last_b2, gref})
            if (p) (void)hipFree(p);
        if (glist) (void)hipFree(glist);
        if (gstat) (void)hipFree(gstat);
    }
};

static int build_fft(std::unique_ptr<FftLayer>& slot, const parrot_tte_cfg& c, int heads, const parrot_fft_weights& w) {
    std::unique_ptr<FftLayer> L(new FftLayer());
    const int D = c.d_model, F = c.n_filter_ffn;
    if (D % heads) return fail(PARROT_E_INVALID, "tte_create: d_model % n_head != 0");  // fft.py:44
    L->heads = heads;
    // The reference projects twice on each side of the attention core (quirk Q3: the block's own bias-free qkv / wo
    // Linear around nn.MultiheadAttention's bias-free in_proj / out_proj, fft.py:48-57).  Two linear maps with
    // nothing in between are ONE linear map: the products are formed here in fp64 and rounded once to fp32
    //     W_qkv' = blockdiag(W_in_q, W_in_k, W_in_v) * W_qkv   (3D x D),     W_o' = W_wo * W_out   (D x D)
    // which removes two launches per block (PARROT_TTE_MERGE=0 keeps the four separate projections).
    const bool merge = create_merge();
    L->merged = merge;
    if (merge) {
        std::vector<float> wq((size_t)3 * D * D), wo((size_t)D * D);
        std::vector<double> row(D);
        for (int g = 0; g < 3; ++g)
            for (int i = 0; i < D; ++i) {  // row i of group g: sum_j in_proj[gD+i][j] * qkv[gD+j][:]
                std::fill(row.begin(), row.end(), 0.0);
                for (int j = 0; j < D; ++j) {
                    const double a = w.in_proj[((size_t)g * D + i) * D + j];
                    const float* q = w.qkv + ((size_t)g * D + j) * D;
                    for (int c2 = 0; c2 < D; ++c2) row[c2] += a * (double)q[c2];
                }
                for (int c2 = 0; c2 < D; ++c2) wq[((size_t)g * D + i) * D + c2] = (float)row[c2];
            }
        for (int i = 0; i < D; ++i) {  // W_o'[i][:] = sum_j wo[i][j] * out_proj[j][:]
            std::fill(row.begin(), row.end(), 0.0);
            for (int j = 0; j < D; ++j) {
                const double a = w.wo[(size_t)i * D + j];
                const float* q = w.out_proj + (size_t)j * D;
                for (int c2 = 0; c2 < D; ++c2) row[c2] += a * (double)q[c2];
            }
            for (int c2 = 0; c2 < D; ++c2) wo[(size_t)i * D + c2] = (float)row[c2];
        }
        TRY(make_conv(L->qkv, D, 3 * D, 1, 1, 0, 0, 1, PRE_NONE, 0.f, ACT_NONE, wq.data(), nullptr));
        TRY(make_conv(L->wo, D, D, 1, 1, 0, 0, 1, PRE_NONE, 0.f, ACT_NONE, wo.data(), nullptr));
    } else {
        TRY(make_conv(L->qkv, D, 3 * D, 1, 1, 0, 0, 1, PRE_NONE, 0.f, ACT_NONE, w.qkv, nullptr));
        // MHA in_proj: three bias-free (D,D) projections of three different inputs = a grouped 1x1 conv
        TRY(make_conv(L->in_proj, 3 * D, 3 * D, 1, 1, 0, 0, 1, PRE_NONE, 0.f, ACT_NONE, w.in_proj, nullptr, 3));
        TRY(make_conv(L->out_proj, D, D, 1, 1, 0, 0, 1, PRE_NONE, 0.f, ACT_NONE, w.out_proj, nullptr));
        TRY(make_conv(L->wo, D, D, 1, 1, 0, 0, 1, PRE_NONE, 0.f, ACT_NONE, w.wo, nullptr));
    }
    // the residual stream of an FFT block is ~10x larger than what a sub-layer adds to it: add it AFTER the sum (as the
    // reference does, fft.py:97,99), not as the accumulator's starting value
    L->wo->late_res = true;
    TRY(make_conv(L->conv1, D, F, c.ffn_k1, 1, (c.ffn_k1 - 1) / 2, 0, 1, PRE_NONE, 0.f, ACT_RELU, w.conv1_w, w.conv1_b));
    TRY(make_conv(L->conv2, F, D, c.ffn_k2, 1, (c.ffn_k2 - 1) / 2, 0, 1, PRE_NONE, 0.f, ACT_NONE, w.conv2_w, w.conv2_b));
    L->conv2->late_res = true;
    TRY(upload(&L->an_w, w.attn_norm_w, D));
    TRY(upload(&L->an_b, w.attn_norm_b, D));
    TRY(upload(&L->cn_w, w.conv_norm_w, D));
    TRY(upload(&L->cn_b, w.conv_norm_b, D));
    slot = std::move(L);
    return PARROT_OK;
}

static int tte_create(parrot_tte_t** out, const parrot_tte_cfg* cfg, const parrot_tte_weights* w, int prec, int merge) {
    CreateScope scope(prec, -1, merge);  // (thread-local: the process defaults are not touched)
    if (!out || !cfg || !w) return fail(PARROT_E_INVALID, "tte_create: null argument");
    const parrot_tte_cfg& c = *cfg;
    if (c.d_model <= 0 || c.n_filter_ffn <= 0 || c.max_len <= 0 || c.vocab <= 0 || c.n_codes <= 0 || c.dp_filter <= 0 ||
        c.enc_layers < 0 || c.dec_layers < 0 || c.ffn_k1 <= 0 || c.ffn_k2 <= 0 || c.dp_kernel <= 0)
        return fail(PARROT_E_INVALID, "tte_create: bad config");
    if (!(c.ffn_k1 & 1) || !(c.ffn_k2 & 1)) return fail(PARROT_E_UNSUPPORTED, "tte_create: even FFN kernel sizes change the sequence length");
    if (c.dp_kernel != 3) return fail(PARROT_E_UNSUPPORTED, "tte_create: duration_predictor.kernel_size != 3 changes the sequence length in the reference (padding=1 is hard-coded, duration.py:34)");
    std::unique_ptr<parrot_tte> t(new parrot_tte());
    t->cfg = c;
    t->scheme = create_prec();
    {
        // flash attention runs on the fp16 split pipe: the default scheme and the fp16 reduced-precision mode take it; the exact
        // (f32), bf16x6 and bf16 handles keep the fp32-MFMA cores (fused for T <= 256, three kernels beyond)
        static const bool want = [] { const char* e = getenv("PARROT_FLASH_ATTN"); return !e || atoi(e) != 0; }();
        // (attn_flash_kernel is built on the fp16 pipe: a bf16 handle keeps fp32's exponent range by staying on the fp32-MFMA cores)
        const bool sch_ok = t->scheme == PARROT_PREC_F16X3 || t->scheme == PARROT_PREC_F16;
        auto hd_ok = [&](int layers, int heads) { return layers == 0 || (heads > 0 && c.d_model % heads == 0 && attn_flash_has(c.d_model / heads)); };
        t->flash = want && sch_ok && hd_ok(c.enc_layers, c.enc_heads) && hd_ok(c.dec_layers, c.dec_heads);
    }
    const int D = c.d_model;
    TRY(upload(&t->pe, w->pe, (size_t)c.max_len * D));
    TRY(upload(&t->tok, w->tok_emb, (size_t)c.vocab * D));
    if (c.n_speaker > 1) {
        if (!w->speaker_emb) return fail(PARROT_E_INVALID, "tte_create: n_speaker > 1 without speaker_emb");
        TRY(upload(&t->spk, w->speaker_emb, (size_t)c.n_speaker * D));
    }
    TRY(t->err.init());
    TRY(make_conv(t->dp0, D, c.dp_filter, c.dp_kernel, 1, (c.dp_kernel - 1) / 2, 0, 1, PRE_NONE, 0.f, ACT_NONE, w->dp_conv0_w, w->dp_conv0_b));
    TRY(make_conv(t->dp1, c.dp_filter, c.dp_filter, c.dp_kernel, 1, 1 /* Q4 */, 0, 1, PRE_NONE, 0.f, ACT_NONE, w->dp_conv1_w, w->dp_conv1_b));
    TRY(make_conv(t->dp_proj, c.dp_filter, 1, 1, 1, 0, 0, 1, PRE_NONE, 0.f, ACT_NONE, w->dp_proj_w, w->dp_proj_b));
    TRY(upload(&t->ln0_w, w->dp_ln0_w, c.dp_filter));
    TRY(upload(&t->ln0_b, w->dp_ln0_b, c.dp_filter));
    TRY(upload(&t->ln1_w, w->dp_ln1_w, c.dp_filter));
    TRY(upload(&t->ln1_b, w->dp_ln1_b, c.dp_filter));
    t->merged = create_merge();
    t->enc.resize(c.enc_layers);
    t->dec.resize(c.dec_layers);
    for (int i = 0; i < c.enc_layers; ++i) TRY(build_fft(t->enc[i], c, c.enc_heads, w->enc[i]));
    for (int i = 0; i < c.dec_layers; ++i) TRY(build_fft(t->dec[i], c, c.dec_heads, w->dec[i]));
    TRY(make_conv(t->head, D, c.n_codes, 1, 1, 0, 0, 1, PRE_NONE, 0.f, ACT_NONE, w->head_w, w->head_b));
    {   // tie guard: PARROT_TIE_GUARD = margin below which a position's head is re-evaluated in fp64 (0 switches it off)
        const char* e = getenv("PARROT_TIE_GUARD");
        t->guard = e ? (float)atof(e) : 1e-4f;
        {   // (D, V): the refine kernel reads one code per thread, coalesced
            std::vector<float> wt((size_t)c.n_codes * D);
            for (int v = 0; v < c.n_codes; ++v)
                for (int ch = 0; ch < D; ++ch) wt[(size_t)ch * c.n_codes + v] = w->head_w[(size_t)v * D + ch];
            TRY(upload(&t->head_w, wt.data(), wt.size()));
        }
        if (w->head_b) TRY(upload(&t->head_b, w->head_b, (size_t)c.n_codes));
        if (c.dec_layers > 0 && c.ffn_k2 == 1) {  // deep guard: the last decoder block's conv2 as (F, D) + its bias
            const parrot_fft_weights& lw = w->dec[c.dec_layers - 1];
            const int F = c.n_filter_ffn;
            std::vector<float> wt((size_t)F * D);
            for (int o = 0; o < D; ++o)
                for (int j = 0; j < F; ++j) wt[(size_t)j * D + o] = lw.conv2_w[(size_t)o * F + j];
            TRY(upload(&t->last_w2t, wt.data(), wt.size()));
            if (lw.conv2_b) TRY(upload(&t->last_b2, lw.conv2_b, (size_t)D));
        }
        HIP_TRY(hipMalloc((void**)&t->gref, (size_t)parrot_tte::LANES * TIE_GUARD_MAX * c.n_codes * sizeof(float)));
        HIP_TRY(hipMalloc((void**)&t->glist, (size_t)parrot_tte::LANES * 2 * TIE_GUARD_MAX * sizeof(int)));
        HIP_TRY(hipMalloc((void**)&t->gstat, (size_t)parrot_tte::LANES * 4 * sizeof(int)));
        HIP_TRY(hipMemset(t->gstat, 0, (size_t)parrot_tte::LANES * 4 * sizeof(int)));
    }
    *out = t.release();
    return PARROT_OK;
}
extern "C" int parrot_tte_create(parrot_tte_t** out, const parrot_tte_cfg* cfg, const parrot_tte_weights* w) { return tte_create(out, cfg, w, -1, -1); }
extern "C" int parrot_tte_create_ex(parrot_tte_t** out, const parrot_tte_cfg* cfg, const parrot_tte_weights* w, int32_t precision,
                                    int32_t merge_projections) {
    if (precision > PARROT_PREC_F16 || merge_projections > 1) return fail(PARROT_E_INVALID, "tte_create_ex: precision in -1 .. 4, merge_projections in -1 .. 1");
    return tte_create(out, cfg, w, precision, merge_projections);
}
extern "C" int parrot_tte_precision(const parrot_tte_t* t) { return t ? t->scheme : PARROT_E_INVALID; }
extern "C" void parrot_tte_destroy(parrot_tte_t* t) { delete t; }

struct TteState {  // persists between encode and decode (sized by B,S only)
    float* enc_out;
    int32_t* cum;
    int32_t* out_len;
};
static TteState tte_state(const parrot_tte* t, Arena& a, int B, int S) {
    TteState st;
    st.enc_out = a.take<float>((size_t)B * t->cfg.d_model * S);
    st.cum = a.take<int32_t>((size_t)B * S);
    st.out_len = a.take<int32_t>((size_t)B);
    return st;
}
struct TteScratch {
    float *x, *n, *qkv1, *qkv2, *scores, *ctx, *o, *h, *f, *logits;
};
static TteScratch tte_scratch(const parrot_tte* t, Arena& a, int B, int T, bool with_logits) {
    const parrot_tte_cfg& c = t->cfg;
    const int Hmax = std::max(std::max(c.enc_heads, c.dec_heads), 1);
    const size_t DT = (size_t)B * c.d_model * T;
    const int Fmax = std::max(c.n_filter_ffn, c.dp_filter);
    TteScratch s;
    s.x = a.take<float>(DT);
    s.n = a.take<float>(std::max(DT, (size_t)B * c.dp_filter * T));
    s.qkv1 = a.take<float>(3 * DT);
    s.qkv2 = a.take<float>(3 * DT);
    s.scores = t->flash ? nullptr : a.take<float>((size_t)B * Hmax * T * T);  // (only the three-kernel attention path materialises scores)
    s.ctx = a.take<float>(DT);
    s.o = a.take<float>(DT);
    s.h = a.take<float>(DT);
    s.f = a.take<float>((size_t)B * Fmax * T);
    s.logits = with_logits ? a.take<float>((size_t)B * c.n_codes * T) : nullptr;
    return s;
}

extern "C" size_t parrot_tte_state_bytes(const parrot_tte_t* t, int32_t B, int32_t S) {
    if (!t || B <= 0 || S <= 0) return 0;
    Arena a(nullptr, 0);
    (void)tte_state(t, a, B, S);
    return align_up(a.off, 256);
}
extern "C" size_t parrot_tte_workspace_bytes(const parrot_tte_t* t, int32_t B, int32_t S, int32_t L_max) {
    if (!t || B <= 0 || S <= 0) return 0;
    Arena a(nullptr, 0);
    (void)tte_scratch(t, a, B, std::max(S, L_max), L_max > 0);
    return align_up(a.off, 256);
}

// row-exact mode: row b holds len[b] real positions (NULL: dense rows)
static ConvOpts rows_of(const int32_t* len) {
    ConvOpts o;
    o.rows.len = len;
    return o;
}
static int layernorm(const float* x, const float* g, const float* b, float* y, int B, int C, int T, int relu_in, hipStream_t s) {
    hipLaunchKernelGGL(layernorm_cf_kernel<16>, dim3((T + 63) / 64, B), dim3(16 * 64), 0, s, x, g, b, y, C, T, 1e-5f, relu_in);
    HIP_TRY(hipGetLastError());
    return PARROT_OK;
}

// The attention core softmax(q k^T sqrt(1/hd) + key mask) v of one FFT block on the channel-first (B, 3, D, T) projections:
// ctx (B, D, T).  `core` names the launch sequence (fft_block picks it; parrot_debug_attention runs any of them on its own):
//   ATTN_CORE_THREE  bgemm_mfma_kernel -> softmax_mask_kernel -> bgemm_mfma_kernel through scores (B, H, T, T): any hd, any T
//   ATTN_CORE_FUSED  attn_fused_kernel<128, 32>, one launch: hd = 128 and T <= ATTN_TMAX only
//   ATTN_CORE_FLASH  attn_flash_kernel<hd>, online softmax on the fp16 split pipe: attn_flash_has(hd), any T
// The caller has checked that the core takes the shape; scores is only read by ATTN_CORE_THREE.
enum { ATTN_CORE_THREE = 0, ATTN_CORE_FUSED = 1, ATTN_CORE_FLASH = 2 };
static int attention_core(int core, const float* qkv, const uint8_t* valid, float* ctx, float* scores, int B, int T, int H, int D,
                          hipStream_t s) {
    const int hd = D / H;
    const long DT = (long)D * T;
    if (core == ATTN_CORE_FLASH) {  // any T, online softmax, no score tensor (attn.h: attn_flash_kernel)
        AttnParams p{};
        p.qkv = qkv; p.valid = valid; p.ctx = ctx;
        p.T = T; p.H = H; p.D = D; p.hd = hd;
        p.alpha = (float)std::sqrt(1.0 / (double)hd);
        HIP_TRY(launch_attn_flash(p, B, s));
    } else if (core == ATTN_CORE_FUSED) {  // scores, softmax and context in one launch (attn.h)
        AttnParams p{};
        p.qkv = qkv; p.valid = valid; p.ctx = ctx;
        p.T = T; p.H = H; p.D = D; p.hd = hd;
        p.alpha = (float)std::sqrt(1.0 / (double)hd);
        const size_t lds = (size_t)32 * (((T + 31) / 32) * 32 + 1) * sizeof(float);  // 32-query tiles (33 KiB at T = 256: no opt-in needed)
        hipLaunchKernelGGL((attn_fused_kernel<128, 32>), dim3((T + 31) / 32, B * H), dim3(256), lds, s, p);
        HIP_TRY(hipGetLastError());
    } else {
    {   // scores[b,h][tq][tk] = sum_c (q[c][tq] * sqrt(1/hd)) * k[c][tk]
        BgemmParams p{};
        p.A = qkv; p.B = qkv + DT; p.C = scores;
        p.M = T; p.N = T; p.K = hd;
        p.a_sk = T; p.a_sm = 1; p.b_sk = T; p.b_sn = 1;
        p.a_zb = 3 * DT; p.a_zh = (long)hd * T; p.b_zb = 3 * DT; p.b_zh = (long)hd * T;
        p.c_zb = (long)H * T * T; p.c_zh = (long)T * T; p.ldc = T; p.H = H;
        p.alpha = (float)std::sqrt(1.0 / (double)hd);
        hipLaunchKernelGGL(bgemm_mfma_kernel, dim3((T + 63) / 64, (T + 63) / 64, B * H), dim3(256), 0, s, p);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(softmax_mask_kernel, dim3((B * H * T + 3) / 4), dim3(256), 0, s, scores, valid, B * H * T, T, H * T);
    HIP_TRY(hipGetLastError());
    {   // ctx[b][h*hd + c][tq] = sum_tk v[c][tk] * P[tq][tk]
        BgemmParams p{};
        p.A = qkv + 2 * DT; p.B = scores; p.C = ctx;
        p.M = hd; p.N = T; p.K = T;
        p.a_sk = 1; p.a_sm = T; p.b_sk = 1; p.b_sn = T;
        p.a_zb = 3 * DT; p.a_zh = (long)hd * T; p.b_zb = (long)H * T * T; p.b_zh = (long)T * T;
        p.c_zb = DT; p.c_zh = (long)hd * T; p.ldc = T; p.H = H;
        p.alpha = 1.0f;
        hipLaunchKernelGGL(bgemm_mfma_kernel, dim3((T + 63) / 64, (hd + 63) / 64, B * H), dim3(256), 0, s, p);
        HIP_TRY(hipGetLastError());
    }
    }
    return PARROT_OK;
}

// FFTBlock.forward (fft.py:94-100): x -> out (may alias x).  valid (B,T) u8: 1 = attend to this key.
// row_len (B) i32 device, nullable: ROW-EXACT mode -- row b holds row_len[b] real positions and every conv applies its zero padding
// at the row's own end (the reference run of that utterance alone, fft.py:78-82); NULL: the reference's padded-batch semantics, pad
// frames leak through the k = 9 conv (quirk Q7).
static int fft_block(const parrot_tte* t, const FftLayer* L, TteScratch& w, float* x, const uint8_t* valid, int B, int T, hipStream_t s,
                     const int32_t* row_len = nullptr) {
    const int D = t->cfg.d_model, H = L->heads, hd = D / H;
    TRY(layernorm(x, L->an_w, L->an_b, w.n, B, D, T, 0, s));
    if (L->merged) {
        TRY(conv_launch(L->qkv.get(), w.n, nullptr, w.qkv2, B, T, EPI_STORE, 1.f, s));
    } else {
        TRY(conv_launch(L->qkv.get(), w.n, nullptr, w.qkv1, B, T, EPI_STORE, 1.f, s));
        TRY(conv_launch(L->in_proj.get(), w.qkv1, nullptr, w.qkv2, B, T, EPI_STORE, 1.f, s));
    }
    // the selection rule: a flash handle takes attn_flash_kernel at any T; the fp32-MFMA handles take the fused core where it
    // fits (hd = 128, T <= 256) and the three-kernel path everywhere else
    const int core = t->flash ? ATTN_CORE_FLASH : (T <= ATTN_TMAX && hd == 128) ? ATTN_CORE_FUSED : ATTN_CORE_THREE;
    TRY(attention_core(core, w.qkv2, valid, w.ctx, w.scores, B, T, H, D, s));
    if (L->merged) {
        TRY(conv_launch(L->wo.get(), w.ctx, x, w.h, B, T, EPI_STORE, 1.f, s));        // h = x + attn
    } else {
        TRY(conv_launch(L->out_proj.get(), w.ctx, nullptr, w.o, B, T, EPI_STORE, 1.f, s));
        TRY(conv_launch(L->wo.get(), w.o, x, w.h, B, T, EPI_STORE, 1.f, s));          // h = x + attn
    }
    TRY(layernorm(w.h, L->cn_w, L->cn_b, w.n, B, D, T, 0, s));
    // (a 1x1 conv has no neighbours to leak from: only the k > 1 convs take the per-row ends)
    TRY(conv_launch(L->conv1.get(), w.n, nullptr, w.f, B, T, EPI_STORE, 1.f, s, rows_of(t->cfg.ffn_k1 > 1 ? row_len : nullptr)));  // relu fused
    TRY(conv_launch(L->conv2.get(), w.f, w.h, x, B, T, EPI_STORE, 1.f, s, rows_of(t->cfg.ffn_k2 > 1 ? row_len : nullptr)));      // out = h + ffn
    return PARROT_OK;
}

// The launches of the duration / length-regulator / argmax glue kernels (kernels_misc.h), one helper each: the model paths below and
// the parrot_debug_* entry points (tests) run the same launch code.
static int launch_durations(const float* ld_raw, const uint8_t* src_valid, float* log_dur, int64_t* dur, int32_t* cum, int32_t* out_len, int B,
                            int S, const int32_t* src_len, int* err, hipStream_t s) {
    hipLaunchKernelGGL(duration_kernel, dim3(B), dim3(256), 0, s, ld_raw, src_valid, log_dur, dur, cum, out_len, S, src_len, err);
    HIP_TRY(hipGetLastError());
    return PARROT_OK;
}
static int launch_dur_prefix(const int64_t* dur, int32_t* cum, int32_t* out_len, int B, int S, int* err, const int32_t* src_len, hipStream_t s) {
    hipLaunchKernelGGL(dur_prefix_kernel, dim3(B), dim3(256), 0, s, dur, cum, out_len, S, err, src_len);
    HIP_TRY(hipGetLastError());
    return PARROT_OK;
}
static int launch_length_regulate(const float* enc, const int32_t* cum, const int32_t* out_len, const float* pe, float* y, uint8_t* tgt_mask, int B,
                                  int S, int L, int D, int* gstat, int gstat_reset, int row_exact, int pe_stride, hipStream_t s) {
    hipLaunchKernelGGL(length_regulate_kernel, dim3((L + 63) / 64, B), dim3(256), 0, s, enc, cum, out_len, pe, y, tgt_mask, S, L, D, gstat,
                       gstat_reset, row_exact, pe_stride);
    HIP_TRY(hipGetLastError());
    return PARROT_OK;
}
// the tie guard's fp64 re-evaluation (tie_guard_refine_kernel): x == NULL switches it off
struct RefineArgs {
    const float *x = nullptr, *hwt = nullptr, *hb = nullptr;                     // (B, D, L), (D, V), (V) nullable
    const float *f = nullptr, *h = nullptr, *w2t = nullptr, *b2 = nullptr;       // deep form (f != NULL): (B, F, L), (B, D, L), (F, D), (D) nullable
    int D = 0, F = 0;
    float* gref = nullptr;
};
// argmax + tie guard: gstat = {count, ids changed, min margin (float bits), first list entry of this row group}; glist / gstat NULL: ids only
static int launch_argmax_guard(const float* logits, int64_t* ids, int B, int V, int L, int* err, float guard, int* glist, int* gstat, int row0,
                               const RefineArgs& r, hipStream_t s) {
    hipLaunchKernelGGL(argmax_cf_kernel, dim3((L + 63) / 64, B), dim3(64 * ARGMAX_WAVES), 0, s, logits, ids, V, L, err, guard, glist, gstat, row0);
    HIP_TRY(hipGetLastError());
    if (gstat && r.x) {  // re-evaluate the head of the low-margin positions in fp64 (workgroups beyond the count exit at once)
        const bool deep = r.f != nullptr;
        hipLaunchKernelGGL(tie_guard_refine_kernel, dim3(TIE_GUARD_MAX), dim3(256), (size_t)(r.D + (deep ? r.F : 0)) * sizeof(double), s, r.x, r.hwt,
                           r.hb, ids, r.D, V, L, glist, gstat, r.f, r.h, r.w2t, r.b2, r.F, r.gref, row0);
        HIP_TRY(hipGetLastError());
    }
    return PARROT_OK;
}

// Encode rows [row0, row0 + B) of a batch of Bfull rows: every pointer argument is the GROUP's first row; the group's encoder
// output / duration prefix sums land in rows row0.. of `state` (sized for Bfull rows).  The encoder works row by row and pe[S] is
// indexed by the padded length S alone (fft.py:18), so a row's result does not depend on the grouping.
static int tte_encode_rows(parrot_tte_t* t, const int64_t* phones, const uint8_t* src_mask, const int64_t* speaker, const int32_t* src_len,
                           int32_t Bfull, int32_t S, int32_t row0, int32_t B, float* log_dur, int64_t* dur, int32_t* out_lens, void* state,
                           size_t state_bytes, void* ws, size_t ws_bytes, void* stream) {
    if (!t || !phones || !src_mask || !log_dur || !dur || !out_lens || !state || !ws) return fail(PARROT_E_INVALID, "tte_encode: null argument");
    if (Bfull <= 0 || S <= 0) return fail(PARROT_E_INVALID, "tte_encode: empty batch");
    if (row0 < 0 || B <= 0 || row0 + B > Bfull) return fail(PARROT_E_INVALID, "tte_encode: row group outside the batch");
    const parrot_tte_cfg& c = t->cfg;
    if (S >= c.max_len) return fail(PARROT_E_RANGE, "tte_encode: sequence length >= max_len (pe[T] out of range, fft.py:18)");
    if (t->spk && !speaker) return fail(PARROT_E_INVALID, "tte_encode: multi-speaker model needs speaker ids");
    hipStream_t s = (hipStream_t)stream;
    Arena sa(state, state_bytes);
    TteState st = tte_state(t, sa, Bfull, S);
    Arena a(ws, ws_bytes);
    TteScratch w = tte_scratch(t, a, B, S, false);
    if (!sa.ok || !a.ok) return fail(PARROT_E_NOMEM, "tte_encode: state/workspace too small");
    st.enc_out += (size_t)row0 * c.d_model * S;
    st.cum += (size_t)row0 * S;
    st.out_len += row0;
    const int D = c.d_model;
    // pe[S] of the padded batch (quirk Q1 / Q7), or -- row-exact -- pe[src_len[b]]: what the row's own B = 1 run adds (fft.py:18)
    hipLaunchKernelGGL(tte_embed_kernel, dim3((S + 63) / 64, (D + 63) / 64, B), dim3(256), 0, s, phones, t->tok, t->pe, src_len,
                       w.x, S, D, c.vocab, t->err);
    HIP_TRY(hipGetLastError());
    auto dbg = [&](const std::vector<float*>& v, size_t idx, const float* src, size_t n) -> int {
        if (idx < v.size() && v[idx]) HIP_TRY(hipMemcpyAsync(v[idx] + (size_t)row0 * D * S, src, n * sizeof(float), hipMemcpyDeviceToDevice, s));
        return PARROT_OK;
    };
    TRY(dbg(t->dbg_enc, 0, w.x, (size_t)B * D * S));
    for (size_t n = 0; n < t->enc.size(); ++n) {
        TRY(fft_block(t, t->enc[n].get(), w, w.x, src_mask, B, S, s, src_len));
        TRY(dbg(t->dbg_enc, 1 + n, w.x, (size_t)B * D * S));
    }
    if (t->spk) {
        const size_t total = (size_t)B * D * S;
        hipLaunchKernelGGL(add_channel_vec_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, w.x, speaker, t->spk, D, S,
                           c.n_speaker, total, t->err);
        HIP_TRY(hipGetLastError());
    }
    TRY(dbg(t->dbg_enc, 1 + t->enc.size(), w.x, (size_t)B * D * S));
    HIP_TRY(hipMemcpyAsync(st.enc_out, w.x, (size_t)B * D * S * sizeof(float), hipMemcpyDeviceToDevice, s));
    // duration predictor (duration.py:29-48): conv -> relu -> LN -> conv(pad 1) -> relu -> LN -> linear
    const int NF = c.dp_filter;
    TRY(conv_launch(t->dp0.get(), w.x, nullptr, w.f, B, S, EPI_STORE, 1.f, s, rows_of(src_len)));
    TRY(layernorm(w.f, t->ln0_w, t->ln0_b, w.n, B, NF, S, 1, s));
    TRY(conv_launch(t->dp1.get(), w.n, nullptr, w.f, B, S, EPI_STORE, 1.f, s, rows_of(src_len)));
    TRY(layernorm(w.f, t->ln1_w, t->ln1_b, w.n, B, NF, S, 1, s));
    TRY(conv_launch(t->dp_proj.get(), w.n, nullptr, w.o, B, S, EPI_STORE, 1.f, s));  // (B,1,S)
    TRY(launch_durations(w.o, src_mask, log_dur, dur, st.cum, st.out_len, B, S, src_len, t->err, s));
    HIP_TRY(hipMemcpyAsync(out_lens, st.out_len, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    return PARROT_OK;
}
extern "C" int parrot_tte_encode(parrot_tte_t* t, const int64_t* phones, const uint8_t* src_mask, const int64_t* speaker,
                                 const int32_t* src_len, int32_t B, int32_t S, float* log_dur, int64_t* dur, int32_t* out_lens, void* state,
                                 size_t state_bytes, void* ws, size_t ws_bytes, void* stream) {
    if (poison_word() && B > 0 && S > 0) {
        hipStream_t s = (hipStream_t)stream;
        TRY(poison(state, state_bytes, s));
        TRY(poison(ws, ws_bytes, s));
        TRY(poison(log_dur, (size_t)B * S * sizeof(float), s));
        TRY(poison(dur, (size_t)B * S * sizeof(int64_t), s));
        TRY(poison(out_lens, (size_t)B * sizeof(int32_t), s));
    }
    return tte_encode_rows(t, phones, src_mask, speaker, src_len, B, S, 0, B, log_dur, dur, out_lens, state, state_bytes, ws, ws_bytes, stream);
}

// Decode rows [row0, row0 + n) of the batch that parrot_tte_encode left in `state` (B rows).  ids / tgt_mask / logits point at the
// group's own first row.  L is the WHOLE batch's expanded length (pe[L], parrot.py:106) whichever rows are decoded, and every
// kernel of the decoder works row by row, so a row decoded in a group equals the same row decoded with the whole batch bit for bit.
// key_mask (nullable, (B,L) u8 of the group's rows, read only): the caller's key mask (teacher forcing, parrot.py:104-108) replaces
// the one the length regulator builds; tgt_mask is then not written and may be NULL.
static int tte_decode_rows(parrot_tte_t* t, int32_t Bfull, int32_t S, int32_t L, int32_t row0, int32_t B, int64_t* ids, uint8_t* tgt_mask,
                           float* logits, void* state, size_t state_bytes, void* ws, size_t ws_bytes, void* stream, int lane, bool guard_restart,
                           bool new_batch, bool row_exact, const uint8_t* key_mask = nullptr) {
    if (lane < 0 || lane >= parrot_tte::LANES) return fail(PARROT_E_INVALID, "tte_decode: lane out of range");
    if (!t || !ids || !(tgt_mask || key_mask) || !state || !ws) return fail(PARROT_E_INVALID, "tte_decode: null argument");
    if (key_mask) tgt_mask = nullptr;
    if (Bfull <= 0 || S <= 0) return fail(PARROT_E_INVALID, "tte_decode: empty batch");
    if (row0 < 0 || B <= 0 || row0 + B > Bfull) return fail(PARROT_E_INVALID, "tte_decode: row group outside the encoded batch");
    if (L <= 0) return fail(PARROT_E_INVALID, "tte_decode: L must be > 0 (all durations zero: the reference fails in MultiheadAttention too)");
    const parrot_tte_cfg& c = t->cfg;
    if (L >= c.max_len) return fail(PARROT_E_RANGE, "tte_decode: expanded length >= max_len (pe[T] out of range, fft.py:18)");
    hipStream_t s = (hipStream_t)stream;
    Arena sa(state, state_bytes);
    TteState st = tte_state(t, sa, Bfull, S);
    Arena a(ws, ws_bytes);
    TteScratch w = tte_scratch(t, a, B, std::max(S, L), true);
    if (!sa.ok || !a.ok) return fail(PARROT_E_NOMEM, "tte_decode: state/workspace too small");
    const int D = c.d_model, V = c.n_codes;
    // tie-guard state of this lane: a lane's first group of a batch restarts its statistics, later groups of the lane append
    int* const gstat = t->gstat ? t->gstat + 4 * lane : nullptr;
    int* const glist = t->glist ? t->glist + (size_t)lane * 2 * TIE_GUARD_MAX : nullptr;
    float* const gref = t->gref ? t->gref + (size_t)lane * TIE_GUARD_MAX * V : nullptr;
    t->lanes_used = (new_batch ? 0 : t->lanes_used) | (1 << lane);
    TRY(launch_length_regulate(st.enc_out + (size_t)row0 * D * S, st.cum + (size_t)row0 * S, st.out_len + row0, t->pe, w.x, tgt_mask, B, S, L, D,
                               t->guard > 0.f ? gstat : nullptr, guard_restart ? 1 : 0, row_exact ? 1 : 0, -1, s));
    const uint8_t* const valid = key_mask ? key_mask : tgt_mask;
    auto dbg = [&](size_t idx, const float* src, size_t n) -> int {
        if (idx < t->dbg_dec.size() && t->dbg_dec[idx])
            HIP_TRY(hipMemcpyAsync(t->dbg_dec[idx] + (size_t)row0 * D * L, src, n * sizeof(float), hipMemcpyDeviceToDevice, s));
        return PARROT_OK;
    };
    TRY(dbg(0, w.x, (size_t)B * D * L));
    for (size_t n = 0; n < t->dec.size(); ++n) {
        TRY(fft_block(t, t->dec[n].get(), w, w.x, valid, B, L, s, row_exact ? st.out_len + row0 : nullptr));
        TRY(dbg(1 + n, w.x, (size_t)B * D * L));
    }
    TRY(conv_launch(t->head.get(), w.x, nullptr, w.logits, B, L, EPI_STORE, 1.f, s));
    {   // argmax + tie guard: gstat = {count, ids changed, min margin (float bits)} of this decode
        const bool on = t->guard > 0.f;  // (length_regulate_kernel, the first kernel of this decode, has reset gstat)
        // w.f / w.h still hold the last decoder block's relu(conv1) and x + attn: with them the refinement starts one layer
        // earlier (conv2 + bias + residual in fp64, then the head); without a decoder block it starts at w.x
        const bool deep = t->last_w2t != nullptr && !t->dec.empty();
        RefineArgs r;
        r.x = w.x; r.hwt = t->head_w; r.hb = t->head_b;
        r.f = deep ? w.f : nullptr; r.h = deep ? w.h : nullptr; r.w2t = t->last_w2t; r.b2 = t->last_b2;
        r.D = D; r.F = c.n_filter_ffn; r.gref = gref;
        TRY(launch_argmax_guard(w.logits, ids, B, V, L, t->err, t->guard, on ? glist : nullptr, on ? gstat : nullptr, row0, r, s));
    }
    if (logits) {
        hipLaunchKernelGGL(transpose_cf_to_cl_kernel, dim3((L + 63) / 64, (V + 63) / 64, B), dim3(256), 0, s, w.logits, logits, V, L);
        HIP_TRY(hipGetLastError());
    }
    return PARROT_OK;
}
extern "C" int parrot_tte_decode(parrot_tte_t* t, int32_t B, int32_t S, int32_t L, int32_t row_exact, int64_t* ids, uint8_t* tgt_mask,
                                 float* logits, void* state, size_t state_bytes, void* ws, size_t ws_bytes, void* stream) {
    if (poison_word() && t && B > 0 && L > 0) {
        hipStream_t s = (hipStream_t)stream;
        TRY(poison(ws, ws_bytes, s));
        TRY(poison(ids, (size_t)B * L * sizeof(int64_t), s));
        TRY(poison(tgt_mask, (size_t)B * L, s));
        TRY(poison(logits, (size_t)B * L * t->cfg.n_codes * sizeof(float), s));
    }
    return tte_decode_rows(t, B, S, L, 0, B, ids, tgt_mask, logits, state, state_bytes, ws, ws_bytes, stream, 0, true, true, row_exact != 0);
}

// Teacher forcing (parrot.py:104, duration.py:6-24): the caller's durations replace the predicted ones in `state`
extern "C" int parrot_tte_set_durations(parrot_tte_t* t, const int64_t* dur, int32_t B, int32_t S, const int32_t* src_len, int32_t* out_lens,
                                        void* state, size_t state_bytes, void* stream) {
    if (!t || !dur || !out_lens || !state) return fail(PARROT_E_INVALID, "tte_set_durations: null argument");
    if (B <= 0 || S <= 0) return fail(PARROT_E_INVALID, "tte_set_durations: empty batch");
    hipStream_t s = (hipStream_t)stream;
    Arena sa(state, state_bytes);
    TteState st = tte_state(t, sa, B, S);
    if (!sa.ok) return fail(PARROT_E_NOMEM, "tte_set_durations: state too small");
    if (poison_word()) TRY(poison(out_lens, (size_t)B * sizeof(int32_t), s));
    TRY(launch_dur_prefix(dur, st.cum, st.out_len, B, S, t->err, src_len, s));
    HIP_TRY(hipMemcpyAsync(out_lens, st.out_len, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    return PARROT_OK;
}
extern "C" int parrot_tte_decode_masked(parrot_tte_t* t, int32_t B, int32_t S, int32_t L, int32_t row_exact, const uint8_t* key_mask,
                                        int64_t* ids, float* logits, void* state, size_t state_bytes, void* ws, size_t ws_bytes, void* stream) {
    if (!t || !key_mask || !ids || !state || !ws) return fail(PARROT_E_INVALID, "tte_decode_masked: null argument");
    if (poison_word() && B > 0 && L > 0) {
        hipStream_t s = (hipStream_t)stream;
        TRY(poison(ws, ws_bytes, s));
        TRY(poison(ids, (size_t)B * L * sizeof(int64_t), s));
        TRY(poison(logits, (size_t)B * L * t->cfg.n_codes * sizeof(float), s));
    }
    return tte_decode_rows(t, B, S, L, 0, B, ids, nullptr, logits, state, state_bytes, ws, ws_bytes, stream, 0, true, true, row_exact != 0,
                           key_mask);
}

// ModelLoss (modules/loss.py:5-21): loss_rows_kernel + loss_reduce_kernel (kernels_misc.h); with the gradient, loss_count_kernel first
static size_t loss_ws(Arena& a, int32_t N, double** nll, LossCounts** cnt, int64_t** bad) {
    const size_t nblk = (size_t)std::max((N + LOSS_WAVES - 1) / LOSS_WAVES, 1);
    *nll = a.take<double>(nblk);
    *cnt = a.take<LossCounts>(nblk);
    *bad = a.take<int64_t>(nblk);
    return align_up(a.off, 256);
}
extern "C" size_t parrot_tte_loss_workspace_bytes(int32_t N) {
    if (N < 0) return 0;
    Arena a(nullptr, 0);
    double* nll;
    LossCounts* cnt;
    int64_t* bad;
    return loss_ws(a, N, &nll, &cnt, &bad);
}
extern "C" int parrot_tte_loss(const float* logits, const int64_t* targets, int32_t N, int32_t V, int64_t ignore_index, const float* log_dur,
                               const int64_t* dur, const uint8_t* src_mask, int32_t n_src, double* out, float* losses, void* ws, size_t ws_bytes,
                               void* stream) {
    if (!logits || !targets || !log_dur || !dur || !src_mask || !out || !ws) return fail(PARROT_E_INVALID, "tte_loss: null argument");
    if (N <= 0 || V <= 0 || n_src < 0) return fail(PARROT_E_INVALID, "tte_loss: empty logits or negative size");
    hipStream_t s = (hipStream_t)stream;
    Arena a(ws, ws_bytes);
    double* nll;
    LossCounts* cnt;
    int64_t* bad;
    (void)loss_ws(a, N, &nll, &cnt, &bad);
    if (!a.ok) return fail(PARROT_E_NOMEM, "tte_loss: workspace too small");
    if (poison_word()) {
        TRY(poison(ws, ws_bytes, s));
        TRY(poison(out, 8 * sizeof(double), s));
        TRY(poison(losses, 3 * sizeof(float), s));
    }
    const int nblk = (N + LOSS_WAVES - 1) / LOSS_WAVES;
    hipLaunchKernelGGL(loss_rows_kernel<false>, dim3(nblk), dim3(64 * LOSS_WAVES), 0, s, logits, targets, N, V, ignore_index, nll, cnt, bad, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(LOSS_REDUCE), 0, s, nll, cnt, bad, nblk, log_dur, dur, src_mask, n_src, out, losses);
    HIP_TRY(hipGetLastError());
    return PARROT_OK;
}

// The same with the gradient (train.py:72-85): count + duration gradient, rows + logit gradient, the forward's reduction
static size_t loss_grad_ws(Arena& a, int32_t N, double** nll, LossCounts** cnt, int64_t** bad, LossScale** scale) {
    (void)loss_ws(a, N, nll, cnt, bad);
    *scale = a.take<LossScale>(1);
    return align_up(a.off, 256);
}
extern "C" size_t parrot_tte_loss_grad_workspace_bytes(int32_t N) {
    if (N < 0) return 0;
    Arena a(nullptr, 0);
    double* nll;
    LossCounts* cnt;
    int64_t* bad;
    LossScale* scale;
    return loss_grad_ws(a, N, &nll, &cnt, &bad, &scale);
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
    double* nll;
    LossCounts* cnt;
    int64_t* bad;
    LossScale* scale;
    (void)loss_grad_ws(a, N, &nll, &cnt, &bad, &scale);
    if (!a.ok) return fail(PARROT_E_NOMEM, "tte_loss_grad: workspace too small");
    if (poison_word()) {
        TRY(poison(ws, ws_bytes, s));
        TRY(poison(out, 8 * sizeof(double), s));
        TRY(poison(losses, 3 * sizeof(float), s));
        TRY(poison(grad_logits, (size_t)N * V * sizeof(float), s));
        TRY(poison(grad_log_dur, (size_t)n_src * sizeof(float), s));
    }
    const int nblk = (N + LOSS_WAVES - 1) / LOSS_WAVES;
    hipLaunchKernelGGL(loss_count_kernel, dim3(1), dim3(LOSS_REDUCE), 0, s, targets, N, V, ignore_index, log_dur, dur, src_mask, n_src, weights, scale,
                       grad_log_dur);
    HIP_TRY(hipGetLastError());
    if (grad_logits)
        hipLaunchKernelGGL(loss_rows_kernel<true>, dim3(nblk), dim3(64 * LOSS_WAVES), 0, s, logits, targets, N, V, ignore_index, nll, cnt, bad, scale,
                           grad_logits);
    else
        hipLaunchKernelGGL(loss_rows_kernel<false>, dim3(nblk), dim3(64 * LOSS_WAVES), 0, s, logits, targets, N, V, ignore_index, nll, cnt, bad, nullptr,
                           nullptr);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(LOSS_REDUCE), 0, s, nll, cnt, bad, nblk, log_dur, dur, src_mask, n_src, out, losses);
    HIP_TRY(hipGetLastError());
    return PARROT_OK;
}

// ---------------------------------------------------------------------------------------------
// The attention cores and the LayerNorm on their own (tests: include/parrot_hip_debug.h).  Both run the functions fft_block runs.
// ---------------------------------------------------------------------------------------------
static float* debug_attention_ws(Arena& a, int B, int T, int H, int core) {
    float* scores = core == ATTN_CORE_THREE ? a.take<float>((size_t)B * H * T * T) : nullptr;
    a.take<char>(1);  // (never empty: the fused and flash cores take no workspace, and the entry refuses a null one)
    return scores;
}
extern "C" size_t parrot_debug_attention_workspace_bytes(int32_t B, int32_t T, int32_t H, int32_t core) {
    if (B <= 0 || T <= 0 || H <= 0 || core < ATTN_CORE_THREE || core > ATTN_CORE_FLASH) return 0;
    Arena a(nullptr, 0);
    (void)debug_attention_ws(a, B, T, H, core);
    return align_up(a.off, 256);
}
extern "C" int parrot_debug_attention(const float* qkv, const uint8_t* valid, float* ctx, int32_t B, int32_t T, int32_t H, int32_t hd,
                                      int32_t core, void* ws, size_t ws_bytes, void* stream) {
    if (!qkv || !valid || !ctx || !ws) return fail(PARROT_E_INVALID, "debug_attention: null argument");
    if (B <= 0 || T <= 0 || H <= 0 || hd <= 0) return fail(PARROT_E_INVALID, "debug_attention: non-positive size");
    if (core < ATTN_CORE_THREE || core > ATTN_CORE_FLASH) return fail(PARROT_E_INVALID, "debug_attention: core in 0 .. 2");
    if ((long)B * H > 65535 || (long)B * H * T >= (1L << 30) || (long)H * hd >= (1L << 30))  // (grid rows; softmax_mask_kernel's int row count)
        return fail(PARROT_E_UNSUPPORTED, "debug_attention: B H > 65535, or B H T / H hd beyond the kernels' 32-bit indices");
    if (core == ATTN_CORE_FUSED && (hd != 128 || T > ATTN_TMAX))
        return fail(PARROT_E_UNSUPPORTED, "debug_attention: the fused core takes hd = 128 and T <= 256 only");
    if (core == ATTN_CORE_FLASH && !attn_flash_has(hd)) return fail(PARROT_E_UNSUPPORTED, "debug_attention: the flash core takes hd in {16, 32, 64, 128} only");
    hipStream_t s = (hipStream_t)stream;
    Arena a(ws, ws_bytes);
    float* scores = debug_attention_ws(a, B, T, H, core);
    if (!a.ok) return fail(PARROT_E_NOMEM, "debug_attention: workspace too small");
    if (poison_word()) {
        TRY(poison(ws, ws_bytes, s));
        TRY(poison(ctx, (size_t)B * H * hd * T * sizeof(float), s));
    }
    return attention_core(core, qkv, valid, ctx, scores, B, T, H, H * hd, s);
}
extern "C" int parrot_debug_layernorm(const float* x, const float* gamma, const float* beta, float* y, int32_t B, int32_t C, int32_t T,
                                      int32_t relu_in, void* stream) {
    if (!x || !gamma || !beta || !y) return fail(PARROT_E_INVALID, "debug_layernorm: null argument");
    if (B <= 0 || C <= 0 || T <= 0) return fail(PARROT_E_INVALID, "debug_layernorm: non-positive size");
    if (B > 65535) return fail(PARROT_E_UNSUPPORTED, "debug_layernorm: B > 65535 (one grid row per batch row)");
    hipStream_t s = (hipStream_t)stream;
    if (poison_word()) TRY(poison(y, (size_t)B * C * T * sizeof(float), s));
    return layernorm(x, gamma, beta, y, B, C, T, relu_in != 0, s);
}

// ---------------------------------------------------------------------------------------------
// The duration, length-regulator and argmax / tie-guard kernels on their own (tests: include/parrot_hip_debug.h), through the launch
// helpers the model runs, on caller-owned buffers.  `status` stands in for the handle's device status word.
// ---------------------------------------------------------------------------------------------
static int debug_sizes(const char* who, long B, long n1, long n2, long n3) {
    if (B <= 0 || n1 <= 0 || n2 <= 0 || n3 <= 0) return fail(PARROT_E_INVALID, std::string(who) + ": non-positive size");
    if (B > 65535 || n1 > PARROT_DEBUG_MAX_DIM || n2 > PARROT_DEBUG_MAX_DIM || n3 > PARROT_DEBUG_MAX_DIM)
        return fail(PARROT_E_UNSUPPORTED, std::string(who) + ": B > 65535 or a dimension beyond PARROT_DEBUG_MAX_DIM");
    return PARROT_OK;
}
extern "C" int parrot_debug_durations(const float* ld_raw, const uint8_t* src_valid, const int32_t* src_len, int32_t B, int32_t S, float* log_dur,
                                      int64_t* dur, int32_t* cum, int32_t* out_len, int32_t* status, void* stream) {
    if (!ld_raw || !src_valid || !log_dur || !dur || !cum || !out_len || !status) return fail(PARROT_E_INVALID, "debug_durations: null argument");
    TRY(debug_sizes("debug_durations", B, S, 1, 1));
    hipStream_t s = (hipStream_t)stream;
    if (poison_word()) {
        TRY(poison(log_dur, (size_t)B * S * sizeof(float), s));
        TRY(poison(dur, (size_t)B * S * sizeof(int64_t), s));
        TRY(poison(cum, (size_t)B * S * sizeof(int32_t), s));
        TRY(poison(out_len, (size_t)B * sizeof(int32_t), s));
    }
    return launch_durations(ld_raw, src_valid, log_dur, dur, cum, out_len, B, S, src_len, status, s);
}
extern "C" int parrot_debug_length_regulate(const float* enc, const int64_t* dur, const int32_t* src_len, const float* pe, int32_t B, int32_t S,
                                            int32_t D, int32_t L, int32_t P, int32_t row_exact, float* y, uint8_t* tgt_mask, int32_t* cum,
                                            int32_t* out_len, int32_t* status, void* stream) {
    if (!enc || !dur || !pe || !y || !cum || !out_len || !status) return fail(PARROT_E_INVALID, "debug_length_regulate: null argument");
    if (L <= 0) return fail(PARROT_E_INVALID, "debug_length_regulate: L must be > 0");
    TRY(debug_sizes("debug_length_regulate", B, S, D, L));
    if (L >= P) return fail(PARROT_E_RANGE, "debug_length_regulate: L >= P (pe[L] out of range, fft.py:18)");
    hipStream_t s = (hipStream_t)stream;
    if (poison_word()) {
        TRY(poison(y, (size_t)B * D * L * sizeof(float), s));
        TRY(poison(tgt_mask, (size_t)B * L, s));
        TRY(poison(cum, (size_t)B * S * sizeof(int32_t), s));
        TRY(poison(out_len, (size_t)B * sizeof(int32_t), s));
    }
    TRY(launch_dur_prefix(dur, cum, out_len, B, S, status, src_len, s));
    return launch_length_regulate(enc, cum, out_len, pe, y, tgt_mask, B, S, L, D, nullptr, 1, row_exact ? 1 : 0, -1, s);
}
extern "C" int parrot_debug_argmax_guard(const float* logits, int32_t B, int32_t V, int32_t L, float guard, int32_t row0, const float* x, int32_t D,
                                         const float* hwt, const float* hb, const float* f, const float* h, const float* w2t, const float* b2,
                                         int32_t F, const int32_t* gstat_start, int64_t* ids, int32_t* glist, int32_t* gstat, float* gref,
                                         int32_t* status, void* stream) {
    if (!logits || !ids || !glist || !gstat || !status) return fail(PARROT_E_INVALID, "debug_argmax_guard: null argument");
    TRY(debug_sizes("debug_argmax_guard", B, V, L, 1));
    if (!(guard >= 0.f) || row0 < 0) return fail(PARROT_E_INVALID, "debug_argmax_guard: guard and row0 must be >= 0");
    const bool on = guard > 0.f, deep = f != nullptr;
    if (x) {
        if (!hwt || !gref || (deep && (!h || !w2t))) return fail(PARROT_E_INVALID, "debug_argmax_guard: refinement without hwt / gref (deep form: h, w2t)");
        TRY(debug_sizes("debug_argmax_guard", B, D, deep ? F : 1, 1));
        if ((size_t)(D + (deep ? F : 0)) * sizeof(double) > 60000) return fail(PARROT_E_UNSUPPORTED, "debug_argmax_guard: D + F doubles beyond the workgroup's LDS");
    }
    if (gstat_start && (gstat_start[0] < 0 || gstat_start[3] < 0 || gstat_start[3] > std::min(gstat_start[0], TIE_GUARD_MAX)))
        return fail(PARROT_E_INVALID, "debug_argmax_guard: gstat_start needs 0 <= [3] <= min([0], 256)");
    hipStream_t s = (hipStream_t)stream;
    if (poison_word()) {  // (a preset list is an input: with gstat_start, and with the guard off, list / statistics / refined rows stay the caller's)
        TRY(poison(ids, (size_t)B * L * sizeof(int64_t), s));
        if (on && !gstat_start) {
            TRY(poison(glist, (size_t)2 * TIE_GUARD_MAX * sizeof(int32_t), s));
            if (x) TRY(poison(gref, (size_t)TIE_GUARD_MAX * V * sizeof(float), s));
        }
    }
    if (on) {  // what length_regulate_kernel leaves at the start of a decode: a restart, or the caller's second row group of a lane
        const int32_t restart[4] = {0, 0, 0x7f800000, 0};
        HIP_TRY(hipMemcpyAsync(gstat, gstat_start ? gstat_start : restart, sizeof(restart), hipMemcpyHostToDevice, s));
    }
    RefineArgs r;
    r.x = x; r.hwt = hwt; r.hb = hb; r.f = f; r.h = h; r.w2t = w2t; r.b2 = b2; r.D = D; r.F = F; r.gref = gref;
    return launch_argmax_guard(logits, ids, B, V, L, status, guard, on ? glist : nullptr, on ? gstat : nullptr, row0, r, s);
}

extern "C" int parrot_tte_debug_stages(parrot_tte_t* t, float* const* enc_ptrs, float* const* dec_ptrs) {
    if (!t) return fail(PARROT_E_INVALID, "tte_debug_stages: null handle");
    t->dbg_enc.clear();
    t->dbg_dec.clear();
    if (enc_ptrs) t->dbg_enc.assign(enc_ptrs, enc_ptrs + t->enc.size() + 2);
    if (dec_ptrs) t->dbg_dec.assign(dec_ptrs, dec_ptrs + t->dec.size() + 1);
    return PARROT_OK;
}

// length_regulator on its own (duration.py:6-24): channel-last in / out around the decoder's kernel
struct LrScratch {
    float *seq_cf, *out_cf, *zero;  // channel-first input (B, D, S) and output (B, D, L), a zero vector (D)
    int32_t *cum, *lens;
};
static LrScratch lr_scratch(Arena& a, int B, int S, int D, int L) {
    LrScratch w{};
    w.seq_cf = a.take<float>((size_t)B * D * S);
    w.out_cf = a.take<float>((size_t)B * D * L);
    w.zero = a.take<float>((size_t)D);
    w.cum = a.take<int32_t>((size_t)B * S);
    w.lens = a.take<int32_t>((size_t)B);
    return w;
}
extern "C" size_t parrot_length_regulator_workspace_bytes(int32_t B, int32_t S, int32_t D, int32_t L) {
    if (B <= 0 || S <= 0 || D <= 0 || L < 0) return 0;
    Arena a(nullptr, 0);
    (void)lr_scratch(a, B, S, D, std::max(L, 1));
    return align_up(a.off, 256);
}
extern "C" int parrot_length_regulator(const float* seq, const int64_t* dur, int32_t B, int32_t S, int32_t D, int32_t L, float* out,
                                       uint8_t* mask, int32_t* out_lens, void* ws, size_t ws_bytes, void* stream) {
    if (!seq || !dur || !out || !mask || !out_lens || !ws) return fail(PARROT_E_INVALID, "length_regulator: null argument");
    if (B <= 0 || S <= 0 || D <= 0 || L <= 0) return fail(PARROT_E_INVALID, "length_regulator: empty batch or L = 0");
    hipStream_t s = (hipStream_t)stream;
    Arena a(ws, ws_bytes);
    const LrScratch w = lr_scratch(a, B, S, D, L);
    if (!a.ok) return fail(PARROT_E_NOMEM, "length_regulator: workspace too small");
    if (poison_word()) {
        TRY(poison(ws, ws_bytes, s));
        TRY(poison(out, (size_t)B * L * D * sizeof(float), s));
        TRY(poison(mask, (size_t)B * L, s));
        TRY(poison(out_lens, (size_t)B * sizeof(int32_t), s));
    }
    HIP_TRY(hipMemsetAsync(w.zero, 0, (size_t)D * sizeof(float), s));
    // (B,S,D) -> (B,D,S): the transpose kernel with the roles of C and T swapped
    hipLaunchKernelGGL(transpose_cf_to_cl_kernel, dim3((D + 63) / 64, (S + 63) / 64, B), dim3(256), 0, s, seq, w.seq_cf, S, D);
    TRY(launch_dur_prefix(dur, w.cum, w.lens, B, S, nullptr, nullptr, s));
    TRY(launch_length_regulate(w.seq_cf, w.cum, w.lens, w.zero, w.out_cf, mask, B, S, L, D, nullptr, 1, 0, 0, s));
    hipLaunchKernelGGL(transpose_cf_to_cl_kernel, dim3((L + 63) / 64, (D + 63) / 64, B), dim3(256), 0, s, w.out_cf, out, D, L);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_lens, w.lens, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    return PARROT_OK;
}

extern "C" int parrot_tte_status_peek_async(parrot_tte_t* t, int32_t* dst_dev, void* stream) { return peek_async(t ? t->err.p : nullptr, dst_dev, (hipStream_t)stream, "tte_status_peek"); }
extern "C" int parrot_tte_status_async(parrot_tte_t* t, int32_t* dst_dev, void* stream) { return t ? status_async(t->err, dst_dev, (hipStream_t)stream) : PARROT_E_INVALID; }
// Tie-guard statistics of the last decode, copied to dst_dev[0..2] (device memory) on `stream` without synchronising:
// {positions whose top-2 logit margin was below the guard, ids changed by the fp64 re-evaluation of the head, the smallest
// margin of the call as float bits}
static __global__ void guard_stats_sum_kernel(const int* __restrict__ gstat, int mask, int* __restrict__ dst) {
    int n = 0, ch = 0, mn = 0x7f800000;
    for (int l = 0; l < parrot_tte::LANES; ++l)
        if ((mask >> l) & 1) {
            n += gstat[4 * l];
            ch += gstat[4 * l + 1];
            mn = min(mn, gstat[4 * l + 2]);
        }
    dst[0] = n; dst[1] = ch; dst[2] = mn;
}
// out row i = the i-th guarded position of the batch, lanes in order (each lane holds at most TIE_GUARD_MAX)
static __global__ void guard_gather_kernel(const float* __restrict__ gref, const int* __restrict__ glist, const int* __restrict__ gstat, int mask,
                                           int V, int max_n, float* __restrict__ logits, int* __restrict__ list) {
    const int i = blockIdx.x;
    int base = 0, lane = -1, j = 0;
    for (int l = 0; l < parrot_tte::LANES && lane < 0; ++l)
        if ((mask >> l) & 1) {
            const int nl = min(gstat[4 * l], TIE_GUARD_MAX);
            if (i < base + nl) { lane = l; j = i - base; }
            base += nl;
        }
    if (lane < 0 || i >= max_n) return;
    const float* src = gref + ((size_t)lane * TIE_GUARD_MAX + j) * V;
    for (int v = threadIdx.x; v < V; v += blockDim.x) logits[(size_t)i * V + v] = src[v];
    if (threadIdx.x < 2) list[2 * i + threadIdx.x] = glist[((size_t)lane * TIE_GUARD_MAX + j) * 2 + threadIdx.x];
}
extern "C" int parrot_tte_guard_stats_async(parrot_tte_t* t, int32_t* dst_dev, void* stream) {
    if (!t || !dst_dev) return fail(PARROT_E_INVALID, "tte_guard_stats: null argument");
    if (!t->gstat) {
        HIP_TRY(hipMemsetAsync(dst_dev, 0, 3 * sizeof(int), (hipStream_t)stream));
        return PARROT_OK;
    }
    hipLaunchKernelGGL(guard_stats_sum_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, t->gstat, t->lanes_used, dst_dev);
    HIP_TRY(hipGetLastError());
    return PARROT_OK;
}
// Refined (fp64-evaluated, rounded to fp32) logits of the guarded positions of the last decode: logits_dev (max_n x V floats) and
// their (b, t) pairs list_dev (2 max_n ints), device memory, no synchronisation; the count is guard_stats[0] (at most 256 per decoder lane).
extern "C" int parrot_tte_guard_logits(parrot_tte_t* t, float* logits_dev, int32_t* list_dev, int32_t max_n, void* stream) {
    if (!t || !logits_dev || !list_dev || max_n <= 0) return fail(PARROT_E_INVALID, "tte_guard_logits: null argument");
    if (!t->gref) return fail(PARROT_E_UNSUPPORTED, "tte_guard_logits: the tie guard of this handle is off");
    hipLaunchKernelGGL(guard_gather_kernel, dim3(max_n), dim3(256), 0, (hipStream_t)stream, t->gref, t->glist, t->gstat, t->lanes_used,
                       t->cfg.n_codes, max_n, logits_dev, list_dev);
    HIP_TRY(hipGetLastError());
    return PARROT_OK;
}
static int tte_status(int status) { return model_status("tte", status); }
extern "C" int parrot_tte_check(parrot_tte_t* t, void* stream) { return t ? check_flag(t->err, (hipStream_t)stream, tte_status) : PARROT_E_INVALID; }
