// host_tte.hip -- the text-to-unit model: create, the FFT block, encode / decode with the tie guard, and the stand-alone length
// regulator.  Plain host code: every kernel is reached through the launchers of attn.h and tte_glue.h (tu_tte.hip), the same ones
// the parrot_debug_* entry points (host_tte_debug.hip) call.  The loss is host_tte_loss.hip.
#include "host_common.h"

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "attn.h"
#include "tte_glue.h"

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
    static constexpr int LANES = TTE_LANES;
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

// FFTBlock.forward (fft.py:94-100): x -> out (may alias x).  valid (B,T) u8: 1 = attend to this key.
// row_len (B) i32 device, nullable: ROW-EXACT mode -- row b holds row_len[b] real positions and every conv applies its zero padding
// at the row's own end (the reference run of that utterance alone, fft.py:78-82); NULL: the reference's padded-batch semantics, pad
// frames leak through the k = 9 conv (quirk Q7).
static int fft_block(const parrot_tte* t, const FftLayer* L, TteScratch& w, float* x, const uint8_t* valid, int B, int T, hipStream_t s,
                     const int32_t* row_len = nullptr) {
    const int D = t->cfg.d_model, H = L->heads, hd = D / H;
    HIP_TRY(launch_layernorm(x, L->an_w, L->an_b, w.n, B, D, T, 0, s));
    if (L->merged) {
        TRY(conv_launch(L->qkv.get(), w.n, nullptr, w.qkv2, B, T, EPI_STORE, 1.f, s));
    } else {
        TRY(conv_launch(L->qkv.get(), w.n, nullptr, w.qkv1, B, T, EPI_STORE, 1.f, s));
        TRY(conv_launch(L->in_proj.get(), w.qkv1, nullptr, w.qkv2, B, T, EPI_STORE, 1.f, s));
    }
    // the selection rule: a flash handle takes attn_flash_kernel at any T; the fp32-MFMA handles take the fused core where it
    // fits (hd = 128, T <= 256) and the three-kernel path everywhere else
    const int core = t->flash ? ATTN_CORE_FLASH : (T <= ATTN_TMAX && hd == 128) ? ATTN_CORE_FUSED : ATTN_CORE_THREE;
    HIP_TRY(launch_attention_core(core, attn_params(w.qkv2, valid, w.ctx, T, H, D), B, w.scores, s));
    if (L->merged) {
        TRY(conv_launch(L->wo.get(), w.ctx, x, w.h, B, T, EPI_STORE, 1.f, s));        // h = x + attn
    } else {
        TRY(conv_launch(L->out_proj.get(), w.ctx, nullptr, w.o, B, T, EPI_STORE, 1.f, s));
        TRY(conv_launch(L->wo.get(), w.o, x, w.h, B, T, EPI_STORE, 1.f, s));          // h = x + attn
    }
    HIP_TRY(launch_layernorm(w.h, L->cn_w, L->cn_b, w.n, B, D, T, 0, s));
    // (a 1x1 conv has no neighbours to leak from: only the k > 1 convs take the per-row ends)
    TRY(conv_launch(L->conv1.get(), w.n, nullptr, w.f, B, T, EPI_STORE, 1.f, s, rows_of(t->cfg.ffn_k1 > 1 ? row_len : nullptr)));  // relu fused
    TRY(conv_launch(L->conv2.get(), w.f, w.h, x, B, T, EPI_STORE, 1.f, s, rows_of(t->cfg.ffn_k2 > 1 ? row_len : nullptr)));      // out = h + ffn
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
    HIP_TRY(launch_tte_embed(phones, t->tok, t->pe, src_len, w.x, B, S, D, c.vocab, t->err, s));
    auto dbg = [&](const std::vector<float*>& v, size_t idx, const float* src, size_t n) -> int {
        if (idx < v.size() && v[idx]) HIP_TRY(hipMemcpyAsync(v[idx] + (size_t)row0 * D * S, src, n * sizeof(float), hipMemcpyDeviceToDevice, s));
        return PARROT_OK;
    };
    TRY(dbg(t->dbg_enc, 0, w.x, (size_t)B * D * S));
    for (size_t n = 0; n < t->enc.size(); ++n) {
        TRY(fft_block(t, t->enc[n].get(), w, w.x, src_mask, B, S, s, src_len));
        TRY(dbg(t->dbg_enc, 1 + n, w.x, (size_t)B * D * S));
    }
    if (t->spk) HIP_TRY(launch_add_channel_vec(w.x, speaker, t->spk, B, D, S, c.n_speaker, t->err, s));
    TRY(dbg(t->dbg_enc, 1 + t->enc.size(), w.x, (size_t)B * D * S));
    HIP_TRY(hipMemcpyAsync(st.enc_out, w.x, (size_t)B * D * S * sizeof(float), hipMemcpyDeviceToDevice, s));
    // duration predictor (duration.py:29-48): conv -> relu -> LN -> conv(pad 1) -> relu -> LN -> linear
    const int NF = c.dp_filter;
    TRY(conv_launch(t->dp0.get(), w.x, nullptr, w.f, B, S, EPI_STORE, 1.f, s, rows_of(src_len)));
    HIP_TRY(launch_layernorm(w.f, t->ln0_w, t->ln0_b, w.n, B, NF, S, 1, s));
    TRY(conv_launch(t->dp1.get(), w.n, nullptr, w.f, B, S, EPI_STORE, 1.f, s, rows_of(src_len)));
    HIP_TRY(launch_layernorm(w.f, t->ln1_w, t->ln1_b, w.n, B, NF, S, 1, s));
    TRY(conv_launch(t->dp_proj.get(), w.n, nullptr, w.o, B, S, EPI_STORE, 1.f, s));  // (B,1,S)
    HIP_TRY(launch_durations(w.o, src_mask, log_dur, dur, st.cum, st.out_len, B, S, src_len, t->err, s));
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
    HIP_TRY(launch_length_regulate(st.enc_out + (size_t)row0 * D * S, st.cum + (size_t)row0 * S, st.out_len + row0, t->pe, w.x, tgt_mask, B, S, L, D,
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
        HIP_TRY(launch_argmax_guard(w.logits, ids, B, V, L, t->err, t->guard, on ? glist : nullptr, on ? gstat : nullptr, row0, r, s));
    }
    if (logits) HIP_TRY(launch_transpose_cf_to_cl(w.logits, logits, B, V, L, s));
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
    HIP_TRY(launch_dur_prefix(dur, st.cum, st.out_len, B, S, t->err, src_len, s));
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
    HIP_TRY(launch_transpose_cf_to_cl(seq, w.seq_cf, B, S, D, s));
    HIP_TRY(launch_dur_prefix(dur, w.cum, w.lens, B, S, nullptr, nullptr, s));
    HIP_TRY(launch_length_regulate(w.seq_cf, w.cum, w.lens, w.zero, w.out_cf, mask, B, S, L, D, nullptr, 1, 0, 0, s));
    HIP_TRY(launch_transpose_cf_to_cl(w.out_cf, out, B, D, L, s));
    HIP_TRY(hipMemcpyAsync(out_lens, w.lens, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    return PARROT_OK;
}

extern "C" int parrot_tte_status_peek_async(parrot_tte_t* t, int32_t* dst_dev, void* stream) { return peek_async(t ? t->err.p : nullptr, dst_dev, (hipStream_t)stream, "tte_status_peek"); }
extern "C" int parrot_tte_status_async(parrot_tte_t* t, int32_t* dst_dev, void* stream) { return t ? status_async(t->err, dst_dev, (hipStream_t)stream) : PARROT_E_INVALID; }
// Tie-guard statistics of the last decode, copied to dst_dev[0..2] (device memory) on `stream` without synchronising:
// {positions whose top-2 logit margin was below the guard, ids changed by the fp64 re-evaluation of the head, the smallest
// margin of the call as float bits}
extern "C" int parrot_tte_guard_stats_async(parrot_tte_t* t, int32_t* dst_dev, void* stream) {
    if (!t || !dst_dev) return fail(PARROT_E_INVALID, "tte_guard_stats: null argument");
    if (!t->gstat) {
        HIP_TRY(hipMemsetAsync(dst_dev, 0, 3 * sizeof(int), (hipStream_t)stream));
        return PARROT_OK;
    }
    HIP_TRY(launch_guard_stats_sum(t->gstat, t->lanes_used, dst_dev, (hipStream_t)stream));
    return PARROT_OK;
}
// Refined (fp64-evaluated, rounded to fp32) logits of the guarded positions of the last decode: logits_dev (max_n x V floats) and
// their (b, t) pairs list_dev (2 max_n ints), device memory, no synchronisation; the count is guard_stats[0] (at most 256 per decoder lane).
extern "C" int parrot_tte_guard_logits(parrot_tte_t* t, float* logits_dev, int32_t* list_dev, int32_t max_n, void* stream) {
    if (!t || !logits_dev || !list_dev || max_n <= 0) return fail(PARROT_E_INVALID, "tte_guard_logits: null argument");
    if (!t->gref) return fail(PARROT_E_UNSUPPORTED, "tte_guard_logits: the tie guard of this handle is off");
    HIP_TRY(launch_guard_gather(t->gref, t->glist, t->gstat, t->lanes_used, t->cfg.n_codes, max_n, logits_dev, list_dev, (hipStream_t)stream));
    return PARROT_OK;
}
static int tte_status(int status) { return model_status("tte", status); }
extern "C" int parrot_tte_check(parrot_tte_t* t, void* stream) { return t ? check_flag(t->err, (hipStream_t)stream, tte_status) : PARROT_E_INVALID; }
