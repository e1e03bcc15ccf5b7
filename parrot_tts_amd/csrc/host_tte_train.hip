// host_tte_train.hip -- training the text-to-unit model: the teacher-forced forward with dropout and the full backward as two
// stateless calls (kernels: tte_train.h / tu_tte_train.hip; the matrix products: train_gemm_host.h, attn.h).  No handle, no packed
// weights, no host copy and no synchronisation: every weight is read from the device pointer it is given, in torch's layout.
// Activations are channel-last (B, T, C) throughout, so a Linear is one tap_gemm over all B T rows and a conv one per batch row.
#include "host_common.h"

#include <algorithm>
#include <cmath>
#include <string>

#include "train_gemm_host.h"
#include "tte_train.h"

using namespace parrot;

namespace {

constexpr int ML = PARROT_TTE_TRAIN_MAX_LAYERS;
constexpr int TTE_MAX_TAPS = 9;  // the FFN's widest kernel here (tap_gemm_kernel itself takes TG_MAX_TAPS)
static_assert(TTE_MAX_TAPS <= TG_MAX_TAPS, "one slot per tap");

struct Dims {
    int B, S, L, D, F, K1, K2, NF, DK, V, vocab, nspk, He, Hd, Le, Ld, Tm;
};
Dims dims(const parrot_tte_train_cfg& c, int B, int S, int L) {
    const parrot_tte_cfg& t = c.tte;
    return Dims{B, S, L, t.d_model, t.n_filter_ffn, t.ffn_k1, t.ffn_k2, t.dp_filter, t.dp_kernel, t.n_codes, t.vocab, t.n_speaker > 1 ? t.n_speaker : 0,
                t.enc_heads, t.dec_heads, t.enc_layers, t.dec_layers, std::max(S, L)};
}

struct BlockSaved {
    float *mean1, *rstd1, *ln1, *qkv0, *qkv1, *P, *ctx, *o1, *h, *mean2, *rstd2, *ln2, *f1, *y;
};
// What the forward keeps for the backward: per FFT block the two LayerNorms' statistics and outputs, both projections of q, k, v,
// the softmax probabilities BEFORE dropout (B, H, T, T), the context, the first output projection, the attention residual, the FFN's
// hidden activations and the block's output; the embedded input, the encoder output, the duration predictor's two ReLU outputs with
// their LayerNorm statistics and dropped outputs, the decoder input and the duration prefix sums.  Dropout masks are not kept.
struct Saved {
    float* emb;
    BlockSaved enc[ML], dec[ML];
    float *enc_out, *c0, *m0, *r0, *d0, *c1, *m1, *r1, *d1, *dec_in;
    int32_t* cum;
};
BlockSaved block_saved(Arena& ar, const Dims& d, int T, int H) {
    const size_t R = (size_t)d.B * T, D = d.D;
    BlockSaved b{};
    b.mean1 = ar.take<float>(R); b.rstd1 = ar.take<float>(R); b.ln1 = ar.take<float>(R * D);
    b.qkv0 = ar.take<float>(R * 3 * D); b.qkv1 = ar.take<float>(R * 3 * D);
    b.P = ar.take<float>(R * H * T);
    b.ctx = ar.take<float>(R * D); b.o1 = ar.take<float>(R * D); b.h = ar.take<float>(R * D);
    b.mean2 = ar.take<float>(R); b.rstd2 = ar.take<float>(R); b.ln2 = ar.take<float>(R * D);
    b.f1 = ar.take<float>(R * d.F); b.y = ar.take<float>(R * D);
    return b;
}
Saved saved_layout(Arena& ar, const Dims& d) {
    const size_t RS = (size_t)d.B * d.S, RL = (size_t)d.B * d.L;
    Saved sv{};
    sv.emb = ar.take<float>(RS * d.D);
    for (int i = 0; i < d.Le; ++i) sv.enc[i] = block_saved(ar, d, d.S, d.He);
    sv.enc_out = ar.take<float>(RS * d.D);
    sv.c0 = ar.take<float>(RS * d.NF); sv.m0 = ar.take<float>(RS); sv.r0 = ar.take<float>(RS); sv.d0 = ar.take<float>(RS * d.NF);
    sv.c1 = ar.take<float>(RS * d.NF); sv.m1 = ar.take<float>(RS); sv.r1 = ar.take<float>(RS); sv.d1 = ar.take<float>(RS * d.NF);
    sv.dec_in = ar.take<float>(RL * d.D);
    for (int i = 0; i < d.Ld; ++i) sv.dec[i] = block_saved(ar, d, d.L, d.Hd);
    sv.cum = ar.take<int32_t>((size_t)d.B * (d.S + 1));
    return sv;
}
size_t saved_bytes(const Dims& d) {
    Arena ar(nullptr, 0);
    (void)saved_layout(ar, d);
    return align_up(ar.off, 256);
}
size_t part_floats_for(const Dims& d) {  // the weight-gradient partials of the largest layer, every layer sized for B Tm rows
    const size_t D = d.D, F = d.F, NF = d.NF;
    const int R = d.B * d.Tm;
    return std::max({wgrad_part_floats(R, 3 * D * D, 1), wgrad_part_floats(R, F * D, d.K1), wgrad_part_floats(R, D * F, d.K2),
                     wgrad_part_floats(R, NF * D, d.DK), wgrad_part_floats(R, NF * NF, d.DK), wgrad_part_floats(R, (size_t)d.V * D, 1)});
}
// One workspace layout for both calls.  pd, t0 and ld_raw serve every call; after them the region of an eval forward's `saved` (used
// only when the caller keeps nothing: training = 0, saved = NULL) and the backward's own buffers share the same bytes -- no call uses
// both -- so the workspace is the common part plus the larger of the two.
struct Scratch {
    float *pd, *t0, *ld_raw;  // P after dropout (B, H, Tm, Tm); a (B Tm, D) temporary; the duration head before masking
    char* saved;              // saved_bytes: where an eval forward keeps what a training one hands to the caller
    float *ga, *gb, *ge, *ge2, *gf, *gqkv1, *gqkv0, *gctx, *go1, *gln, *tmp, *dP, *zl, *zd, *part;
    double* colpart;
    size_t part_floats;
};
Scratch scratch_layout(Arena& ar, const Dims& d) {
    const size_t R = (size_t)d.B * d.Tm, D = d.D, H = std::max(d.He, d.Hd);
    const size_t W = std::max({D, (size_t)d.F, (size_t)d.NF});
    const size_t chunks = (size_t)wgrad_chunks(d.B * d.Tm);
    Scratch w{};
    w.pd = ar.take<float>(R * H * d.Tm);
    w.t0 = ar.take<float>(R * D);
    w.ld_raw = ar.take<float>((size_t)d.B * d.S);
    const size_t common = ar.off;
    w.saved = ar.take<char>(saved_bytes(d));
    const size_t eval_end = ar.off;
    ar.off = common;  // the backward's buffers lie over the eval forward's `saved`
    w.ga = ar.take<float>(R * D); w.gb = ar.take<float>(R * D);
    w.ge = ar.take<float>((size_t)d.B * d.S * D); w.ge2 = ar.take<float>((size_t)d.B * d.S * D);
    w.gf = ar.take<float>(R * W);
    w.gqkv1 = ar.take<float>(R * 3 * D); w.gqkv0 = ar.take<float>(R * 3 * D);
    w.gctx = ar.take<float>(R * D); w.go1 = ar.take<float>(R * D);
    w.gln = ar.take<float>(R * W); w.tmp = ar.take<float>(R * W);
    w.dP = ar.take<float>(R * H * d.Tm);
    w.zl = ar.take<float>((size_t)d.B * d.L * d.V);
    w.zd = ar.take<float>((size_t)d.B * d.S);
    w.part_floats = part_floats_for(d);
    w.part = ar.take<float>(w.part_floats);
    w.colpart = ar.take<double>(chunks * std::max({3 * D, (size_t)d.F, (size_t)d.NF, (size_t)d.V}));
    if (ar.off < eval_end) {
        if (ar.base && eval_end > ar.cap) ar.ok = false;
        ar.off = eval_end;
    }
    return w;
}

bool cfg_quiet_ok(const parrot_tte_train_cfg* c, int B, int S, int L) {
    if (!c) return false;
    const parrot_tte_cfg& t = c->tte;
    if (t.d_model < 1 || t.n_filter_ffn < 1 || t.dp_filter < 1 || t.vocab < 1 || t.n_codes < 1 || t.max_len < 1) return false;
    if (t.enc_layers < 0 || t.dec_layers < 0 || t.enc_layers > ML || t.dec_layers > ML) return false;
    if (t.enc_heads < 1 || t.dec_heads < 1 || t.d_model % t.enc_heads || t.d_model % t.dec_heads) return false;
    if (t.ffn_k1 < 1 || t.ffn_k2 < 1 || !(t.ffn_k1 & 1) || !(t.ffn_k2 & 1) || t.ffn_k1 > TTE_MAX_TAPS || t.ffn_k2 > TTE_MAX_TAPS || t.dp_kernel != 3) return false;
    if (!(c->p_enc >= 0.f && c->p_enc <= 1.f && c->p_dec >= 0.f && c->p_dec <= 1.f && c->p_dp >= 0.f && c->p_dp <= 1.f)) return false;
    if (B < 1 || S < 1 || L < 1) return false;
    const long Tm = std::max(S, L), H = std::max(t.enc_heads, t.dec_heads);
    if ((long)B * H > 65535 || (long)B * Tm > 0x3fffffffL || (long)wgrad_chunks((int)(B * Tm)) * TTE_MAX_TAPS > 65535) return false;
    return true;
}
int cfg_ok(const parrot_tte_train_cfg* c, int B, int S, int L, const std::string& who) {
    if (!cfg_quiet_ok(c, B, S, L))
        return fail(PARROT_E_INVALID, who + ": shape outside the limits (positive sizes, at most 16 layers per stack, d_model a multiple of the heads, "
                                            "odd FFN kernels of at most 9 taps, duration kernel 3, 0 <= p <= 1, B x heads <= 65535, B max(S, L) <= 1 863 936)");
    if (std::max(S, L) >= c->tte.max_len) return fail(PARROT_E_RANGE, who + ": index " + std::to_string(std::max(S, L)) + " is out of bounds for pos_emb.pe with max_len " + std::to_string(c->tte.max_len));
    return PARROT_OK;
}
int weights_ok(const parrot_tte_train_cfg* c, const parrot_tte_dev_weights* w, const std::string& who) {
    bool ok = w->pe && w->tok_emb && w->dp_conv0_w && w->dp_conv0_b && w->dp_ln0_w && w->dp_ln0_b && w->dp_conv1_w && w->dp_conv1_b && w->dp_ln1_w &&
              w->dp_ln1_b && w->dp_proj_w && w->dp_proj_b && w->head_w && w->head_b && (c->tte.n_speaker <= 1 || w->speaker_emb);
    auto blk = [&](const parrot_fft_weights& f) {
        return f.qkv && f.in_proj && f.out_proj && f.wo && f.conv1_w && f.conv1_b && f.conv2_w && f.conv2_b && f.attn_norm_w && f.attn_norm_b &&
               f.conv_norm_w && f.conv_norm_b;
    };
    for (int i = 0; i < c->tte.enc_layers; ++i) ok = ok && blk(w->enc[i]);
    for (int i = 0; i < c->tte.dec_layers; ++i) ok = ok && blk(w->dec[i]);
    return ok ? PARROT_OK : fail(PARROT_E_INVALID, who + ": null weight");
}

// ---- the matrix products, by shape (train_gemm_host.h, channel-last; a Linear: one batch row of all B T rows) -----------------
// Y (rows, out; row stride ldy) = X (rows, in; ldx) W^T + bias, W (out, in)
int lin(const float* W, const float* X, long ldx, float* Y, long ldy, int out, int in, long rows, const float* bias, hipStream_t s) {
    Epi e;
    e.bias0 = bias;
    return conv_fwd(ConvW{W, out, in, 1, 1, 0}, X, chan_last((int)rows, ldx), Y, chan_last((int)rows, ldy), 1, (int)rows, e, s);
}
// dX (rows, in; ldx) = dY (rows, out; ldy) W
int lin_dx(const float* W, const float* dY, long ldy, float* dX, long ldx, int out, int in, long rows, hipStream_t s) {
    return conv_dx(ConvW{W, out, in, 1, 1, 0}, dY, chan_last((int)rows, ldy), dX, chan_last((int)rows, ldx), 1, (int)rows, Epi(), s);
}
// dW[m][k][j] = sum_(b, t) dY[b][t][m] X[b][t + j - pad][k], taps in groups that fit the partial buffer; kk = 1, B = 1: a Linear
int conv_dw(const float* dY, long ldy, const float* X, long ldx, float* dW, int cout, int cin, int kk, int pad, int B, int T, const Scratch& w,
            hipStream_t s) {
    if (!dW) return PARROT_OK;
    return parrot::conv_dw(ConvW{nullptr, cout, cin, kk, 1, pad}, dY, chan_last(T, ldy), X, chan_last(T, ldx), dW, B, T, w.part, w.part_floats, s);
}
// Y (B, T, cout) = act(conv1d(X (B, T, cin), W (cout, cin, kk), padding = pad) + bias)
int conv(const float* W, const float* bias, const float* X, float* Y, int cout, int cin, int kk, int pad, int B, int T, int relu, hipStream_t s) {
    Epi e;
    e.bias0 = bias; e.relu = relu;
    return conv_fwd(ConvW{W, cout, cin, kk, 1, pad}, X, chan_last(T, cin), Y, chan_last(T, cout), B, T, e, s);
}
// dX[b][t][k] = sum_j sum_m W[m][k][j] dY[b][t - (j - pad)][m]
int conv_dx(const float* W, const float* dY, float* dX, int cout, int cin, int kk, int pad, int B, int T, hipStream_t s) {
    return parrot::conv_dx(ConvW{W, cout, cin, kk, 1, pad}, dY, chan_last(T, cout), dX, chan_last(T, cin), B, T, Epi(), s);
}
int colsum(const float* src, long rows, int M, float* out, const Scratch& w, hipStream_t s) {
    return out ? parrot::colsum(src, rows, M, M, w.colpart, out, nullptr, s) : PARROT_OK;
}
// the attention's batched products: operand (b, h) of an array of row stride ld lies at b T ld + h hd; of P at (b H + h) T T
BgemmTrainParams bg(const float* A, long a_sk, long a_sm, long a_zb, long a_zh, const float* Bm, long b_sk, long b_sn, long b_zb, long b_zh, float* C,
                    long c_zb, long c_zh, long ldc, int M, int N, int K, int H, float alpha) {
    BgemmTrainParams p{};
    p.A = A; p.a_sk = a_sk; p.a_sm = a_sm; p.a_zb = a_zb; p.a_zh = a_zh;
    p.B = Bm; p.b_sk = b_sk; p.b_sn = b_sn; p.b_zb = b_zb; p.b_zh = b_zh;
    p.C = C; p.c_zb = c_zb; p.c_zh = c_zh; p.ldc = ldc;
    p.M = M; p.N = N; p.K = K; p.H = H; p.alpha = alpha;
    return p;
}

// ---- one FFT block (modules/fft.py:94-100) ---------------------------------------------------------------------------------
int block_fwd(const Dims& d, const parrot_fft_weights& f, const float* x, const uint8_t* kv, int T, int H, const BlockSaved& sv, const Scratch& w,
              DropArgs drop, hipStream_t s) {
    const int B = d.B, D = d.D, hd = D / H;
    const long R = (long)B * T, D3 = 3L * D, TT = (long)T * T;
    HIP_TRY(tt_launch_ln_fwd(x, f.attn_norm_w, f.attn_norm_b, sv.ln1, sv.mean1, sv.rstd1, R, D, s));
    TRY(lin(f.qkv, sv.ln1, D, sv.qkv0, D3, 3 * D, D, R, nullptr, s));
    for (int i = 0; i < 3; ++i) TRY(lin(f.in_proj + (size_t)i * D * D, sv.qkv0 + i * D, D3, sv.qkv1 + i * D, D3, D, D, R, nullptr, s));
    const float alpha = (float)std::sqrt(1.0 / (double)hd);
    HIP_TRY(tt_launch_bgemm(bg(sv.qkv1, 1, D3, T * D3, hd, sv.qkv1 + D, 1, D3, T * D3, hd, sv.P, H * TT, TT, T, T, T, hd, H, alpha), B * H, s));
    float* pd = drop.p > 0.f ? w.pd : nullptr;
    HIP_TRY(tt_launch_softmax_fwd(sv.P, pd, kv, R * H, T, H * T, drop, s));
    HIP_TRY(tt_launch_bgemm(bg(pd ? pd : sv.P, 1, T, H * TT, TT, sv.qkv1 + 2 * D, D3, 1, T * D3, hd, sv.ctx, (long)T * D, hd, D, T, hd, T, H, 1.f), B * H, s));
    TRY(lin(f.out_proj, sv.ctx, D, sv.o1, D, D, D, R, nullptr, s));
    TRY(lin(f.wo, sv.o1, D, w.t0, D, D, D, R, nullptr, s));
    HIP_TRY(tt_launch_add(x, w.t0, sv.h, (size_t)R * D, s));
    HIP_TRY(tt_launch_ln_fwd(sv.h, f.conv_norm_w, f.conv_norm_b, sv.ln2, sv.mean2, sv.rstd2, R, D, s));
    TRY(conv(f.conv1_w, f.conv1_b, sv.ln2, sv.f1, d.F, D, d.K1, (d.K1 - 1) / 2, B, T, 1, s));
    TRY(conv(f.conv2_w, f.conv2_b, sv.f1, w.t0, D, d.F, d.K2, (d.K2 - 1) / 2, B, T, 0, s));
    HIP_TRY(tt_launch_add(sv.h, w.t0, sv.y, (size_t)R * D, s));
    return PARROT_OK;
}
// in: w.ga = the gradient at the block's output; out: w.ga = the gradient at its input x
int block_bwd(const Dims& d, const parrot_fft_weights& f, const parrot_fft_grads& g, const float* x, int T, int H, const BlockSaved& sv, const Scratch& w,
              DropArgs drop, hipStream_t s) {
    const int B = d.B, D = d.D, F = d.F, hd = D / H;
    const long R = (long)B * T, D3 = 3L * D, TT = (long)T * T;
    // FFN: conv2, ReLU, conv1
    TRY(colsum(w.ga, R, D, g.conv2_b, w, s));
    TRY(conv_dw(w.ga, D, sv.f1, F, g.conv2_w, D, F, d.K2, (d.K2 - 1) / 2, B, T, w, s));
    TRY(conv_dx(f.conv2_w, w.ga, w.gf, D, F, d.K2, (d.K2 - 1) / 2, B, T, s));
    HIP_TRY(tt_launch_relu_bwd(sv.f1, w.gf, w.gf, (size_t)R * F, s));
    TRY(colsum(w.gf, R, F, g.conv1_b, w, s));
    TRY(conv_dw(w.gf, F, sv.ln2, D, g.conv1_w, F, D, d.K1, (d.K1 - 1) / 2, B, T, w, s));
    TRY(conv_dx(f.conv1_w, w.gf, w.gln, F, D, d.K1, (d.K1 - 1) / 2, B, T, s));
    HIP_TRY(tt_launch_ln_bwd(w.gln, sv.h, f.conv_norm_w, sv.mean2, sv.rstd2, w.ga, w.gb, w.tmp, R, D, 0, s));  // gb = d h
    TRY(colsum(w.tmp, R, D, g.conv_norm_w, w, s));
    TRY(colsum(w.gln, R, D, g.conv_norm_b, w, s));
    // attention: wo, out_proj, the core, in_proj, qkv
    TRY(conv_dw(w.gb, D, sv.o1, D, g.wo, D, D, 1, 0, 1, (int)R, w, s));
    TRY(lin_dx(f.wo, w.gb, D, w.go1, D, D, D, R, s));
    TRY(conv_dw(w.go1, D, sv.ctx, D, g.out_proj, D, D, 1, 0, 1, (int)R, w, s));
    TRY(lin_dx(f.out_proj, w.go1, D, w.gctx, D, D, D, R, s));
    const float alpha = (float)std::sqrt(1.0 / (double)hd);
    const float* v = sv.qkv1 + 2 * D;
    // d Pd[tq][tk] = sum_c dctx[tq][c] v[tk][c]
    HIP_TRY(tt_launch_bgemm(bg(w.gctx, 1, D, (long)T * D, hd, v, 1, D3, T * D3, hd, w.dP, H * TT, TT, T, T, T, hd, H, 1.f), B * H, s));
    const float* pd = sv.P;
    if (drop.p > 0.f) {  // the probabilities after dropout again, from the kept ones and the regenerated mask
        HIP_TRY(tt_launch_dropout(sv.P, w.pd, (size_t)R * H * T, drop, s));
        pd = w.pd;
    }
    // dv[tk][c] = sum_tq Pd[tq][tk] dctx[tq][c]
    HIP_TRY(tt_launch_bgemm(bg(pd, T, 1, H * TT, TT, w.gctx, D, 1, (long)T * D, hd, w.gqkv1 + 2 * D, T * D3, hd, D3, T, hd, T, H, 1.f), B * H, s));
    HIP_TRY(tt_launch_softmax_bwd(sv.P, w.dP, R * H, T, drop, s));  // dP <- dS
    // dq[tq][c] = alpha sum_tk dS[tq][tk] k[tk][c];  dk[tk][c] = alpha sum_tq dS[tq][tk] q[tq][c]
    HIP_TRY(tt_launch_bgemm(bg(w.dP, 1, T, H * TT, TT, sv.qkv1 + D, D3, 1, T * D3, hd, w.gqkv1, T * D3, hd, D3, T, hd, T, H, alpha), B * H, s));
    HIP_TRY(tt_launch_bgemm(bg(w.dP, T, 1, H * TT, TT, sv.qkv1, D3, 1, T * D3, hd, w.gqkv1 + D, T * D3, hd, D3, T, hd, T, H, alpha), B * H, s));
    for (int i = 0; i < 3; ++i) {
        TRY(conv_dw(w.gqkv1 + i * D, D3, sv.qkv0 + i * D, D3, g.in_proj ? g.in_proj + (size_t)i * D * D : nullptr, D, D, 1, 0, 1, (int)R, w, s));
        TRY(lin_dx(f.in_proj + (size_t)i * D * D, w.gqkv1 + i * D, D3, w.gqkv0 + i * D, D3, D, D, R, s));
    }
    TRY(conv_dw(w.gqkv0, D3, sv.ln1, D, g.qkv, 3 * D, D, 1, 0, 1, (int)R, w, s));
    TRY(lin_dx(f.qkv, w.gqkv0, D3, w.gln, D, 3 * D, D, R, s));
    HIP_TRY(tt_launch_ln_bwd(w.gln, x, f.attn_norm_w, sv.mean1, sv.rstd1, w.gb, w.ga, w.tmp, R, D, 0, s));  // ga = d x
    TRY(colsum(w.tmp, R, D, g.attn_norm_w, w, s));
    TRY(colsum(w.gln, R, D, g.attn_norm_b, w, s));
    return PARROT_OK;
}

DropArgs drop_args(float p, uint64_t seed, uint64_t offset, int site, int training) { return DropArgs{training ? p : 0.f, seed, offset, site}; }

int poison_grad(float* p, size_t n, hipStream_t s) { return p ? poison(p, n * sizeof(float), s) : PARROT_OK; }
int poison_block_grads(const parrot_fft_grads& g, const Dims& d, hipStream_t s) {
    const size_t D = d.D, F = d.F;
    TRY(poison_grad(g.qkv, 3 * D * D, s)); TRY(poison_grad(g.in_proj, 3 * D * D, s)); TRY(poison_grad(g.out_proj, D * D, s)); TRY(poison_grad(g.wo, D * D, s));
    TRY(poison_grad(g.conv1_w, F * D * d.K1, s)); TRY(poison_grad(g.conv1_b, F, s)); TRY(poison_grad(g.conv2_w, D * F * d.K2, s)); TRY(poison_grad(g.conv2_b, D, s));
    TRY(poison_grad(g.attn_norm_w, D, s)); TRY(poison_grad(g.attn_norm_b, D, s)); TRY(poison_grad(g.conv_norm_w, D, s)); TRY(poison_grad(g.conv_norm_b, D, s));
    return PARROT_OK;
}

}  // namespace

extern "C" size_t parrot_tte_train_saved_bytes(const parrot_tte_train_cfg* cfg, int32_t B, int32_t S, int32_t L) {
    return cfg_quiet_ok(cfg, B, S, L) ? saved_bytes(dims(*cfg, B, S, L)) : 0;
}
extern "C" size_t parrot_tte_train_workspace_bytes(const parrot_tte_train_cfg* cfg, int32_t B, int32_t S, int32_t L) {
    if (!cfg_quiet_ok(cfg, B, S, L)) return 0;
    Arena ar(nullptr, 0);
    (void)scratch_layout(ar, dims(*cfg, B, S, L));
    return align_up(ar.off, 256);
}

extern "C" int parrot_tte_train_forward(const parrot_tte_train_cfg* cfg, const parrot_tte_dev_weights* wt, const int64_t* phones, const uint8_t* src_mask,
                                        const int64_t* speaker, const int64_t* duration, const uint8_t* tgt_mask, int32_t B, int32_t S, int32_t L,
                                        int32_t training, uint64_t seed, uint64_t offset, float* logits, float* log_dur, void* saved, void* ws,
                                        size_t ws_bytes, void* stream) {
    const std::string who = "tte_train_forward";
    if (!cfg || !wt || !phones || !src_mask || !duration || !tgt_mask || !logits || !log_dur || !ws) return fail(PARROT_E_INVALID, who + ": null argument");
    TRY(cfg_ok(cfg, B, S, L, who));
    TRY(weights_ok(cfg, wt, who));
    if (cfg->tte.n_speaker > 1 && !speaker) return fail(PARROT_E_INVALID, who + ": the model has a speaker embedding: speaker ids are needed");
    if (training && !saved) return fail(PARROT_E_INVALID, who + ": training needs the saved buffer");
    hipStream_t s = (hipStream_t)stream;
    const Dims d = dims(*cfg, B, S, L);
    Arena ar(ws, ws_bytes);
    const Scratch w = scratch_layout(ar, d);
    if (!ar.ok) return fail(PARROT_E_NOMEM, who + ": workspace too small");
    const size_t sv_bytes = saved_bytes(d);
    if (poison_word()) {
        TRY(poison(ws, ws_bytes, s));
        if (saved) TRY(poison(saved, sv_bytes, s));
        TRY(poison(logits, (size_t)B * L * d.V * sizeof(float), s));
        TRY(poison(log_dur, (size_t)B * S * sizeof(float), s));
    }
    Arena sa(saved ? saved : (void*)w.saved, sv_bytes);
    const Saved sv = saved_layout(sa, d);
    const int D = d.D, NF = d.NF;
    const long RS = (long)B * S, RL = (long)B * L;
    // tok_emb + pe[S] (fft.py:18: the single row of the padded length), the encoder, the speaker embedding
    HIP_TRY(tt_launch_embed(phones, wt->tok_emb, wt->pe + (size_t)S * D, sv.emb, RS, D, d.vocab, s));
    const float* x = sv.emb;
    for (int i = 0; i < d.Le; ++i) {
        TRY(block_fwd(d, wt->enc[i], x, src_mask, S, d.He, sv.enc[i], w, drop_args(cfg->p_enc, seed, offset, 2 + i, training), s));
        x = sv.enc[i].y;
    }
    if (d.nspk) HIP_TRY(tt_launch_add_speaker(x, speaker, wt->speaker_emb, sv.enc_out, B, S, D, d.nspk, s));
    else HIP_TRY(hipMemcpyAsync(sv.enc_out, x, (size_t)RS * D * sizeof(float), hipMemcpyDeviceToDevice, s));
    // the duration predictor on the encoder output (duration.py:29-48): conv, ReLU, LayerNorm, dropout, twice; Linear; mask
    TRY(conv(wt->dp_conv0_w, wt->dp_conv0_b, sv.enc_out, sv.c0, NF, D, d.DK, (d.DK - 1) / 2, B, S, 1, s));
    HIP_TRY(tt_launch_ln_fwd(sv.c0, wt->dp_ln0_w, wt->dp_ln0_b, sv.d0, sv.m0, sv.r0, RS, NF, s));
    HIP_TRY(tt_launch_dropout(sv.d0, sv.d0, (size_t)RS * NF, drop_args(cfg->p_dp, seed, offset, 0, training), s));
    TRY(conv(wt->dp_conv1_w, wt->dp_conv1_b, sv.d0, sv.c1, NF, NF, d.DK, 1, B, S, 1, s));
    HIP_TRY(tt_launch_ln_fwd(sv.c1, wt->dp_ln1_w, wt->dp_ln1_b, sv.d1, sv.m1, sv.r1, RS, NF, s));
    HIP_TRY(tt_launch_dropout(sv.d1, sv.d1, (size_t)RS * NF, drop_args(cfg->p_dp, seed, offset, 1, training), s));
    TRY(lin(wt->dp_proj_w, sv.d1, NF, w.ld_raw, 1, 1, NF, RS, wt->dp_proj_b, s));
    HIP_TRY(tt_launch_mask(w.ld_raw, src_mask, log_dur, (size_t)RS, s));
    // the length regulator on the caller's durations, + pe[L], the decoder, the head
    HIP_TRY(tt_launch_dur_cum(duration, sv.cum, B, S, L, s));
    HIP_TRY(tt_launch_lr_fwd(sv.enc_out, sv.cum, wt->pe + (size_t)L * D, sv.dec_in, B, S, L, D, s));
    x = sv.dec_in;
    for (int i = 0; i < d.Ld; ++i) {
        TRY(block_fwd(d, wt->dec[i], x, tgt_mask, L, d.Hd, sv.dec[i], w, drop_args(cfg->p_dec, seed, offset, 2 + d.Le + i, training), s));
        x = sv.dec[i].y;
    }
    TRY(lin(wt->head_w, x, D, logits, d.V, d.V, D, RL, wt->head_b, s));
    return PARROT_OK;
}

extern "C" int parrot_tte_train_backward(const parrot_tte_train_cfg* cfg, const parrot_tte_dev_weights* wt, const int64_t* phones, const uint8_t* src_mask,
                                         const int64_t* speaker, const int64_t* duration, const uint8_t* tgt_mask, const void* saved,
                                         const float* grad_logits, const float* grad_log_dur, int32_t B, int32_t S, int32_t L, uint64_t seed,
                                         uint64_t offset, const parrot_tte_grads* gr, void* ws, size_t ws_bytes, void* stream) {
    const std::string who = "tte_train_backward";
    if (!cfg || !wt || !phones || !src_mask || !duration || !tgt_mask || !saved || !gr || !ws) return fail(PARROT_E_INVALID, who + ": null argument");
    TRY(cfg_ok(cfg, B, S, L, who));
    TRY(weights_ok(cfg, wt, who));
    if (cfg->tte.n_speaker > 1 && !speaker) return fail(PARROT_E_INVALID, who + ": the model has a speaker embedding: speaker ids are needed");
    hipStream_t s = (hipStream_t)stream;
    const Dims d = dims(*cfg, B, S, L);
    Arena ar(ws, ws_bytes);
    const Scratch w = scratch_layout(ar, d);
    if (!ar.ok) return fail(PARROT_E_NOMEM, who + ": workspace too small");
    const int D = d.D, NF = d.NF;
    const long RS = (long)B * S, RL = (long)B * L;
    if (poison_word()) {
        TRY(poison(ws, ws_bytes, s));
        TRY(poison_grad(gr->tok_emb, (size_t)d.vocab * D, s));
        if (d.nspk) TRY(poison_grad(gr->speaker_emb, (size_t)d.nspk * D, s));
        TRY(poison_grad(gr->dp_conv0_w, (size_t)NF * D * d.DK, s)); TRY(poison_grad(gr->dp_conv0_b, NF, s));
        TRY(poison_grad(gr->dp_ln0_w, NF, s)); TRY(poison_grad(gr->dp_ln0_b, NF, s));
        TRY(poison_grad(gr->dp_conv1_w, (size_t)NF * NF * d.DK, s)); TRY(poison_grad(gr->dp_conv1_b, NF, s));
        TRY(poison_grad(gr->dp_ln1_w, NF, s)); TRY(poison_grad(gr->dp_ln1_b, NF, s));
        TRY(poison_grad(gr->dp_proj_w, NF, s)); TRY(poison_grad(gr->dp_proj_b, 1, s));
        TRY(poison_grad(gr->head_w, (size_t)d.V * D, s)); TRY(poison_grad(gr->head_b, d.V, s));
        for (int i = 0; i < d.Le; ++i) TRY(poison_block_grads(gr->enc[i], d, s));
        for (int i = 0; i < d.Ld; ++i) TRY(poison_block_grads(gr->dec[i], d, s));
    }
    Arena sa(const_cast<void*>(saved), saved_bytes(d));
    const Saved sv = saved_layout(sa, d);
    if (!grad_logits) {  // a missing upstream gradient is a zero one
        HIP_TRY(hipMemsetAsync(w.zl, 0, (size_t)RL * d.V * sizeof(float), s));
        grad_logits = w.zl;
    }
    if (!grad_log_dur) {
        HIP_TRY(hipMemsetAsync(w.zd, 0, (size_t)RS * sizeof(float), s));
        grad_log_dur = w.zd;
    }
    // ---- head, decoder -----------------------------------------------------------------------------------------------------
    const float* dec_out = d.Ld ? sv.dec[d.Ld - 1].y : sv.dec_in;
    TRY(colsum(grad_logits, RL, d.V, gr->head_b, w, s));
    TRY(conv_dw(grad_logits, d.V, dec_out, D, gr->head_w, d.V, D, 1, 0, 1, (int)RL, w, s));
    TRY(lin_dx(wt->head_w, grad_logits, d.V, w.ga, D, d.V, D, RL, s));
    for (int i = d.Ld - 1; i >= 0; --i)
        TRY(block_bwd(d, wt->dec[i], gr->dec[i], i ? sv.dec[i - 1].y : sv.dec_in, L, d.Hd, sv.dec[i], w,
                      drop_args(cfg->p_dec, seed, offset, 2 + d.Le + i, 1), s));
    // ---- length regulator: every source position gets the sum of its segment -----------------------------------------------
    HIP_TRY(tt_launch_lr_bwd(w.ga, sv.cum, nullptr, w.ge, B, S, L, D, s));
    // ---- duration predictor, last to first ---------------------------------------------------------------------------------
    HIP_TRY(tt_launch_mask(grad_log_dur, src_mask, w.t0, (size_t)RS, s));  // t0 (B S): the gradient at the Linear's output
    TRY(colsum(w.t0, RS, 1, gr->dp_proj_b, w, s));
    TRY(conv_dw(w.t0, 1, sv.d1, NF, gr->dp_proj_w, 1, NF, 1, 0, 1, (int)RS, w, s));
    TRY(lin_dx(wt->dp_proj_w, w.t0, 1, w.gf, NF, 1, NF, RS, s));
    HIP_TRY(tt_launch_dropout(w.gf, w.gf, (size_t)RS * NF, drop_args(cfg->p_dp, seed, offset, 1, 1), s));
    HIP_TRY(tt_launch_ln_bwd(w.gf, sv.c1, wt->dp_ln1_w, sv.m1, sv.r1, nullptr, w.gln, w.tmp, RS, NF, 1, s));  // gln = d conv1's output
    TRY(colsum(w.tmp, RS, NF, gr->dp_ln1_w, w, s));
    TRY(colsum(w.gf, RS, NF, gr->dp_ln1_b, w, s));
    TRY(colsum(w.gln, RS, NF, gr->dp_conv1_b, w, s));
    TRY(conv_dw(w.gln, NF, sv.d0, NF, gr->dp_conv1_w, NF, NF, d.DK, 1, B, S, w, s));
    TRY(conv_dx(wt->dp_conv1_w, w.gln, w.gf, NF, NF, d.DK, 1, B, S, s));
    HIP_TRY(tt_launch_dropout(w.gf, w.gf, (size_t)RS * NF, drop_args(cfg->p_dp, seed, offset, 0, 1), s));
    HIP_TRY(tt_launch_ln_bwd(w.gf, sv.c0, wt->dp_ln0_w, sv.m0, sv.r0, nullptr, w.gln, w.tmp, RS, NF, 1, s));
    TRY(colsum(w.tmp, RS, NF, gr->dp_ln0_w, w, s));
    TRY(colsum(w.gf, RS, NF, gr->dp_ln0_b, w, s));
    TRY(colsum(w.gln, RS, NF, gr->dp_conv0_b, w, s));
    TRY(conv_dw(w.gln, NF, sv.enc_out, D, gr->dp_conv0_w, NF, D, d.DK, (d.DK - 1) / 2, B, S, w, s));
    TRY(conv_dx(wt->dp_conv0_w, w.gln, w.ge2, NF, D, d.DK, (d.DK - 1) / 2, B, S, s));
    HIP_TRY(tt_launch_add(w.ge, w.ge2, w.ga, (size_t)RS * D, s));  // ga = d encoder output
    // ---- speaker embedding, encoder, token embedding -----------------------------------------------------------------------
    if (d.nspk && gr->speaker_emb) HIP_TRY(tt_launch_embed_grad(speaker, w.ga, gr->speaker_emb, RS, S, D, d.nspk, -1, s));
    for (int i = d.Le - 1; i >= 0; --i)
        TRY(block_bwd(d, wt->enc[i], gr->enc[i], i ? sv.enc[i - 1].y : sv.emb, S, d.He, sv.enc[i], w, drop_args(cfg->p_enc, seed, offset, 2 + i, 1), s));
    if (gr->tok_emb) HIP_TRY(tt_launch_embed_grad(phones, w.ga, gr->tok_emb, RS, 1, D, d.vocab, cfg->pad_idx, s));
    return PARROT_OK;
}

extern "C" int parrot_tte_train_dropout_mask(uint64_t seed, uint64_t offset, int32_t site, int64_t n, float p, uint8_t* out_u8, void* stream) {
    if (!out_u8 || n < 1) return fail(PARROT_E_INVALID, "tte_train_dropout_mask: null or empty output");
    if (site < 0 || site > 255 || !(p >= 0.f && p <= 1.f)) return fail(PARROT_E_INVALID, "tte_train_dropout_mask: site outside [0, 255] or p outside [0, 1]");
    HIP_TRY(tt_launch_dropout_mask(out_u8, (size_t)n, DropArgs{p, seed, offset, site}, (hipStream_t)stream));
    return PARROT_OK;
}

// ---------------------------------------------------------------------------------------------
// Debug entry points (include/parrot_hip_debug.h): the kernels of tte_train.h alone, and conv_dw with a chosen tap group, on
// caller-owned dense buffers whose sizes follow from the dimensions given.  Nothing is launched before the sizes are checked.
// ---------------------------------------------------------------------------------------------
namespace {
bool drop_ok(float p, int site) { return p >= 0.f && p <= 1.f && site >= 0 && site <= 255; }
}  // namespace

extern "C" int parrot_debug_tte_ln_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int64_t rows,
                                       int32_t C, void* stream) {
    if (!x || !gamma || !beta || !y || !mean || !rstd) return fail(PARROT_E_INVALID, "debug_tte_ln_fwd: null argument");
    if (rows < 1 || C < 1 || rows > 0x3fffffffL) return fail(PARROT_E_INVALID, "debug_tte_ln_fwd: rows and C must be positive");
    HIP_TRY(tt_launch_ln_fwd(x, gamma, beta, y, mean, rstd, rows, C, (hipStream_t)stream));
    return PARROT_OK;
}
extern "C" int parrot_debug_tte_ln_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, const float* res,
                                       float* dx, float* dyxh, int64_t rows, int32_t C, int32_t relu_mask, void* stream) {
    if (!dy || !x || !gamma || !mean || !rstd || !dx || !dyxh) return fail(PARROT_E_INVALID, "debug_tte_ln_bwd: null argument");
    if (rows < 1 || C < 1 || rows > 0x3fffffffL) return fail(PARROT_E_INVALID, "debug_tte_ln_bwd: rows and C must be positive");
    HIP_TRY(tt_launch_ln_bwd(dy, x, gamma, mean, rstd, res, dx, dyxh, rows, C, relu_mask ? 1 : 0, (hipStream_t)stream));
    return PARROT_OK;
}
extern "C" int parrot_debug_tte_softmax_drop_fwd(float* scores, float* pd, const uint8_t* key_valid, int32_t B, int32_t H, int32_t T, float p,
                                                 uint64_t seed, uint64_t offset, int32_t site, void* stream) {
    if (!scores || !key_valid) return fail(PARROT_E_INVALID, "debug_tte_softmax_drop_fwd: null argument");
    if (B < 1 || H < 1 || T < 1 || (long)B * H * T > 0x3fffffffL || !drop_ok(p, site)) return fail(PARROT_E_INVALID, "debug_tte_softmax_drop_fwd: bad sizes, p or site");
    HIP_TRY(tt_launch_softmax_fwd(scores, pd, key_valid, (long)B * H * T, T, H * T, DropArgs{p, seed, offset, site}, (hipStream_t)stream));
    return PARROT_OK;
}
extern "C" int parrot_debug_tte_softmax_drop_bwd(const float* P, float* dP, int32_t B, int32_t H, int32_t T, float p, uint64_t seed, uint64_t offset,
                                                 int32_t site, void* stream) {
    if (!P || !dP) return fail(PARROT_E_INVALID, "debug_tte_softmax_drop_bwd: null argument");
    if (B < 1 || H < 1 || T < 1 || (long)B * H * T > 0x3fffffffL || !drop_ok(p, site)) return fail(PARROT_E_INVALID, "debug_tte_softmax_drop_bwd: bad sizes, p or site");
    HIP_TRY(tt_launch_softmax_bwd(P, dP, (long)B * H * T, T, DropArgs{p, seed, offset, site}, (hipStream_t)stream));
    return PARROT_OK;
}
extern "C" int parrot_debug_tte_dropout(const float* x, float* y, int64_t n, float p, uint64_t seed, uint64_t offset, int32_t site, void* stream) {
    if (!x || !y || n < 1 || !drop_ok(p, site)) return fail(PARROT_E_INVALID, "debug_tte_dropout: null argument, empty array, bad p or site");
    HIP_TRY(tt_launch_dropout(x, y, (size_t)n, DropArgs{p, seed, offset, site}, (hipStream_t)stream));
    return PARROT_OK;
}
extern "C" int parrot_debug_tte_lr_bwd(const float* dy, const int64_t* dur, const float* add, float* denc, int32_t* cum, int32_t B, int32_t S, int32_t L,
                                       int32_t D, void* stream) {
    if (!dy || !dur || !denc || !cum) return fail(PARROT_E_INVALID, "debug_tte_lr_bwd: null argument");
    if (B < 1 || B > 65535 || S < 1 || L < 1 || D < 1) return fail(PARROT_E_INVALID, "debug_tte_lr_bwd: B, S, L and D must be positive, B <= 65535");
    HIP_TRY(tt_launch_dur_cum(dur, cum, B, S, L, (hipStream_t)stream));
    HIP_TRY(tt_launch_lr_bwd(dy, cum, add, denc, B, S, L, D, (hipStream_t)stream));
    return PARROT_OK;
}
extern "C" int parrot_debug_tte_embed_grad(const int64_t* ids, const float* dx, float* dtab, int64_t rows, int32_t per, int32_t D, int32_t V,
                                           int32_t pad_idx, void* stream) {
    if (!ids || !dx || !dtab) return fail(PARROT_E_INVALID, "debug_tte_embed_grad: null argument");
    if (rows < 1 || per < 1 || D < 1 || V < 1 || V > 0x7fffffff / 2) return fail(PARROT_E_INVALID, "debug_tte_embed_grad: rows, per, D and V must be positive");
    HIP_TRY(tt_launch_embed_grad(ids, dx, dtab, rows, per, D, V, pad_idx, (hipStream_t)stream));
    return PARROT_OK;
}
namespace {
bool conv_dw_sizes_ok(int cout, int cin, int kk, int pad, int B, int T, int group) {
    return cout >= 1 && cin >= 1 && kk >= 1 && kk <= TTE_MAX_TAPS && pad >= 0 && pad < kk && B >= 1 && T >= 1 && (long)B * T <= 0x3fffffffL && group >= 1 &&
           group <= kk && (long)wgrad_chunks(B * T) * group <= 65535;
}
}  // namespace
extern "C" size_t parrot_debug_tte_conv_dw_workspace_bytes(int32_t cout, int32_t cin, int32_t kk, int32_t B, int32_t T, int32_t group) {
    return conv_dw_sizes_ok(cout, cin, kk, 0, B, T, group) ? (size_t)wgrad_chunks(B * T) * group * cout * cin * sizeof(float) : 0;
}
// dW (cout, cin, kk) from dY (B, T, cout) and X (B, T, cin) through conv_dw, the weight gradient of every conv and Linear of the
// training backward, with the partial buffer sized for `group` taps: group < kk takes the tap-group path (several wgrad launches,
// each reduced into its own taps of dW).
extern "C" int parrot_debug_tte_conv_dw(const float* dY, const float* X, float* dW, int32_t cout, int32_t cin, int32_t kk, int32_t pad, int32_t B,
                                        int32_t T, int32_t group, void* ws, size_t ws_bytes, void* stream) {
    if (!dY || !X || !dW || !ws) return fail(PARROT_E_INVALID, "debug_tte_conv_dw: null argument");
    if (!conv_dw_sizes_ok(cout, cin, kk, pad, B, T, group)) return fail(PARROT_E_INVALID, "debug_tte_conv_dw: sizes outside the limits (1 <= group <= kk <= 9, 0 <= pad < kk)");
    const size_t need = parrot_debug_tte_conv_dw_workspace_bytes(cout, cin, kk, B, T, group);
    if (ws_bytes < need) return fail(PARROT_E_INVALID, "debug_tte_conv_dw: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    if (poison_word()) TRY(poison(ws, need, s));
    Scratch w{};
    w.part = (float*)ws;
    w.part_floats = need / sizeof(float);
    return conv_dw(dY, cout, X, cin, dW, cout, cin, kk, pad, B, T, w, s);
}
