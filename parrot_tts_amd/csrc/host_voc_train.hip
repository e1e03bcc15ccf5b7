// host_voc_train.hip -- training the vocoder's generator: CodeGenerator.forward with weight norm attached and its full backward as
// two stateless calls (kernels: voc_train.h / tu_voc_train.hip; the matrix products: train_gemm_host.h).  No handle, no packed weights,
// no host copy and no synchronisation: every parameter is read from the device pointer it is given, in torch's layout.  Activations
// are channel-first (B, C, T) throughout, so a conv is one tap_gemm per batch row (grid z = B) and a transposed conv one per phase.
#include "host_common.h"

#include <algorithm>
#include <string>
#include <vector>

#include "train_gemm_host.h"
#include "tte_train.h"  // (borrowed: tt_launch_embed_grad alone, the fixed-order fp64 row scatter of both tables' gradients)
#include "voc_train.h"

using namespace parrot;

namespace {

constexpr float SLOPE = 0.1f, SLOPE_POST = 0.01f;  // LRELU_SLOPE (models.py:10) and F.leaky_relu's default (models.py:107)
constexpr int MAX_K = TG_MAX_TAPS;

struct LayerDesc {
    int cin, cout, k, dil, u, transposed;
    int Tin, Tout;
    int rows() const { return transposed ? cin : cout; }  // dim 0 of the weight
    ConvW conv(const float* W) const { return ConvW{W, cout, cin, k, dil, (k - 1) / 2 * dil}; }  // (not transposed: padding dil (k - 1) / 2)
    Lay in() const { return chan_first(cin, Tin); }
    Lay out() const { return chan_first(cout, Tout); }
    size_t len() const { return (size_t)(transposed ? cout : cin) * k; }
    size_t wsize() const { return (size_t)cin * cout * k; }
};
// Every layer in state_dict order: conv_pre, ups[0 .. S), rb[...] as parrot_voc_weights.rb_w indexes them, conv_post.
struct Dims {
    int B, U, E, multi, Cin0, C0, S, NK, ND, type, n_emb, n_spkr, per_rb;
    int C[PARROT_MAX_STAGES + 1], T[PARROT_MAX_STAGES + 1];  // channels and frames after stage i - 1 (index 0: conv_pre's output)
    std::vector<LayerDesc> L;  // 1 + S + S NK per_rb + 1
    size_t max_act, max_w;
    int n_layers() const { return (int)L.size(); }
    int up(int i) const { return 1 + i; }
    int rb(int i, int j, int c) const { return 1 + S + (i * NK + j) * per_rb + c; }
    int post() const { return 1 + S + S * NK * per_rb; }
};

bool cfg_quiet_ok(const parrot_voc_cfg* c, long B, long U) {
    if (!c) return false;
    if (B < 1 || B > 65535 || U < 1 || U > 0x3fffffffL) return false;
    if (c->num_embeddings < 1 || c->embedding_dim < 1 || c->upsample_initial_channel < 1) return false;
    if (c->multispkr && c->n_spkr < 1) return false;
    if (c->model_in_dim != c->embedding_dim * (c->multispkr ? 2 : 1)) return false;
    if (c->n_stages < 1 || c->n_stages > PARROT_MAX_STAGES || c->n_kernels < 1 || c->n_kernels > PARROT_MAX_KERNELS) return false;
    if (c->n_dil < 1 || c->n_dil > PARROT_MAX_DIL || (c->resblock_type != 1 && c->resblock_type != 2)) return false;
    if ((c->upsample_initial_channel >> c->n_stages) < 1) return false;
    long T = U, maxk = 7;
    const long lim = 0x3fffffffL;
    if (B * U * std::max<long>(c->model_in_dim, c->upsample_initial_channel) > lim) return false;
    for (int i = 0; i < c->n_stages; ++i) {
        const long u = c->upsample_rates[i], k = c->upsample_kernel_sizes[i];
        if (u < 1 || k < u || k > MAX_K) return false;
        T = (T - 1) * u - 2 * ((k - u) / 2) + k;
        if (T < 1 || B * T * (c->upsample_initial_channel >> i) > lim) return false;
        maxk = std::max(maxk, k);
    }
    for (int j = 0; j < c->n_kernels; ++j) {
        const long k = c->resblock_kernel_sizes[j];
        if (k < 1 || !(k & 1) || k > MAX_K) return false;
        maxk = std::max(maxk, k);
        for (int m = 0; m < c->n_dil; ++m) {
            const long dl = c->resblock_dilation_sizes[j][m];
            if (dl < 1 || dl * k > lim) return false;
        }
    }
    if ((B * T + TG_RCHUNK - 1) / TG_RCHUNK * maxk > 65535) return false;
    return true;
}
int cfg_ok(const parrot_voc_cfg* c, int B, int U, const std::string& who) {
    if (!cfg_quiet_ok(c, B, U))
        return fail(PARROT_E_INVALID, who + ": shape outside the limits (positive sizes, U >= 1, B <= 65535, model_in_dim == embedding_dim (1 + multispkr), "
                                            "odd resblock kernels and upsample kernels of at most 11 taps with rate <= kernel, activations below 2^30 elements, "
                                            "ceil(B T / 256) x taps <= 65535)");
    return PARROT_OK;
}

Dims dims(const parrot_voc_cfg& c, int B, int U) {
    Dims d{};
    d.B = B; d.U = U; d.E = c.embedding_dim; d.multi = c.multispkr ? 1 : 0; d.Cin0 = c.model_in_dim; d.C0 = c.upsample_initial_channel;
    d.S = c.n_stages; d.NK = c.n_kernels; d.ND = c.n_dil; d.type = c.resblock_type; d.n_emb = c.num_embeddings; d.n_spkr = c.n_spkr;
    d.per_rb = d.type == 1 ? 2 * d.ND : d.ND;
    d.C[0] = d.C0; d.T[0] = U;
    d.L.push_back(LayerDesc{d.Cin0, d.C0, 7, 1, 1, 0, U, U});
    for (int i = 0; i < d.S; ++i) {
        const int u = c.upsample_rates[i], k = c.upsample_kernel_sizes[i];
        d.C[i + 1] = d.C0 >> (i + 1);
        d.T[i + 1] = (d.T[i] - 1) * u - 2 * ((k - u) / 2) + k;
        d.L.push_back(LayerDesc{d.C0 >> i, d.C[i + 1], k, 1, u, 1, d.T[i], d.T[i + 1]});
    }
    for (int i = 0; i < d.S; ++i)
        for (int j = 0; j < d.NK; ++j)
            for (int m = 0; m < d.ND; ++m) {
                const int ch = d.C[i + 1], k = c.resblock_kernel_sizes[j], T = d.T[i + 1];
                d.L.push_back(LayerDesc{ch, ch, k, c.resblock_dilation_sizes[j][m], 1, 0, T, T});
                if (d.type == 1) d.L.push_back(LayerDesc{ch, ch, k, 1, 1, 0, T, T});
            }
    d.L.push_back(LayerDesc{d.C[d.S], 1, 7, 1, 1, 0, d.T[d.S], d.T[d.S]});
    d.max_act = (size_t)B * std::max(d.Cin0, d.C0) * U;
    d.max_w = 0;
    for (int i = 1; i <= d.S; ++i) d.max_act = std::max(d.max_act, (size_t)B * d.C[i] * d.T[i]);
    for (const LayerDesc& l : d.L) d.max_w = std::max(d.max_w, l.wsize());
    return d;
}

const parrot_voc_layer_ptrs& layer_ptrs(const parrot_voc_train_ptrs& p, const Dims& d, int l) {
    if (l == 0) return p.conv_pre;
    if (l <= d.S) return p.ups[l - 1];
    if (l == d.post()) return p.conv_post;
    return p.rb[l - 1 - d.S];
}

// What the forward keeps for the backward, in this order, every buffer at a multiple of 256 bytes:
//   emb (B, model_in_dim, U); per stage i: a_up[i] (B, C_(i-1), T_(i-1)), then per resblock and conv its activated input a (B, C_i, T_i);
//   a_post (B, C_last, T_last); y (B, T_last); per layer in state_dict order: norm (dim-0 rows) and the folded weight.
struct Saved {
    float* emb;
    float* a_up[PARROT_MAX_STAGES];
    std::vector<float*> a_rb;  // index: Dims::rb(i, j, c) - (1 + S)
    float *a_post, *y;
    std::vector<float*> norm, w;
};
Saved saved_layout(Arena& ar, const Dims& d) {
    Saved sv{};
    const size_t B = d.B;
    sv.emb = ar.take<float>(B * d.Cin0 * d.U);
    sv.a_rb.resize((size_t)d.S * d.NK * d.per_rb);
    for (int i = 0; i < d.S; ++i) {
        sv.a_up[i] = ar.take<float>(B * d.C[i] * d.T[i]);
        for (int q = 0; q < d.NK * d.per_rb; ++q) sv.a_rb[(size_t)i * d.NK * d.per_rb + q] = ar.take<float>(B * d.C[i + 1] * d.T[i + 1]);
    }
    sv.a_post = ar.take<float>(B * d.C[d.S] * d.T[d.S]);
    sv.y = ar.take<float>(B * d.T[d.S]);
    for (const LayerDesc& l : d.L) {
        sv.norm.push_back(ar.take<float>(l.rows()));
        sv.w.push_back(ar.take<float>(l.wsize()));
    }
    return sv;
}
size_t saved_bytes(const Dims& d) {
    Arena ar(nullptr, 0);
    (void)saved_layout(ar, d);
    return align_up(ar.off, 256);
}
// The lrelu sites in execution order -> (buffer, elements)
struct Site { const float* a; size_t n; };
std::vector<Site> sites(const Saved& sv, const Dims& d) {
    std::vector<Site> out;
    for (int i = 0; i < d.S; ++i) {
        out.push_back(Site{sv.a_up[i], (size_t)d.B * d.C[i] * d.T[i]});
        for (int q = 0; q < d.NK * d.per_rb; ++q) out.push_back(Site{sv.a_rb[(size_t)i * d.NK * d.per_rb + q], (size_t)d.B * d.C[i + 1] * d.T[i + 1]});
    }
    out.push_back(Site{sv.a_post, (size_t)d.B * d.C[d.S] * d.T[d.S]});
    return out;
}

size_t part_floats_for(const Dims& d) {
    size_t need = 0;
    for (const LayerDesc& l : d.L) need = std::max(need, wgrad_part_floats(d.B * l.Tin, (size_t)l.cin * l.cout, l.k));
    return need;
}
// The forward's workspace: conv_pre's output, the stage's running x, one buffer per resblock of the stage, conv_post's output, and
// the region of `saved` for a forward that keeps nothing.
struct FwdScratch {
    float *t0, *x, *r, *z;
    char* saved;
};
FwdScratch fwd_layout(Arena& ar, const Dims& d) {
    FwdScratch w{};
    w.t0 = ar.take<float>((size_t)d.B * d.C0 * d.U);
    w.x = ar.take<float>(d.max_act);
    w.r = ar.take<float>(d.max_act * d.NK);
    w.z = ar.take<float>((size_t)d.B * d.T[d.S]);
    w.saved = ar.take<char>(saved_bytes(d));
    return w;
}
struct BwdScratch {
    float *gz, *gx, *gr, *gb, *gsum, *t1, *dw, *gemb, *part;
    size_t part_floats;
};
BwdScratch bwd_layout(Arena& ar, const Dims& d) {
    BwdScratch w{};
    w.gz = ar.take<float>((size_t)d.B * d.T[d.S]);
    w.gx = ar.take<float>(d.max_act); w.gr = ar.take<float>(d.max_act); w.gb = ar.take<float>(d.max_act);
    w.gsum = ar.take<float>(d.max_act); w.t1 = ar.take<float>(d.max_act);
    w.dw = ar.take<float>(d.max_w);
    w.gemb = ar.take<float>((size_t)d.B * d.U * d.E);
    w.part_floats = part_floats_for(d);
    w.part = ar.take<float>(w.part_floats);
    return w;
}
size_t workspace_bytes(const Dims& d) {
    Arena a(nullptr, 0), b(nullptr, 0);
    (void)fwd_layout(a, d);
    (void)bwd_layout(b, d);
    return align_up(std::max(a.off, b.off), 256);
}

// ---- the matrix products, by shape (train_gemm_host.h, channel-first) -------------------------------------------------------
// Y (B, cout, T) = conv1d(X (B, cin, T), W (cout, cin, k), dilation dil, padding dil (k - 1) / 2) + bias: tap j has shift (j - (k - 1) / 2) dil
int conv_fwd(const LayerDesc& l, const float* W, const float* bias, const float* X, float* Y, int B, Epi e, hipStream_t s) {
    e.bias0 = bias;
    return parrot::conv_fwd(l.conv(W), X, l.in(), Y, l.out(), B, l.Tin, e, s);
}
// dX[b][ci][t] = sum_j sum_co W[co][ci][j] dY[b][co][t - shift_j]
int conv_dx(const LayerDesc& l, const float* W, const float* dY, float* dX, int B, const Epi& e, hipStream_t s) {
    return parrot::conv_dx(l.conv(W), dY, l.out(), dX, l.in(), B, l.Tin, e, s);
}
// Rows [ci0, ci0 + E) of conv_pre's data gradient, written as (B, U, E) for tt_launch_embed_grad.  (A raw struct: a sub-range of
// the weight's input channels is no ConvW, and nobody else wants one.)
int conv_pre_dx_rows(const LayerDesc& l, const float* W, const float* dY, float* dX, int B, int ci0, int E, hipStream_t s) {
    TapGemmParams g{};
    g.ntaps = l.k;
    for (int j = 0; j < l.k; ++j) { g.A[j] = W + (size_t)ci0 * l.k + j; g.shift[j] = -(j - (l.k - 1) / 2) * l.dil; }
    g.a_sm = l.k; g.a_sk = (long)l.cin * l.k;
    g.X = dY; g.x_sz = (long)l.cout * l.Tin; g.x_sk = l.Tin; g.x_sn = 1;
    g.C = dX; g.c_sz = (long)l.Tin * E; g.c_sm = 1; g.c_sn = E;
    g.M = E; g.N = l.Tin; g.K = l.cout;
    HIP_TRY(launch_tap_gemm(g, B, s));
    return PARROT_OK;
}
// dW[co][ci][j] = sum_(b, t) dY[b][co][t] X[b][ci][t + shift_j]
int conv_dw(const LayerDesc& l, const float* dY, const float* X, float* dW, int B, float* part, size_t part_floats, hipStream_t s) {
    return parrot::conv_dw(l.conv(nullptr), dY, l.out(), X, l.in(), dW, B, l.Tin, part, part_floats, s);
}
// ConvTranspose1d(cin, cout, k, u, padding p = (k - u) / 2), W (cin, cout, k), by output phase: sample n u + r is a conv over the taps
// j = r + p (mod u) with shift (r + p - j) / u, written with column stride u.  X is bounded by Tin, not by the phase's length.
int convt_fwd(const LayerDesc& l, const float* W, const float* bias, const float* X, float* Y, int B, hipStream_t s) {
    const int p = (l.k - l.u) / 2;
    for (int r = 0; r < l.u; ++r) {
        const int Nr = (l.Tout - r + l.u - 1) / l.u;
        if (Nr < 1) continue;
        TapGemmParams g{};
        for (int j = (r + p) % l.u; j < l.k; j += l.u) {
            g.A[g.ntaps] = W + j;
            g.shift[g.ntaps] = (r + p - j) / l.u;  // (exact: u divides r + p - j)
            ++g.ntaps;
        }
        g.a_sm = l.k; g.a_sk = (long)l.cout * l.k;
        g.X = X; g.x_sz = (long)l.cin * l.Tin; g.x_sk = l.Tin; g.x_sn = 1; g.x_n = l.Tin;
        g.C = Y + r; g.c_sz = (long)l.cout * l.Tout; g.c_sm = l.Tout; g.c_sn = l.u;
        g.M = l.cout; g.N = Nr; g.K = l.cin;
        g.bias0 = bias;
        HIP_TRY(launch_tap_gemm(g, B, s));
    }
    return PARROT_OK;
}
// dX[b][ci][n] = sum_j sum_co W[ci][co][j] dY[b][co][n u + j - p]: a strided read with a per-tap offset, bounded by Tout
int convt_dx(const LayerDesc& l, const float* W, const float* dY, float* dX, int B, const Epi& e, hipStream_t s) {
    const int p = (l.k - l.u) / 2;
    TapGemmParams g{};
    g.ntaps = l.k;
    for (int j = 0; j < l.k; ++j) { g.A[j] = W + j; g.shift[j] = j - p; }
    g.a_sm = (long)l.cout * l.k; g.a_sk = l.k;
    g.X = dY; g.x_sz = (long)l.cout * l.Tout; g.x_sk = l.Tout; g.x_sn = 1; g.x_mul = l.u; g.x_n = l.Tout;
    g.C = dX; g.c_sz = (long)l.cin * l.Tin; g.c_sm = l.Tin; g.c_sn = 1;
    g.M = l.cin; g.N = l.Tin; g.K = l.cout;
    set_epi(g, e);
    HIP_TRY(launch_tap_gemm(g, B, s));
    return PARROT_OK;
}
// dW[ci][co][j] = sum_(b, n) X[b][ci][n] dY[b][co][n u + j - p]: X in dY's role, dY (time stride u, per-tap offset, bound Tout) in X's
int convt_dw(const LayerDesc& l, const float* dY, const float* X, float* dW, int B, float* part, size_t part_floats, hipStream_t s) {
    const int p = (l.k - l.u) / 2;
    WgradParams q{};
    q.dY = X; q.y_sz = (long)l.cin * l.Tin; q.y_sm = l.Tin; q.y_st = 1;
    q.X = dY; q.x_sz = (long)l.cout * l.Tout; q.x_sk = l.Tout; q.x_st = 1; q.x_mul = l.u; q.x_T = l.Tout;
    q.M = l.cin; q.K = l.cout; q.T = l.Tin; q.R = B * l.Tin;
    int shifts[MAX_K];
    for (int j = 0; j < l.k; ++j) shifts[j] = j - p;
    return wgrad_taps(q, shifts, l.k, dW, (long)l.cout * l.k, l.k, 1, part, part_floats, s);
}

int ptrs_ok(const Dims& d, const parrot_voc_train_ptrs* w, const std::string& who) {
    bool ok = w->dict && (!d.multi || w->spkr);
    for (int l = 0; l < d.n_layers(); ++l) ok = ok && layer_ptrs(*w, d, l).v && layer_ptrs(*w, d, l).bias;
    return ok ? PARROT_OK : fail(PARROT_E_INVALID, who + ": null parameter");
}
// the weight layer l runs on: v itself, or the folded one in `saved`
const float* weight_of(const Dims& d, const parrot_voc_train_ptrs& w, const Saved& sv, int l) {
    const parrot_voc_layer_ptrs& p = layer_ptrs(w, d, l);
    return p.g ? sv.w[l] : p.v;
}

// bias, weight (through weight norm where the layer has g) of layer l from the gradient dY at its output and its input X
int layer_grads(const Dims& d, int l, const parrot_voc_train_ptrs& wt, const parrot_voc_train_ptrs& gr, const Saved& sv, const float* dY,
                const float* X, const BwdScratch& w, hipStream_t s) {
    const LayerDesc& ld = d.L[l];
    const parrot_voc_layer_ptrs &p = layer_ptrs(wt, d, l), &g = layer_ptrs(gr, d, l);
    if (g.bias) HIP_TRY(vt_launch_chansum(dY, g.bias, d.B, ld.cout, ld.Tout, s));
    const bool wn = p.g != nullptr;
    if (!g.v && !(wn && g.g)) return PARROT_OK;
    float* dW = wn ? w.dw : g.v;
    if (ld.transposed) TRY(convt_dw(ld, dY, X, dW, d.B, w.part, w.part_floats, s));
    else TRY(conv_dw(ld, dY, X, dW, d.B, w.part, w.part_floats, s));
    if (wn) HIP_TRY(vt_launch_wn_bwd(dW, p.v, p.g, sv.norm[l], g.v, g.g, ld.rows(), (int)ld.len(), s));
    return PARROT_OK;
}

int poison_grad(float* p, size_t n, hipStream_t s) { return p ? poison(p, n * sizeof(float), s) : PARROT_OK; }

}  // namespace

extern "C" int64_t parrot_voc_train_out_len(const parrot_voc_cfg* cfg, int32_t U) {
    if (!cfg_quiet_ok(cfg, 1, U)) return 0;
    const Dims d = dims(*cfg, 1, U);
    return d.T[d.S];
}
extern "C" size_t parrot_voc_train_saved_bytes(const parrot_voc_cfg* cfg, int32_t B, int32_t U) {
    return cfg_quiet_ok(cfg, B, U) ? saved_bytes(dims(*cfg, B, U)) : 0;
}
extern "C" size_t parrot_voc_train_workspace_bytes(const parrot_voc_cfg* cfg, int32_t B, int32_t U) {
    return cfg_quiet_ok(cfg, B, U) ? workspace_bytes(dims(*cfg, B, U)) : 0;
}

extern "C" int parrot_voc_train_forward(const parrot_voc_cfg* cfg, const parrot_voc_train_ptrs* wt, const int64_t* code, const int64_t* spkr,
                                        int32_t B, int32_t U, float* wav, void* saved, void* ws, size_t ws_bytes, void* stream) {
    const std::string who = "voc_train_forward";
    if (!cfg || !wt || !code || !wav || !ws) return fail(PARROT_E_INVALID, who + ": null argument");
    TRY(cfg_ok(cfg, B, U, who));
    const Dims d = dims(*cfg, B, U);
    TRY(ptrs_ok(d, wt, who));
    if (d.multi && !spkr) return fail(PARROT_E_INVALID, who + ": the model has a speaker table: speaker ids are needed");
    if (ws_bytes < workspace_bytes(d)) return fail(PARROT_E_NOMEM, who + ": workspace too small");
    hipStream_t s = (hipStream_t)stream;
    Arena ar(ws, ws_bytes);
    const FwdScratch w = fwd_layout(ar, d);
    if (!ar.ok) return fail(PARROT_E_NOMEM, who + ": workspace too small");
    const size_t sv_bytes = saved_bytes(d);
    if (poison_word()) {
        TRY(poison(ws, ws_bytes, s));
        if (saved) TRY(poison(saved, sv_bytes, s));
        TRY(poison(wav, (size_t)B * d.T[d.S] * sizeof(float), s));
    }
    Arena sa(saved ? saved : (void*)w.saved, sv_bytes);
    const Saved sv = saved_layout(sa, d);
    for (int l = 0; l < d.n_layers(); ++l) {
        const parrot_voc_layer_ptrs& p = layer_ptrs(*wt, d, l);
        if (p.g) HIP_TRY(vt_launch_wn_fwd(p.v, p.g, sv.w[l], sv.norm[l], d.L[l].rows(), (int)d.L[l].len(), s));
    }
    auto W = [&](int l) { return weight_of(d, *wt, sv, l); };
    auto Bi = [&](int l) { return (const float*)layer_ptrs(*wt, d, l).bias; };
    HIP_TRY(vt_launch_embed(code, spkr, wt->dict, wt->spkr, sv.emb, B, U, d.E, d.n_emb, d.n_spkr, d.multi, s));
    TRY(conv_fwd(d.L[0], W(0), Bi(0), sv.emb, w.t0, B, Epi(), s));
    const float* cur_in = w.t0;
    for (int i = 0; i < d.S; ++i) {
        const size_t n = (size_t)B * d.C[i + 1] * d.T[i + 1];
        HIP_TRY(vt_launch_lrelu(cur_in, sv.a_up[i], SLOPE, (size_t)B * d.C[i] * d.T[i], s));
        TRY(convt_fwd(d.L[d.up(i)], W(d.up(i)), Bi(d.up(i)), sv.a_up[i], w.x, B, s));
        for (int j = 0; j < d.NK; ++j) {
            float* rj = w.r + (size_t)j * d.max_act;
            const float* cur = w.x;
            for (int m = 0; m < d.ND; ++m) {
                Epi res;
                res.res = cur;
                if (d.type == 1) {
                    const int l1 = d.rb(i, j, 2 * m), l2 = l1 + 1;
                    float *a1 = sv.a_rb[l1 - 1 - d.S], *a2 = sv.a_rb[l2 - 1 - d.S];
                    HIP_TRY(vt_launch_lrelu(cur, a1, SLOPE, n, s));
                    Epi act;  // (convs1[m]'s output is read through the next leaky ReLU only: a2 is written in its place)
                    act.lrelu = 1; act.lslope = SLOPE;
                    TRY(conv_fwd(d.L[l1], W(l1), Bi(l1), a1, a2, B, act, s));
                    TRY(conv_fwd(d.L[l2], W(l2), Bi(l2), a2, rj, B, res, s));
                } else {
                    const int l1 = d.rb(i, j, m);
                    float* a1 = sv.a_rb[l1 - 1 - d.S];
                    HIP_TRY(vt_launch_lrelu(cur, a1, SLOPE, n, s));
                    TRY(conv_fwd(d.L[l1], W(l1), Bi(l1), a1, rj, B, res, s));
                }
                cur = rj;  // (x = xt + x: the residual is read and written element by element, by the same thread)
            }
        }
        HIP_TRY(vt_launch_mrf(w.r, d.max_act, d.NK, w.x, n, s));
        cur_in = w.x;
    }
    const int lp = d.post();
    HIP_TRY(vt_launch_lrelu(cur_in, sv.a_post, SLOPE_POST, (size_t)B * d.C[d.S] * d.T[d.S], s));
    TRY(conv_fwd(d.L[lp], W(lp), Bi(lp), sv.a_post, w.z, B, Epi(), s));
    HIP_TRY(vt_launch_tanh(w.z, wav, sv.y, (size_t)B * d.T[d.S], s));
    return PARROT_OK;
}

extern "C" int parrot_voc_train_backward(const parrot_voc_cfg* cfg, const parrot_voc_train_ptrs* wt, const int64_t* code, const int64_t* spkr,
                                         const void* saved, const float* grad_wav, int32_t B, int32_t U, const parrot_voc_train_ptrs* gr, void* ws,
                                         size_t ws_bytes, void* stream) {
    const std::string who = "voc_train_backward";
    if (!cfg || !wt || !code || !saved || !grad_wav || !gr || !ws) return fail(PARROT_E_INVALID, who + ": null argument");
    TRY(cfg_ok(cfg, B, U, who));
    const Dims d = dims(*cfg, B, U);
    TRY(ptrs_ok(d, wt, who));
    if (d.multi && !spkr) return fail(PARROT_E_INVALID, who + ": the model has a speaker table: speaker ids are needed");
    if (ws_bytes < workspace_bytes(d)) return fail(PARROT_E_NOMEM, who + ": workspace too small");
    hipStream_t s = (hipStream_t)stream;
    Arena ar(ws, ws_bytes);
    const BwdScratch w = bwd_layout(ar, d);
    if (!ar.ok) return fail(PARROT_E_NOMEM, who + ": workspace too small");
    if (poison_word()) {
        TRY(poison(ws, ws_bytes, s));
        TRY(poison_grad(gr->dict, (size_t)d.n_emb * d.E, s));
        if (d.multi) TRY(poison_grad(gr->spkr, (size_t)d.n_spkr * d.E, s));
        for (int l = 0; l < d.n_layers(); ++l) {
            const parrot_voc_layer_ptrs& g = layer_ptrs(*gr, d, l);
            TRY(poison_grad(g.v, d.L[l].wsize(), s)); TRY(poison_grad(g.g, d.L[l].rows(), s)); TRY(poison_grad(g.bias, d.L[l].cout, s));
        }
    }
    Arena sa(const_cast<void*>(saved), saved_bytes(d));
    const Saved sv = saved_layout(sa, d);
    auto W = [&](int l) { return weight_of(d, *wt, sv, l); };
    auto masked = [](const float* a, float slope, const float* res) {
        Epi e;
        e.mask = a; e.mslope = slope; e.res = res;
        return e;
    };
    // ---- tanh, conv_post, the leaky ReLU before it ---------------------------------------------------------------------------
    const int lp = d.post();
    HIP_TRY(vt_launch_tanh_bwd(sv.y, grad_wav, w.gz, (size_t)B * d.T[d.S], s));
    TRY(layer_grads(d, lp, *wt, *gr, sv, w.gz, sv.a_post, w, s));
    TRY(conv_dx(d.L[lp], W(lp), w.gz, w.gx, B, masked(sv.a_post, SLOPE_POST, nullptr), s));
    // ---- the stages, last to first: w.gx holds the gradient at the stage's output -------------------------------------------
    for (int i = d.S - 1; i >= 0; --i) {
        const size_t n = (size_t)B * d.C[i + 1] * d.T[i + 1];
        HIP_TRY(vt_launch_div(w.gx, d.NK, w.gr, n, s));  // every resblock's output gets g / n_kernels
        for (int j = 0; j < d.NK; ++j) {
            const float* gcur = w.gr;
            for (int m = d.ND - 1; m >= 0; --m) {
                if (d.type == 1) {
                    const int l1 = d.rb(i, j, 2 * m), l2 = l1 + 1;
                    const float *a1 = sv.a_rb[l1 - 1 - d.S], *a2 = sv.a_rb[l2 - 1 - d.S];
                    TRY(layer_grads(d, l2, *wt, *gr, sv, gcur, a2, w, s));
                    TRY(conv_dx(d.L[l2], W(l2), gcur, w.t1, B, masked(a2, SLOPE, nullptr), s));  // t1: the gradient at convs1[m]'s output
                    TRY(layer_grads(d, l1, *wt, *gr, sv, w.t1, a1, w, s));
                    TRY(conv_dx(d.L[l1], W(l1), w.t1, w.gb, B, masked(a1, SLOPE, gcur), s));  // (+ the residual's, element by element)
                    gcur = w.gb;
                } else {
                    const int l1 = d.rb(i, j, m);
                    const float* a1 = sv.a_rb[l1 - 1 - d.S];
                    float* out = gcur == w.gb ? w.t1 : w.gb;  // (the operand is read with shifts: never in place)
                    TRY(layer_grads(d, l1, *wt, *gr, sv, gcur, a1, w, s));
                    TRY(conv_dx(d.L[l1], W(l1), gcur, out, B, masked(a1, SLOPE, gcur), s));
                    gcur = out;
                }
            }
            if (j == 0) HIP_TRY(hipMemcpyAsync(w.gsum, gcur, n * sizeof(float), hipMemcpyDeviceToDevice, s));
            else HIP_TRY(vt_launch_add(w.gsum, gcur, w.gsum, n, s));
        }
        const int lu = d.up(i);
        TRY(layer_grads(d, lu, *wt, *gr, sv, w.gsum, sv.a_up[i], w, s));
        TRY(convt_dx(d.L[lu], W(lu), w.gsum, w.gx, B, masked(sv.a_up[i], SLOPE, nullptr), s));
    }
    // ---- conv_pre and the two tables: w.gx is the gradient at conv_pre's output ----------------------------------------------
    TRY(layer_grads(d, 0, *wt, *gr, sv, w.gx, sv.emb, w, s));
    const long RU = (long)B * U;
    if (gr->dict) {
        TRY(conv_pre_dx_rows(d.L[0], W(0), w.gx, w.gemb, B, 0, d.E, s));
        HIP_TRY(tt_launch_embed_grad(code, w.gemb, gr->dict, RU, 1, d.E, d.n_emb, -1, s));
    }
    if (d.multi && gr->spkr) {
        TRY(conv_pre_dx_rows(d.L[0], W(0), w.gx, w.gemb, B, d.E, d.E, s));
        HIP_TRY(tt_launch_embed_grad(spkr, w.gemb, gr->spkr, RU, U, d.E, d.n_spkr, -1, s));
    }
    return PARROT_OK;
}

extern "C" int32_t parrot_voc_train_lrelu_sites(const parrot_voc_cfg* cfg) {
    if (!cfg_quiet_ok(cfg, 1, 1)) return 0;
    const Dims d = dims(*cfg, 1, 1);
    return d.S * (1 + d.NK * d.per_rb) + 1;
}
extern "C" int64_t parrot_voc_train_lrelu_site_elems(const parrot_voc_cfg* cfg, int32_t B, int32_t U, int32_t site) {
    if (!cfg_quiet_ok(cfg, B, U)) return 0;
    const Dims d = dims(*cfg, B, U);
    Arena sa(nullptr, 0);
    const std::vector<Site> st = sites(saved_layout(sa, d), d);
    return site >= 0 && site < (int)st.size() ? (int64_t)st[site].n : 0;
}
extern "C" int parrot_voc_train_lrelu_mask(const parrot_voc_cfg* cfg, int32_t B, int32_t U, const void* saved, int32_t site, uint8_t* out_u8,
                                           void* stream) {
    const std::string who = "voc_train_lrelu_mask";
    if (!cfg || !saved || !out_u8) return fail(PARROT_E_INVALID, who + ": null argument");
    TRY(cfg_ok(cfg, B, U, who));
    const Dims d = dims(*cfg, B, U);
    Arena sa(const_cast<void*>(saved), saved_bytes(d));
    const std::vector<Site> st = sites(saved_layout(sa, d), d);
    if (site < 0 || site >= (int)st.size()) return fail(PARROT_E_INVALID, who + ": no such site");
    HIP_TRY(vt_launch_mask(st[site].a, out_u8, st[site].n, (hipStream_t)stream));
    return PARROT_OK;
}

// ---------------------------------------------------------------------------------------------
// Debug entry points (include/parrot_hip_debug.h): one conv of the training path alone, and the weight norm.  Nothing is launched
// before the sizes are checked.
// ---------------------------------------------------------------------------------------------
namespace {
bool debug_conv_ok(long B, long cin, long cout, long k, long dil, long u, int transposed, long Tin, LayerDesc* l) {
    if (B < 1 || B > 65535 || cin < 1 || cout < 1 || k < 1 || k > MAX_K || dil < 1 || u < 1 || Tin < 1) return false;
    if (transposed ? (dil != 1 || u > k) : (u != 1 || !(k & 1))) return false;
    const long Tout = transposed ? (Tin - 1) * u - 2 * ((k - u) / 2) + k : Tin;
    const long lim = 0x3fffffffL;
    if (Tout < 1 || B * Tin * cin > lim || B * Tout * cout > lim || dil * k > lim || cin * cout * k > lim) return false;
    if ((B * Tin + TG_RCHUNK - 1) / TG_RCHUNK * k > 65535) return false;
    *l = LayerDesc{(int)cin, (int)cout, (int)k, (int)dil, (int)u, transposed ? 1 : 0, (int)Tin, (int)Tout};
    return true;
}
}  // namespace

extern "C" int parrot_debug_voc_conv_fwd(const float* x, const float* w, const float* bias, float* y, int32_t B, int32_t c_in, int32_t c_out, int32_t k,
                                         int32_t dil, int32_t u, int32_t transposed, int32_t T_in, void* stream) {
    LayerDesc l{};
    if (!x || !w || !y) return fail(PARROT_E_INVALID, "debug_voc_conv_fwd: null argument");
    if (!debug_conv_ok(B, c_in, c_out, k, dil, u, transposed, T_in, &l)) return fail(PARROT_E_INVALID, "debug_voc_conv_fwd: sizes outside the limits");
    return transposed ? convt_fwd(l, w, bias, x, y, B, (hipStream_t)stream) : conv_fwd(l, w, bias, x, y, B, Epi(), (hipStream_t)stream);
}
extern "C" int parrot_debug_voc_conv_dx(const float* dy, const float* w, float* dx, int32_t B, int32_t c_in, int32_t c_out, int32_t k, int32_t dil,
                                        int32_t u, int32_t transposed, int32_t T_in, void* stream) {
    LayerDesc l{};
    if (!dy || !w || !dx) return fail(PARROT_E_INVALID, "debug_voc_conv_dx: null argument");
    if (!debug_conv_ok(B, c_in, c_out, k, dil, u, transposed, T_in, &l)) return fail(PARROT_E_INVALID, "debug_voc_conv_dx: sizes outside the limits");
    return transposed ? convt_dx(l, w, dy, dx, B, Epi(), (hipStream_t)stream) : conv_dx(l, w, dy, dx, B, Epi(), (hipStream_t)stream);
}
extern "C" size_t parrot_debug_voc_conv_dw_workspace_bytes(int32_t B, int32_t c_in, int32_t c_out, int32_t k, int32_t T_in) {
    LayerDesc l{};
    if (!debug_conv_ok(B, c_in, c_out, k, 1, 1, 1, T_in, &l)) return 0;
    return (size_t)wgrad_chunks(B * T_in) * k * c_in * c_out * sizeof(float);
}
extern "C" int parrot_debug_voc_conv_dw(const float* dy, const float* x, float* dw, int32_t B, int32_t c_in, int32_t c_out, int32_t k, int32_t dil,
                                        int32_t u, int32_t transposed, int32_t T_in, void* ws, size_t ws_bytes, void* stream) {
    LayerDesc l{};
    if (!dy || !x || !dw || !ws) return fail(PARROT_E_INVALID, "debug_voc_conv_dw: null argument");
    if (!debug_conv_ok(B, c_in, c_out, k, dil, u, transposed, T_in, &l)) return fail(PARROT_E_INVALID, "debug_voc_conv_dw: sizes outside the limits");
    const size_t need = (size_t)wgrad_chunks(B * T_in) * k * c_in * c_out * sizeof(float);
    if (ws_bytes < need) return fail(PARROT_E_INVALID, "debug_voc_conv_dw: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    if (poison_word()) TRY(poison(ws, need, s));
    return transposed ? convt_dw(l, dy, x, dw, B, (float*)ws, need / sizeof(float), s) : conv_dw(l, dy, x, dw, B, (float*)ws, need / sizeof(float), s);
}
extern "C" int parrot_debug_voc_wn_fwd(const float* v, const float* g, float* w, float* norm, int32_t rows, int32_t len, void* stream) {
    if (!v || !g || !w || !norm || rows < 1 || len < 1) return fail(PARROT_E_INVALID, "debug_voc_wn_fwd: null argument or a size below 1");
    HIP_TRY(vt_launch_wn_fwd(v, g, w, norm, rows, len, (hipStream_t)stream));
    return PARROT_OK;
}
extern "C" int parrot_debug_voc_wn_bwd(const float* dw, const float* v, const float* g, const float* norm, float* dv, float* dg, int32_t rows,
                                       int32_t len, void* stream) {
    if (!dw || !v || !g || !norm || rows < 1 || len < 1) return fail(PARROT_E_INVALID, "debug_voc_wn_bwd: null argument or a size below 1");
    HIP_TRY(vt_launch_wn_bwd(dw, v, g, norm, dv, dg, rows, len, (hipStream_t)stream));
    return PARROT_OK;
}
