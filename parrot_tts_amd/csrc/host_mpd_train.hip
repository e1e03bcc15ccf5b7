// host_mpd_train.hip -- training the multi-period discriminator: MultiPeriodDiscriminator.forward with weight norm attached and its
// full backward as two stateless calls (kernels: mpd_train.h / tu_mpd_train.hip; the matrix products: train_gemm_host.h; weight norm
// and bias gradients: voc_train.h).  No handle, no packed weights, no host copy and no synchronisation: every parameter is read from
// the device pointer it is given, in torch's layout.  Maps are period-major, (N, p, C, H): every layer is a 1-D conv over H on
// Z = N p rows (grid z = Z), a strided one reading its input at column stride `stride` (x_mul), its data gradient one launch per
// phase of that stride.
#include "host_common.h"

#include <algorithm>
#include <string>

#include "mpd_train.h"
#include "train_gemm_host.h"
#include "voc_train.h"  // (borrowed: vt_launch_wn_fwd / _wn_bwd and vt_launch_chansum)

using namespace parrot;

namespace {

constexpr int NL = PARROT_MPD_LAYERS;  // convs[0 .. 5) and conv_post

// One conv over H on rows (Z, cin, Hin) -> (Z, cout, Hout): k taps, stride s, padding `pad`
struct SConv {
    int cin, cout, k, s, pad, Hin, Hout;
    Lay in() const { return chan_first(cin, Hin); }
    Lay out() const { return chan_first(cout, Hout); }
    size_t wsize() const { return (size_t)cin * cout * k; }
};
struct Period {
    int p, H0;        // H0 = (T + n_pad) / p
    SConv L[NL];
    size_t elems(int l, int N) const { return (size_t)N * p * L[l].cout * L[l].Hout; }  // of map l
};
struct Dims {
    int N, T, P;
    Period per[PARROT_MPD_MAX_PERIODS];
    size_t max_map, max_w, max_score, part_floats, dpart;
};

const char* LIMITS =
    ": shape outside the limits (1 to 8 periods, each >= 1; N, T and the widths >= 1; kernel_size odd, at most 11 and at most the padded "
    "rows of every layer; 1 <= stride <= kernel_size; T > n_pad = p - T mod p for every period (a reflect pad is smaller than its input); N p <= 65535; "
    "every map below 2^30 elements and N p H <= 65535 x 256 past the first layer)";

bool dims_ok(const parrot_mpd_cfg* c, long N, long T, Dims* out) {
    if (!c) return false;
    if (c->n_periods < 1 || c->n_periods > PARROT_MPD_MAX_PERIODS || N < 1 || T < 1 || T > 0x3fffffffL) return false;
    if (c->kernel_size < 1 || !(c->kernel_size & 1) || c->kernel_size > TG_MAX_TAPS || c->stride < 1 || c->stride > c->kernel_size) return false;
    for (int i = 0; i < 4; ++i)
        if (c->channels[i] < 1 || c->channels[i] > 65535) return false;
    const long lim = 0x3fffffffL;
    Dims d{};
    d.N = (int)N; d.T = (int)T; d.P = c->n_periods;
    for (int i = 0; i < d.P; ++i) {
        const long p = c->periods[i];
        if (p < 1 || N * p > 65535) return false;
        const long n_pad = T % p ? p - T % p : 0;
        if (T <= n_pad) return false;
        Period& pe = d.per[i];
        pe.p = (int)p; pe.H0 = (int)((T + n_pad) / p);
        long H = pe.H0;
        int cin = 1;
        for (int l = 0; l < NL; ++l) {
            const bool post = l == NL - 1;
            const int k = post ? MD_POST_K : c->kernel_size, s = l < 4 ? c->stride : 1, pad = post ? 1 : MD_PAD;
            const int cout = post ? 1 : c->channels[std::min(l, 3)];
            if (H + 2 * pad < k) return false;
            const long Ho = (H + 2 * pad - k) / s + 1;
            if (l >= 1 && (N * p * Ho + TG_RCHUNK - 1) / TG_RCHUNK > 65535) return false;
            if (N * p * Ho * cout > lim || N * p * H * cin > lim || (long)cin * cout * k > lim) return false;
            pe.L[l] = SConv{cin, cout, k, s, pad, (int)H, (int)Ho};
            d.max_map = std::max(d.max_map, pe.elems(l, d.N));
            d.max_w = std::max(d.max_w, pe.L[l].wsize());
            if (l >= 1 && !post) d.part_floats = std::max(d.part_floats, wgrad_part_floats((int)(N * p * Ho), (size_t)cin * cout, k));
            H = Ho; cin = cout;
        }
        d.max_score = std::max(d.max_score, pe.elems(NL - 1, d.N));
        d.dpart = std::max(d.dpart, (size_t)md_chunks(N * p * pe.L[0].Hout) * pe.L[0].cout * pe.L[0].k);
        d.dpart = std::max(d.dpart, (size_t)md_chunks(N * p * pe.L[NL - 1].Hin) * pe.L[NL - 1].cin * MD_POST_K);
    }
    if (out) *out = d;
    return true;
}

// What the forward keeps for the backward besides the maps, which are the caller's: per period and layer, in state_dict order, the
// norm of every dim-0 row (cout floats) and the folded weight (cout cin k floats), every buffer at a multiple of 256 bytes.
struct Saved {
    float *norm[PARROT_MPD_MAX_PERIODS][NL], *w[PARROT_MPD_MAX_PERIODS][NL];
};
Saved saved_layout(Arena& ar, const Dims& d) {
    Saved sv{};
    for (int i = 0; i < d.P; ++i)
        for (int l = 0; l < NL; ++l) {
            sv.norm[i][l] = ar.take<float>(d.per[i].L[l].cout);
            sv.w[i][l] = ar.take<float>(d.per[i].L[l].wsize());
        }
    return sv;
}
size_t saved_bytes(const Dims& d) {
    Arena ar(nullptr, 0);
    (void)saved_layout(ar, d);
    return align_up(ar.off, 256);
}
// The backward's workspace: two gradient buffers of the largest map, a zero score gradient, one weight gradient, the partials
struct BwdScratch {
    float *ga, *gb, *gz, *dw, *part;
    double* dpart;
};
BwdScratch bwd_layout(Arena& ar, const Dims& d) {
    BwdScratch w{};
    w.ga = ar.take<float>(d.max_map); w.gb = ar.take<float>(d.max_map);
    w.gz = ar.take<float>(d.max_score);
    w.dw = ar.take<float>(d.max_w);
    w.part = ar.take<float>(d.part_floats);
    w.dpart = ar.take<double>(d.dpart);
    return w;
}
size_t workspace_bytes(const Dims& d) {
    Arena b(nullptr, 0);
    (void)bwd_layout(b, d);
    return align_up(std::max(b.off, saved_bytes(d)), 256);  // (the forward's: the region of `saved` when nothing is kept)
}

// ---- the four convs between the ends (train_gemm_host.h) ---------------------------------------------------------------------
// Y[z][co][h] = lrelu(sum_j sum_ci W[co][ci][j] X[z][ci][h s + j - pad] + bias[co])
int sconv_fwd(const SConv& l, const float* W, const float* bias, const float* X, float* Y, int Z, int act, float slope, hipStream_t s) {
    TapGemmParams g{};
    g.ntaps = l.k;
    for (int j = 0; j < l.k; ++j) { g.A[j] = W + j; g.shift[j] = j - l.pad; }
    g.a_sm = (long)l.cin * l.k; g.a_sk = l.k;
    g.X = X; g.x_sz = l.in().sz; g.x_sk = l.in().sc; g.x_sn = 1; g.x_mul = l.s; g.x_n = l.Hin;
    g.C = Y; g.c_sz = l.out().sz; g.c_sm = l.out().sc; g.c_sn = 1;
    g.M = l.cout; g.N = l.Hout; g.K = l.cin;
    g.bias0 = bias; g.lrelu = act; g.lslope = slope;
    HIP_TRY(launch_tap_gemm(g, Z, s));
    return PARROT_OK;
}
// dX[z][ci][n s + r] = mask(pre + sum over the taps j = r + pad (mod s) of sum_co W[co][ci][j] dY[z][co][n + (r + pad - j) / s]): the
// phase split of a transposed conv (host_voc_train.hip, convt_fwd), written with column stride s; dY is bounded by Hout.  Every
// phase has a tap, because s <= k.
int sconv_dx(const SConv& l, const float* W, const float* dY, float* dX, int Z, const float* pre, const float* mask, float mslope, hipStream_t s) {
    for (int r = 0; r < l.s; ++r) {
        const int Nr = (l.Hin - r + l.s - 1) / l.s;
        if (Nr < 1) continue;
        TapGemmParams g{};
        for (int j = (r + l.pad) % l.s; j < l.k; j += l.s) {
            g.A[g.ntaps] = W + j;
            g.shift[g.ntaps] = (r + l.pad - j) / l.s;  // (exact: s divides r + pad - j)
            ++g.ntaps;
        }
        g.a_sm = l.k; g.a_sk = (long)l.cin * l.k;
        g.X = dY; g.x_sz = l.out().sz; g.x_sk = l.out().sc; g.x_sn = 1; g.x_n = l.Hout;
        g.C = dX + r; g.c_sz = l.in().sz; g.c_sm = l.in().sc; g.c_sn = l.s;
        g.M = l.cin; g.N = Nr; g.K = l.cout;
        g.pre = pre ? pre + r : nullptr;
        g.mask = mask ? mask + r : nullptr; g.mslope = mslope;
        HIP_TRY(launch_tap_gemm(g, Z, s));
    }
    return PARROT_OK;
}
// dW[co][ci][j] = sum_(z, h) dY[z][co][h] X[z][ci][h s + j - pad]: X at time stride s, bounded by Hin (convt_dw's form)
int sconv_dw(const SConv& l, const float* dY, const float* X, float* dW, int Z, float* part, size_t part_floats, hipStream_t s) {
    WgradParams q{};
    q.dY = dY; q.y_sz = l.out().sz; q.y_sm = l.out().sc; q.y_st = 1;
    q.X = X; q.x_sz = l.in().sz; q.x_sk = l.in().sc; q.x_st = 1; q.x_mul = l.s; q.x_T = l.Hin;
    q.M = l.cout; q.K = l.cin; q.T = l.Hout; q.R = Z * l.Hout;
    int shifts[TG_MAX_TAPS];
    for (int j = 0; j < l.k; ++j) shifts[j] = j - l.pad;
    return wgrad_taps(q, shifts, l.k, dW, (long)l.cin * l.k, l.k, 1, part, part_floats, s);
}
MdFirst first_of(const Period& pe, int N, int T) { return MdFirst{N, T, pe.p, pe.H0, pe.L[0].Hout, pe.L[0].cout, pe.L[0].k, pe.L[0].s}; }

int ptrs_ok(const Dims& d, const parrot_mpd_ptrs* w, const std::string& who) {
    bool ok = true;
    for (int i = 0; i < d.P; ++i)
        for (int l = 0; l < NL; ++l) ok = ok && w->layer[i][l].v && w->layer[i][l].bias;
    return ok ? PARROT_OK : fail(PARROT_E_INVALID, who + ": null parameter");
}
int maps_ok(const Dims& d, const parrot_mpd_maps* m, const std::string& who) {
    bool ok = true;
    for (int i = 0; i < d.P; ++i)
        for (int l = 0; l < NL; ++l) ok = ok && m->map[i][l];
    return ok ? PARROT_OK : fail(PARROT_E_INVALID, who + ": null map");
}
int poison_grad(float* p, size_t n, hipStream_t s) { return p ? poison(p, n * sizeof(float), s) : PARROT_OK; }

}  // namespace

extern "C" int64_t parrot_mpd_train_map_rows(const parrot_mpd_cfg* cfg, int32_t T, int32_t period, int32_t layer) {
    Dims d;
    if (!dims_ok(cfg, 1, T, &d) || period < 0 || period >= d.P || layer < 0 || layer >= NL) return 0;
    return d.per[period].L[layer].Hout;
}
extern "C" size_t parrot_mpd_train_saved_bytes(const parrot_mpd_cfg* cfg, int32_t N, int32_t T) {
    Dims d;
    return dims_ok(cfg, N, T, &d) ? saved_bytes(d) : 0;
}
extern "C" size_t parrot_mpd_train_workspace_bytes(const parrot_mpd_cfg* cfg, int32_t N, int32_t T) {
    Dims d;
    return dims_ok(cfg, N, T, &d) ? workspace_bytes(d) : 0;
}

extern "C" int parrot_mpd_train_forward(const parrot_mpd_cfg* cfg, const parrot_mpd_ptrs* wt, const float* wav, int32_t N, int32_t T,
                                        const parrot_mpd_maps* maps, void* saved, void* ws, size_t ws_bytes, void* stream) {
    const std::string who = "mpd_train_forward";
    if (!cfg || !wt || !wav || !maps || !ws) return fail(PARROT_E_INVALID, who + ": null argument");
    Dims d;
    if (!dims_ok(cfg, N, T, &d)) return fail(PARROT_E_INVALID, who + LIMITS);
    TRY(ptrs_ok(d, wt, who));
    TRY(maps_ok(d, maps, who));
    if (ws_bytes < workspace_bytes(d)) return fail(PARROT_E_NOMEM, who + ": workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const size_t sv_bytes = saved_bytes(d);
    if (poison_word()) {
        TRY(poison(ws, ws_bytes, s));
        if (saved) TRY(poison(saved, sv_bytes, s));
        for (int i = 0; i < d.P; ++i)
            for (int l = 0; l < NL; ++l) TRY(poison(maps->map[i][l], d.per[i].elems(l, N) * sizeof(float), s));
    }
    Arena sa(saved ? saved : ws, sv_bytes);
    const Saved sv = saved_layout(sa, d);
    for (int i = 0; i < d.P; ++i) {
        const Period& pe = d.per[i];
        const int Z = N * pe.p;
        auto W = [&](int l) { return wt->layer[i][l].g ? (const float*)sv.w[i][l] : (const float*)wt->layer[i][l].v; };
        for (int l = 0; l < NL; ++l) {
            const parrot_voc_layer_ptrs& p = wt->layer[i][l];
            if (p.g) HIP_TRY(vt_launch_wn_fwd(p.v, p.g, sv.w[i][l], sv.norm[i][l], pe.L[l].cout, pe.L[l].cin * pe.L[l].k, s));
        }
        HIP_TRY(md_launch_first_fwd(first_of(pe, N, T), wav, W(0), wt->layer[i][0].bias, maps->map[i][0], cfg->slope, s));
        for (int l = 1; l < NL - 1; ++l) TRY(sconv_fwd(pe.L[l], W(l), wt->layer[i][l].bias, maps->map[i][l - 1], maps->map[i][l], Z, 1, cfg->slope, s));
        HIP_TRY(md_launch_post_fwd(maps->map[i][NL - 2], W(NL - 1), wt->layer[i][NL - 1].bias, maps->map[i][NL - 1], Z, pe.L[NL - 1].cin,
                                   pe.L[NL - 1].Hin, s));
    }
    return PARROT_OK;
}

extern "C" int parrot_mpd_train_backward(const parrot_mpd_cfg* cfg, const parrot_mpd_ptrs* wt, const float* wav, const parrot_mpd_maps* maps,
                                         const void* saved, const parrot_mpd_maps* grad_maps, int32_t N, int32_t T, const parrot_mpd_ptrs* gr,
                                         float* grad_wav, void* ws, size_t ws_bytes, void* stream) {
    const std::string who = "mpd_train_backward";
    if (!cfg || !wt || !wav || !maps || !saved || !grad_maps || !gr || !ws) return fail(PARROT_E_INVALID, who + ": null argument");
    Dims d;
    if (!dims_ok(cfg, N, T, &d)) return fail(PARROT_E_INVALID, who + LIMITS);
    TRY(ptrs_ok(d, wt, who));
    TRY(maps_ok(d, maps, who));
    if (ws_bytes < workspace_bytes(d)) return fail(PARROT_E_NOMEM, who + ": workspace too small");
    hipStream_t s = (hipStream_t)stream;
    Arena ar(ws, ws_bytes);
    const BwdScratch w = bwd_layout(ar, d);
    if (!ar.ok) return fail(PARROT_E_NOMEM, who + ": workspace too small");
    if (poison_word()) {
        TRY(poison(ws, ws_bytes, s));
        TRY(poison_grad(grad_wav, (size_t)N * T, s));
        for (int i = 0; i < d.P; ++i)
            for (int l = 0; l < NL; ++l) {
                const parrot_voc_layer_ptrs& g = gr->layer[i][l];
                const SConv& L = d.per[i].L[l];
                TRY(poison_grad(g.v, L.wsize(), s)); TRY(poison_grad(g.g, L.cout, s)); TRY(poison_grad(g.bias, L.cout, s));
            }
    }
    Arena sa(const_cast<void*>(saved), saved_bytes(d));
    const Saved sv = saved_layout(sa, d);
    const float slope = cfg->slope;
    for (int i = 0; i < d.P; ++i) {
        const Period& pe = d.per[i];
        const int Z = N * pe.p;
        auto W = [&](int l) { return wt->layer[i][l].g ? (const float*)sv.w[i][l] : (const float*)wt->layer[i][l].v; };
        auto up = [&](int l) { return (const float*)grad_maps->map[i][l]; };
        // the weight gradient formed in dW (w.dw under weight norm, else the caller's field) goes through the weight norm's backward
        auto wants_w = [&](int l) { return gr->layer[i][l].v || (wt->layer[i][l].g && gr->layer[i][l].g); };
        auto dw_of = [&](int l) { return wt->layer[i][l].g ? w.dw : gr->layer[i][l].v; };
        auto wn_bwd = [&](int l) -> int {
            const parrot_voc_layer_ptrs &p = wt->layer[i][l], &g = gr->layer[i][l];
            if (p.g) HIP_TRY(vt_launch_wn_bwd(w.dw, p.v, p.g, sv.norm[i][l], g.v, g.g, pe.L[l].cout, pe.L[l].cin * pe.L[l].k, s));
            return PARROT_OK;
        };
        // ---- conv_post: the gradient at the score is what arrives from outside, or zero ---------------------------------------
        const SConv& Lp = pe.L[NL - 1];
        const float* g = up(NL - 1);
        if (!g) {
            HIP_TRY(hipMemsetAsync(w.gz, 0, pe.elems(NL - 1, N) * sizeof(float), s));
            g = w.gz;
        }
        if (gr->layer[i][NL - 1].bias) HIP_TRY(vt_launch_chansum(g, gr->layer[i][NL - 1].bias, Z, 1, Lp.Hout, s));
        if (wants_w(NL - 1)) {
            HIP_TRY(md_launch_post_dw(g, maps->map[i][NL - 2], w.dpart, dw_of(NL - 1), Z, Lp.cin, Lp.Hin, s));
            TRY(wn_bwd(NL - 1));
        }
        HIP_TRY(md_launch_post_dx(g, W(NL - 1), up(NL - 2), maps->map[i][NL - 2], slope, w.ga, Z, Lp.cin, Lp.Hin, s));
        // ---- convs[4 .. 1]: cur is the gradient at map l, past its mask -----------------------------------------------------------
        float* cur = w.ga;
        for (int l = NL - 2; l >= 1; --l) {
            const SConv& L = pe.L[l];
            if (gr->layer[i][l].bias) HIP_TRY(vt_launch_chansum(cur, gr->layer[i][l].bias, Z, L.cout, L.Hout, s));
            if (wants_w(l)) {
                TRY(sconv_dw(L, cur, maps->map[i][l - 1], dw_of(l), Z, w.part, d.part_floats, s));
                TRY(wn_bwd(l));
            }
            float* out = cur == w.ga ? w.gb : w.ga;
            TRY(sconv_dx(L, W(l), cur, out, Z, up(l - 1), maps->map[i][l - 1], slope, s));
            cur = out;
        }
        // ---- convs[0], the fold and the reflect pad ------------------------------------------------------------------------------
        const MdFirst f = first_of(pe, N, T);
        if (gr->layer[i][0].bias) HIP_TRY(vt_launch_chansum(cur, gr->layer[i][0].bias, Z, f.C1, f.H1, s));
        if (wants_w(0)) {
            HIP_TRY(md_launch_first_dw(f, cur, wav, w.dpart, dw_of(0), s));
            TRY(wn_bwd(0));
        }
        if (grad_wav) HIP_TRY(md_launch_first_dx(f, cur, W(0), grad_wav, i > 0, s));  // (periods are added in their order)
    }
    return PARROT_OK;
}

// ---------------------------------------------------------------------------------------------
// Debug entry points (include/parrot_hip_debug.h): each new form alone.  Nothing is launched before the sizes are checked.
// ---------------------------------------------------------------------------------------------
namespace {
bool debug_conv_ok(long Z, long cin, long cout, long k, long stride, long Hin, SConv* l) {
    if (Z < 1 || Z > 65535 || cin < 1 || cout < 1 || k < 1 || !(k & 1) || k > TG_MAX_TAPS || stride < 1 || stride > k || Hin < 1 || Hin + 2 * MD_PAD < k) return false;
    const long Ho = (Hin + 2 * MD_PAD - k) / stride + 1, lim = 0x3fffffffL;
    if ((Z * Ho + TG_RCHUNK - 1) / TG_RCHUNK > 65535 || Z * Hin * cin > lim || Z * Ho * cout > lim || cin * cout * k > lim) return false;
    *l = SConv{(int)cin, (int)cout, (int)k, (int)stride, MD_PAD, (int)Hin, (int)Ho};
    return true;
}
bool debug_first_ok(long N, long T, long p, long C1, long k, long stride, MdFirst* f) {
    if (N < 1 || N > 65535 || T < 1 || T > 0x3fffffffL || p < 1 || N * p > 65535 || C1 < 1 || C1 > 65535) return false;
    if (k < 1 || !(k & 1) || k > TG_MAX_TAPS || stride < 1 || stride > k) return false;
    const long n_pad = T % p ? p - T % p : 0, H = (T + n_pad) / p;
    if (T <= n_pad || H + 2 * MD_PAD < k) return false;
    const long H1 = (H + 2 * MD_PAD - k) / stride + 1;
    if (N * p * H1 * C1 > 0x3fffffffL) return false;
    *f = MdFirst{(int)N, (int)T, (int)p, (int)H, (int)H1, (int)C1, (int)k, (int)stride};
    return true;
}
bool debug_post_ok(long Z, long C, long H) { return Z >= 1 && C >= 1 && C <= 65535 && H >= 1 && Z * C * H <= 0x3fffffffL; }
}  // namespace

extern "C" int parrot_debug_mpd_conv_fwd(const float* x, const float* w, const float* bias, float* y, int32_t Z, int32_t c_in, int32_t c_out, int32_t k,
                                         int32_t stride, int32_t H_in, int32_t act, float slope, void* stream) {
    SConv l{};
    if (!x || !w || !y) return fail(PARROT_E_INVALID, "debug_mpd_conv_fwd: null argument");
    if (!debug_conv_ok(Z, c_in, c_out, k, stride, H_in, &l)) return fail(PARROT_E_INVALID, "debug_mpd_conv_fwd: sizes outside the limits");
    return sconv_fwd(l, w, bias, x, y, Z, act ? 1 : 0, slope, (hipStream_t)stream);
}
extern "C" int parrot_debug_mpd_conv_dx(const float* dy, const float* w, const float* pre, const float* mask, float slope, float* dx, int32_t Z,
                                        int32_t c_in, int32_t c_out, int32_t k, int32_t stride, int32_t H_in, void* stream) {
    SConv l{};
    if (!dy || !w || !dx) return fail(PARROT_E_INVALID, "debug_mpd_conv_dx: null argument");
    if (!debug_conv_ok(Z, c_in, c_out, k, stride, H_in, &l)) return fail(PARROT_E_INVALID, "debug_mpd_conv_dx: sizes outside the limits");
    return sconv_dx(l, w, dy, dx, Z, pre, mask, slope, (hipStream_t)stream);
}
extern "C" size_t parrot_debug_mpd_conv_dw_workspace_bytes(int32_t Z, int32_t c_in, int32_t c_out, int32_t k, int32_t stride, int32_t H_in) {
    SConv l{};
    if (!debug_conv_ok(Z, c_in, c_out, k, stride, H_in, &l)) return 0;
    return wgrad_part_floats(Z * l.Hout, (size_t)c_in * c_out, k) * sizeof(float);
}
extern "C" int parrot_debug_mpd_conv_dw(const float* dy, const float* x, float* dw, int32_t Z, int32_t c_in, int32_t c_out, int32_t k, int32_t stride,
                                        int32_t H_in, void* ws, size_t ws_bytes, void* stream) {
    SConv l{};
    if (!dy || !x || !dw || !ws) return fail(PARROT_E_INVALID, "debug_mpd_conv_dw: null argument");
    if (!debug_conv_ok(Z, c_in, c_out, k, stride, H_in, &l)) return fail(PARROT_E_INVALID, "debug_mpd_conv_dw: sizes outside the limits");
    const size_t need = wgrad_part_floats(Z * l.Hout, (size_t)c_in * c_out, k) * sizeof(float);
    if (ws_bytes < need) return fail(PARROT_E_INVALID, "debug_mpd_conv_dw: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    if (poison_word()) TRY(poison(ws, need, s));
    return sconv_dw(l, dy, x, dw, Z, (float*)ws, need / sizeof(float), s);
}
extern "C" int parrot_debug_mpd_first_fwd(const float* wav, const float* w, const float* bias, float* y, int32_t N, int32_t T, int32_t period,
                                          int32_t c1, int32_t k, int32_t stride, float slope, void* stream) {
    MdFirst f{};
    if (!wav || !w || !bias || !y) return fail(PARROT_E_INVALID, "debug_mpd_first_fwd: null argument");
    if (!debug_first_ok(N, T, period, c1, k, stride, &f)) return fail(PARROT_E_INVALID, "debug_mpd_first_fwd: sizes outside the limits");
    HIP_TRY(md_launch_first_fwd(f, wav, w, bias, y, slope, (hipStream_t)stream));
    return PARROT_OK;
}
extern "C" int parrot_debug_mpd_first_dx(const float* dy, const float* w, float* dwav, int32_t N, int32_t T, int32_t period, int32_t c1, int32_t k,
                                         int32_t stride, void* stream) {
    MdFirst f{};
    if (!dy || !w || !dwav) return fail(PARROT_E_INVALID, "debug_mpd_first_dx: null argument");
    if (!debug_first_ok(N, T, period, c1, k, stride, &f)) return fail(PARROT_E_INVALID, "debug_mpd_first_dx: sizes outside the limits");
    HIP_TRY(md_launch_first_dx(f, dy, w, dwav, 0, (hipStream_t)stream));
    return PARROT_OK;
}
extern "C" size_t parrot_debug_mpd_first_dw_workspace_bytes(int32_t N, int32_t T, int32_t period, int32_t c1, int32_t k, int32_t stride) {
    MdFirst f{};
    if (!debug_first_ok(N, T, period, c1, k, stride, &f)) return 0;
    return (size_t)md_chunks((long)N * period * f.H1) * c1 * k * sizeof(double);
}
extern "C" int parrot_debug_mpd_first_dw(const float* dy, const float* wav, float* dw, int32_t N, int32_t T, int32_t period, int32_t c1, int32_t k,
                                         int32_t stride, void* ws, size_t ws_bytes, void* stream) {
    MdFirst f{};
    if (!dy || !wav || !dw || !ws) return fail(PARROT_E_INVALID, "debug_mpd_first_dw: null argument");
    if (!debug_first_ok(N, T, period, c1, k, stride, &f)) return fail(PARROT_E_INVALID, "debug_mpd_first_dw: sizes outside the limits");
    const size_t need = (size_t)md_chunks((long)N * period * f.H1) * c1 * k * sizeof(double);
    if (ws_bytes < need) return fail(PARROT_E_INVALID, "debug_mpd_first_dw: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    if (poison_word()) TRY(poison(ws, need, s));
    HIP_TRY(md_launch_first_dw(f, dy, wav, (double*)ws, dw, s));
    return PARROT_OK;
}
extern "C" int parrot_debug_mpd_post_fwd(const float* x, const float* w, const float* bias, float* y, int32_t Z, int32_t C, int32_t H, void* stream) {
    if (!x || !w || !bias || !y) return fail(PARROT_E_INVALID, "debug_mpd_post_fwd: null argument");
    if (!debug_post_ok(Z, C, H)) return fail(PARROT_E_INVALID, "debug_mpd_post_fwd: sizes outside the limits");
    HIP_TRY(md_launch_post_fwd(x, w, bias, y, Z, C, H, (hipStream_t)stream));
    return PARROT_OK;
}
extern "C" int parrot_debug_mpd_post_dx(const float* dy, const float* w, const float* pre, const float* mask, float slope, float* dx, int32_t Z,
                                        int32_t C, int32_t H, void* stream) {
    if (!dy || !w || !dx) return fail(PARROT_E_INVALID, "debug_mpd_post_dx: null argument");
    if (!debug_post_ok(Z, C, H)) return fail(PARROT_E_INVALID, "debug_mpd_post_dx: sizes outside the limits");
    HIP_TRY(md_launch_post_dx(dy, w, pre, mask, slope, dx, Z, C, H, (hipStream_t)stream));
    return PARROT_OK;
}
extern "C" size_t parrot_debug_mpd_post_dw_workspace_bytes(int32_t Z, int32_t C, int32_t H) {
    return debug_post_ok(Z, C, H) ? (size_t)md_chunks((long)Z * H) * C * MD_POST_K * sizeof(double) : 0;
}
extern "C" int parrot_debug_mpd_post_dw(const float* dy, const float* x, float* dw, int32_t Z, int32_t C, int32_t H, void* ws, size_t ws_bytes,
                                        void* stream) {
    if (!dy || !x || !dw || !ws) return fail(PARROT_E_INVALID, "debug_mpd_post_dw: null argument");
    if (!debug_post_ok(Z, C, H)) return fail(PARROT_E_INVALID, "debug_mpd_post_dw: sizes outside the limits");
    const size_t need = parrot_debug_mpd_post_dw_workspace_bytes(Z, C, H);
    if (ws_bytes < need) return fail(PARROT_E_INVALID, "debug_mpd_post_dw: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    if (poison_word()) TRY(poison(ws, need, s));
    HIP_TRY(md_launch_post_dw(dy, x, (double*)ws, dw, Z, C, H, s));
    return PARROT_OK;
}
