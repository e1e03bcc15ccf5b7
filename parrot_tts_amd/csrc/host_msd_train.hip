// host_msd_train.hip -- training the multi-scale discriminator: MultiScaleDiscriminator.forward (spectral norm on the scales
// cfg->spectral names, weight norm or plain weights on the others) and its full backward as two stateless calls (kernels:
// msd_train.h / tu_msd_train.hip; convs[6]: train_gemm_host.h; conv_post: mpd_train.h's md_launch_post_*; weight norm and bias
// gradients: voc_train.h).  No handle, no packed weights, no host copy and no synchronisation.  Maps are torch's, (N, C, L), real rows
// first.  A spectral layer has two folded weights, one per half of the batch: the kernels that take a row split (convs[0], the
// grouped convs) run once, the others once per half on offset pointers; its two weight gradients are formed per half and meet in
// ms_launch_sn_bwd.
#include "host_common.h"

#include <algorithm>
#include <string>

#include "mpd_train.h"  // (borrowed: md_launch_post_fwd / _dx / _dw, md_chunks)
#include "msd_train.h"
#include "train_gemm_host.h"
#include "voc_train.h"  // (borrowed: vt_launch_wn_fwd / _wn_bwd and vt_launch_chansum)

using namespace parrot;

namespace {

constexpr int NL = PARROT_MSD_LAYERS;  // convs[0 .. 7) and conv_post
constexpr int LAST = 6;                // convs[6], dense
constexpr int STRIDES[NL] = {1, 2, 2, 4, 4, 1, 1, 1};
constexpr int KERNELS[NL] = {MS_FIRST_K, MS_K, MS_K, MS_K, MS_K, MS_K, 5, MD_POST_K};

struct SLayer {
    int cin, cout, G, k, s, pad, Lin, Lout;
    int cols() const { return cin / G * k; }
    size_t wsize() const { return (size_t)cout * cols(); }
    MsGconv gconv() const { return MsGconv{cin, cout, G, k, s, pad, Lin, Lout}; }
    ConvW dense(const float* w) const { return ConvW{w, cout, cin, k, 1, pad}; }
    Lay in() const { return chan_first(cin, Lin); }
    Lay out() const { return chan_first(cout, Lout); }
};
struct Scale {
    int T, spectral;  // T: the waveform after `scale` pools
    SLayer L[NL];
    size_t elems(int l, int N) const { return (size_t)N * L[l].cout * L[l].Lout; }
};
struct Dims {
    int N, T, S;
    Scale sc[PARROT_MSD_MAX_SCALES];
    size_t max_map, max_w, max_score, part_floats, dpart, max_vec;
};

const char* LIMITS =
    ": shape outside the limits (1 to 4 scales; N even, 2 <= N <= 65534; T >= 1; widths >= 1, each a multiple of its groups; groups[0] = "
    "groups[6] = 1; every map below 2^30 elements and N L <= 65535 x 256 at the grouped layers)";

bool dims_ok(const parrot_msd_cfg* c, long N, long T, Dims* out) {
    if (!c) return false;
    if (c->n_scales < 1 || c->n_scales > PARROT_MSD_MAX_SCALES || N < 2 || N > 65534 || (N & 1) || T < 1 || T > 0x3fffffffL) return false;
    for (int l = 0; l < 7; ++l)
        if (c->channels[l] < 1 || c->channels[l] > 65535 || c->groups[l] < 1) return false;
    if (c->groups[0] != 1 || c->groups[LAST] != 1) return false;
    const long lim = 0x3fffffffL;
    Dims d{};
    d.N = (int)N; d.T = (int)T; d.S = c->n_scales;
    long Ti = T;
    for (int i = 0; i < d.S; ++i) {
        Scale& sc = d.sc[i];
        sc.T = (int)Ti; sc.spectral = c->spectral[i] ? 1 : 0;
        long L = Ti;
        int cin = 1;
        for (int l = 0; l < NL; ++l) {
            const bool post = l == NL - 1;
            const int k = KERNELS[l], s = STRIDES[l], pad = (k - 1) / 2, cout = post ? 1 : c->channels[l], G = post ? 1 : c->groups[l];
            if (cin % G || cout % G) return false;
            const long Lo = (L - 1) / s + 1;
            if (N * Lo * cout > lim || N * L * cin > lim || (long)cout * (cin / G) * k > lim) return false;
            if (l >= 1 && !post && (N * Lo + TG_RCHUNK - 1) / TG_RCHUNK > 65535) return false;
            sc.L[l] = SLayer{cin, cout, G, k, s, pad, (int)L, (int)Lo};
            d.max_map = std::max(d.max_map, sc.elems(l, d.N));
            d.max_w = std::max(d.max_w, sc.L[l].wsize());
            d.max_vec = std::max(d.max_vec, (size_t)cout + sc.L[l].cols());
            if (l >= 1 && l < LAST) d.part_floats = std::max(d.part_floats, ms_gwgrad_part_floats(sc.L[l].gconv(), d.N));
            if (l == LAST) d.part_floats = std::max(d.part_floats, wgrad_part_floats((int)(N * Lo), (size_t)cin * cout, k));
            d.dpart = std::max(d.dpart, (size_t)2 * (ms_chunks((long)sc.L[l].wsize()) + 1));
            L = Lo; cin = cout;
        }
        d.max_score = std::max(d.max_score, sc.elems(NL - 1, d.N));
        d.dpart = std::max(d.dpart, (size_t)ms_chunks(N * Ti) * sc.L[0].cout * MS_FIRST_K);
        d.dpart = std::max(d.dpart, (size_t)md_chunks(N * sc.L[NL - 1].Lin) * sc.L[NL - 1].cin * MD_POST_K);
        Ti = Ti / 2 + 1;
    }
    if (out) *out = d;
    return true;
}

// What the forward keeps for the backward besides the maps, which are the caller's: the pooled waveforms; per scale and layer the
// norm of every dim-0 row and the folded weight; per layer of a spectral scale the second folded weight and both (u, v, sigma).
struct Saved {
    float* wav[PARROT_MSD_MAX_SCALES];
    float *norm[PARROT_MSD_MAX_SCALES][NL], *w[PARROT_MSD_MAX_SCALES][NL][2];
    float *u[PARROT_MSD_MAX_SCALES][NL][2], *v[PARROT_MSD_MAX_SCALES][NL][2], *sigma[PARROT_MSD_MAX_SCALES][NL][2];
};
Saved saved_layout(Arena& ar, const Dims& d) {
    Saved sv{};
    for (int i = 0; i < d.S; ++i) {
        if (i > 0) sv.wav[i] = ar.take<float>((size_t)d.N * d.sc[i].T);
        for (int l = 0; l < NL; ++l) {
            const SLayer& L = d.sc[i].L[l];
            sv.norm[i][l] = ar.take<float>(L.cout);
            sv.w[i][l][0] = ar.take<float>(L.wsize());
            if (!d.sc[i].spectral) continue;
            sv.w[i][l][1] = ar.take<float>(L.wsize());
            for (int h = 0; h < 2; ++h) {
                sv.u[i][l][h] = ar.take<float>(L.cout);
                sv.v[i][l][h] = ar.take<float>(L.cols());
                sv.sigma[i][l][h] = ar.take<float>(1);
            }
        }
    }
    return sv;
}
size_t saved_bytes(const Dims& d) {
    Arena ar(nullptr, 0);
    (void)saved_layout(ar, d);
    return align_up(ar.off, 256);
}
// The forward's workspace: the two mat-vec results of a power iteration, then the region of `saved` when nothing is kept
size_t fwd_tmp_bytes(const Dims& d) { return align_up(d.max_vec * sizeof(float), 256); }
// The backward's: two gradient buffers of the largest map, a zero score gradient, two weight gradients (a spectral layer's halves),
// the fp32 and fp64 partials, and the waveform gradients of the pooled scales
struct BwdScratch {
    float *ga, *gb, *gz, *dw[2], *part, *gwav[PARROT_MSD_MAX_SCALES];
    double* dpart;
};
BwdScratch bwd_layout(Arena& ar, const Dims& d) {
    BwdScratch w{};
    w.ga = ar.take<float>(d.max_map); w.gb = ar.take<float>(d.max_map);
    w.gz = ar.take<float>(d.max_score);
    w.dw[0] = ar.take<float>(d.max_w); w.dw[1] = ar.take<float>(d.max_w);
    w.part = ar.take<float>(d.part_floats);
    w.dpart = ar.take<double>(d.dpart);
    for (int i = 1; i < d.S; ++i) w.gwav[i] = ar.take<float>((size_t)d.N * d.sc[i].T);
    return w;
}
size_t workspace_bytes(const Dims& d) {
    Arena b(nullptr, 0);
    (void)bwd_layout(b, d);
    return align_up(std::max(b.off, fwd_tmp_bytes(d) + saved_bytes(d)), 256);
}

int ptrs_ok(const Dims& d, const parrot_msd_ptrs* w, const std::string& who) {
    for (int i = 0; i < d.S; ++i)
        for (int l = 0; l < NL; ++l) {
            const parrot_msd_layer_ptrs& p = w->layer[i][l];
            if (!p.v || !p.bias) return fail(PARROT_E_INVALID, who + ": null parameter");
            if (d.sc[i].spectral && (!p.u || !p.sv || p.g)) return fail(PARROT_E_INVALID, who + ": a spectral layer takes weight_orig, weight_u and weight_v and no weight_g");
        }
    return PARROT_OK;
}
int maps_ok(const Dims& d, const parrot_msd_maps* m, const std::string& who) {
    bool ok = true;
    for (int i = 0; i < d.S; ++i)
        for (int l = 0; l < NL; ++l) ok = ok && m->map[i][l];
    return ok ? PARROT_OK : fail(PARROT_E_INVALID, who + ": null map");
}
int poison_grad(float* p, size_t n, hipStream_t s) { return p ? poison(p, n * sizeof(float), s) : PARROT_OK; }

}  // namespace

extern "C" int64_t parrot_msd_train_map_len(const parrot_msd_cfg* cfg, int32_t T, int32_t scale, int32_t layer) {
    Dims d;
    if (!dims_ok(cfg, 2, T, &d) || scale < 0 || scale >= d.S || layer < 0 || layer >= NL) return 0;
    return d.sc[scale].L[layer].Lout;
}
extern "C" size_t parrot_msd_train_saved_bytes(const parrot_msd_cfg* cfg, int32_t N, int32_t T) {
    Dims d;
    return dims_ok(cfg, N, T, &d) ? saved_bytes(d) : 0;
}
extern "C" size_t parrot_msd_train_workspace_bytes(const parrot_msd_cfg* cfg, int32_t N, int32_t T) {
    Dims d;
    return dims_ok(cfg, N, T, &d) ? workspace_bytes(d) : 0;
}

extern "C" int parrot_msd_train_forward(const parrot_msd_cfg* cfg, const parrot_msd_ptrs* wt, const float* wav, int32_t N, int32_t T,
                                        int32_t power_iterations, const parrot_msd_maps* maps, void* saved, void* ws, size_t ws_bytes,
                                        void* stream) {
    const std::string who = "msd_train_forward";
    if (!cfg || !wt || !wav || !maps || !ws) return fail(PARROT_E_INVALID, who + ": null argument");
    if (power_iterations < 0 || power_iterations > 1) return fail(PARROT_E_INVALID, who + ": power_iterations is 0 or 1");
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
        for (int i = 0; i < d.S; ++i)
            for (int l = 0; l < NL; ++l) TRY(poison(maps->map[i][l], d.sc[i].elems(l, N) * sizeof(float), s));
    }
    float* tmp = (float*)ws;
    Arena sa(saved ? saved : (void*)((char*)ws + fwd_tmp_bytes(d)), sv_bytes);
    const Saved sv = saved_layout(sa, d);
    const int B = N / 2;
    const float slope = cfg->slope;
    for (int i = 0; i < d.S; ++i) {
        const Scale& sc = d.sc[i];
        if (i > 0) HIP_TRY(ms_launch_pool_fwd(i == 1 ? wav : sv.wav[i - 1], sv.wav[i], N, d.sc[i - 1].T, s));
        const float* x = i == 0 ? wav : sv.wav[i];
        // ---- the weights every layer runs on --------------------------------------------------------------------------------------
        const float* W[NL][2];
        for (int l = 0; l < NL; ++l) {
            const parrot_msd_layer_ptrs& p = wt->layer[i][l];
            const SLayer& L = sc.L[l];
            if (sc.spectral) {
                for (int h = 0; h < 2; ++h) {
                    HIP_TRY(ms_launch_sn_fold(p.v, p.u, p.sv, L.cout, L.cols(), power_iterations, sv.w[i][l][h], sv.sigma[i][l][h], tmp, s));
                    HIP_TRY(hipMemcpyAsync(sv.u[i][l][h], p.u, L.cout * sizeof(float), hipMemcpyDeviceToDevice, s));
                    HIP_TRY(hipMemcpyAsync(sv.v[i][l][h], p.sv, L.cols() * sizeof(float), hipMemcpyDeviceToDevice, s));
                    W[l][h] = sv.w[i][l][h];
                }
            } else {
                if (p.g) HIP_TRY(vt_launch_wn_fwd(p.v, p.g, sv.w[i][l][0], sv.norm[i][l], L.cout, L.cols(), s));
                W[l][0] = W[l][1] = p.g ? (const float*)sv.w[i][l][0] : (const float*)p.v;
            }
        }
        const int zs = sc.spectral ? B : N, nh = sc.spectral ? 2 : 1, Zh = N / nh;
        auto bias = [&](int l) { return (const float*)wt->layer[i][l].bias; };
        HIP_TRY(ms_launch_first_fwd(x, W[0][0], W[0][1], zs, bias(0), maps->map[i][0], N, sc.T, sc.L[0].cout, slope, s));
        for (int l = 1; l < LAST; ++l)
            HIP_TRY(ms_launch_gconv_fwd(sc.L[l].gconv(), maps->map[i][l - 1], W[l][0], W[l][1], zs, bias(l), maps->map[i][l], N, 1, slope, s));
        const SLayer &Ld = sc.L[LAST], &Lp = sc.L[NL - 1];
        for (int h = 0; h < nh; ++h) {
            Epi e{};
            e.bias0 = bias(LAST); e.lrelu = 1; e.lslope = slope;
            TRY(conv_fwd(Ld.dense(W[LAST][h]), maps->map[i][LAST - 1] + (size_t)h * Zh * Ld.in().sz, Ld.in(),
                         maps->map[i][LAST] + (size_t)h * Zh * Ld.out().sz, Ld.out(), Zh, Ld.Lout, e, s));
        }
        for (int h = 0; h < nh; ++h)
            HIP_TRY(md_launch_post_fwd(maps->map[i][LAST] + (size_t)h * Zh * Lp.in().sz, W[NL - 1][h], bias(NL - 1),
                                       maps->map[i][NL - 1] + (size_t)h * Zh * Lp.Lout, Zh, Lp.cin, Lp.Lin, s));
    }
    return PARROT_OK;
}

extern "C" int parrot_msd_train_backward(const parrot_msd_cfg* cfg, const parrot_msd_ptrs* wt, const float* wav, const parrot_msd_maps* maps,
                                         const void* saved, const parrot_msd_maps* grad_maps, int32_t N, int32_t T, const parrot_msd_ptrs* gr,
                                         float* grad_wav, void* ws, size_t ws_bytes, void* stream) {
    const std::string who = "msd_train_backward";
    if (!cfg || !wt || !wav || !maps || !saved || !grad_maps || !gr || !ws) return fail(PARROT_E_INVALID, who + ": null argument");
    Dims d;
    if (!dims_ok(cfg, N, T, &d)) return fail(PARROT_E_INVALID, who + LIMITS);
    TRY(ptrs_ok(d, wt, who));
    TRY(maps_ok(d, maps, who));
    if (ws_bytes < workspace_bytes(d)) return fail(PARROT_E_NOMEM, who + ": workspace too small");
    hipStream_t s = (hipStream_t)stream;
    Arena ar(ws, ws_bytes);
    BwdScratch w = bwd_layout(ar, d);
    if (!ar.ok) return fail(PARROT_E_NOMEM, who + ": workspace too small");
    if (poison_word()) {
        TRY(poison(ws, ws_bytes, s));
        TRY(poison_grad(grad_wav, (size_t)N * T, s));
        for (int i = 0; i < d.S; ++i)
            for (int l = 0; l < NL; ++l) {
                const parrot_msd_layer_ptrs& g = gr->layer[i][l];
                const SLayer& L = d.sc[i].L[l];
                TRY(poison_grad(g.v, L.wsize(), s)); TRY(poison_grad(g.g, L.cout, s)); TRY(poison_grad(g.bias, L.cout, s));
            }
    }
    Arena sa(const_cast<void*>(saved), saved_bytes(d));
    const Saved sv = saved_layout(sa, d);
    const float slope = cfg->slope;
    const int B = N / 2;
    w.gwav[0] = grad_wav;
    for (int i = d.S - 1; i >= 0; --i) {  // (the pooled scales first: their waveform gradients flow back through the pools)
        const Scale& sc = d.sc[i];
        const int zs = sc.spectral ? B : N, nh = sc.spectral ? 2 : 1, Zh = N / nh;
        const float* x = i == 0 ? wav : sv.wav[i];
        auto W = [&](int l, int h) {
            if (sc.spectral) return (const float*)sv.w[i][l][h];
            return wt->layer[i][l].g ? (const float*)sv.w[i][l][0] : (const float*)wt->layer[i][l].v;
        };
        auto up = [&](int l) { return (const float*)grad_maps->map[i][l]; };
        auto map = [&](int l) { return (const float*)maps->map[i][l]; };
        // The weight gradient of layer l: form(first row, rows, out) writes it for a range of rows; a spectral layer's two halves meet
        // in the backward through sigma, a weight-normed layer's goes through the weight norm's, a plain one's is the caller's field.
        auto wgrad = [&](int l, auto form) -> int {
            const parrot_msd_layer_ptrs &p = wt->layer[i][l], &g = gr->layer[i][l];
            const SLayer& L = sc.L[l];
            if (sc.spectral) {
                if (!g.v) return PARROT_OK;
                TRY(form(0, B, w.dw[0]));
                TRY(form(B, B, w.dw[1]));
                HIP_TRY(ms_launch_sn_bwd(w.dw[0], w.dw[1], p.v, sv.u[i][l][0], sv.v[i][l][0], sv.sigma[i][l][0], sv.u[i][l][1], sv.v[i][l][1],
                                         sv.sigma[i][l][1], g.v, L.cout, L.cols(), w.dpart, s));
            } else if (p.g) {
                if (!g.v && !g.g) return PARROT_OK;
                TRY(form(0, N, w.dw[0]));
                HIP_TRY(vt_launch_wn_bwd(w.dw[0], p.v, p.g, sv.norm[i][l], g.v, g.g, L.cout, L.cols(), s));
            } else if (g.v) {
                TRY(form(0, N, g.v));
            }
            return PARROT_OK;
        };
        // ---- conv_post: the gradient at the score is what arrives from outside, or zero ---------------------------------------
        const SLayer& Lp = sc.L[NL - 1];
        const float* g = up(NL - 1);
        if (!g) {
            HIP_TRY(hipMemsetAsync(w.gz, 0, sc.elems(NL - 1, N) * sizeof(float), s));
            g = w.gz;
        }
        if (gr->layer[i][NL - 1].bias) HIP_TRY(vt_launch_chansum(g, gr->layer[i][NL - 1].bias, N, 1, Lp.Lout, s));
        TRY(wgrad(NL - 1, [&](int z0, int Z, float* out) -> int {
            HIP_TRY(md_launch_post_dw(g + (size_t)z0 * Lp.Lout, map(LAST) + (size_t)z0 * Lp.in().sz, w.dpart, out, Z, Lp.cin, Lp.Lin, s));
            return PARROT_OK;
        }));
        for (int h = 0; h < nh; ++h) {
            const size_t o = (size_t)h * Zh * Lp.in().sz;
            HIP_TRY(md_launch_post_dx(g + (size_t)h * Zh * Lp.Lout, W(NL - 1, h), up(LAST) ? up(LAST) + o : nullptr, map(LAST) + o, slope, w.ga + o, Zh,
                                      Lp.cin, Lp.Lin, s));
        }
        // ---- convs[6 .. 1]: cur is the gradient at map l, past its mask --------------------------------------------------------------
        float* cur = w.ga;
        for (int l = LAST; l >= 1; --l) {
            const SLayer& L = sc.L[l];
            if (gr->layer[i][l].bias) HIP_TRY(vt_launch_chansum(cur, gr->layer[i][l].bias, N, L.cout, L.Lout, s));
            float* out = cur == w.ga ? w.gb : w.ga;
            if (l == LAST) {
                TRY(wgrad(l, [&](int z0, int Z, float* dw) -> int {
                    return conv_dw(L.dense(nullptr), cur + (size_t)z0 * L.out().sz, L.out(), map(l - 1) + (size_t)z0 * L.in().sz, L.in(), dw, Z, L.Lout,
                                   w.part, d.part_floats, s);
                }));
                for (int h = 0; h < nh; ++h) {
                    const size_t o = (size_t)h * Zh * L.in().sz;
                    Epi e{};
                    e.mask = map(l - 1) + o; e.mslope = slope; e.pre = up(l - 1) ? up(l - 1) + o : nullptr;
                    TRY(conv_dx(L.dense(W(l, h)), cur + (size_t)h * Zh * L.out().sz, L.out(), out + o, L.in(), Zh, L.Lin, e, s));
                }
            } else {
                TRY(wgrad(l, [&](int z0, int Z, float* dw) -> int {
                    HIP_TRY(ms_launch_gconv_dw(L.gconv(), cur + (size_t)z0 * L.out().sz, map(l - 1) + (size_t)z0 * L.in().sz, dw, Z, w.part,
                                               d.part_floats, s));
                    return PARROT_OK;
                }));
                HIP_TRY(ms_launch_gconv_dx(L.gconv(), cur, W(l, 0), W(l, 1), zs, up(l - 1), map(l - 1), slope, out, N, s));
            }
            cur = out;
        }
        // ---- convs[0] and the pools ------------------------------------------------------------------------------------------------
        const SLayer& L0 = sc.L[0];
        if (gr->layer[i][0].bias) HIP_TRY(vt_launch_chansum(cur, gr->layer[i][0].bias, N, L0.cout, sc.T, s));
        TRY(wgrad(0, [&](int z0, int Z, float* dw) -> int {
            HIP_TRY(ms_launch_first_dw(cur + (size_t)z0 * L0.out().sz, x + (size_t)z0 * sc.T, w.dpart, dw, Z, sc.T, L0.cout, s));
            return PARROT_OK;
        }));
        if (grad_wav) {
            HIP_TRY(ms_launch_first_dx(cur, W(0, 0), W(0, 1), zs, w.gwav[i], N, sc.T, L0.cout, s));
            if (i + 1 < d.S) HIP_TRY(ms_launch_pool_bwd(w.gwav[i + 1], w.gwav[i], N, sc.T, 1, s));
        }
    }
    return PARROT_OK;
}

// ---------------------------------------------------------------------------------------------
// Debug entry points (include/parrot_hip_debug.h): each new form alone.  Nothing is launched before the sizes are checked (the
// launchers of tu_msd_train.hip refuse what their kernels cannot take).
// ---------------------------------------------------------------------------------------------
namespace {
bool debug_gconv_ok(long Z, long cin, long cout, long G, long k, long stride, long Tin, MsGconv* d) {
    if (Z < 1 || Z > 65535 || cin < 1 || cin > 65535 || cout < 1 || cout > 65535 || G < 1 || k < 1 || !(k & 1) || k > MS_K || stride < 1 ||
        stride > MS_MAX_STRIDE || stride > k || Tin < 1 || Tin > 0x3fffffffL)
        return false;
    if (cin % G || cout % G) return false;
    *d = MsGconv{(int)cin, (int)cout, (int)G, (int)k, (int)stride, (int)(k - 1) / 2, (int)Tin, (int)((Tin - 1) / stride + 1)};
    return ms_gwgrad_part_floats(*d, (int)Z) > 0;  // (the launchers' own check, and the weight gradient's chunk limit below)
}
bool debug_first_ok(long Z, long T, long C) { return Z >= 1 && Z <= 65535 && T >= 1 && C >= 1 && C <= 65535 && Z * T * C <= 0x3fffffffL; }
}  // namespace

extern "C" int parrot_debug_msd_gconv_fwd(const float* x, const float* w, const float* bias, float* y, int32_t Z, int32_t c_in, int32_t c_out,
                                          int32_t groups, int32_t k, int32_t stride, int32_t T_in, int32_t act, float slope, void* stream) {
    MsGconv d{};
    if (!x || !w || !y) return fail(PARROT_E_INVALID, "debug_msd_gconv_fwd: null argument");
    if (!debug_gconv_ok(Z, c_in, c_out, groups, k, stride, T_in, &d)) return fail(PARROT_E_INVALID, "debug_msd_gconv_fwd: sizes outside the limits");
    HIP_TRY(ms_launch_gconv_fwd(d, x, w, w, Z, bias, y, Z, act ? 1 : 0, slope, (hipStream_t)stream));
    return PARROT_OK;
}
extern "C" int parrot_debug_msd_gconv_dx(const float* dy, const float* w, const float* pre, const float* mask, float slope, float* dx, int32_t Z,
                                         int32_t c_in, int32_t c_out, int32_t groups, int32_t k, int32_t stride, int32_t T_in, void* stream) {
    MsGconv d{};
    if (!dy || !w || !dx) return fail(PARROT_E_INVALID, "debug_msd_gconv_dx: null argument");
    if (!debug_gconv_ok(Z, c_in, c_out, groups, k, stride, T_in, &d)) return fail(PARROT_E_INVALID, "debug_msd_gconv_dx: sizes outside the limits");
    HIP_TRY(ms_launch_gconv_dx(d, dy, w, w, Z, pre, mask, slope, dx, Z, (hipStream_t)stream));
    return PARROT_OK;
}
extern "C" size_t parrot_debug_msd_gconv_dw_workspace_bytes(int32_t Z, int32_t c_in, int32_t c_out, int32_t groups, int32_t k, int32_t stride,
                                                            int32_t T_in) {
    MsGconv d{};
    if (!debug_gconv_ok(Z, c_in, c_out, groups, k, stride, T_in, &d) || ((long)Z * d.Tout + TG_RCHUNK - 1) / TG_RCHUNK > 65535) return 0;
    return ms_gwgrad_part_floats(d, Z) * sizeof(float);
}
extern "C" int parrot_debug_msd_gconv_dw(const float* dy, const float* x, float* dw, int32_t Z, int32_t c_in, int32_t c_out, int32_t groups, int32_t k,
                                         int32_t stride, int32_t T_in, void* ws, size_t ws_bytes, void* stream) {
    MsGconv d{};
    if (!dy || !x || !dw || !ws) return fail(PARROT_E_INVALID, "debug_msd_gconv_dw: null argument");
    const size_t need = parrot_debug_msd_gconv_dw_workspace_bytes(Z, c_in, c_out, groups, k, stride, T_in);
    if (!need || !debug_gconv_ok(Z, c_in, c_out, groups, k, stride, T_in, &d)) return fail(PARROT_E_INVALID, "debug_msd_gconv_dw: sizes outside the limits");
    if (ws_bytes < need) return fail(PARROT_E_INVALID, "debug_msd_gconv_dw: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    if (poison_word()) TRY(poison(ws, need, s));
    HIP_TRY(ms_launch_gconv_dw(d, dy, x, dw, Z, (float*)ws, need / sizeof(float), s));
    return PARROT_OK;
}
extern "C" int parrot_debug_msd_first_fwd(const float* wav, const float* w, const float* bias, float* y, int32_t Z, int32_t T, int32_t c1, float slope,
                                          void* stream) {
    if (!wav || !w || !bias || !y) return fail(PARROT_E_INVALID, "debug_msd_first_fwd: null argument");
    if (!debug_first_ok(Z, T, c1)) return fail(PARROT_E_INVALID, "debug_msd_first_fwd: sizes outside the limits");
    HIP_TRY(ms_launch_first_fwd(wav, w, w, Z, bias, y, Z, T, c1, slope, (hipStream_t)stream));
    return PARROT_OK;
}
extern "C" int parrot_debug_msd_first_dx(const float* dy, const float* w, float* dwav, int32_t Z, int32_t T, int32_t c1, void* stream) {
    if (!dy || !w || !dwav) return fail(PARROT_E_INVALID, "debug_msd_first_dx: null argument");
    if (!debug_first_ok(Z, T, c1)) return fail(PARROT_E_INVALID, "debug_msd_first_dx: sizes outside the limits");
    HIP_TRY(ms_launch_first_dx(dy, w, w, Z, dwav, Z, T, c1, (hipStream_t)stream));
    return PARROT_OK;
}
extern "C" size_t parrot_debug_msd_first_dw_workspace_bytes(int32_t Z, int32_t T, int32_t c1) {
    return debug_first_ok(Z, T, c1) ? (size_t)ms_chunks((long)Z * T) * c1 * MS_FIRST_K * sizeof(double) : 0;
}
extern "C" int parrot_debug_msd_first_dw(const float* dy, const float* wav, float* dw, int32_t Z, int32_t T, int32_t c1, void* ws, size_t ws_bytes,
                                         void* stream) {
    if (!dy || !wav || !dw || !ws) return fail(PARROT_E_INVALID, "debug_msd_first_dw: null argument");
    const size_t need = parrot_debug_msd_first_dw_workspace_bytes(Z, T, c1);
    if (!need) return fail(PARROT_E_INVALID, "debug_msd_first_dw: sizes outside the limits");
    if (ws_bytes < need) return fail(PARROT_E_INVALID, "debug_msd_first_dw: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    if (poison_word()) TRY(poison(ws, need, s));
    HIP_TRY(ms_launch_first_dw(dy, wav, (double*)ws, dw, Z, T, c1, s));
    return PARROT_OK;
}
extern "C" int parrot_debug_msd_pool_fwd(const float* x, float* y, int32_t Z, int32_t T, void* stream) {
    if (!x || !y) return fail(PARROT_E_INVALID, "debug_msd_pool_fwd: null argument");
    if (Z < 1 || Z > 65535 || T < 1 || (long)Z * T > 0x3fffffffL) return fail(PARROT_E_INVALID, "debug_msd_pool_fwd: sizes outside the limits");
    HIP_TRY(ms_launch_pool_fwd(x, y, Z, T, (hipStream_t)stream));
    return PARROT_OK;
}
extern "C" int parrot_debug_msd_pool_bwd(const float* dy, float* dx, int32_t Z, int32_t T, void* stream) {
    if (!dy || !dx) return fail(PARROT_E_INVALID, "debug_msd_pool_bwd: null argument");
    if (Z < 1 || Z > 65535 || T < 1 || (long)Z * T > 0x3fffffffL) return fail(PARROT_E_INVALID, "debug_msd_pool_bwd: sizes outside the limits");
    HIP_TRY(ms_launch_pool_bwd(dy, dx, Z, T, 0, (hipStream_t)stream));
    return PARROT_OK;
}
extern "C" int parrot_debug_msd_sn_fold(const float* w, float* u, float* v, int32_t rows, int32_t cols, int32_t iterate, float* wf, float* sigma,
                                        void* ws, size_t ws_bytes, void* stream) {
    if (!w || !u || !v || !wf || !sigma || !ws) return fail(PARROT_E_INVALID, "debug_msd_sn_fold: null argument");
    if (rows < 1 || cols < 1 || (long)rows * cols > 0x3fffffffL) return fail(PARROT_E_INVALID, "debug_msd_sn_fold: sizes outside the limits");
    const size_t need = ((size_t)rows + cols) * sizeof(float);
    if (ws_bytes < need) return fail(PARROT_E_INVALID, "debug_msd_sn_fold: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    if (poison_word()) TRY(poison(ws, need, s));
    HIP_TRY(ms_launch_sn_fold(w, u, v, rows, cols, iterate ? 1 : 0, wf, sigma, (float*)ws, s));
    return PARROT_OK;
}
extern "C" size_t parrot_debug_msd_sn_bwd_workspace_bytes(int32_t rows, int32_t cols) {
    if (rows < 1 || cols < 1 || (long)rows * cols > 0x3fffffffL) return 0;
    return (size_t)2 * (ms_chunks((long)rows * cols) + 1) * sizeof(double);
}
extern "C" int parrot_debug_msd_sn_bwd(const float* ga, const float* gb, const float* w, const float* ua, const float* va, const float* sa,
                                       const float* ub, const float* vb, const float* sb, float* dw, int32_t rows, int32_t cols, void* ws,
                                       size_t ws_bytes, void* stream) {
    if (!ga || !w || !ua || !va || !sa || !dw || !ws || (gb && (!ub || !vb || !sb))) return fail(PARROT_E_INVALID, "debug_msd_sn_bwd: null argument");
    const size_t need = parrot_debug_msd_sn_bwd_workspace_bytes(rows, cols);
    if (!need) return fail(PARROT_E_INVALID, "debug_msd_sn_bwd: sizes outside the limits");
    if (ws_bytes < need) return fail(PARROT_E_INVALID, "debug_msd_sn_bwd: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    if (poison_word()) TRY(poison(ws, need, s));
    HIP_TRY(ms_launch_sn_bwd(ga, gb, w, ua, va, sa, ub, vb, sb, dw, rows, cols, (double*)ws, s));
    return PARROT_OK;
}
