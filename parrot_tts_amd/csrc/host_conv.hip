// host_conv.hip -- the conv plan: weight packing at create, kernel choice at launch (conv_launch), the parrot_conv_* entries
// and the MFMA layout self test.
#include "host_common.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "conv_split.h"
#include "conv_split16.h"
#include "conv_mfma16.h"
#include "conv_valu.h"
#include "kernels_conv.h"
#include "weight_pack.h"

using namespace parrot;
static_assert(SchBf16x6::ID == PARROT_PREC_BF16X6 && SchF16x3::ID == PARROT_PREC_F16X3 && SchBf16::ID == PARROT_PREC_BF16 && SchF16::ID == PARROT_PREC_F16,
              "weight_pack.h reads a scheme off its PARROT_PREC_* number");

static int choose_cfg(int M, int k) {
    if (M <= 16) return 6;
    if (M <= 32) return 2;
    if (M <= 64) return 1;
    return (k <= 3) ? 3 : 0;
}

static bool valu_kernels_enabled() {
    static const bool on = [] { const char* e = getenv("PARROT_VALU_KERNELS"); return !e || atoi(e) != 0; }();
    return on;
}
static bool mfma16_enabled() {
    static const bool on = [] { const char* e = getenv("PARROT_MFMA16"); return !e || atoi(e) != 0; }();
    return on;
}
// PARROT_SMALL_TILES: 2 (default) = 64-column tiles for underfilled launches and 64-row tiles for far-underfilled ones, 1 = the
// 64-column tiles only, 0 = neither
static int small_tiles_mode() {
    static const int m = [] { const char* e = getenv("PARROT_SMALL_TILES"); return e ? atoi(e) : 2; }();
    return m;
}

// Build a plan.  `groups` > 1: torch grouped-conv weight layout (c_out, c_in/groups, k), d.c_in = TOTAL.
int parrot::conv_build(parrot_conv** out, const parrot_conv_desc* d, int groups, const float* w, const float* bias, bool allow16) {
    if (!out || !d || !w) return fail(PARROT_E_INVALID, "conv_create: null argument");
    if (d->c_in <= 0 || d->c_out <= 0 || d->k <= 0 || d->dilation <= 0 || groups <= 0 || d->c_in % groups || d->c_out % groups)
        return fail(PARROT_E_INVALID, "conv_create: bad dimensions");
    std::unique_ptr<parrot_conv> c(new parrot_conv());
    c->d = *d;
    c->groups = groups;
    c->Cout = d->c_out;
    c->Cin = d->c_in / groups;
    int dmin = 0;
    if (d->transposed) {
        if (d->stride > 64) return fail(PARROT_E_UNSUPPORTED, "conv_create: transposed stride > 64");
        if (groups != 1 || d->dilation != 1 || d->stride <= 0) return fail(PARROT_E_UNSUPPORTED, "conv_create: transposed conv needs groups=1, dilation=1");
        // polyphase gather form: output tau = t*u + r uses taps kappa = r + p - delta*u, input t + delta
        const int u = d->stride, p = d->padding, k = d->k;
        int dlo = 1 << 30, dhi = -(1 << 30);
        for (int r = 0; r < u; ++r)
            for (int kap = 0; kap < k; ++kap)
                if ((r + p - kap) % u == 0) {
                    int dl = (r + p - kap) / u;
                    dlo = std::min(dlo, dl);
                    dhi = std::max(dhi, dl);
                }
        if (dlo > dhi) return fail(PARROT_E_INVALID, "conv_create: transposed conv has no taps");
        dmin = dlo;
        c->u = u;
        c->kk = dhi - dlo + 1;
        c->dil = 1;
        c->pad_left = -dlo;
        c->M = d->c_out * u;
    } else {
        if (d->stride > 1) return fail(PARROT_E_UNSUPPORTED, "conv_create: strided Conv1d is not on the path");
        c->u = 1;
        c->kk = d->k;
        c->dil = d->dilation;
        c->pad_left = d->padding;
        c->M = d->c_out;
    }
    c->Mg = c->M / groups;
    if ((c->kk - 1) * c->dil > CONV_HALO) return fail(PARROT_E_UNSUPPORTED, "conv_create: (k-1)*dilation exceeds the LDS halo (64)");
    c->cfg = (d->tile_cfg >= 0) ? d->tile_cfg : choose_cfg(c->Mg, c->kk);
    if (c->cfg >= NUM_TILE_CFGS) return fail(PARROT_E_INVALID, "conv_create: tile_cfg out of range");
    if (c->cfg == 6 && (d->transposed || groups != 1 || c->M > 16)) {
        if (d->tile_cfg == 6) return fail(PARROT_E_UNSUPPORTED, "conv_create: the 16-row tile needs a plain conv with <= 16 output channels");
        c->cfg = 2;
    }
    const TileCfg t = tile_cfg(c->cfg);
    if (groups > 1 && c->Mg % t.bm) return fail(PARROT_E_UNSUPPORTED, "conv_create: rows per group must be a multiple of the tile height");
    const int CI = t.ci, QN = CI / 8;
    c->nchunks = (c->Cin + CI - 1) / CI;
    c->n_it = c->cfg == 6 ? c->nchunks * c->kk : c->nchunks * c->kk * QN;
    const int kk = c->kk;
    const GemmWeights W{w, c->M, c->Cin, d->k, d->transposed != 0, d->c_out, c->u, d->padding, dmin};
    const int want_prec = (d->precision >= 0) ? d->precision : create_prec();
    if (want_prec > PARROT_PREC_F16) return fail(PARROT_E_INVALID, "conv_create: unknown precision");
    // split kernels: at 32 rows the exact kernel is as fast (measured); the slab fetch needs whole 16-channel chunks
    // and evaluates the leaky ReLU as max(v, slope * v).  Everything else runs on the exact kernel (same results class).
    const bool slope_ok = d->pre_act != PRE_LRELU || (d->pre_slope >= 0.f && d->pre_slope <= 1.f);
    if (want_prec >= 1 && c->Mg >= 32 && d->tile_cfg < 0 && c->Cin % 16 == 0 && slope_ok) {
        // split plan: one MFMA k-step per (chunk, tap); [row tile][chunk*tap][piece][lane][8]
        c->prec = want_prec;
        c->cfg = (c->Mg <= 32) ? 2 : (c->Mg <= 64) ? 1 : 0;  // exact-kernel tile ids with the same block shapes
        const TileCfg t16 = tile_cfg(c->cfg);
        if (groups > 1 && c->Mg % t16.bm) return fail(PARROT_E_UNSUPPORTED, "conv_create: rows per group must be a multiple of the tile height");
        if (scheme_is_f16(want_prec)) c->wscale = f16_weight_scale(w, (size_t)d->c_in / groups * d->c_out * d->k);
        // wide plain convs: the 16x16x32 kernel (conv_split16.h): 16-row tiles, 32-channel chunks; else 32-row tiles, 16-channel chunks
        c->mfma16 = allow16 && mfma16_enabled() && split16_has(want_prec, c->kk) && !d->transposed && groups == 1 && c->Cin % 32 == 0 && c->M >= 64;
        int rows = 32, bm = t16.bm;
        if (c->mfma16) {
            int bn16;
            rows = 16;
            split16_tile(c->M >= 128 ? 0 : 1, bm, bn16);
        }
        const int chans = 512 / rows;  // channels of a chunk: 8 per lane group
        c->nchunks = (c->Cin + chans - 1) / chans;
        c->n_it16 = c->nchunks * c->kk;
        const size_t n_steps = (size_t)((c->M + bm - 1) / bm * (bm / rows)) * c->n_it16;
        const size_t n16 = (n_steps + 1) * scheme_pieces(want_prec) * 512;  // (+1 pad step: the kernels prefetch one past the end)
        if (n16 * sizeof(uint16_t) >= ((size_t)1 << 31)) return fail(PARROT_E_UNSUPPORTED, "conv_create: packed weight stream larger than 2 GiB");
        std::vector<uint16_t> pk16(n16, 0);
        const int n_it16 = c->n_it16;
        // step = (row tile, chunk, tap); lane: row = lane % rows, channels 8 * (lane / rows) .. + 7 of the chunk
        pack_pieces(pk16.data(), n_steps, want_prec, c->wscale, W, [=](size_t st, int lane, int e) {
            const int mt = (int)(st / n_it16), ch = (int)(st % n_it16) / kk, j = (int)(st % n_it16) % kk;
            return WeightAt{mt * rows + lane % rows, ch * chans + 8 * (lane / rows) + e, j};
        });
        HIP_TRY(hipMalloc((void**)&c->wfrag16, pk16.size() * sizeof(uint16_t)));
        HIP_TRY(hipMemcpy(c->wfrag16, pk16.data(), pk16.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    } else {
        const size_t n_steps = c->cfg == 6 ? (size_t)c->n_it : (size_t)((c->M + t.bm - 1) / t.bm * (t.bm / 32)) * c->n_it;
        std::vector<float> pk((n_steps + 1) * 256, 0.f);  // +1 group: the kernel prefetches one past the end
        if (c->cfg == 6)  // 16x16x4 fragments, step = (chunk, tap): row = lane&15, channel = 16*chunk + 4*e + (lane>>4)
            pack_f32(pk.data(), n_steps, W, [=](size_t st, int lane, int e) { return WeightAt{lane & 15, (int)st / kk * 16 + 4 * e + (lane >> 4), (int)st % kk}; });
        else {  // 32x32x2 fragments, step = (32-row tile, chunk, tap, channel octet q): row = lane&31, channel = CI*chunk + 8*q + 2*e + (lane>>5)
            const int n_it = c->n_it;
            pack_f32(pk.data(), n_steps, W, [=](size_t st, int lane, int e) {
                const int mt = (int)(st / n_it), r = (int)(st % n_it), q = r % QN, j = r / QN % kk, ch = r / QN / kk;
                return WeightAt{mt * 32 + (lane & 31), ch * CI + 8 * q + 2 * e + (lane >> 5), j};
            });
        }
        HIP_TRY(hipMalloc((void**)&c->wfrag, pk.size() * sizeof(float)));
        HIP_TRY(hipMemcpy(c->wfrag, pk.data(), pk.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    // the two narrowest vocoder layers stream through plain fp32 FMA kernels (conv_valu.h) in either precision mode
    if (d->tile_cfg < 0 && groups == 1 && slope_ok && d->dilation == 1 && valu_kernels_enabled()) {
        if (!d->transposed && d->c_out == 1 && ((d->k == 7 && d->padding == 3) || (d->k == 1 && d->padding == 0)) &&
            (d->act == ACT_NONE || d->act == ACT_TANH))
            c->valu_kind = 1;  // conv_post; the duration predictor's Linear(256 -> 1)
        if (d->transposed && d->c_out == 16 && d->k == 4 && d->stride == 2 && d->padding == 1 && d->act == ACT_NONE) c->valu_kind = 2;
        if (c->valu_kind) {
            const size_t n = (size_t)d->c_in * d->c_out * d->k;
            HIP_TRY(hipMalloc((void**)&c->wraw, n * sizeof(float)));
            HIP_TRY(hipMemcpy(c->wraw, w, n * sizeof(float), hipMemcpyHostToDevice));
        }
    }
    if (bias) {
        HIP_TRY(hipMalloc((void**)&c->bias, (size_t)d->c_out * sizeof(float)));
        HIP_TRY(hipMemcpy(c->bias, bias, (size_t)d->c_out * sizeof(float), hipMemcpyHostToDevice));
    }
    *out = c.release();
    return PARROT_OK;
}

int parrot::conv_launch(const parrot_conv* c, const float* x, const float* res, float* y, int B, int Tin, int epi, float div, hipStream_t s,
                        const ConvOpts& o) {
    const PlaneArgs& pl = o.planes;
    if (B <= 0 || Tin <= 0) return fail(PARROT_E_INVALID, "conv_run: empty batch or sequence");
    const int Tout = c->out_len(Tin);
    if (Tout <= 0) return fail(PARROT_E_INVALID, "conv_run: sequence shorter than the kernel");
    if (c->valu_kind && !res && epi == EPI_STORE && (double)c->d.c_in * Tin * 4.0 < 2147483648.0) {
        ConvValuParams q{};
        q.x = x; q.w = c->wraw; q.bias = c->bias; q.y = y;
        q.B = B; q.Cin = c->d.c_in; q.Tin = Tin; q.Tout = Tout;
        q.slope = c->d.pre_act == PRE_LRELU ? c->d.pre_slope : 1.f;
        q.act = c->d.act;
        q.row_len = o.rows.len; q.row_len_mul = o.rows.mul; q.row_len_add = o.rows.add;
        q.err = c->err_flag;
        ProfRec rec{};
        const double macs = (double)B * c->d.c_out * c->d.c_in * c->d.k * (c->d.transposed ? (double)Tin : (double)Tout);
        if (prof_on()) TRY(prof_open(rec, c->valu_kind == 1 ? PROF_VALU_CONV1 : PROF_VALU_CONVT, 2.0 * macs, 4.0 * B * ((double)c->d.c_in * Tin + (double)c->d.c_out * Tout), s));
        if (c->valu_kind == 1 && c->d.k == 7 && (Tin & 3) == 0 && (reinterpret_cast<size_t>(x) & 15) == 0 && (reinterpret_cast<size_t>(y) & 15) == 0)
            hipLaunchKernelGGL(conv1_valu7_vec_kernel, dim3((Tout + 1023) / 1024, B), dim3(256), 0, s, q);
        else if (c->valu_kind == 1 && c->d.k == 7) hipLaunchKernelGGL(conv1_valu_kernel<7>, dim3((Tout + 1023) / 1024, B), dim3(256), 0, s, q);
        else if (c->valu_kind == 1) hipLaunchKernelGGL(linear1_valu_kernel, dim3((Tout + 63) / 64, B), dim3(256), 0, s, q);
        else hipLaunchKernelGGL((convt_valu_kernel<16, 4, 2, 1>), dim3((Tin + 255) / 256, B), dim3(256), 0, s, q);
        HIP_TRY(hipGetLastError());
        if (prof_on()) TRY(prof_close(rec, s));
        return PARROT_OK;
    }
    ConvParams p{};
    p.x = x; p.wfrag = c->wfrag; p.bias = c->bias; p.res = res; p.y = y;
    p.B = B; p.Cin = c->Cin; p.Tin = Tin; p.M = c->M; p.Cout = c->Cout;
    p.Ncols = (c->u > 1) ? (Tout + c->u - 1) / c->u : Tout;
    p.Tout = Tout;
    p.k = c->kk; p.dil = c->dil; p.pad_left = c->pad_left;
    p.nchunks = c->nchunks; p.n_it = c->n_it;
    p.pre = c->d.pre_act; p.pre_slope = c->d.pre_slope; p.act = c->d.act;
    p.epi = epi; p.div = div; p.u = c->u; p.u_inv16 = (65536 + c->u - 1) / c->u;
    p.groups = c->groups; p.Mg = c->Mg;
    p.row_len = o.rows.len; p.row_len_mul = o.rows.mul; p.row_len_add = o.rows.add;
    p.acc_scale = p.out_scale = 1.f;
    p.lean = 1;  // conv_split_kernel: the buffer-addressed prologue / epilogue instantiations for plain convs (conv_lean_ok)
    p.n_cus = num_cus();
    p.fold_res = c->late_res ? 0 : 1;
    if (pl.xplane || pl.yplane) {
        if (!plane_ok(c) || (pl.yplane && epi != EPI_STORE)) return fail(PARROT_E_INVALID, "conv_run: operand planes need a conv_split16 layer (k = 7 / 11) and EPI_STORE");
        p.xplane = pl.xplane; p.yplane = pl.yplane;
        p.xplane_bstride = (long)plane_row_bytes(c->prec, c->Cin, Tin);
        p.yplane_bstride = (long)plane_row_bytes(c->prec, c->M, Tout);
        p.yplane_slope = pl.yslope; p.plane_only = pl.plane_only;
    }
    p.x_bstride = (long)c->d.c_in * Tin;  // (dense batch rows)
    p.y_bstride = (long)c->Cout * Tout;
    p.res_bstride = p.y_bstride;
    int cfg = c->cfg;
    if (c->prec == 0 && (cfg == 0 || cfg == 3) && p.Ncols <= 64 && tile_cfg(4).ci == tile_cfg(cfg).ci) cfg = 4;  // same packing, narrower tile
    if (c->prec >= 1) {
        p.wfrag = reinterpret_cast<const float*>(c->wfrag16);
        p.n_it = c->n_it16;
        p.acc_scale = scheme_xs(c->prec) * c->wscale;
        p.out_scale = 1.f / p.acc_scale;
        // 32-bit byte offsets inside one batch row (buffer addressing of the slab fetch)
        if ((double)c->Cin * Tin * 4.0 >= 2147483648.0) return fail(PARROT_E_UNSUPPORTED, "conv_run: batch row larger than 2 GiB");
    }
    TileCfg t = tile_cfg(cfg);
    int variant16 = 0;
    const bool small_tiles = small_tiles_mode() >= 1;
    if (c->mfma16) {
        variant16 = c->M >= 128 ? 0 : 1;
        split16_tile(variant16, t.bm, t.bn, c->kk);
        // small batches: a launch that would not give every CU a workgroup takes the 64-column tiles (2-3x the workgroups,
        // a half / third of the MFMAs per step: the per-launch latency is what counts there, not the operand reuse)
        if (small_tiles && (long)((p.Ncols + t.bn - 1) / t.bn) * B * ((c->M + t.bm - 1) / t.bm) < num_cus()) {
            variant16 += 2;
            // ... and 64-row workgroups for the 128-row layers when even that leaves more than half of the CUs idle (one to four
            // utterances): four waves per workgroup, one per SIMD, twice the workgroups -- single utterance 2.08 -> 2.00 ms, B = 4
            // 2.63 -> 2.57 ms; 32-row workgroups (2 waves, four slab items per thread) measured slower (2.11 / 2.69 ms)
            split16_tile(variant16, t.bm, t.bn, c->kk);
            if (small_tiles_mode() >= 2 && (long)((p.Ncols + t.bn - 1) / t.bn) * B * ((c->M + t.bm - 1) / t.bm) * 2 <= num_cus() && c->M >= 128) variant16 = 3;
        } else if (small_tiles && p.Ncols <= 64) variant16 += 2;  // sequences of <= 64 steps (the TTE encoder side) would leave half of a 128-column tile empty
        else if (variant16 == 0 && split16_wide_fits(p.Ncols, B, (c->M + 127) / 128, num_cus())) variant16 = 4;  // 128 x 160: no half-empty last round
        split16_tile(variant16, t.bm, t.bn, c->kk);
        // conv_split16_kernel addresses the (M, Tout) output / residual tile of a batch row with 32-bit byte offsets (RowTile)
        if ((double)c->M * Tout * 4.0 >= 2147483648.0) return fail(PARROT_E_UNSUPPORTED, "conv_run: output row tile larger than 2 GiB");
        {   // rows that start on 16-byte boundaries take the 16-byte epilogue (round-4 A/B on one box, profiles/r04a_*: the dominant
            // kernel 231.0 us per launch with it, 231.1 us without -- the C/D-layout stores were not what bounds the epilogue)
            auto al16 = [](const void* q, long stride) { return (reinterpret_cast<size_t>(q) & 15) == 0 && (stride & 3) == 0; };
            p.epi16 = (Tout % 4 == 0) && al16(y, p.y_bstride) && (!res || al16(res, p.res_bstride));
        }
    } else if (c->prec >= 1) {
        // 1x1 convs (Linear layers) have one MFMA step per barrier: the 128x64 / 3-waves-per-SIMD variant hides that
        // better (76 vs 61 TF on the qkv projection); every other layer is faster on the 64x64 wave tile
        // (and so are sequences of <= 64 steps -- the TTE encoder side -- which would leave half of a 128-column tile empty)
        const bool few = small_tiles && cfg == 0 && (c->kk == 3 || c->kk == 9) && (long)((p.Ncols + 127) / 128) * B * ((c->M + 127) / 128) < num_cus();
        variant16 = (cfg == 2) ? 3 : (cfg == 0 && (c->kk == 1 || p.Ncols <= 64 || few)) ? 2 : cfg;
        split_tile(variant16, t.bm, t.bn);
    }
    p.tiles_n = (p.Ncols + t.bn - 1) / t.bn;
    ProfRec rec{};
    if (prof_on()) {
        // algorithmic work of the layer (real taps only; DESIGN.md "roofline accounting")
        const double macs = (double)B * c->d.c_out * c->Cin * c->d.k * (c->d.transposed ? (double)Tin : (double)Tout);
        const double elems = (double)B * ((double)c->d.c_in * Tin + (double)c->Cout * Tout * (1 + (res ? 1 : 0) + (epi != EPI_STORE ? 1 : 0)));
        const int row = c->mfma16 ? (variant16 == 4 ? PROF_SPLIT16_WIDE : (variant16 & 1) ? PROF_SPLIT16_ODD : PROF_SPLIT16)
                                  : (c->prec >= 1) ? (variant16 == 2 ? PROF_SPLIT_V2 : variant16 == 3 ? PROF_SPLIT_V3 : PROF_SPLIT + cfg) : cfg;  // (exact kernels: row = tile id)
        TRY(prof_open(rec, row, 2.0 * macs, 4.0 * (elems + (double)c->d.c_out * c->Cin * c->d.k), s));
    }
    HIP_TRY(c->mfma16 ? launch_conv_split16(c->prec, variant16, p, s) : c->prec >= 1 ? launch_conv_split(c->prec, variant16, p, s) : (cfg == 6 ? launch_conv_mfma16(p, s) : launch_conv(cfg, p, s)));
    if (c->d.act == ACT_TANH) {  // dense (B, Cout, Tout) output assumed for the tanh layers (conv_post)
        const size_t n = (size_t)B * c->Cout * Tout;
        hipLaunchKernelGGL(tanh_inplace_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, y, n, c->err_flag);
        HIP_TRY(hipGetLastError());
    }
    if (prof_on()) TRY(prof_close(rec, s));
    return PARROT_OK;
}

int parrot::upload(float** dst, const float* src, size_t n) {
    HIP_TRY(hipMalloc((void**)dst, n * sizeof(float)));
    HIP_TRY(hipMemcpy(*dst, src, n * sizeof(float), hipMemcpyHostToDevice));
    return PARROT_OK;
}

int parrot::make_conv(std::unique_ptr<parrot_conv>& slot, int cin, int cout, int k, int dil, int pad, int transposed, int stride, int pre,
                      float slope, int act, const float* w, const float* b, int groups, bool allow16) {
    parrot_conv_desc d{};
    d.c_in = cin; d.c_out = cout; d.k = k; d.dilation = dil; d.padding = pad; d.transposed = transposed; d.stride = stride;
    d.pre_act = pre; d.pre_slope = slope; d.act = act; d.tile_cfg = -1; d.precision = -1;
    parrot_conv* c = nullptr;
    TRY(conv_build(&c, &d, groups, w, b, allow16));
    slot.reset(c);
    return PARROT_OK;
}

extern "C" int parrot_conv_create(parrot_conv_t** out, const parrot_conv_desc* d, const float* w_host, const float* bias_host) {
    return conv_build(out, d, 1, w_host, bias_host);
}
extern "C" void parrot_conv_destroy(parrot_conv_t* c) { delete c; }
extern "C" int parrot_conv_out_len(const parrot_conv_t* c, int32_t T_in) { return c ? c->out_len(T_in) : PARROT_E_INVALID; }
extern "C" int parrot_conv_num_tile_cfgs(void) { return NUM_TILE_CFGS; }
extern "C" int parrot_conv_run(parrot_conv_t* c, const float* x, const float* res, float* y, int32_t B, int32_t T_in,
                               int32_t epilogue, float div, void* stream) {
    if (!c || !x || !y) return fail(PARROT_E_INVALID, "conv_run: null argument");
    if (epilogue < 0 || epilogue > 2) return fail(PARROT_E_INVALID, "conv_run: bad epilogue");
    if (epilogue == EPI_STORE && y != x && y != res && c->out_len(T_in) > 0)
        TRY(poison(y, (size_t)B * c->Cout * c->out_len(T_in) * sizeof(float), (hipStream_t)stream));
    return conv_launch(c, x, res, y, B, T_in, epilogue, div, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// self test: MFMA fragment layout
// ---------------------------------------------------------------------------------------------
extern "C" int parrot_selftest(void* stream) {
    float* d = nullptr;
    HIP_TRY(hipMalloc((void**)&d, 64 * 16 * sizeof(float)));
    hipLaunchKernelGGL(mfma_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, d);
    std::vector<float> h(64 * 16);
    hipError_t e = hipMemcpy(h.data(), d, h.size() * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(PARROT_E_HIP, hipGetErrorString(e));
    for (int lane = 0; lane < 64; ++lane)
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), col = lane & 31;
            const float want = (float)(col + 1) * (float)(1001 * row + 100000);
            if (h[lane * 16 + r] != want) {
                char buf[160];
                snprintf(buf, sizeof buf, "mfma 32x32x2 layout probe: lane %d reg %d got %g want %g", lane, r, h[lane * 16 + r], want);
                return fail(PARROT_E_UNSUPPORTED, buf);
            }
        }
    return PARROT_OK;
}
