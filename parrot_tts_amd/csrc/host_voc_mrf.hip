// host_voc_mrf.hip -- how the MRF of a vocoder stage is run: the choice between the whole-stage, pair-kernel, fused and
// layer-by-layer launches, the branch-stream fork / join (mrf_stage), and the create-time half of the same knowledge, the ResBlock
// weight streams (mrf_create).  The only unit that includes resblock_fused.h: those kernels are instantiated wherever
// launch_resblock_fused is called, and a second includer would emit a second copy.
#include "voc.h"

#include "resblock_split.h"
#include "resblock_fused.h"
#include "weight_pack.h"

using namespace parrot;

// One fused launch for ResBlock (stage i, kernel j) when the stage is narrow enough to live in LDS.
// Fused whole-ResBlock kernels (resblock_fused.h): mode 0 off, 1 every eligible stage (16 and 32 channels), 2 only the
// 16-channel stages.  Default 2: measured at B=64, the 16-channel kernel (16x16x4 MFMA, 1024-column windows) beats
// the layer-by-layer path (5.3 vs 6.6 ms for stage 4) while the 32-channel one does not yet (10.5 vs 8.5 ms for
// stage 3: 512-column windows pay 12-23 % halo recompute).  PARROT_FUSED / parrot_set_fused_resblocks override.
static bool resblock_fusable(const parrot_voc* v, int stage, int j) {
    const parrot_voc_cfg& c = v->cfg;
    const int C = v->chan(stage), k = c.resblock_kernel_sizes[j];
    const int fm = v->fused;
    if (fm == 0 || !(C == 16 || (C == 32 && fm == 1)) || !(k & 1)) return false;
    const int per_rb = v->per_rb(), base = v->rb_base(stage, j);
    if (per_rb > RB_MAX_CONVS) return false;
    for (int m = 0; m < c.n_dil; ++m)
        if ((k - 1) / 2 * c.resblock_dilation_sizes[j][m] > RB_PAD) return false;
    for (int q = 0; q < per_rb; ++q)
        if (v->rb[base + q]->prec != 0 || v->rb[base + q]->cfg != (C == 16 ? 6 : 2) || !v->rb[base + q]->wfrag) return false;
    return resblock_window(C) - 2 * v->branch_reach(stage, j) >= 128;
}
static int resblock_fused_launch(const parrot_voc* v, int stage, int j, const Branch& br) {
    const int B = br.B, T = br.T;
    const parrot_voc_cfg& c = v->cfg;
    const int per_rb = v->per_rb(), base = v->rb_base(stage, j);
    ResblockParams p{};
    p.x = br.x; p.y = br.y;
    p.n_conv = per_rb; p.type = c.resblock_type;
    p.k = c.resblock_kernel_sizes[j]; p.C = v->chan(stage); p.T = T; p.B = B;
    p.epi = br.epi; p.div = br.div; p.slope = 0.1f;
    p.row_len = br.rows.len; p.row_len_mul = br.rows.mul; p.row_len_add = br.rows.add;
    double macs = 0;
    for (int q = 0; q < per_rb; ++q) {
        const parrot_conv* pc = v->rb[base + q].get();
        p.wfrag[q] = pc->wfrag; p.bias[q] = pc->bias; p.dil[q] = pc->dil;
        macs += (double)B * p.C * p.C * p.k * T;
    }
    p.H = v->branch_reach(stage, j);
    p.TT = resblock_window(p.C) - 2 * p.H;
    p.tiles = (T + p.TT - 1) / p.TT;
    ProfRec rec{};
    if (br.before_last) HIP_TRY(hipStreamWaitEvent(br.s, br.before_last, 0));
    if (prof_on()) TRY(prof_open(rec, PROF_RESBLOCK_FUSED, 2.0 * macs, 4.0 * B * (double)p.C * T * (2 + (br.epi != EPI_STORE ? 1 : 0)), br.s));
    HIP_TRY(launch_resblock_fused(p, br.s));
    if (prof_on()) TRY(prof_close(rec, br.s));
    return PARROT_OK;
}

// Split-bf16 fused pair kernel for a 32-channel ResBlock1 block: the pairs are grouped into launches whose total reach
// stays <= hmax columns per side (a 384-column window keeps >= 84 % of its columns at hmax = 30); every launch but
// the last stores its running residual to a scratch buffer.
constexpr int RBS_HMAX = 30;
static int resblock_split_launch(const parrot_voc* v, int stage, int j, const Branch& br) {
    const int B = br.B, T = br.T;
    hipStream_t s = br.s;
    const parrot_voc_cfg& c = v->cfg;
    const int per_rb = v->per_rb(), base = v->rb_base(stage, j), k = c.resblock_kernel_sizes[j], C = v->chan(stage);
    const int W = resblock_split_window(C);
    const int hmax = RBS_HMAX * W / RBS_W;  // the same fraction of the window
    const uint16_t* stream = v->branch_stream(stage, j);
    const float* src = br.x;
    int m0 = 0, n_launch = 0;
    while (m0 < per_rb) {
        int m1 = m0, H = 0;
        while (m1 < per_rb) {
            const int h2 = (k - 1) / 2 * (v->rb[base + m1]->dil + v->rb[base + m1 + 1]->dil);
            if (m1 > m0 && H + h2 > hmax) break;
            H += h2;
            m1 += 2;
        }
        const bool last = (m1 == per_rb);
        ResblockSplitParams p{};
        p.x = src;
        p.y = last ? br.y : ((n_launch & 1) ? br.res_b : br.res_a);
        p.wstream = stream + (size_t)m0 * v->rb_conv_halves[v->branch(stage, j)];
        p.n_conv = m1 - m0;
        p.early = 1;
        for (int q = m0; q < m1; ++q) {
            p.bias[q - m0] = v->rb[base + q]->bias;
            p.wsc[q - m0] = v->rb_wsc[base + q];
            p.dil[q - m0] = v->rb[base + q]->dil;
            if ((k - 1) / 2 * v->rb[base + q]->dil > 32) p.early = 0;
        }
        p.T = T; p.B = B; p.H = H; p.k = k;
        p.TT = W - 2 * H;
        if (p.TT < 32) return fail(PARROT_E_UNSUPPORTED, "resblock: receptive field too wide for the fused window");
        p.tiles = (T + p.TT - 1) / p.TT;
        p.epi = last ? br.epi : EPI_STORE;
        p.div = br.div; p.slope = 0.1f;
        p.row_len = br.rows.len; p.row_len_mul = br.rows.mul; p.row_len_add = br.rows.add;
        ProfRec rec{};
        const double macs = (double)B * C * C * k * T * (m1 - m0);
        if (last && br.before_last) HIP_TRY(hipStreamWaitEvent(s, br.before_last, 0));  // the MRF sum is accumulated in branch order
        // rows: one per kernel instantiation (C = 32 / 64 / 128 / 256 are resblock_split_kernel<SCH, 2 / 4 / 8 / 16>)
        const ProfRow prow = C == 16 ? PROF_RBS_16 : C == 32 ? PROF_RBS_32 : C == 64 ? PROF_RBS_64 : C == 128 ? PROF_RBS_128 : PROF_RBS_256;
        if (prof_on()) TRY(prof_open(rec, prow, 2.0 * macs, 4.0 * B * (double)C * T * (2 + (p.epi != EPI_STORE ? 1 : 0)), s));
        HIP_TRY(launch_resblock_split(v->scheme, C, p, s));
        if (prof_on()) TRY(prof_close(rec, s));
        src = p.y;
        m0 = m1;
        ++n_launch;
    }
    return PARROT_OK;
}

// output columns per window of a whole-MRF launch of this stage (window minus twice the widest branch's total reach)
static int mrf_tile_cols(const parrot_voc* v, int stage) {
    return std::max(1, rbs_mrf_window(v->chan(stage)) - 2 * v->stage_reach(stage));
}
// Whole-MRF launch of the 32-channel stage (resblock_split.h, MRF instantiations): y = sum_j ResBlock_j(x) / n_kernels.
static int mrf_split_launch(const parrot_voc* v, int stage, const float* x, float* y, int B, int T, hipStream_t s, const RowLens& rows) {
    const parrot_voc_cfg& c = v->cfg;
    const int per_rb = v->per_rb(), C = v->chan(stage), nk = c.n_kernels;
    const int W = rbs_mrf_window(C);
    ResblockSplitParams p{};
    p.x = x; p.y = y;
    p.n_conv = per_rb; p.n_branch = nk;
    const int Hmax = v->stage_reach(stage);
    int early = 1;
    double macs = 0;
    for (int j = 0; j < nk; ++j) {
        const int base = v->rb_base(stage, j), k = c.resblock_kernel_sizes[j];
        p.bstream[j] = v->branch_stream(stage, j);
        p.bk[j] = k;
        for (int q = 0; q < per_rb; ++q) {
            p.bias[j * per_rb + q] = v->rb[base + q]->bias;
            p.wsc[j * per_rb + q] = v->rb_wsc[base + q];
            p.dil[j * per_rb + q] = v->rb[base + q]->dil;
            if ((k - 1) / 2 * v->rb[base + q]->dil > 32) early = 0;
        }
        macs += (double)B * C * C * k * T * per_rb;
    }
    p.k = p.bk[0];
    p.early = early;
    p.T = T; p.B = B; p.H = Hmax;
    p.TT = W - 2 * Hmax;
    p.tiles = (T + p.TT - 1) / p.TT;
    p.epi = nk > 1 ? EPI_ADD_DIV : EPI_STORE;
    p.div = (float)nk; p.slope = 0.1f;
    p.row_len = rows.len; p.row_len_mul = rows.mul; p.row_len_add = rows.add;
    ProfRec rec{};
    if (prof_on()) TRY(prof_open(rec, PROF_MRF, 2.0 * macs, 4.0 * B * (double)C * T * 2, s));
    HIP_TRY(launch_mrf_split(v->scheme, C, p, s));
    if (prof_on()) TRY(prof_close(rec, s));
    return PARROT_OK;
}

// A ResBlock branch layer by layer: one conv launch per layer, the running residual alternating between res_a and res_b.
static int resblock_layers_launch(const parrot_voc* v, int stage, int j, const Branch& br) {
    const parrot_voc_cfg& c = v->cfg;
    const int base = v->rb_base(stage, j), nd = c.n_dil, B = br.B, T = br.T;
    const size_t n_act = (size_t)B * v->chan(stage) * T;
    ConvOpts o;
    o.rows = br.rows;
    // Operand planes (conv_split16.h; PARROT_PLANES=0 switches them off): the tensor between the two convs of a pair
    // exists only as the second conv's ready-made operand -- written once by the first conv's epilogue, the same
    // bytes per element as the fp32 tensor it replaces (two fp16 pieces), bit-identical operands -- and, in the
    // single-piece modes (bf16 / f16: 2 bytes per element), each pair's output is written as a plane beside the
    // fp32 residual, so that the next pair's first conv converts nothing either.
    bool planes = v->planes && !v->dbg_absmax && c.resblock_type == 1;
    for (int q = 0; q < v->per_rb() && planes; ++q) planes = plane_ok(v->rb[base + q].get());
    const bool dual = planes && v->scheme != PARROT_PREC_F16X3;  // (one piece: the two planes share mid's 4 C T bytes per row)
    char* const plane_a = reinterpret_cast<char*>(br.mid);
    char* const plane_b = plane_a + (size_t)B * plane_row_bytes(v->scheme, v->chan(stage), T);
    auto slope_of = [&](int q) { return v->rb[base + q]->d.pre_act == PRE_LRELU ? v->rb[base + q]->d.pre_slope : 1.f; };
    const void* xin = nullptr;  // plane of `r` for the next first conv (dual mode)
    const float* r = br.x;
    for (int m = 0; m < nd; ++m) {
        const bool last = (m == nd - 1);
        float* dst = last ? br.y : ((m & 1) ? br.res_b : br.res_a);
        if (m > 0) TRY(voc_amax(v, 1 + stage, r, n_act, br.s));
        if (c.resblock_type == 1) {
            o.planes = PlaneArgs();
            o.planes.xplane = xin;
            if (planes) { o.planes.yplane = plane_a; o.planes.plane_only = 1; o.planes.yslope = slope_of(2 * m + 1); }
            TRY(conv_launch(v->rb[base + 2 * m].get(), r, nullptr, br.mid, B, T, EPI_STORE, 1.f, br.s, o));
            TRY(voc_amax(v, 1 + stage, br.mid, n_act, br.s));
        }
        if (last && br.before_last) HIP_TRY(hipStreamWaitEvent(br.s, br.before_last, 0));
        if (c.resblock_type == 1) {
            o.planes = PlaneArgs();
            if (planes) o.planes.xplane = plane_a;
            if (dual && !last) { o.planes.yplane = plane_b; o.planes.yslope = slope_of(2 * m + 2); xin = plane_b; }
            TRY(conv_launch(v->rb[base + 2 * m + 1].get(), br.mid, r, dst, B, T, last ? br.epi : EPI_STORE, br.div, br.s, o));
        } else
            TRY(conv_launch(v->rb[base + m].get(), r, r, dst, B, T, last ? br.epi : EPI_STORE, br.div, br.s, o));
        r = dst;
    }
    return PARROT_OK;
}

// The MRF of a stage, y = sum_j ResBlock_j(x) / n_kernels, is one of four things:
//   the whole stage in ONE launch (mrf_split_launch) when mrf_whole() says so; else per branch j, on its own stream when ns > 1,
//   the split pair kernel (resblock_split_launch) | the fused exact kernel (resblock_fused_launch) | layer by layer.
// Which kernel family runs a block never depends on the batch size or on the launch size: row b of a batch must equal the same
// utterance run alone BIT FOR BIT -- the batched driver's byte-identical WAVs rest on it.  (At B = 1 the 96-column windows of the
// 128- / 256-channel pair kernels are only 16-61 workgroups: 3.4 instead of 3.2 ms per utterance.)  The one exception is the whole-MRF
// launch, which has the same bits as the per-branch pair kernels at 32 channels.
// (the fused kernels address a batch row with 32-bit byte offsets: rows of 2 GiB and more go layer by layer)
static bool row_fits_32bit(const parrot_voc* v, int stage, int T) { return (double)v->chan(stage) * T * 4.0 < 2147483648.0; }
// every branch of the stage in ONE launch -- when that launch fills the chip twice over (one 512-thread workgroup per CU
// walks 18 convs: a few windows are faster as per-branch launches on the branch streams; same bits either way at 32 channels)
static bool mrf_whole(const parrot_voc* v, int stage, int B, int T) {
    return v->mrf_ok[stage] && row_fits_32bit(v, stage, T) && (long)B * ((T + mrf_tile_cols(v, stage) - 1) / mrf_tile_cols(v, stage)) >= 2L * num_cus();
}
static int branch_launch(const parrot_voc* v, int stage, int j, const Branch& br) {
    if (v->fused != 0 && v->branch_stream(stage, j) && row_fits_32bit(v, stage, br.T)) return resblock_split_launch(v, stage, j, br);
    if (resblock_fusable(v, stage, j)) return resblock_fused_launch(v, stage, j, br);
    return resblock_layers_launch(v, stage, j, br);
}

// The MRF of stage `stage` on stream s: XS = sum_j ResBlock_j(X) / n_kernels, ns branches at a time (ns > 1: the caller holds
// side_mu), each with its own (mid, res_a, res_b) of w.
int parrot::mrf_stage(const parrot_voc* v, int stage, const float* X, float* XS, const VocScratch& w, int B, int T, hipStream_t s, int ns,
                      const RowLens& rows) {
    const int nk = v->cfg.n_kernels;
    const size_t n_act = (size_t)B * v->chan(stage) * T;
    const parrot_voc::StreamSet& ss = v->ss;
    if (mrf_whole(v, stage, B, T)) {
        TRY(voc_amax(v, 1 + stage, X, n_act, s));
        return mrf_split_launch(v, stage, X, XS, B, T, s, rows);
    }
    if (ns > 1) {  // fork: the side streams see the upsampled stage input
        HIP_TRY(hipEventRecord(ss.ev_fork, s));
        for (int j = 1; j < ns; ++j) HIP_TRY(hipStreamWaitEvent(ss.side[j], ss.ev_fork, 0));
    }
    for (int j = 0; j < nk; ++j) {
        // the longest branch (largest kernel size = last) stays on the caller's stream
        const int slot = (ns > 1) ? (j + 1) % nk : 0;
        if (j == 0) TRY(voc_amax(v, 1 + stage, X, n_act, s));  // the stage input feeds the first conv of every branch
        Branch br{};
        br.x = X; br.y = XS;
        br.mid = w.tmp[slot].mid; br.res_a = w.tmp[slot].res_a; br.res_b = w.tmp[slot].res_b;
        br.B = B; br.T = T;
        br.epi = (nk == 1 || j == 0) ? EPI_STORE : (j == nk - 1 ? EPI_ADD_DIV : EPI_ADD);
        br.div = (float)nk;
        br.s = (slot == 0) ? s : ss.side[slot];
        br.rows = rows;
        br.before_last = (ns > 1 && j > 0) ? ss.ev_last[j - 1] : nullptr;  // XS accumulates in branch order (models.py:100-106)
        TRY(branch_launch(v, stage, j, br));
        if (ns > 1) HIP_TRY(hipEventRecord(ss.ev_last[j], br.s));
    }
    if (ns > 1)  // join: every branch (and with it every reader of X and of the branch temporaries) is done
        for (int j = 0; j < nk; ++j) HIP_TRY(hipStreamWaitEvent(s, ss.ev_last[j], 0));
    return PARROT_OK;
}

// block (stage, j) has a fused pair kernel: its convs keep the 32x32x16 packing of their plans (voc_create) and get a weight stream
bool parrot::mrf_pair_shape(const parrot_voc* v, int stage, int j) {
    return v->cfg.resblock_type == 1 && resblock_split_has(v->chan(stage), v->cfg.resblock_kernel_sizes[j]) && v->per_rb() <= RBS_MAX_CONVS;
}

// Create time, after the ResBlock conv plans: the weight streams of the pair kernels and which stages run as one launch.
int parrot::mrf_create(parrot_voc* v, const parrot_voc_weights* w) {
    const parrot_voc_cfg* cfg = &v->cfg;
    const int per_rb = v->per_rb();
    // ResBlock1 blocks of the 64-, 32- and 16-channel stages under a split scheme: one concatenated weight stream per
    // block for the fused pair kernels (resblock_split.h), [conv][step][piece][lane][8 x 16 bit] + padding for the prefetch past the end.
    //   32 / 64 channels: the conv plans' own streams ([row tile][chunk * k + tap]);
    //   16 channels: packed here for the 16x16x32 MFMA (step = tap pair; lane = row l&15, channels 8(g&1).., tap 2*step + (g>>1)).
    v->rb_stream.assign((size_t)cfg->n_stages * cfg->n_kernels, nullptr);
    v->rb_wsc.assign((size_t)w->n_rb, 1.f);
    v->rb_conv_halves.assign((size_t)cfg->n_stages * cfg->n_kernels, 0);
    const int NP = scheme_pieces(v->scheme);
    for (int i = 0; i < cfg->n_stages && v->scheme >= 1; ++i)
        for (int j = 0; j < cfg->n_kernels; ++j) {
            const int rk = cfg->resblock_kernel_sizes[j], C = v->chan(i);
            if (!mrf_pair_shape(v, i, j)) continue;
            const int base = v->rb_base(i, j);
            const int steps = resblock_split_steps(C, rk);
            const size_t step_b = (size_t)NP * 1024, conv_b = (size_t)steps * step_b;
            v->rb_conv_halves[v->branch(i, j)] = conv_b / 2;
            if (C >= 32) {  // the plans' streams are already [row tile][chunk * k + tap]
                bool ok = true;
                for (int q = 0; q < per_rb; ++q) {
                    const parrot_conv* pc = v->rb[base + q].get();
                    ok = ok && pc->prec == v->scheme && !pc->mfma16 && pc->wfrag16 && pc->nchunks == C / 16 && (C / 32) * pc->n_it16 == steps && pc->M == C &&
                         C % tile_cfg(pc->cfg).bm == 0;  // (whole M-blocks: the stream is [32-row tile][chunk * k + tap] over all C / 32 tiles)
                }
                if (!ok) continue;
                // (the kernel's in-place prefetch after the last tap reads "the next conv's" tap 0 of both chunks: one
                //  whole conv of padding keeps that inside the allocation)
                uint16_t* st = nullptr;
                HIP_TRY(hipMalloc((void**)&st, (per_rb + 1) * conv_b));
                v->rb_stream[v->branch(i, j)] = st;
                for (int q = 0; q <= per_rb; ++q)
                    HIP_TRY(hipMemcpy(reinterpret_cast<char*>(st) + q * conv_b, v->rb[base + (q < per_rb ? q : 0)]->wfrag16, conv_b, hipMemcpyDeviceToDevice));
                for (int q = 0; q < per_rb; ++q) v->rb_wsc[base + q] = v->rb[base + q]->wscale;
            } else {
                const size_t step_h = (size_t)NP * 512;
                std::vector<uint16_t> pk(((size_t)per_rb * steps + 2) * step_h, 0);
                for (int q = 0; q < per_rb; ++q) {
                    const GemmWeights W{w->rb_w[base + q], 16, 16, rk, false, 0, 1, 0, 0};  // (16, 16, rk)
                    const float wsc = scheme_is_f16(v->scheme) ? f16_weight_scale(W.w, (size_t)16 * 16 * rk) : 1.f;
                    v->rb_wsc[base + q] = wsc;
                    pack_pieces(pk.data() + (size_t)q * steps * step_h, steps, v->scheme, wsc, W, [](size_t st, int lane, int e) {
                        return WeightAt{lane & 15, 8 * ((lane >> 4) & 1) + e, 2 * (int)st + (lane >> 5)};
                    });
                }
                uint16_t* st = nullptr;
                HIP_TRY(hipMalloc((void**)&st, pk.size() * sizeof(uint16_t)));
                v->rb_stream[v->branch(i, j)] = st;
                HIP_TRY(hipMemcpy(st, pk.data(), pk.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
            }
        }
    // whole-MRF launches for the 32-channel stage (PARROT_MRF_FUSED, default on): all branches of a stage in one kernel, on the pair
    // kernels' own weight streams -- bit-identical to the per-branch launches and no slower (2.27 vs 2.31 ms per step at B = 64; 14 -> 2
    // passes over the stage's activations).  (64 channels were built and measured slower: profiles/r05b_mrf_ab.jsonl.)
    v->mrf_ok.assign((size_t)cfg->n_stages, 0);
    {
        static const bool want = [] { const char* e = getenv("PARROT_MRF_FUSED"); return !e || atoi(e) != 0; }();
        for (int i = 0; i < cfg->n_stages && want && v->fused != 0 && v->scheme >= 1 && resblock_mrf_scheme(v->scheme); ++i) {
            const int C = v->chan(i);
            if (cfg->resblock_type != 1 || !resblock_mrf_has(C) || per_rb > RBS_MAX_CONVS || cfg->n_kernels > RBS_MAX_BRANCH) continue;
            bool ok = true;
            for (int j = 0; j < cfg->n_kernels; ++j) ok = ok && (cfg->resblock_kernel_sizes[j] & 1) && v->branch_stream(i, j);
            v->mrf_ok[i] = ok && rbs_mrf_window(C) - 2 * v->stage_reach(i) >= rbs_mrf_window(C) / 2;
        }
    }
    return PARROT_OK;
}
