// parrot_hip.hip -- the vocoder handle: create, the MRF dispatch (whole-stage / pair / fused / layer-by-layer launches), the direct
// forward, the graph cache of small shapes and the chunk-streamed forward.
#include "host_common.h"

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "conv_split.h"
#include "conv_split16.h"
#include "kernels_voc.h"
#include "resblock_split.h"
#include "resblock_fused.h"
#include "weight_pack.h"

using namespace parrot;

// ---------------------------------------------------------------------------------------------
// vocoder
// ---------------------------------------------------------------------------------------------
struct parrot_voc {
    parrot_voc_cfg cfg{};
    float* dict = nullptr;
    float* spkr = nullptr;
    DevFlag err;
    std::unique_ptr<parrot_conv> conv_pre, conv_post;
    std::vector<std::unique_ptr<parrot_conv>> ups, rb;
    std::vector<uint16_t*> rb_stream;  // per (stage, kernel): concatenated split weight stream of the block (or null)
    std::vector<float> rb_wsc;         // per resblock conv: weight scale inside that stream (fp16 schemes; else 1)
    std::vector<size_t> rb_conv_halves;  // 16-bit words per conv in that stream
    // whole-MRF launches (resblock_split.h, MRF instantiation): mrf_ok[stage] = every branch of the stage has a pair-kernel weight
    // stream (rb_stream) and the window survives the widest branch's reach
    std::vector<char> mrf_ok;
    int up_total = 1;
    bool odd_stage = false;            // some stage has odd kernel_size - rate: T_out = T u + 1 there (no constant hop)
    int scheme = 0;                    // PARROT_PREC_* captured at create (immutable afterwards)
    int fused = 2;                     // fused-ResBlock mode captured at create
    bool planes = true;                // operand planes between the layer-by-layer convs of a pair (PARROT_PLANES, read at create)
    // MRF branch concurrency: the n_kernels ResBlocks of a stage are independent chains until the final sum, so each runs
    // on its own HIP stream (the caller's + side streams owned by the handle), forked / joined with events; the final
    // accumulating launches are ordered with events (sum order j = 0, 1, 2 as models.py:100-106).  One branch's
    // launch tails, prologues and epilogues then overlap another branch's main loops.
    int mrf_streams = 1;
    bool mrf_auto = true;
    std::mutex side_mu;  // the side streams / events are the handle's: concurrent callers enqueue their fork-join sequences one at a time
    struct StreamSet {
        hipStream_t side[PARROT_MAX_KERNELS] = {};
        hipEvent_t ev_fork = nullptr, ev_last[PARROT_MAX_KERNELS] = {};
    } ss;
    // chunk lanes of the chunk-streamed forward (lane 0 is the caller's stream)
    static constexpr int MAX_LANES = 4;
    hipStream_t lane_stream[MAX_LANES] = {};
    hipEvent_t ev_lane_fork = nullptr, ev_lane_join[MAX_LANES] = {};
    // stage events (parrot_voc_wait_stage): recorded on the caller's stream when stage i of a direct forward begins (after its
    // upsampling conv), so that ANOTHER stream can start work beside a chosen part of the forward -- the two-stage pipeline across
    // batches runs the next batch's TTE beside the LDS-resident stage 3 / 4 kernels (one workgroup per CU, barrier waits to fill)
    // instead of beside the chip-filling stage 0 / 1 layer convs
    hipEvent_t ev_stage[PARROT_MAX_STAGES] = {};
    bool capturing = false;            // (a graph capture is in progress on cap_stream: no event records into it)
    float* dbg_absmax = nullptr;       // parrot_voc_debug_absmax: (n_stages + 2) device floats, max |conv input| per group (caller-owned)
    // HIP-graph replay of small forwards (PARROT_VOC_GRAPH, default on; B x U <= 8192 units): a forward is ~130 dependent launches
    // of 7-40 us on up to three streams -- at one utterance the fork / join events and the launch gaps are a fifth of it.  A SHAPE
    // (B, U, with / without speaker ids and row lengths) that keeps recurring is captured once (GRAPH_AFTER below; the first calls also warm lazy
    // state), on a stream of the handle and into staging buffers of the handle (ids, lengths, waveform, workspace: one allocation per
    // cached shape, made at capture time -- never per call): PyTorch's allocator hands out different addresses from call to call, and
    // a graph bakes its addresses in.  A replay copies the caller's ids / lengths in (a few KB), launches the graph and copies the
    // waveform out: the same kernels with the same arguments in the same order, the MRF branch streams as graph edges.
    struct Graph {
        int B = 0, U = 0;
        bool has_spkr = false, has_lens = false;
        char* mem = nullptr;  // one allocation: code | spkr | lens | wav | ws
        int64_t *code = nullptr, *spkr = nullptr;
        int32_t* lens = nullptr;
        float* wav = nullptr;
        void* ws = nullptr;
        size_t ws_bytes = 0, wav_bytes = 0, mem_bytes = 0;
        hipGraphExec_t exec = nullptr;
        hipEvent_t done = nullptr;     // recorded behind the last replay's copy-out: a replay on ANOTHER stream waits for it first
        hipStream_t last = nullptr;
        bool launched = false, dead = false;
        int seen = 0;
        unsigned long stamp = 0;
        void release() {
            if (exec) (void)hipGraphExecDestroy(exec);
            if (done) (void)hipEventDestroy(done);
            if (mem) (void)hipFree(mem);
            exec = nullptr; done = nullptr; mem = nullptr;
        }
    };
    // A shape is captured at its GRAPH_AFTER-th sighting (capture + instantiate + the staging allocation cost milliseconds: a
    // driver that feeds ever-changing lengths, one utterance per call, must not pay them -- it never does: its shapes do not recur
    // often enough within the MAX_SHAPES most recent ones); at most MAX_GRAPHS shapes hold a graph, least recently used first out
    static constexpr int MAX_GRAPHS = 8, MAX_SHAPES = 64, GRAPH_AFTER = 4;
    // (staging memory of all cached shapes of a handle together: PARROT_VOC_GRAPH_MB, default 1024 -- see voc_forward_graphed)
    std::vector<Graph> graphs;
    std::mutex graph_mu;
    unsigned long graph_clock = 0;
    hipStream_t cap_stream = nullptr;
    ~parrot_voc() {
        for (Graph& g : graphs) g.release();
        if (cap_stream) (void)hipStreamDestroy(cap_stream);
        for (hipStream_t st : ss.side)
            if (st) (void)hipStreamDestroy(st);
        if (ss.ev_fork) (void)hipEventDestroy(ss.ev_fork);
        for (hipEvent_t e : ss.ev_last)
            if (e) (void)hipEventDestroy(e);
        for (hipStream_t st : lane_stream)
            if (st) (void)hipStreamDestroy(st);
        if (ev_lane_fork) (void)hipEventDestroy(ev_lane_fork);
        for (hipEvent_t e : ev_stage)
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : ev_lane_join)
            if (e) (void)hipEventDestroy(e);
        for (uint16_t* q : rb_stream)
            if (q) (void)hipFree(q);
        if (dict) (void)hipFree(dict);
        if (spkr) (void)hipFree(spkr);
    }
    int chan(int stage) const { return cfg.upsample_initial_channel >> (stage + 1); }
    // rb holds the ResBlock convs of (stage, kernel j) back to back: per_rb() convs from rb_base(stage, j)
    int per_rb() const { return (cfg.resblock_type == 1 ? 2 : 1) * cfg.n_dil; }
    int rb_base(int stage, int j) const { return (stage * cfg.n_kernels + j) * per_rb(); }
    // columns either side of an output column that branch (stage, j) reads: sum over its convs of (k - 1) / 2 * dilation
    int branch_reach(int stage, int j) const {
        int H = 0;
        for (int q = 0; q < per_rb(); ++q) H += (cfg.resblock_kernel_sizes[j] - 1) / 2 * rb[rb_base(stage, j) + q]->dil;
        return H;
    }
    int stage_reach(int stage) const {  // the widest branch of the stage
        int H = 0;
        for (int j = 0; j < cfg.n_kernels; ++j) H = std::max(H, branch_reach(stage, j));
        return H;
    }
    size_t branch(int stage, int j) const { return (size_t)stage * cfg.n_kernels + j; }  // index of rb_stream / rb_conv_halves
    uint16_t* branch_stream(int stage, int j) const { return rb_stream[branch(stage, j)]; }
};

static int voc_create(parrot_voc_t** out, const parrot_voc_cfg* cfg, const parrot_voc_weights* w, int prec, int fused) {
    CreateScope scope(prec, fused, -1);  // (thread-local: the process defaults are not touched)
    if (!out || !cfg || !w) return fail(PARROT_E_INVALID, "voc_create: null argument");
    if (cfg->n_stages <= 0 || cfg->n_stages > PARROT_MAX_STAGES || cfg->n_kernels <= 0 || cfg->n_kernels > PARROT_MAX_KERNELS ||
        cfg->n_dil <= 0 || cfg->n_dil > PARROT_MAX_DIL || (cfg->resblock_type != 1 && cfg->resblock_type != 2))
        return fail(PARROT_E_INVALID, "voc_create: bad config");
    const int in_dim = cfg->embedding_dim * (cfg->multispkr ? 2 : 1);
    // model_in_dim - in_dim input channels come from the caller's extra conditioning streams (parrot_voc_forward_feats)
    if (cfg->model_in_dim < in_dim) return fail(PARROT_E_INVALID, "voc_create: model_in_dim smaller than embedding_dim * (1 + multispkr)");
    if ((cfg->upsample_initial_channel >> cfg->n_stages) < 1) return fail(PARROT_E_INVALID, "voc_create: too many stages for upsample_initial_channel");
    std::unique_ptr<parrot_voc> v(new parrot_voc());
    v->cfg = *cfg;
    const int per_rb = v->per_rb();
    if (w->n_rb != cfg->n_stages * cfg->n_kernels * per_rb) return fail(PARROT_E_INVALID, "voc_create: wrong number of resblock convs");
    query_device();
    v->scheme = create_prec();
    v->fused = create_fused();
    for (int i = 0; i < cfg->n_stages; ++i) HIP_TRY(hipEventCreateWithFlags(&v->ev_stage[i], hipEventDisableTiming));
    {   // operand planes: default ON for the single-piece schemes (bf16 / f16: -0.4 ms of 11.1 per step, the configs[2] data path),
        // OFF for fp16x3 (bit-identical, but +-0: co-resident workgroups already hide the conversion, profiles/r06h_planes_ab.txt);
        // PARROT_PLANES=0 / 1 forces either
        const char* e = getenv("PARROT_PLANES");
        v->planes = e ? atoi(e) != 0 : (v->scheme == PARROT_PREC_BF16 || v->scheme == PARROT_PREC_F16);
    }
    {
        const char* e = getenv("PARROT_MRF_STREAMS");
        // default "auto": concurrent branches for small batches (B = 1 ... 16: -6 ... -11 % per batch: their launches do not
        // fill the chip), one stream at B x U > 8192 units (measured +-0 at B = 64: power-limited, not tail-limited -- and
        // per-kernel timings stay clean there).  PARROT_MRF_STREAMS=1 / 3 forces either.
        const bool on = e ? atoi(e) > 1 : true;
        v->mrf_auto = (e == nullptr);
        v->mrf_streams = (on && cfg->n_kernels > 1) ? cfg->n_kernels : 1;
        if (v->mrf_streams > 1) {
            for (int j = 1; j < v->mrf_streams; ++j) HIP_TRY(hipStreamCreateWithFlags(&v->ss.side[j], hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&v->ss.ev_fork, hipEventDisableTiming));
            for (int j = 0; j < v->mrf_streams; ++j) HIP_TRY(hipEventCreateWithFlags(&v->ss.ev_last[j], hipEventDisableTiming));
        }
        for (int l = 1; l < parrot_voc::MAX_LANES; ++l) {
            HIP_TRY(hipStreamCreateWithFlags(&v->lane_stream[l], hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&v->ev_lane_join[l], hipEventDisableTiming));
        }
        HIP_TRY(hipEventCreateWithFlags(&v->ev_lane_fork, hipEventDisableTiming));
    }
    // ConvTranspose1d(k, stride u, padding (k - u) // 2) (models.py:80-83) yields T u samples for even k - u (every shipped
    // config) and T u + 1 for odd k - u: lengths are taken from the convs' own out_len chain (voc_out_len), ragged rows carry
    // the extra samples as `row_len_add`.  k < u would mean a negative padding, which torch rejects too.
    for (int i = 0; i < cfg->n_stages; ++i) {
        const int u = cfg->upsample_rates[i], k = cfg->upsample_kernel_sizes[i];
        if (u <= 0 || k < u) return fail(PARROT_E_UNSUPPORTED, "voc_create: upsample_kernel_size must be >= upsample_rate (negative padding)");
        if ((k - u) & 1) v->odd_stage = true;
    }
    TRY(upload(&v->dict, w->dict, (size_t)cfg->num_embeddings * cfg->embedding_dim));
    if (cfg->multispkr) {
        if (!w->spkr) return fail(PARROT_E_INVALID, "voc_create: multispkr without spkr table");
        TRY(upload(&v->spkr, w->spkr, (size_t)cfg->n_spkr * cfg->embedding_dim));
    }
    TRY(v->err.init());
    const int C0 = cfg->upsample_initial_channel;
    TRY(make_conv(v->conv_pre, cfg->model_in_dim, C0, 7, 1, 3, 0, 1, PRE_NONE, 0.f, ACT_NONE, w->conv_pre_w, w->conv_pre_b));
    v->ups.resize(cfg->n_stages);
    v->rb.resize(w->n_rb);
    for (int i = 0; i < cfg->n_stages; ++i) {
        const int cin = C0 >> i, cout = C0 >> (i + 1), u = cfg->upsample_rates[i], k = cfg->upsample_kernel_sizes[i];
        v->up_total *= u;
        TRY(make_conv(v->ups[i], cin, cout, k, 1, (k - u) / 2, 1, u, PRE_LRELU, 0.1f, ACT_NONE, w->ups_w[i], w->ups_b[i]));
        for (int j = 0; j < cfg->n_kernels; ++j) {
            const int rk = cfg->resblock_kernel_sizes[j];
            // (blocks that run on the fused pair kernels reuse their plans' 32x32x16 weight streams: keep that packing)
            const bool a16 = !(v->fused != 0 && cfg->resblock_type == 1 && resblock_split_has(cout, rk) && per_rb <= RBS_MAX_CONVS);
            for (int m = 0; m < cfg->n_dil; ++m) {
                const int dl = cfg->resblock_dilation_sizes[j][m];
                const int base = v->rb_base(i, j);
                if (cfg->resblock_type == 1) {
                    TRY(make_conv(v->rb[base + 2 * m], cout, cout, rk, dl, (rk * dl - dl) / 2, 0, 1, PRE_LRELU, 0.1f, ACT_NONE,
                                  w->rb_w[base + 2 * m], w->rb_b[base + 2 * m], 1, a16));
                    TRY(make_conv(v->rb[base + 2 * m + 1], cout, cout, rk, 1, (rk - 1) / 2, 0, 1, PRE_LRELU, 0.1f, ACT_NONE,
                                  w->rb_w[base + 2 * m + 1], w->rb_b[base + 2 * m + 1], 1, a16));
                } else {
                    TRY(make_conv(v->rb[base + m], cout, cout, rk, dl, (rk * dl - dl) / 2, 0, 1, PRE_LRELU, 0.1f, ACT_NONE,
                                  w->rb_w[base + m], w->rb_b[base + m], 1, a16));
                }
            }
        }
    }
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
            if (cfg->resblock_type != 1 || !resblock_split_has(C, rk) || per_rb > RBS_MAX_CONVS) continue;
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
    // final F.leaky_relu(x) uses the DEFAULT slope 0.01 (models.py:107, quirk Q5)
    TRY(make_conv(v->conv_post, C0 >> cfg->n_stages, 1, 7, 1, 3, 0, 1, PRE_LRELU, 0.01f, ACT_TANH, w->conv_post_w, w->conv_post_b));
    v->conv_post->err_flag = v->err;  // a non-finite waveform sample (an activation left the fp16 split range) raises the handle's flag
    *out = v.release();
    return PARROT_OK;
}
extern "C" int parrot_voc_create(parrot_voc_t** out, const parrot_voc_cfg* cfg, const parrot_voc_weights* w) { return voc_create(out, cfg, w, -1, -1); }
extern "C" int parrot_voc_create_ex(parrot_voc_t** out, const parrot_voc_cfg* cfg, const parrot_voc_weights* w, int32_t precision,
                                    int32_t fused_resblocks) {
    if (precision > PARROT_PREC_F16 || fused_resblocks > 2) return fail(PARROT_E_INVALID, "voc_create_ex: precision in -1 .. 4, fused_resblocks in -1 .. 2");
    return voc_create(out, cfg, w, precision, fused_resblocks);
}
extern "C" void parrot_voc_destroy(parrot_voc_t* v) { delete v; }
extern "C" int parrot_voc_precision(const parrot_voc_t* v) { return v ? v->scheme : PARROT_E_INVALID; }
// Debug aid (range headroom of the fp16 split scheme, |x| < 8190): while dst_dev != NULL every conv launched by
// parrot_voc_forward records max |input element| into dst_dev[group] (atomic max; group 0 = conv_pre, 1 + i = the layers of
// stage i (ups_i and its ResBlocks), n_stages + 1 = conv_post).  Fused ResBlock launches only see their block's input: create the
// handle with fused_resblocks = 0 (parrot_voc_create_ex) to cover every layer.  The caller zeroes the n_stages + 2 floats.
extern "C" int parrot_voc_debug_absmax(parrot_voc_t* v, float* dst_dev) {
    if (!v) return fail(PARROT_E_INVALID, "voc_debug_absmax: null handle");
    v->dbg_absmax = dst_dev;
    return PARROT_OK;
}

static size_t voc_max_act(const parrot_voc* v, int B, int U) {
    size_t mx = (size_t)B * v->cfg.upsample_initial_channel * U;
    int T = U;
    for (int i = 0; i < v->cfg.n_stages; ++i) {
        T = v->ups[i]->out_len(T);
        mx = std::max(mx, (size_t)B * v->chan(i) * (size_t)T);
    }
    return mx;
}
// waveform samples of an utterance of U units: the transposed convs' out_len chain (U * hop unless a stage has odd k - u)
static long voc_out_len(const parrot_voc* v, int U) {
    long T = U;
    for (int i = 0; i < v->cfg.n_stages; ++i) T = v->ups[i]->out_len((int)T);
    return T;
}
extern "C" int64_t parrot_voc_out_len(const parrot_voc_t* v, int32_t U) { return (v && U > 0) ? voc_out_len(v, U) : 0; }

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
// One ResBlock branch of an MRF stage: y (epi: =, +=, or += then / div) ResBlock_j(x) on stream s.  mid / res_a / res_b: the branch's
// scratch tensors (between the convs of a pair; the running residual, alternating); before_last: the event the launch that accumulates into y waits for (the MRF sum runs in branch order).
struct Branch {
    const float* x;
    float* y;
    float *mid, *res_a, *res_b;
    int B, T, epi;
    float div;
    hipStream_t s;
    RowLens rows;
    hipEvent_t before_last;
};
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

// MRF branches that run concurrently for this shape: the handle's stream count, or one above B x U = 8192 units in auto mode
// (one rule for the workspace size and for the forward pass)
static int voc_streams(const parrot_voc* v, int B, int U) { return (v->mrf_auto && (long)B * U > 8192) ? 1 : v->mrf_streams; }

static size_t voc_ws_bytes(const parrot_voc* v, int B, int U, int ns) {
    Arena a(nullptr, 0);
    a.take<float>((size_t)B * v->cfg.model_in_dim * U);
    const size_t mx = voc_max_act(v, B, U);
    for (int i = 0; i < 3 + 3 * ns; ++i) a.take<float>(mx);  // stage in / ups out / MRF sum + (T1, RA, RB) per concurrent branch
    return align_up(a.off, 256);
}
extern "C" size_t parrot_voc_workspace_bytes(const parrot_voc_t* v, int32_t B, int32_t U) {
    if (!v || B <= 0 || U <= 0) return 0;
    return voc_ws_bytes(v, B, U, voc_streams(v, B, U));
}

// Receptive field of the generator in units, either side of an output frame: the interval [tau, tau] of one waveform sample is
// propagated back through conv_post, every MRF stage (the widest ResBlock), every ConvTranspose1d (tau = t u - p + kappa) and
// conv_pre, for every phase tau mod hop; a chunk computed with this much real context equals the whole-utterance forward.
static int voc_receptive_units(const parrot_voc* v) {
    const parrot_voc_cfg& c = v->cfg;
    const long hop = v->up_total, base = 4096;  // far from the origin: integer divisions below see positive numbers only
    long worst = 0;
    for (long ph = 0; ph < hop; ++ph) {
        long lo = base * hop + ph, hi = lo;
        lo -= 3; hi += 3;  // conv_post (k = 7)
        for (int i = c.n_stages - 1; i >= 0; --i) {
            const long reach = v->stage_reach(i);  // the widest ResBlock of the stage
            lo -= reach; hi += reach;
            const long u = c.upsample_rates[i], k = c.upsample_kernel_sizes[i], p = (k - u) / 2;
            // output tau depends on inputs t with tau = t u - p + kappa, kappa in [0, k): t in [ceil((tau + p - k + 1) / u), floor((tau + p) / u)]
            lo = (lo + p - k + 1 + u - 1) / u;
            hi = (hi + p) / u;
        }
        lo -= 3; hi += 3;  // conv_pre (k = 7)
        worst = std::max(worst, std::max(base - lo, hi - base));
    }
    return (int)worst;
}
extern "C" int parrot_voc_receptive_units(const parrot_voc_t* v) { return v ? voc_receptive_units(v) : PARROT_E_INVALID; }

// (declared ahead of its body: the graph cache and the chunked forward below call it, and the MRF dispatch it rests on follows them)
static int voc_forward_impl(parrot_voc_t* v, const int64_t* code, int code_stride, const int64_t* spkr, const float* feats,
                            int32_t n_feat_channels, const int32_t* unit_lens, int32_t B, int32_t U, float* wav_out,
                            float* const* stage_out, void* ws, size_t ws_bytes, void* stream, int ns_sized = 0);

// Small forwards through the graph cache (see parrot_voc::Graph); everything else -- and every failure of the graph path -- direct.
static int voc_forward_graphed(parrot_voc_t* v, const int64_t* code, int code_stride, const int64_t* spkr, const float* feats,
                               int32_t n_feat, const int32_t* unit_lens, int32_t B, int32_t U, float* wav_out, float* const* stage_out,
                               void* ws, size_t ws_bytes, void* stream) {
    static const bool want = [] { const char* e = getenv("PARROT_VOC_GRAPH"); return !e || atoi(e) != 0; }();
    hipStream_t s = (hipStream_t)stream;
    auto direct = [&]() {
        if (poison_word() && v && B > 0 && U > 0) {
            TRY(poison(ws, ws_bytes, s));
            if (wav_out) TRY(poison(wav_out, (size_t)B * (size_t)voc_out_len(v, U) * sizeof(float), s));
        }
        return voc_forward_impl(v, code, code_stride, spkr, feats, n_feat, unit_lens, B, U, wav_out, stage_out, ws, ws_bytes, stream);
    };
    const bool small = v && B > 0 && U > 0 && (long)B * U <= 8192;
    if (!want || !small || stage_out || v->dbg_absmax || prof_on() || !code || !wav_out || !ws || n_feat != 0 || feats ||
        (v->cfg.multispkr && !spkr) || v->cfg.model_in_dim != v->cfg.embedding_dim * (v->cfg.multispkr ? 2 : 1))
        return direct();  // (argument errors are reported by the direct path)
    {
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &st) != hipSuccess || st != hipStreamCaptureStatusNone) return direct();  // the caller is capturing: stay inside ITS graph
    }
    // the caller's workspace must be what a direct run needs (a replay does not touch it, but the contract is the same call)
    if (ws_bytes < voc_ws_bytes(v, B, U, voc_streams(v, B, U))) return direct();
    const bool has_spkr = v->cfg.multispkr && spkr != nullptr, has_lens = unit_lens != nullptr;
    std::unique_lock<std::mutex> lk(v->graph_mu);
    parrot_voc::Graph* g = nullptr;
    for (parrot_voc::Graph& q : v->graphs)
        if (q.B == B && q.U == U && q.has_spkr == has_spkr && q.has_lens == has_lens) {
            g = &q;
            break;
        }
    auto drop = [&](size_t i) {  // (a graph may still be running: its buffers are freed only after the device has drained what uses them)
        if (v->graphs[i].launched && v->graphs[i].done) (void)hipEventSynchronize(v->graphs[i].done);
        v->graphs[i].release();
    };
    if (!g) {  // first sighting: count the shape (the least recently seen shape makes room), run directly
        if ((int)v->graphs.size() >= parrot_voc::MAX_SHAPES) {
            size_t old = 0;
            for (size_t i = 1; i < v->graphs.size(); ++i)
                if (v->graphs[i].stamp < v->graphs[old].stamp) old = i;
            drop(old);
            v->graphs.erase(v->graphs.begin() + old);
        }
        parrot_voc::Graph q{};
        q.B = B; q.U = U; q.has_spkr = has_spkr; q.has_lens = has_lens;
        q.seen = 1;
        q.stamp = ++v->graph_clock;
        v->graphs.push_back(q);
        lk.unlock();
        return direct();
    }
    g->stamp = ++v->graph_clock;
    if (g->dead || (!g->exec && ++g->seen < parrot_voc::GRAPH_AFTER)) {
        lk.unlock();
        return direct();
    }
    if (!g->exec) {  // this shape keeps coming: staging buffers + capture on the handle's own stream (nothing runs during the capture)
        const size_t n_code = (size_t)B * U * sizeof(int64_t), n_spkr = has_spkr ? (size_t)B * sizeof(int64_t) : 0,
                     n_lens = has_lens ? (size_t)B * sizeof(int32_t) : 0;
        g->wav_bytes = (size_t)B * (size_t)voc_out_len(v, U) * sizeof(float);
        g->ws_bytes = voc_ws_bytes(v, B, U, voc_streams(v, B, U));
        size_t off = 0;
        auto take = [&](size_t n) { const size_t o = off; off = align_up(off + n, 256); return o; };
        const size_t o_code = take(n_code), o_spkr = take(n_spkr), o_lens = take(n_lens), o_wav = take(g->wav_bytes), o_ws = take(g->ws_bytes);
        // it takes a graph slot and `off` bytes of staging memory: least recently used graphs give theirs up until both fit
        // (PARROT_VOC_GRAPH_MB caps the staging memory of one handle, default 1024 -- it is hipMalloc'ed, outside torch's allocator)
        static const size_t cap = [] { const char* e = getenv("PARROT_VOC_GRAPH_MB"); return (size_t)(e ? std::max(0, atoi(e)) : 1024) << 20; }();
        for (;;) {
            int n_graphs = 0;
            size_t in_use = 0, lru = v->graphs.size();
            for (size_t i = 0; i < v->graphs.size(); ++i) {
                in_use += v->graphs[i].mem_bytes;
                if (v->graphs[i].exec) {
                    ++n_graphs;
                    if (lru == v->graphs.size() || v->graphs[i].stamp < v->graphs[lru].stamp) lru = i;
                }
            }
            if ((n_graphs < parrot_voc::MAX_GRAPHS && in_use + off <= cap) || lru == v->graphs.size()) break;
            drop(lru);
            v->graphs[lru].mem_bytes = 0;
            v->graphs[lru].seen = 0;
            v->graphs[lru].launched = false;
        }
        size_t in_use = 0;
        for (const parrot_voc::Graph& q : v->graphs) in_use += q.mem_bytes;
        if (in_use + off > cap) {  // larger than the whole cap: direct, and not asked again for a while
            g->seen = -1000;
            lk.unlock();
            return direct();
        }
        bool ok = hipMalloc((void**)&g->mem, off) == hipSuccess;
        if (ok) {
            g->mem_bytes = off;
            g->code = reinterpret_cast<int64_t*>(g->mem + o_code);
            g->spkr = has_spkr ? reinterpret_cast<int64_t*>(g->mem + o_spkr) : nullptr;
            g->lens = has_lens ? reinterpret_cast<int32_t*>(g->mem + o_lens) : nullptr;
            g->wav = reinterpret_cast<float*>(g->mem + o_wav);
            g->ws = g->mem + o_ws;
            ok = hipEventCreateWithFlags(&g->done, hipEventDisableTiming) == hipSuccess;
        }
        if (ok && !v->cap_stream) ok = hipStreamCreateWithFlags(&v->cap_stream, hipStreamNonBlocking) == hipSuccess;
        hipGraph_t graph = nullptr;
        if (ok) ok = hipStreamBeginCapture(v->cap_stream, hipStreamCaptureModeRelaxed) == hipSuccess;
        if (ok) {
            v->capturing = true;
            const int rc = voc_forward_impl(v, g->code, U, g->spkr, nullptr, 0, g->lens, B, U, g->wav, nullptr, g->ws, g->ws_bytes, (void*)v->cap_stream);
            v->capturing = false;
            const hipError_t e_end = hipStreamEndCapture(v->cap_stream, &graph);
            ok = rc == PARROT_OK && e_end == hipSuccess && graph && hipGraphInstantiate(&g->exec, graph, nullptr, nullptr, 0) == hipSuccess;
        }
        if (graph) (void)hipGraphDestroy(graph);
        if (!ok) {  // this shape goes direct from now on
            (void)hipGetLastError();
            g->release();
            g->mem_bytes = 0;
            g->dead = true;
            lk.unlock();
            return direct();
        }
    }
    if (g->launched && g->last != s) HIP_TRY(hipStreamWaitEvent(s, g->done, 0));  // the staging buffers are still the previous replay's
    HIP_TRY(hipMemcpy2DAsync(g->code, (size_t)U * sizeof(int64_t), code, (size_t)code_stride * sizeof(int64_t), (size_t)U * sizeof(int64_t), B,
                             hipMemcpyDeviceToDevice, s));
    if (g->spkr) HIP_TRY(hipMemcpyAsync(g->spkr, spkr, (size_t)B * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    if (g->lens) HIP_TRY(hipMemcpyAsync(g->lens, unit_lens, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (poison_word()) {
        TRY(poison(g->ws, g->ws_bytes, s));
        TRY(poison(g->wav, g->wav_bytes, s));
        TRY(poison(wav_out, g->wav_bytes, s));
        TRY(poison(ws, ws_bytes, s));
    }
    HIP_TRY(hipGraphLaunch(g->exec, s));
    HIP_TRY(hipMemcpyAsync(wav_out, g->wav, g->wav_bytes, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipEventRecord(g->done, s));
    g->last = s;
    g->launched = true;
    return PARROT_OK;
}

// Make `stream` wait until the most recently ENQUEUED direct forward of this handle has reached stage `stage` (its upsampling conv
// is done, its MRF begins; the events are created with the handle and recorded by every direct forward).  Before the first forward,
// and for graph replays (small shapes), there is nothing to wait for -- a caller that overlaps work with the forward loses the
// delay, never correctness.
extern "C" int parrot_voc_wait_stage(parrot_voc_t* v, int32_t stage, void* stream) {
    if (!v || stage < 0 || stage >= v->cfg.n_stages) return fail(PARROT_E_INVALID, "voc_wait_stage: stage out of range");
    if (!v->ev_stage[stage]) return PARROT_OK;
    HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, v->ev_stage[stage], 0));  // (never recorded yet: no wait)
    return PARROT_OK;
}

extern "C" int parrot_voc_forward(parrot_voc_t* v, const int64_t* code, const int64_t* spkr, const int32_t* unit_lens, int32_t B,
                                  int32_t U, float* wav_out, float* const* stage_out, void* ws, size_t ws_bytes, void* stream) {
    return voc_forward_graphed(v, code, U, spkr, nullptr, 0, unit_lens, B, U, wav_out, stage_out, ws, ws_bytes, stream);
}

extern "C" int parrot_voc_forward_feats(parrot_voc_t* v, const int64_t* code, const int64_t* spkr, const float* feats,
                                        int32_t n_feat_channels, const int32_t* unit_lens, int32_t B, int32_t U, float* wav_out,
                                        float* const* stage_out, void* ws, size_t ws_bytes, void* stream) {
    return voc_forward_graphed(v, code, U, spkr, feats, n_feat_channels, unit_lens, B, U, wav_out, stage_out, ws, ws_bytes, stream);
}

// Chunk-streamed synthesis inside the library (`chunk_units`; BASELINE configs[4]): consecutive chunks of
// `chunk_units` units are vocoded with `halo_units` (< 0: the generator's receptive field, computed from the config: 21 units
// for the shipped one) of real context on both sides and only their own samples are copied into wav_out -- equal to the
// whole-utterance forward, with the activation memory of chunk_units + 2 halo_units units.  Chunks that touch a true sequence
// edge contain the edge.
// Chunk lanes: consecutive chunks are independent (each is vocoded with its own halo), so several are kept in flight -- chunk c on
// lane c % n, each lane with its own stream, scratch and workspace, and WITHOUT the MRF branch streams: one 256-unit chunk of a
// B = 8 batch is a ninth of the BASELINE batch, its launches leave CUs idle that the other lanes' launches fill, and whole chunks
// overlap better than the three branches of one (B = 8 x 1500 units in 256-unit chunks: 15.9 ms one chunk at a time with branch
// streams, 15.5 with two lanes of three branch streams, 13.4 with two plain lanes; whole utterance 12.0).  PARROT_CHUNK_LANES=1..4.
static int chunk_lanes() {
    static const int n = [] { const char* e = getenv("PARROT_CHUNK_LANES"); const int q = e ? atoi(e) : 2; return std::min(std::max(q, 1), (int)parrot_voc::MAX_LANES); }();
    return n;
}
extern "C" size_t parrot_voc_chunked_workspace_bytes(const parrot_voc_t* v, int32_t B, int32_t chunk_units, int32_t halo_units) {
    if (!v || B <= 0 || chunk_units <= 0) return 0;
    const int halo = halo_units < 0 ? voc_receptive_units(v) : halo_units;
    const int span = chunk_units + 2 * halo;
    Arena a(nullptr, 0);
    for (int lane = 0; lane < chunk_lanes(); ++lane) {
        a.take<float>((size_t)B * span * v->up_total);
        a.take<int32_t>((size_t)B);
        a.off = align_up(a.off, 256) + voc_ws_bytes(v, B, span, 1);
    }
    // a call that ends up on ONE lane (a single chunk, PARROT_CHUNK_LANES=1) runs its chunks with the shape's MRF branch streams
    Arena one(nullptr, 0);
    one.take<float>((size_t)B * span * v->up_total);
    one.take<int32_t>((size_t)B);
    one.off = align_up(one.off, 256) + voc_ws_bytes(v, B, span, voc_streams(v, B, span));
    return align_up(std::max(a.off, one.off), 256);
}
extern "C" int parrot_voc_forward_chunked(parrot_voc_t* v, const int64_t* code, const int64_t* spkr, const int32_t* unit_lens, int32_t B,
                                          int32_t U, int32_t chunk_units, int32_t halo_units, float* wav_out, void* ws, size_t ws_bytes,
                                          void* stream) {
    if (!v || !code || !wav_out || !ws) return fail(PARROT_E_INVALID, "voc_forward_chunked: null argument");
    if (B <= 0 || U <= 0 || chunk_units <= 0) return fail(PARROT_E_INVALID, "voc_forward_chunked: empty batch or chunk");
    if (v->cfg.model_in_dim != v->cfg.embedding_dim * (v->cfg.multispkr ? 2 : 1))
        return fail(PARROT_E_UNSUPPORTED, "voc_forward_chunked: models with extra conditioning streams go through parrot_voc_forward_feats");
    if (v->odd_stage)
        return fail(PARROT_E_UNSUPPORTED, "voc_forward_chunked: a stage with odd upsample_kernel_size - upsample_rate has no constant samples-per-unit hop to cut chunks on");
    const int halo = halo_units < 0 ? voc_receptive_units(v) : halo_units;
    const int span = chunk_units + 2 * halo, hop = v->up_total;
    hipStream_t s = (hipStream_t)stream;
    const int n_chunks = (U + chunk_units - 1) / chunk_units;
    const int n_lanes = std::min(chunk_lanes(), n_chunks);
    if (poison_word()) {
        TRY(poison(ws, ws_bytes, s));
        TRY(poison(wav_out, (size_t)B * U * hop * sizeof(float), s));
    }
    // lanes run WITHOUT the MRF branch streams (whole chunks overlap better than the branches of one); a call on one lane only -- a
    // single chunk, PARROT_CHUNK_LANES=1 -- keeps the branch streams of its shape, like parrot_voc_forward on that span
    const int ns_chunk = n_lanes > 1 ? 1 : voc_streams(v, B, span);
    Arena a(ws, ws_bytes);
    const size_t inner = voc_ws_bytes(v, B, span, ns_chunk);
    float* tmp[parrot_voc::MAX_LANES] = {};
    int32_t* lens[parrot_voc::MAX_LANES] = {};
    void* inner_ws[parrot_voc::MAX_LANES] = {};
    for (int lane = 0; lane < n_lanes; ++lane) {
        tmp[lane] = a.take<float>((size_t)B * span * hop);
        lens[lane] = a.take<int32_t>((size_t)B);
        a.off = align_up(a.off, 256);
        inner_ws[lane] = (char*)ws + a.off;
        a.off += inner;
    }
    if (!a.ok || a.off > ws_bytes) return fail(PARROT_E_NOMEM, "voc_forward_chunked: workspace too small");
    std::unique_lock<std::mutex> side_lock(v->side_mu, std::defer_lock);  // the lane streams and events are the handle's
    if (n_lanes > 1) side_lock.lock();                                     // (one lane: voc_forward_impl takes it for its branch streams)
    // Whatever happens below, the caller's stream must not run past work that the lanes still have queued on ws / wav_out (the
    // caller may free them right after an error return): the join runs on every exit once the lanes have been forked.
    struct LaneJoin {
        parrot_voc* v; hipStream_t s; int n; bool armed;
        ~LaneJoin() {
            if (!armed) return;
            for (int l = 1; l < n; ++l)
                if (hipEventRecord(v->ev_lane_join[l], v->lane_stream[l]) == hipSuccess) (void)hipStreamWaitEvent(s, v->ev_lane_join[l], 0);
        }
    } join{v, s, n_lanes, false};
    if (n_lanes > 1) {  // the other lanes see what the caller's stream has produced so far (code, spkr, unit_lens)
        HIP_TRY(hipEventRecord(v->ev_lane_fork, s));
        join.armed = true;
        for (int l = 1; l < n_lanes; ++l) HIP_TRY(hipStreamWaitEvent(v->lane_stream[l], v->ev_lane_fork, 0));
    }
    int c = 0;
    for (int start = 0; start < U; start += chunk_units, ++c) {
        const int lane = c % n_lanes;
        hipStream_t sl = lane ? v->lane_stream[lane] : s;
        const int stop = std::min(U, start + chunk_units);
        const int lo = std::max(0, start - halo), hi = std::min(U, stop + halo), n = hi - lo;
        if (unit_lens) {
            hipLaunchKernelGGL(rebase_lens_kernel, dim3((B + 255) / 256), dim3(256), 0, sl, unit_lens, lens[lane], B, lo, n);
            HIP_TRY(hipGetLastError());
        }
        // (the branch-stream count the lane's workspace was sized for)
        TRY(voc_forward_impl(v, code + lo, U, spkr, nullptr, 0, unit_lens ? lens[lane] : nullptr, B, n, tmp[lane], nullptr, inner_ws[lane], inner,
                             (void*)sl, ns_chunk));
        HIP_TRY(hipMemcpy2DAsync(wav_out + (size_t)start * hop, (size_t)U * hop * sizeof(float), tmp[lane] + (size_t)(start - lo) * hop,
                                 (size_t)n * hop * sizeof(float), (size_t)(stop - start) * hop * sizeof(float), B, hipMemcpyDeviceToDevice, sl));
    }
    // (join: LaneJoin's destructor -- the caller's stream continues when every lane has written its chunks)
    return PARROT_OK;
}

// debug: max |conv input| per layer group (parrot_voc_debug_absmax)
static int voc_amax(const parrot_voc* v, int group, const float* src, size_t n, hipStream_t q) {
    if (v->dbg_absmax) {
        hipLaunchKernelGGL(absmax_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 2048)), dim3(256), 0, q, src, n, v->dbg_absmax + group);
        HIP_TRY(hipGetLastError());
    }
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

// ns_sized > 0 (chunked path): the number of concurrent MRF branches the caller sized the workspace with
static int voc_forward_impl(parrot_voc_t* v, const int64_t* code, int code_stride, const int64_t* spkr, const float* feats,
                            int32_t n_feat_channels, const int32_t* unit_lens, int32_t B, int32_t U, float* wav_out,
                            float* const* stage_out, void* ws, size_t ws_bytes, void* stream, int ns_sized) {
    if (!v || !code || !wav_out || !ws) return fail(PARROT_E_INVALID, "voc_forward: null argument");
    {
        const int base = v->cfg.embedding_dim * (v->cfg.multispkr ? 2 : 1);
        if (n_feat_channels != v->cfg.model_in_dim - base || (n_feat_channels > 0 && !feats))
            return fail(PARROT_E_INVALID, "voc_forward: extra feature channels must fill model_in_dim - embedding_dim * (1 + multispkr)");
    }
    if (B <= 0 || U <= 0) return fail(PARROT_E_INVALID, "voc_forward: empty batch");
    if (v->cfg.multispkr && !spkr) return fail(PARROT_E_INVALID, "voc_forward: multispkr model needs spkr ids");
    hipStream_t s = (hipStream_t)stream;
    const parrot_voc_cfg& c = v->cfg;
    Arena a(ws, ws_bytes);
    float* x0 = a.take<float>((size_t)B * c.model_in_dim * U);
    const size_t mx = voc_max_act(v, B, U);
    // concurrent MRF branches: the shape's own rule, or -- chunked path -- the count the caller sized the workspace with
    // (parrot_voc_workspace_bytes reserves exactly these; chunk lanes run without branch streams)
    const int ns = ns_sized > 0 ? std::min(ns_sized, v->mrf_streams) : voc_streams(v, B, U);
    const parrot_voc::StreamSet& ss = v->ss;
    std::unique_lock<std::mutex> side_lock(v->side_mu, std::defer_lock);
    if (ns > 1) side_lock.lock();
    float* P[3];
    for (int i = 0; i < 3; ++i) P[i] = a.take<float>(mx);
    float* TMP[PARROT_MAX_KERNELS][3];  // (T1, RA, RB) per concurrent branch
    for (int j = 0; j < ns; ++j)
        for (int q = 0; q < 3; ++q) TMP[j][q] = a.take<float>(mx);
    if (!a.ok) return fail(PARROT_E_NOMEM, "voc_forward: workspace too small");

    {
        const int base = c.embedding_dim * (c.multispkr ? 2 : 1);
        dim3 grid((U + 63) / 64, (base + 63) / 64, B);
        hipLaunchKernelGGL(voc_embed_kernel, grid, dim3(256), 0, s, code, spkr, v->dict, v->spkr, x0, U, c.embedding_dim,
                           base, c.model_in_dim, c.num_embeddings, c.n_spkr, v->err, code_stride);
        HIP_TRY(hipGetLastError());
        if (n_feat_channels > 0)  // extra conditioning streams (already upsampled to U frames) behind the embeddings
            HIP_TRY(hipMemcpy2DAsync(x0 + (size_t)base * U, (size_t)c.model_in_dim * U * sizeof(float), feats,
                                     (size_t)n_feat_channels * U * sizeof(float), (size_t)n_feat_channels * U * sizeof(float), B,
                                     hipMemcpyDeviceToDevice, s));
    }
    auto snap = [&](int idx, const float* src, size_t n) -> int {
        if (stage_out && stage_out[idx]) HIP_TRY(hipMemcpyAsync(stage_out[idx], src, n * sizeof(float), hipMemcpyDeviceToDevice, s));
        return PARROT_OK;
    };
    int ia = 0;
    // unit_lens (optional): per-row number of real units; every layer then applies ITS zero padding at the row's own
    // end (row_len * samples-per-unit so far), so a padded batch row equals the reference's B=1 run of that utterance
    ConvOpts o;
    o.rows.len = unit_lens;  // a row of n units holds n * mul + add samples at the current layer
    TRY(voc_amax(v, 0, x0, (size_t)B * c.model_in_dim * U, s));
    TRY(conv_launch(v->conv_pre.get(), x0, nullptr, P[ia], B, U, EPI_STORE, 1.f, s, o));
    TRY(snap(0, P[ia], (size_t)B * c.upsample_initial_channel * U));
    int T = U;
    const int nk = c.n_kernels;
    for (int i = 0; i < c.n_stages; ++i) {
        float* A = P[ia];
        float* X = P[(ia + 1) % 3];
        float* XS = P[(ia + 2) % 3];
        TRY(voc_amax(v, 1 + i, A, (size_t)B * (c.upsample_initial_channel >> i) * T, s));
        TRY(conv_launch(v->ups[i].get(), A, nullptr, X, B, T, EPI_STORE, 1.f, s, o));
        T = v->ups[i]->out_len(T);
        o.rows.mul *= c.upsample_rates[i];
        o.rows.add = o.rows.add * c.upsample_rates[i] + ((c.upsample_kernel_sizes[i] - c.upsample_rates[i]) & 1);  // out_len(n mul + add)
        const size_t n_act = (size_t)B * v->chan(i) * T;
        if (v->ev_stage[i] && !v->capturing) HIP_TRY(hipEventRecord(v->ev_stage[i], s));
        TRY(snap(1 + 2 * i, X, n_act));
        if (mrf_whole(v, i, B, T)) {
            TRY(voc_amax(v, 1 + i, X, n_act, s));
            TRY(mrf_split_launch(v, i, X, XS, B, T, s, o.rows));
        } else {
            if (ns > 1) {  // fork: the side streams see the upsampled stage input
                HIP_TRY(hipEventRecord(ss.ev_fork, s));
                for (int j = 1; j < ns; ++j) HIP_TRY(hipStreamWaitEvent(ss.side[j], ss.ev_fork, 0));
            }
            for (int j = 0; j < nk; ++j) {
                // the longest branch (largest kernel size = last) stays on the caller's stream
                const int slot = (ns > 1) ? (j + 1) % nk : 0;
                if (j == 0) TRY(voc_amax(v, 1 + i, X, n_act, s));  // the stage input feeds the first conv of every branch
                Branch br{};
                br.x = X; br.y = XS;
                br.mid = TMP[slot][0]; br.res_a = TMP[slot][1]; br.res_b = TMP[slot][2];
                br.B = B; br.T = T;
                br.epi = (nk == 1 || j == 0) ? EPI_STORE : (j == nk - 1 ? EPI_ADD_DIV : EPI_ADD);
                br.div = (float)nk;
                br.s = (slot == 0) ? s : ss.side[slot];
                br.rows = o.rows;
                br.before_last = (ns > 1 && j > 0) ? ss.ev_last[j - 1] : nullptr;  // XS accumulates in branch order (models.py:100-106)
                TRY(branch_launch(v, i, j, br));
                if (ns > 1) HIP_TRY(hipEventRecord(ss.ev_last[j], br.s));
            }
            if (ns > 1)  // join: every branch (and with it every reader of X and of the branch temporaries) is done
                for (int j = 0; j < nk; ++j) HIP_TRY(hipStreamWaitEvent(s, ss.ev_last[j], 0));
        }
        TRY(snap(2 + 2 * i, XS, n_act));
        ia = (ia + 2) % 3;
    }
    TRY(voc_amax(v, 1 + c.n_stages, P[ia], (size_t)B * v->chan(c.n_stages - 1) * T, s));
    TRY(conv_launch(v->conv_post.get(), P[ia], nullptr, wav_out, B, T, EPI_STORE, 1.f, s, o));
    return PARROT_OK;
}

extern "C" int parrot_wav_to_int16(const float* wav, int16_t* out, size_t n, void* stream) {
    if (!wav || !out) return fail(PARROT_E_INVALID, "wav_to_int16: null argument");
    if (n == 0) return PARROT_OK;
    hipLaunchKernelGGL(wav_to_int16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, wav, out, n);
    HIP_TRY(hipGetLastError());
    return PARROT_OK;
}

extern "C" int parrot_voc_status_async(parrot_voc_t* v, int32_t* dst_dev, void* stream) { return v ? status_async(v->err, dst_dev, (hipStream_t)stream) : PARROT_E_INVALID; }
// ... and without clearing it (the shims' first-forward range probe: a bad-id flag stays for the regular reporting path)
extern "C" int parrot_voc_status_peek_async(parrot_voc_t* v, int32_t* dst_dev, void* stream) { return peek_async(v ? v->err.p : nullptr, dst_dev, (hipStream_t)stream, "voc_status_peek"); }
static int voc_status(int status) { return model_status("vocoder", status); }
extern "C" int parrot_voc_check(parrot_voc_t* v, void* stream) { return v ? check_flag(v->err, (hipStream_t)stream, voc_status) : PARROT_E_INVALID; }
