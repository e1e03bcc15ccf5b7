// host_voc.hip -- the vocoder handle: create and destroy, the queries, the workspace layouts, the direct forward and the
// chunk-streamed forward.  How a stage's MRF is run: host_voc_mrf.hip; the graph cache of small shapes: host_voc_graph.hip (voc.h).
#include "voc.h"

#include <cstring>

#include "kernels_voc.h"

using namespace parrot;

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
            const bool a16 = !(v->fused != 0 && mrf_pair_shape(v.get(), i, j));
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
    TRY(mrf_create(v.get(), w));  // the pair kernels' weight streams, and which stages run as one launch
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
long parrot::voc_out_len(const parrot_voc* v, int U) {
    long T = U;
    for (int i = 0; i < v->cfg.n_stages; ++i) T = v->ups[i]->out_len((int)T);
    return T;
}
extern "C" int64_t parrot_voc_out_len(const parrot_voc_t* v, int32_t U) { return (v && U > 0) ? voc_out_len(v, U) : 0; }

// MRF branches that run concurrently for this shape: the handle's stream count, or one above B x U = 8192 units in auto mode
// (one rule for the workspace size and for the forward pass)
int parrot::voc_streams(const parrot_voc* v, int B, int U) { return (v->mrf_auto && (long)B * U > 8192) ? 1 : v->mrf_streams; }

// the workspace of a forward of (B, U) with ns concurrent MRF branches
static VocScratch voc_scratch(const parrot_voc* v, Arena& a, int B, int U, int ns) {
    VocScratch w{};
    w.x0 = a.take<float>((size_t)B * v->cfg.model_in_dim * U);
    const size_t mx = voc_max_act(v, B, U);
    for (float*& p : w.P) p = a.take<float>(mx);  // stage in / ups out / MRF sum
    for (int j = 0; j < ns; ++j) {                // + (T1, RA, RB) per concurrent branch
        w.tmp[j].mid = a.take<float>(mx);
        w.tmp[j].res_a = a.take<float>(mx);
        w.tmp[j].res_b = a.take<float>(mx);
    }
    return w;
}
size_t parrot::voc_ws_bytes(const parrot_voc* v, int B, int U, int ns) {
    Arena a(nullptr, 0);
    (void)voc_scratch(v, a, B, U, ns);
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

// debug: max |conv input| per layer group (parrot_voc_debug_absmax)
int parrot::voc_amax(const parrot_voc* v, int group, const float* src, size_t n, hipStream_t q) {
    if (v->dbg_absmax) {
        hipLaunchKernelGGL(absmax_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 2048)), dim3(256), 0, q, src, n, v->dbg_absmax + group);
        HIP_TRY(hipGetLastError());
    }
    return PARROT_OK;
}

// The forward itself (voc.h: ns_sized, stage_events).
int parrot::voc_forward_impl(parrot_voc* v, const VocCall& call, int ns_sized, bool stage_events) {
    const int64_t *code = call.code, *spkr = call.spkr;
    const int B = call.B, U = call.U, n_feat_channels = call.n_feat;
    float* const* stage_out = call.stage_out;
    if (!v || !code || !call.wav_out || !call.ws) return fail(PARROT_E_INVALID, "voc_forward: null argument");
    {
        const int base = v->cfg.embedding_dim * (v->cfg.multispkr ? 2 : 1);
        if (n_feat_channels != v->cfg.model_in_dim - base || (n_feat_channels > 0 && !call.feats))
            return fail(PARROT_E_INVALID, "voc_forward: extra feature channels must fill model_in_dim - embedding_dim * (1 + multispkr)");
    }
    if (B <= 0 || U <= 0) return fail(PARROT_E_INVALID, "voc_forward: empty batch");
    if (v->cfg.multispkr && !spkr) return fail(PARROT_E_INVALID, "voc_forward: multispkr model needs spkr ids");
    hipStream_t s = call.s;
    const parrot_voc_cfg& c = v->cfg;
    // concurrent MRF branches: the shape's own rule, or -- chunked path -- the count the caller sized the workspace with
    // (parrot_voc_workspace_bytes reserves exactly these; chunk lanes run without branch streams)
    const int ns = ns_sized > 0 ? std::min(ns_sized, v->mrf_streams) : voc_streams(v, B, U);
    std::unique_lock<std::mutex> side_lock(v->side_mu, std::defer_lock);
    if (ns > 1) side_lock.lock();
    Arena a(call.ws, call.ws_bytes);
    const VocScratch w = voc_scratch(v, a, B, U, ns);
    if (!a.ok) return fail(PARROT_E_NOMEM, "voc_forward: workspace too small");

    {
        const int base = c.embedding_dim * (c.multispkr ? 2 : 1);
        dim3 grid((U + 63) / 64, (base + 63) / 64, B);
        hipLaunchKernelGGL(voc_embed_kernel, grid, dim3(256), 0, s, code, spkr, v->dict, v->spkr, w.x0, U, c.embedding_dim,
                           base, c.model_in_dim, c.num_embeddings, c.n_spkr, v->err, call.code_stride);
        HIP_TRY(hipGetLastError());
        if (n_feat_channels > 0)  // extra conditioning streams (already upsampled to U frames) behind the embeddings
            HIP_TRY(hipMemcpy2DAsync(w.x0 + (size_t)base * U, (size_t)c.model_in_dim * U * sizeof(float), call.feats,
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
    o.rows.len = call.unit_lens;  // a row of n units holds n * mul + add samples at the current layer
    TRY(voc_amax(v, 0, w.x0, (size_t)B * c.model_in_dim * U, s));
    TRY(conv_launch(v->conv_pre.get(), w.x0, nullptr, w.P[ia], B, U, EPI_STORE, 1.f, s, o));
    TRY(snap(0, w.P[ia], (size_t)B * c.upsample_initial_channel * U));
    int T = U;
    for (int i = 0; i < c.n_stages; ++i) {
        float* A = w.P[ia];
        float* X = w.P[(ia + 1) % 3];
        float* XS = w.P[(ia + 2) % 3];
        TRY(voc_amax(v, 1 + i, A, (size_t)B * (c.upsample_initial_channel >> i) * T, s));
        TRY(conv_launch(v->ups[i].get(), A, nullptr, X, B, T, EPI_STORE, 1.f, s, o));
        T = v->ups[i]->out_len(T);
        o.rows.mul *= c.upsample_rates[i];
        o.rows.add = o.rows.add * c.upsample_rates[i] + ((c.upsample_kernel_sizes[i] - c.upsample_rates[i]) & 1);  // out_len(n mul + add)
        const size_t n_act = (size_t)B * v->chan(i) * T;
        if (v->ev_stage[i] && stage_events) HIP_TRY(hipEventRecord(v->ev_stage[i], s));
        TRY(snap(1 + 2 * i, X, n_act));
        TRY(mrf_stage(v, i, X, XS, w, B, T, s, ns, o.rows));
        TRY(snap(2 + 2 * i, XS, n_act));
        ia = (ia + 2) % 3;
    }
    TRY(voc_amax(v, 1 + c.n_stages, w.P[ia], (size_t)B * v->chan(c.n_stages - 1) * T, s));
    TRY(conv_launch(v->conv_post.get(), w.P[ia], nullptr, call.wav_out, B, T, EPI_STORE, 1.f, s, o));
    return PARROT_OK;
}
// ... with the caller's buffers poisoned first in poison mode: what parrot_voc_forward runs where the graph cache does not
int parrot::voc_forward_direct(parrot_voc* v, const VocCall& c) {
    if (poison_word() && v && c.B > 0 && c.U > 0) {
        TRY(poison(c.ws, c.ws_bytes, c.s));
        if (c.wav_out) TRY(poison(c.wav_out, (size_t)c.B * (size_t)voc_out_len(v, c.U) * sizeof(float), c.s));
    }
    return voc_forward_impl(v, c, 0, true);
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
    return voc_forward_graphed(v, VocCall{code, U, spkr, nullptr, 0, unit_lens, B, U, wav_out, stage_out, ws, ws_bytes, (hipStream_t)stream});
}

extern "C" int parrot_voc_forward_feats(parrot_voc_t* v, const int64_t* code, const int64_t* spkr, const float* feats,
                                        int32_t n_feat_channels, const int32_t* unit_lens, int32_t B, int32_t U, float* wav_out,
                                        float* const* stage_out, void* ws, size_t ws_bytes, void* stream) {
    return voc_forward_graphed(v, VocCall{code, U, spkr, feats, n_feat_channels, unit_lens, B, U, wav_out, stage_out, ws, ws_bytes, (hipStream_t)stream});
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
// n_lanes lanes, each: the chunk's waveform, its rebased row lengths and the workspace of a forward of `span` units with ns branch streams
struct ChunkScratch {
    float* tmp[parrot_voc::MAX_LANES];
    int32_t* lens[parrot_voc::MAX_LANES];
    void* ws[parrot_voc::MAX_LANES];
    size_t inner;  // bytes of each ws
};
static ChunkScratch chunk_scratch(const parrot_voc* v, Arena& a, int B, int span, int n_lanes, int ns) {
    ChunkScratch w{};
    w.inner = voc_ws_bytes(v, B, span, ns);
    for (int lane = 0; lane < n_lanes; ++lane) {
        w.tmp[lane] = a.take<float>((size_t)B * span * v->up_total);
        w.lens[lane] = a.take<int32_t>((size_t)B);
        w.ws[lane] = a.take<char>(w.inner);
    }
    return w;
}
extern "C" size_t parrot_voc_chunked_workspace_bytes(const parrot_voc_t* v, int32_t B, int32_t chunk_units, int32_t halo_units) {
    if (!v || B <= 0 || chunk_units <= 0) return 0;
    const int halo = halo_units < 0 ? voc_receptive_units(v) : halo_units;
    const int span = chunk_units + 2 * halo;
    Arena a(nullptr, 0);
    (void)chunk_scratch(v, a, B, span, chunk_lanes(), 1);
    // a call that ends up on ONE lane (a single chunk, PARROT_CHUNK_LANES=1) runs its chunks with the shape's MRF branch streams
    Arena one(nullptr, 0);
    (void)chunk_scratch(v, one, B, span, 1, voc_streams(v, B, span));
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
    const ChunkScratch w = chunk_scratch(v, a, B, span, n_lanes, ns_chunk);
    if (!a.ok) return fail(PARROT_E_NOMEM, "voc_forward_chunked: workspace too small");
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
            hipLaunchKernelGGL(rebase_lens_kernel, dim3((B + 255) / 256), dim3(256), 0, sl, unit_lens, w.lens[lane], B, lo, n);
            HIP_TRY(hipGetLastError());
        }
        // (the branch-stream count the lane's workspace was sized for)
        TRY(voc_forward_impl(v, VocCall{code + lo, U, spkr, nullptr, 0, unit_lens ? w.lens[lane] : nullptr, B, n, w.tmp[lane], nullptr, w.ws[lane], w.inner, sl},
                             ns_chunk, true));
        HIP_TRY(hipMemcpy2DAsync(wav_out + (size_t)start * hop, (size_t)U * hop * sizeof(float), w.tmp[lane] + (size_t)(start - lo) * hop,
                                 (size_t)n * hop * sizeof(float), (size_t)(stop - start) * hop * sizeof(float), B, hipMemcpyDeviceToDevice, sl));
    }
    // (join: LaneJoin's destructor -- the caller's stream continues when every lane has written its chunks)
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
