// host_voc_graph.hip -- the vocoder's graph cache of small shapes (VocGraphs, voc.h): which calls go through it, the bookkeeping
// of shapes, the eviction, the capture and the replay.  Everything else -- and every failure of the graph path -- runs direct.
#include "voc.h"

using namespace parrot;
using Graph = VocGraphs::Graph;

// Which calls the cache takes: small plain forwards of a caller that is not capturing itself.  (Argument errors are reported by
// the direct path.)
static bool graph_eligible(const parrot_voc* v, const VocCall& c) {
    static const bool want = [] { const char* e = getenv("PARROT_VOC_GRAPH"); return !e || atoi(e) != 0; }();
    const bool small = v && c.B > 0 && c.U > 0 && (long)c.B * c.U <= 8192;
    if (!want || !small || c.stage_out || v->dbg_absmax || prof_on() || !c.code || !c.wav_out || !c.ws || c.n_feat != 0 || c.feats ||
        (v->cfg.multispkr && !c.spkr) || v->cfg.model_in_dim != v->cfg.embedding_dim * (v->cfg.multispkr ? 2 : 1))
        return false;
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(c.s, &st) != hipSuccess || st != hipStreamCaptureStatusNone) return false;  // the caller is capturing: stay inside ITS graph
    // the caller's workspace must be what a direct run needs (a replay does not touch it, but the contract is the same call)
    return c.ws_bytes >= voc_ws_bytes(v, c.B, c.U, voc_streams(v, c.B, c.U));
}

static void graph_drop(VocGraphs& gc, size_t i) {  // (a graph may still be running: its buffers are freed only after the device has drained what uses them)
    if (gc.graphs[i].launched && gc.graphs[i].done) (void)hipEventSynchronize(gc.graphs[i].done);
    gc.graphs[i].release();
}

// The entry of this shape, freshly stamped -- or, at its first sighting, null: the shape is counted (the least recently seen shape
// makes room) and the call runs directly.
static Graph* graph_find_or_count(VocGraphs& gc, int B, int U, bool has_spkr, bool has_lens) {
    for (Graph& q : gc.graphs)
        if (q.B == B && q.U == U && q.has_spkr == has_spkr && q.has_lens == has_lens) {
            q.stamp = ++gc.clock;
            return &q;
        }
    if ((int)gc.graphs.size() >= VocGraphs::MAX_SHAPES) {
        size_t old = 0;
        for (size_t i = 1; i < gc.graphs.size(); ++i)
            if (gc.graphs[i].stamp < gc.graphs[old].stamp) old = i;
        graph_drop(gc, old);
        gc.graphs.erase(gc.graphs.begin() + old);
    }
    Graph q{};
    q.B = B; q.U = U; q.has_spkr = has_spkr; q.has_lens = has_lens;
    q.seen = 1;
    q.stamp = ++gc.clock;
    gc.graphs.push_back(q);
    return nullptr;
}

// A new graph takes a graph slot and `need` bytes of staging memory: least recently used graphs give theirs up until both fit
// (PARROT_VOC_GRAPH_MB caps the staging memory of one handle, default 1024 -- it is hipMalloc'ed, outside torch's allocator).
// false: larger than the whole cap.
static bool graph_make_room(VocGraphs& gc, size_t need) {
    static const size_t cap = [] { const char* e = getenv("PARROT_VOC_GRAPH_MB"); return (size_t)(e ? std::max(0, atoi(e)) : 1024) << 20; }();
    for (;;) {
        int n_graphs = 0;
        size_t in_use = 0, lru = gc.graphs.size();
        for (size_t i = 0; i < gc.graphs.size(); ++i) {
            in_use += gc.graphs[i].mem_bytes;
            if (gc.graphs[i].exec) {
                ++n_graphs;
                if (lru == gc.graphs.size() || gc.graphs[i].stamp < gc.graphs[lru].stamp) lru = i;
            }
        }
        if ((n_graphs < VocGraphs::MAX_GRAPHS && in_use + need <= cap) || lru == gc.graphs.size()) return in_use + need <= cap;
        graph_drop(gc, lru);
        gc.graphs[lru].mem_bytes = 0;
        gc.graphs[lru].seen = 0;
        gc.graphs[lru].launched = false;
    }
}

// This shape keeps coming: staging buffers + capture on the handle's own stream (nothing runs during the capture).  false: the
// call runs directly -- and so does the shape from now on, or, where it alone exceeds the cap, for a while.
static bool graph_capture(parrot_voc* v, Graph* g) {
    VocGraphs& gc = v->gc;
    const int B = g->B, U = g->U;
    const size_t n_code = (size_t)B * U * sizeof(int64_t), n_spkr = g->has_spkr ? (size_t)B * sizeof(int64_t) : 0,
                 n_lens = g->has_lens ? (size_t)B * sizeof(int32_t) : 0;
    g->wav_bytes = (size_t)B * (size_t)voc_out_len(v, U) * sizeof(float);
    g->ws_bytes = voc_ws_bytes(v, B, U, voc_streams(v, B, U));
    size_t off = 0;
    auto take = [&](size_t n) { const size_t o = off; off = align_up(off + n, 256); return o; };
    const size_t o_code = take(n_code), o_spkr = take(n_spkr), o_lens = take(n_lens), o_wav = take(g->wav_bytes), o_ws = take(g->ws_bytes);
    if (!graph_make_room(gc, off)) {  // not asked again for a while
        g->seen = -1000;
        return false;
    }
    bool ok = hipMalloc((void**)&g->mem, off) == hipSuccess;
    if (ok) {
        g->mem_bytes = off;
        g->code = reinterpret_cast<int64_t*>(g->mem + o_code);
        g->spkr = g->has_spkr ? reinterpret_cast<int64_t*>(g->mem + o_spkr) : nullptr;
        g->lens = g->has_lens ? reinterpret_cast<int32_t*>(g->mem + o_lens) : nullptr;
        g->wav = reinterpret_cast<float*>(g->mem + o_wav);
        g->ws = g->mem + o_ws;
        ok = hipEventCreateWithFlags(&g->done, hipEventDisableTiming) == hipSuccess;
    }
    if (ok && !gc.cap_stream) ok = hipStreamCreateWithFlags(&gc.cap_stream, hipStreamNonBlocking) == hipSuccess;
    hipGraph_t graph = nullptr;
    if (ok) ok = hipStreamBeginCapture(gc.cap_stream, hipStreamCaptureModeRelaxed) == hipSuccess;
    if (ok) {
        const VocCall cap{g->code, U, g->spkr, nullptr, 0, g->lens, B, U, g->wav, nullptr, g->ws, g->ws_bytes, gc.cap_stream};
        const int rc = voc_forward_impl(v, cap, 0, false);
        const hipError_t e_end = hipStreamEndCapture(gc.cap_stream, &graph);
        ok = rc == PARROT_OK && e_end == hipSuccess && graph && hipGraphInstantiate(&g->exec, graph, nullptr, nullptr, 0) == hipSuccess;
    }
    if (graph) (void)hipGraphDestroy(graph);
    if (!ok) {  // this shape goes direct from now on
        (void)hipGetLastError();
        g->release();
        g->mem_bytes = 0;
        g->dead = true;
    }
    return ok;
}

static int graph_replay(Graph* g, const VocCall& c) {
    hipStream_t s = c.s;
    if (g->launched && g->last != s) HIP_TRY(hipStreamWaitEvent(s, g->done, 0));  // the staging buffers are still the previous replay's
    HIP_TRY(hipMemcpy2DAsync(g->code, (size_t)c.U * sizeof(int64_t), c.code, (size_t)c.code_stride * sizeof(int64_t), (size_t)c.U * sizeof(int64_t), c.B,
                             hipMemcpyDeviceToDevice, s));
    if (g->spkr) HIP_TRY(hipMemcpyAsync(g->spkr, c.spkr, (size_t)c.B * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    if (g->lens) HIP_TRY(hipMemcpyAsync(g->lens, c.unit_lens, (size_t)c.B * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (poison_word()) {
        TRY(poison(g->ws, g->ws_bytes, s));
        TRY(poison(g->wav, g->wav_bytes, s));
        TRY(poison(c.wav_out, g->wav_bytes, s));
        TRY(poison(c.ws, c.ws_bytes, s));
    }
    HIP_TRY(hipGraphLaunch(g->exec, s));
    HIP_TRY(hipMemcpyAsync(c.wav_out, g->wav, g->wav_bytes, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipEventRecord(g->done, s));
    g->last = s;
    g->launched = true;
    return PARROT_OK;
}

// Small forwards through the graph cache (see VocGraphs); the cache's lock is released before every direct fallback.
int parrot::voc_forward_graphed(parrot_voc* v, const VocCall& c) {
    if (!graph_eligible(v, c)) return voc_forward_direct(v, c);
    std::unique_lock<std::mutex> lk(v->gc.mu);
    Graph* g = graph_find_or_count(v->gc, c.B, c.U, v->cfg.multispkr && c.spkr != nullptr, c.unit_lens != nullptr);
    if (!g || g->dead || (!g->exec && (++g->seen < VocGraphs::GRAPH_AFTER || !graph_capture(v, g)))) {
        lk.unlock();
        return voc_forward_direct(v, c);
    }
    return graph_replay(g, c);
}
