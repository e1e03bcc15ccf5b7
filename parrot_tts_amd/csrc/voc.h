// voc.h -- the vocoder handle and what crosses its three host units: host_voc.hip (create, queries, the direct and the chunked
// forward), host_voc_mrf.hip (how a stage's MRF is run) and host_voc_graph.hip (the graph cache of small shapes).
// Internal: nothing here is part of the C ABI.
#pragma once
#include "host_common.h"

#include <algorithm>
#include <mutex>
#include <vector>

namespace parrot {

// HIP-graph replay of small forwards (PARROT_VOC_GRAPH, default on; B x U <= 8192 units): a forward is ~130 dependent launches
// of 7-40 us on up to three streams -- at one utterance the fork / join events and the launch gaps are a fifth of it.  A SHAPE
// (B, U, with / without speaker ids and row lengths) that keeps recurring is captured once (GRAPH_AFTER below; the first calls also warm lazy
// state), on a stream of the handle and into staging buffers of the handle (ids, lengths, waveform, workspace: one allocation per
// cached shape, made at capture time -- never per call): PyTorch's allocator hands out different addresses from call to call, and
// a graph bakes its addresses in.  A replay copies the caller's ids / lengths in (a few KB), launches the graph and copies the
// waveform out: the same kernels with the same arguments in the same order, the MRF branch streams as graph edges.
struct VocGraphs {
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
    // (staging memory of all cached shapes of a handle together: PARROT_VOC_GRAPH_MB, default 1024 -- see graph_make_room)
    std::vector<Graph> graphs;
    std::mutex mu;
    unsigned long clock = 0;
    hipStream_t cap_stream = nullptr;
    void clear() {  // (the handle's destructor)
        for (Graph& g : graphs) g.release();
        if (cap_stream) (void)hipStreamDestroy(cap_stream);
    }
};

}  // namespace parrot

// ---------------------------------------------------------------------------------------------
// vocoder
// ---------------------------------------------------------------------------------------------
struct parrot_voc {
    parrot_voc_cfg cfg{};
    float* dict = nullptr;
    float* spkr = nullptr;
    parrot::DevFlag err;
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
    float* dbg_absmax = nullptr;       // parrot_voc_debug_absmax: (n_stages + 2) device floats, max |conv input| per group (caller-owned)
    parrot::VocGraphs gc;              // the graph cache of small shapes (host_voc_graph.hip)
    ~parrot_voc() {
        gc.clear();
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

namespace parrot {

// The workspace of one forward of (B, U) with ns concurrent MRF branches: ONE function sizes and carves it (voc_scratch).
struct VocScratch {
    float* x0;                  // the embedded input (B, model_in_dim, U)
    float* P[3];                // stage in / ups out / MRF sum, rotating
    struct Tmp {
        float *mid, *res_a, *res_b;
    } tmp[PARROT_MAX_KERNELS];  // per concurrent branch
};

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

// the arguments of one forward (parrot_voc_forward_feats'; code rows code_stride apart)
struct VocCall {
    const int64_t* code; int code_stride;
    const int64_t* spkr;
    const float* feats; int32_t n_feat;
    const int32_t* unit_lens;
    int32_t B, U;
    float* wav_out;
    float* const* stage_out;
    void* ws; size_t ws_bytes;
    hipStream_t s;
};

// host_voc.hip
int voc_streams(const parrot_voc* v, int B, int U);
size_t voc_ws_bytes(const parrot_voc* v, int B, int U, int ns);
long voc_out_len(const parrot_voc* v, int U);
int voc_amax(const parrot_voc* v, int group, const float* src, size_t n, hipStream_t q);
// ns_sized > 0 (chunked path): the number of concurrent MRF branches the caller sized the workspace with, else the shape's own
// rule; stage_events: record the handle's stage events (not while a graph capture is running on c.s: no event records into it)
int voc_forward_impl(parrot_voc* v, const VocCall& c, int ns_sized, bool stage_events);
int voc_forward_direct(parrot_voc* v, const VocCall& c);  // (+ poison mode)

// host_voc_mrf.hip
bool mrf_pair_shape(const parrot_voc* v, int stage, int j);  // block (stage, j) has a fused pair kernel (resblock_split.h)
int mrf_create(parrot_voc* v, const parrot_voc_weights* w);  // rb_stream, rb_wsc, rb_conv_halves, mrf_ok
int mrf_stage(const parrot_voc* v, int stage, const float* X, float* XS, const VocScratch& w, int B, int T, hipStream_t s, int ns,
              const RowLens& rows);

// host_voc_graph.hip
int voc_forward_graphed(parrot_voc* v, const VocCall& c);

}  // namespace parrot
