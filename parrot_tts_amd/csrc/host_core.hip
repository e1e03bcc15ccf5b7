// host_core.hip -- what every host unit leans on: errors, poison mode, the profiler table, the process defaults with their
// parrot_set_* entries, the per-create scope and the status-flag helpers (declared in host_common.h).
#include "host_common.h"

#include <atomic>
#include <cstring>
#include <mutex>
#include <vector>

using namespace parrot;

// ---------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------
static thread_local std::string g_err;
int parrot::fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

extern "C" int parrot_abi_version(void) { return PARROT_ABI_VERSION; }
extern "C" const char* parrot_last_error(void) { return g_err.c_str(); }

// ---------------------------------------------------------------------------------------------
// Poison mode (tests only): PARROT_POISON_WS = nan | inf | 7f fills every caller-provided workspace / state / output buffer -- and
// the graph cache's staging buffers -- with that bit pattern at the top of each compute entry point, on the caller's stream.  A
// kernel that reads a byte nobody wrote then fails deterministically (NaN / 0 x inf / 3.4e38 in the result) instead of depending
// on what the allocator happened to leave behind.  Unset: no cost, no launches.
// ---------------------------------------------------------------------------------------------
uint32_t parrot::poison_word() {
    static const uint32_t w = [] {
        const char* e = getenv("PARROT_POISON_WS");
        if (!e || !*e || !strcmp(e, "0")) return 0u;
        if (!strcmp(e, "inf")) return 0x7f800000u;
        if (!strcmp(e, "7f")) return 0x7f7f7f7fu;
        return 0x7fc00000u;  // "nan", "1", anything else
    }();
    return w;
}
int parrot::poison(void* p, size_t bytes, hipStream_t s) {
    const uint32_t w = poison_word();
    if (!w || !p || bytes == 0) return PARROT_OK;
    if ((uintptr_t)p & 3) {  // (an unaligned view: bytes)
        HIP_TRY(hipMemsetAsync(p, 0x7f, bytes, s));
        return PARROT_OK;
    }
    const size_t words = bytes / 4;
    if (words) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)p, (int)w, words, s));
    if (bytes & 3) HIP_TRY(hipMemsetAsync((char*)p + 4 * words, 0x7f, bytes & 3, s));
    return PARROT_OK;
}

// ---------------------------------------------------------------------------------------------
// optional per-launch timing of the conv kernel (HIP events on the launch stream), aggregated per
// tile configuration: feeds bench.py's roofline object.  Off by default.
// ---------------------------------------------------------------------------------------------
// (process-wide profiler: one mutex around its state; the flag is an atomic so un-profiled launches never take the lock)
static std::atomic<bool> g_prof_on{false};
static std::mutex g_prof_mu;
static std::vector<ProfRec> g_prof;
static std::vector<std::pair<hipEvent_t, hipEvent_t>> g_prof_pool;

static std::atomic<int> g_prof_row{-1};  // >= 0: only launches of this table row are timed (parrot_prof_begin_row)
bool parrot::prof_on() { return g_prof_on; }
int parrot::prof_open(ProfRec& rec, int row, double flops, double bytes, hipStream_t s) {
    rec.a = rec.b = nullptr;
    const int only = g_prof_row.load();
    if (only >= 0 && row != only) return PARROT_OK;
    bool fresh = false;
    {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        if (g_prof_pool.empty()) fresh = true;
        else {
            rec.a = g_prof_pool.back().first;
            rec.b = g_prof_pool.back().second;
            g_prof_pool.pop_back();
        }
    }
    if (fresh) {
        HIP_TRY(hipEventCreate(&rec.a));
        HIP_TRY(hipEventCreate(&rec.b));
    }
    rec.cfg = row;
    rec.flops = flops;
    rec.bytes = bytes;
    HIP_TRY(hipEventRecord(rec.a, s));
    return PARROT_OK;
}
int parrot::prof_close(ProfRec& rec, hipStream_t s) {
    if (!rec.a) return PARROT_OK;  // (row filtered out)
    HIP_TRY(hipEventRecord(rec.b, s));
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof.push_back(rec);
    return PARROT_OK;
}

extern "C" int parrot_prof_begin(void) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto& r : g_prof) g_prof_pool.push_back({r.a, r.b});
    g_prof.clear();
    g_prof_row = -1;
    g_prof_on = true;
    return PARROT_OK;
}
// The same, timing only the launches of ONE row of the table (the dominant kernel): a pair of event records around every launch
// of a step costs 0.6 ms at B = 64 and 0.4 ms of a 2 ms single-utterance step (they keep consecutive kernels from overlapping
// their ramp-up / drain), which is measurement overhead, not work of the path.
extern "C" int parrot_prof_begin_row(int32_t row) {
    if (row < 0) return fail(PARROT_E_INVALID, "prof_begin_row: row must be >= 0");
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto& r : g_prof) g_prof_pool.push_back({r.a, r.b});
    g_prof.clear();
    g_prof_row = row;
    g_prof_on = true;
    return PARROT_OK;
}
// out[cfg*4 + {0,1,2,3}] = {launches, total ms, algorithmic flops, algorithmic bytes}; n_cfg rows.
extern "C" int parrot_prof_end(double* out, int32_t n_cfg) {
    g_prof_on = false;
    if (!out || n_cfg <= 0) return fail(PARROT_E_INVALID, "prof_end: bad output buffer");
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (int i = 0; i < n_cfg * 4; ++i) out[i] = 0.0;
    for (auto& r : g_prof) {
        HIP_TRY(hipEventSynchronize(r.b));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, r.a, r.b));
        if (r.cfg < n_cfg) {
            out[r.cfg * 4 + 0] += 1.0;
            out[r.cfg * 4 + 1] += ms;
            out[r.cfg * 4 + 2] += r.flops;
            out[r.cfg * 4 + 3] += r.bytes;
        }
    }
    return PARROT_OK;
}

// Process-wide DEFAULTS, read once by every *_create (the handle keeps its own copy and is immutable afterwards, so
// handles stay re-entrant; changing a default never affects a live handle).  Atomics: setters may race with creates.
static std::atomic<int> g_default_prec{-1};
static int parse_prec(const char* e) {
    if (!e) return PARROT_PREC_F16X3;
    if (!strcmp(e, "f32") || !strcmp(e, "0")) return PARROT_PREC_F32;
    if (!strcmp(e, "bf16x6") || !strcmp(e, "1")) return PARROT_PREC_BF16X6;
    if (!strcmp(e, "bf16") || !strcmp(e, "3")) return PARROT_PREC_BF16;
    if (!strcmp(e, "f16") || !strcmp(e, "4")) return PARROT_PREC_F16;
    return PARROT_PREC_F16X3;
}
int parrot::default_prec() {
    int v = g_default_prec.load();
    if (v < 0) {
        v = parse_prec(getenv("PARROT_PRECISION"));
        g_default_prec.store(v);
    }
    return v;
}
extern "C" int parrot_set_default_precision(int32_t prec) {
    if (prec < 0 || prec > PARROT_PREC_F16) return fail(PARROT_E_INVALID, "set_default_precision: PARROT_PREC_* (0..4)");
    g_default_prec.store(prec);
    return PARROT_OK;
}

// Fused whole-ResBlock kernels: 0 off, 1 every eligible stage, 2 (default) all but the exact-fp32 32-channel kernel
// (resblock_fused.h; slower than layer by layer).  PARROT_FUSED / parrot_set_fused_resblocks set the default for
// handles created afterwards.
static std::atomic<int> g_fused{-1};
static int fused_mode() {
    int v = g_fused.load();
    if (v < 0) {
        const char* e = getenv("PARROT_FUSED");
        v = e ? atoi(e) : 2;
        if (v < 0 || v > 2) v = 2;
        g_fused.store(v);
    }
    return v;
}
extern "C" int parrot_set_fused_resblocks(int32_t mode) {
    if (mode < 0 || mode > 2) return fail(PARROT_E_INVALID, "set_fused_resblocks: mode must be 0, 1 or 2");
    g_fused.store(mode);
    return PARROT_OK;
}

// Default for handles created afterwards: fold the back-to-back bias-free projections of an FFT block (quirk Q3) into one each.
// PARROT_TTE_MERGE / parrot_set_tte_merge; parrot_tte_create_ex overrides it per handle.
static std::atomic<int> g_tte_merge{-1};
static int tte_merge_default() {
    int v = g_tte_merge.load();
    if (v < 0) {
        const char* e = getenv("PARROT_TTE_MERGE");
        v = (!e || atoi(e) != 0) ? 1 : 0;
        g_tte_merge.store(v);
    }
    return v;
}
extern "C" int parrot_set_tte_merge(int32_t on) {
    g_tte_merge.store(on ? 1 : 0);
    return PARROT_OK;
}

static int g_num_cus = 256;  // (MI355X; refreshed from the device at the first *_create)
void parrot::query_device() {
    static bool done = false;
    if (done) return;
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) g_num_cus = n;
    done = true;
}
int parrot::num_cus() { return g_num_cus; }

// (the per-create scope: host_common.h)
static thread_local int tl_prec = -1, tl_fused = -1, tl_merge = -1;
CreateScope::CreateScope(int prec, int fused, int merge) : p0(tl_prec), f0(tl_fused), m0(tl_merge) {
    if (prec >= 0) tl_prec = prec;
    if (fused >= 0) tl_fused = fused;
    if (merge >= 0) tl_merge = merge ? 1 : 0;
}
CreateScope::~CreateScope() { tl_prec = p0; tl_fused = f0; tl_merge = m0; }
int parrot::create_prec() { return tl_prec >= 0 ? tl_prec : default_prec(); }
int parrot::create_fused() { return tl_fused >= 0 ? tl_fused : fused_mode(); }
bool parrot::create_merge() { return (tl_merge >= 0 ? tl_merge : tte_merge_default()) != 0; }
int parrot::resolve_parity_prec(int prec, const char* who, int* scheme) {
    if (prec > PARROT_PREC_F16) return fail(PARROT_E_INVALID, std::string(who) + ": unknown precision");
    const int s = prec >= 0 ? prec : default_prec();
    const bool single = s == PARROT_PREC_BF16 || s == PARROT_PREC_F16;  // (the single-MFMA modes)
    if (single && prec >= 0) return fail(PARROT_E_UNSUPPORTED, std::string(who) + ": parity-grade precisions only (f16x3, bf16x6, f32)");
    *scheme = single ? PARROT_PREC_F16X3 : s;
    return PARROT_OK;
}

// ---------------------------------------------------------------------------------------------
// status flags (bad unit / speaker / phone ids <-> the reference's Embedding IndexError, non-finite outputs, bad durations)
// ---------------------------------------------------------------------------------------------
int DevFlag::init() {
    HIP_TRY(hipMalloc((void**)&p, sizeof(int)));
    HIP_TRY(hipMemset(p, 0, sizeof(int)));
    return PARROT_OK;
}
int parrot::check_flag(int* flag, hipStream_t s, int (*decode)(int status)) {
    int h = 0;
    HIP_TRY(hipMemcpyAsync(&h, flag, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (!h) return PARROT_OK;
    HIP_TRY(hipMemsetAsync(flag, 0, sizeof(int), s));
    return decode(h);
}
int parrot::model_status(const char* who, int h) {
    if (h == 6) return fail(PARROT_E_INVALID, std::string(who) + ": repeats can not be negative (a negative duration, duration.py:14)");
    if (h == 7) return fail(PARROT_E_INVALID, std::string(who) + ": row-exact durations: a nonzero duration at a padded source position");
    if (h == 5)
        return fail(PARROT_E_NONFINITE, std::string(who) + ": non-finite output (waveform sample / logits) -- an activation left the range of the fp16 split "
                                                            "scheme (|x| < 8190); create the handle with PARROT_PREC_BF16X6 or PARROT_PREC_F32");
    return fail(PARROT_E_RANGE, std::string(who) + ": embedding index out of range (code " + std::to_string(h) + ")");
}
int parrot::status_async(int* flag, int32_t* dst_dev, hipStream_t s) {
    if (!dst_dev) return fail(PARROT_E_INVALID, "status_async: null destination");
    HIP_TRY(hipMemcpyAsync(dst_dev, flag, sizeof(int), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemsetAsync(flag, 0, sizeof(int), s));
    return PARROT_OK;
}
int parrot::peek_async(int* flag, int32_t* dst_dev, hipStream_t s, const char* who) {
    if (!flag || !dst_dev) return fail(PARROT_E_INVALID, std::string(who) + ": null argument");
    HIP_TRY(hipMemcpyAsync(dst_dev, flag, sizeof(int), hipMemcpyDeviceToDevice, s));
    return PARROT_OK;
}
