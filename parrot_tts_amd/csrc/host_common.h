// host_common.h -- what the host units (host_*.hip) share: error reporting, the workspace arena, the conv plan and its launch
// options, and the declarations of the helpers that cross units.  Internal: nothing here is part of the C ABI.
// Every piece of process-wide or thread-local state has ONE definition (host_core.hip) and is reached through the functions below.
#pragma once
#include "../../include/parrot_hip_debug.h"  // (parrot_hip.h + the test / profiling entry points)

#include <hip/hip_runtime.h>

#include <memory>
#include <string>

#include "conv_consts.h"  // (NUM_TILE_CFGS, the PRE_* / ACT_* / EPI_* constants)

namespace parrot {

// errors: the message lands in the calling thread's parrot_last_error()
int fail(int code, const std::string& msg);
}  // namespace parrot
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return fail(PARROT_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));          \
    } while (0)
#define TRY(expr)                \
    do {                         \
        int _r = (expr);         \
        if (_r != PARROT_OK) return _r; \
    } while (0)

namespace parrot {

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// bump allocator over the caller's workspace
struct Arena {
    char* base;
    size_t cap, off;
    bool ok;
    Arena(void* p, size_t n) : base((char*)p), cap(n), off(0), ok(true) {}
    template <typename T>
    T* take(size_t n) {
        off = align_up(off, 256);
        size_t bytes = n * sizeof(T);
        if (base && off + bytes > cap) ok = false;
        T* r = base ? (T*)(base + off) : nullptr;
        off += bytes;
        return r;
    }
};

// Poison mode (tests only, PARROT_POISON_WS): host_core.hip
uint32_t poison_word();
int poison(void* p, size_t bytes, hipStream_t s);

// optional per-launch timing (parrot_prof_*): host_core.hip
// A row of the table is one kernel instantiation; the numbers are the positions of bench.py's TILE_NAMES (rows 0 .. NUM_TILE_CFGS - 1:
// conv_mfma_kernel of that tile id, then the enumerators below).
enum ProfRow {
    PROF_SPLIT = NUM_TILE_CFGS,          // conv_split_kernel on the block shape of exact tile 0 ...
    PROF_SPLIT_T1,                       // ... and of exact tile 1 (PROF_SPLIT + tile id)
    PROF_RESBLOCK_FUSED,               // resblock_fused16_kernel (and resblock_fused_kernel)
    PROF_SPLIT_V2,                       // conv_split_kernel variant 2 (128 x 64 tile)
    PROF_SPLIT_V3,                       // conv_split_kernel variant 3
    PROF_RBS_32,                         // resblock_split_kernel<SCH, 2>
    PROF_RBS_16,                         // resblock16_split_kernel
    PROF_VALU_CONV1,                     // conv1_valu_kernel / linear1_valu_kernel (valu_kind 1)
    PROF_VALU_CONVT,                     // convt_valu_kernel (valu_kind 2)
    PROF_SPLIT16,                        // conv_split16_kernel, even variants
    PROF_SPLIT16_ODD,                    // conv_split16_kernel, odd variants (the 64-row tile)
    PROF_UNUSED,
    PROF_SPLIT16_WIDE,                   // conv_split16_kernel variant 4 (128 x 160)
    PROF_RBS_64,                         // resblock_split_kernel<SCH, 4>
    PROF_RBS_128,                        // resblock_split_kernel<SCH, 8>
    PROF_RBS_256,                        // resblock_split_kernel<SCH, 16>
    PROF_MRF,                            // the whole-MRF launch
    PROF_ROW_COUNT
};
static_assert(PROF_SPLIT_V2 == PROF_SPLIT + 3 && PROF_VALU_CONVT == PROF_VALU_CONV1 + 1 && PROF_SPLIT16_ODD == PROF_SPLIT16 + 1 && PROF_ROW_COUNT == NUM_TILE_CFGS + 17, "profiler rows follow bench.py's TILE_NAMES");
struct ProfRec {
    hipEvent_t a, b;
    int cfg;
    double flops, bytes;
};
bool prof_on();  // (an atomic flag: un-profiled launches never take the profiler's lock)
int prof_open(ProfRec& rec, int row, double flops, double bytes, hipStream_t s);
int prof_close(ProfRec& rec, hipStream_t s);

// Process-wide defaults and the per-create scope (host_core.hip).
int default_prec();
void query_device();  // refreshes num_cus() from the device; every *_create calls it
int num_cus();
// Per-handle modes (parrot_*_create_ex) reach the plan builders through a THREAD-LOCAL scope, never through the process
// defaults: a create on one thread cannot leak its precision / fusion / merge mode into a parrot_conv_create or another
// *_create running on a second thread, and a concurrent parrot_set_* is neither seen half-way nor reverted afterwards.
struct CreateScope {
    int p0, f0, m0;
    CreateScope(int prec, int fused, int merge);
    ~CreateScope();
};
int create_prec();
int create_fused();
bool create_merge();
// handles that offer the parity-grade schemes only (mel, aligner): `prec` < 0 = the process default, a single-MFMA default -> fp16x3
int resolve_parity_prec(int prec, const char* who, int* scheme);

// The device status word of a handle: kernels raise it, parrot_*_check / _status_async report and clear it.
struct DevFlag {
    int* p = nullptr;
    DevFlag() = default;
    DevFlag(const DevFlag&) = delete;
    ~DevFlag() { if (p) (void)hipFree(p); }
    int init();  // allocate and zero
    operator int*() const { return p; }
};
// Synchronises the stream; 0, or clears the flag and returns decode(status word) -- the handle's own fail(code, message)
int check_flag(int* flag, hipStream_t s, int (*decode)(int status));
// vocoder / TTE status words: 5 non-finite output, 6 / 7 bad durations, anything else a bad embedding index
int model_status(const char* who, int status);
// The flag without a synchronisation: copy it to dst_dev[0] (device memory) on `stream` and clear it, so the caller can read it
// with a device-to-host transfer it performs anyway (the shims fetch it together with the TTE's expanded lengths).
int status_async(int* flag, int32_t* dst_dev, hipStream_t s);
// ... and without clearing it (the shims' first-forward range probe: a bad-id flag stays for the regular reporting path)
int peek_async(int* flag, int32_t* dst_dev, hipStream_t s, const char* who);

}  // namespace parrot

// ---------------------------------------------------------------------------------------------
// conv plan (host_conv.hip)
// ---------------------------------------------------------------------------------------------
struct parrot_conv {
    parrot_conv_desc d{};
    int groups = 1;
    int M = 0, Mg = 0, Cout = 0, Cin = 0;  // Cin per group
    int kk = 1, dil = 1, pad_left = 0, u = 1;
    int cfg = 0;
    int nchunks = 0, n_it = 0;
    float* wfrag = nullptr;
    float* bias = nullptr;
    int prec = 0;              // 0: exact fp32 MFMA, else the split scheme of conv_split.h (PARROT_PREC_*: 16-bit MFMAs, fp32 accumulate)
    uint16_t* wfrag16 = nullptr;  // [m_tile][chunk*tap][piece][lane][8 x 16 bit]
    int n_it16 = 0;
    float wscale = 1.f;        // power-of-two weight scale inside the fp16 pieces (1 for bf16 schemes)
    bool mfma16 = false;       // split plan packed for conv_split16_kernel (16x16x32 MFMA, 32-channel chunks)
    int* err_flag = nullptr;   // device flag of the owning model (set on a non-finite tanh output: conv_post)
    bool late_res = false;     // add the residual in the epilogue instead of folding it into the accumulator init (TTE layers)
    int valu_kind = 0;         // 1: conv1_valu_kernel<7>, 2: convt_valu_kernel<16,4,2,1> (conv_valu.h); weights in their original layout
    float* wraw = nullptr;

    ~parrot_conv() {
        if (wraw) (void)hipFree(wraw);
        if (wfrag16) (void)hipFree(wfrag16);
        if (wfrag) (void)hipFree(wfrag);
        if (bias) (void)hipFree(bias);
    }
    int out_len(int Tin) const {
        if (!d.transposed) return Tin + 2 * d.padding - d.dilation * (d.k - 1);
        return (Tin - 1) * d.stride - 2 * d.padding + d.k;
    }
};

namespace parrot {

// Operand planes between conv_split16 layers (conv_split16.h): `xplane` replaces x as the input (the values are the same: the
// producer applied this layer's own leaky ReLU / scale / split); `yplane` is written beside y -- or instead of it (plane_only) --
// with the NEXT layer's slope.  Dense batch rows of pieces x 2 C T bytes.
struct PlaneArgs {
    const void* xplane = nullptr;
    void* yplane = nullptr;
    float yslope = 1.f;
    int plane_only = 0;
};
// can layer `c` take its input from / write its output to an operand plane?  (conv_split16 plans of the MRF: k = 7 / 11)
inline bool plane_ok(const parrot_conv* c) { return c && c->mfma16 && c->prec >= 1 && (c->kk == 7 || c->kk == 11) && c->M % 16 == 0 && c->Cin % 32 == 0; }
inline size_t plane_row_bytes(int prec, int C, int T) { return (size_t)(prec == PARROT_PREC_F16X3 ? 2 : 1) * 2 * C * T; }
// Ragged batches: row b holds len[b] real units = len[b] * mul + add samples at the current layer (row_true_len, conv_mfma.h); every
// layer applies its zero padding at the row's own end.  len == nullptr: dense rows.
struct RowLens {
    const int32_t* len = nullptr;
    int mul = 1, add = 0;
};
// what only some callers of conv_launch pass
struct ConvOpts {
    RowLens rows;
    PlaneArgs planes;
};

// Build a plan.  `groups` > 1: torch grouped-conv weight layout (c_out, c_in/groups, k), d.c_in = TOTAL.
int conv_build(parrot_conv** out, const parrot_conv_desc* d, int groups, const float* w, const float* bias, bool allow16 = true);
int make_conv(std::unique_ptr<parrot_conv>& slot, int cin, int cout, int k, int dil, int pad, int transposed, int stride, int pre, float slope,
              int act, const float* w, const float* b, int groups = 1, bool allow16 = true);
int upload(float** dst, const float* src, size_t n);
int conv_launch(const parrot_conv* c, const float* x, const float* res, float* y, int B, int Tin, int epi, float div, hipStream_t s,
                const ConvOpts& o = ConvOpts());

}  // namespace parrot
