// host_tte_debug.hip -- the text-to-unit model's kernels on their own (tests: include/parrot_hip_debug.h), on caller-owned buffers,
// through the launchers of attn.h and tte_glue.h that fft_block, encode and decode (host_tte.hip) call.
#include "host_common.h"

#include <algorithm>

#include "attn.h"
#include "tte_glue.h"

using namespace parrot;

// ---------------------------------------------------------------------------------------------
// The attention cores and the LayerNorm.
// ---------------------------------------------------------------------------------------------
static float* debug_attention_ws(Arena& a, int B, int T, int H, int core) {
    float* scores = core == ATTN_CORE_THREE ? a.take<float>((size_t)B * H * T * T) : nullptr;
    a.take<char>(1);  // (never empty: the fused and flash cores take no workspace, and the entry refuses a null one)
    return scores;
}
extern "C" size_t parrot_debug_attention_workspace_bytes(int32_t B, int32_t T, int32_t H, int32_t core) {
    if (B <= 0 || T <= 0 || H <= 0 || core < ATTN_CORE_THREE || core > ATTN_CORE_FLASH) return 0;
    Arena a(nullptr, 0);
    (void)debug_attention_ws(a, B, T, H, core);
    return align_up(a.off, 256);
}
extern "C" int parrot_debug_attention(const float* qkv, const uint8_t* valid, float* ctx, int32_t B, int32_t T, int32_t H, int32_t hd,
                                      int32_t core, void* ws, size_t ws_bytes, void* stream) {
    if (!qkv || !valid || !ctx || !ws) return fail(PARROT_E_INVALID, "debug_attention: null argument");
    if (B <= 0 || T <= 0 || H <= 0 || hd <= 0) return fail(PARROT_E_INVALID, "debug_attention: non-positive size");
    if (core < ATTN_CORE_THREE || core > ATTN_CORE_FLASH) return fail(PARROT_E_INVALID, "debug_attention: core in 0 .. 2");
    if ((long)B * H > 65535 || (long)B * H * T >= (1L << 30) || (long)H * hd >= (1L << 30))  // (grid rows; softmax_mask_kernel's int row count)
        return fail(PARROT_E_UNSUPPORTED, "debug_attention: B H > 65535, or B H T / H hd beyond the kernels' 32-bit indices");
    if (core == ATTN_CORE_FUSED && (hd != 128 || T > ATTN_TMAX))
        return fail(PARROT_E_UNSUPPORTED, "debug_attention: the fused core takes hd = 128 and T <= 256 only");
    if (core == ATTN_CORE_FLASH && !attn_flash_has(hd)) return fail(PARROT_E_UNSUPPORTED, "debug_attention: the flash core takes hd in {16, 32, 64, 128} only");
    hipStream_t s = (hipStream_t)stream;
    Arena a(ws, ws_bytes);
    float* scores = debug_attention_ws(a, B, T, H, core);
    if (!a.ok) return fail(PARROT_E_NOMEM, "debug_attention: workspace too small");
    if (poison_word()) {
        TRY(poison(ws, ws_bytes, s));
        TRY(poison(ctx, (size_t)B * H * hd * T * sizeof(float), s));
    }
    HIP_TRY(launch_attention_core(core, attn_params(qkv, valid, ctx, T, H, H * hd), B, scores, s));
    return PARROT_OK;
}
extern "C" int parrot_debug_layernorm(const float* x, const float* gamma, const float* beta, float* y, int32_t B, int32_t C, int32_t T,
                                      int32_t relu_in, void* stream) {
    if (!x || !gamma || !beta || !y) return fail(PARROT_E_INVALID, "debug_layernorm: null argument");
    if (B <= 0 || C <= 0 || T <= 0) return fail(PARROT_E_INVALID, "debug_layernorm: non-positive size");
    if (B > 65535) return fail(PARROT_E_UNSUPPORTED, "debug_layernorm: B > 65535 (one grid row per batch row)");
    hipStream_t s = (hipStream_t)stream;
    if (poison_word()) TRY(poison(y, (size_t)B * C * T * sizeof(float), s));
    HIP_TRY(launch_layernorm(x, gamma, beta, y, B, C, T, relu_in != 0, s));
    return PARROT_OK;
}

// ---------------------------------------------------------------------------------------------
// The duration, length-regulator and argmax / tie-guard kernels.  `status` stands in for the handle's device status word.
// ---------------------------------------------------------------------------------------------
static int debug_sizes(const char* who, long B, long n1, long n2, long n3) {
    if (B <= 0 || n1 <= 0 || n2 <= 0 || n3 <= 0) return fail(PARROT_E_INVALID, std::string(who) + ": non-positive size");
    if (B > 65535 || n1 > PARROT_DEBUG_MAX_DIM || n2 > PARROT_DEBUG_MAX_DIM || n3 > PARROT_DEBUG_MAX_DIM)
        return fail(PARROT_E_UNSUPPORTED, std::string(who) + ": B > 65535 or a dimension beyond PARROT_DEBUG_MAX_DIM");
    return PARROT_OK;
}
extern "C" int parrot_debug_durations(const float* ld_raw, const uint8_t* src_valid, const int32_t* src_len, int32_t B, int32_t S, float* log_dur,
                                      int64_t* dur, int32_t* cum, int32_t* out_len, int32_t* status, void* stream) {
    if (!ld_raw || !src_valid || !log_dur || !dur || !cum || !out_len || !status) return fail(PARROT_E_INVALID, "debug_durations: null argument");
    TRY(debug_sizes("debug_durations", B, S, 1, 1));
    hipStream_t s = (hipStream_t)stream;
    if (poison_word()) {
        TRY(poison(log_dur, (size_t)B * S * sizeof(float), s));
        TRY(poison(dur, (size_t)B * S * sizeof(int64_t), s));
        TRY(poison(cum, (size_t)B * S * sizeof(int32_t), s));
        TRY(poison(out_len, (size_t)B * sizeof(int32_t), s));
    }
    HIP_TRY(launch_durations(ld_raw, src_valid, log_dur, dur, cum, out_len, B, S, src_len, status, s));
    return PARROT_OK;
}
extern "C" int parrot_debug_length_regulate(const float* enc, const int64_t* dur, const int32_t* src_len, const float* pe, int32_t B, int32_t S,
                                            int32_t D, int32_t L, int32_t P, int32_t row_exact, float* y, uint8_t* tgt_mask, int32_t* cum,
                                            int32_t* out_len, int32_t* status, void* stream) {
    if (!enc || !dur || !pe || !y || !cum || !out_len || !status) return fail(PARROT_E_INVALID, "debug_length_regulate: null argument");
    if (L <= 0) return fail(PARROT_E_INVALID, "debug_length_regulate: L must be > 0");
    TRY(debug_sizes("debug_length_regulate", B, S, D, L));
    if (L >= P) return fail(PARROT_E_RANGE, "debug_length_regulate: L >= P (pe[L] out of range, fft.py:18)");
    hipStream_t s = (hipStream_t)stream;
    if (poison_word()) {
        TRY(poison(y, (size_t)B * D * L * sizeof(float), s));
        TRY(poison(tgt_mask, (size_t)B * L, s));
        TRY(poison(cum, (size_t)B * S * sizeof(int32_t), s));
        TRY(poison(out_len, (size_t)B * sizeof(int32_t), s));
    }
    HIP_TRY(launch_dur_prefix(dur, cum, out_len, B, S, status, src_len, s));
    HIP_TRY(launch_length_regulate(enc, cum, out_len, pe, y, tgt_mask, B, S, L, D, nullptr, 1, row_exact ? 1 : 0, -1, s));
    return PARROT_OK;
}
extern "C" int parrot_debug_argmax_guard(const float* logits, int32_t B, int32_t V, int32_t L, float guard, int32_t row0, const float* x, int32_t D,
                                         const float* hwt, const float* hb, const float* f, const float* h, const float* w2t, const float* b2,
                                         int32_t F, const int32_t* gstat_start, int64_t* ids, int32_t* glist, int32_t* gstat, float* gref,
                                         int32_t* status, void* stream) {
    if (!logits || !ids || !glist || !gstat || !status) return fail(PARROT_E_INVALID, "debug_argmax_guard: null argument");
    TRY(debug_sizes("debug_argmax_guard", B, V, L, 1));
    if (!(guard >= 0.f) || row0 < 0) return fail(PARROT_E_INVALID, "debug_argmax_guard: guard and row0 must be >= 0");
    const bool on = guard > 0.f, deep = f != nullptr;
    if (x) {
        if (!hwt || !gref || (deep && (!h || !w2t))) return fail(PARROT_E_INVALID, "debug_argmax_guard: refinement without hwt / gref (deep form: h, w2t)");
        TRY(debug_sizes("debug_argmax_guard", B, D, deep ? F : 1, 1));
        if ((size_t)(D + (deep ? F : 0)) * sizeof(double) > 60000) return fail(PARROT_E_UNSUPPORTED, "debug_argmax_guard: D + F doubles beyond the workgroup's LDS");
    }
    if (gstat_start && (gstat_start[0] < 0 || gstat_start[3] < 0 || gstat_start[3] > std::min(gstat_start[0], TIE_GUARD_MAX)))
        return fail(PARROT_E_INVALID, "debug_argmax_guard: gstat_start needs 0 <= [3] <= min([0], 256)");
    hipStream_t s = (hipStream_t)stream;
    if (poison_word()) {  // (a preset list is an input: with gstat_start, and with the guard off, list / statistics / refined rows stay the caller's)
        TRY(poison(ids, (size_t)B * L * sizeof(int64_t), s));
        if (on && !gstat_start) {
            TRY(poison(glist, (size_t)2 * TIE_GUARD_MAX * sizeof(int32_t), s));
            if (x) TRY(poison(gref, (size_t)TIE_GUARD_MAX * V * sizeof(float), s));
        }
    }
    if (on) {  // what length_regulate_kernel leaves at the start of a decode: a restart, or the caller's second row group of a lane
        const int32_t restart[4] = {0, 0, 0x7f800000, 0};
        HIP_TRY(hipMemcpyAsync(gstat, gstat_start ? gstat_start : restart, sizeof(restart), hipMemcpyHostToDevice, s));
    }
    RefineArgs r;
    r.x = x; r.hwt = hwt; r.hb = hb; r.f = f; r.h = h; r.w2t = w2t; r.b2 = b2; r.D = D; r.F = F; r.gref = gref;
    HIP_TRY(launch_argmax_guard(logits, ids, B, V, L, status, guard, on ? glist : nullptr, on ? gstat : nullptr, row0, r, s));
    return PARROT_OK;
}
