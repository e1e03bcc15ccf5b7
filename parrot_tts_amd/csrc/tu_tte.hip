// tu_tte.hip -- one translation unit of libparrot_hip.so: the text-to-unit model's own kernels (the fp32-MFMA attention cores of
// attn.h, tte_glue.h, tte_loss.h) and their launchers, built with the default flags.  Shapes are validated by the callers in
// host_tte*.hip.
#define PARROT_TTE_TU
#include "attn.h"
#include "tte_glue.h"
#include "tte_loss.h"

#define LAUNCH_TRY(...)                         \
    do {                                        \
        hipLaunchKernelGGL(__VA_ARGS__);        \
        hipError_t _e = hipGetLastError();      \
        if (_e != hipSuccess) return _e;        \
    } while (0)

namespace parrot {

hipError_t launch_attention_core(int core, const AttnParams& ap, int B, float* scores, hipStream_t s) {
    const int T = ap.T, H = ap.H, hd = ap.hd;
    const long DT = (long)ap.D * T;
    if (core == ATTN_CORE_FLASH) return launch_attn_flash(ap, B, s);  // any T, online softmax, no score tensor (attn_flash_kernel)
    if (core == ATTN_CORE_FUSED) {  // scores, softmax and context in one launch
        const size_t lds = (size_t)32 * (((T + 31) / 32) * 32 + 1) * sizeof(float);  // 32-query tiles (33 KiB at T = 256: no opt-in needed)
        LAUNCH_TRY((attn_fused_kernel<128, 32>), dim3((T + 31) / 32, B * H), dim3(256), lds, s, ap);
        return hipSuccess;
    }
    {   // scores[b,h][tq][tk] = sum_c (q[c][tq] * sqrt(1/hd)) * k[c][tk]
        BgemmParams p{};
        p.A = ap.qkv; p.B = ap.qkv + DT; p.C = scores;
        p.M = T; p.N = T; p.K = hd;
        p.a_sk = T; p.a_sm = 1; p.b_sk = T; p.b_sn = 1;
        p.a_zb = 3 * DT; p.a_zh = (long)hd * T; p.b_zb = 3 * DT; p.b_zh = (long)hd * T;
        p.c_zb = (long)H * T * T; p.c_zh = (long)T * T; p.ldc = T; p.H = H;
        p.alpha = ap.alpha;
        LAUNCH_TRY(bgemm_mfma_kernel, dim3((T + 63) / 64, (T + 63) / 64, B * H), dim3(256), 0, s, p);
    }
    LAUNCH_TRY(softmax_mask_kernel, dim3((B * H * T + 3) / 4), dim3(256), 0, s, scores, ap.valid, B * H * T, T, H * T);
    {   // ctx[b][h*hd + c][tq] = sum_tk v[c][tk] * P[tq][tk]
        BgemmParams p{};
        p.A = ap.qkv + 2 * DT; p.B = scores; p.C = ap.ctx;
        p.M = hd; p.N = T; p.K = T;
        p.a_sk = 1; p.a_sm = T; p.b_sk = 1; p.b_sn = T;
        p.a_zb = 3 * DT; p.a_zh = (long)hd * T; p.b_zb = (long)H * T * T; p.b_zh = (long)T * T;
        p.c_zb = DT; p.c_zh = (long)hd * T; p.ldc = T; p.H = H;
        p.alpha = 1.0f;
        LAUNCH_TRY(bgemm_mfma_kernel, dim3((T + 63) / 64, (hd + 63) / 64, B * H), dim3(256), 0, s, p);
    }
    return hipSuccess;
}

hipError_t launch_tte_embed(const int64_t* phones, const float* emb, const float* pe, const int32_t* row_len, float* x, int B, int S, int D, int vocab,
                            int* err, hipStream_t s) {
    LAUNCH_TRY(tte_embed_kernel, dim3((S + 63) / 64, (D + 63) / 64, B), dim3(256), 0, s, phones, emb, pe, row_len, x, S, D, vocab, err);
    return hipSuccess;
}
hipError_t launch_add_channel_vec(float* x, const int64_t* id, const float* tab, int B, int C, int T, int n_rows, int* err, hipStream_t s) {
    const size_t total = (size_t)B * C * T;
    LAUNCH_TRY(add_channel_vec_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, id, tab, C, T, n_rows, total, err);
    return hipSuccess;
}
hipError_t launch_layernorm(const float* x, const float* g, const float* b, float* y, int B, int C, int T, int relu_in, hipStream_t s) {
    LAUNCH_TRY(layernorm_cf_kernel<16>, dim3((T + 63) / 64, B), dim3(16 * 64), 0, s, x, g, b, y, C, T, 1e-5f, relu_in);
    return hipSuccess;
}
hipError_t launch_transpose_cf_to_cl(const float* x, float* y, int B, int C, int T, hipStream_t s) {
    LAUNCH_TRY(transpose_cf_to_cl_kernel, dim3((T + 63) / 64, (C + 63) / 64, B), dim3(256), 0, s, x, y, C, T);
    return hipSuccess;
}
hipError_t launch_durations(const float* ld_raw, const uint8_t* src_valid, float* log_dur, int64_t* dur, int32_t* cum, int32_t* out_len, int B, int S,
                            const int32_t* src_len, int* err, hipStream_t s) {
    LAUNCH_TRY(duration_kernel, dim3(B), dim3(256), 0, s, ld_raw, src_valid, log_dur, dur, cum, out_len, S, src_len, err);
    return hipSuccess;
}
hipError_t launch_dur_prefix(const int64_t* dur, int32_t* cum, int32_t* out_len, int B, int S, int* err, const int32_t* src_len, hipStream_t s) {
    LAUNCH_TRY(dur_prefix_kernel, dim3(B), dim3(256), 0, s, dur, cum, out_len, S, err, src_len);
    return hipSuccess;
}
hipError_t launch_length_regulate(const float* enc, const int32_t* cum, const int32_t* out_len, const float* pe, float* y, uint8_t* tgt_mask, int B,
                                  int S, int L, int D, int* gstat, int gstat_reset, int row_exact, int pe_stride, hipStream_t s) {
    LAUNCH_TRY(length_regulate_kernel, dim3((L + 63) / 64, B), dim3(256), 0, s, enc, cum, out_len, pe, y, tgt_mask, S, L, D, gstat, gstat_reset,
               row_exact, pe_stride);
    return hipSuccess;
}
hipError_t launch_argmax_guard(const float* logits, int64_t* ids, int B, int V, int L, int* err, float guard, int* glist, int* gstat, int row0,
                               const RefineArgs& r, hipStream_t s) {
    LAUNCH_TRY(argmax_cf_kernel, dim3((L + 63) / 64, B), dim3(64 * ARGMAX_WAVES), 0, s, logits, ids, V, L, err, guard, glist, gstat, row0);
    if (gstat && r.x) {  // re-evaluate the head of the low-margin positions in fp64 (workgroups beyond the count exit at once)
        const bool deep = r.f != nullptr;
        LAUNCH_TRY(tie_guard_refine_kernel, dim3(TIE_GUARD_MAX), dim3(256), (size_t)(r.D + (deep ? r.F : 0)) * sizeof(double), s, r.x, r.hwt, r.hb,
                   ids, r.D, V, L, glist, gstat, r.f, r.h, r.w2t, r.b2, r.F, r.gref, row0);
    }
    return hipSuccess;
}
hipError_t launch_guard_stats_sum(const int* gstat, int mask, int* dst, hipStream_t s) {
    LAUNCH_TRY(guard_stats_sum_kernel, dim3(1), dim3(1), 0, s, gstat, mask, dst);
    return hipSuccess;
}
hipError_t launch_guard_gather(const float* gref, const int* glist, const int* gstat, int mask, int V, int max_n, float* logits, int* list,
                               hipStream_t s) {
    LAUNCH_TRY(guard_gather_kernel, dim3(max_n), dim3(256), 0, s, gref, glist, gstat, mask, V, max_n, logits, list);
    return hipSuccess;
}

hipError_t launch_tte_loss(const float* logits, const int64_t* targets, int N, int V, int64_t ignore_index, const float* log_dur, const int64_t* dur,
                           const uint8_t* src_mask, int n_src, double* nll, LossCounts* cnt, int64_t* bad, double* out, float* losses, hipStream_t s) {
    const int nblk = (N + LOSS_WAVES - 1) / LOSS_WAVES;
    LAUNCH_TRY(loss_rows_kernel<false>, dim3(nblk), dim3(64 * LOSS_WAVES), 0, s, logits, targets, N, V, ignore_index, nll, cnt, bad, nullptr, nullptr);
    LAUNCH_TRY(loss_reduce_kernel, dim3(1), dim3(LOSS_REDUCE), 0, s, nll, cnt, bad, nblk, log_dur, dur, src_mask, n_src, out, losses);
    return hipSuccess;
}
hipError_t launch_tte_loss_grad(const float* logits, const int64_t* targets, int N, int V, int64_t ignore_index, const float* log_dur,
                                const int64_t* dur, const uint8_t* src_mask, int n_src, const double* weights, double* nll, LossCounts* cnt,
                                int64_t* bad, LossScale* scale, double* out, float* losses, float* grad_logits, float* grad_log_dur, hipStream_t s) {
    const int nblk = (N + LOSS_WAVES - 1) / LOSS_WAVES;
    LAUNCH_TRY(loss_count_kernel, dim3(1), dim3(LOSS_REDUCE), 0, s, targets, N, V, ignore_index, log_dur, dur, src_mask, n_src, weights, scale,
               grad_log_dur);
    if (grad_logits)
        LAUNCH_TRY(loss_rows_kernel<true>, dim3(nblk), dim3(64 * LOSS_WAVES), 0, s, logits, targets, N, V, ignore_index, nll, cnt, bad, scale,
                   grad_logits);
    else
        LAUNCH_TRY(loss_rows_kernel<false>, dim3(nblk), dim3(64 * LOSS_WAVES), 0, s, logits, targets, N, V, ignore_index, nll, cnt, bad, nullptr,
                   nullptr);
    LAUNCH_TRY(loss_reduce_kernel, dim3(1), dim3(LOSS_REDUCE), 0, s, nll, cnt, bad, nblk, log_dur, dur, src_mask, n_src, out, losses);
    return hipSuccess;
}

}  // namespace parrot
