// tu_tte_train.hip -- one translation unit of libparrot_hip.so: the TTE's training kernels (tte_train.h), their launchers, and this
// unit's own instantiation of bgemm_mfma_kernel (attn.h) behind a launcher that takes any strides.  A launcher refuses
// (hipErrorInvalidValue, before any launch) sizes below 1 and grids beyond the limits; the model's shapes are validated by the
// callers in host_tte_train.hip.
#define PARROT_TTE_TU  // (attn.h shows its kernel bodies to the unit that instantiates them)
#include "attn.h"
#define PARROT_TTE_TRAIN_TU
#include "tte_train.h"

#define LAUNCH(...)                     \
    do {                                \
        hipLaunchKernelGGL(__VA_ARGS__); \
        return hipGetLastError();       \
    } while (0)

namespace parrot {

static inline bool grid_ok(size_t blocks) { return blocks >= 1 && blocks <= 0x7fffffffu; }
static inline unsigned blocks256(size_t n) { return (unsigned)((n + 255) / 256); }

hipError_t tt_launch_bgemm(const BgemmTrainParams& q, int Z, hipStream_t s) {
    if (q.M < 1 || q.N < 1 || q.K < 1 || q.H < 1 || Z < 1 || Z > 65535 || (q.M + 63) / 64 > 65535) return hipErrorInvalidValue;
    BgemmParams p{};
    p.A = q.A; p.B = q.B; p.C = q.C;
    p.M = q.M; p.N = q.N; p.K = q.K;
    p.a_sk = q.a_sk; p.a_sm = q.a_sm; p.b_sk = q.b_sk; p.b_sn = q.b_sn;
    p.a_zb = q.a_zb; p.a_zh = q.a_zh; p.b_zb = q.b_zb; p.b_zh = q.b_zh;
    p.c_zb = q.c_zb; p.c_zh = q.c_zh; p.ldc = q.ldc; p.H = q.H;
    p.alpha = q.alpha;
    LAUNCH(bgemm_mfma_kernel, dim3((q.N + 63) / 64, (q.M + 63) / 64, Z), dim3(256), 0, s, p);
}
hipError_t tt_launch_ln_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, long rows, int C, hipStream_t s) {
    if (rows < 1 || C < 1 || !grid_ok((size_t)(rows + 3) / 4)) return hipErrorInvalidValue;
    LAUNCH(ln_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, x, gamma, beta, y, mean, rstd, rows, C);
}
hipError_t tt_launch_ln_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, const float* res, float* dx,
                            float* dyxh, long rows, int C, int relu_mask, hipStream_t s) {
    if (rows < 1 || C < 1 || !grid_ok((size_t)(rows + 3) / 4)) return hipErrorInvalidValue;
    LAUNCH(ln_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, dy, x, gamma, mean, rstd, res, dx, dyxh, rows, C, relu_mask);
}
hipError_t tt_launch_softmax_fwd(float* sc, float* pd, const uint8_t* key_valid, long rows, int T, int HT, DropArgs d, hipStream_t s) {
    if (rows < 1 || T < 1 || HT < 1 || !grid_ok((size_t)(rows + 3) / 4)) return hipErrorInvalidValue;
    LAUNCH(softmax_drop_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, sc, pd, key_valid, rows, T, HT, d);
}
hipError_t tt_launch_softmax_bwd(const float* P, float* dP, long rows, int T, DropArgs d, hipStream_t s) {
    if (rows < 1 || T < 1 || !grid_ok((size_t)(rows + 3) / 4)) return hipErrorInvalidValue;
    LAUNCH(softmax_drop_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, P, dP, rows, T, d);
}
hipError_t tt_launch_dropout(const float* x, float* y, size_t n, DropArgs d, hipStream_t s) {
    if (!grid_ok((n + 255) / 256)) return hipErrorInvalidValue;
    LAUNCH(dropout_kernel, dim3(blocks256(n)), dim3(256), 0, s, x, y, n, d);
}
hipError_t tt_launch_dropout_mask(uint8_t* out, size_t n, DropArgs d, hipStream_t s) {
    if (!grid_ok((n + 255) / 256)) return hipErrorInvalidValue;
    LAUNCH(dropout_mask_kernel, dim3(blocks256(n)), dim3(256), 0, s, out, n, d);
}
hipError_t tt_launch_relu_bwd(const float* y, const float* dy, float* dx, size_t n, hipStream_t s) {
    if (!grid_ok((n + 255) / 256)) return hipErrorInvalidValue;
    LAUNCH(relu_bwd_kernel, dim3(blocks256(n)), dim3(256), 0, s, y, dy, dx, n);
}
hipError_t tt_launch_add(const float* a, const float* b, float* y, size_t n, hipStream_t s) {
    if (!grid_ok((n + 255) / 256)) return hipErrorInvalidValue;
    LAUNCH(tt_add_kernel, dim3(blocks256(n)), dim3(256), 0, s, a, b, y, n);
}
hipError_t tt_launch_mask(const float* x, const uint8_t* valid, float* y, size_t n, hipStream_t s) {
    if (!grid_ok((n + 255) / 256)) return hipErrorInvalidValue;
    LAUNCH(tt_mask_kernel, dim3(blocks256(n)), dim3(256), 0, s, x, valid, y, n);
}
hipError_t tt_launch_embed(const int64_t* phones, const float* tok_emb, const float* pe_row, float* x, long rows, int D, int vocab, hipStream_t s) {
    if (rows < 1 || D < 1 || !grid_ok(((size_t)rows * D + 255) / 256)) return hipErrorInvalidValue;
    LAUNCH(tt_embed_kernel, dim3(blocks256((size_t)rows * D)), dim3(256), 0, s, phones, tok_emb, pe_row, x, rows, D, vocab);
}
hipError_t tt_launch_add_speaker(const float* x, const int64_t* speaker, const float* tab, float* y, int B, int S, int D, int n_speaker, hipStream_t s) {
    const size_t n = (size_t)B * S * D;
    if (B < 1 || S < 1 || D < 1 || !grid_ok((n + 255) / 256)) return hipErrorInvalidValue;
    LAUNCH(tt_add_speaker_kernel, dim3(blocks256(n)), dim3(256), 0, s, x, speaker, tab, y, S, D, n_speaker, n);
}
hipError_t tt_launch_dur_cum(const int64_t* dur, int32_t* cum, int B, int S, int L, hipStream_t s) {
    if (B < 1 || S < 1 || L < 1) return hipErrorInvalidValue;
    LAUNCH(dur_cum_kernel, dim3((B + 63) / 64), dim3(64), 0, s, dur, cum, B, S, L);
}
hipError_t tt_launch_lr_fwd(const float* enc, const int32_t* cum, const float* pe_row, float* y, int B, int S, int L, int D, hipStream_t s) {
    if (B < 1 || B > 65535 || S < 1 || L < 1 || D < 1) return hipErrorInvalidValue;
    LAUNCH(lr_fwd_kernel, dim3(L, B), dim3(256), 0, s, enc, cum, pe_row, y, S, L, D);
}
hipError_t tt_launch_lr_bwd(const float* dy, const int32_t* cum, const float* add, float* denc, int B, int S, int L, int D, hipStream_t s) {
    if (B < 1 || B > 65535 || S < 1 || L < 1 || D < 1) return hipErrorInvalidValue;
    LAUNCH(lr_bwd_kernel, dim3(S, B), dim3(256), 0, s, dy, cum, add, denc, S, L, D);
}
hipError_t tt_launch_embed_grad(const int64_t* ids, const float* dx, float* dtab, long rows, int per, int D, int V, int pad_idx, hipStream_t s) {
    if (rows < 1 || per < 1 || D < 1 || V < 1 || (D + 255) / 256 > 65535) return hipErrorInvalidValue;
    LAUNCH(embed_grad_kernel, dim3(V, (D + 255) / 256), dim3(256), 0, s, ids, dx, dtab, rows, per, D, pad_idx);
}

}  // namespace parrot
