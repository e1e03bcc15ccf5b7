/*
 * parrot_hip_debug.h -- test, profiling and probe entry points of libparrot_hip.so.  NOT part of the interface a user switching
 * from the reference needs (that is parrot_hip.h); bench.py, the tests and the tools under tools/ bind these.
 */
#ifndef PARROT_HIP_DEBUG_H
#define PARROT_HIP_DEBUG_H

#include "parrot_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Runs the MFMA fragment-layout probe on the current device (0 = layouts as assumed). */
int parrot_selftest(void* stream);
/* Rows of the per-kernel timing table (tile configurations of the exact-fp32 kernel; the other kernel rows follow). */
int parrot_conv_num_tile_cfgs(void);

/* dst[i] = src[i], 4 bytes per lane: known-byte-count kernel for calibrating the HBM PMC counters. */
/* Process-wide DEFAULTS for handles created afterwards (tests and benches that build several handles under different modes in one
 * process; a product passes the mode per handle to *_create_ex).  Read once by every *_create; a live handle never changes. */
int parrot_set_default_precision(int32_t prec);
/* Fused ResBlock kernels (csrc/resblock_split.h, resblock_fused.h): 0 off (layer by layer), 1 every eligible stage,
 * 2 (default; env PARROT_FUSED) all but the exact-fp32 32-channel kernel.  Default for handles created afterwards. */
int parrot_set_fused_resblocks(int32_t mode);
/* FFT blocks project twice on each side of the attention core (quirk Q3, modules/fft.py:48-57: qkv then MHA in_proj; MHA
 * out_proj then wo; all bias-free).  1 (default; env PARROT_TTE_MERGE): each pair is evaluated as its fp64-formed product, one
 * launch; 0: one after the other as the reference does.  Default for handles created afterwards. */
int parrot_set_tte_merge(int32_t on);
int parrot_debug_copy(const float* src, float* dst, size_t n, void* stream);
/* Measurement aid (bench.py `roofline.ceiling_probe_tflops`): the rate a bare fp16 MFMA stream sustains on this device under
 * its power limit -- shape 0 = v_mfma_f32_32x32x16_f16, 1 = v_mfma_f32_16x16x32_f16; random operands (constant_data = 0) or one
 * constant (1); two waves per SIMD, ~20-40 ms.  Synchronises the device.  TFLOP/s of 16-bit MFMA work in *tflops_out. */
int parrot_debug_mfma_ceiling(int32_t shape, int32_t constant_data, double* tflops_out);
/* Per-launch timing of the conv kernels (HIP events on the launch stream, aggregated per kernel row: bench.py's roofline
 * object).  parrot_prof_begin times every launch; parrot_prof_begin_row only the launches of one row (the dominant kernel):
 * event records around every launch of a step are themselves 3 % of a B = 64 step and 20 % of a single-utterance one.
 * parrot_prof_end: out[4 row + {0,1,2,3}] = {launches, total ms, algorithmic flops, algorithmic bytes}. */
int parrot_prof_begin(void);
int parrot_prof_begin_row(int32_t row);
int parrot_prof_end(double* out, int32_t n_cfg);

/* Debug aid: headroom to the fp16 split scheme's range.  While dst_dev != NULL every conv launched by parrot_voc_forward records
 * max |input element| into dst_dev[group] (device floats, atomic max; the caller zeroes them): group 0 = conv_pre, 1 + i = the
 * layers of stage i (ups_i, its ResBlock convs), n_stages + 1 = conv_post.  Fused ResBlock launches only see their block's input:
 * create the handle with fused_resblocks = 0 to cover every layer.  NULL switches it off. */
int parrot_voc_debug_absmax(parrot_voc_t*, float* dst_dev);
/* Tests / error localisation: while set, the next encode / decode calls copy the channel-first (B, D, T) activation
 * after each stage to the given DEVICE buffers (NULL entries are skipped): enc_ptrs[0] = embedding + pe[S],
 * enc_ptrs[1 + n] = encoder block n, enc_ptrs[1 + enc_layers] = encoder output (+ speaker); dec_ptrs[0] = length
 * regulator output + pe[L], dec_ptrs[1 + n] = decoder block n.  Pass NULL, NULL to switch it off. */
int parrot_tte_debug_stages(parrot_tte_t*, float* const* enc_ptrs, float* const* dec_ptrs);
/* Tests: the TTE's attention cores and its LayerNorm on their own, through the very launchers the FFT block calls (csrc/attn.h, tte_glue.h).
 * parrot_debug_attention: ctx (B, H hd, T) = softmax(q k^T sqrt(1 / hd) + key mask) v per (batch, head) of the channel-first
 * projections qkv (B, 3, H hd, T); valid (B, T) u8, non-zero = attend to this key (a row without a valid key: NaN throughout, as
 * torch).  core: 0 the three-kernel path (batched GEMM, masked softmax, batched GEMM over a (B, H, T, T) score tensor in ws; any
 * hd and T), 1 the fused core (hd = 128 and T <= 256), 2 the flash core on the fp16 split pipe (hd in {16, 32, 64, 128}, any T).
 * A core that does not take the shape: PARROT_E_UNSUPPORTED.  ws: parrot_debug_attention_workspace_bytes (never 0 for valid sizes).
 * parrot_debug_layernorm: y = LayerNorm over the channels of x (B, C, T) (of relu(x) when relu_in), eps 1e-5, affine (C). */
size_t parrot_debug_attention_workspace_bytes(int32_t B, int32_t T, int32_t H, int32_t core);
int parrot_debug_attention(const float* qkv, const uint8_t* valid, float* ctx, int32_t B, int32_t T, int32_t H, int32_t hd, int32_t core,
                           void* ws, size_t ws_bytes, void* stream);
int parrot_debug_layernorm(const float* x, const float* gamma, const float* beta, float* y, int32_t B, int32_t C, int32_t T,
                           int32_t relu_in, void* stream);
/* Tests: the TTE's duration, length-regulator and argmax / tie-guard kernels on their own, through the launchers the model calls
 * (csrc/tte_glue.h), on caller-owned DEVICE buffers.  `status` (one device int, never NULL) takes the place of the handle's status
 * word: 5 a non-finite log-duration of a real token or a non-finite logit, 6 a negative duration, 7 a duration at s >= src_len.
 * Null or empty arguments: PARROT_E_INVALID; more than 65535 rows or a dimension beyond PARROT_DEBUG_MAX_DIM: PARROT_E_UNSUPPORTED;
 * all before any launch.
 * parrot_debug_durations: duration_kernel -- log_dur (B, S) = ld_raw where the token is real (src_valid (B, S) u8 non-zero, or --
 *   src_len (B) given -- s < src_len[b]) and 0 elsewhere; dur i64 = max(rint(exp(log_dur) - 1), 0); cum (B, S) i32 its inclusive
 *   prefix sums and out_len (B) the row sums, both saturated at INT32_MAX.
 * parrot_debug_length_regulate: dur_prefix_kernel, then length_regulate_kernel, no transposes -- enc (B, D, S) channel-first,
 *   dur (B, S) i64, src_len nullable, pe (P, D); y (B, D, L) = pe[L] (row_exact: pe[min(len_b, L)]) + the expanded rows;
 *   tgt_mask (B, L) u8 nullable: t <= len_b (row_exact: t < max(len_b, 1)).  L <= 0: PARROT_E_INVALID; L >= P: PARROT_E_RANGE.
 * parrot_debug_argmax_guard: argmax_cf_kernel on logits (B, V, L) -> ids (B, L) i64, and with guard > 0 the tie guard: glist
 *   (2 x 256 ints, (row0 + b, t) pairs), gstat (4 ints: positions guarded, ids changed, smallest margin as float bits, first list
 *   entry of this row group).  gstat_start (4 HOST ints, nullable) is what gstat holds before the launch -- a test's second row
 *   group of a decoder lane: [0] entries already listed, [3] = where this group's start; NULL: {0, 0, +inf, 0}.  guard = 0:
 *   glist / gstat are not touched.  x (B, D, L) non-NULL: tie_guard_refine_kernel follows -- hwt (D, V), hb (V) nullable, and the
 *   deep form when f (B, F, L) is given: h (B, D, L), w2t (F, D), b2 (D) nullable; gref (256, V) takes the refined logits. */
#define PARROT_DEBUG_MAX_DIM (1 << 20)
int parrot_debug_durations(const float* ld_raw, const uint8_t* src_valid, const int32_t* src_len, int32_t B, int32_t S, float* log_dur,
                           int64_t* dur, int32_t* cum, int32_t* out_len, int32_t* status, void* stream);
int parrot_debug_length_regulate(const float* enc, const int64_t* dur, const int32_t* src_len, const float* pe, int32_t B, int32_t S,
                                 int32_t D, int32_t L, int32_t P, int32_t row_exact, float* y, uint8_t* tgt_mask, int32_t* cum,
                                 int32_t* out_len, int32_t* status, void* stream);
int parrot_debug_argmax_guard(const float* logits, int32_t B, int32_t V, int32_t L, float guard, int32_t row0, const float* x, int32_t D,
                              const float* hwt, const float* hb, const float* f, const float* h, const float* w2t, const float* b2,
                              int32_t F, const int32_t* gstat_start, int64_t* ids, int32_t* glist, int32_t* gstat, float* gref,
                              int32_t* status, void* stream);
/* Stage taps of the aligner: while set, every parrot_aligner_forward copies the activation after the third BatchNorm, channel-first
 * (B, conv_dim, T), to bn3_dev and the LSTM output (B, T, 2 lstm_dim) to lstm_dev (DEVICE buffers; NULL entries are skipped). */
int parrot_aligner_debug_stages(parrot_aligner_t*, float* bn3_dev, float* lstm_dev);
/* Tests: the aligner's training kernels (csrc/train_gemm.h, csrc/aligner_train.h) on their own, through the launch code of parrot_aligner_train_forward /
 * _backward (csrc/host_aligner_train.hip), on caller-owned DEVICE buffers.  Each descriptor mirrors the kernel's parameter struct;
 * every buffer it names is a parrot_debug_buf: the pointer and the number of floats behind it.  Before any launch the entry point
 * computes on the host the smallest and largest element index the strides, offsets, shifts and sizes can reach in every buffer:
 * a null or empty argument, a size < 1, a reach below 0 or at / beyond the count, or a workspace that is too small:
 * PARROT_E_INVALID; more than PARROT_DEBUG_MAX_TAPS taps, or a grid beyond what the launchers take: PARROT_E_UNSUPPORTED.
 * parrot_debug_tap_gemm: C[z][m][n] = act(sum_j sum_k A_j[m][k] X[z][k][n + shift_j] + bias0[m] + bias1[m]), z < Z; X is zero outside
 *   0 <= n + shift_j < N; element (m, k) of tap j at A[j].p + m a_sm + k a_sk, X[z][k][n] at X.p + x_off[j] + z x_sz + k x_sk + n x_sn,
 *   C[z][m][n] at C.p + z c_sz + m c_sm + n c_sn; bias0 nullable, bias1 only beside bias0.  Elements of C the strides do not address
 *   are not written.
 * parrot_debug_wgrad: out[m o_sm + k o_sk + j o_sj] = sum over b < R / T, t < T of dY[b][m][t] X[b][k][t + shift_j] (X zero outside
 *   0 <= t + shift_j < T; R a multiple of T): fp32 partials per 256 (b, t) pairs, added in fp64 and rounded once.  ws:
 *   parrot_debug_wgrad_workspace_bytes(R, ntaps, M, K) (0 for sizes that are not valid).
 * parrot_debug_colsum: out0[m] (and out1[m], nullable) = sum_r src[r ld + m], r < R, m < M, in fp64, rounded once.  ws:
 *   parrot_debug_colsum_workspace_bytes(R, M).
 * parrot_debug_bn_train / parrot_debug_bn_relu_bwd: BatchNorm1d over (B, C, T) on batch statistics (training; B T >= 2) or the
 *   running ones, and its backward fused with the ReLU's (x is the ReLU's output; dx may be dy; dgamma / dbeta nullable). */
#define PARROT_DEBUG_MAX_TAPS 5
typedef struct parrot_debug_buf {
    float* p;
    int64_t n;
} parrot_debug_buf;
typedef struct parrot_debug_tap_gemm_desc {
    parrot_debug_buf A[PARROT_DEBUG_MAX_TAPS];
    int64_t x_off[PARROT_DEBUG_MAX_TAPS];
    int32_t shift[PARROT_DEBUG_MAX_TAPS];
    int32_t ntaps;
    parrot_debug_buf X, C, bias0, bias1;
    int32_t M, N, K, Z;
    int64_t a_sm, a_sk, x_sz, x_sk, x_sn, c_sz, c_sm, c_sn;
    int32_t relu;
} parrot_debug_tap_gemm_desc;
typedef struct parrot_debug_wgrad_desc {
    parrot_debug_buf dY, X, out;
    int32_t M, K, T, R, ntaps;
    int32_t shift[PARROT_DEBUG_MAX_TAPS];
    int64_t y_sz, y_sm, y_st, x_sz, x_sk, x_st, o_sm, o_sk, o_sj;
} parrot_debug_wgrad_desc;
typedef struct parrot_debug_colsum_desc {
    parrot_debug_buf src, out0, out1;
    int32_t R, M;
    int64_t ld;
} parrot_debug_colsum_desc;
typedef struct parrot_debug_bn_train_desc {
    parrot_debug_buf x, y, gamma, beta, run_mean, run_var, mean, invstd;
    int32_t B, C, T, training;
    float eps;
} parrot_debug_bn_train_desc;
typedef struct parrot_debug_bn_bwd_desc {
    parrot_debug_buf dy, x, dx, gamma, mean, invstd, dgamma, dbeta;
    int32_t B, C, T;
} parrot_debug_bn_bwd_desc;
int parrot_debug_tap_gemm(const parrot_debug_tap_gemm_desc* d, void* stream);
size_t parrot_debug_wgrad_workspace_bytes(int32_t R, int32_t ntaps, int32_t M, int32_t K);
int parrot_debug_wgrad(const parrot_debug_wgrad_desc* d, void* ws, size_t ws_bytes, void* stream);
size_t parrot_debug_colsum_workspace_bytes(int32_t R, int32_t M);
int parrot_debug_colsum(const parrot_debug_colsum_desc* d, void* ws, size_t ws_bytes, void* stream);
int parrot_debug_bn_train(const parrot_debug_bn_train_desc* d, void* stream);
int parrot_debug_bn_relu_bwd(const parrot_debug_bn_bwd_desc* d, void* stream);
/* Tests: the aligner's bidirectional LSTM recurrence on its own, through the step loop parrot_aligner_forward runs (kernel 0:
 * lstm_step_kernel, csrc/aligner.h) or the one parrot_aligner_train_forward runs (kernel 1: lstm_train_step_kernel,
 * csrc/aligner_train.h), on caller-owned DEVICE buffers.  w_hh [2][4H][H] (forward, backward direction; gates i, f, g, o), xproj
 * (B, T, 8H) = W_ih x + b_ih + b_hh of both directions, h0 / c0 [2][B][H] the state before step 0 (both NULL: zeros).  Steps
 * 0 .. n_steps - 1 only: the forward direction writes frames 0 .. n_steps - 1 of out (B, T, 2H) [forward, backward], the backward
 * direction frames T - 1 .. T - n_steps; every other element of out (and of gates / c_all) is left as the caller gave it.  h_n / c_n
 * [2][B][H]: the state after the last step.  gates (B, T, 8H): sigmoid(i), sigmoid(f), tanh(g), sigmoid(o) per direction, and c_all
 * (B, T, 2H): kernel 1 only (kernel 0: both NULL).  ws: parrot_debug_lstm_workspace_bytes (0 for sizes that are not valid).
 * Before any launch: a null argument, h0 without c0, B, T or H < 1, n_steps outside [1, T], a kernel other than 0 / 1, gates / c_all
 * that do not match the kernel: PARROT_E_INVALID; H not a multiple of 16 or > 1024, B > 65535, T > 32768, a workspace that is too
 * small: PARROT_E_UNSUPPORTED. */
size_t parrot_debug_lstm_workspace_bytes(int32_t B, int32_t T, int32_t H, int32_t kernel);
int parrot_debug_lstm(const float* w_hh, const float* xproj, const float* h0, const float* c0, int32_t B, int32_t T, int32_t H,
                      int32_t n_steps, int32_t kernel, float* out, float* h_n, float* c_n, float* gates, float* c_all, void* ws,
                      size_t ws_bytes, void* stream);
/* Tests: the dropout mask parrot_tte_train_forward / _backward apply at `site` under (seed, offset) with probability p (the rule:
 * parrot_hip.h), elements 0 .. n - 1: out_u8[i] = 1 kept, 0 dropped (DEVICE, n bytes).  site in [0, 255], 0 <= p <= 1. */
int parrot_tte_train_dropout_mask(uint64_t seed, uint64_t offset, int32_t site, int64_t n, float p, uint8_t* out_u8, void* stream);
/* Tests: the TTE's training kernels (csrc/tte_train.h) alone, on caller-owned dense DEVICE buffers whose sizes follow from the
 * dimensions given; dropout arguments as parrot_tte_train_dropout_mask's.  A null argument or a size below 1: PARROT_E_INVALID.
 *   ln_fwd            x (rows, C) -> y, mean (rows), rstd (rows)
 *   ln_bwd            dx (rows, C) = LayerNorm's data gradient of dy + res (nullable), 0 where relu_mask and x <= 0; dyxh = dy xhat
 *   softmax_drop_fwd  scores (B, H, T, T) -> P in place under key_valid (B, T); pd (nullable): P after dropout
 *   softmax_drop_bwd  dP (B, H, T, T), the gradient at the dropped probabilities, -> dS in place
 *   dropout           y[i] = keep(i) ? x[i] / (1 - p) : 0, i < n; p = 0 copies
 *   lr_bwd            denc (B, S, D) = the segment sums of dy (B, L, D) under dur (B, S) i64 (+ add, nullable); cum: (B, S + 1) i32 scratch
 *   embed_grad        dtab (V, D) = sum over rows r with ids[r / per] == v of dx (rows, D); row pad_idx (if >= 0) exactly 0
 *   conv_dw           dW (cout, cin, kk) of conv1d(X (B, T, cin), W, padding = pad) from dY (B, T, cout), reduced `group` taps at a
 *                     time (1 <= group <= kk <= 9): group < kk is the path a weight gradient takes when its partials exceed the
 *                     workspace bound.  ws: parrot_debug_tte_conv_dw_workspace_bytes (0 for sizes that are not valid). */
int parrot_debug_tte_ln_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int64_t rows, int32_t C,
                            void* stream);
int parrot_debug_tte_ln_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd, const float* res, float* dx,
                            float* dyxh, int64_t rows, int32_t C, int32_t relu_mask, void* stream);
int parrot_debug_tte_softmax_drop_fwd(float* scores, float* pd, const uint8_t* key_valid, int32_t B, int32_t H, int32_t T, float p, uint64_t seed,
                                      uint64_t offset, int32_t site, void* stream);
int parrot_debug_tte_softmax_drop_bwd(const float* P, float* dP, int32_t B, int32_t H, int32_t T, float p, uint64_t seed, uint64_t offset,
                                      int32_t site, void* stream);
int parrot_debug_tte_dropout(const float* x, float* y, int64_t n, float p, uint64_t seed, uint64_t offset, int32_t site, void* stream);
int parrot_debug_tte_lr_bwd(const float* dy, const int64_t* dur, const float* add, float* denc, int32_t* cum, int32_t B, int32_t S, int32_t L,
                            int32_t D, void* stream);
int parrot_debug_tte_embed_grad(const int64_t* ids, const float* dx, float* dtab, int64_t rows, int32_t per, int32_t D, int32_t V, int32_t pad_idx,
                                void* stream);
size_t parrot_debug_tte_conv_dw_workspace_bytes(int32_t cout, int32_t cin, int32_t kk, int32_t B, int32_t T, int32_t group);
int parrot_debug_tte_conv_dw(const float* dY, const float* X, float* dW, int32_t cout, int32_t cin, int32_t kk, int32_t pad, int32_t B, int32_t T,
                             int32_t group, void* ws, size_t ws_bytes, void* stream);
/* Tests: the leaky-ReLU sites of parrot_voc_train_forward / _backward, numbered in the reference's execution order: per stage the one
 * before ups[i], then per resblock and dilation the one before convs1[m] and the one before convs2[m] (ResBlock2: the one before
 * convs[m]); last the one before conv_post.  5 + 5 x 3 x 6 + 1 = 96 for the shipped config.
 *   lrelu_sites       their number (0 beyond the limits)
 *   lrelu_site_elems  the elements B C T of site `site` (0 beyond the limits)
 *   lrelu_mask        out_u8[i] = 1 where the backward passes the gradient through (x > 0), 0 where it multiplies by the slope, read
 *                     from the `saved` buffer of a forward at (cfg, B, U): the counterpart of parrot_tte_train_dropout_mask. */
int32_t parrot_voc_train_lrelu_sites(const parrot_voc_cfg* cfg);
int64_t parrot_voc_train_lrelu_site_elems(const parrot_voc_cfg* cfg, int32_t B, int32_t U, int32_t site);
int parrot_voc_train_lrelu_mask(const parrot_voc_cfg* cfg, int32_t B, int32_t U, const void* saved, int32_t site, uint8_t* out_u8, void* stream);
/* Tests: the pieces of the vocoder's training alone (csrc/voc_train.h and the launches host_voc_train.hip makes of tap_gemm_kernel /
 * wgrad_kernel), on caller-owned dense DEVICE buffers whose sizes follow from the dimensions given.  A conv is described by
 * (c_in, c_out, k, dil, u, transposed): transposed == 0 is Conv1d(c_in, c_out, k, dilation = dil, padding = dil (k - 1) / 2) with
 * w (c_out, c_in, k) and T_out = T_in (u must be 1); transposed != 0 is ConvTranspose1d(c_in, c_out, k, u, padding = (k - u) / 2)
 * with w (c_in, c_out, k) and T_out = (T_in - 1) u - 2 ((k - u) / 2) + k (dil must be 1).
 *   conv_fwd   y (B, c_out, T_out) = conv(x (B, c_in, T_in)) + bias (nullable)
 *   conv_dx    dx (B, c_in, T_in) from dy (B, c_out, T_out)
 *   conv_dw    dw (w's shape) from dy and x; ws: parrot_debug_voc_conv_dw_workspace_bytes (0 for sizes that are not valid)
 *   wn_fwd     w (rows, len) = v (g / ||v||), norm (rows);  wn_bwd: dv (rows, len), dg (rows) from dw (either nullable)
 * A null argument, a size below 1, k > 11, an even k of a Conv1d, u > k: PARROT_E_INVALID, before any launch. */
int parrot_debug_voc_conv_fwd(const float* x, const float* w, const float* bias, float* y, int32_t B, int32_t c_in, int32_t c_out, int32_t k,
                              int32_t dil, int32_t u, int32_t transposed, int32_t T_in, void* stream);
int parrot_debug_voc_conv_dx(const float* dy, const float* w, float* dx, int32_t B, int32_t c_in, int32_t c_out, int32_t k, int32_t dil, int32_t u,
                             int32_t transposed, int32_t T_in, void* stream);
size_t parrot_debug_voc_conv_dw_workspace_bytes(int32_t B, int32_t c_in, int32_t c_out, int32_t k, int32_t T_in);
int parrot_debug_voc_conv_dw(const float* dy, const float* x, float* dw, int32_t B, int32_t c_in, int32_t c_out, int32_t k, int32_t dil, int32_t u,
                             int32_t transposed, int32_t T_in, void* ws, size_t ws_bytes, void* stream);
int parrot_debug_voc_wn_fwd(const float* v, const float* g, float* w, float* norm, int32_t rows, int32_t len, void* stream);
int parrot_debug_voc_wn_bwd(const float* dw, const float* v, const float* g, const float* norm, float* dv, float* dg, int32_t rows, int32_t len,
                            void* stream);
/* Tests: the pieces of the multi-period discriminator's training alone (csrc/mpd_train.h and the launches host_mpd_train.hip makes
 * of tap_gemm_kernel / wgrad_kernel), on caller-owned dense DEVICE buffers whose sizes follow from the dimensions given.
 *   conv_*   one conv over H on Z independent rows: x (Z, c_in, H_in), w (c_out, c_in, k), padding 2, stride `stride`,
 *            H_out = (H_in + 4 - k) / stride + 1.  fwd: y (Z, c_out, H_out) = conv + bias (nullable), then the leaky ReLU when act;
 *            dx (Z, c_in, H_in) = mask(pre + the data gradient of dy), pre and mask (Z, c_in, H_in) nullable; dw (w's shape); ws:
 *            parrot_debug_mpd_conv_dw_workspace_bytes (0 for sizes that are not valid)
 *   first_*  convs[0] fused with the reflect pad and the fold: wav (N, T), w (c1, k), y (N, period, c1, H_1); dx: d wav (N, T) from dy
 *            (y's shape); dw (c1, k); ws: parrot_debug_mpd_first_dw_workspace_bytes
 *   post_*   conv_post: x (Z, C, H), w (C, 3), y (Z, H); dx (Z, C, H) = mask(pre + w (x) dy); dw (C, 3); ws: ..._post_dw_workspace_bytes
 * A null argument, a size below 1, an even k or k > 11, stride > k, T <= n_pad: PARROT_E_INVALID, before any launch. */
int parrot_debug_mpd_conv_fwd(const float* x, const float* w, const float* bias, float* y, int32_t Z, int32_t c_in, int32_t c_out, int32_t k,
                              int32_t stride, int32_t H_in, int32_t act, float slope, void* stream);
int parrot_debug_mpd_conv_dx(const float* dy, const float* w, const float* pre, const float* mask, float slope, float* dx, int32_t Z, int32_t c_in,
                             int32_t c_out, int32_t k, int32_t stride, int32_t H_in, void* stream);
size_t parrot_debug_mpd_conv_dw_workspace_bytes(int32_t Z, int32_t c_in, int32_t c_out, int32_t k, int32_t stride, int32_t H_in);
int parrot_debug_mpd_conv_dw(const float* dy, const float* x, float* dw, int32_t Z, int32_t c_in, int32_t c_out, int32_t k, int32_t stride,
                             int32_t H_in, void* ws, size_t ws_bytes, void* stream);
int parrot_debug_mpd_first_fwd(const float* wav, const float* w, const float* bias, float* y, int32_t N, int32_t T, int32_t period, int32_t c1,
                               int32_t k, int32_t stride, float slope, void* stream);
int parrot_debug_mpd_first_dx(const float* dy, const float* w, float* dwav, int32_t N, int32_t T, int32_t period, int32_t c1, int32_t k,
                              int32_t stride, void* stream);
size_t parrot_debug_mpd_first_dw_workspace_bytes(int32_t N, int32_t T, int32_t period, int32_t c1, int32_t k, int32_t stride);
int parrot_debug_mpd_first_dw(const float* dy, const float* wav, float* dw, int32_t N, int32_t T, int32_t period, int32_t c1, int32_t k,
                              int32_t stride, void* ws, size_t ws_bytes, void* stream);
int parrot_debug_mpd_post_fwd(const float* x, const float* w, const float* bias, float* y, int32_t Z, int32_t C, int32_t H, void* stream);
int parrot_debug_mpd_post_dx(const float* dy, const float* w, const float* pre, const float* mask, float slope, float* dx, int32_t Z, int32_t C,
                             int32_t H, void* stream);
size_t parrot_debug_mpd_post_dw_workspace_bytes(int32_t Z, int32_t C, int32_t H);
int parrot_debug_mpd_post_dw(const float* dy, const float* x, float* dw, int32_t Z, int32_t C, int32_t H, void* ws, size_t ws_bytes, void* stream);
/* Tests: the pieces of the multi-scale discriminator's training alone (csrc/msd_train.h), on caller-owned dense DEVICE buffers.
 *   gconv_*  one grouped conv: x (Z, c_in, T_in), w (c_out, c_in / groups, k), padding (k - 1) / 2, stride <= 4, k odd <= 41,
 *            T_out = (T_in - 1) / stride + 1.  fwd: y (Z, c_out, T_out) = conv + bias (nullable), then the leaky ReLU when act;
 *            dx (Z, c_in, T_in) = mask(pre + the data gradient of dy), pre and mask nullable; dw (w's shape); ws:
 *            parrot_debug_msd_gconv_dw_workspace_bytes (0 for sizes that are not valid)
 *   first_*  convs[0]: wav (Z, T), w (c1, 15), y (Z, c1, T); dx: d wav (Z, T); dw (c1, 15); ws: ..._first_dw_workspace_bytes
 *   pool_*   AvgPool1d(4, 2, padding=2): x (Z, T) -> y (Z, T / 2 + 1); bwd: dx (Z, T) from dy (Z, T / 2 + 1)
 *   sn_fold  w (rows, cols); iterate: one power iteration on u (rows), v (cols) in place; sigma[0] = u^T (w v), wf = w / sigma;
 *            ws: (rows + cols) floats
 *   sn_bwd   dw = ga / sa - (<ga, w> / sa^2) ua va^T (+ the same of gb, ub, vb, sb when gb != NULL); sa, sb: one device float each;
 *            ws: parrot_debug_msd_sn_bwd_workspace_bytes
 * A null argument or a size outside the limits: PARROT_E_INVALID, before any launch. */
int parrot_debug_msd_gconv_fwd(const float* x, const float* w, const float* bias, float* y, int32_t Z, int32_t c_in, int32_t c_out, int32_t groups,
                               int32_t k, int32_t stride, int32_t T_in, int32_t act, float slope, void* stream);
int parrot_debug_msd_gconv_dx(const float* dy, const float* w, const float* pre, const float* mask, float slope, float* dx, int32_t Z, int32_t c_in,
                              int32_t c_out, int32_t groups, int32_t k, int32_t stride, int32_t T_in, void* stream);
size_t parrot_debug_msd_gconv_dw_workspace_bytes(int32_t Z, int32_t c_in, int32_t c_out, int32_t groups, int32_t k, int32_t stride, int32_t T_in);
int parrot_debug_msd_gconv_dw(const float* dy, const float* x, float* dw, int32_t Z, int32_t c_in, int32_t c_out, int32_t groups, int32_t k,
                              int32_t stride, int32_t T_in, void* ws, size_t ws_bytes, void* stream);
int parrot_debug_msd_first_fwd(const float* wav, const float* w, const float* bias, float* y, int32_t Z, int32_t T, int32_t c1, float slope,
                               void* stream);
int parrot_debug_msd_first_dx(const float* dy, const float* w, float* dwav, int32_t Z, int32_t T, int32_t c1, void* stream);
size_t parrot_debug_msd_first_dw_workspace_bytes(int32_t Z, int32_t T, int32_t c1);
int parrot_debug_msd_first_dw(const float* dy, const float* wav, float* dw, int32_t Z, int32_t T, int32_t c1, void* ws, size_t ws_bytes, void* stream);
int parrot_debug_msd_pool_fwd(const float* x, float* y, int32_t Z, int32_t T, void* stream);
int parrot_debug_msd_pool_bwd(const float* dy, float* dx, int32_t Z, int32_t T, void* stream);
int parrot_debug_msd_sn_fold(const float* w, float* u, float* v, int32_t rows, int32_t cols, int32_t iterate, float* wf, float* sigma, void* ws,
                             size_t ws_bytes, void* stream);
size_t parrot_debug_msd_sn_bwd_workspace_bytes(int32_t rows, int32_t cols);
int parrot_debug_msd_sn_bwd(const float* ga, const float* gb, const float* w, const float* ua, const float* va, const float* sa, const float* ub,
                            const float* vb, const float* sb, float* dw, int32_t rows, int32_t cols, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PARROT_HIP_DEBUG_H */
