/*
 * parrot_hip.h -- C ABI of libparrot_hip.so: the MI355X (gfx950) implementation of the
 * Parrot-TTS synthesis hot path (TTE -> length regulator -> HiFi-GAN unit vocoder).
 *
 * The reference (parrot-tts/Parrot-TTS) is pure Python on torch.nn and has no FFI of its own;
 * the seam this library plugs into is the nn.Module surface the reference drivers call.  Each
 * entry point below names the reference code it replaces (paths relative to the reference
 * repo).  The Python shims in parrot_tts_amd/ (tte.py, vocoder.py) bind these with ctypes --
 * see INTEGRATION.md.  Test / profiling / probe entry points live in parrot_hip_debug.h.
 *
 * Conventions
 *   - plain C types only; no torch / C++ types cross the boundary
 *   - return 0 on success, a negative PARROT_E_* code otherwise; parrot_last_error() gives a
 *     thread-local message; no C++ exception crosses the ABI
 *   - weights are HOST pointers (fp32, row-major, already weight-norm-folded): *_create packs them
 *     into MFMA fragment order and uploads them once; the handle owns that device copy
 *   - activations / ids / outputs are DEVICE pointers allocated by the caller (PyTorch's caching
 *     allocator); the library never allocates per call: callers pass a workspace sized by
 *     *_workspace_bytes().  All launches are asynchronous on the hipStream_t passed (as void*)
 *   - one process per GPU; a handle is bound to the device current at *_create
 */
#ifndef PARROT_HIP_H
#define PARROT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PARROT_ABI_VERSION 7  /* 7: parrot_voc_wait_stage */

enum {
    PARROT_OK = 0,
    PARROT_E_INVALID = -1,     /* bad argument / unsupported dimension                         */
    PARROT_E_RANGE = -2,       /* T >= max_len (reference: IndexError at modules/fft.py:18)    */
    PARROT_E_HIP = -3,         /* a HIP runtime call failed                                    */
    PARROT_E_NOMEM = -4,       /* workspace too small / allocation failed                      */
    PARROT_E_UNSUPPORTED = -5, /* configuration outside what the kernels cover                 */
    PARROT_E_NONFINITE = -6,   /* parrot_voc_check: a waveform sample was NaN / inf (fp16 split range exceeded) */
};

int parrot_abi_version(void);
const char* parrot_last_error(void);

/* ------------------------------------------------------------------------------------------
 * Single Conv1d / ConvTranspose1d plan: the dilated-Conv1d implicit-GEMM kernel behind every
 * torch.nn.Conv1d / ConvTranspose1d / Linear on the path
 *   (utils/vocoder/models.py:17-28,75,81-83,91; modules/fft.py:48-50,65-76; modules/duration.py:64-72).
 * y[b,o,t] = act(bias[o] + sum_{i,j} w[o,i,j] * pre(x[b,i,t + j*dil - pad])) (+ res[b,o,t])
 * ------------------------------------------------------------------------------------------ */
typedef struct parrot_conv parrot_conv_t;

typedef struct {
    int32_t c_in, c_out, k, dilation, padding; /* Conv1d: symmetric zero padding                 */
    int32_t transposed;                        /* 1: ConvTranspose1d, weight (c_in,c_out,k)      */
    int32_t stride;                            /* ConvTranspose1d stride (upsample rate); else 1 */
    int32_t pre_act;                           /* 0 none, 1 leaky_relu(pre_slope) on the input   */
    float pre_slope;
    int32_t act;                               /* 0 none, 1 relu, 2 tanh (applied to bias+sum)   */
    int32_t tile_cfg;                          /* -1 = auto; else index into the tile table      */
    int32_t precision;                         /* PARROT_PREC_*; -1 = library default            */
} parrot_conv_desc;

/* How the fp32 products of layers with >= 16 channels are evaluated.  Inputs, outputs, residual stream and accumulation
 * are fp32 in every mode (csrc/conv_split.h has the details).
 *   PARROT_PREC_F32    v_mfma_f32_32x32x2_f32: exact fp32 fma chain.
 *   PARROT_PREC_F16X3  (default) each operand split into 2 fp16 pieces (pre-scaled by powers of two), 3 fp16 MFMAs per
 *                      product group (dropped term <= 2^-22 of the product), fp32 accumulate: fp32-class error, held to
 *                      the same parity tolerances as PARROT_PREC_F32, at 16/3 the MFMA rate.  Activations must stay
 *                      below 8190 in magnitude (fp16 range after the 2^3 pre-scale): beyond that the output turns
 *                      into inf/NaN, never into a silently wrong finite value.
 *   PARROT_PREC_BF16X6 each operand split into 3 bf16 pieces, 6 bf16 MFMAs per product group (dropped terms <= 2^-23),
 *                      fp32's full exponent range; same tolerances, 16/6 the MFMA rate.
 *   PARROT_PREC_BF16 / PARROT_PREC_F16   operands rounded once to bf16 / fp16, ONE MFMA per product group, fp32
 *                      accumulate, fp32 residual stream: the reduced-precision operating point (BASELINE configs[2]
 *                      "bf16"); NOT parity-grade -- reported by SNR against the fp32 result (36 dB / 54 dB).
 * The process-wide default (PARROT_PRECISION env: "f32" | "f16x3" | "bf16x6" | "bf16" | "f16", else f16x3)
 * is read ONCE by every *_create: a handle keeps the mode it was created under and is immutable afterwards. */
#define PARROT_PREC_F32 0
#define PARROT_PREC_BF16X6 1
#define PARROT_PREC_F16X3 2
#define PARROT_PREC_BF16 3
#define PARROT_PREC_F16 4
/* (Per handle: parrot_voc_create_ex / parrot_tte_create_ex / parrot_conv_desc.precision.  The process-wide DEFAULTS -- precision,
 * fused ResBlock kernels (env PARROT_FUSED: 0 off, 1 every eligible stage, 2 default), merged TTE projections (env PARROT_TTE_MERGE) --
 * come from the environment; their setters are test / bench conveniences and live in parrot_hip_debug.h.) */

int parrot_conv_create(parrot_conv_t** out, const parrot_conv_desc* d, const float* w_host, const float* bias_host);
void parrot_conv_destroy(parrot_conv_t*);
/* epilogue: 0 store, 1 y += v, 2 y = (y + v) / div  (MRF sum, models.py:100-106) */
int parrot_conv_run(parrot_conv_t*, const float* x, const float* res, float* y, int32_t B, int32_t T_in,
                    int32_t epilogue, float div, void* stream);
int parrot_conv_out_len(const parrot_conv_t*, int32_t T_in);

/* ------------------------------------------------------------------------------------------
 * HiFi-GAN unit vocoder: CodeGenerator.forward (utils/vocoder/models.py:153-169) ->
 * Generator.forward (:95-111) with ResBlock1/2 (:31-38,:58-62).
 * ------------------------------------------------------------------------------------------ */
typedef struct parrot_voc parrot_voc_t;

#define PARROT_MAX_STAGES 8
#define PARROT_MAX_KERNELS 4
#define PARROT_MAX_DIL 4

typedef struct {
    int32_t num_embeddings, embedding_dim; /* h.num_embeddings, h.embedding_dim                 */
    int32_t multispkr, n_spkr;             /* bool(h.multispkr); spkr table rows (10)           */
    int32_t model_in_dim;                  /* conv_pre input channels                           */
    int32_t upsample_initial_channel;
    int32_t n_stages;
    int32_t upsample_rates[PARROT_MAX_STAGES];
    int32_t upsample_kernel_sizes[PARROT_MAX_STAGES];
    int32_t n_kernels;
    int32_t resblock_kernel_sizes[PARROT_MAX_KERNELS];
    int32_t n_dil;
    int32_t resblock_dilation_sizes[PARROT_MAX_KERNELS][PARROT_MAX_DIL];
    int32_t resblock_type;                 /* 1 = ResBlock1, 2 = ResBlock2 (h.resblock)         */
} parrot_voc_cfg;

/* Folded fp32 weights on the HOST, torch layouts.  resblock conv index:
 *   ResBlock1: [(stage*n_kernels + j)*2*n_dil + m*2 + {0: convs1[m], 1: convs2[m]}]
 *   ResBlock2: [(stage*n_kernels + j)*n_dil + m]                                              */
typedef struct {
    const float* dict;      /* (num_embeddings, embedding_dim)  */
    const float* spkr;      /* (n_spkr, embedding_dim) or NULL  */
    const float* conv_pre_w; const float* conv_pre_b;   /* (C0, model_in_dim, 7), (C0)          */
    const float* ups_w[PARROT_MAX_STAGES];               /* (C_in, C_in/2, k)                    */
    const float* ups_b[PARROT_MAX_STAGES];
    const float* const* rb_w;                            /* array of (C, C, k) pointers          */
    const float* const* rb_b;
    int32_t n_rb;
    const float* conv_post_w; const float* conv_post_b; /* (1, C_last, 7), (1)                  */
} parrot_voc_weights;

int parrot_voc_create(parrot_voc_t** out, const parrot_voc_cfg* cfg, const parrot_voc_weights* w);
/* The same with this handle's own precision (PARROT_PREC_*, -1 = the process default) and fused-ResBlock mode (0 / 1 / 2,
 * -1 = default): what the shims' range-safe fallback uses to rebuild a handle in PARROT_PREC_BF16X6 (fp32's range) after the
 * default fp16x3 scheme reported PARROT_E_NONFINITE -- reference checkpoints carry no range promise (utils/vocoder/models.py has
 * no normalisation layer), so |activation| < 8190 cannot be assumed of a real one. */
int parrot_voc_create_ex(parrot_voc_t** out, const parrot_voc_cfg* cfg, const parrot_voc_weights* w, int32_t precision,
                         int32_t fused_resblocks);
void parrot_voc_destroy(parrot_voc_t*);
/* PARROT_PREC_* this handle was created with (the "precision in use" after a fallback). */
int parrot_voc_precision(const parrot_voc_t*);
size_t parrot_voc_workspace_bytes(const parrot_voc_t*, int32_t B, int32_t U);
/* code (B,U) int64, spkr (B,1) int64 or NULL -> wav (B,1,U*prod(rates)) fp32 in (-1,1).
 * unit_lens: optional (B) int32 device array of real units per row (ragged batch padded to U): every layer applies its
 * zero padding at each row's own end, so row b[: unit_lens[b]*hop] equals the reference's B=1 run of that utterance
 * (the reference never batches the vocoder, utils/vocoder/inference.py:149); samples beyond are unspecified.  NULL = all U.
 * stage_out: optional array of 2*n_stages+1 device pointers (conv_pre, ups_i, mrf_i ...) that
 * receive copies of the intermediate activations (tests only); NULL in production.            */
int parrot_voc_forward(parrot_voc_t*, const int64_t* code, const int64_t* spkr, const int32_t* unit_lens, int32_t B, int32_t U,
                       float* wav_out, float* const* stage_out, void* ws, size_t ws_bytes, void* stream);
/* CodeGenerator.forward with extra conditioning keywords (utils/vocoder/models.py:162-167: every keyword tensor other
 * than code / spkr / f0 is upsampled to U frames and concatenated behind the embeddings).  `feats`: dense fp32
 * (B, n_feat_channels, U), the caller's streams already upsampled and concatenated in keyword order; it fills input
 * channels [embedding_dim * (1 + multispkr), model_in_dim).  NULL / 0 when the model has none. */
int parrot_voc_forward_feats(parrot_voc_t*, const int64_t* code, const int64_t* spkr, const float* feats, int32_t n_feat_channels,
                             const int32_t* unit_lens, int32_t B, int32_t U, float* wav_out, float* const* stage_out, void* ws,
                             size_t ws_bytes, void* stream);
/* Chunk-streamed synthesis (long-form utterances, BASELINE configs[4]): chunks of `chunk_units` units are vocoded with
 * `halo_units` units of real context on both sides (< 0: the generator's receptive field, parrot_voc_receptive_units: 21 units for the shipped config) and only
 * their own samples land in wav_out (B,1,U*hop): equal to parrot_voc_forward on the whole utterance to fp32 round-off, with
 * the activation memory of chunk_units + 2*halo_units units.  Not for models with extra conditioning streams. */
size_t parrot_voc_chunked_workspace_bytes(const parrot_voc_t*, int32_t B, int32_t chunk_units, int32_t halo_units);
int parrot_voc_forward_chunked(parrot_voc_t*, const int64_t* code, const int64_t* spkr, const int32_t* unit_lens, int32_t B, int32_t U,
                               int32_t chunk_units, int32_t halo_units, float* wav_out, void* ws, size_t ws_bytes, void* stream);
/* Synchronises `stream` and reports what the device flagged since the last check: PARROT_E_RANGE for a unit / speaker id
 * outside the embedding tables (the reference's IndexError), PARROT_E_NONFINITE when a waveform sample left [-1, 1] as NaN /
 * inf (an activation beyond the fp16 split scheme's range: never a silently wrong finite value). */
int parrot_voc_check(parrot_voc_t*, void* stream);
/* The same flag WITHOUT a synchronisation: copies its value (0 = ok, 1 / 2 bad unit / speaker id, 5 non-finite sample) to
 * dst_dev[0] (device memory) on `stream` and clears it -- for callers that fetch it with a device-to-host copy they do anyway. */
int parrot_voc_status_async(parrot_voc_t*, int32_t* dst_dev, void* stream);
/* ... and without clearing it: the shims look at it once, synchronously, after the FIRST forward of every handle (range-safe
 * fallback: 5 -> rebuild in PARROT_PREC_BF16X6 and re-run); any other value stays set for the regular reporting path. */
int parrot_voc_status_peek_async(parrot_voc_t*, int32_t* dst_dev, void* stream);
/* Make `stream` wait until the most recently enqueued (direct, non-graph) forward of this handle has reached MRF stage `stage`
 * (0 .. n_stages - 1): a caller that runs other work beside the forward -- SynthesisPipeline.submit: the next batch's TTE, reference
 * inference.py + utils/vocoder/inference.py back to back -- chooses which part of the forward it shares the chip with.  Before the
 * handle's first forward (and after a graph replay of a small shape) there is nothing to wait for: the call returns at once. */
int parrot_voc_wait_stage(parrot_voc_t*, int32_t stage, void* stream);
/* Receptive field of the generator in units, either side of an output frame, from the handle's configuration (interval
 * propagation through conv_post, the MRF stages, the transposed convs of reference utils/vocoder/models.py:80-83 and conv_pre):
 * 21 for the shipped config.  The default halo of parrot_voc_forward_chunked. */
int parrot_voc_receptive_units(const parrot_voc_t*);
/* Waveform samples of an utterance of U units: U * prod(upsample_rates) for the shipped configs; a stage with odd
 * upsample_kernel_size - upsample_rate adds one sample (ConvTranspose1d then yields T u + 1, models.py:80-83): wav_out of
 * parrot_voc_forward holds B rows of parrot_voc_out_len(U) samples, and a row of n units has parrot_voc_out_len(n) real ones. */
int64_t parrot_voc_out_len(const parrot_voc_t*, int32_t U);
/* wav (n) fp32 -> int16 as `(x*32768).astype('int16')` does (utils/vocoder/inference.py:71-73) */
int parrot_wav_to_int16(const float* wav, int16_t* out, size_t n, void* stream);

/* ------------------------------------------------------------------------------------------
 * TTE: Parrot.forward(inference=True) / Parrot.infer  (modules/parrot.py:90-120) with
 * FFTBlock (modules/fft.py:85-100), DurationPredictor + length_regulator (modules/duration.py),
 * get_mask_from_lengths (modules/data.py:8-20).
 * ------------------------------------------------------------------------------------------ */
typedef struct parrot_tte parrot_tte_t;

typedef struct {
    int32_t d_model, n_filter_ffn, ffn_k1, ffn_k2, max_len;
    int32_t enc_layers, enc_heads, dec_layers, dec_heads;
    int32_t dp_filter, dp_kernel;
    int32_t vocab, n_speaker /* 0/1 = no speaker_emb */, n_codes /* head width (hubert_codes) */;
} parrot_tte_cfg;

typedef struct {
    const float *qkv, *in_proj, *out_proj, *wo;                   /* (3D,D) (3D,D) (D,D) (D,D)  */
    const float *conv1_w, *conv1_b, *conv2_w, *conv2_b;           /* (F,D,k1) (F) (D,F,k2) (D)  */
    const float *attn_norm_w, *attn_norm_b, *conv_norm_w, *conv_norm_b;
} parrot_fft_weights;

typedef struct {
    const float* pe;         /* (max_len, D)  pos_emb.pe                                        */
    const float* tok_emb;    /* (vocab, D)                                                       */
    const float* speaker_emb;/* (n_speaker, D) or NULL                                           */
    const float *dp_conv0_w, *dp_conv0_b, *dp_ln0_w, *dp_ln0_b;
    const float *dp_conv1_w, *dp_conv1_b, *dp_ln1_w, *dp_ln1_b;
    const float *dp_proj_w, *dp_proj_b;
    const parrot_fft_weights* enc;  /* enc_layers entries */
    const parrot_fft_weights* dec;  /* dec_layers entries */
    const float *head_w, *head_b;   /* (n_codes, D), (n_codes) */
} parrot_tte_weights;

int parrot_tte_create(parrot_tte_t** out, const parrot_tte_cfg* cfg, const parrot_tte_weights* w);
/* The same with this handle's own precision (PARROT_PREC_*, -1 = default) and projection merge (0 / 1, -1 = default): the
 * range-safe fallback of the shims, and the merged-vs-unmerged rows of the parity report. */
int parrot_tte_create_ex(parrot_tte_t** out, const parrot_tte_cfg* cfg, const parrot_tte_weights* w, int32_t precision,
                         int32_t merge_projections);
void parrot_tte_destroy(parrot_tte_t*);
int parrot_tte_precision(const parrot_tte_t*);
/* `state` carries the encoder output + duration prefix sums from encode to decode (sized by B,S);
 * `ws` is scratch: encode needs workspace_bytes(B,S,0), decode workspace_bytes(B,S,L).         */
size_t parrot_tte_state_bytes(const parrot_tte_t*, int32_t B, int32_t S);
size_t parrot_tte_workspace_bytes(const parrot_tte_t*, int32_t B, int32_t S, int32_t L_max);
/* Phase 1 (parrot.py:94-102 up to the durations): phones (B,S) i64, src_mask (B,S) u8 1=valid,
 * speaker (B) i64 or NULL -> log_dur (B,S) f32, dur (B,S) i64, out_lens (B) i32 (sum of dur).
 * src_len: NULL = the reference's PADDED-BATCH semantics (Parrot.forward on the padded batch: pe[S] of the padded length,
 *   pad frames leak through the k = 9 / k = 3 convs -- quirk Q7: a row's result depends on the batch it is padded into).
 *   (B) i32 device = ROW-EXACT mode: row b holds src_len[b] real tokens (src_mask must be that prefix) and is evaluated as the
 *   reference evaluates that utterance ALONE (its drivers run batch_size = 1, inference.py:34): pe[src_len[b]] (fft.py:18), every
 *   conv zero-padded at the row's own end (fft.py:78-82, duration.py:64-72), keys beyond it masked.                          */
int parrot_tte_encode(parrot_tte_t*, const int64_t* phones, const uint8_t* src_mask, const int64_t* speaker,
                      const int32_t* src_len /* nullable */, int32_t B, int32_t S, float* log_dur, int64_t* dur, int32_t* out_lens,
                      void* state, size_t state_bytes, void* ws, size_t ws_bytes, void* stream);
/* Phase 2 (duration.py:6-24, parrot.py:106-108,115): needs L = max(out_lens) from the host
 * (the reference's own host sync, duration.py:10).  -> ids (B,L) i64 argmax, tgt_mask (B,L) u8
 * (ids <= len, quirk Q2), optional logits (B,L,n_codes) f32 (tests).
 * row_exact != 0 (after an encode with src_len): row b is decoded as its own B = 1 run -- pe[out_lens[b]] (parrot.py:106), convs
 * zero-padded and keys masked at out_lens[b]; tgt_mask[b] = t < max(out_lens[b], 1): the row's ids are ids[b, :out_lens[b]]
 * (alone, a row is the longest of its batch and emits exactly its length -- no extra frame).                                */
int parrot_tte_decode(parrot_tte_t*, int32_t B, int32_t S, int32_t L, int32_t row_exact,
                      int64_t* ids, uint8_t* tgt_mask, float* logits /* nullable */,
                      void* state, size_t state_bytes, void* ws, size_t ws_bytes, void* stream);
/* Teacher forcing: Parrot.forward(batch) with inference=False (modules/parrot.py:90-110) feeds the CALLER's durations to the length
 * regulator (forward_duration(..., tgt_mask, dur_target), parrot.py:77-87; length_regulator(..., tgt_mask), duration.py:6-24) and
 * decodes under the caller's target mask.  Call parrot_tte_set_durations between parrot_tte_encode and parrot_tte_decode_masked.
 * dur (B,S) i64 device replaces the predicted durations in `state` (its prefix sums and out_len, rebuilt as the encode builds them);
 * every position counts, padded ones included (repeat_interleave expands what it is given, duration.py:13-14); out_lens (B) i32
 * device <- the per-row sums (L = their max, read by the caller with the transfer it makes anyway).  A negative duration sets device
 * status 6 (torch: "repeats can not be negative"); src_len: the row-exact encode's (B) i32 (NULL after a padded-batch encode) -- a
 * nonzero duration at s >= src_len[b] sets status 7 (a row alone has no such token).  Both are reported by
 * parrot_tte_status_async / parrot_tte_check, not by the return value. */
int parrot_tte_set_durations(parrot_tte_t*, const int64_t* dur, int32_t B, int32_t S, const int32_t* src_len /* nullable */,
                             int32_t* out_lens, void* state, size_t state_bytes, void* stream);
/* parrot_tte_decode with the caller's key mask (parrot.py:107: forward_decoder(out, ~tgt_mask)): key_mask (B,L) u8, 1 = attend, read
 * only, is the attention mask of every decoder block; no tgt_mask is written.  Padded mode: pe[L] (parrot.py:106), pad frames leak
 * through the k = 9 conv as in parrot_tte_decode (quirk Q7).  row_exact != 0 (after a row-exact encode): as parrot_tte_decode's
 * row-exact mode -- pe[out_lens[b]], convs zero-padded at out_lens[b] -- with key_mask the row's own (t < max(out_lens[b], 1)).
 * ids (B,L) i64 argmax with the tie guard, optional logits (B,L,n_codes) f32, workspace_bytes(B,S,L). */
int parrot_tte_decode_masked(parrot_tte_t*, int32_t B, int32_t S, int32_t L, int32_t row_exact, const uint8_t* key_mask,
                             int64_t* ids, float* logits /* nullable */, void* state, size_t state_bytes, void* ws, size_t ws_bytes,
                             void* stream);
/* ModelLoss.forward (modules/loss.py:5-21): CrossEntropyLoss(ignore_index = hubert_codes) of logits (N,V) f32 channel-last (the
 * layout Parrot.forward returns, reshaped (-1, V), loss.py:16) against targets (N) i64, plus MSELoss of log_dur (n_src) f32 against
 * log(dur + 1) (dur (n_src) i64) over src_mask (n_src) u8 (loss.py:13-14,17).  Per position a max-shifted log-sum-exp in fp32 and the
 * first-max argmax; sums in fp64, fixed order, no value atomics: two calls agree bit for bit.  All pointers device.
 * out (8 doubles) <- {sum nll, n_valid, n_correct (argmax == target), sum sq, n_src valid, n_bad, first bad target, 0}: a target
 * outside [0, V) other than ignore_index counts in n_bad (torch: IndexError "Target ... is out of bounds."); losses (3 floats,
 * nullable) <- {code + dur, code = sum nll / n_valid, dur = sum sq / n_src} in fp32 (NaN for an all-ignored batch / an empty
 * src_mask, as torch).  ws: parrot_tte_loss_workspace_bytes(N). */
size_t parrot_tte_loss_workspace_bytes(int32_t N);
int parrot_tte_loss(const float* logits, const int64_t* targets, int32_t N, int32_t V, int64_t ignore_index, const float* log_dur,
                    const int64_t* dur, const uint8_t* src_mask, int32_t n_src, double* out, float* losses /* nullable */, void* ws,
                    size_t ws_bytes, void* stream);
/* ModelLoss with its gradient (modules/loss.py:5-21; train.py:72-85: the loss training_step returns and Lightning's
 * loss.backward()), in one stateless call that runs the forward itself.  out and losses are parrot_tte_loss's for the same inputs,
 * bit for bit.  weights: DEVICE pointer to {w_code, w_dur} doubles, the gradients arriving at code_loss and dur_loss (a backward
 * needs no host synchronisation); NULL = {1, 1}, the gradient of losses[0].
 *   grad_logits (N,V) f32   <- (w_code / n_valid) (softmax(logits[n]) - onehot(targets[n])); a row with targets[n] == ignore_index is
 *                              exactly 0; a row whose target is outside [0, V) otherwise is NaN (it counts in n_bad; nothing is
 *                              indexed through the value)
 *   grad_log_dur (n_src) f32 <- src_mask[i] ? (2 w_dur / n_src valid) (log_dur[i] - log(dur[i] + 1)) : 0
 * The two quotients are formed in fp64 and rounded to fp32 once.  An all-ignored batch / an empty src_mask: NaN losses (as
 * parrot_tte_loss) and all-zero gradients, as torch's autograd gives.  Either gradient may be NULL, not both; grad_logits must not
 * alias logits nor grad_log_dur log_dur (PARROT_E_INVALID).  Every output element is written exactly once; no floating-point
 * atomics: two calls agree bit for bit, and a row's gradient depends on that row, n_valid and w_code only.  For V % 4 == 0,
 * V <= 1024 and 16-byte aligned logits the logits are read from memory once.  ws: parrot_tte_loss_grad_workspace_bytes(N). */
size_t parrot_tte_loss_grad_workspace_bytes(int32_t N);
int parrot_tte_loss_grad(const float* logits, const int64_t* targets, int32_t N, int32_t V, int64_t ignore_index, const float* log_dur,
                         const int64_t* dur, const uint8_t* src_mask, int32_t n_src, const double* weights /* device, nullable */,
                         double* out, float* losses /* nullable */, float* grad_logits /* nullable */,
                         float* grad_log_dur /* nullable */, void* ws, size_t ws_bytes, void* stream);
/* Device-side flags.  Synchronises `stream`, clears the flag; returns 0, PARROT_E_RANGE (a bad phone / speaker id <-> the
 * reference's Embedding IndexError) or PARROT_E_NONFINITE (NaN / inf logits at some position of the last decode: an
 * activation beyond the fp16 split scheme's range -- the ids of that call are not to be trusted). */
int parrot_tte_check(parrot_tte_t*, void* stream);
/* Tie guard of the unit-id argmax (reference modules/parrot.py:115: torch.argmax over 1000 fp32 logits).  parrot_tte_decode
 * measures every position's top-2 margin; where it is below PARROT_TIE_GUARD (default 1e-4; 0 = off) the head is re-evaluated
 * for that position in fp64 (exact products of the fp32 weights and activations, no accumulation-order dependence) and the
 * argmax taken again.  dst_dev[0..2] <- {guarded positions of the last decode, ids the re-evaluation changed, its smallest
 * margin (float bits)}; no synchronisation.  What no implementation can do is follow the reference below ITS OWN noise: its
 * fp32 logits move by ~1.2e-5 with the CPU thread count (tests/test_oracle_golden.py), so an id with a smaller margin is not
 * determined by the reference itself. */
int parrot_tte_guard_stats_async(parrot_tte_t*, int32_t* dst_dev, void* stream);
/* The guard's re-evaluation starts one layer before the head when the last decoder block's conv2 is 1x1 (the shipped config): that
 * conv2 + bias + residual (modules/fft.py:81,99) are recomputed in fp64 from the block's own fp32 intermediates, then the head.
 * logits_dev (max_n x n_codes floats) / list_dev (2 max_n ints: (b, t) pairs) <- the refined logits of the guarded positions of
 * the last decode (first guard_stats[0], at most 256); device memory, no synchronisation.  Tests / parity reports. */
int parrot_tte_guard_logits(parrot_tte_t*, float* logits_dev, int32_t* list_dev, int32_t max_n, void* stream);
/* The same flag without a synchronisation (3 / 4 bad phone / speaker id, 5 non-finite logits): see parrot_voc_status_async. */
int parrot_tte_status_async(parrot_tte_t*, int32_t* dst_dev, void* stream);
int parrot_tte_status_peek_async(parrot_tte_t*, int32_t* dst_dev, void* stream);
/* length_regulator alone (modules/duration.py:6-24 + modules/data.py:8-20), on the kernel the decoder uses:
 * seq (B,S,D) f32 as the reference holds it, dur (B,S) i64 -> out (B,L,D) (rows repeat_interleave'd, zero right-padded),
 * mask (B,L) u8 = ids <= len (quirk Q2), out_lens (B) i32.  L = max over rows of sum(dur), computed by the caller like
 * duration.py:10; ws: 2*B*D*max(S,L) floats + B*S + B int32 (parrot_length_regulator_workspace_bytes). */
size_t parrot_length_regulator_workspace_bytes(int32_t B, int32_t S, int32_t D, int32_t L);
int parrot_length_regulator(const float* seq, const int64_t* dur, int32_t B, int32_t S, int32_t D, int32_t L, float* out,
                            uint8_t* mask, int32_t* out_lens, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Log-mel spectrogram and mel L1: the vocoder's validation metric (validation/mel_spec_error, utils/vocoder/train.py:198-227):
 * mel_spectrogram (utils/vocoder/dataset.py:43-69, center = False) and F.l1_loss of two such spectrograms (train.py:213).
 *   reflect-pad by (n_fft - hop) / 2 -> STFT with the caller's fp32 window (zero-padded, centred, to n_fft as torch.stft does)
 *   -> sqrt(re^2 + im^2 + 1e-9) -> basis @ spec -> log(clamp(., 1e-5)).
 * The framed DFT runs as a Conv1d (hop -> 2 (n_fft / 2 + 1) channels, ceil(n_fft / hop) taps) over a polyphase view of the padded
 * signal and the mel projection as a 1x1 conv, both on the parrot_conv kernels; their weights are formed in fp64 from the fp32
 * window and rounded once.  window_host[win] and basis_host[n_mels x (n_fft / 2 + 1)] (row-major) are HOST data of the caller:
 * the library never computes a window or a mel scale.
 * Precision: the parity-grade modes only -- PARROT_PREC_F16X3 (default), PARROT_PREC_BF16X6, PARROT_PREC_F32.  Under a process
 * default of PARROT_PREC_BF16 / PARROT_PREC_F16 a mel handle is built in PARROT_PREC_F16X3: the metric does not move with the
 * vocoder's operating point (asking parrot_mel_create_ex for one of the two is PARROT_E_UNSUPPORTED).  The fp16x3 range rule
 * applies to the spectral magnitudes (< 8190: a full-scale sine at n_fft = 1024 reaches 512).  PARROT_PREC_F32 sums the DFT in
 * up to 8 channel groups whose partial sums are added afterwards (one fp32 accumulator chain over n_fft products costs more
 * accuracy than the split schemes lose), each group with its own 2 (n_fft / 2 + 1) rows padded to whole 128-row tiles: its
 * spectrum workspace is up to 9 times that of the other two modes (n_fft 1024: 8 x 1152 rows against 1026).
 * ------------------------------------------------------------------------------------------ */
typedef struct parrot_mel parrot_mel_t;

typedef struct {
    int32_t n_fft, hop, win, n_mels; /* h.n_fft, h.hop_size, h.win_size, h.num_mels; 1 <= hop <= n_fft, win <= n_fft */
} parrot_mel_cfg;

int parrot_mel_create(parrot_mel_t** out, const parrot_mel_cfg* cfg, const float* window_host, const float* basis_host);
int parrot_mel_create_ex(parrot_mel_t** out, const parrot_mel_cfg* cfg, const float* window_host, const float* basis_host,
                         int32_t precision /* PARROT_PREC_F32 / BF16X6 / F16X3; -1 = default */);
void parrot_mel_destroy(parrot_mel_t*);
int parrot_mel_precision(const parrot_mel_t*);
/* frames of a row of n_samples samples: n_samples / hop */
int parrot_mel_frames(const parrot_mel_t*, int32_t n_samples);
size_t parrot_mel_workspace_bytes(const parrot_mel_t*, int32_t B, int32_t N);
/* wav: B rows of N fp32 samples, row_stride elements apart -> mel_out (B, n_mels, N / hop) fp32.
 * n_samples: optional (B) int32 device array of real samples per row (ragged batch padded to N): the reflection happens at each
 * row's own end, row b yields n_samples[b] / hop frames that equal that utterance run alone bit for bit, samples beyond
 * n_samples[b] are never read, and the frames beyond are written as zero.  NULL = all N.
 * Reported by parrot_mel_check / parrot_mel_status_async, not by the return value: status 8, a row no longer than the reflect
 * pad (torch's F.pad raises); status 5, a non-finite mel value (NaN / inf input, or the fp16x3 range exceeded). */
int parrot_mel_forward(parrot_mel_t*, const float* wav, int64_t row_stride, const int32_t* n_samples /* nullable */, int32_t B, int32_t N,
                       float* mel_out, void* ws, size_t ws_bytes, void* stream);
/* sum |a - b| per row over n_mels x n_frames[b] (NULL: T) elements of two (B, n_mels, T) fp32 device tensors.  fp64 sums in a
 * fixed order, no value atomics: two calls agree bit for bit.  out_f64 (2B doubles) <- the row sums, then the row counts
 * n_mels * n_frames[b]; mean_f32 (1 float, nullable) <- sum of sums / sum of counts, rounded once to fp32 (F.l1_loss's mean
 * when the rows are of one length; NaN for an empty batch). */
size_t parrot_mel_l1_workspace_bytes(int32_t B, int32_t n_mels, int32_t T);
int parrot_mel_l1(const float* a, const float* b, const int32_t* n_frames /* nullable */, int32_t B, int32_t n_mels, int32_t T,
                  double* out_f64, float* mean_f32 /* nullable */, void* ws, size_t ws_bytes, void* stream);
/* The training loss of the generator (utils/vocoder/train.py:157, F.l1_loss(y_mel, y_g_hat_mel), before the factor 45) and its
 * gradient with respect to the waveform, in one stateless call that runs the forward itself:
 *   loss = reduce |parrot_mel_forward(wav, n_samples) - target|,   grad_wav = scale * d loss / d wav        (B, N) fp32, dense rows
 * target (B, n_mels, N / hop) fp32.  reduction PARROT_MEL_REDUCE_MEAN: loss (1 float) is parrot_mel_l1's mean_f32 of the two
 * spectrograms with n_frames = n_samples / hop, bit for bit; PARROT_MEL_REDUCE_SUM: loss (1 double) is the row sums added in row
 * order, every real element weighted 1, so that a row's gradient depends on that row alone.  out_f64 (2B doubles) as parrot_mel_l1.
 * torch's autograd rules of dataset.py:55-67: d|x| = sgn(x) (0 at 0); the clamp passes the gradient where mel >= 1e-5 and 0 below;
 * the magnitude's gradient re / mag, im / mag is finite at re = im = 0; the reflect pad's adjoint adds the mirrored contributions
 * onto the interior samples, row b folding at its OWN end n_samples[b] - 1; grad_wav[b, n_samples[b]:] is exactly 0, frames at and
 * beyond n_samples[b] / hop contribute nothing, and padded samples no frame reads get nothing.  No floating-point atomics: two
 * calls agree bit for bit.
 * Precision: the forward half is the handle's own; the two transposed GEMMs (basis^T, DFT^T) are plans of their own in
 * PARROT_PREC_F32 for every handle (1 / mel reaches 5e4, beyond the fp16 split scheme's range), the DFT's summed in 8 channel
 * groups as the f32 handle's forward DFT is; they run on unit-weight operands: scale / count is applied once, where grad_wav is
 * written.  Status through parrot_mel_check / parrot_mel_status_async as the forward: 8 a short row, 5 a
 * non-finite mel or gradient value. */
#define PARROT_MEL_REDUCE_MEAN 0
#define PARROT_MEL_REDUCE_SUM 1
size_t parrot_mel_l1_grad_workspace_bytes(const parrot_mel_t*, int32_t B, int32_t N);
int parrot_mel_l1_grad(parrot_mel_t*, const float* wav, int64_t row_stride, const int32_t* n_samples /* nullable */, const float* target,
                       int32_t B, int32_t N, int32_t reduction, double scale, double* out_f64, void* loss, float* grad_wav, void* ws,
                       size_t ws_bytes, void* stream);
/* Synchronises `stream`, clears the flag: 0, PARROT_E_INVALID (status 8) or PARROT_E_NONFINITE (status 5). */
int parrot_mel_check(parrot_mel_t*, void* stream);
/* The same flag without a synchronisation: see parrot_voc_status_async. */
int parrot_mel_status_async(parrot_mel_t*, int32_t* dst_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Forced aligner: Aligner.forward (utils/aligner/model.py:24-48), the softmax of utils/aligner/extract_durations.py:91-93 and
 * extract_durations_with_dijkstra (utils/aligner/duration_extraction.py:52-85).
 *   mel (B, T, n_mels) -> 3 x [Conv1d(k = 5, pad 2, no bias) -> ReLU -> BatchNorm1d (eval, running statistics)] (model.py:6-21)
 *   -> one-layer bidirectional LSTM (gates i, f, g, o; output [forward, backward]) -> Linear(2 lstm_dim, num_symbols).
 * The five GEMMs run on the parrot_conv kernels (the LSTM input projection of both directions for all frames as one 1x1 plan);
 * the recurrence is one launch of lstm_step_kernel per frame, fp32 in every mode, with stream order as its only synchronisation.
 * The padded batch runs as it stands (dataset.py:66-75): the backward direction of a short row starts inside the padding, so a
 * row's logits depend on the T it is padded to, as the reference's do; mel_len enters at the softmax.
 * conv_dim and lstm_dim: multiples of 16 (else PARROT_E_UNSUPPORTED), lstm_dim <= 1024; n_mels, num_symbols, B arbitrary;
 * T <= 32768 frames, N <= 2048 tokens per utterance (beyond: PARROT_E_UNSUPPORTED).
 * Precision: as the mel handle -- PARROT_PREC_F16X3 (default), PARROT_PREC_BF16X6, PARROT_PREC_F32; under a process default of
 * PARROT_PREC_BF16 / PARROT_PREC_F16 the handle is built in PARROT_PREC_F16X3 and asking _create_ex for either is
 * PARROT_E_UNSUPPORTED.
 * ------------------------------------------------------------------------------------------ */
typedef struct parrot_aligner parrot_aligner_t;

typedef struct {
    int32_t n_mels, num_symbols, lstm_dim, conv_dim; /* Aligner.__init__ (model.py:26-30); num_symbols = len(symbols) + 1 */
    float bn_eps;                                    /* BatchNorm1d.eps (1e-5) */
} parrot_aligner_cfg;

/* fp32 HOST pointers, torch layouts (state_dict keys of model.py in brackets) */
typedef struct {
    const float* conv_w[3];    /* [convs.i.conv.weight]  (conv_dim, n_mels | conv_dim, 5) */
    const float* bn_weight[3]; /* [convs.i.bnorm.weight / bias / running_mean / running_var]  (conv_dim) each */
    const float* bn_bias[3];
    const float* bn_mean[3];
    const float* bn_var[3];
    const float* w_ih[2];      /* [rnn.weight_ih_l0, rnn.weight_ih_l0_reverse]  (4 lstm_dim, conv_dim) */
    const float* w_hh[2];      /* [rnn.weight_hh_l0, ..._reverse]               (4 lstm_dim, lstm_dim) */
    const float* b_ih[2];      /* [rnn.bias_ih_l0, ..._reverse]                 (4 lstm_dim) */
    const float* b_hh[2];      /* [rnn.bias_hh_l0, ..._reverse]                 (4 lstm_dim) */
    const float* lin_w;        /* [lin.weight]  (num_symbols, 2 lstm_dim) */
    const float* lin_b;        /* [lin.bias]    (num_symbols) */
} parrot_aligner_weights;

int parrot_aligner_create(parrot_aligner_t** out, const parrot_aligner_cfg* cfg, const parrot_aligner_weights* w);
int parrot_aligner_create_ex(parrot_aligner_t** out, const parrot_aligner_cfg* cfg, const parrot_aligner_weights* w,
                             int32_t precision /* PARROT_PREC_F32 / BF16X6 / F16X3; -1 = default */);
void parrot_aligner_destroy(parrot_aligner_t*);
int parrot_aligner_precision(const parrot_aligner_t*);
size_t parrot_aligner_workspace_bytes(const parrot_aligner_t*, int32_t B, int32_t T);
/* Aligner.forward (model.py:41-48): mel (B, T, n_mels) fp32 -> logits (B, T, num_symbols) fp32, every frame of the padded batch. */
int parrot_aligner_forward(parrot_aligner_t*, const float* mel, int32_t B, int32_t T, float* logits, void* ws, size_t ws_bytes, void* stream);
/* torch.softmax(logits[b, :mel_len[b]], -1) (extract_durations.py:91-93): logits (B, T, num_symbols) -> pred of the same shape,
 * fp32, max-shifted; mel_len (B) int32 device (NULL: T); frames at or beyond mel_len[b] are written as zero.  May run in place.
 * A non-finite logit of a real frame sets status 5, a mel_len[b] outside [1, T] status 9 (it is clamped, nothing is read through
 * it; 9 wins over 5) (parrot_aligner_check / _status_async). */
int parrot_align_softmax(parrot_aligner_t*, const float* logits, const int32_t* mel_len, int32_t B, int32_t T, float* pred, void* stream);
/* Synchronises `stream`, clears the flag: 0, PARROT_E_NONFINITE (status 5) or PARROT_E_INVALID (status 9). */
int parrot_aligner_check(parrot_aligner_t*, void* stream);
/* The same flag without a synchronisation: see parrot_voc_status_async. */
int parrot_aligner_status_async(parrot_aligner_t*, int32_t* dst_dev, void* stream);
/* extract_durations_with_dijkstra (duration_extraction.py:52-85) for a ragged batch, one workgroup per utterance.  It takes
 * PROBABILITIES: pred (B, T, V) fp32, tokens (B, N) int64, mel_len / tokens_len (B) int32, all device; row b uses
 * pred[b, :mel_len[b]] and tokens[b, :tokens_len[b]] (tokens_len[b] > mel_len[b] is legal).
 *   w[i][j] = fl32(1 - pred[i][tokens[j]]) widened to fp64; dist[0][0] = 0,
 *   dist[i][j] = min(dist[i-1][j-1], dist[i-1][j], dist[i][j-1]) + w[i][j] in fp64 -- the sums scipy's Dijkstra forms;
 * every frame counts for the last token the cheapest path visits in its row.  Tie rule (the reference's choice among equally
 * cheap paths follows no fixed rule): equal predecessors -> diagonal, then previous frame, then previous token.
 * dur_out (B, N) int32 (sums to mel_len[b]; zero beyond tokens_len[b]), cost_out (B) fp64 = dist[mel_len-1][tokens_len-1].
 * ws: parrot_align_workspace_bytes(B, T, N); its first int32 is the call's status, 0 or 9: a token outside [0, V) or a length
 * outside [1, T] / [1, N] -- nothing is read through such a value; that row's durations are zero and its cost NaN. */
size_t parrot_align_workspace_bytes(int32_t B, int32_t T, int32_t N);
int parrot_align_durations(const float* pred, const int64_t* tokens, const int32_t* mel_len, const int32_t* tokens_len, int32_t B, int32_t T,
                           int32_t V, int32_t N, int32_t* dur_out, double* cost_out, void* ws, size_t ws_bytes, void* stream);
/* The aligner's validation loss, the CTC loss of utils/aligner/trainer.py:60-63:
 *   pred = model(mel); pred.transpose(0, 1).log_softmax(2); CTCLoss()(pred, tokens, mel_len, tokens_len)
 * with torch's defaults (blank = 0, no zero_infinity), forward pass only.  It takes LOGITS: logits (B, T, V) fp32, tokens (B, N)
 * int64, mel_len / tokens_len (B) int32, all device; row b uses logits[b, :mel_len[b]] and tokens[b, :tokens_len[b]], nothing
 * beyond them is read.  Per real frame the fp32 max-shifted log-sum-exp over V (the reference's fp32 log_softmax); then, one
 * workgroup per utterance, the forward recursion over the S = 2 tokens_len + 1 states blank, tok_0, blank, ..., blank in fp64:
 *   lp[t][c] = logits[t][c] - lse[t];  alpha_0[0] = lp[0][blank], alpha_0[1] = lp[0][tok_0], -inf elsewhere;
 *   alpha_t[s] = logaddexp(alpha_{t-1}[s], alpha_{t-1}[s-1], alpha_{t-1}[s-2] if s is odd and tok differs from the previous tok)
 *                + lp[t][label_s];
 *   nll = -logaddexp(alpha_{T-1}[S-1], alpha_{T-1}[S-2]).
 * A token equal to the blank is legal.  A row with mel_len < tokens_len + (number of repeated neighbours) has no path: its nll
 * is exactly +inf and the other rows are untouched.
 * nll_out (B) fp64; mean_out (1) fp32, nullable: mean_b(nll[b] / tokens_len[b]) (torch's reduction='mean'), summed in fp64 in row
 * order.  Deterministic: two calls agree bit for bit, and a row's nll does not depend on the rows beside it.
 * T <= 32768, N <= 2048 (beyond: PARROT_E_UNSUPPORTED; parrot_ctc_workspace_bytes returns 0).
 * ws: parrot_ctc_workspace_bytes(B, T, N); its first int32 is the call's status: 0; 5, a NaN / inf logit in a real frame; or 9,
 * a token outside [0, V) among the first tokens_len[b] or a length outside [1, T] / [1, N] -- nothing is read through such a
 * value and that row's nll is NaN.  The larger status wins. */
size_t parrot_ctc_workspace_bytes(int32_t B, int32_t T, int32_t N);
int parrot_ctc_loss(const float* logits, const int64_t* tokens, const int32_t* mel_len, const int32_t* tokens_len, int32_t B, int32_t T,
                    int32_t V, int32_t N, double* nll_out /* (B) */, float* mean_out /* (1), nullable */, void* ws, size_t ws_bytes,
                    void* stream);
/* The same loss with its gradient with respect to the LOGITS (the log-softmax folded in): what loss.backward() of
 * utils/aligner/trainer.py:60-71 hands to the network.  Arguments, limits, status word and error codes are parrot_ctc_loss's;
 * nll_out holds the same bits.  The call is stateless: it recomputes alpha, keeps it, runs the mirror-image recursion
 *   beta_{T-1}[S-1] = lp[T-1][blank], beta_{T-1}[S-2] = lp[T-1][label_{S-2}], -inf elsewhere;
 *   beta_t[s] = logaddexp(beta_{t+1}[s], beta_{t+1}[s+1], beta_{t+1}[s+2] if state s+2 may be entered by a skip) + lp[t][label_s]
 * in fp64 and writes, for every row b, frame t and symbol v,
 *   gamma_t(v)    = sum over the states s labelled v of exp(alpha_t[s] + beta_t[s] - lp[t][v] + nll[b]),
 *   grad[b][t][v] = (float)(w_b (exp(lp[t][v]) - gamma_t(v)))   for t < mel_len[b],        exactly 0 for mel_len[b] <= t < T,
 * with w_b = row_weight[b] (fp64, device; null: all ones) -- the caller's reduction and upstream gradient.  Every element of
 * grad_out (B, T, V) fp32 is written.  This is the true gradient: torch's CPU backward drops the final blank state's term at
 * the last frame of a row whose last token is the blank, and differs there.
 * Special rows: a row without a path (nll = +inf) is NaN on its real frames and 0 beyond them, as torch's; with zero_infinity
 * != 0 it is 0 throughout.  A row that raised status 9 is NaN throughout, and nothing is read through the bad value.  Other rows
 * are untouched by either.
 * Deterministic: no floating-point atomics; every gamma_t(v) is summed in an order fixed by the row's tokens, so two calls agree
 * bit for bit and a row's gradient depends on that row, T and V only -- not on B or on the rows beside it.
 * ws: parrot_ctc_grad_workspace_bytes(B, T, V, N) (0 beyond the limits): the status word, lse, alpha (B, T, 2 N + 1) fp64 and
 * the sorted token index. */
size_t parrot_ctc_grad_workspace_bytes(int32_t B, int32_t T, int32_t V, int32_t N);
int parrot_ctc_loss_grad(const float* logits, const int64_t* tokens, const int32_t* mel_len, const int32_t* tokens_len, int32_t B,
                         int32_t T, int32_t V, int32_t N, const double* row_weight /* (B), nullable: all ones */, int32_t zero_infinity,
                         double* nll_out /* (B) */, float* grad_out /* (B, T, V) */, void* ws, size_t ws_bytes, void* stream);

/* ---- training the aligner (utils/aligner/model.py:5-48 under model.train(); trainer.py:60-71) ----
 * The forward on BATCH statistics and the full backward, as two stateless calls.  Every weight is read from the DEVICE pointer
 * given here, in torch's layout: nothing is packed, cached or copied to the host, and neither call synchronises, so a parameter an
 * optimiser has just updated in place is seen by the next call.
 *   per block: conv(k = 5, pad 2, no bias) -> ReLU -> BatchNorm1d.  training != 0: per channel over all n = B T values of the
 *   padded batch (nothing is masked), y = (x - mean) rsqrt(var_biased + eps) gamma + beta, and the running buffers are updated
 *   in place: running_mean <- 0.9 running_mean + 0.1 mean, running_var <- 0.9 running_var + 0.1 var_biased n / (n - 1)
 *   (num_batches_tracked is the caller's).  training == 0: the running statistics, and no buffer is touched.
 *   then the bidirectional LSTM (gates i, f, g, o; h_0 = c_0 = 0) and Linear(2 lstm_dim -> num_symbols).
 * All products are exact fp32 (fp32 MFMA / FMA, fp32 accumulation); the batch statistics and every gradient that sums over B T
 * (weights, biases, gamma, beta) are summed in fp64 over fixed blocks in a fixed order and rounded once.  No floating-point
 * atomics: two calls on the same inputs agree bit for bit.  NaN / inf propagate as in torch and nothing is raised.
 * Limits and argument errors are parrot_aligner_forward's (conv_dim, lstm_dim multiples of 16, lstm_dim <= 1024, T <= 32768),
 * and B T <= 3 355 392; B T == 1 with training != 0 is PARROT_E_INVALID (torch: "Expected more than 1 value per channel"). */
typedef struct {
    const float* conv_w[3];    /* the fields of parrot_aligner_weights, as fp32 DEVICE pointers */
    const float* bn_weight[3];
    const float* bn_bias[3];
    float* bn_mean[3];         /* running_mean / running_var: updated in place by a training forward */
    float* bn_var[3];
    const float* w_ih[2];
    const float* w_hh[2];
    const float* b_ih[2];
    const float* b_hh[2];
    const float* lin_w;
    const float* lin_b;
} parrot_aligner_dev_weights;
/* Where the backward writes d loss / d parameter: device, the parameter's own shape.  A null field is not computed. */
typedef struct {
    float* conv_w[3];
    float* bn_weight[3];
    float* bn_bias[3];
    float* w_ih[2];
    float* w_hh[2];
    float* b_ih[2];            /* b_ih and b_hh receive the same bits */
    float* b_hh[2];
    float* lin_w;
    float* lin_b;
} parrot_aligner_grads;
/* Bytes of what the forward keeps for the backward, and of the workspace of either call (0 beyond the limits). */
size_t parrot_aligner_train_saved_bytes(const parrot_aligner_cfg* cfg, int32_t B, int32_t T);
size_t parrot_aligner_train_workspace_bytes(const parrot_aligner_cfg* cfg, int32_t B, int32_t T);
/* mel (B, T, n_mels) -> logits (B, T, num_symbols).  saved: parrot_aligner_train_saved_bytes, may be NULL when training == 0. */
int parrot_aligner_train_forward(const parrot_aligner_cfg* cfg, const parrot_aligner_dev_weights* w, const float* mel, int32_t B, int32_t T,
                                 int32_t training, float* logits, void* saved, void* ws, size_t ws_bytes, void* stream);
/* The gradients of every parameter from grad_logits (B, T, num_symbols), after a training forward on the same mel, weights and
 * `saved`.  mel gets no gradient. */
int parrot_aligner_train_backward(const parrot_aligner_cfg* cfg, const parrot_aligner_dev_weights* w, const float* mel, const void* saved,
                                  const float* grad_logits, int32_t B, int32_t T, const parrot_aligner_grads* grads, void* ws, size_t ws_bytes,
                                  void* stream);

/* ---- training the TTE (modules/parrot.py:90-110 with inference=False under model.train(); train.py:72-85) ----
 * The teacher-forced forward with dropout and the full backward, as two stateless calls shaped like the aligner's.  Every weight is
 * read from the DEVICE pointer given here, in torch's layout: nothing is packed, cached or copied to the host, neither call
 * synchronises, and a parameter an optimiser has just updated in place is seen by the next call.
 *   forward: tok_emb[phones] + pe[S] (the single row of the padded length, fft.py:18) -> the encoder FFT blocks under src_mask ->
 *   + speaker_emb[speaker] (n_speaker > 1) -> the duration predictor on that output, masked to 0 outside src_mask -> the length
 *   regulator on the CALLER's durations (every position counts; rows shorter than L are zero-padded) -> + pe[L] -> the decoder
 *   blocks under tgt_mask -> the head.  phones, duration (B, S) i64; src_mask (B, S), tgt_mask (B, L) u8, 1 = attend; speaker (B) i64
 *   (NULL without a speaker embedding); logits (B, L, n_codes), log_dur (B, S) f32.  The caller checks what torch would raise on:
 *   ids inside their tables, durations >= 0 with max row sum == L (an id outside its table gives NaN rows here, never an access
 *   through it; durations are saturated into [0, L]).
 *   training != 0: dropout acts on the softmax probabilities of every FFT block (p_enc / p_dec) and after the two LayerNorms of the
 *   duration predictor (p_dp), nowhere else.  Element i of dropout site `site` is kept iff
 *       philox4x32_10(counter {lo32(i), hi32(i), lo32(offset), (hi32(offset) & 0xffffff) | site << 24}, key {lo32(seed), hi32(seed)})[0] >> 8
 *           >= floor(p 2^24 + 0.5)
 *   and a survivor is multiplied by the fp32 quotient 1 / (1 - p); p = 0 is the identity, p = 1 gives zeros.  Sites: 0, 1 the
 *   duration predictor's (i = (b S + s) n_filter + c), 2 + l encoder block l, 2 + enc_layers + l decoder block l
 *   (i = ((b H + h) T + tq) T + tk).  The backward regenerates the masks from (seed, offset): they are not stored.
 *   saved (parrot_tte_train_saved_bytes; may be NULL when training == 0) keeps every activation the backward reads, the softmax
 *   probabilities before dropout among them: about B (S (14 D + F) + 2 H S^2) floats per encoder block, the same with L per decoder
 *   block.  The weight-gradient partials in the workspace are bounded by max(64 MiB, ceil(B max(S, L) / 256) x the largest one-tap
 *   weight): wider convs are reduced a few taps at a time.
 * backward: the gradient of every parameter from grad_logits (B, L, n_codes) and grad_log_dur (B, S); either may be NULL (zero).
 * All products are exact fp32 (fp32 MFMA, fp32 accumulation); every gradient that sums over B T (weights, biases, gamma, beta, the
 * embedding rows, the length regulator's segments) is summed in fp64 in a fixed order and rounded once.  No floating-point atomics:
 * two calls on the same inputs and (seed, offset) agree bit for bit.  NaN / inf propagate.  Limits (PARROT_E_INVALID): at most
 * PARROT_TTE_TRAIN_MAX_LAYERS blocks per stack, odd FFN kernels of at most 9 taps, duration kernel 3, B x heads <= 65535,
 * B max(S, L) <= 1 863 936; max(S, L) >= max_len is PARROT_E_RANGE (pe[T]), before any launch. */
#define PARROT_TTE_TRAIN_MAX_LAYERS 16
typedef struct {
    parrot_tte_cfg tte;
    int32_t pad_idx;             /* tok_emb's padding_idx: that row's gradient is exactly 0; -1 = none */
    float p_enc, p_dec, p_dp;    /* the three dropout probabilities */
} parrot_tte_train_cfg;
typedef struct {
    const float *pe, *tok_emb, *speaker_emb;   /* the fields of parrot_tte_weights, as fp32 DEVICE pointers */
    const float *dp_conv0_w, *dp_conv0_b, *dp_ln0_w, *dp_ln0_b;
    const float *dp_conv1_w, *dp_conv1_b, *dp_ln1_w, *dp_ln1_b;
    const float *dp_proj_w, *dp_proj_b;
    const float *head_w, *head_b;
    parrot_fft_weights enc[PARROT_TTE_TRAIN_MAX_LAYERS];
    parrot_fft_weights dec[PARROT_TTE_TRAIN_MAX_LAYERS];
} parrot_tte_dev_weights;
typedef struct {
    float *qkv, *in_proj, *out_proj, *wo;
    float *conv1_w, *conv1_b, *conv2_w, *conv2_b;
    float *attn_norm_w, *attn_norm_b, *conv_norm_w, *conv_norm_b;
} parrot_fft_grads;
/* Where the backward writes d loss / d parameter: device, the parameter's own shape.  A null field is not computed; pe is a
 * buffer and is never written. */
typedef struct {
    float *pe, *tok_emb, *speaker_emb;
    float *dp_conv0_w, *dp_conv0_b, *dp_ln0_w, *dp_ln0_b;
    float *dp_conv1_w, *dp_conv1_b, *dp_ln1_w, *dp_ln1_b;
    float *dp_proj_w, *dp_proj_b;
    float *head_w, *head_b;
    parrot_fft_grads enc[PARROT_TTE_TRAIN_MAX_LAYERS];
    parrot_fft_grads dec[PARROT_TTE_TRAIN_MAX_LAYERS];
} parrot_tte_grads;
/* Bytes of what the forward keeps for the backward, and of the workspace of either call (0 beyond the limits). */
size_t parrot_tte_train_saved_bytes(const parrot_tte_train_cfg* cfg, int32_t B, int32_t S, int32_t L);
size_t parrot_tte_train_workspace_bytes(const parrot_tte_train_cfg* cfg, int32_t B, int32_t S, int32_t L);
int parrot_tte_train_forward(const parrot_tte_train_cfg* cfg, const parrot_tte_dev_weights* w, const int64_t* phones, const uint8_t* src_mask,
                             const int64_t* speaker, const int64_t* duration, const uint8_t* tgt_mask, int32_t B, int32_t S, int32_t L,
                             int32_t training, uint64_t seed, uint64_t offset, float* logits, float* log_dur, void* saved, void* ws,
                             size_t ws_bytes, void* stream);
int parrot_tte_train_backward(const parrot_tte_train_cfg* cfg, const parrot_tte_dev_weights* w, const int64_t* phones, const uint8_t* src_mask,
                              const int64_t* speaker, const int64_t* duration, const uint8_t* tgt_mask, const void* saved,
                              const float* grad_logits, const float* grad_log_dur, int32_t B, int32_t S, int32_t L, uint64_t seed,
                              uint64_t offset, const parrot_tte_grads* grads, void* ws, size_t ws_bytes, void* stream);

/* ---- the vocoder's adversarial losses (utils/vocoder/models.py:279-310; train.py:141-148, 159-165) ----
 * feature_loss, generator_loss and discriminator_loss are sums of means over dense fp32 arrays.  One call evaluates a whole
 * table of such TERMS -- the 54 feature maps and 8 scores of a generator step, say -- with their gradients: one launch reads
 * every a and b once and writes every requested gradient once, a second one of a single workgroup forms the means.
 *   PARROT_GAN_L1   mean |a - b|    (one feature_loss term)            grad_b = sgn(b - a) w / n,  grad_a = -grad_b
 *   PARROT_GAN_SQ1  mean (1 - a)^2  (generator_loss; the real term     grad_a = -2 (1 - a) w / n
 *                                    of discriminator_loss), b unused
 *   PARROT_GAN_SQ0  mean a^2        (discriminator_loss's generated    grad_a = 2 a w / n
 *                                    term), b unused
 * Each element's contribution is formed in fp64 from the fp32 inputs and summed in fp64 in a fixed order over tiles of
 * parrot_gan_loss_tile() elements that start at the term's element 0: no atomics, two calls agree bit for bit, and a term's
 * mean and gradients depend on that term's data, n and weight only -- not on K, on the other terms or on its place in the table.
 * An L1 gradient element is (float)(w / n) with the sign of the COMPARISON of a and b (exactly 0 where a == b, and where either
 * is NaN, as torch's sgn); a squares gradient element is the fp64 product rounded once.  n = 0: the mean is NaN (torch's mean
 * of nothing), no gradient element is touched, the other terms are as ever.  NaN / inf inputs propagate; there is no status word.
 * More than PARROT_GAN_MAX_TERMS terms become several launches inside the call. */
#define PARROT_GAN_L1 0
#define PARROT_GAN_SQ1 1
#define PARROT_GAN_SQ0 2
#define PARROT_GAN_MAX_TERMS 64 /* terms per launch: the table travels in the kernel arguments */
#define PARROT_GAN_GRID_CAP 2048 /* workgroups per launch; further tiles are reached by stride */
typedef struct {
    const float* a;
    const float* b; /* PARROT_GAN_L1 only */
    float* grad_a;  /* nullable: not wanted */
    float* grad_b;  /* nullable; PARROT_GAN_L1 only */
    int64_t n;
    int32_t op;
    int32_t reserved;
} parrot_gan_term_t; /* 48 bytes */
/* elements per tile */
int32_t parrot_gan_loss_tile(void);
/* needs no device; 0 for K <= 0 or a term with n < 0.  A function of K and of the number of tiles alone. */
size_t parrot_gan_loss_workspace_bytes(const parrot_gan_term_t* terms /* host */, int32_t K);
/* terms: HOST array of K terms with DEVICE pointers inside.  weights: DEVICE, K doubles, the gradient arriving at each term's mean
 * (a backward needs no host synchronisation); NULL = ones.  term_out (device, K, nullable) <- the unweighted means in fp64;
 * total (device, 1, nullable) <- (float)(scale * sum_k term_out[k]), summed in fp64 in table order and rounded once; scale enters
 * nothing else.  With both null (a backward) the call is the one launch and ws may be null; values without any gradient are the
 * forward alone.  PARROT_E_INVALID, before any HIP call: a null table with K > 0, an unknown op, n < 0, a null a (or b of an L1
 * term), grad_b on a squares term, a gradient that aliases its term's a or b, neither values nor a gradient requested;
 * PARROT_E_NOMEM: ws_bytes < parrot_gan_loss_workspace_bytes(terms, K) when values are requested. */
int parrot_gan_loss(const parrot_gan_term_t* terms, int32_t K, const double* weights /* device, nullable */, double scale,
                    double* term_out /* device, K, nullable */, float* total /* device, 1, nullable */, void* ws, size_t ws_bytes,
                    void* stream);

/* ---- fused multi-tensor AdamW (torch.optim.AdamW without amsgrad; utils/vocoder/train.py:80-82, 151, 168) ----
 * One call updates a whole parameter group: every tensor's p, m (exp_avg) and v (exp_avg_sq) from its gradient g, each array read
 * once and written once, in as few launches as ceil(K / parrot_adamw_max_tensors()).  Stateless: no handle, no device allocation,
 * no copy, no host synchronisation; the table travels in the kernel arguments.  The update is this rule, every line one correctly
 * rounded fp32 operation and nothing contracted:
 *   host, in double, each rounded to fp32 once:
 *     decay = 1 - lr wd    w1 = 1 - beta1    b2 = beta2    w2 = 1 - beta2    e = eps
 *     per tensor:  ns = -lr / (1 - beta1^step)    rs = sqrt(1 - beta2^step)
 *   device, per element:
 *     p <- p decay;  m <- m + (g - m) w1;  v <- v b2 + (g w2) g;  d <- sqrt(v) / rs + e;  p <- p + ns (m / d)
 * `step` is the tensor's step count AFTER this update (>= 1), per tensor as torch keeps it per parameter.  g is read only.  The
 * arrays are dense fp32 at any 4-byte alignment (16-byte accesses where all four bases allow them); nothing outside [0, n) is read
 * or written; a tensor with n == 0 is skipped.  An element's result depends on its own p, g, m, v and the scalars only: two calls
 * agree bit for bit.  NaN / inf propagate; there is no status word.
 * PARROT_E_INVALID, before any HIP call: a null table with K > 0, K < 0, a null pointer, n < 0, step < 1, lr < 0, eps < 0,
 * weight_decay < 0, a beta outside [0, 1), two of a tensor's four pointers equal. */
typedef struct {
    float* p;
    const float* g;
    float* m;
    float* v;
    int64_t n;
    int64_t step;
} parrot_adamw_tensor_t; /* 48 bytes */
/* t: HOST array of K tensors with DEVICE pointers inside */
int parrot_adamw_step(const parrot_adamw_tensor_t* t, int32_t K, double lr, double beta1, double beta2, double eps, double weight_decay,
                      void* stream);
/* elements one block updates */
int32_t parrot_adamw_chunk(void);
/* tensors one launch's by-value table holds */
int32_t parrot_adamw_max_tensors(void);

/* ---- training the vocoder's generator (utils/vocoder/models.py:69-169 with weight norm attached; train.py:131-168) ----
 * CodeGenerator.forward and its full backward as two stateless calls shaped like the TTE's.  Every parameter is read from the DEVICE
 * pointer given here, in torch's layout, through strides: nothing is packed, cached or copied to the host, neither call synchronises,
 * and a parameter an optimiser has just updated in place is seen by the next call.
 *   forward (models.py:153-169, :95-111): x = dict[code] transposed to (B, E, U), with spkr[spkr] broadcast over the frames below it
 *   when multispkr (model_in_dim == embedding_dim (1 + multispkr): conditioning features are not trainable here) -> conv_pre ->
 *   per stage: leaky ReLU 0.1, ConvTranspose1d(C, C / 2, k, u, padding (k - u) / 2) by output phase, the n_kernels ResBlock1 / ResBlock2
 *   (:31-38, :58-62) and ((r0 + r1) + r2) / n_kernels -> leaky ReLU 0.01 (:107) -> conv_post -> tanh.  code (B, U) i64, spkr (B) i64
 *   (NULL without multispkr), wav (B, 1, parrot_voc_train_out_len(cfg, U)) f32.  An id outside its table gives NaN, never an access.
 *   Weight norm (models.py:75-91, old style, dim 0): a layer with g runs on w = v (g / ||v||), the norm per row of dim 0 -- the INPUT
 *   channels of a ConvTranspose1d -- summed in fp64 in a fixed order and rounded once; a layer with g == NULL runs on v as it is
 *   (remove_weight_norm(), :113-119).  A zero row gives what torch._weight_norm gives: nothing is clamped.
 *   saved (parrot_voc_train_saved_bytes; NULL = keep nothing, for a forward without a backward) keeps the embedded input, every
 *   conv's activated input a = lrelu(x), the waveform, and every layer's norms and folded weight.  The leaky ReLU's backward reads
 *   its mask from there: a > 0, the same predicate as x > 0, so x == 0 takes the slope as in torch.
 * backward: the gradient of every parameter named in `grads` from grad_wav (B, 1, T).  With s = sum(dw v) in fp64 per row:
 *   dg = s / ||v||, dv = (g / ||v||) dw - (g s / ||v||^3) v; a layer without g gets dw in `v`.  d dict and d spkr are fixed-order fp64
 *   row scatters (ascending (b, t)).
 * All products are exact fp32 (fp32 MFMA, fp32 accumulation); every sum that ends in one number is fp64 in a fixed order.  No
 * floating-point atomics: two calls on the same inputs agree bit for bit, and a batch row's waveform does not depend on the rows
 * beside it.  NaN / inf propagate.  Limits (PARROT_E_INVALID, before any HIP call): positive sizes, U >= 1, B <= 65535, odd resblock
 * kernels and upsample kernels of at most 11 taps with rate <= kernel, every activation below 2^30 elements, and
 * ceil(B T / 256) x taps <= 65535 for every weight gradient. */
#define PARROT_VOC_TRAIN_MAX_RB (PARROT_MAX_STAGES * PARROT_MAX_KERNELS * 2 * PARROT_MAX_DIL)
typedef struct {
    float* v;    /* weight_v, or the plain weight when g == NULL: (C_out, C_in, k), a ConvTranspose1d's (C_in, C_out, k) */
    float* g;    /* weight_g (dim 0 rows), nullable */
    float* bias;
} parrot_voc_layer_ptrs;
/* DEVICE pointers of every parameter (the forward and the backward read them) or of every gradient (the backward writes them; a
 * null field is not wanted and is not computed).  rb is indexed as parrot_voc_weights.rb_w. */
typedef struct {
    float* dict;  /* (num_embeddings, embedding_dim) */
    float* spkr;  /* (n_spkr, embedding_dim), NULL without multispkr */
    parrot_voc_layer_ptrs conv_pre;
    parrot_voc_layer_ptrs ups[PARROT_MAX_STAGES];
    parrot_voc_layer_ptrs rb[PARROT_VOC_TRAIN_MAX_RB];
    parrot_voc_layer_ptrs conv_post;
} parrot_voc_train_ptrs;
/* Samples per row for U units: the ConvTranspose1d length chain (models.py:80-83); 0 beyond the limits. */
int64_t parrot_voc_train_out_len(const parrot_voc_cfg* cfg, int32_t U);
/* Bytes of what the forward keeps for the backward, and of the workspace of either call (0 beyond the limits). */
size_t parrot_voc_train_saved_bytes(const parrot_voc_cfg* cfg, int32_t B, int32_t U);
size_t parrot_voc_train_workspace_bytes(const parrot_voc_cfg* cfg, int32_t B, int32_t U);
/* models.py:153-169 (train.py:131: y_g_hat = generator(**x)) */
int parrot_voc_train_forward(const parrot_voc_cfg* cfg, const parrot_voc_train_ptrs* w, const int64_t* code, const int64_t* spkr, int32_t B,
                             int32_t U, float* wav, void* saved, void* ws, size_t ws_bytes, void* stream);
/* the backward of that graph (train.py:166: loss_gen_all.backward()) */
int parrot_voc_train_backward(const parrot_voc_cfg* cfg, const parrot_voc_train_ptrs* w, const int64_t* code, const int64_t* spkr,
                              const void* saved, const float* grad_wav, int32_t B, int32_t U, const parrot_voc_train_ptrs* grads, void* ws,
                              size_t ws_bytes, void* stream);

/* ---- training the multi-period discriminator (utils/vocoder/models.py:171-225 with weight norm attached; train.py:141-142, :159-163) ----
 * MultiPeriodDiscriminator.forward and its full backward as two stateless calls shaped like the generator's: parameters are read
 * from the DEVICE pointers given here, in torch's layout ((C_out, C_in, k, 1) is (C_out, C_in, k)); nothing is packed, cached or copied
 * to the host, and neither call synchronises.
 *   forward: wav (N, 1, T) f32 -- the caller stacks real and generated rows, N = 2 B.  Per period p: the tail is reflect-padded by
 *   n_pad = p - T mod p when T mod p != 0 and the row viewed as (H, p); convs[0 .. 4) are (kernel_size, 1) convs of stride (stride, 1),
 *   convs[4] has stride 1, each with padding (2, 0) whatever kernel_size is, bias and leaky ReLU `slope`; conv_post is (3, 1), padding
 *   (1, 0), no activation.  The widths are 1 -> channels[0] -> ... -> channels[3] -> channels[3] -> 1.
 *   Maps: the caller owns the six maps of every period and gets them PERIOD-MAJOR: map[i][l] is a dense (N, periods[i], C_l, H_l)
 *   array, H_l = parrot_mpd_train_map_rows(cfg, T, i, l); torch's (N, C_l, H_l, p) is its permutation (0, 2, 3, 1), and the score the
 *   flattened sixth map.  The maps are also what the backward reads (the leaky ReLU's mask is map > 0, the next layer's weight
 *   gradient reads the same buffer): they must reach it unchanged.
 *   saved (parrot_mpd_train_saved_bytes; NULL = keep nothing): every layer's weight-norm row norms and folded weight.
 * backward: grad_maps->map[i][l] is the gradient that arrives at map[i][l] from outside, in the map's layout, or NULL for zero; the
 *   gradient at a map is (that + the next layer's data gradient), and the sum passes the map's mask.  Outputs: the gradient of every
 *   parameter named in `grads` (a null field is neither wanted nor computed; weight norm as in parrot_voc_train_backward) and, when
 *   grad_wav != NULL, d wav (N, 1, T), the periods added in their order; the reflect pad's backward adds padded sample T + i into
 *   sample T - 2 - i once, after the sample's own gradient.  With grad_wav == NULL the first layer's data gradient is not launched.
 * Numerics: the generator's contract (exact fp32 products, fp32 accumulation in bounded chains, fp64 fixed-order sums for everything
 * that ends in one number, no floating-point atomics, rows independent, NaN / inf propagate).  Limits (PARROT_E_INVALID, before any
 * HIP call): 1 to 8 periods, each >= 1; N, T and the widths >= 1; kernel_size odd and <= 11; 1 <= stride <= kernel_size; T > n_pad
 * for every period (torch refuses a reflect pad that is not smaller than its input); N p <= 65535; a null parameter or map; a
 * workspace that is too small is PARROT_E_NOMEM. */
#define PARROT_MPD_MAX_PERIODS 8
#define PARROT_MPD_LAYERS 6 /* convs[0 .. 5), conv_post */
typedef struct {
    int32_t n_periods;
    int32_t periods[PARROT_MPD_MAX_PERIODS]; /* reference: 2, 3, 5, 7, 11 */
    int32_t channels[4];                     /* reference: 32, 128, 512, 1024 (hard-coded there; a field here so that tests can run narrow) */
    int32_t kernel_size;                     /* 5 */
    int32_t stride;                          /* 3 */
    float slope;                             /* LRELU_SLOPE = 0.1 */
} parrot_mpd_cfg;
/* DEVICE pointers of every parameter, or of every gradient: layer[i][l] is discriminators.i.convs.l, l = 5: conv_post */
typedef struct {
    parrot_voc_layer_ptrs layer[PARROT_MPD_MAX_PERIODS][PARROT_MPD_LAYERS];
} parrot_mpd_ptrs;
typedef struct {
    float* map[PARROT_MPD_MAX_PERIODS][PARROT_MPD_LAYERS];
} parrot_mpd_maps;
/* Rows H_l of map `layer` of period index `period` for rows of T samples; 0 beyond the limits. */
int64_t parrot_mpd_train_map_rows(const parrot_mpd_cfg* cfg, int32_t T, int32_t period, int32_t layer);
/* Bytes of what the forward keeps besides the maps, and of the workspace of either call (0 beyond the limits). */
size_t parrot_mpd_train_saved_bytes(const parrot_mpd_cfg* cfg, int32_t N, int32_t T);
size_t parrot_mpd_train_workspace_bytes(const parrot_mpd_cfg* cfg, int32_t N, int32_t T);
int parrot_mpd_train_forward(const parrot_mpd_cfg* cfg, const parrot_mpd_ptrs* w, const float* wav, int32_t N, int32_t T,
                             const parrot_mpd_maps* maps, void* saved, void* ws, size_t ws_bytes, void* stream);
int parrot_mpd_train_backward(const parrot_mpd_cfg* cfg, const parrot_mpd_ptrs* w, const float* wav, const parrot_mpd_maps* maps,
                              const void* saved, const parrot_mpd_maps* grad_maps, int32_t N, int32_t T, const parrot_mpd_ptrs* grads,
                              float* grad_wav, void* ws, size_t ws_bytes, void* stream);

/* ---- training the multi-scale discriminator (utils/vocoder/models.py:228-276; train.py:142-143, :160-164) ----
 * MultiScaleDiscriminator.forward and its full backward as two stateless calls shaped like the multi-period discriminator's.
 *   forward: wav (N, 1, T) f32, N = 2 B even: the caller stacks real rows [0, B) and generated rows [B, 2 B).  Scale i sees the
 *   waveform after i AvgPool1d(4, 2, padding=2) (length T / 2 + 1 each time, always divided by 4).  Every scale is convs[0] (1 -> c0, 15
 *   taps, padding 7), convs[1 .. 5] (41 taps, padding 20, strides 2, 2, 4, 4, 1, groups[l]), convs[6] (5 taps, padding 2), each with bias
 *   and leaky ReLU `slope`, and conv_post (c6 -> 1, 3 taps, padding 1, no activation).  Weights are torch's: (C_out, C_in / groups, k).
 *   A layer is one of: plain (v = weight), weight-normed (v, g) or spectral-normed (v = weight_orig, u, sv = the buffers weight_u and
 *   weight_v); cfg->spectral[i] says which scales are spectral, and every layer of such a scale must carry u and sv.
 *   Spectral norm: sigma = u^T (W v) with W = weight_orig as (C_out, C_in / groups k); the layer runs on W / sigma.  The reference calls
 *   the discriminator once on the real and once on the generated rows, and a call in training mode starts with one power iteration
 *   (v = normalize(W^T u), u = normalize(W v), eps 1e-12): with power_iterations = 1 the real rows run on the fold after one iteration, the
 *   generated rows on the fold after two, and u and sv are UPDATED IN PLACE, two iterations on.  With power_iterations = 0 (eval) the
 *   buffers are read only and both halves use one sigma.
 *   Maps: the caller owns the eight maps of every scale, map[i][l] a dense (N, C_l, L_l) array, L_l = parrot_msd_train_map_len(cfg, T, i, l);
 *   the score is the flattened eighth.  They are also what the backward reads and must reach it unchanged.
 *   saved (parrot_msd_train_saved_bytes; NULL = keep nothing): the pooled waveforms, every layer's weight-norm row norms and folded
 *   weight and, per spectral layer, both folded weights and both (u, v, sigma) triples -- the caller's buffers have moved on by the
 *   time the backward runs.
 * backward: grad_maps as in parrot_mpd_train_backward.  Outputs: the gradient of every parameter named in `grads` (v, g, bias; u and sv
 *   are ignored; a null field is neither wanted nor computed) and, when grad_wav != NULL, d wav (N, 1, T): scale 0's gradient plus the
 *   pool's backward of the scales below, chained.  Through sigma the backward treats u and v as constants:
 *   d weight_orig = G_r / s1 - (<G_r, W> / s1^2) u1 v1^T + G_g / s2 - (<G_g, W> / s2^2) u2 v2^T.
 * Numerics: the generator's contract.  Limits (PARROT_E_INVALID, before any HIP call): 1 to 4 scales; N even, 2 <= N <= 65534; T >= 1;
 * widths >= 1, each a multiple of its groups; groups[0] = groups[6] = 1; power_iterations 0 or 1; every map below 2^30 elements and
 * N L <= 65535 x 256 at the grouped layers; a null parameter or map, a spectral layer without u / sv or with g; a workspace that is
 * too small is PARROT_E_NOMEM. */
#define PARROT_MSD_MAX_SCALES 4
#define PARROT_MSD_LAYERS 8 /* convs[0 .. 7), conv_post */
typedef struct {
    int32_t n_scales;                        /* reference: 3 */
    int32_t spectral[PARROT_MSD_MAX_SCALES]; /* reference: 1, 0, 0 */
    int32_t channels[7];                     /* reference: 128, 128, 256, 512, 1024, 1024, 1024 (hard-coded there; tests run narrow) */
    int32_t groups[7];                       /* reference: 1, 4, 16, 16, 16, 16, 1 */
    float slope;                             /* LRELU_SLOPE = 0.1 */
} parrot_msd_cfg;
typedef struct {
    float *v, *g, *bias, *u, *sv;
} parrot_msd_layer_ptrs;
/* DEVICE pointers of every parameter, or of every gradient: layer[i][l] is discriminators.i.convs.l, l = 7: conv_post */
typedef struct {
    parrot_msd_layer_ptrs layer[PARROT_MSD_MAX_SCALES][PARROT_MSD_LAYERS];
} parrot_msd_ptrs;
typedef struct {
    float* map[PARROT_MSD_MAX_SCALES][PARROT_MSD_LAYERS];
} parrot_msd_maps;
/* Length L_l of map `layer` of scale `scale` for rows of T samples; 0 beyond the limits. */
int64_t parrot_msd_train_map_len(const parrot_msd_cfg* cfg, int32_t T, int32_t scale, int32_t layer);
size_t parrot_msd_train_saved_bytes(const parrot_msd_cfg* cfg, int32_t N, int32_t T);
size_t parrot_msd_train_workspace_bytes(const parrot_msd_cfg* cfg, int32_t N, int32_t T);
int parrot_msd_train_forward(const parrot_msd_cfg* cfg, const parrot_msd_ptrs* w, const float* wav, int32_t N, int32_t T,
                             int32_t power_iterations, const parrot_msd_maps* maps, void* saved, void* ws, size_t ws_bytes, void* stream);
int parrot_msd_train_backward(const parrot_msd_cfg* cfg, const parrot_msd_ptrs* w, const float* wav, const parrot_msd_maps* maps,
                              const void* saved, const parrot_msd_maps* grad_maps, int32_t N, int32_t T, const parrot_msd_ptrs* grads,
                              float* grad_wav, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PARROT_HIP_H */
