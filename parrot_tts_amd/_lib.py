"""ctypes binding of libparrot_hip.so (include/parrot_hip.h; test / profiling entry points: include/parrot_hip_debug.h).  Fails loudly when the HIP library
is missing or does not load: there is NO CPU / eager fallback in this package."""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# PARROT_HIP_LIB: kernel-experiment builds of the same library (tools/); the default is the in-tree build
LIB_PATH = os.environ.get("PARROT_HIP_LIB") or os.path.join(HERE, "libparrot_hip.so")

MAX_STAGES, MAX_KERNELS, MAX_DIL = 8, 4, 4
ABI_VERSION = 7  # PARROT_ABI_VERSION of include/parrot_hip.h
c_float_p = C.POINTER(C.c_float)


class ParrotHipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libparrot_hip error {code}: {msg}")
        self.code = code


class ConvDesc(C.Structure):
    _fields_ = [("c_in", C.c_int32), ("c_out", C.c_int32), ("k", C.c_int32), ("dilation", C.c_int32),
                ("padding", C.c_int32), ("transposed", C.c_int32), ("stride", C.c_int32), ("pre_act", C.c_int32),
                ("pre_slope", C.c_float), ("act", C.c_int32), ("tile_cfg", C.c_int32), ("precision", C.c_int32)]


class VocCfg(C.Structure):
    _fields_ = [("num_embeddings", C.c_int32), ("embedding_dim", C.c_int32), ("multispkr", C.c_int32),
                ("n_spkr", C.c_int32), ("model_in_dim", C.c_int32), ("upsample_initial_channel", C.c_int32),
                ("n_stages", C.c_int32), ("upsample_rates", C.c_int32 * MAX_STAGES),
                ("upsample_kernel_sizes", C.c_int32 * MAX_STAGES), ("n_kernels", C.c_int32),
                ("resblock_kernel_sizes", C.c_int32 * MAX_KERNELS), ("n_dil", C.c_int32),
                ("resblock_dilation_sizes", (C.c_int32 * MAX_DIL) * MAX_KERNELS), ("resblock_type", C.c_int32)]


class VocWeights(C.Structure):
    _fields_ = [("dict", c_float_p), ("spkr", c_float_p), ("conv_pre_w", c_float_p), ("conv_pre_b", c_float_p),
                ("ups_w", c_float_p * MAX_STAGES), ("ups_b", c_float_p * MAX_STAGES),
                ("rb_w", C.POINTER(c_float_p)), ("rb_b", C.POINTER(c_float_p)), ("n_rb", C.c_int32),
                ("conv_post_w", c_float_p), ("conv_post_b", c_float_p)]


class TteCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("d_model", "n_filter_ffn", "ffn_k1", "ffn_k2", "max_len", "enc_layers",
                                         "enc_heads", "dec_layers", "dec_heads", "dp_filter", "dp_kernel", "vocab",
                                         "n_speaker", "n_codes")]


class FftWeights(C.Structure):
    _fields_ = [(n, c_float_p) for n in ("qkv", "in_proj", "out_proj", "wo", "conv1_w", "conv1_b", "conv2_w",
                                         "conv2_b", "attn_norm_w", "attn_norm_b", "conv_norm_w", "conv_norm_b")]


class TteWeights(C.Structure):
    _fields_ = [("pe", c_float_p), ("tok_emb", c_float_p), ("speaker_emb", c_float_p),
                ("dp_conv0_w", c_float_p), ("dp_conv0_b", c_float_p), ("dp_ln0_w", c_float_p), ("dp_ln0_b", c_float_p),
                ("dp_conv1_w", c_float_p), ("dp_conv1_b", c_float_p), ("dp_ln1_w", c_float_p), ("dp_ln1_b", c_float_p),
                ("dp_proj_w", c_float_p), ("dp_proj_b", c_float_p),
                ("enc", C.POINTER(FftWeights)), ("dec", C.POINTER(FftWeights)),
                ("head_w", c_float_p), ("head_b", c_float_p)]


class MelCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_fft", "hop", "win", "n_mels")]


class AlignerCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_mels", "num_symbols", "lstm_dim", "conv_dim")] + [("bn_eps", C.c_float)]


class AlignerWeights(C.Structure):
    _fields_ = [(n, c_float_p * 3) for n in ("conv_w", "bn_weight", "bn_bias", "bn_mean", "bn_var")] + \
               [(n, c_float_p * 2) for n in ("w_ih", "w_hh", "b_ih", "b_hh")] + [("lin_w", c_float_p), ("lin_b", c_float_p)]


class AlignerDevWeights(C.Structure):  # parrot_aligner_dev_weights: DEVICE pointers, torch layouts
    _fields_ = [(n, C.c_void_p * 3) for n in ("conv_w", "bn_weight", "bn_bias", "bn_mean", "bn_var")] + \
               [(n, C.c_void_p * 2) for n in ("w_ih", "w_hh", "b_ih", "b_hh")] + [("lin_w", C.c_void_p), ("lin_b", C.c_void_p)]


class AlignerGrads(C.Structure):  # parrot_aligner_grads: where the backward writes; a null field is not computed
    _fields_ = [(n, C.c_void_p * 3) for n in ("conv_w", "bn_weight", "bn_bias")] + \
               [(n, C.c_void_p * 2) for n in ("w_ih", "w_hh", "b_ih", "b_hh")] + [("lin_w", C.c_void_p), ("lin_b", C.c_void_p)]


TTE_TRAIN_MAX_LAYERS = 16  # PARROT_TTE_TRAIN_MAX_LAYERS of include/parrot_hip.h
FFT_FIELDS = ("qkv", "in_proj", "out_proj", "wo", "conv1_w", "conv1_b", "conv2_w", "conv2_b", "attn_norm_w", "attn_norm_b", "conv_norm_w",
              "conv_norm_b")
TTE_TOP_FIELDS = ("pe", "tok_emb", "speaker_emb", "dp_conv0_w", "dp_conv0_b", "dp_ln0_w", "dp_ln0_b", "dp_conv1_w", "dp_conv1_b", "dp_ln1_w",
                  "dp_ln1_b", "dp_proj_w", "dp_proj_b", "head_w", "head_b")


class TteTrainCfg(C.Structure):  # parrot_tte_train_cfg
    _fields_ = [("tte", TteCfg), ("pad_idx", C.c_int32), ("p_enc", C.c_float), ("p_dec", C.c_float), ("p_dp", C.c_float)]


class FftDevPtrs(C.Structure):  # parrot_fft_weights with DEVICE pointers / parrot_fft_grads: the same layout
    _fields_ = [(n, C.c_void_p) for n in FFT_FIELDS]


class TteDevPtrs(C.Structure):  # parrot_tte_dev_weights / parrot_tte_grads: the same layout
    _fields_ = [(n, C.c_void_p) for n in TTE_TOP_FIELDS] + [("enc", FftDevPtrs * TTE_TRAIN_MAX_LAYERS), ("dec", FftDevPtrs * TTE_TRAIN_MAX_LAYERS)]


VOC_TRAIN_MAX_RB = MAX_STAGES * MAX_KERNELS * 2 * MAX_DIL  # PARROT_VOC_TRAIN_MAX_RB of include/parrot_hip.h


class VocLayerPtrs(C.Structure):  # parrot_voc_layer_ptrs: DEVICE pointers of one weight-normed layer (g null: a plain weight in v)
    _fields_ = [("v", C.c_void_p), ("g", C.c_void_p), ("bias", C.c_void_p)]


class VocTrainPtrs(C.Structure):  # parrot_voc_train_ptrs: the parameters, or where the backward writes their gradients
    _fields_ = [("dict", C.c_void_p), ("spkr", C.c_void_p), ("conv_pre", VocLayerPtrs), ("ups", VocLayerPtrs * MAX_STAGES),
                ("rb", VocLayerPtrs * VOC_TRAIN_MAX_RB), ("conv_post", VocLayerPtrs)]


MPD_MAX_PERIODS, MPD_LAYERS = 8, 6  # PARROT_MPD_MAX_PERIODS, PARROT_MPD_LAYERS of include/parrot_hip.h


class MpdCfg(C.Structure):  # parrot_mpd_cfg
    _fields_ = [("n_periods", C.c_int32), ("periods", C.c_int32 * MPD_MAX_PERIODS), ("channels", C.c_int32 * 4), ("kernel_size", C.c_int32),
                ("stride", C.c_int32), ("slope", C.c_float)]


class MpdPtrs(C.Structure):  # parrot_mpd_ptrs: the parameters, or where the backward writes their gradients
    _fields_ = [("layer", (VocLayerPtrs * MPD_LAYERS) * MPD_MAX_PERIODS)]


class MpdMaps(C.Structure):  # parrot_mpd_maps: the six maps of every period, or the gradients that arrive at them
    _fields_ = [("map", (C.c_void_p * MPD_LAYERS) * MPD_MAX_PERIODS)]


MSD_MAX_SCALES, MSD_LAYERS = 4, 8  # PARROT_MSD_MAX_SCALES, PARROT_MSD_LAYERS of include/parrot_hip.h


class MsdCfg(C.Structure):  # parrot_msd_cfg
    _fields_ = [("n_scales", C.c_int32), ("spectral", C.c_int32 * MSD_MAX_SCALES), ("channels", C.c_int32 * 7), ("groups", C.c_int32 * 7),
                ("slope", C.c_float)]


class MsdLayerPtrs(C.Structure):  # parrot_msd_layer_ptrs: v (weight, weight_v or weight_orig), g, bias, and a spectral layer's buffers u, sv
    _fields_ = [("v", C.c_void_p), ("g", C.c_void_p), ("bias", C.c_void_p), ("u", C.c_void_p), ("sv", C.c_void_p)]


class MsdPtrs(C.Structure):  # parrot_msd_ptrs: the parameters, or where the backward writes their gradients
    _fields_ = [("layer", (MsdLayerPtrs * MSD_LAYERS) * MSD_MAX_SCALES)]


class MsdMaps(C.Structure):  # parrot_msd_maps: the eight maps of every scale, or the gradients that arrive at them
    _fields_ = [("map", (C.c_void_p * MSD_LAYERS) * MSD_MAX_SCALES)]


class GanTerm(C.Structure):  # parrot_gan_term_t: 48 bytes
    _fields_ = [("a", C.c_void_p), ("b", C.c_void_p), ("grad_a", C.c_void_p), ("grad_b", C.c_void_p), ("n", C.c_int64),
                ("op", C.c_int32), ("reserved", C.c_int32)]


class AdamwTensor(C.Structure):  # parrot_adamw_tensor_t: 48 bytes
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("n", C.c_int64), ("step", C.c_int64)]


DEBUG_MAX_TAPS = 5  # PARROT_DEBUG_MAX_TAPS of include/parrot_hip_debug.h


class DebugBuf(C.Structure):  # parrot_debug_buf: a DEVICE buffer and the number of floats behind the pointer
    _fields_ = [("p", C.c_void_p), ("n", C.c_int64)]


class DebugTapGemmDesc(C.Structure):
    _fields_ = [("A", DebugBuf * DEBUG_MAX_TAPS), ("x_off", C.c_int64 * DEBUG_MAX_TAPS), ("shift", C.c_int32 * DEBUG_MAX_TAPS),
                ("ntaps", C.c_int32)] + [(n, DebugBuf) for n in ("X", "C", "bias0", "bias1")] + \
               [(n, C.c_int32) for n in ("M", "N", "K", "Z")] + \
               [(n, C.c_int64) for n in ("a_sm", "a_sk", "x_sz", "x_sk", "x_sn", "c_sz", "c_sm", "c_sn")] + [("relu", C.c_int32)]


class DebugWgradDesc(C.Structure):
    _fields_ = [(n, DebugBuf) for n in ("dY", "X", "out")] + [(n, C.c_int32) for n in ("M", "K", "T", "R", "ntaps")] + \
               [("shift", C.c_int32 * DEBUG_MAX_TAPS)] + \
               [(n, C.c_int64) for n in ("y_sz", "y_sm", "y_st", "x_sz", "x_sk", "x_st", "o_sm", "o_sk", "o_sj")]


class DebugColsumDesc(C.Structure):
    _fields_ = [(n, DebugBuf) for n in ("src", "out0", "out1")] + [("R", C.c_int32), ("M", C.c_int32), ("ld", C.c_int64)]


class DebugBnTrainDesc(C.Structure):
    _fields_ = [(n, DebugBuf) for n in ("x", "y", "gamma", "beta", "run_mean", "run_var", "mean", "invstd")] + \
               [(n, C.c_int32) for n in ("B", "C", "T", "training")] + [("eps", C.c_float)]


class DebugBnBwdDesc(C.Structure):
    _fields_ = [(n, DebugBuf) for n in ("dy", "x", "dx", "gamma", "mean", "invstd", "dgamma", "dbeta")] + \
               [(n, C.c_int32) for n in ("B", "C", "T")]


GAN_L1, GAN_SQ1, GAN_SQ0 = 0, 1, 2  # PARROT_GAN_* of include/parrot_hip.h
GAN_MAX_TERMS, GAN_GRID_CAP = 64, 2048  # PARROT_GAN_MAX_TERMS, PARROT_GAN_GRID_CAP

# name -> (restype, argtypes); every symbol include/parrot_hip.h and include/parrot_hip_debug.h declare
vp, i32, sz, f32 = C.c_void_p, C.c_int32, C.c_size_t, C.c_float
SIGNATURES = {
    "parrot_abi_version": (C.c_int, []),
    "parrot_last_error": (C.c_char_p, []),
    "parrot_selftest": (C.c_int, [vp]),
    "parrot_set_default_precision": (C.c_int, [i32]),
    "parrot_set_fused_resblocks": (C.c_int, [i32]),
    "parrot_set_tte_merge": (C.c_int, [i32]),
    "parrot_conv_create": (C.c_int, [C.POINTER(vp), C.POINTER(ConvDesc), c_float_p, c_float_p]),
    "parrot_conv_destroy": (None, [vp]),
    "parrot_conv_run": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, f32, vp]),
    "parrot_conv_out_len": (C.c_int, [vp, i32]),
    "parrot_conv_num_tile_cfgs": (C.c_int, []),
    "parrot_debug_copy": (C.c_int, [vp, vp, sz, vp]),
    "parrot_debug_mfma_ceiling": (C.c_int, [i32, i32, C.POINTER(C.c_double)]),
    "parrot_prof_begin": (C.c_int, []),
    "parrot_prof_begin_row": (C.c_int, [i32]),
    "parrot_prof_end": (C.c_int, [C.POINTER(C.c_double), i32]),
    "parrot_voc_create": (C.c_int, [C.POINTER(vp), C.POINTER(VocCfg), C.POINTER(VocWeights)]),
    "parrot_voc_create_ex": (C.c_int, [C.POINTER(vp), C.POINTER(VocCfg), C.POINTER(VocWeights), i32, i32]),
    "parrot_voc_destroy": (None, [vp]),
    "parrot_voc_precision": (C.c_int, [vp]),
    "parrot_voc_debug_absmax": (C.c_int, [vp, vp]),
    "parrot_voc_workspace_bytes": (sz, [vp, i32, i32]),
    "parrot_voc_forward": (C.c_int, [vp, vp, vp, vp, i32, i32, vp, C.POINTER(vp), vp, sz, vp]),
    "parrot_voc_forward_feats": (C.c_int, [vp, vp, vp, vp, i32, vp, i32, i32, vp, C.POINTER(vp), vp, sz, vp]),
    "parrot_voc_chunked_workspace_bytes": (sz, [vp, i32, i32, i32]),
    "parrot_voc_forward_chunked": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, sz, vp]),
    "parrot_voc_check": (C.c_int, [vp, vp]),
    "parrot_voc_status_async": (C.c_int, [vp, vp, vp]),
    "parrot_voc_status_peek_async": (C.c_int, [vp, vp, vp]),
    "parrot_voc_receptive_units": (C.c_int, [vp]),
    "parrot_voc_wait_stage": (C.c_int, [vp, C.c_int32, vp]),
    "parrot_voc_out_len": (C.c_int64, [vp, i32]),
    "parrot_wav_to_int16": (C.c_int, [vp, vp, sz, vp]),
    "parrot_tte_create": (C.c_int, [C.POINTER(vp), C.POINTER(TteCfg), C.POINTER(TteWeights)]),
    "parrot_tte_create_ex": (C.c_int, [C.POINTER(vp), C.POINTER(TteCfg), C.POINTER(TteWeights), i32, i32]),
    "parrot_tte_destroy": (None, [vp]),
    "parrot_tte_precision": (C.c_int, [vp]),
    "parrot_tte_guard_logits": (C.c_int, [vp, vp, vp, i32, vp]),
    "parrot_tte_state_bytes": (sz, [vp, i32, i32]),
    "parrot_tte_workspace_bytes": (sz, [vp, i32, i32, i32]),
    "parrot_tte_encode": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, sz, vp, sz, vp]),
    "parrot_tte_decode": (C.c_int, [vp, i32, i32, i32, i32, vp, vp, vp, vp, sz, vp, sz, vp]),
    "parrot_tte_set_durations": (C.c_int, [vp, vp, i32, i32, vp, vp, vp, sz, vp]),
    "parrot_tte_decode_masked": (C.c_int, [vp, i32, i32, i32, i32, vp, vp, vp, vp, sz, vp, sz, vp]),
    "parrot_tte_loss_workspace_bytes": (sz, [i32]),
    "parrot_tte_loss": (C.c_int, [vp, vp, i32, i32, C.c_int64, vp, vp, vp, i32, vp, vp, vp, sz, vp]),
    "parrot_tte_loss_grad_workspace_bytes": (sz, [i32]),
    "parrot_tte_loss_grad": (C.c_int, [vp, vp, i32, i32, C.c_int64, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, sz, vp]),
    "parrot_tte_check": (C.c_int, [vp, vp]),
    "parrot_tte_status_async": (C.c_int, [vp, vp, vp]),
    "parrot_tte_status_peek_async": (C.c_int, [vp, vp, vp]),
    "parrot_tte_guard_stats_async": (C.c_int, [vp, vp, vp]),
    "parrot_tte_debug_stages": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp)]),
    "parrot_debug_attention_workspace_bytes": (sz, [i32, i32, i32, i32]),
    "parrot_debug_attention": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, i32, vp, sz, vp]),
    "parrot_debug_layernorm": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "parrot_debug_durations": (C.c_int, [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]),
    "parrot_debug_length_regulate": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]),
    "parrot_debug_argmax_guard": (C.c_int, [vp, i32, i32, i32, f32, i32, vp, i32, vp, vp, vp, vp, vp, vp, i32, C.POINTER(i32), vp, vp, vp, vp,
                                            vp, vp]),
    "parrot_length_regulator_workspace_bytes": (sz, [i32, i32, i32, i32]),
    "parrot_length_regulator": (C.c_int, [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, sz, vp]),
    "parrot_mel_create": (C.c_int, [C.POINTER(vp), C.POINTER(MelCfg), c_float_p, c_float_p]),
    "parrot_mel_create_ex": (C.c_int, [C.POINTER(vp), C.POINTER(MelCfg), c_float_p, c_float_p, i32]),
    "parrot_mel_destroy": (None, [vp]),
    "parrot_mel_precision": (C.c_int, [vp]),
    "parrot_mel_frames": (C.c_int, [vp, i32]),
    "parrot_mel_workspace_bytes": (sz, [vp, i32, i32]),
    "parrot_mel_forward": (C.c_int, [vp, vp, C.c_int64, vp, i32, i32, vp, vp, sz, vp]),
    "parrot_mel_l1_workspace_bytes": (sz, [i32, i32, i32]),
    "parrot_mel_l1": (C.c_int, [vp, vp, vp, i32, i32, i32, vp, vp, vp, sz, vp]),
    "parrot_mel_l1_grad_workspace_bytes": (sz, [vp, i32, i32]),
    "parrot_mel_l1_grad": (C.c_int, [vp, vp, C.c_int64, vp, vp, i32, i32, i32, C.c_double, vp, vp, vp, vp, sz, vp]),
    "parrot_mel_check": (C.c_int, [vp, vp]),
    "parrot_mel_status_async": (C.c_int, [vp, vp, vp]),
    "parrot_aligner_create": (C.c_int, [C.POINTER(vp), C.POINTER(AlignerCfg), C.POINTER(AlignerWeights)]),
    "parrot_aligner_create_ex": (C.c_int, [C.POINTER(vp), C.POINTER(AlignerCfg), C.POINTER(AlignerWeights), i32]),
    "parrot_aligner_destroy": (None, [vp]),
    "parrot_aligner_precision": (C.c_int, [vp]),
    "parrot_aligner_debug_stages": (C.c_int, [vp, vp, vp]),
    "parrot_aligner_workspace_bytes": (sz, [vp, i32, i32]),
    "parrot_aligner_forward": (C.c_int, [vp, vp, i32, i32, vp, vp, sz, vp]),
    "parrot_align_softmax": (C.c_int, [vp, vp, vp, i32, i32, vp, vp]),
    "parrot_aligner_check": (C.c_int, [vp, vp]),
    "parrot_aligner_status_async": (C.c_int, [vp, vp, vp]),
    "parrot_align_workspace_bytes": (sz, [i32, i32, i32]),
    "parrot_align_durations": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, sz, vp]),
    "parrot_ctc_workspace_bytes": (sz, [i32, i32, i32]),
    "parrot_ctc_loss": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, sz, vp]),
    "parrot_ctc_grad_workspace_bytes": (sz, [i32, i32, i32, i32]),
    "parrot_ctc_loss_grad": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, vp, i32, vp, vp, vp, sz, vp]),
    "parrot_aligner_train_saved_bytes": (sz, [C.POINTER(AlignerCfg), i32, i32]),
    "parrot_aligner_train_workspace_bytes": (sz, [C.POINTER(AlignerCfg), i32, i32]),
    "parrot_aligner_train_forward": (C.c_int, [C.POINTER(AlignerCfg), C.POINTER(AlignerDevWeights), vp, i32, i32, i32, vp, vp, vp, sz, vp]),
    "parrot_aligner_train_backward": (C.c_int, [C.POINTER(AlignerCfg), C.POINTER(AlignerDevWeights), vp, vp, vp, i32, i32,
                                                C.POINTER(AlignerGrads), vp, sz, vp]),
    "parrot_tte_train_saved_bytes": (sz, [C.POINTER(TteTrainCfg), i32, i32, i32]),
    "parrot_tte_train_workspace_bytes": (sz, [C.POINTER(TteTrainCfg), i32, i32, i32]),
    "parrot_tte_train_forward": (C.c_int, [C.POINTER(TteTrainCfg), C.POINTER(TteDevPtrs), vp, vp, vp, vp, vp, i32, i32, i32, i32, C.c_uint64,
                                           C.c_uint64, vp, vp, vp, vp, sz, vp]),
    "parrot_tte_train_backward": (C.c_int, [C.POINTER(TteTrainCfg), C.POINTER(TteDevPtrs), vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32,
                                            C.c_uint64, C.c_uint64, C.POINTER(TteDevPtrs), vp, sz, vp]),
    "parrot_tte_train_dropout_mask": (C.c_int, [C.c_uint64, C.c_uint64, i32, C.c_int64, f32, vp, vp]),
    "parrot_debug_tte_ln_fwd": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int64, i32, vp]),
    "parrot_debug_tte_ln_bwd": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, C.c_int64, i32, i32, vp]),
    "parrot_debug_tte_softmax_drop_fwd": (C.c_int, [vp, vp, vp, i32, i32, i32, f32, C.c_uint64, C.c_uint64, i32, vp]),
    "parrot_debug_tte_softmax_drop_bwd": (C.c_int, [vp, vp, i32, i32, i32, f32, C.c_uint64, C.c_uint64, i32, vp]),
    "parrot_debug_tte_dropout": (C.c_int, [vp, vp, C.c_int64, f32, C.c_uint64, C.c_uint64, i32, vp]),
    "parrot_debug_tte_lr_bwd": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "parrot_debug_tte_embed_grad": (C.c_int, [vp, vp, vp, C.c_int64, i32, i32, i32, i32, vp]),
    "parrot_debug_tte_conv_dw_workspace_bytes": (sz, [i32, i32, i32, i32, i32, i32]),
    "parrot_debug_tte_conv_dw": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, sz, vp]),
    "parrot_voc_train_out_len": (C.c_int64, [C.POINTER(VocCfg), i32]),
    "parrot_voc_train_saved_bytes": (sz, [C.POINTER(VocCfg), i32, i32]),
    "parrot_voc_train_workspace_bytes": (sz, [C.POINTER(VocCfg), i32, i32]),
    "parrot_voc_train_forward": (C.c_int, [C.POINTER(VocCfg), C.POINTER(VocTrainPtrs), vp, vp, i32, i32, vp, vp, vp, sz, vp]),
    "parrot_voc_train_backward": (C.c_int, [C.POINTER(VocCfg), C.POINTER(VocTrainPtrs), vp, vp, vp, vp, i32, i32, C.POINTER(VocTrainPtrs), vp,
                                            sz, vp]),
    "parrot_voc_train_lrelu_sites": (i32, [C.POINTER(VocCfg)]),
    "parrot_voc_train_lrelu_site_elems": (C.c_int64, [C.POINTER(VocCfg), i32, i32, i32]),
    "parrot_voc_train_lrelu_mask": (C.c_int, [C.POINTER(VocCfg), i32, i32, vp, i32, vp, vp]),
    "parrot_debug_voc_conv_fwd": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
    "parrot_debug_voc_conv_dx": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
    "parrot_debug_voc_conv_dw_workspace_bytes": (sz, [i32, i32, i32, i32, i32]),
    "parrot_debug_voc_conv_dw": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, sz, vp]),
    "parrot_debug_voc_wn_fwd": (C.c_int, [vp, vp, vp, vp, i32, i32, vp]),
    "parrot_debug_voc_wn_bwd": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, i32, vp]),
    "parrot_mpd_train_map_rows": (C.c_int64, [C.POINTER(MpdCfg), i32, i32, i32]),
    "parrot_mpd_train_saved_bytes": (sz, [C.POINTER(MpdCfg), i32, i32]),
    "parrot_mpd_train_workspace_bytes": (sz, [C.POINTER(MpdCfg), i32, i32]),
    "parrot_mpd_train_forward": (C.c_int, [C.POINTER(MpdCfg), C.POINTER(MpdPtrs), vp, i32, i32, C.POINTER(MpdMaps), vp, vp, sz, vp]),
    "parrot_mpd_train_backward": (C.c_int, [C.POINTER(MpdCfg), C.POINTER(MpdPtrs), vp, C.POINTER(MpdMaps), vp, C.POINTER(MpdMaps), i32, i32,
                                            C.POINTER(MpdPtrs), vp, vp, sz, vp]),
    "parrot_debug_mpd_conv_fwd": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, f32, vp]),
    "parrot_debug_mpd_conv_dx": (C.c_int, [vp, vp, vp, vp, f32, vp, i32, i32, i32, i32, i32, i32, vp]),
    "parrot_debug_mpd_conv_dw_workspace_bytes": (sz, [i32, i32, i32, i32, i32, i32]),
    "parrot_debug_mpd_conv_dw": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, sz, vp]),
    "parrot_debug_mpd_first_fwd": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, vp]),
    "parrot_debug_mpd_first_dx": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "parrot_debug_mpd_first_dw_workspace_bytes": (sz, [i32, i32, i32, i32, i32, i32]),
    "parrot_debug_mpd_first_dw": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, sz, vp]),
    "parrot_debug_mpd_post_fwd": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, vp]),
    "parrot_debug_mpd_post_dx": (C.c_int, [vp, vp, vp, vp, f32, vp, i32, i32, i32, vp]),
    "parrot_debug_mpd_post_dw_workspace_bytes": (sz, [i32, i32, i32]),
    "parrot_debug_mpd_post_dw": (C.c_int, [vp, vp, vp, i32, i32, i32, vp, sz, vp]),
    "parrot_msd_train_map_len": (C.c_int64, [C.POINTER(MsdCfg), i32, i32, i32]),
    "parrot_msd_train_saved_bytes": (sz, [C.POINTER(MsdCfg), i32, i32]),
    "parrot_msd_train_workspace_bytes": (sz, [C.POINTER(MsdCfg), i32, i32]),
    "parrot_msd_train_forward": (C.c_int, [C.POINTER(MsdCfg), C.POINTER(MsdPtrs), vp, i32, i32, i32, C.POINTER(MsdMaps), vp, vp, sz, vp]),
    "parrot_msd_train_backward": (C.c_int, [C.POINTER(MsdCfg), C.POINTER(MsdPtrs), vp, C.POINTER(MsdMaps), vp, C.POINTER(MsdMaps), i32, i32,
                                            C.POINTER(MsdPtrs), vp, vp, sz, vp]),
    "parrot_debug_msd_gconv_fwd": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, f32, vp]),
    "parrot_debug_msd_gconv_dx": (C.c_int, [vp, vp, vp, vp, f32, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
    "parrot_debug_msd_gconv_dw_workspace_bytes": (sz, [i32, i32, i32, i32, i32, i32, i32]),
    "parrot_debug_msd_gconv_dw": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, sz, vp]),
    "parrot_debug_msd_first_fwd": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, f32, vp]),
    "parrot_debug_msd_first_dx": (C.c_int, [vp, vp, vp, i32, i32, i32, vp]),
    "parrot_debug_msd_first_dw_workspace_bytes": (sz, [i32, i32, i32]),
    "parrot_debug_msd_first_dw": (C.c_int, [vp, vp, vp, i32, i32, i32, vp, sz, vp]),
    "parrot_debug_msd_pool_fwd": (C.c_int, [vp, vp, i32, i32, vp]),
    "parrot_debug_msd_pool_bwd": (C.c_int, [vp, vp, i32, i32, vp]),
    "parrot_debug_msd_sn_fold": (C.c_int, [vp, vp, vp, i32, i32, i32, vp, vp, vp, sz, vp]),
    "parrot_debug_msd_sn_bwd_workspace_bytes": (sz, [i32, i32]),
    "parrot_debug_msd_sn_bwd": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, sz, vp]),
    "parrot_debug_tap_gemm": (C.c_int, [C.POINTER(DebugTapGemmDesc), vp]),
    "parrot_debug_wgrad_workspace_bytes": (sz, [i32, i32, i32, i32]),
    "parrot_debug_wgrad": (C.c_int, [C.POINTER(DebugWgradDesc), vp, sz, vp]),
    "parrot_debug_colsum_workspace_bytes": (sz, [i32, i32]),
    "parrot_debug_colsum": (C.c_int, [C.POINTER(DebugColsumDesc), vp, sz, vp]),
    "parrot_debug_bn_train": (C.c_int, [C.POINTER(DebugBnTrainDesc), vp]),
    "parrot_debug_bn_relu_bwd": (C.c_int, [C.POINTER(DebugBnBwdDesc), vp]),
    "parrot_debug_lstm_workspace_bytes": (sz, [i32, i32, i32, i32]),
    "parrot_debug_lstm": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, sz, vp]),
    "parrot_gan_loss_tile": (i32, []),
    "parrot_gan_loss_workspace_bytes": (sz, [C.POINTER(GanTerm), i32]),
    "parrot_gan_loss": (C.c_int, [C.POINTER(GanTerm), i32, vp, C.c_double, vp, vp, vp, sz, vp]),
    "parrot_adamw_step": (C.c_int, [C.POINTER(AdamwTensor), i32, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, vp]),
    "parrot_adamw_chunk": (i32, []),
    "parrot_adamw_max_tensors": (i32, []),
}

_lib = None


def lib() -> C.CDLL:
    """Load (once) and return the bound library; raises if it is absent -- never falls back."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `python -m parrot_tts_amd.build` (hipcc, gfx950). "
                              "parrot_tts_amd has no CPU fallback.")
        # torch first, always: it brings its own HIP runtime, and the library must bind to THAT copy -- loaded the other
        # way round (e.g. __graft_entry__.build() before the first `import torch`) the process ends up with two
        # runtimes and the second one sees no device
        import torch  # noqa: F401
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype, fn.argtypes = res, args
        if handle.parrot_abi_version() != ABI_VERSION:
            raise ImportError("libparrot_hip.so ABI version mismatch")
        _lib = handle
    return _lib


def check(code: int) -> None:
    if code != 0:
        raise ParrotHipError(code, lib().parrot_last_error().decode())


E_RANGE, E_NONFINITE = -2, -6  # PARROT_E_RANGE, PARROT_E_NONFINITE of include/parrot_hip.h
ST_NONFINITE = 5  # device status word of every handle kind: a non-finite output (csrc/tte_glue.h, aligner.h, mel.h)


def reraise(e: ParrotHipError, on_nonfinite=None):
    """Inside ``except ParrotHipError as e``: PARROT_E_RANGE <-> the reference's IndexError (pe[T], Embedding), PARROT_E_NONFINITE
    (a flag raised by an earlier run) -> FloatingPointError, same message, chain suppressed; anything else is raised as it is.
    ``on_nonfinite``: called before the FloatingPointError is raised."""
    if e.code == E_RANGE:
        raise IndexError(str(e)) from None
    if e.code == E_NONFINITE:
        if on_nonfinite is not None:
            on_nonfinite()
        raise FloatingPointError(str(e)) from None
    raise e


def destroy(fn_name: str, handle) -> None:
    """The one guarded destroy (invalidation and every ``__del__``): nothing for a null handle, and nothing once module globals
    are gone -- `_lib` is None again while the interpreter tears down (and a live handle means the library was loaded).
    At that time the CALLER's globals are going too, this function among them: a ``__del__`` reaches it through a default
    argument bound at definition time (``_destroy=_lib.destroy``), never through its module's global ``_lib``."""
    if handle and _lib is not None:
        getattr(_lib, fn_name)(handle)


def fptr(t):
    """Host fp32 pointer of a contiguous CPU float tensor (caller keeps `t` alive)."""
    assert t.device.type == "cpu" and t.dtype.is_floating_point and t.is_contiguous()
    return C.cast(t.data_ptr(), c_float_p)
