"""Training the text-to-unit model on the GPU: ``TrainableParrot``, the reference's ``Parrot`` (modules/parrot.py:12-110) under
``model.train()`` -- dropout included -- with its whole backward, backed by libparrot_hip.so (``parrot_tte_train_forward`` /
``parrot_tte_train_backward``).

    TrainableParrot(data_config, src_vocab_size, src_pad_idx)    the reference's constructor (reads <root_path>/speakers.json),
                                                                 state_dict keys and shapes; ``pos_emb.pe`` is a buffer
    .forward(batch) -> (out, src_mask, tgt_mask, log_dur_preds)  train mode with grad enabled: dropout on the attention
                                                                 probabilities and in the duration predictor, one autograd node
                                                                 over all parameters; .eval() or no_grad: the same kernels
                                                                 without dropout, no graph

The parameters are real ``nn.Parameter``s on the device and the library reads them where they live: an optimiser's in-place step is
seen by the next forward with nothing rebuilt or copied.  A state dict moves freely between this module, the reference's ``Parrot``
and the inference ``Parrot`` of tte.py.  Dropout bits come from a counter-based generator keyed by (seed, offset, site, element):
the seed is ``torch.initial_seed()`` at the first training forward, the offset a step counter that advances on every training
forward (not part of the state dict), so ``torch.manual_seed(42)`` reproduces a run; nothing accumulates atomically, and
``torch.use_deterministic_algorithms(True)`` is supported.  There is no CPU path: a CPU tensor raises, as in the other shims."""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import List, Optional

import torch
from torch import nn

from . import _lib
from ._handle import _attach
from .ops import _workspace, dptr, require_cuda, stream_ptr
from .synth import sinusoid_table
from .tte import parrot_param_shapes

_TOP = {"tok_emb.weight": "tok_emb", "speaker_emb.weight": "speaker_emb",
        "duration_predictor.layers.0.conv.weight": "dp_conv0_w", "duration_predictor.layers.0.conv.bias": "dp_conv0_b",
        "duration_predictor.layers.2.weight": "dp_ln0_w", "duration_predictor.layers.2.bias": "dp_ln0_b",
        "duration_predictor.layers.4.conv.weight": "dp_conv1_w", "duration_predictor.layers.4.conv.bias": "dp_conv1_b",
        "duration_predictor.layers.6.weight": "dp_ln1_w", "duration_predictor.layers.6.bias": "dp_ln1_b",
        "duration_predictor.proj.weight": "dp_proj_w", "duration_predictor.proj.bias": "dp_proj_b",
        "head.weight": "head_w", "head.bias": "head_b"}
_FFT = {"attention.qkv.weight": "qkv", "attention.mha.in_proj_weight": "in_proj", "attention.mha.out_proj.weight": "out_proj",
        "attention.wo.weight": "wo", "convlayer.conv1.weight": "conv1_w", "convlayer.conv1.bias": "conv1_b",
        "convlayer.conv2.weight": "conv2_w", "convlayer.conv2.bias": "conv2_b", "attn_norm.weight": "attn_norm_w",
        "attn_norm.bias": "attn_norm_b", "conv_norm.weight": "conv_norm_w", "conv_norm.bias": "conv_norm_b"}


def _set(struct, key: str, tensor) -> None:
    """Put ``tensor``'s device pointer (None: null) into the field of a TteDevPtrs that belongs to state_dict key ``key``."""
    ptr = None if tensor is None else tensor.data_ptr()
    if key in _TOP:
        setattr(struct, _TOP[key], ptr)
        return
    side, n, leaf = key.split(".", 2)
    setattr(getattr(struct, "enc" if side == "encoder_layers" else "dec")[int(n)], _FFT[leaf], ptr)


def _dev_weights(keys, params, pe) -> "_lib.TteDevPtrs":
    w = _lib.TteDevPtrs()
    w.pe = pe.data_ptr()
    for k, p in zip(keys, params):
        _set(w, k, p)
    return w


def _train_forward(cfg, keys, params, pe, batch_t, L: int, training: bool, seed: int, offset: int):
    """One parrot_tte_train_forward call on validated tensors -> (logits, log_dur, saved buffer or None)."""
    phones, src_mask, speaker, duration, tgt_mask = batch_t
    dev = phones.device
    B, S = int(phones.shape[0]), int(phones.shape[1])
    lib = _lib.lib()
    logits = torch.empty((B, L, cfg.tte.n_codes), dtype=torch.float32, device=dev)
    log_dur = torch.empty((B, S), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        n_ws = int(lib.parrot_tte_train_workspace_bytes(C.byref(cfg), B, S, L))
        n_sv = int(lib.parrot_tte_train_saved_bytes(C.byref(cfg), B, S, L))
        ws = _workspace(n_ws, dev)  # (0 bytes beyond the limits: the call then fails at the library's own shape check)
        saved = _workspace(n_sv, dev) if training else None
        w = _dev_weights(keys, params, pe)
        try:
            _lib.check(lib.parrot_tte_train_forward(C.byref(cfg), C.byref(w), dptr(phones), dptr(src_mask), dptr(speaker), dptr(duration),
                                                    dptr(tgt_mask), B, S, L, int(training), seed, offset, dptr(logits), dptr(log_dur),
                                                    dptr(saved), dptr(ws), n_ws, stream_ptr(dev)))
        except _lib.ParrotHipError as e:
            _lib.reraise(e)
    return logits, log_dur, saved


class _ParrotTrainFn(torch.autograd.Function):
    """forward(cfg, keys, pe, batch tensors, L, seed, offset, *parameters): one training forward, which owns the ``saved`` buffer;
    backward: one parrot_tte_train_backward call.  A parameter that needs no gradient gets none (its field is null and is not
    computed), and there is no double backward."""

    @staticmethod
    def forward(ctx, cfg, keys, pe, batch_t, L, seed, offset, *params):
        logits, log_dur, saved = _train_forward(cfg, keys, params, pe, batch_t, L, True, seed, offset)
        ctx.save_for_backward(*params)
        ctx.cfg, ctx.keys, ctx.pe, ctx.batch_t, ctx.L, ctx.seed, ctx.offset, ctx.saved = cfg, keys, pe, batch_t, L, seed, offset, saved
        return logits, log_dur

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_logits, grad_log_dur):
        params = ctx.saved_tensors
        phones, src_mask, speaker, duration, tgt_mask = ctx.batch_t
        dev = phones.device
        B, S, L = int(phones.shape[0]), int(phones.shape[1]), ctx.L
        lib = _lib.lib()
        grad_logits = None if grad_logits is None else grad_logits.to(torch.float32).contiguous()
        grad_log_dur = None if grad_log_dur is None else grad_log_dur.to(torch.float32).contiguous()
        grads = [torch.empty_like(p) if need else None for p, need in zip(params, ctx.needs_input_grad[7:])]
        g = _lib.TteDevPtrs()
        for k, t in zip(ctx.keys, grads):
            _set(g, k, t)
        with torch.cuda.device(dev):
            n_ws = int(lib.parrot_tte_train_workspace_bytes(C.byref(ctx.cfg), B, S, L))
            ws = _workspace(n_ws, dev)
            w = _dev_weights(ctx.keys, params, ctx.pe)
            _lib.check(lib.parrot_tte_train_backward(C.byref(ctx.cfg), C.byref(w), dptr(phones), dptr(src_mask), dptr(speaker), dptr(duration),
                                                     dptr(tgt_mask), dptr(ctx.saved), dptr(grad_logits), dptr(grad_log_dur), B, S, L, ctx.seed,
                                                     ctx.offset, C.byref(g), dptr(ws), n_ws, stream_ptr(dev)))
        return (None,) * 7 + tuple(grads)


class TrainableParrot(nn.Module):
    """The reference's ``Parrot`` as a trainable module on the HIP kernels: same constructor, ``state_dict`` keys and shapes."""

    def __init__(self, data_config, src_vocab_size, src_pad_idx) -> None:
        super().__init__()
        tr = data_config["transformer"]
        self.max_len, self.d_model = tr["max_len"], tr["d_model"]
        self.data_config = data_config
        self.src_vocab_size, self.src_pad_idx = int(src_vocab_size), src_pad_idx
        if self.d_model % tr["encoder"]["n_head"] or self.d_model % tr["decoder"]["n_head"]:
            raise AssertionError("d_model % n_head != 0")  # reference modules/fft.py:44
        if max(tr["encoder"]["n_layer"], tr["decoder"]["n_layer"]) > _lib.TTE_TRAIN_MAX_LAYERS:
            raise ValueError(f"TrainableParrot: at most {_lib.TTE_TRAIN_MAX_LAYERS} layers per stack")
        with open(os.path.join(data_config["path"]["root_path"], "speakers.json"), "r") as f:
            self.n_speaker = len(json.load(f))
        _attach(self, "pos_emb.pe", sinusoid_table(self.max_len, self.d_model), buffer=True)
        self._keys: List[str] = []
        shapes = parrot_param_shapes(data_config, self.src_vocab_size, self.n_speaker)
        for key, shape in shapes.items():
            # torch's own initialisation: N(0, 1) embeddings (padding row 0), ones / zeros LayerNorm, U(-1 / sqrt(fan), ..) elsewhere
            if key in ("tok_emb.weight", "speaker_emb.weight"):
                t = torch.randn(shape)
                if key == "tok_emb.weight" and src_pad_idx is not None:
                    t[src_pad_idx] = 0
            elif key.endswith("norm.weight") or key in ("duration_predictor.layers.2.weight", "duration_predictor.layers.6.weight"):
                t = torch.ones(shape)
            elif key.endswith("norm.bias") or key in ("duration_predictor.layers.2.bias", "duration_predictor.layers.6.bias"):
                t = torch.zeros(shape)
            else:
                fan = 1
                for n in shapes[key[:-4] + "weight"][1:] if key.endswith("bias") else shape[1:]:
                    fan *= n
                t = (torch.rand(shape) * 2 - 1) / max(fan, 1) ** 0.5
            _attach(self, key, t)
            self._keys.append(key)
        self._seed: Optional[int] = None  # torch.initial_seed() at the first training forward
        self._offset = 0                  # training forwards so far: the dropout generator's offset (not in the state dict)

    def _cfg(self) -> "_lib.TteTrainCfg":
        cfgd = self.data_config
        tr, dp = cfgd["transformer"], cfgd["duration_predictor"]
        tte = _lib.TteCfg(tr["d_model"], tr["conv_n_filter"], tr["conv_kernel_sizes"][0], tr["conv_kernel_sizes"][1], tr["max_len"],
                          tr["encoder"]["n_layer"], tr["encoder"]["n_head"], tr["decoder"]["n_layer"], tr["decoder"]["n_head"],
                          dp["n_filter"], dp["kernel_size"], self.src_vocab_size, self.n_speaker, cfgd["preprocess"]["hubert_codes"])
        return _lib.TteTrainCfg(tte, -1 if self.src_pad_idx is None else int(self.src_pad_idx), float(tr["encoder"]["dropout_p"]),
                                float(tr["decoder"]["dropout_p"]), float(dp["dropout_p"]))

    def _tensors(self, dev):
        named = dict(self.named_parameters())
        params = [named[k] for k in self._keys]
        pe = self.get_buffer("pos_emb.pe")
        for name, t in list(zip(self._keys, params)) + [("pos_emb.pe", pe)]:
            require_cuda(t, name)
            if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"TrainableParrot: `{name}` must be a contiguous fp32 tensor on {dev} (got {t.dtype} on {t.device})")
        return params, pe

    def forward(self, batch, inference=False):
        """Reference modules/parrot.py:90-110 with inference=False: ``batch`` holds phones (B, S), src_mask (B, S) bool, speaker (B),
        duration (B, S) and tgt_mask (B, max row sum of duration) bool, all on the GPU."""
        if inference is True:
            raise NotImplementedError("TrainableParrot runs the teacher-forced forward only; use parrot_tts_amd.Parrot for inference")
        assert "duration" in batch.keys()  # reference modules/parrot.py:92
        phones, src_mask, duration, tgt_mask = batch["phones"], batch["src_mask"], batch["duration"], batch["tgt_mask"]
        speaker = batch.get("speaker") if self.n_speaker > 1 else None
        for name, t in (("phones", phones), ("src_mask", src_mask), ("duration", duration), ("tgt_mask", tgt_mask), ("speaker", speaker)):
            if t is not None:
                require_cuda(t, name)
        if self.n_speaker > 1 and speaker is None:
            raise KeyError("speaker")
        if phones.dim() != 2 or phones.shape[0] < 1 or phones.shape[1] < 1 or src_mask.shape != phones.shape or duration.shape != phones.shape:
            raise ValueError(f"TrainableParrot: phones, src_mask and duration must be (B, S) with B, S >= 1; got {tuple(phones.shape)}, "
                             f"{tuple(src_mask.shape)}, {tuple(duration.shape)}")
        B, S = int(phones.shape[0]), int(phones.shape[1])
        dev = phones.device
        phones_t = phones.detach().to(torch.int64).contiguous()
        dur_t = duration.detach().to(torch.int64).contiguous()
        spk_t = None if speaker is None else speaker.detach().to(torch.int64).contiguous().view(-1)
        # what torch raises on, in one transfer (the reference's own host sync is the max row sum, duration.py:10)
        bad_spk = torch.zeros((), dtype=torch.bool, device=dev) if spk_t is None else ((spk_t < 0) | (spk_t >= self.n_speaker)).any()
        probe = torch.stack([dur_t.sum(dim=1).max(), dur_t.min(), ((phones_t < 0) | (phones_t >= self.src_vocab_size)).any().long(),
                             bad_spk.long()]).tolist()
        L = int(probe[0])
        if probe[2] or probe[3]:
            raise IndexError("index out of range in self")
        if probe[1] < 0:
            raise RuntimeError("repeats can not be negative")
        if tgt_mask.dim() != 2 or tgt_mask.shape[0] != B or tgt_mask.shape[1] != L:
            raise AssertionError(f"tgt_mask.shape[1] == max_len: got {tuple(tgt_mask.shape)}, the durations sum to {L}")  # duration.py:12
        if spk_t is not None and spk_t.shape[0] != B:
            raise ValueError(f"TrainableParrot: speaker must be (B,), got {tuple(speaker.shape)}")
        if L < 1:
            raise ValueError("TrainableParrot: the durations sum to 0")
        batch_t = (phones_t, src_mask.detach().to(torch.uint8).contiguous(), spk_t, dur_t, tgt_mask.detach().to(torch.uint8).contiguous())
        params, pe = self._tensors(dev)
        cfg = self._cfg()
        if self.training and torch.is_grad_enabled():
            if self._seed is None:
                self._seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF
            offset = self._offset
            self._offset += 1
            out, log_dur = _ParrotTrainFn.apply(cfg, tuple(self._keys), pe, batch_t, L, self._seed, offset, *params)
        else:
            with torch.no_grad():
                out, log_dur, _ = _train_forward(cfg, tuple(self._keys), params, pe, batch_t, L, False, 0, 0)
        return (out, batch["src_mask"], batch["tgt_mask"], log_dur)


def dropout_mask(seed: int, offset: int, site: int, n: int, p: float, device="cuda") -> torch.Tensor:
    """The keep mask (uint8, n elements) the training kernels apply at ``site`` under (seed, offset): parrot_tte_train_dropout_mask."""
    out = torch.empty((n,), dtype=torch.uint8, device=device)
    with torch.cuda.device(out.device):
        _lib.check(_lib.lib().parrot_tte_train_dropout_mask(seed, offset, site, n, p, dptr(out), stream_ptr(out.device)))
    return out
