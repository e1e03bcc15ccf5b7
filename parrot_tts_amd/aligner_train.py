"""Training the forced aligner on the GPU: ``TrainableAligner``, the reference's ``Aligner`` (utils/aligner/model.py:5-64) under
``model.train()`` with its backward, backed by libparrot_hip.so (``parrot_aligner_train_forward`` / ``parrot_aligner_train_backward``).

    TrainableAligner(n_mels, num_symbols, lstm_dim, conv_dim)   the reference's constructor, state_dict keys and shapes
    TrainableAligner.from_checkpoint(checkpoint), .get_step()    as the reference
    .forward(mel) -> logits (B, T, num_symbols)                  train mode with grad enabled: BatchNorm on batch statistics, the
                                                                 running buffers updated, one autograd node over the 19 parameters;
                                                                 .eval() or no_grad: the running statistics, no graph

The parameters are real ``nn.Parameter``s on the device and the library reads them where they live: an optimiser's in-place step
is seen by the next forward with nothing rebuilt or copied.  A state dict moves freely between this module, the reference's
``Aligner`` and the inference ``Aligner`` of aligner.py.  The reference trainer's loop body (trainer.py:60-71) runs unchanged on
it, also under ``torch.use_deterministic_algorithms(True)`` with ``parrot_tts_amd.aligner.CTCLoss()`` as the loss: nothing here
accumulates atomically, and two runs agree bit for bit.  Adam and ``clip_grad_norm_`` stay torch's.  There is no CPU path: a CPU
tensor raises, as in the other shims."""
from __future__ import annotations

import ctypes as C
from typing import List

import torch
from torch import nn

from . import _lib
from ._handle import _attach
from .ops import _workspace, dptr, require_cuda, stream_ptr

BN_EPS = 1e-5

# the 19 parameters in the order of parrot_aligner_grads' fields
PARAM_KEYS: List[str] = (
    [f"convs.{i}.conv.weight" for i in range(3)] + [f"convs.{i}.bnorm.weight" for i in range(3)] + [f"convs.{i}.bnorm.bias" for i in range(3)]
    + [f"rnn.{k}_l0{sfx}" for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh") for sfx in ("", "_reverse")]
    + ["lin.weight", "lin.bias"])
_GRAD_FIELDS = [("conv_w", i) for i in range(3)] + [("bn_weight", i) for i in range(3)] + [("bn_bias", i) for i in range(3)] \
    + [(f, d) for f in ("w_ih", "w_hh", "b_ih", "b_hh") for d in range(2)] + [("lin_w", None), ("lin_b", None)]


def _set_field(struct, field, index, tensor) -> None:
    ptr = None if tensor is None else tensor.data_ptr()
    if index is None:
        setattr(struct, field, ptr)
    else:
        getattr(struct, field)[index] = ptr


def _dev_weights(params, run_mean, run_var) -> "_lib.AlignerDevWeights":
    w = _lib.AlignerDevWeights()
    for (field, index), p in zip(_GRAD_FIELDS, params):
        _set_field(w, field, index, p)
    for i in range(3):
        w.bn_mean[i], w.bn_var[i] = run_mean[i].data_ptr(), run_var[i].data_ptr()
    return w


def _train_forward(cfg, params, run_mean, run_var, mel, training: bool):
    """One parrot_aligner_train_forward call on validated tensors -> (logits, saved buffer or None)."""
    dev = mel.device
    B, T = int(mel.shape[0]), int(mel.shape[1])
    lib = _lib.lib()
    logits = torch.empty((B, T, cfg.num_symbols), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        n_ws = int(lib.parrot_aligner_train_workspace_bytes(C.byref(cfg), B, T))
        n_sv = int(lib.parrot_aligner_train_saved_bytes(C.byref(cfg), B, T))
        ws = _workspace(n_ws, dev)  # (0 bytes beyond the limits: the call then fails at the library's own shape check)
        saved = _workspace(n_sv, dev) if training else None
        w = _dev_weights(params, run_mean, run_var)
        _lib.check(lib.parrot_aligner_train_forward(C.byref(cfg), C.byref(w), dptr(mel), B, T, int(training), dptr(logits), dptr(saved),
                                                    dptr(ws), n_ws, stream_ptr(dev)))
    return logits, saved


class _AlignerTrainFn(torch.autograd.Function):
    """forward(mel, cfg, running means, running vars, *19 parameters): one training forward, which owns the ``saved`` buffer;
    backward: one parrot_aligner_train_backward call.  A parameter that needs no gradient gets none (its field is null and is not
    computed), ``mel`` gets None, and there is no double backward."""

    @staticmethod
    def forward(ctx, mel, cfg, run_mean, run_var, *params):
        logits, saved = _train_forward(cfg, params, run_mean, run_var, mel, True)
        ctx.save_for_backward(mel, *params)
        ctx.cfg, ctx.saved, ctx.run_mean, ctx.run_var = cfg, saved, run_mean, run_var
        return logits

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_logits):
        mel, *params = ctx.saved_tensors
        dev = mel.device
        B, T = int(mel.shape[0]), int(mel.shape[1])
        lib = _lib.lib()
        grad_logits = grad_logits.to(torch.float32).contiguous()
        grads = [torch.empty_like(p) if need else None for p, need in zip(params, ctx.needs_input_grad[4:])]
        g = _lib.AlignerGrads()
        for (field, index), t in zip(_GRAD_FIELDS, grads):
            _set_field(g, field, index, t)
        with torch.cuda.device(dev):
            n_ws = int(lib.parrot_aligner_train_workspace_bytes(C.byref(ctx.cfg), B, T))
            ws = _workspace(n_ws, dev)
            w = _dev_weights(params, ctx.run_mean, ctx.run_var)
            _lib.check(lib.parrot_aligner_train_backward(C.byref(ctx.cfg), C.byref(w), dptr(mel), dptr(ctx.saved), dptr(grad_logits), B, T,
                                                         C.byref(g), dptr(ws), n_ws, stream_ptr(dev)))
        return (None, None, None, None, *grads)


class TrainableAligner(nn.Module):
    """The reference's ``Aligner`` as a trainable module on the HIP kernels: same constructor, ``state_dict`` keys and shapes
    (``step`` and the BatchNorm buffers included), ``from_checkpoint`` and ``get_step``.  ``step`` increments on every forward, as
    the reference's does (``if self.train:`` tests a bound method)."""

    def __init__(self, n_mels: int, num_symbols: int, lstm_dim: int, conv_dim: int) -> None:
        super().__init__()
        from .aligner import aligner_param_shapes
        self.n_mels, self.num_symbols, self.lstm_dim, self.conv_dim = int(n_mels), int(num_symbols), int(lstm_dim), int(conv_dim)
        self.register_buffer("step", torch.tensor(1, dtype=torch.int))
        for key, shape in aligner_param_shapes(self.n_mels, self.num_symbols, self.lstm_dim, self.conv_dim).items():
            leaf = key.rsplit(".", 1)[1]
            if leaf in ("running_mean", "running_var"):
                _attach(self, key, torch.zeros(shape) if leaf == "running_mean" else torch.ones(shape), buffer=True)
            elif ".bnorm." in key:
                _attach(self, key, torch.ones(shape) if leaf == "weight" else torch.zeros(shape))
            else:  # torch's own initialisation of Conv1d / LSTM / Linear: U(-1 / sqrt(fan), 1 / sqrt(fan))
                if key.startswith("rnn."):
                    fan = self.lstm_dim
                elif key.startswith("lin."):
                    fan = 2 * self.lstm_dim
                else:
                    fan = shape[1] * shape[2]
                _attach(self, key, (torch.rand(shape) * 2 - 1) / fan ** 0.5)
        for i in range(3):
            _attach(self, f"convs.{i}.bnorm.num_batches_tracked", torch.tensor(0, dtype=torch.long), buffer=True)

    # ---- the reference's surface ---------------------------------------------------------------
    def get_step(self):
        return self.step.data.item()

    @classmethod
    def from_checkpoint(cls, checkpoint: dict) -> "TrainableAligner":
        config = checkpoint["config"]
        symbols = checkpoint["symbols"]
        model = cls(n_mels=config["audio"]["n_mels"], num_symbols=len(symbols) + 1, **config["model"])
        model.load_state_dict(checkpoint["model"])
        return model

    # ---- compute -------------------------------------------------------------------------------
    def _tensors(self, dev):
        named = dict(self.named_parameters())
        params = [named[k] for k in PARAM_KEYS]
        bufs = dict(self.named_buffers())
        run_mean = [bufs[f"convs.{i}.bnorm.running_mean"] for i in range(3)]
        run_var = [bufs[f"convs.{i}.bnorm.running_var"] for i in range(3)]
        for name, t in list(zip(PARAM_KEYS, params)) + [("running_mean", t) for t in run_mean] + [("running_var", t) for t in run_var]:
            require_cuda(t, name)
            if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"TrainableAligner: `{name}` must be a contiguous fp32 tensor on {dev} (got {t.dtype} on {t.device})")
        return params, run_mean, run_var

    def forward(self, mel: torch.Tensor) -> torch.Tensor:
        """mel (B, T, n_mels) on the GPU -> logits (B, T, num_symbols), the padded batch as it stands."""
        require_cuda(mel, "mel")
        if mel.dim() != 3 or mel.shape[2] != self.n_mels:
            raise ValueError(f"TrainableAligner: expected mel (B, T, {self.n_mels}), got {tuple(mel.shape)}")
        if mel.shape[0] < 1 or mel.shape[1] < 1:
            raise ValueError("TrainableAligner: empty batch or sequence")
        training = self.training and torch.is_grad_enabled()
        if training and mel.shape[0] * mel.shape[1] == 1:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {(1, self.conv_dim, 1)}")
        x = mel.detach().to(torch.float32).contiguous()
        params, run_mean, run_var = self._tensors(x.device)
        cfg = _lib.AlignerCfg(self.n_mels, self.num_symbols, self.lstm_dim, self.conv_dim, BN_EPS)
        if training:
            logits = _AlignerTrainFn.apply(x, cfg, run_mean, run_var, *params)
            with torch.no_grad():
                for i in range(3):
                    self.get_buffer(f"convs.{i}.bnorm.num_batches_tracked").add_(1)
        else:
            with torch.no_grad():
                logits, _ = _train_forward(cfg, params, run_mean, run_var, x, False)
        with torch.no_grad():
            self.step += 1
        return logits
