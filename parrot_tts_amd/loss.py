"""Drop-in ``ModelLoss`` for reference modules/loss.py:5-21 backed by libparrot_hip.so (``parrot_tte_loss``).

Same constructor ``ModelLoss(data_config)`` and ``forward(out, log_dur_preds, batch) -> (loss, code_loss, dur_loss)``: the
cross entropy of ``out.reshape(-1, V)`` against ``batch["codes"].reshape(-1)`` with ``ignore_index = hubert_codes`` plus the
MSE of the log-durations against ``log(batch["duration"] + 1)`` over ``batch["src_mask"]``.  The reductions run in one HIP
kernel pair (fp32 log-sum-exp per position, fp64 fixed-order sums: two calls agree bit for bit); the results are 0-dim fp32
device tensors.  One synchronisation per call reads the kernel's target check (torch's IndexError).

The loss is differentiable with respect to ``out`` and ``log_dur_preds`` (train.py:72-85: the loss ``training_step`` returns
for ``loss.backward()``): when either requires grad, ``forward`` returns tensors with a graph whose backward is one
``parrot_tte_loss_grad`` call -- deterministic, no atomics, no host synchronisation; ``loss_and_grad`` returns the losses and
both gradients from one call.  For a torch-built model: the HIP ``Parrot.forward`` has no backward."""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib
from .ops import _workspace, dptr, require_cuda, stream_ptr


def _loss_call(a, weights=None, grad_logits: bool = False, grad_log_dur: bool = False):
    """One device call on ``ModelLoss._args``'s tensors -> (sums (8) fp64, losses (3) fp32, grad_logits (N, V) fp32 or None,
    grad_log_dur fp32 in log_dur's shape or None): parrot_tte_loss without a gradient, parrot_tte_loss_grad with one (``weights``:
    {w_code, w_dur}, a 2-element fp64 device tensor, None = {1, 1})."""
    logits, codes, log_dur, dur, src = a
    dev = logits.device
    lib = _lib.lib()
    N, V = logits.shape
    sums = torch.empty(8, dtype=torch.float64, device=dev)
    losses = torch.empty(3, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        if not (grad_logits or grad_log_dur):
            ws = _workspace(lib.parrot_tte_loss_workspace_bytes(N), dev)
            _lib.check(lib.parrot_tte_loss(dptr(logits), dptr(codes), N, V, V, dptr(log_dur), dptr(dur), dptr(src), src.numel(),
                                           dptr(sums), dptr(losses), dptr(ws), ws.numel(), stream_ptr(dev)))
            return sums, losses, None, None
        g_logits = torch.empty_like(logits) if grad_logits else None
        g_dur = torch.empty_like(log_dur) if grad_log_dur else None
        ws = _workspace(lib.parrot_tte_loss_grad_workspace_bytes(N), dev)
        _lib.check(lib.parrot_tte_loss_grad(dptr(logits), dptr(codes), N, V, V, dptr(log_dur), dptr(dur), dptr(src), src.numel(),
                                            dptr(weights), dptr(sums), dptr(losses), dptr(g_logits), dptr(g_dur), dptr(ws), ws.numel(),
                                            stream_ptr(dev)))
    return sums, losses, g_logits, g_dur


class _ModelLossFn(torch.autograd.Function):
    """The forward is ``ModelLoss``'s plain path (parrot_tte_loss); the backward is one parrot_tte_loss_grad call with
    w_code = g_loss + g_code and w_dur = g_loss + g_dur, formed on the device.  No double backward."""

    @staticmethod
    def forward(ctx, out, log_dur_preds, module, batch):
        a = module._args(out, log_dur_preds, batch)
        ctx.save_for_backward(*a)
        ctx.shapes = (out.shape, out.dtype, log_dur_preds.shape, log_dur_preds.dtype, log_dur_preds.device)
        loss, code, dur = module._checked(*_loss_call(a)[:2])
        return loss.clone(), code.clone(), dur.clone()  # (three outputs of their own, not views of one tensor)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, g_code, g_dur):
        a = ctx.saved_tensors
        need_out, need_dur = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        o_shape, o_dtype, d_shape, d_dtype, d_dev = ctx.shapes
        w = torch.stack([g_loss + g_code, g_loss + g_dur]).to(a[0].device, torch.float64)
        _, _, g_logits, g_ld = _loss_call(a, w, need_out, need_dur)
        return (g_logits.reshape(o_shape).to(o_dtype) if need_out else None,
                g_ld.reshape(d_shape).to(d_dev, d_dtype) if need_dur else None, None, None)


class ModelLoss(nn.Module):
    def __init__(self, data_config):
        super().__init__()
        self.num_codes = int(data_config["preprocess"]["hubert_codes"])
        self.last_stats: dict = {}  # counts of the last call: n_valid, n_correct (argmax == target), n_src

    def _args(self, out, log_dur_preds, batch):
        """The kernels' arguments, validated: (logits (N, V) f32, codes (N) i64, log_dur f32, dur i64, src u8), dense on out's device."""
        V = self.num_codes
        logits = out.reshape(-1, V)  # loss.py:16
        codes = batch["codes"].reshape(-1)
        if logits.shape[0] != codes.shape[0]:  # nn.CrossEntropyLoss's message
            raise ValueError(f"Expected input batch_size ({logits.shape[0]}) to match target batch_size ({codes.shape[0]}).")
        require_cuda(logits, "out")
        dev = logits.device
        logits = logits.detach().to(torch.float32).contiguous()
        codes = codes.to(dev, torch.int64).contiguous()
        src_mask = batch["src_mask"].to(dev)
        log_dur = log_dur_preds.detach().to(dev, torch.float32)
        dur = batch["duration"].to(dev, torch.int64)
        if not (src_mask.shape == log_dur.shape == dur.shape):  # loss.py:13-14 masks both with src_mask
            raise RuntimeError(f"src_mask {tuple(src_mask.shape)}, log_dur_preds {tuple(log_dur.shape)} and duration "
                               f"{tuple(dur.shape)} must have one shape")
        return logits, codes, log_dur.contiguous(), dur.contiguous(), src_mask.to(torch.uint8).contiguous()

    def _checked(self, sums, losses):
        """The one synchronisation: the target check (torch's IndexError) and ``last_stats`` -> (loss, code_loss, dur_loss)."""
        h = sums.cpu()
        if h[5] > 0:
            raise IndexError(f"Target {int(h[6])} is out of bounds.")
        self.last_stats = {"n_valid": int(h[1]), "n_correct": int(h[2]), "n_src": int(h[4]), "sum_nll": float(h[0]), "sum_sq": float(h[3])}
        return losses[0], losses[1], losses[2]

    def forward(self, out, log_dur_preds, batch):
        if torch.is_grad_enabled() and (out.requires_grad or log_dur_preds.requires_grad):
            return _ModelLossFn.apply(out, log_dur_preds, self, batch)
        with torch.no_grad():
            return self._checked(*_loss_call(self._args(out, log_dur_preds, batch))[:2])

    @torch.no_grad()
    def loss_and_grad(self, out, log_dur_preds, batch, weights=(1.0, 1.0)):
        """``forward`` and the gradient in one device call: -> ((loss, code_loss, dur_loss), grad_out, grad_log_dur), the
        gradient of ``weights[0] * code_loss + weights[1] * dur_loss`` with respect to ``out`` and ``log_dur_preds`` in their
        shapes and dtypes ((1, 1): of ``loss``).  The losses are ``forward``'s bit for bit; positions whose code is the ignore
        index and durations outside ``src_mask`` get exactly 0.  Raises as ``forward``."""
        a = self._args(out, log_dur_preds, batch)
        w = torch.as_tensor(weights, dtype=torch.float64).reshape(2).to(a[0].device)
        sums, losses, g_logits, g_ld = _loss_call(a, w, True, True)
        res = self._checked(sums, losses)
        return res, g_logits.reshape(out.shape).to(out.dtype), g_ld.reshape(log_dur_preds.shape).to(log_dur_preds.device, log_dur_preds.dtype)
