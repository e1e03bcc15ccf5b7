"""Drop-in ``ModelLoss`` for reference modules/loss.py:5-21 backed by libparrot_hip.so (``parrot_tte_loss``).

Same constructor ``ModelLoss(data_config)`` and ``forward(out, log_dur_preds, batch) -> (loss, code_loss, dur_loss)``: the
cross entropy of ``out.reshape(-1, V)`` against ``batch["codes"].reshape(-1)`` with ``ignore_index = hubert_codes`` plus the
MSE of the log-durations against ``log(batch["duration"] + 1)`` over ``batch["src_mask"]``.  The reductions run in one HIP
kernel pair (fp32 log-sum-exp per position, fp64 fixed-order sums: two calls agree bit for bit); the results are 0-dim fp32
device tensors.  One synchronisation per call reads the kernel's target check (torch's IndexError)."""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib
from .ops import dptr, require_cuda, stream_ptr


class ModelLoss(nn.Module):
    def __init__(self, data_config):
        super().__init__()
        self.num_codes = int(data_config["preprocess"]["hubert_codes"])
        self.last_stats: dict = {}  # counts of the last call: n_valid, n_correct (argmax == target), n_src

    @torch.no_grad()
    def forward(self, out, log_dur_preds, batch):
        V = self.num_codes
        logits = out.reshape(-1, V)  # loss.py:16
        codes = batch["codes"].reshape(-1)
        if logits.shape[0] != codes.shape[0]:  # nn.CrossEntropyLoss's message
            raise ValueError(f"Expected input batch_size ({logits.shape[0]}) to match target batch_size ({codes.shape[0]}).")
        require_cuda(logits, "out")
        dev = logits.device
        logits = logits.to(torch.float32).contiguous()
        codes = codes.to(dev, torch.int64).contiguous()
        src_mask = batch["src_mask"].to(dev)
        log_dur = log_dur_preds.to(dev, torch.float32)
        dur = batch["duration"].to(dev, torch.int64)
        if not (src_mask.shape == log_dur.shape == dur.shape):  # loss.py:13-14 masks both with src_mask
            raise RuntimeError(f"src_mask {tuple(src_mask.shape)}, log_dur_preds {tuple(log_dur.shape)} and duration "
                               f"{tuple(dur.shape)} must have one shape")
        src = src_mask.to(torch.uint8).contiguous()
        log_dur, dur = log_dur.contiguous(), dur.contiguous()
        lib = _lib.lib()
        N = logits.shape[0]
        sums = torch.empty(8, dtype=torch.float64, device=dev)
        losses = torch.empty(3, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            ws = torch.empty(max(int(lib.parrot_tte_loss_workspace_bytes(N)), 1), dtype=torch.uint8, device=dev)
            _lib.check(lib.parrot_tte_loss(dptr(logits), dptr(codes), N, V, V, dptr(log_dur), dptr(dur), dptr(src), src.numel(),
                                           dptr(sums), dptr(losses), dptr(ws), ws.numel(), stream_ptr(dev)))
            h = sums.cpu()  # the one synchronisation: the target check
        if h[5] > 0:
            raise IndexError(f"Target {int(h[6])} is out of bounds.")
        self.last_stats = {"n_valid": int(h[1]), "n_correct": int(h[2]), "n_src": int(h[4]), "sum_nll": float(h[0]), "sum_sq": float(h[3])}
        return losses[0], losses[1], losses[2]
