"""``FusedAdamW``: ``torch.optim.AdamW`` (decoupled weight decay, no amsgrad) whose ``step()`` is ONE ``parrot_adamw_step`` call per
parameter group -- a fused multi-tensor kernel of libparrot_hip.so that reads p, g, exp_avg, exp_avg_sq and writes p, exp_avg,
exp_avg_sq once, where torch's default (foreach) path walks every tensor in about ten passes.  The two optimisers of the vocoder's
trainer (reference utils/vocoder/train.py:80-82, 151, 168) are its use: ~160 and ~290 tensors of 1 to 5.2 M elements.

It takes AdamW's constructor arguments and defaults, keeps torch's state per parameter (``step``: a 0-dim fp32 CPU tensor,
``exp_avg``, ``exp_avg_sq``) and the ``param_groups`` keys this torch's AdamW writes, so state dicts go both ways between the two
classes and torch's LR schedulers drive it unchanged.  The update rule is the one of include/parrot_hip.h (every line one correctly
rounded fp32 operation); ``step_scalars`` is its host half.  Parameters are fp32, dense and contiguous on one GPU; there is no CPU
fallback."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .ops import stream_ptr

_UNSUPPORTED = ("amsgrad", "maximize", "capturable", "differentiable")


def step_scalars(lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, step: int):
    """The host half of the update rule -> (decay, w1, b2, w2, e, ns, rs) as numpy float32: formed in double, each rounded to fp32
    once, exactly as host_optim.hip forms them.  ``step``: the count after this update (>= 1)."""
    lr, beta1, beta2, eps, weight_decay = float(lr), float(beta1), float(beta2), float(eps), float(weight_decay)
    f = np.float32
    return (f(1.0 - lr * weight_decay), f(1.0 - beta1), f(beta2), f(1.0 - beta2), f(eps),
            f(-lr / (1.0 - math.pow(beta1, float(step)))), f(math.sqrt(1.0 - math.pow(beta2, float(step)))))


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False, foreach=None,
                 capturable=False, differentiable=False, fused=None):
        given = dict(amsgrad=amsgrad, maximize=maximize, capturable=capturable, differentiable=differentiable)
        for name in _UNSUPPORTED:
            if given[name]:
                raise NotImplementedError(f"parrot_tts_amd.FusedAdamW: {name}=True is not implemented")
        if isinstance(lr, torch.Tensor):
            raise NotImplementedError("parrot_tts_amd.FusedAdamW: a tensor lr is not implemented")
        # torch's own AdamW validates the values and names the keys of a group (they differ between torch versions)
        probe = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        defaults = dict(probe.defaults)
        defaults.update(foreach=foreach, fused=fused)
        super().__init__(params, defaults)
        self._tables: dict = {}   # group index -> (the ctypes table, what each slot holds): built once and refilled
        self._ready: dict = {}    # id(parameter) -> (exp_avg, exp_avg_sq, numel) as validated; a replaced state tensor is checked again

    def _check_param(self, p: torch.Tensor, dev):
        if p.device.type != "cuda":
            raise RuntimeError(f"parrot_tts_amd: FusedAdamW parameters must live on the GPU (got {p.device}); there is no CPU fallback")
        if p.device != dev:
            raise RuntimeError("parrot_tts_amd: the parameters of one FusedAdamW must live on one device")
        if p.dtype != torch.float32 or p.layout != torch.strided or p.is_sparse or not p.is_contiguous():
            raise RuntimeError(f"parrot_tts_amd: FusedAdamW parameters must be dense contiguous fp32 (got {p.dtype}, {tuple(p.shape)}, "
                               f"strides {tuple(p.stride())})")

    def _prepare(self, p: torch.Tensor, state: dict, dev):
        """Validate a parameter and its state (created here at its first gradient) -> the ``_ready`` entry."""
        self._check_param(p, dev)
        if len(state) == 0:
            state["step"] = torch.tensor(0.0, dtype=torch.float32)
            state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        st = state["step"]
        if st.device.type != "cpu" or st.dtype != torch.float32:  # (a state written by a capturable / fused torch optimiser)
            state["step"] = st.detach().to("cpu", torch.float32)
        m, v, n = state["exp_avg"], state["exp_avg_sq"], p.numel()
        for t in (m, v):
            if t.dtype != torch.float32 or t.layout != torch.strided or not t.is_contiguous() or t.device != dev or t.numel() != n:
                raise RuntimeError("parrot_tts_amd: FusedAdamW state (exp_avg, exp_avg_sq) must be dense contiguous fp32 like its parameter")
        entry = self._ready[id(p)] = (m, v, n)
        return entry

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        first = next((p for g in self.param_groups for p in g["params"]), None)
        if first is None:
            return loss
        if first.device.type != "cuda":
            raise RuntimeError(f"parrot_tts_amd: FusedAdamW parameters must live on the GPU (got {first.device}); there is no CPU fallback")
        dev = first.device
        lib = _lib.lib()
        f32, strided, ready = torch.float32, torch.strided, self._ready
        for gi, group in enumerate(self.param_groups):
            for name in _UNSUPPORTED:
                if group.get(name):
                    raise NotImplementedError(f"parrot_tts_amd.FusedAdamW: {name}=True is not implemented")
            if isinstance(group["lr"], torch.Tensor):
                raise NotImplementedError("parrot_tts_amd.FusedAdamW: a tensor lr is not implemented")
            params = group["params"]
            table, held = self._tables.get(gi, (None, None))
            if table is None or len(table) < len(params):
                table, held = (_lib.AdamwTensor * max(len(params), 1))(), [None] * max(len(params), 1)
                self._tables[gi] = (table, held)
            K, keep, steps = 0, [], []
            for p in params:
                g = p.grad  # (re-read every step: zero_grad() sets it to None)
                if g is None:
                    continue
                state = self.state[p]
                entry = ready.get(id(p))
                if entry is None or entry[0] is not state.get("exp_avg") or entry[1] is not state.get("exp_avg_sq"):
                    entry = self._prepare(p, state, dev)
                m, v, n = entry
                if g.layout is not strided:
                    raise RuntimeError("parrot_tts_amd: FusedAdamW does not support sparse gradients")
                if g.dtype is not f32 or g.device != dev or g.numel() != n:
                    raise RuntimeError("parrot_tts_amd: a gradient must be fp32 on its parameter's device and of its shape")
                if not g.is_contiguous():
                    g = g.contiguous()
                    keep.append(g)
                st = state["step"]
                steps.append(st)
                if n == 0:
                    continue
                # the slot: rewritten whole when it held something else, else the gradient pointer and the step alone
                now = (p.data_ptr(), m.data_ptr(), v.data_ptr(), n)
                t = table[K]
                if held[K] != now:
                    t.p, t.m, t.v, t.n = now
                    held[K] = now
                t.g, t.step = g.data_ptr(), int(st.item()) + 1
                K += 1
            if steps:
                torch._foreach_add_(steps, 1)
            if K == 0:
                continue
            beta1, beta2 = group["betas"]
            with torch.cuda.device(dev):
                _lib.check(lib.parrot_adamw_step(table, K, float(group["lr"]), float(beta1), float(beta2), float(group["eps"]),
                                                 float(group["weight_decay"]), stream_ptr(dev)))
            del keep
        return loss
