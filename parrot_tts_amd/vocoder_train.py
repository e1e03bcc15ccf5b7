"""Training the vocoder's generator on the GPU: ``TrainableCodeGenerator``, the reference's ``CodeGenerator``
(utils/vocoder/models.py:69-169) with weight norm attached and its whole backward, backed by libparrot_hip.so
(``parrot_voc_train_forward`` / ``parrot_voc_train_backward``).

    TrainableCodeGenerator(h)               the reference's constructor, state_dict keys and shapes (``*.weight_g``, ``*.weight_v``,
                                            ``*.bias``, ``dict.weight``, ``spkr.weight``); plain ``weight`` keys load into a layer
                                            without ``g``
    .forward(code=, spkr=) -> (B, 1, T)     with grad enabled: one autograd node over all parameters; under no_grad or .eval(): the
                                            same kernels with no graph and nothing kept (the generator has no dropout and no BatchNorm,
                                            so the values are the same)
    .remove_weight_norm()                   folds on the device; the module keeps working, and training, on plain weights
    .lrelu_masks()                          the leaky-ReLU masks of the last training forward, in site order (tests)

The parameters are real ``nn.Parameter``s on the device and the library reads them where they live: an optimiser's in-place step is
seen by the next forward with nothing rebuilt or copied.  A state dict moves freely between this module, the reference's
``CodeGenerator`` and the inference ``CodeGenerator`` of vocoder.py.  Nothing accumulates atomically, and
``torch.use_deterministic_algorithms(True)`` is supported.  Conditioning features other than ``spkr`` are not trainable here: any
keyword beyond ``code``, ``spkr`` and ``f0`` raises NotImplementedError.  There is no CPU path: a CPU tensor raises."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import torch
from torch import nn

from . import _lib
from .ops import _workspace, dptr, require_cuda, stream_ptr
from .vocoder import _ResBlock, _WNConv


def _fill(ptrs: "_lib.VocTrainPtrs", meta, tensors) -> None:
    """Put every tensor's device pointer (None: null) into the field of a VocTrainPtrs that ``meta`` names: (kind, index, field)."""
    for (kind, idx, field), t in zip(meta, tensors):
        ptr = None if t is None else t.data_ptr()
        if kind in ("dict", "spkr"):
            setattr(ptrs, kind, ptr)
            continue
        layer = ptrs.conv_pre if kind == "pre" else ptrs.conv_post if kind == "post" else getattr(ptrs, kind)[idx]
        setattr(layer, field, ptr)


def _train_forward(cfg, meta, params, code, spkr, keep: bool):
    """One parrot_voc_train_forward call on validated tensors -> (wav, saved buffer or None)."""
    dev = code.device
    B, U = int(code.shape[0]), int(code.shape[1])
    lib = _lib.lib()
    with torch.cuda.device(dev):
        T = int(lib.parrot_voc_train_out_len(C.byref(cfg), U))
        n_ws = int(lib.parrot_voc_train_workspace_bytes(C.byref(cfg), B, U))
        n_sv = int(lib.parrot_voc_train_saved_bytes(C.byref(cfg), B, U))
        wav = torch.empty((B, 1, max(T, 1)), dtype=torch.float32, device=dev)
        ws = _workspace(n_ws, dev)  # (0 bytes beyond the limits: the call then fails at the library's own shape check)
        saved = _workspace(n_sv, dev) if keep else None
        w = _lib.VocTrainPtrs()
        _fill(w, meta, params)
        _lib.check(lib.parrot_voc_train_forward(C.byref(cfg), C.byref(w), dptr(code), dptr(spkr), B, U, dptr(wav), dptr(saved), dptr(ws), n_ws,
                                                stream_ptr(dev)))
    return wav, saved


class _GeneratorTrainFn(torch.autograd.Function):
    """forward(cfg, meta, code, spkr, holder, *parameters): one training forward, which owns the ``saved`` buffer; backward: one
    parrot_voc_train_backward call.  A parameter that needs no gradient gets none (its field is null and is not computed), and there
    is no double backward."""

    @staticmethod
    def forward(ctx, cfg, meta, code, spkr, holder, *params):
        wav, saved = _train_forward(cfg, meta, params, code, spkr, True)
        ctx.save_for_backward(*params)
        ctx.cfg, ctx.meta, ctx.code, ctx.spkr, ctx.saved = cfg, meta, code, spkr, saved
        holder["last"] = (cfg, int(code.shape[0]), int(code.shape[1]), saved)
        return wav

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_wav):
        params = ctx.saved_tensors
        dev = ctx.code.device
        B, U = int(ctx.code.shape[0]), int(ctx.code.shape[1])
        lib = _lib.lib()
        grad_wav = grad_wav.to(torch.float32).contiguous()
        grads = [torch.empty_like(p) if need else None for p, need in zip(params, ctx.needs_input_grad[5:])]
        g = _lib.VocTrainPtrs()
        _fill(g, ctx.meta, grads)
        with torch.cuda.device(dev):
            n_ws = int(lib.parrot_voc_train_workspace_bytes(C.byref(ctx.cfg), B, U))
            ws = _workspace(n_ws, dev)
            w = _lib.VocTrainPtrs()
            _fill(w, ctx.meta, params)
            _lib.check(lib.parrot_voc_train_backward(C.byref(ctx.cfg), C.byref(w), dptr(ctx.code), dptr(ctx.spkr), dptr(ctx.saved), dptr(grad_wav),
                                                     B, U, C.byref(g), dptr(ws), n_ws, stream_ptr(dev)))
        return (None,) * 5 + tuple(grads)


class _TrainWNConv(_WNConv):
    """vocoder._WNConv (same keys, same initialisation) whose ``remove_weight_norm`` folds on the device, with the kernel the
    training forward folds with."""

    def remove_weight_norm(self):
        if "weight" in self._parameters:
            raise ValueError("weight_norm of this layer was already removed")  # torch raises ValueError too
        v, g = self.weight_v.detach(), self.weight_g.detach()
        if v.device.type != "cuda":
            w = torch._weight_norm(v, g, 0)  # (a module that has not been moved yet: there is nothing to run on)
        else:
            v32, g32 = v.to(torch.float32).contiguous(), g.to(torch.float32).contiguous()
            w, norm = torch.empty_like(v32), torch.empty_like(g32)
            with torch.cuda.device(v.device):
                _lib.check(_lib.lib().parrot_debug_voc_wn_fwd(dptr(v32), dptr(g32), dptr(w), dptr(norm), int(v32.shape[0]),
                                                              int(v32[0].numel()), stream_ptr(v.device)))
        del self._parameters["weight_g"], self._parameters["weight_v"]
        self.weight = nn.Parameter(w)


class _TrainResBlock(_ResBlock):
    def __init__(self, kind: str, ch: int, k: int, n_dil: int):
        nn.Module.__init__(self)
        self.kind = kind
        if kind == "1":
            self.convs1 = nn.ModuleList([_TrainWNConv((ch, ch, k), ch) for _ in range(n_dil)])
            self.convs2 = nn.ModuleList([_TrainWNConv((ch, ch, k), ch) for _ in range(n_dil)])
        else:
            self.convs = nn.ModuleList([_TrainWNConv((ch, ch, k), ch) for _ in range(n_dil)])


class TrainableCodeGenerator(nn.Module):
    """The reference's ``CodeGenerator`` as a trainable module on the HIP kernels: same constructor, ``state_dict`` keys and shapes."""

    def __init__(self, h):
        super().__init__()
        self.h = h
        get = h.get if hasattr(h, "get") else (lambda k, d=None: getattr(h, k, d))
        self._kind = "1" if str(get("resblock")) == "1" else "2"  # models.py:77: anything but '1' is ResBlock2
        self._rates = list(get("upsample_rates"))
        self._up_k = list(get("upsample_kernel_sizes"))
        self._rb_k = list(get("resblock_kernel_sizes"))
        self._rb_d = [list(d) for d in get("resblock_dilation_sizes")]
        self._c0 = int(get("upsample_initial_channel"))
        self._in_dim = int(get("model_in_dim", 128))
        self._emb_dim = int(get("embedding_dim"))
        self._n_emb = int(get("num_embeddings"))
        self.f0 = get("f0", None)
        self.multispkr = get("multispkr", None)
        self._n_dil = 3 if self._kind == "1" else 2  # what the reference's constructors read (models.py:17-22, 51-54)
        if len(self._rb_d) < len(self._rb_k):
            raise IndexError("resblock_dilation_sizes has fewer entries than resblock_kernel_sizes")
        for d in self._rb_d[:len(self._rb_k)]:
            if len(d) < self._n_dil:
                raise IndexError("tuple index out of range")  # what `dilation[%d]` raises in the reference
        self._rb_d = [d[:self._n_dil] for d in self._rb_d[:len(self._rb_k)]]
        if len(self._rates) > _lib.MAX_STAGES or len(self._rb_k) > _lib.MAX_KERNELS:
            raise ValueError(f"TrainableCodeGenerator: at most {_lib.MAX_STAGES} stages and {_lib.MAX_KERNELS} resblock kernel sizes")
        self.num_kernels = len(self._rb_k)
        self.num_upsamples = len(self._rates)

        self.conv_pre = _TrainWNConv((self._c0, self._in_dim, 7), self._c0)
        self.ups = nn.ModuleList()
        self.resblocks = nn.ModuleList()
        for i, (u, k) in enumerate(zip(self._rates, self._up_k)):
            cin, cout = self._c0 // (2 ** i), self._c0 // (2 ** (i + 1))
            self.ups.append(_TrainWNConv((cin, cout, k), cout))
        for i in range(len(self._rates)):
            ch = self._c0 // (2 ** (i + 1))
            for k in self._rb_k:
                self.resblocks.append(_TrainResBlock(self._kind, ch, k, self._n_dil))
        self.conv_post = _TrainWNConv((1, self._c0 // (2 ** len(self._rates)), 7), 1)
        self.dict = nn.Embedding(self._n_emb, self._emb_dim)
        if self.multispkr:
            self.spkr = nn.Embedding(10, self._emb_dim)
        self._holder = {}  # "last": (cfg, B, U, saved) of the last training forward

    # ---- layout ---------------------------------------------------------------------------------------------------------------
    def _cfg(self) -> "_lib.VocCfg":
        cfg = _lib.VocCfg()
        cfg.num_embeddings, cfg.embedding_dim = self._n_emb, self._emb_dim
        cfg.multispkr, cfg.n_spkr = int(bool(self.multispkr)), 10
        cfg.model_in_dim, cfg.upsample_initial_channel = self._in_dim, self._c0
        cfg.n_stages = len(self._rates)
        for i, (u, k) in enumerate(zip(self._rates, self._up_k)):
            cfg.upsample_rates[i], cfg.upsample_kernel_sizes[i] = u, k
        cfg.n_kernels, cfg.n_dil = len(self._rb_k), self._n_dil
        for j, k in enumerate(self._rb_k):
            cfg.resblock_kernel_sizes[j] = k
            for m, d in enumerate(self._rb_d[j]):
                cfg.resblock_dilation_sizes[j][m] = d
        cfg.resblock_type = 1 if self._kind == "1" else 2
        return cfg

    def _wn_layers(self):
        """(kind, index, module) of every conv in the library's order: conv_pre, ups, the resblock convs as rb_w indexes them, conv_post."""
        out = [("pre", 0, self.conv_pre)] + [("ups", i, m) for i, m in enumerate(self.ups)]
        n = 0
        for rb in self.resblocks:
            for m in rb.ordered():
                out.append(("rb", n, m))
                n += 1
        return out + [("post", 0, self.conv_post)]

    def _table(self, dev):
        meta, params = [], []
        for kind, idx, m in self._wn_layers():
            if "weight" in m._parameters:
                fields = (("v", m.weight), ("bias", m.bias))
            else:
                fields = (("v", m.weight_v), ("g", m.weight_g), ("bias", m.bias))
            for f, p in fields:
                meta.append((kind, idx, f))
                params.append(p)
        meta.append(("dict", 0, ""))
        params.append(self.dict.weight)
        if self.multispkr:
            meta.append(("spkr", 0, ""))
            params.append(self.spkr.weight)
        for (kind, idx, f), t in zip(meta, params):
            name = f"{kind}[{idx}].{f}"
            require_cuda(t, name)
            if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"TrainableCodeGenerator: `{name}` must be a contiguous fp32 tensor on {dev} (got {t.dtype} on {t.device})")
        return tuple(meta), params

    def remove_weight_norm(self):
        """reference models.py:113-119 -- afterwards state_dict() has plain ``weight`` keys, and forward / backward run on them."""
        for _, _, m in self._wn_layers():
            m.remove_weight_norm()

    def out_samples(self, units: int) -> int:
        T = units
        for u, k in zip(self._rates, self._up_k):
            T = (T - 1) * u - 2 * ((k - u) // 2) + k
        return T if units > 0 else 0

    # ---- forward --------------------------------------------------------------------------------------------------------------
    def forward(self, **kwargs) -> torch.Tensor:
        """``generator(code=LongTensor(B, U), spkr=LongTensor(B, 1)) -> FloatTensor(B, 1, T)`` as in the reference (models.py:153-169)."""
        extra = [k for k in kwargs if k not in ("code", "spkr", "f0")]
        if extra:
            raise NotImplementedError(f"TrainableCodeGenerator: conditioning features are not trainable here (got {extra}); "
                                      "use parrot_tts_amd.vocoder.CodeGenerator for inference with them")
        if self._in_dim != self._emb_dim * (2 if self.multispkr else 1):
            raise NotImplementedError("TrainableCodeGenerator: model_in_dim must be embedding_dim * (1 + multispkr): conditioning features "
                                      "are not trainable here")
        code = kwargs["code"]
        require_cuda(code, "code")
        if code.dim() != 2 or code.dtype != torch.int64 or code.shape[0] < 1 or code.shape[1] < 1:
            raise ValueError("code must be a LongTensor of shape (B, U) with B, U >= 1")
        dev = code.device
        code = code.detach().contiguous()
        spkr = None
        if self.multispkr:
            if kwargs.get("spkr") is None:
                raise KeyError("spkr")
            spkr = kwargs["spkr"]
            require_cuda(spkr, "spkr")
            if spkr.dtype != torch.int64 or spkr.dim() > 2 or spkr.numel() != code.shape[0]:
                raise ValueError("spkr must be a LongTensor of shape (B, 1)")
            spkr = spkr.detach().reshape(-1).contiguous()
        # what nn.Embedding raises on, in one transfer
        bad = ((code < 0) | (code >= self._n_emb)).any()
        if spkr is not None:
            bad = bad | ((spkr < 0) | (spkr >= 10)).any()
        if bool(bad):
            raise IndexError("index out of range in self")
        meta, params = self._table(dev)
        cfg = self._cfg()
        if self.training and torch.is_grad_enabled():
            return _GeneratorTrainFn.apply(cfg, meta, code, spkr, self._holder, *params)
        with torch.no_grad():
            wav, _ = _train_forward(cfg, meta, params, code, spkr, False)
        return wav

    def lrelu_masks(self) -> List[torch.Tensor]:
        """The masks the backward of the last training forward applies, as bool tensors (B, C, T) in site order: True where the
        gradient passes unchanged (x > 0), False where it is multiplied by the slope."""
        if "last" not in self._holder:
            raise RuntimeError("lrelu_masks: no training forward has run")
        cfg, B, U, saved = self._holder["last"]
        lib = _lib.lib()
        dev = saved.device
        shapes, T = [], U
        per = self.num_kernels * self._n_dil * (2 if self._kind == "1" else 1)
        for i, (u, k) in enumerate(zip(self._rates, self._up_k)):
            shapes.append((B, self._c0 >> i, T))
            T = (T - 1) * u - 2 * ((k - u) // 2) + k
            shapes += [(B, self._c0 >> (i + 1), T)] * per
        shapes.append((B, self._c0 >> len(self._rates), T))
        assert len(shapes) == int(lib.parrot_voc_train_lrelu_sites(C.byref(cfg)))
        out = []
        with torch.cuda.device(dev):
            for s, shape in enumerate(shapes):
                m = torch.empty(shape, dtype=torch.uint8, device=dev)
                assert m.numel() == int(lib.parrot_voc_train_lrelu_site_elems(C.byref(cfg), B, U, s))
                _lib.check(lib.parrot_voc_train_lrelu_mask(C.byref(cfg), B, U, dptr(saved), s, dptr(m), stream_ptr(dev)))
                out.append(m.bool())
        return out
