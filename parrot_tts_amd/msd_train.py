"""Training the vocoder's multi-scale discriminator on the GPU: ``TrainableMultiScaleDiscriminator``, the reference's
``MultiScaleDiscriminator`` (utils/vocoder/models.py:228-276) -- spectral norm on discriminator 0, weight norm on the others, the two
average pools between them -- and its whole backward, backed by libparrot_hip.so (``parrot_msd_train_forward`` /
``parrot_msd_train_backward``).

    TrainableMultiScaleDiscriminator()      the reference's module: same state_dict keys, shapes and order
                                            (``discriminators.0.convs.{l}.bias|weight_orig|weight_u|weight_v``,
                                            ``discriminators.{i}.convs.{l}.bias|weight_g|weight_v`` for i >= 1, ``conv_post`` alike);
                                            channels and groups are arguments so that tests can run narrow
    .forward(y, y_hat)                      -> (y_d_rs, y_d_gs, fmap_rs, fmap_gs) with the reference's nesting and shapes.  The two
                                            waveforms run as ONE batch of 2 B rows; with grad enabled there is one autograd node over
                                            every parameter and, when ``y_hat`` requires grad, the waveform
    .remove_weight_norm()                   folds the weight-normed scales on the device; spectral norm stays (the reference never
                                            removes it)

Spectral norm follows the reference call by call: it runs the discriminator on ``y`` and then on ``y_hat``, and in training mode each
call starts with one power iteration.  So the real rows see ``weight_orig / sigma`` after one iteration, the generated rows after two,
and ``weight_u`` / ``weight_v`` end two iterations on -- under ``torch.no_grad()`` too.  In ``eval()`` nothing iterates, the buffers
stay bit for bit and both halves use one sigma.  The backward treats u and v as constants, as torch's does.

The maps handed out are views of the buffers the backward reads: autograd's version check refuses a backward after one of them was
written in place.  Nothing accumulates atomically, and ``torch.use_deterministic_algorithms(True)`` is supported.  There is no CPU
path: a CPU tensor raises."""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from .ops import _workspace, dptr, require_cuda, stream_ptr
from .vocoder_train import _TrainWNConv

LRELU_SLOPE = 0.1  # reference utils/vocoder/models.py:10
NL = _lib.MSD_LAYERS
KERNELS = (15, 41, 41, 41, 41, 41, 5)  # models.py:233-237; conv_post: 3
STRIDES = (1, 2, 2, 4, 4, 1, 1)


def _fill(ptrs: "_lib.MsdPtrs", meta, tensors) -> None:
    """Put every tensor's device pointer (None: null) into the field of an MsdPtrs that ``meta`` names: (scale, layer, field)."""
    for (i, l, field), t in zip(meta, tensors):
        setattr(ptrs.layer[i][l], field, None if t is None else t.data_ptr())


def _map_table(bufs) -> "_lib.MsdMaps":
    m = _lib.MsdMaps()
    for i, sc in enumerate(bufs):
        for l, t in enumerate(sc):
            m.map[i][l] = None if t is None else t.data_ptr()
    return m


def _shapes(cfg, N: int, T: int):
    """The shape (N, C, L) of every map: [scale][layer]."""
    lib = _lib.lib()
    widths = list(cfg.channels) + [1]
    return [[(N, widths[l], int(lib.parrot_msd_train_map_len(C.byref(cfg), T, i, l))) for l in range(NL)] for i in range(cfg.n_scales)]


def _train_forward(cfg, meta, params, bmeta, buffers, iters: int, wav, keep: bool):
    """One parrot_msd_train_forward call on validated tensors -> (the map buffers [scale][layer], saved buffer or None).  With
    ``iters`` = 1 the library moves the spectral layers' ``weight_u`` / ``weight_v`` two power iterations on, in place."""
    dev = wav.device
    N, T = int(wav.shape[0]), int(wav.shape[-1])
    lib = _lib.lib()
    with torch.cuda.device(dev):
        n_ws = int(lib.parrot_msd_train_workspace_bytes(C.byref(cfg), N, T))
        n_sv = int(lib.parrot_msd_train_saved_bytes(C.byref(cfg), N, T))
        # (beyond the limits every length is 0: the call then fails at the library's own shape check, on one-element maps)
        bufs = [[torch.empty(tuple(max(d, 1) for d in s), dtype=torch.float32, device=dev) for s in sc] for sc in _shapes(cfg, N, T)]
        ws = _workspace(n_ws, dev)
        saved = _workspace(n_sv, dev) if keep else None
        w = _lib.MsdPtrs()
        _fill(w, meta, params)
        _fill(w, bmeta, buffers)
        maps = _map_table(bufs)
        _lib.check(lib.parrot_msd_train_forward(C.byref(cfg), C.byref(w), dptr(wav), N, T, iters, C.byref(maps), dptr(saved), dptr(ws), n_ws,
                                                stream_ptr(dev)))
    return bufs, saved


def _views(bufs, B: int):
    """The real rows [0, B) and the generated rows [B, 2 B) of every map, scale by scale."""
    out = []
    for sc in bufs:
        for t in sc:
            out += [t[:B], t[B:]]
    return out


class _MsdTrainFn(torch.autograd.Function):
    """forward(cfg, meta, bmeta, buffers, iters, wav (2 B, 1, T), *parameters) -> for every scale and layer the real and the generated
    half of the map, as views of the buffer the library wrote; backward: one parrot_msd_train_backward call.  An output that received
    no gradient counts as zero, a parameter that needs no gradient gets none (its field is null and is not computed), the waveform's
    gradient is formed only when it is needed, and there is no double backward.  What the backward needs of the spectral layers'
    buffers is in the saved buffer: the module's own have moved on."""

    @staticmethod
    def forward(ctx, cfg, meta, bmeta, buffers, iters, wav, *params):
        bufs, saved = _train_forward(cfg, meta, params, bmeta, buffers, iters, wav, True)
        outs = _views(bufs, int(wav.shape[0]) // 2)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(wav, *params, *outs)
        ctx.cfg, ctx.meta, ctx.bmeta, ctx.buffers, ctx.saved, ctx.n_params = cfg, meta, bmeta, buffers, saved, len(params)
        ctx.bufs = bufs  # (the owners of the memory behind `outs`)
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *gouts):
        saved_t = ctx.saved_tensors  # (raises if a map was modified in place)
        wav, params = saved_t[0], saved_t[1:1 + ctx.n_params]
        dev = wav.device
        N, T = int(wav.shape[0]), int(wav.shape[-1])
        B = N // 2
        lib = _lib.lib()
        gbufs, k = [], 0
        for sc in ctx.bufs:
            row = []
            for t in sc:
                gr, gg = gouts[k], gouts[k + 1]
                k += 2
                if gr is None and gg is None:
                    row.append(None)
                    continue
                g = torch.empty_like(t)
                for half, src in ((g[:B], gr), (g[B:], gg)):
                    if src is None:
                        half.zero_()
                    else:
                        half.copy_(src)
                row.append(g)
            gbufs.append(row)
        grads = [torch.empty_like(p) if need else None for p, need in zip(params, ctx.needs_input_grad[6:])]
        gwav = torch.empty_like(wav) if ctx.needs_input_grad[5] else None
        g = _lib.MsdPtrs()
        _fill(g, ctx.meta, grads)
        with torch.cuda.device(dev):
            n_ws = int(lib.parrot_msd_train_workspace_bytes(C.byref(ctx.cfg), N, T))
            ws = _workspace(n_ws, dev)
            w = _lib.MsdPtrs()
            _fill(w, ctx.meta, params)
            _fill(w, ctx.bmeta, ctx.buffers)
            maps, gmaps = _map_table(ctx.bufs), _map_table(gbufs)
            _lib.check(lib.parrot_msd_train_backward(C.byref(ctx.cfg), C.byref(w), dptr(wav), C.byref(maps), dptr(ctx.saved), C.byref(gmaps), N, T,
                                                     C.byref(g), dptr(gwav), dptr(ws), n_ws, stream_ptr(dev)))
        return (None, None, None, None, None, gwav) + tuple(grads)


class _MsdWNConv(_TrainWNConv):
    """One weight-normed Conv1d of DiscriminatorS: weight_v (cout, cin / groups, k), weight_g (cout, 1, 1), bias (cout)."""

    def __init__(self, cout: int, cin: int, k: int, groups: int):
        nn.Module.__init__(self)
        conv = nn.Conv1d(cin, cout, k, groups=groups)  # (torch's own initialisation, as the reference's constructor draws it)
        v = conv.weight.detach().clone()
        self.bias = nn.Parameter(conv.bias.detach().clone())  # (the reference's key order: bias, weight_g, weight_v)
        self.weight_g = nn.Parameter(v.flatten(1).norm(dim=1).reshape(-1, 1, 1))
        self.weight_v = nn.Parameter(v)


class _MsdSNConv(nn.Module):
    """One spectral-normed Conv1d: bias and weight_orig (cout, cin / groups, k) are parameters, weight_u (cout) and weight_v
    (cin / groups k) buffers, unit vectors drawn as torch.nn.utils.spectral_norm draws them (no iteration at construction)."""

    def __init__(self, cout: int, cin: int, k: int, groups: int):
        super().__init__()
        conv = nn.Conv1d(cin, cout, k, groups=groups)
        w = conv.weight.detach().clone()
        self.bias = nn.Parameter(conv.bias.detach().clone())  # (the reference's key order: bias, weight_orig, then the buffers)
        self.weight_orig = nn.Parameter(w)
        self.register_buffer("weight_u", F.normalize(torch.randn(cout), dim=0, eps=1e-12))
        self.register_buffer("weight_v", F.normalize(torch.randn(w[0].numel()), dim=0, eps=1e-12))


class _DiscriminatorS(nn.Module):
    def __init__(self, channels, groups, use_spectral_norm: bool):
        super().__init__()
        make = _MsdSNConv if use_spectral_norm else _MsdWNConv
        c = [1] + list(channels)
        self.spectral = bool(use_spectral_norm)
        self.convs = nn.ModuleList([make(c[l + 1], c[l], KERNELS[l], groups[l]) for l in range(7)])
        self.conv_post = make(1, c[7], 3, 1)

    def layers(self):
        return list(self.convs) + [self.conv_post]


class TrainableMultiScaleDiscriminator(nn.Module):
    """The reference's ``MultiScaleDiscriminator`` as a trainable module on the HIP kernels: same ``state_dict`` keys, shapes, order."""

    def __init__(self, channels=(128, 128, 256, 512, 1024, 1024, 1024), groups=(1, 4, 16, 16, 16, 16, 1), n_scales: int = 3):
        super().__init__()
        channels, groups, n_scales = [int(c) for c in channels], [int(g) for g in groups], int(n_scales)
        if len(channels) != 7 or len(groups) != 7 or not 1 <= n_scales <= _lib.MSD_MAX_SCALES:
            raise ValueError(f"TrainableMultiScaleDiscriminator: seven channel widths, seven group counts and 1 to {_lib.MSD_MAX_SCALES} scales")
        cin = [1] + channels[:-1]
        if groups[0] != 1 or groups[6] != 1 or any(g < 1 or a % g or b % g for g, a, b in zip(groups, cin, channels)):
            raise ValueError("TrainableMultiScaleDiscriminator: groups[0] = groups[6] = 1, and every group count divides both of its widths")
        self.channels, self.groups, self.n_scales = channels, groups, n_scales
        self.discriminators = nn.ModuleList([_DiscriminatorS(channels, groups, i == 0) for i in range(n_scales)])
        self.meanpools = nn.ModuleList([nn.AvgPool1d(4, 2, padding=2) for _ in range(n_scales - 1)])  # (no state: the library pools)

    # ---- layout ---------------------------------------------------------------------------------------------------------------
    def _cfg(self) -> "_lib.MsdCfg":
        cfg = _lib.MsdCfg()
        cfg.n_scales = self.n_scales
        for i, d in enumerate(self.discriminators):
            cfg.spectral[i] = int(d.spectral)
        for i, (c, g) in enumerate(zip(self.channels, self.groups)):
            cfg.channels[i], cfg.groups[i] = c, g
        cfg.slope = LRELU_SLOPE
        return cfg

    def _table(self, dev):
        """-> (meta, parameters, buffer meta, buffers): the differentiable tensors and the spectral layers' u / v, each with its field."""
        meta, params, bmeta, buffers = [], [], [], []
        for i, d in enumerate(self.discriminators):
            for l, m in enumerate(d.layers()):
                if d.spectral:
                    fields = (("v", m.weight_orig), ("bias", m.bias))
                    bmeta += [(i, l, "u"), (i, l, "sv")]
                    buffers += [m.weight_u, m.weight_v]
                elif "weight" in m._parameters:
                    fields = (("v", m.weight), ("bias", m.bias))
                else:
                    fields = (("v", m.weight_v), ("g", m.weight_g), ("bias", m.bias))
                for f, p in fields:
                    meta.append((i, l, f))
                    params.append(p)
        for (i, l, f), t in zip(meta + bmeta, params + buffers):
            name = f"discriminators.{i}.{'conv_post' if l == NL - 1 else 'convs.%d' % l}.{f}"
            require_cuda(t, name)
            if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"TrainableMultiScaleDiscriminator: `{name}` must be a contiguous fp32 tensor on {dev} "
                                 f"(got {t.dtype} on {t.device})")
        return tuple(meta), params, tuple(bmeta), tuple(buffers)

    def remove_weight_norm(self):
        """Afterwards the weight-normed scales have plain ``weight`` keys, and forward / backward run on them.  Spectral norm stays."""
        for d in self.discriminators:
            if not d.spectral:
                for m in d.layers():
                    m.remove_weight_norm()

    # ---- forward --------------------------------------------------------------------------------------------------------------
    def forward(self, y: torch.Tensor, y_hat: torch.Tensor):
        """``msd(y, y_hat) -> (y_d_rs, y_d_gs, fmap_rs, fmap_gs)`` as in the reference (models.py:260-276): per scale the score (B, L)
        of the real and of the generated rows, and the eight feature maps (B, C, L) of each."""
        for name, t in (("y", y), ("y_hat", y_hat)):
            require_cuda(t, name)
            if t.dim() != 3 or t.shape[1] != 1 or t.dtype != torch.float32 or t.shape[0] < 1 or t.shape[2] < 1:
                raise ValueError(f"{name} must be a FloatTensor of shape (B, 1, T) with B, T >= 1")
        if y.shape != y_hat.shape or y.device != y_hat.device:
            raise ValueError(f"y and y_hat must have one shape and one device (got {tuple(y.shape)} and {tuple(y_hat.shape)})")
        dev, B = y.device, int(y.shape[0])
        meta, params, bmeta, buffers = self._table(dev)
        cfg = self._cfg()
        iters = 1 if self.training else 0
        wav = torch.cat([y, y_hat], dim=0).contiguous()
        if torch.is_grad_enabled() and (wav.requires_grad or any(p.requires_grad for p in params)):
            outs = _MsdTrainFn.apply(cfg, meta, bmeta, buffers, iters, wav, *params)
        else:
            with torch.no_grad():
                outs = _views(_train_forward(cfg, meta, params, bmeta, buffers, iters, wav.detach(), False)[0], B)
        y_d_rs, y_d_gs, fmap_rs, fmap_gs = [], [], [], []
        for i in range(self.n_scales):
            sc = outs[2 * NL * i:2 * NL * (i + 1)]
            fmap_rs.append(list(sc[0::2]))
            fmap_gs.append(list(sc[1::2]))
            y_d_rs.append(torch.flatten(sc[-2], 1, -1))
            y_d_gs.append(torch.flatten(sc[-1], 1, -1))
        return y_d_rs, y_d_gs, fmap_rs, fmap_gs
