"""Training the vocoder's multi-period discriminator on the GPU: ``TrainableMultiPeriodDiscriminator``, the reference's
``MultiPeriodDiscriminator`` (utils/vocoder/models.py:171-225) with weight norm attached and its whole backward, backed by
libparrot_hip.so (``parrot_mpd_train_forward`` / ``parrot_mpd_train_backward``).

    TrainableMultiPeriodDiscriminator()     the reference's module: same state_dict keys and shapes
                                            (``discriminators.{i}.convs.{l}.weight_g|weight_v|bias``, ``discriminators.{i}.conv_post.*``);
                                            periods, channels, kernel_size and stride are arguments so that tests can run narrow
    .forward(y, y_hat)                      -> (y_d_rs, y_d_gs, fmap_rs, fmap_gs) with the reference's nesting and shapes.  The two
                                            waveforms run as ONE batch of 2 B rows; with grad enabled there is one autograd node over
                                            every parameter and, when ``y_hat`` requires grad, the waveform
    .remove_weight_norm()                   folds on the device; the module keeps working, and training, on plain weights

The library keeps a map period-major, (N, p, C, H); what is returned are views of that memory in torch's shape (N, C, H, p), so a
consumer that wants dense memory (``gan_loss``) copies it once, and a score is the flattened copy of the sixth map.  The maps handed
out are the buffers the backward reads: autograd's version check refuses a backward after one of them was written in place.
Nothing accumulates atomically, and ``torch.use_deterministic_algorithms(True)`` is supported.  There is no CPU path: a CPU tensor
raises.  The multi-scale discriminator (spectral norm, grouped convs) is ``msd_train.TrainableMultiScaleDiscriminator``;
``use_spectral_norm=True`` raises here."""
from __future__ import annotations

import ctypes as C

import torch
from torch import nn

from . import _lib
from .ops import _workspace, dptr, require_cuda, stream_ptr
from .vocoder_train import _TrainWNConv

LRELU_SLOPE = 0.1  # reference utils/vocoder/models.py:10
NL = _lib.MPD_LAYERS


def _fill(ptrs: "_lib.MpdPtrs", meta, tensors) -> None:
    """Put every tensor's device pointer (None: null) into the field of an MpdPtrs that ``meta`` names: (period index, layer, field)."""
    for (i, l, field), t in zip(meta, tensors):
        setattr(ptrs.layer[i][l], field, None if t is None else t.data_ptr())


def _map_table(bufs) -> "_lib.MpdMaps":
    m = _lib.MpdMaps()
    for i, per in enumerate(bufs):
        for l, t in enumerate(per):
            m.map[i][l] = None if t is None else t.data_ptr()
    return m


def _shapes(cfg, N: int, T: int):
    """The period-major shape (N, p, C, H) of every map: [period][layer]."""
    lib = _lib.lib()
    widths = [cfg.channels[0], cfg.channels[1], cfg.channels[2], cfg.channels[3], cfg.channels[3], 1]
    return [[(N, cfg.periods[i], widths[l], int(lib.parrot_mpd_train_map_rows(C.byref(cfg), T, i, l))) for l in range(NL)]
            for i in range(cfg.n_periods)]


def _train_forward(cfg, meta, params, wav, keep: bool):
    """One parrot_mpd_train_forward call on validated tensors -> (the period-major map buffers [period][layer], saved buffer or None)."""
    dev = wav.device
    N, T = int(wav.shape[0]), int(wav.shape[-1])
    lib = _lib.lib()
    with torch.cuda.device(dev):
        n_ws = int(lib.parrot_mpd_train_workspace_bytes(C.byref(cfg), N, T))
        n_sv = int(lib.parrot_mpd_train_saved_bytes(C.byref(cfg), N, T))
        # (beyond the limits every row count is 0: the call then fails at the library's own shape check, on one-element maps)
        bufs = [[torch.empty(tuple(max(d, 1) for d in s), dtype=torch.float32, device=dev) for s in per] for per in _shapes(cfg, N, T)]
        ws = _workspace(n_ws, dev)
        saved = _workspace(n_sv, dev) if keep else None
        w = _lib.MpdPtrs()
        _fill(w, meta, params)
        maps = _map_table(bufs)
        _lib.check(lib.parrot_mpd_train_forward(C.byref(cfg), C.byref(w), dptr(wav), N, T, C.byref(maps), dptr(saved), dptr(ws), n_ws,
                                                stream_ptr(dev)))
    return bufs, saved


def _views(bufs, B: int):
    """Torch's shape (rows, C, H, p) of the real rows [0, B) and the generated rows [B, 2 B) of every map, period by period."""
    out = []
    for per in bufs:
        for t in per:
            v = t.permute(0, 2, 3, 1)
            out += [v[:B], v[B:]]
    return out


class _MpdTrainFn(torch.autograd.Function):
    """forward(cfg, meta, wav (2 B, 1, T), *parameters) -> for every period and layer the real and the generated half of the map, as
    views of the buffer the library wrote; backward: one parrot_mpd_train_backward call.  An output that received no gradient counts
    as zero, a parameter that needs no gradient gets none (its field is null and is not computed), the waveform's gradient is formed
    only when it is needed, and there is no double backward."""

    @staticmethod
    def forward(ctx, cfg, meta, wav, *params):
        bufs, saved = _train_forward(cfg, meta, params, wav, True)
        outs = _views(bufs, int(wav.shape[0]) // 2)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(wav, *params, *outs)
        ctx.cfg, ctx.meta, ctx.saved, ctx.n_params = cfg, meta, saved, len(params)
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
        for per in ctx.bufs:
            row = []
            for t in per:
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
                        half.copy_(src.permute(0, 3, 1, 2))
                row.append(g)
            gbufs.append(row)
        grads = [torch.empty_like(p) if need else None for p, need in zip(params, ctx.needs_input_grad[3:])]
        gwav = torch.empty_like(wav) if ctx.needs_input_grad[2] else None
        g = _lib.MpdPtrs()
        _fill(g, ctx.meta, grads)
        with torch.cuda.device(dev):
            n_ws = int(lib.parrot_mpd_train_workspace_bytes(C.byref(ctx.cfg), N, T))
            ws = _workspace(n_ws, dev)
            w = _lib.MpdPtrs()
            _fill(w, ctx.meta, params)
            maps, gmaps = _map_table(ctx.bufs), _map_table(gbufs)
            _lib.check(lib.parrot_mpd_train_backward(C.byref(ctx.cfg), C.byref(w), dptr(wav), C.byref(maps), dptr(ctx.saved), C.byref(gmaps), N, T,
                                                     C.byref(g), dptr(gwav), dptr(ws), n_ws, stream_ptr(dev)))
        return (None, None, gwav) + tuple(grads)


class _MpdConv(_TrainWNConv):
    """One weight-normed Conv2d of DiscriminatorP: weight_v (cout, cin, k, 1), weight_g (cout, 1, 1, 1), bias (cout)."""

    def __init__(self, cout: int, cin: int, k: int):
        nn.Module.__init__(self)
        conv = nn.Conv2d(cin, cout, (k, 1))  # (torch's own initialisation, as the reference's constructor draws it)
        v = conv.weight.detach().clone()
        self.bias = nn.Parameter(conv.bias.detach().clone())  # (the reference's key order: bias, weight_g, weight_v)
        self.weight_g = nn.Parameter(v.flatten(1).norm(dim=1).reshape(-1, 1, 1, 1))
        self.weight_v = nn.Parameter(v)


class _DiscriminatorP(nn.Module):
    def __init__(self, period: int, channels, kernel_size: int):
        super().__init__()
        self.period = period
        c = [1] + list(channels) + [channels[-1]]
        self.convs = nn.ModuleList([_MpdConv(c[l + 1], c[l], kernel_size) for l in range(5)])
        self.conv_post = _MpdConv(1, c[5], 3)

    def layers(self):
        return list(self.convs) + [self.conv_post]


class TrainableMultiPeriodDiscriminator(nn.Module):
    """The reference's ``MultiPeriodDiscriminator`` as a trainable module on the HIP kernels: same ``state_dict`` keys and shapes."""

    def __init__(self, periods=(2, 3, 5, 7, 11), channels=(32, 128, 512, 1024), kernel_size: int = 5, stride: int = 3,
                 use_spectral_norm: bool = False):
        super().__init__()
        if use_spectral_norm:
            raise NotImplementedError("TrainableMultiPeriodDiscriminator: spectral norm is the multi-scale discriminator's (MSD): "
                                      "see parrot_tts_amd.msd_train.TrainableMultiScaleDiscriminator")
        periods, channels = [int(p) for p in periods], [int(c) for c in channels]
        if not 1 <= len(periods) <= _lib.MPD_MAX_PERIODS or len(channels) != 4:
            raise ValueError(f"TrainableMultiPeriodDiscriminator: 1 to {_lib.MPD_MAX_PERIODS} periods and four channel widths")
        self.periods, self.channels, self.kernel_size, self.stride = periods, channels, int(kernel_size), int(stride)
        self.discriminators = nn.ModuleList([_DiscriminatorP(p, channels, self.kernel_size) for p in periods])

    # ---- layout ---------------------------------------------------------------------------------------------------------------
    def _cfg(self) -> "_lib.MpdCfg":
        cfg = _lib.MpdCfg()
        cfg.n_periods = len(self.periods)
        for i, p in enumerate(self.periods):
            cfg.periods[i] = p
        for i, c in enumerate(self.channels):
            cfg.channels[i] = c
        cfg.kernel_size, cfg.stride, cfg.slope = self.kernel_size, self.stride, LRELU_SLOPE
        return cfg

    def _table(self, dev):
        meta, params = [], []
        for i, d in enumerate(self.discriminators):
            for l, m in enumerate(d.layers()):
                if "weight" in m._parameters:
                    fields = (("v", m.weight), ("bias", m.bias))
                else:
                    fields = (("v", m.weight_v), ("g", m.weight_g), ("bias", m.bias))
                for f, p in fields:
                    meta.append((i, l, f))
                    params.append(p)
        for (i, l, f), t in zip(meta, params):
            name = f"discriminators.{i}.{'conv_post' if l == NL - 1 else 'convs.%d' % l}.{f}"
            require_cuda(t, name)
            if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"TrainableMultiPeriodDiscriminator: `{name}` must be a contiguous fp32 tensor on {dev} "
                                 f"(got {t.dtype} on {t.device})")
        return tuple(meta), params

    def remove_weight_norm(self):
        """Afterwards state_dict() has plain ``weight`` keys, and forward / backward run on them."""
        for d in self.discriminators:
            for m in d.layers():
                m.remove_weight_norm()

    # ---- forward --------------------------------------------------------------------------------------------------------------
    def forward(self, y: torch.Tensor, y_hat: torch.Tensor):
        """``mpd(y, y_hat) -> (y_d_rs, y_d_gs, fmap_rs, fmap_gs)`` as in the reference (models.py:212-225): per period the score
        (B, H p) of the real and of the generated rows, and the six feature maps (B, C, H, p) of each."""
        for name, t in (("y", y), ("y_hat", y_hat)):
            require_cuda(t, name)
            if t.dim() != 3 or t.shape[1] != 1 or t.dtype != torch.float32 or t.shape[0] < 1 or t.shape[2] < 1:
                raise ValueError(f"{name} must be a FloatTensor of shape (B, 1, T) with B, T >= 1")
        if y.shape != y_hat.shape or y.device != y_hat.device:
            raise ValueError(f"y and y_hat must have one shape and one device (got {tuple(y.shape)} and {tuple(y_hat.shape)})")
        T = int(y.shape[-1])
        for p in self.periods:
            if T % p and T <= p - T % p:  # (what F.pad(..., "reflect") raises on, before anything runs)
                raise RuntimeError(f"Padding size should be less than the corresponding input dimension, but got: padding (0, {p - T % p}) "
                                   f"at dimension 2 of input {list(y.shape)}")
        dev, B = y.device, int(y.shape[0])
        meta, params = self._table(dev)
        cfg = self._cfg()
        wav = torch.cat([y, y_hat], dim=0).contiguous()
        if torch.is_grad_enabled() and (wav.requires_grad or any(p.requires_grad for p in params)):
            outs = _MpdTrainFn.apply(cfg, meta, wav, *params)
        else:
            with torch.no_grad():
                outs = _views(_train_forward(cfg, meta, params, wav.detach(), False)[0], B)
        y_d_rs, y_d_gs, fmap_rs, fmap_gs = [], [], [], []
        for i in range(len(self.periods)):
            per = outs[2 * NL * i:2 * NL * (i + 1)]
            fmap_rs.append(list(per[0::2]))
            fmap_gs.append(list(per[1::2]))
            y_d_rs.append(torch.flatten(per[-2], 1, -1))
            y_d_gs.append(torch.flatten(per[-1], 1, -1))
        return y_d_rs, y_d_gs, fmap_rs, fmap_gs
