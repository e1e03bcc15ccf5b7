"""The vocoder's validation metric on the GPU: ``mel_spectrogram`` of reference utils/vocoder/dataset.py:43-69 and the L1
distance of two log-mel spectrograms (``F.l1_loss``, utils/vocoder/train.py:213), backed by libparrot_hip.so
(``parrot_mel_forward`` / ``parrot_mel_l1``).

    mel_spectrogram(y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center=False)   the reference's signature
    MelSpectrogram(h)(wav, n_samples=None)                                                             ragged batches
    mel_l1(a, b, n_frames=None) -> (batch mean, per-row means)
    MelSpectrogram.l1_loss_and_grad(wav, target, n_samples=None, reduction="mean") -> (loss, d loss / d wav)
    mel_l1_trainable(mel, wav, target, ...) / MelL1Loss(h)(y_g_hat, y_mel)                             the training loss (train.py:157)

The library is handed the window (``torch.hann_window(win_size)``, fp32, as the reference builds it) and the mel basis
(``slaney_mel_basis``); the framed DFT and the mel projection run on the conv kernels in a parity-grade precision (f16x3 by
default, never the bf16 / f16 operating point of the vocoder), everything else in the streaming kernels of csrc/mel.h.  There is
no CPU path: a CPU tensor raises, as in the other shims."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch
from torch import nn

from . import _lib
from .ops import PREC_STR, _prec_arg, _workspace, dptr, require_cuda, stream_ptr


# ---------------------------------------------------------------------------------------------
# mel basis
# ---------------------------------------------------------------------------------------------
_F_SP = 200.0 / 3            # Slaney scale: linear below 1 kHz, 200/3 Hz per mel ...
_MIN_LOG_HZ = 1000.0
_MIN_LOG_MEL = _MIN_LOG_HZ / _F_SP
_LOGSTEP = np.log(6.4) / 27.0  # ... logarithmic above: 27 mels per factor 6.4


def hz_to_mel(f):
    """Slaney's Auditory Toolbox scale (librosa.hz_to_mel with htk=False)."""
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= _MIN_LOG_HZ, _MIN_LOG_MEL + np.log(np.maximum(f, 1e-300) / _MIN_LOG_HZ) / _LOGSTEP, f / _F_SP)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= _MIN_LOG_MEL, _MIN_LOG_HZ * np.exp(_LOGSTEP * (m - _MIN_LOG_MEL)), _F_SP * m)


def slaney_mel_basis(sr, n_fft, n_mels, fmin=0.0, fmax=None) -> np.ndarray:
    """``librosa.filters.mel(sr=, n_fft=, n_mels=, fmin=, fmax=)`` with its defaults (Slaney scale, ``norm='slaney'``, float32) ->
    (n_mels, n_fft // 2 + 1): triangles between n_mels + 2 points equally spaced on the mel scale, each divided by half its
    width in Hz.  ``librosa`` itself is used when it is importable; otherwise this restatement of its published algorithm, in
    its order of operations (fp64 ramps, triangles rounded to float32, then the normalisation).  The restatement could NOT be
    compared against librosa where it was written (the package was not available): its tests pin the properties of the filter
    bank (shape, single triangles, row sums, the scale), not librosa's bits."""
    fmax = float(sr) / 2 if fmax is None else float(fmax)
    try:
        from librosa.filters import mel as librosa_mel
        return np.asarray(librosa_mel(sr=sr, n_fft=n_fft, n_mels=n_mels, fmin=fmin, fmax=fmax), dtype=np.float32)
    except ImportError:
        return slaney_mel_basis_restated(sr, n_fft, n_mels, fmin, fmax)


def slaney_mel_basis_restated(sr, n_fft, n_mels, fmin=0.0, fmax=None) -> np.ndarray:
    """``slaney_mel_basis`` without looking for librosa."""
    fmax = float(sr) / 2 if fmax is None else float(fmax)
    n_freq = n_fft // 2 + 1
    fftfreqs = np.linspace(0.0, float(sr) / 2, n_freq)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    weights = np.zeros((n_mels, n_freq), dtype=np.float32)
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        weights[i] = np.maximum(0.0, np.minimum(lower, upper))
    enorm = 2.0 / (mel_f[2: n_mels + 2] - mel_f[:n_mels])
    return (weights.astype(np.float64) * enorm[:, None]).astype(np.float32)


# ---------------------------------------------------------------------------------------------
# handles
# ---------------------------------------------------------------------------------------------
_FIELDS = ("n_fft", "num_mels", "sampling_rate", "hop_size", "win_size", "fmin")


class MelSpectrogram:
    """The reference's ``mel_spectrogram`` with a configuration fixed up front; ``h``: the vocoder config (n_fft, num_mels,
    sampling_rate, hop_size, win_size, fmin and ``fmax_for_loss`` -- the validation metric's upper edge, train.py:211-212;
    ``None`` / absent = sampling_rate / 2).  Keywords override the config's fields (``fmax=h.fmax`` gives the plotting mel).

    ``__call__(wav, n_samples=None)``: wav (B, N) fp32 on the GPU -> (B, num_mels, N // hop_size).  ``n_samples`` (B): real
    samples per row of a padded batch -- the reflection happens at each row's own end, row b has n_samples[b] // hop_size frames
    that equal that utterance run alone bit for bit, frames beyond are zero.  Counts given on the host (a list, a CPU tensor) must
    lie in [0, N] or ValueError is raised; a device tensor is not read back and the kernels clamp it.  ``precision``: 'f16x3' (default), 'bf16x6', 'f32';
    under PARROT_PRECISION=bf16 / f16 the default stays f16x3."""

    def __init__(self, h=None, *, precision=None, basis: Optional[np.ndarray] = None, window: Optional[torch.Tensor] = None, **kw):
        h = dict(h or {})
        cfg = {k: kw.pop(k, h.get(k)) for k in _FIELDS}
        fmax = kw.pop("fmax", h.get("fmax_for_loss"))
        if kw:
            raise TypeError(f"MelSpectrogram: unexpected arguments {sorted(kw)}")
        missing = [k for k, v in cfg.items() if v is None]
        if missing:
            raise ValueError(f"MelSpectrogram: missing {missing}")
        self.n_fft, self.num_mels, self.hop_size, self.win_size = (int(cfg[k]) for k in ("n_fft", "num_mels", "hop_size", "win_size"))
        self.sampling_rate, self.fmin = cfg["sampling_rate"], cfg["fmin"]
        self.fmax = float(self.sampling_rate) / 2 if fmax is None else fmax
        self.n_freq = self.n_fft // 2 + 1
        self.pad = (self.n_fft - self.hop_size) // 2
        self.precision = _prec_arg(precision)
        basis = slaney_mel_basis(self.sampling_rate, self.n_fft, self.num_mels, self.fmin, self.fmax) if basis is None else basis
        self.basis = torch.from_numpy(np.ascontiguousarray(basis, dtype=np.float32))
        if tuple(self.basis.shape) != (self.num_mels, self.n_freq):
            raise ValueError(f"mel basis must be ({self.num_mels}, {self.n_freq}), got {tuple(self.basis.shape)}")
        self.window = (torch.hann_window(self.win_size) if window is None else window.detach().cpu()).to(torch.float32).contiguous()
        if self.window.numel() != self.win_size:
            raise ValueError("window must hold win_size values")
        self._handles = {}  # device index -> parrot_mel_t*

    def frames(self, n_samples: int) -> int:
        return int(n_samples) // self.hop_size

    def _handle(self, dev: torch.device):
        h = self._handles.get(dev.index)
        if h is None:
            cfg = _lib.MelCfg(self.n_fft, self.hop_size, self.win_size, self.num_mels)
            h = C.c_void_p()
            with torch.cuda.device(dev):
                _lib.check(_lib.lib().parrot_mel_create_ex(C.byref(h), C.byref(cfg), _lib.fptr(self.window), _lib.fptr(self.basis), self.precision))
            self._handles[dev.index] = h
        return h

    def precision_in_use(self, device="cuda") -> str:
        dev = torch.device(device)
        dev = torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev
        return PREC_STR[int(_lib.lib().parrot_mel_precision(self._handle(dev)))]

    def _args(self, wav: torch.Tensor, n_samples):
        """-> (wav (B, N) fp32 with unit sample stride, n_samples (B) int32 on the device or None), validated."""
        require_cuda(wav, "wav")
        if wav.dim() == 3 and wav.shape[1] == 1:  # the generator's (B, 1, N)
            wav = wav[:, 0]
        if wav.dim() != 2:
            raise ValueError(f"mel_spectrogram: expected (B, N) samples, got {tuple(wav.shape)}")
        wav = wav.to(torch.float32)
        if wav.stride(1) != 1 or wav.stride(0) < wav.shape[1]:
            wav = wav.contiguous()
        dev = wav.device
        B, N = wav.shape
        if N <= self.pad and n_samples is None:  # F.pad's own message (dataset.py:55)
            raise RuntimeError(f"Argument #4: Padding size should be less than the corresponding input dimension, but got: padding "
                               f"({self.pad}, {self.pad}) at dimension 2 of input {[B, 1, N]}")
        if N < self.hop_size:
            raise RuntimeError(f"mel_spectrogram: {N} samples hold no frame of hop_size {self.hop_size}")
        ns = None
        if n_samples is not None:
            ns = torch.as_tensor(n_samples)
            if tuple(ns.shape) != (B,):
                raise ValueError(f"n_samples must hold one count per row ({B}), got {tuple(ns.shape)}")
            # host counts are checked here (a device tensor is not read back: the kernels clamp it to [0, N])
            if not ns.is_cuda and B and (int(ns.min()) < 0 or int(ns.max()) > N):
                raise ValueError(f"n_samples must lie in [0, {N}] (samples of a row of the padded batch), got {ns.tolist()}")
            ns = ns.to(dev, torch.int32).contiguous()
        return wav, ns

    @torch.no_grad()
    def __call__(self, wav: torch.Tensor, n_samples=None, check: bool = True) -> torch.Tensor:
        wav, ns = self._args(wav, n_samples)
        dev = wav.device
        B, N = wav.shape
        lib = _lib.lib()
        out = torch.empty((B, self.num_mels, N // self.hop_size), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            h = self._handle(dev)
            ws = _workspace(lib.parrot_mel_workspace_bytes(h, B, N), dev)
            _lib.check(lib.parrot_mel_forward(h, dptr(wav), wav.stride(0), dptr(ns), B, N, dptr(out), dptr(ws), ws.numel(), stream_ptr(dev)))
            if check:
                self.check(dev)
        return out

    @torch.no_grad()
    def l1_loss_and_grad(self, wav: torch.Tensor, target: torch.Tensor, n_samples=None, reduction: str = "mean") -> Tuple[torch.Tensor, torch.Tensor]:
        """The generator's mel loss (train.py:157, ``F.l1_loss(y_mel, y_g_hat_mel)`` before the factor 45) and its gradient with
        respect to the waveform in one device call: -> (loss, grad (B, N) fp32).  ``target`` (B, num_mels, N // hop_size) fp32.
        "mean": ``loss`` is ``mel_l1(self(wav, n_samples), target, n_samples // hop_size)[0]`` bit for bit (0-dim fp32); "sum": the
        sum of |a - b| over the real elements, every one weighted 1 (0-dim fp64), so that a row's gradient depends on that row
        alone.  ``grad = d loss / d wav``: torch's autograd of dataset.py:55-67 (sgn with 0 at 0, the clamp passing where
        mel >= 1e-5, the magnitude's gradient finite at 0, the reflect pad folding at each row's own end), exactly 0 at and beyond
        ``n_samples[b]``.  No atomics on values: two calls agree bit for bit.  Raises as ``__call__`` (a short row, a non-finite
        value: nothing is returned then)."""
        if reduction not in ("mean", "sum"):
            raise ValueError(f"l1_loss_and_grad: reduction must be 'mean' or 'sum', got {reduction!r}")
        wav, ns = self._args(wav, n_samples)
        require_cuda(target, "target")
        dev = wav.device
        B, N = wav.shape
        want = (B, self.num_mels, N // self.hop_size)
        if tuple(target.shape) != want:
            raise ValueError(f"l1_loss_and_grad: target must be {want} (B, num_mels, N // hop_size), got {tuple(target.shape)}")
        target = target.detach().to(dev, torch.float32).contiguous()
        lib = _lib.lib()
        mean = reduction == "mean"
        out = torch.empty(2 * B, dtype=torch.float64, device=dev)
        loss = torch.empty((), dtype=torch.float32 if mean else torch.float64, device=dev)
        grad = torch.empty((B, N), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            h = self._handle(dev)
            ws = _workspace(lib.parrot_mel_l1_grad_workspace_bytes(h, B, N), dev)
            _lib.check(lib.parrot_mel_l1_grad(h, dptr(wav), wav.stride(0), dptr(ns), dptr(target), B, N, 0 if mean else 1, 1.0,
                                              dptr(out), dptr(loss), dptr(grad), dptr(ws), ws.numel(), stream_ptr(dev)))
            self.check(dev)
        return loss, grad

    def check(self, device) -> None:
        """Synchronise and raise what the device flagged since the last check: a row no longer than the reflect pad
        (the reference's F.pad raises), a non-finite mel (or gradient) value."""
        dev = torch.device(device)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().parrot_mel_check(self._handle(dev), stream_ptr(dev)))

    def __del__(self, _destroy=_lib.destroy):  # (bound here: module globals are already torn down at interpreter exit)
        for h in getattr(self, "_handles", {}).values():
            _destroy("parrot_mel_destroy", h)


_cache = {}  # the reference keeps mel_basis / hann_window in module globals keyed by fmax and device (dataset.py:49-53)


def mel_spectrogram(y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center=False):
    """reference utils/vocoder/dataset.py:43-69, same signature: y (B, N) in [-1, 1] on the GPU -> log-mel (B, num_mels, N // hop_size).
    Handles are cached per configuration (and, inside, per device).  ``center=True`` (never used by the reference) raises."""
    if center:
        raise NotImplementedError("mel_spectrogram: center=True is not covered (the reference always passes center=False)")
    require_cuda(y, "y")
    key = (int(n_fft), int(num_mels), sampling_rate, int(hop_size), int(win_size), fmin, fmax)
    m = _cache.get(key)
    if m is None:
        m = _cache[key] = MelSpectrogram(n_fft=n_fft, num_mels=num_mels, sampling_rate=sampling_rate, hop_size=hop_size,
                                         win_size=win_size, fmin=fmin, fmax=fmax)
    return m(y)


@torch.no_grad()
def mel_l1(a: torch.Tensor, b: torch.Tensor, n_frames=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """L1 distance of two (B, n_mels, T) fp32 spectrograms on the GPU -> (mean, row_means): ``mean`` a 0-dim fp32 tensor, the
    sum over all rows' elements divided by their number (``F.l1_loss(a, b)`` when the rows are of one length); ``row_means``
    (B,) fp64, each row's own mean over n_mels x n_frames[b] elements (NaN for a row without frames).  ``n_frames`` (B): real
    frames per row; frames beyond do not enter.  fp64 sums in a fixed order: two calls agree bit for bit."""
    require_cuda(a, "a")
    require_cuda(b, "b")
    if a.shape != b.shape or a.dim() != 3:
        raise ValueError(f"mel_l1: two (B, n_mels, T) tensors of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    dev = a.device
    a, b = a.to(torch.float32).contiguous(), b.to(dev, torch.float32).contiguous()
    B, M, T = a.shape
    nf = None
    if n_frames is not None:
        nf = torch.as_tensor(n_frames).to(dev, torch.int32).contiguous()
        if tuple(nf.shape) != (B,):
            raise ValueError(f"n_frames must hold one count per row ({B}), got {tuple(nf.shape)}")
    lib = _lib.lib()
    out = torch.empty(2 * B, dtype=torch.float64, device=dev)
    mean = torch.empty((), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        ws = _workspace(lib.parrot_mel_l1_workspace_bytes(B, M, T), dev)
        _lib.check(lib.parrot_mel_l1(dptr(a), dptr(b), dptr(nf), B, M, T, dptr(out), dptr(mean), dptr(ws), ws.numel(), stream_ptr(dev)))
    return mean, out[:B] / out[B:]


class _MelL1Fn(torch.autograd.Function):
    """With a waveform that requires a gradient the forward is ONE ``parrot_mel_l1_grad`` call whose unit-scale gradient is kept
    for the backward (training always calls it: nothing is computed twice); otherwise the plain forward and ``mel_l1``.  Only the
    waveform gets a gradient, and there is no double backward."""

    @staticmethod
    def forward(ctx, wav, mel, target, n_samples, reduction):
        ctx.in_shape, ctx.in_dtype = wav.shape, wav.dtype
        # ("sum" without a gradient to keep also takes the one call: its value is the fp64 row sums added in row order on the device,
        # which mel_l1's per-row means do not give back bit for bit; the gradient written beside it is dropped)
        if ctx.needs_input_grad[0] or reduction != "mean":
            loss, grad = mel.l1_loss_and_grad(wav, target, n_samples, reduction)
            if ctx.needs_input_grad[0]:
                ctx.save_for_backward(grad)
            return loss
        n_frames = None if n_samples is None else torch.div(torch.as_tensor(n_samples), mel.hop_size, rounding_mode="floor")
        return mel_l1(mel(wav, n_samples), target, n_frames)[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        (grad,) = ctx.saved_tensors
        g = grad * grad_output.detach().to(grad.device, torch.float32)  # (a 0-dim grad_output broadcasts)
        return g.reshape(ctx.in_shape).to(ctx.in_dtype), None, None, None, None


def mel_l1_trainable(mel: MelSpectrogram, wav: torch.Tensor, target: torch.Tensor, n_samples=None, reduction: str = "mean") -> torch.Tensor:
    """``mel_l1(mel(wav, n_samples), target, n_samples // hop)[0]`` as a differentiable function of ``wav`` ((B, N) or the
    generator's (B, 1, N)): the same value ("mean" 0-dim fp32; "sum" 0-dim fp64), and ``.backward()`` hands on the gradient the
    device computed with the loss -- deterministic, so it also runs under ``torch.use_deterministic_algorithms(True)``.
    ``target`` gets no gradient.  No double backward."""
    if reduction not in ("mean", "sum"):
        raise ValueError(f"mel_l1_trainable: reduction must be 'mean' or 'sum', got {reduction!r}")
    if isinstance(target, torch.Tensor) and target.requires_grad:
        target = target.detach()
    return _MelL1Fn.apply(wav, mel, target, n_samples, reduction)


class MelL1Loss(nn.Module):
    """The mel term of the generator loss for the reference trainer: utils/vocoder/train.py:151-157,
    ``F.l1_loss(y_mel, mel_spectrogram(y_g_hat.squeeze(1), ..., h.fmax_for_loss)) * 45``, becomes ``MelL1Loss(h)(y_g_hat, y_mel) * 45``.
    ``forward(y_g_hat (B, 1, N) or (B, N), y_mel (B, num_mels, N // hop_size), n_samples=None)``; ``h`` and the keywords as
    ``MelSpectrogram``'s."""

    def __init__(self, h=None, reduction: str = "mean", **kw) -> None:
        super().__init__()
        if reduction not in ("mean", "sum"):
            raise ValueError(f"MelL1Loss: reduction must be 'mean' or 'sum', got {reduction!r}")
        self.mel, self.reduction = MelSpectrogram(h, **kw), reduction

    def forward(self, y_g_hat: torch.Tensor, y_mel: torch.Tensor, n_samples=None) -> torch.Tensor:
        return mel_l1_trainable(self.mel, y_g_hat, y_mel, n_samples, self.reduction)
