"""The forced aligner on the GPU: ``Aligner`` of reference utils/aligner/model.py:24-64, the softmax of
utils/aligner/extract_durations.py:86-96 and ``extract_durations_with_dijkstra`` of utils/aligner/duration_extraction.py:52-85,
and the CTC loss of utils/aligner/trainer.py:60-71 with its gradient, backed by libparrot_hip.so (``parrot_aligner_forward`` /
``parrot_align_softmax`` / ``parrot_align_durations`` / ``parrot_ctc_loss`` / ``parrot_ctc_loss_grad``).

    Aligner(n_mels, num_symbols, lstm_dim, conv_dim)           the reference's constructor and state_dict keys
    Aligner.from_checkpoint(checkpoint), .get_step()             as the reference
    .forward(mel) -> logits (B, T, num_symbols)                 the padded batch as it stands
    .predict(mel, mel_len) -> pred                              softmax over the real frames, zero beyond
    .align(mel, mel_len, tokens, tokens_len) -> (durations (B, N) int32, cost (B) fp64, pred)
    .ctc_loss(mel, mel_len, tokens, tokens_len) -> loss          the reference trainer's CTC loss of the batch, forward only
    ctc_loss(logits, tokens, mel_len, tokens_len) -> loss        the same on given logits
    ctc_loss_and_grad(logits, tokens, mel_len, tokens_len) -> (loss, grad)   the loss and d loss / d logits in one call
    ctc_loss_trainable(logits, tokens, mel_len, tokens_len) -> loss           the loss as an autograd node (logits only)
    CTCLoss(blank=0, reduction="mean", zero_infinity=False)      torch.nn.CTCLoss's call shape over ctc_loss_trainable
    extract_durations_with_dijkstra(tokens, pred) -> durations   numpy in, numpy out, the reference's signature
    TrainableAligner(n_mels, num_symbols, lstm_dim, conv_dim)    the same network for TRAINING: batch-statistics forward and the full
                                                                 backward (aligner_train.py); ``Aligner`` itself is inference only

Padding is NOT masked before the softmax, as in the reference: the backward LSTM of a short row starts inside the padding, so a
row's logits depend on the length its batch is padded to.  Durations are those of the cheapest monotonic path; among equally cheap
paths (doubled letters, saturated probabilities) the rule is diagonal, then previous frame, then previous token -- the reference's
own choice there follows no fixed rule.  There is no CPU path: a CPU tensor raises, as in the other shims."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Tuple

import numpy as np
import torch
from torch import nn

from . import _lib
from ._handle import PackedHandleModule, _attach
from ._lib import ST_NONFINITE
from .ops import _prec_arg, _workspace, dptr, param_fingerprint, require_cuda, stream_ptr

MAX_FRAMES, MAX_TOKENS = 32768, 2048  # csrc/aligner.h: ALIGN_MAX_T, ALIGN_MAX_N
ST_BAD_INPUT = 9
BN_EPS = 1e-5


def aligner_param_shapes(n_mels: int, num_symbols: int, lstm_dim: int, conv_dim: int) -> Dict[str, tuple]:
    """state_dict key -> shape of the reference ``Aligner`` (parameters and BatchNorm buffers; ``step`` and the three
    ``num_batches_tracked`` counters are scalars registered beside them)."""
    sh = {}
    for i in range(3):
        sh[f"convs.{i}.conv.weight"] = (conv_dim, n_mels if i == 0 else conv_dim, 5)
        for k in ("weight", "bias", "running_mean", "running_var"):
            sh[f"convs.{i}.bnorm.{k}"] = (conv_dim,)
    for sfx in ("", "_reverse"):
        sh["rnn.weight_ih_l0" + sfx] = (4 * lstm_dim, conv_dim)
        sh["rnn.weight_hh_l0" + sfx] = (4 * lstm_dim, lstm_dim)
        sh["rnn.bias_ih_l0" + sfx] = (4 * lstm_dim,)
        sh["rnn.bias_hh_l0" + sfx] = (4 * lstm_dim,)
    sh["lin.weight"] = (num_symbols, 2 * lstm_dim)
    sh["lin.bias"] = (num_symbols,)
    return sh


class Aligner(PackedHandleModule):
    """Inference-only counterpart of the reference's ``Aligner``: the same constructor, ``state_dict`` keys (``step`` and the
    BatchNorm buffers included), ``from_checkpoint`` and ``get_step``; ``forward`` runs on the HIP kernels.  BatchNorm uses its
    running statistics (the reference's ``.eval()``); ``step`` increments on every forward, as the reference's does in eval too
    (``if self.train:`` tests a bound method)."""

    _destroy_fn, _precision_fn = "parrot_aligner_destroy", "parrot_aligner_precision"

    def __init__(self, n_mels: int, num_symbols: int, lstm_dim: int, conv_dim: int, precision=None) -> None:
        super().__init__()
        self.n_mels, self.num_symbols, self.lstm_dim, self.conv_dim = int(n_mels), int(num_symbols), int(lstm_dim), int(conv_dim)
        self.precision = _prec_arg(precision)
        self.register_buffer("step", torch.tensor(1, dtype=torch.int))
        gen = torch.Generator().manual_seed(0)
        for key, shape in aligner_param_shapes(self.n_mels, self.num_symbols, self.lstm_dim, self.conv_dim).items():
            leaf = key.rsplit(".", 1)[1]
            if leaf in ("running_mean", "running_var"):
                _attach(self, key, torch.zeros(shape) if leaf == "running_mean" else torch.ones(shape), buffer=True)
                continue
            if ".bnorm." in key:
                t = torch.ones(shape) if leaf == "weight" else torch.zeros(shape)
            elif len(shape) == 1:
                t = torch.zeros(shape)
            else:
                fan_in = int(np.prod(shape[1:]))
                t = torch.randn(shape, generator=gen) / max(fan_in, 1) ** 0.5
            _attach(self, key, t, buffer=False)
        for i in range(3):
            _attach(self, f"convs.{i}.bnorm.num_batches_tracked", torch.tensor(0, dtype=torch.long), buffer=True)
        self._taps = None

    # ---- the reference's surface ---------------------------------------------------------------
    def get_step(self):
        return self.step.data.item()

    @classmethod
    def from_checkpoint(cls, checkpoint: dict) -> "Aligner":
        config = checkpoint["config"]
        symbols = checkpoint["symbols"]
        model = cls(n_mels=config["audio"]["n_mels"], num_symbols=len(symbols) + 1, **config["model"])
        model.load_state_dict(checkpoint["model"])
        return model

    # ---- HIP handle (lifecycle: _handle.py) -----------------------------------------------------
    def _weight_fingerprint(self):
        step, self._buffers["step"] = self._buffers["step"], None  # (step changes on every forward and is no weight)
        try:
            return param_fingerprint(self)
        finally:
            self._buffers["step"] = step

    def _build(self, device):
        sd = {k: v.detach().to("cpu", torch.float32).contiguous() for k, v in self.state_dict().items() if v.dim() > 0}
        P = lambda k: _lib.fptr(sd[k])  # noqa: E731
        cfg = _lib.AlignerCfg(self.n_mels, self.num_symbols, self.lstm_dim, self.conv_dim, BN_EPS)
        w = _lib.AlignerWeights()
        for i in range(3):
            w.conv_w[i] = P(f"convs.{i}.conv.weight")
            w.bn_weight[i], w.bn_bias[i] = P(f"convs.{i}.bnorm.weight"), P(f"convs.{i}.bnorm.bias")
            w.bn_mean[i], w.bn_var[i] = P(f"convs.{i}.bnorm.running_mean"), P(f"convs.{i}.bnorm.running_var")
        for d, sfx in enumerate(("", "_reverse")):
            w.w_ih[d], w.w_hh[d] = P("rnn.weight_ih_l0" + sfx), P("rnn.weight_hh_l0" + sfx)
            w.b_ih[d], w.b_hh[d] = P("rnn.bias_ih_l0" + sfx), P("rnn.bias_hh_l0" + sfx)
        w.lin_w, w.lin_b = P("lin.weight"), P("lin.bias")
        hdl = C.c_void_p()
        with torch.cuda.device(device):
            _lib.check(_lib.lib().parrot_aligner_create_ex(C.byref(hdl), C.byref(cfg), C.byref(w), self.precision))
        self._handle, self._handle_device = hdl, device

    # ---- compute -------------------------------------------------------------------------------
    def _check_mel(self, mel: torch.Tensor) -> torch.Tensor:
        require_cuda(mel, "mel")
        if mel.dim() != 3 or mel.shape[2] != self.n_mels:
            raise ValueError(f"Aligner: expected mel (B, T, {self.n_mels}), got {tuple(mel.shape)}")
        if mel.shape[0] < 1 or mel.shape[1] < 1:
            raise ValueError("Aligner: empty batch or sequence")
        return mel.to(torch.float32).contiguous()

    @torch.no_grad()
    def forward(self, mel: torch.Tensor, stages: bool = False):
        """mel (B, T, n_mels) on the GPU -> logits (B, T, num_symbols).  ``stages=True`` (tests): also the activation after the
        third BatchNorm, (B, T, conv_dim) as the reference holds it, and the LSTM output (B, T, 2 lstm_dim)."""
        mel = self._check_mel(mel)
        dev = mel.device
        B, T = int(mel.shape[0]), int(mel.shape[1])
        lib = _lib.lib()
        logits = torch.empty((B, T, self.num_symbols), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            h = self._current_handle(dev)
            bn3 = lstm = None
            if stages:
                bn3 = torch.empty((B, self.conv_dim, T), dtype=torch.float32, device=dev)
                lstm = torch.empty((B, T, 2 * self.lstm_dim), dtype=torch.float32, device=dev)
            _lib.check(lib.parrot_aligner_debug_stages(h, dptr(bn3), dptr(lstm)))
            n_ws = int(lib.parrot_aligner_workspace_bytes(h, B, T))
            ws = _workspace(n_ws, dev)
            try:
                _lib.check(lib.parrot_aligner_forward(h, dptr(mel), B, T, dptr(logits), dptr(ws), n_ws, stream_ptr(dev)))
            finally:
                if stages:
                    lib.parrot_aligner_debug_stages(h, None, None)
        self.step += 1
        if stages:
            return logits, {"bn3": bn3.transpose(1, 2).contiguous(), "lstm": lstm}
        return logits

    @staticmethod
    def _lengths(x, B: int, hi: int, name: str, dev) -> torch.Tensor:
        t = torch.as_tensor(x)
        if tuple(t.shape) != (B,):
            raise ValueError(f"{name} must hold one length per row ({B}), got {tuple(t.shape)}")
        if not t.is_cuda and (int(t.min()) < 1 or int(t.max()) > hi):  # (a device tensor is not read back: the kernels set status 9)
            raise ValueError(f"{name} must lie in [1, {hi}], got {t.tolist()}")
        return t.to(dev, torch.int32).contiguous()

    @torch.no_grad()
    def softmax(self, logits: torch.Tensor, mel_len, check: bool = True) -> torch.Tensor:
        require_cuda(logits, "logits")
        logits = logits.to(torch.float32).contiguous()
        dev = logits.device
        B, T, V = logits.shape
        if V != self.num_symbols:
            raise ValueError(f"Aligner.softmax: expected {self.num_symbols} symbols, got {V}")
        ml = self._lengths(mel_len, B, T, "mel_len", dev)
        pred = torch.empty_like(logits)
        with torch.cuda.device(dev):
            h = self._current_handle(dev)
            _lib.check(_lib.lib().parrot_align_softmax(h, dptr(logits), dptr(ml), B, T, dptr(pred), stream_ptr(dev)))
            if check:
                try:
                    _lib.check(_lib.lib().parrot_aligner_check(h, stream_ptr(dev)))
                except _lib.ParrotHipError as e:
                    if e.code != -1:
                        raise
                    raise ValueError(f"mel_len must lie in [1, {T}] (device status {ST_BAD_INPUT})") from e
        return pred

    def predict(self, mel: torch.Tensor, mel_len, check: bool = True) -> torch.Tensor:
        """pred (B, T, num_symbols): ``torch.softmax(logits[b, :mel_len[b]], -1)`` per row, zero at and beyond ``mel_len[b]``.
        Raises when a logit of a real frame is not finite."""
        return self.softmax(self.forward(mel), mel_len, check=check)

    @staticmethod
    def durations(pred: torch.Tensor, tokens: torch.Tensor, mel_len, tokens_len) -> torch.Tensor:
        """Durations (B, N) int32 of ``align_durations`` (the dynamic programme alone, on given probabilities)."""
        return align_durations(pred, tokens, mel_len, tokens_len)[0]

    def align(self, mel: torch.Tensor, mel_len, tokens: torch.Tensor, tokens_len) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """-> (durations (B, N) int32, cost (B) fp64, pred (B, T, num_symbols)), all on the GPU: row b's durations sum to
        ``mel_len[b]`` and are zero beyond ``tokens_len[b]``."""
        pred = self.predict(mel, mel_len)
        dur, cost = align_durations(pred, tokens, mel_len, tokens_len)
        return dur, cost, pred

    def ctc_loss(self, mel: torch.Tensor, mel_len, tokens: torch.Tensor, tokens_len, reduction: str = "mean") -> torch.Tensor:
        """The reference trainer's loss of this batch (trainer.py:60-63): ``forward`` on the padded batch as it stands, not
        masked, then ``ctc_loss`` of the logits."""
        return ctc_loss(self.forward(mel), tokens, mel_len, tokens_len, reduction=reduction)


def _ragged_args(who: str, x: torch.Tensor, name: str, tokens, mel_len, tokens_len):
    """What ``align_durations`` and ``ctc_loss`` share: x (B, T, V) fp32 on the GPU, tokens (B, N) int64, the lengths (B) int32."""
    require_cuda(x, name)
    if x.dim() != 3:
        raise ValueError(f"{who}: expected {name} (B, T, V), got {tuple(x.shape)}")
    dev = x.device
    x = x.to(torch.float32).contiguous()
    B, T = int(x.shape[0]), int(x.shape[1])
    tokens = torch.as_tensor(tokens)
    if tokens.dim() != 2 or tokens.shape[0] != B:
        raise ValueError(f"{who}: expected tokens ({B}, N), got {tuple(tokens.shape)}")
    tokens = tokens.to(dev, torch.int64).contiguous()
    ml = Aligner._lengths(mel_len, B, T, "mel_len", dev)
    tl = Aligner._lengths(tokens_len, B, int(tokens.shape[1]), "tokens_len", dev)
    return x, tokens, ml, tl


def _call_with_status(who: str, ws_bytes_fn, ws_args: tuple, fn, args: tuple, dev, V: int, what: str) -> None:
    """What the three calls without a handle share: a workspace whose first word is the device status, the call on the current
    stream, one read-back of that word (the synchronisation of the call) and ``_raise_status``.  ``args``: everything before
    (ws, ws_bytes, stream)."""
    with torch.cuda.device(dev):
        n_ws = int(ws_bytes_fn(*ws_args))
        ws = _workspace(n_ws, dev, at_least=4)
        _lib.check(fn(*args, dptr(ws), n_ws, stream_ptr(dev)))
        status = int(ws[:4].view(torch.int32).item())
    _raise_status(who, status, V, what)


def _raise_status(who: str, status: int, V: int, what: str) -> None:
    if status == ST_BAD_INPUT:
        raise ValueError(f"{who}: a token outside [0, {V}) or a length outside [1, T] / [1, N] (device status {status})")
    if status == ST_NONFINITE:
        raise FloatingPointError(f"{who}: a NaN / inf {what} (device status {status})")
    if status:
        raise RuntimeError(f"{who}: device status {status}")


@torch.no_grad()
def align_durations(pred: torch.Tensor, tokens: torch.Tensor, mel_len, tokens_len) -> Tuple[torch.Tensor, torch.Tensor]:
    """The shortest-path dynamic programme for a ragged batch: pred (B, T, V) fp32 PROBABILITIES on the GPU, tokens (B, N)
    integer, mel_len / tokens_len (B) -> (durations (B, N) int32, cost (B) fp64).  Raises ValueError for a token outside [0, V)
    or a length outside its range, FloatingPointError for a NaN / inf probability of a real frame (durations are not returned),
    ParrotHipError beyond 32768 frames / 2048 tokens."""
    pred, tokens, ml, tl = _ragged_args("align_durations", pred, "pred", tokens, mel_len, tokens_len)
    dev = pred.device
    (B, T, V), N = (int(v) for v in pred.shape), int(tokens.shape[1])
    lib = _lib.lib()
    dur = torch.empty((B, N), dtype=torch.int32, device=dev)
    cost = torch.empty((B,), dtype=torch.float64, device=dev)
    _call_with_status("align_durations", lib.parrot_align_workspace_bytes, (B, T, N), lib.parrot_align_durations,
                      (dptr(pred), dptr(tokens), dptr(ml), dptr(tl), B, T, V, N, dptr(dur), dptr(cost)), dev, V, "probability in pred")
    return dur, cost


@torch.no_grad()
def ctc_loss(logits: torch.Tensor, tokens: torch.Tensor, mel_len, tokens_len, reduction: str = "mean") -> torch.Tensor:
    """``CTCLoss()(logits.transpose(0, 1).log_softmax(2), tokens, mel_len, tokens_len)`` of utils/aligner/trainer.py:60-63 (blank
    0, no zero_infinity) for a ragged batch, forward only: logits (B, T, V) fp32 LOGITS on the GPU, tokens (B, N) integer, mel_len
    / tokens_len (B).  The log-sum-exp over V is fp32, the recursion fp64.  ``reduction``: "mean" -> 0-dim fp32,
    mean_b(nll[b] / tokens_len[b]) as torch's; "none" -> nll (B) fp64; "sum" -> 0-dim fp64.  A row that has no path (mel_len <
    tokens_len + repeated neighbours) is +inf.  Raises ValueError for a token outside [0, V) or a length outside its range,
    FloatingPointError for a NaN / inf logit of a real frame, ParrotHipError beyond 32768 frames / 2048 tokens."""
    if reduction not in ("mean", "none", "sum"):
        raise ValueError(f"ctc_loss: reduction must be 'mean', 'none' or 'sum', got {reduction!r}")
    logits, tokens, ml, tl = _ragged_args("ctc_loss", logits, "logits", tokens, mel_len, tokens_len)
    dev = logits.device
    (B, T, V), N = (int(v) for v in logits.shape), int(tokens.shape[1])
    lib = _lib.lib()
    nll = torch.empty((B,), dtype=torch.float64, device=dev)
    mean = torch.empty((), dtype=torch.float32, device=dev)
    _call_with_status("ctc_loss", lib.parrot_ctc_workspace_bytes, (B, T, N), lib.parrot_ctc_loss,
                      (dptr(logits), dptr(tokens), dptr(ml), dptr(tl), B, T, V, N, dptr(nll), dptr(mean)), dev, V, "logit in a real frame")
    if reduction == "mean":
        return mean
    return nll if reduction == "none" else nll.sum()


def ctc_reduction_weights(tokens_len: torch.Tensor, reduction: str) -> torch.Tensor:
    """d loss / d nll[b] of torch's reductions, (B) fp64 on ``tokens_len``'s device: 1 for "none" and "sum"; 1 / (max(N_b, 1) B) for
    "mean", formed as torch's autograd forms it, (1 / B) / max(N_b, 1)."""
    if reduction not in ("mean", "none", "sum"):
        raise ValueError(f"ctc_loss: reduction must be 'mean', 'none' or 'sum', got {reduction!r}")
    B = int(tokens_len.shape[0])
    w = torch.ones((B,), dtype=torch.float64, device=tokens_len.device)
    if reduction == "mean":
        w = w / B / tokens_len.clamp_min(1).to(torch.float64)
    return w


def _reduce_nll(nll: torch.Tensor, tl: torch.Tensor, reduction: str, zero_infinity: bool) -> torch.Tensor:
    """``ctc_loss``'s three results from nll (B) fp64, bit for bit: "mean" is the fp64 sum of nll / tokens_len in row order, over B,
    rounded to fp32 once (csrc/ctc.h ctc_mean_kernel; the running sum is formed on the host, the call has just read the status back
    anyway).  ``zero_infinity``: a row without a path counts 0."""
    if zero_infinity:
        nll = torch.where(torch.isinf(nll), torch.zeros_like(nll), nll)
    if reduction == "none":
        return nll
    if reduction == "sum":
        return nll.sum()
    with np.errstate(invalid="ignore"):
        terms = nll.cpu().numpy() / tl.cpu().numpy().astype(np.float64)
        mean = np.float32(np.cumsum(terms)[-1] / np.float64(terms.shape[0]))  # (cumsum: strictly in row order)
    return torch.tensor(mean, dtype=torch.float32, device=nll.device)


def _ctc_grad_call(logits, tokens, ml, tl, row_weight, zero_infinity: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """parrot_ctc_loss_grad on validated arguments -> (nll (B) fp64, grad (B, T, V) fp32); raises as ``ctc_loss``."""
    dev = logits.device
    (B, T, V), N = (int(v) for v in logits.shape), int(tokens.shape[1])
    lib = _lib.lib()
    nll = torch.empty((B,), dtype=torch.float64, device=dev)
    grad = torch.empty((B, T, V), dtype=torch.float32, device=dev)
    row_weight = row_weight.to(dev, torch.float64).contiguous()
    _call_with_status("ctc_loss_and_grad", lib.parrot_ctc_grad_workspace_bytes, (B, T, V, N), lib.parrot_ctc_loss_grad,
                      (dptr(logits), dptr(tokens), dptr(ml), dptr(tl), B, T, V, N, dptr(row_weight), int(bool(zero_infinity)), dptr(nll),
                       dptr(grad)), dev, V, "logit in a real frame")
    return nll, grad


@torch.no_grad()
def ctc_loss_and_grad(logits: torch.Tensor, tokens: torch.Tensor, mel_len, tokens_len, reduction: str = "mean",
                      zero_infinity: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """``ctc_loss`` and its gradient with respect to the logits in one call (trainer.py:60-71: the loss and ``loss.backward()``):
    -> (loss, grad (B, T, V) fp32).  ``loss`` is ``ctc_loss(..., reduction)``, bit for bit; ``grad[b] = w_b d nll[b] / d logits[b]``
    with w_b = 1 for "none" / "sum" and 1 / (max(N_b, 1) B) for "mean" (torch's rule), exactly 0 at and beyond ``mel_len[b]``.  The
    recursions are fp64 and nothing is accumulated atomically: two calls agree bit for bit and a row's gradient does not depend on
    the rows beside it.  A row without a path: loss +inf and NaN on its real frames, as torch's; with ``zero_infinity`` it counts
    0 and its gradient is 0.  Unlike torch's CPU backward this is the true gradient also for a row whose last token is the
    blank (0).  Raises as ``ctc_loss``."""
    if reduction not in ("mean", "none", "sum"):
        raise ValueError(f"ctc_loss_and_grad: reduction must be 'mean', 'none' or 'sum', got {reduction!r}")
    logits, tokens, ml, tl = _ragged_args("ctc_loss_and_grad", logits, "logits", tokens, mel_len, tokens_len)
    nll, grad = _ctc_grad_call(logits, tokens, ml, tl, ctc_reduction_weights(tl, reduction), zero_infinity)
    return _reduce_nll(nll, tl, reduction, zero_infinity), grad


class _CtcLossFn(torch.autograd.Function):
    """The forward is ``ctc_loss``; the backward is one parrot_ctc_loss_grad call with row_weight = grad_output x the reduction's
    weight.  Only the logits get a gradient, and there is no double backward."""

    @staticmethod
    def forward(ctx, logits, tokens, mel_len, tokens_len, reduction, zero_infinity):
        x, tokens, ml, tl = _ragged_args("ctc_loss_trainable", logits, "logits", tokens, mel_len, tokens_len)
        ctx.save_for_backward(x, tokens, ml, tl)
        ctx.reduction, ctx.zero_infinity, ctx.in_dtype = reduction, bool(zero_infinity), logits.dtype
        if not zero_infinity:
            return ctc_loss(x, tokens, ml, tl, reduction=reduction)
        return _reduce_nll(ctc_loss(x, tokens, ml, tl, reduction="none"), tl, reduction, True)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        x, tokens, ml, tl = ctx.saved_tensors
        w = ctc_reduction_weights(tl, ctx.reduction) * grad_output.detach().to(x.device, torch.float64)  # (a 0-dim grad_output broadcasts)
        _, grad = _ctc_grad_call(x, tokens, ml, tl, w, ctx.zero_infinity)
        return grad.to(ctx.in_dtype), None, None, None, None, None


def ctc_loss_trainable(logits: torch.Tensor, tokens: torch.Tensor, mel_len, tokens_len, reduction: str = "mean",
                       zero_infinity: bool = False) -> torch.Tensor:
    """``ctc_loss`` as a differentiable function of the logits: same values and dtypes ("mean" 0-dim fp32, "none" (B) fp64, "sum"
    0-dim fp64), and ``.backward()`` runs ``parrot_ctc_loss_grad`` -- deterministic, so it also runs under
    ``torch.use_deterministic_algorithms(True)``, where torch's own device backward raises.  For ``TrainableAligner`` or a torch-built
    model: the inference ``Aligner.forward`` has no backward.  No double backward."""
    if reduction not in ("mean", "none", "sum"):
        raise ValueError(f"ctc_loss_trainable: reduction must be 'mean', 'none' or 'sum', got {reduction!r}")
    return _CtcLossFn.apply(logits, tokens, mel_len, tokens_len, reduction, zero_infinity)


class CTCLoss(nn.Module):
    """``torch.nn.CTCLoss`` for the reference trainer (trainer.py:21 becomes ``from parrot_tts_amd.aligner import CTCLoss``):
    ``forward(log_probs (T, B, V), targets (B, N), input_lengths (B), target_lengths (B))``.  The input is transposed to (B, T, V)
    and taken as LOGITS: normalising log-probabilities again changes them by the fp32 log-sum-exp's rounding only, and the gradient
    returned for ``log_probs`` is the one torch returns (softmax minus occupancy).  Result dtypes follow ``ctc_loss``, not torch:
    "mean" is fp32, "none" and "sum" are fp64.  Only ``blank=0``, padded 2-D targets and batched input exist here; anything else
    raises and is never approximated."""

    def __init__(self, blank: int = 0, reduction: str = "mean", zero_infinity: bool = False) -> None:
        super().__init__()
        if blank != 0:
            raise ValueError(f"CTCLoss: only blank=0 is implemented, got {blank}")
        if reduction not in ("mean", "none", "sum"):
            raise ValueError(f"CTCLoss: reduction must be 'mean', 'none' or 'sum', got {reduction!r}")
        self.blank, self.reduction, self.zero_infinity = 0, reduction, bool(zero_infinity)

    def forward(self, log_probs: torch.Tensor, targets: torch.Tensor, input_lengths, target_lengths) -> torch.Tensor:
        if log_probs.dim() != 3:
            raise NotImplementedError(f"CTCLoss: expected batched log_probs (T, B, V), got {tuple(log_probs.shape)}")
        if torch.as_tensor(targets).dim() != 2:
            raise NotImplementedError("CTCLoss: expected padded targets (B, N); 1-D concatenated targets are not implemented")
        return ctc_loss_trainable(log_probs.transpose(0, 1), targets, input_lengths, target_lengths, self.reduction, self.zero_infinity)


def extract_durations_with_dijkstra(tokens: np.ndarray, pred: np.ndarray) -> np.ndarray:
    """Drop-in for reference utils/aligner/duration_extraction.py:52-85: tokens (N,) integer, pred (T, V) probabilities, numpy in,
    -> durations (N,) int32, numpy out; computed on the current GPU."""
    tokens = np.asarray(tokens)
    pred = np.asarray(pred)
    if tokens.ndim != 1 or pred.ndim != 2 or tokens.size == 0 or pred.shape[0] == 0:
        raise ValueError(f"extract_durations_with_dijkstra: expected tokens (N,) and pred (T, V), got {tokens.shape} and {pred.shape}")
    dev = torch.device("cuda", torch.cuda.current_device())
    p = torch.from_numpy(np.ascontiguousarray(pred, dtype=np.float32)).to(dev)[None]
    t = torch.from_numpy(np.ascontiguousarray(tokens, dtype=np.int64))[None]
    dur, _ = align_durations(p, t, [pred.shape[0]], [tokens.shape[0]])
    return dur[0].cpu().numpy().astype(np.int32)


from .aligner_train import TrainableAligner  # noqa: E402,F401  (training: the batch-statistics forward and the full backward)
