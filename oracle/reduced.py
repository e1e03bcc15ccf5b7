"""CPU emulation of the reduced-precision conv modes ``PARROT_PREC_BF16`` / ``PARROT_PREC_F16``.

TEST INFRASTRUCTURE ONLY, like the rest of ``oracle/``.

The contract of these modes (``include/parrot_hip.h``, the ``PARROT_PREC_*`` block): operands rounded ONCE to bf16 / fp16,
one MFMA per product group, fp32 accumulation, fp32 outputs and residual stream.  In detail:

  * bf16: round-to-nearest-even of the fp32 value (``pk_bf16``, ``csrc/conv_split.h``; host weights ``bf16_rn_host``,
    ``csrc/weight_pack.h``);
  * fp16: round-to-nearest-even after a power-of-two scale -- activations by ``XS = 8`` (``SchF16::XS``), the weights of a
    layer by ``f16_weight_scale`` (max|w| * scale in [2^14, 2^15)); overflow gives inf (``pk_f16`` / ``f16_rn_host``);
  * the layer's leaky ReLU is applied BEFORE the rounding (``pre_scale``, ``csrc/conv_split.h``), bias and residual are
    not rounded.

A product of two bf16 (or two fp16) values is exact in fp32, so a conv of the rounded operands evaluated in float32 has the
same error class as the MFMA path and the same evaluation in float64 is its exact value: the pair measures how much a
kernel may differ from the emulation by accumulation order alone.

Which layers the library evaluates in reduced precision at all is ``reduced_layer`` (derived from ``conv_build`` and the
vocoder's kernel selection); every other layer runs on an exact fp32 kernel in these modes too.
"""
from __future__ import annotations

import contextlib
import math
from typing import Optional

import torch
import torch.nn.functional as _TF

from oracle import parrot_oracle as O

MODES = ("bf16", "f16")
F16_XS = 8.0          # SchF16::XS (csrc/conv_split.h): activation scale in front of the fp16 rounding
RBS_MAX_CONVS = 8     # csrc/resblock_split.h: convs of one ResBlock the pair kernels take


# ----------------------------------------------------------------------------------------------------------------------
# rounding (computed in float64 from the exponent, independent of torch's casts -- the CPU tests compare the two)
# ----------------------------------------------------------------------------------------------------------------------
def _round_rne(t: torch.Tensor, mant_bits: int, min_exp: int, max_exp: int) -> torch.Tensor:
    """Round to the nearest value with `mant_bits` stored significand bits (ties to even), exponents clamped below at
    `min_exp` (gradual underflow) and overflowing to inf at 2^(max_exp + 1).  Returns float32."""
    x = t.detach().to(torch.float64)
    finite = torch.isfinite(x) & (x != 0)
    _, e = torch.frexp(torch.where(finite, x, torch.ones_like(x)))  # |x| = m 2^e, m in [0.5, 1)
    e = torch.clamp(e.to(torch.float64) - 1, min=min_exp)           # floor(log2 |x|), no lower than the smallest normal
    q = torch.exp2(e - mant_bits)                                    # spacing of representable values at that exponent
    r = torch.round(x / q) * q                                       # torch.round: half to even; x / q is exact
    r = torch.where(r.abs() >= 2.0 ** (max_exp + 1), torch.copysign(torch.full_like(r, math.inf), r), r)
    return torch.where(finite, r, x).to(torch.float32)               # 0, +-0, inf, nan pass through


def round_bf16(t: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 -> fp32, round-to-nearest-even (``pk_bf16``: v_cvt_pk_bf16_f32; host: ``bf16_rn_host``)."""
    return _round_rne(t, 7, -126, 127)


def round_f16(t: torch.Tensor, scale: float) -> torch.Tensor:
    """(t * scale) -> fp16 -> fp32, then / scale: round-to-nearest-even, overflow -> inf (``pk_f16``: v_cvt_pk_f16_f32;
    host: ``f16_rn_host``).  `scale` is a power of two, so the scaling itself is exact."""
    assert scale > 0 and math.frexp(scale)[0] == 0.5, "the fp16 scales are powers of two"
    x = t.detach().to(torch.float32).to(torch.float64) * scale
    return (_round_rne(x, 10, -14, 15).to(torch.float64) / scale).to(torch.float32)


def round_rtz(t: torch.Tensor, mode: str, scale: float = 1.0) -> torch.Tensor:
    """The same roundings toward zero (truncation): NOT what the library does -- the tests use it to show that they can
    tell the rounding mode apart."""
    x = t.detach().to(torch.float64) * scale
    mant, lo, hi = (7, -126, 127) if mode == "bf16" else (10, -14, 15)
    finite = torch.isfinite(x) & (x != 0)
    _, e = torch.frexp(torch.where(finite, x, torch.ones_like(x)))
    q = torch.exp2(torch.clamp(e.to(torch.float64) - 1, min=lo) - mant)
    r = torch.trunc(x / q) * q
    r = torch.where(r.abs() >= 2.0 ** (hi + 1), torch.copysign(torch.full_like(r, math.inf), r), r)
    return (torch.where(finite, r, x) / scale).to(torch.float32)


def f16_weight_scale(w: torch.Tensor) -> float:
    """``f16_weight_scale`` of csrc/weight_pack.h, line for line: the power of two that puts max|w| into [2^14, 2^15);
    1 for an all-zero or non-finite maximum."""
    mx = float(w.detach().to(torch.float32).abs().max()) if w.numel() else 0.0  # for (...) mx = max(mx, fabs(w[i]))
    if not (mx > 0.0) or not math.isfinite(mx):                                   # if (!(mx > 0.f) || !isfinite(mx)) return 1.f
        return 1.0
    _, e = math.frexp(mx)                                                          # frexp(mx, &e): mx = m 2^e, m in [0.5, 1)
    return math.ldexp(1.0, 15 - e)                                                 # ldexp(1.f, 15 - e)


def round_operand(t: torch.Tensor, mode: str, scale: float = 1.0, rtz: bool = False) -> torch.Tensor:
    """An activation (scale = F16_XS) or weight (scale = f16_weight_scale) operand of a reduced layer in `mode`."""
    if mode not in MODES:
        raise ValueError(f"unknown reduced mode {mode!r}")
    if rtz:
        return round_rtz(t, mode, scale if mode == "f16" else 1.0)
    return round_bf16(t) if mode == "bf16" else round_f16(t, scale)


# ----------------------------------------------------------------------------------------------------------------------
# which layers are reduced
# ----------------------------------------------------------------------------------------------------------------------
def resblock_split_has(c: int, k: int) -> bool:
    """csrc/resblock_split.h ``resblock_split_has``: channel counts / tap counts the fused ResBlock1 pair kernels take."""
    if c in (256, 128):
        return k == 3
    if c == 64:
        return k in (3, 7)
    return c in (32, 16) and k in (3, 7, 11)


def reduced_layer(kind: str, c_in: int, c_out: int, k: int, stride: int = 1, *, dilation: int = 1, padding: int = 0,
                  groups: int = 1, pre_slope: Optional[float] = None, act: str = "none", tile_cfg: int = -1,
                  fused: int = 2, resblock_type: int = 1, n_dil: int = 3, valu_kernels: bool = True) -> bool:
    """Is this layer evaluated on the single-piece (reduced) scheme when the library runs in PARROT_PREC_BF16 / _F16?

    kind: "conv" (a plain Conv1d: ``ConvPlan``, conv_pre, conv_post, TTE layers), "convt" (ConvTranspose1d, `stride` = u),
    "rb" (a conv of a vocoder ResBlock of `c_in` = `c_out` channels; `fused` = the handle's PARROT_FUSED mode).
    pre_slope: the leaky-ReLU slope applied to the input (None: no pre-activation); act: "none" | "relu" | "tanh".
    (The vocoder's layer-by-layer fallback for rows of 2 GiB and more is not modelled: no test shape comes near it.)"""
    if kind not in ("conv", "convt", "rb"):
        raise ValueError(f"unknown layer kind {kind!r}")
    transposed = kind == "convt"
    # host_voc_mrf.hip mrf_create: a ResBlock1 whose (channels, k) the pair kernels take gets a concatenated weight stream
    # (`rb_stream`, needs a split scheme), and voc_forward runs it on resblock_split_launch whenever `v->fused != 0` -- also
    # at 16 channels, where the layer plans themselves are exact (rows < 32, below)
    if kind == "rb" and fused != 0 and resblock_type == 1 and resblock_split_has(c_out, k) and 2 * n_dil <= RBS_MAX_CONVS:
        return True
    # conv_build: `slope_ok` -- the split kernels evaluate the leaky ReLU as max(v, slope v)
    slope_ok = pre_slope is None or 0.0 <= pre_slope <= 1.0
    # conv_build: M = C_out u for the polyphase transposed conv, Mg = M / groups; the split plan iff
    # `want_prec >= 1 && c->Mg >= 32 && d->tile_cfg < 0 && c->Cin % 16 == 0 && slope_ok`
    m = c_out * stride if transposed else c_out
    if not (m // groups >= 32 and tile_cfg < 0 and (c_in // groups) % 16 == 0 and slope_ok):
        return False
    # conv_build, the VALU kernels of conv_valu.h (fp32 FMA in every mode; they replace the plan at launch):
    # `d->tile_cfg < 0 && groups == 1 && slope01 && d->dilation == 1 && valu_kernels_enabled()`, then
    #   c_out == 1, (k 7, pad 3) or (k 1, pad 0), act none / tanh   -> conv1_valu_kernel / linear1_valu_kernel  (never split: Mg = 1)
    #   transposed, c_out 16, k 4, stride 2, pad 1, act none        -> convt_valu_kernel<16, 4, 2, 1>
    if valu_kernels and tile_cfg < 0 and groups == 1 and slope_ok and dilation == 1:
        if transposed and c_out == 16 and k == 4 and stride == 2 and padding == 1 and act == "none":
            return False
    return True


# ----------------------------------------------------------------------------------------------------------------------
# the vocoder under a reduced mode
# ----------------------------------------------------------------------------------------------------------------------
class _ReducedF:
    """Stands in for ``torch.nn.functional`` inside ``oracle.parrot_oracle`` during one generator forward: conv1d /
    conv_transpose1d round the operands of the layers the library evaluates in reduced precision and convolve in
    `acc_dtype` (float32 output, as the library stores it); everything else is torch's."""

    def __init__(self, h: dict, mode: Optional[str], acc_dtype: torch.dtype, fused: int, rtz: bool):
        self.h, self.mode, self.acc, self.fused, self.rtz = h, mode, acc_dtype, fused, rtz
        self.seen_pre = False
        self.stage_c = None
        self.n_dil = 3 if str(h["resblock"]) == "1" else 2
        self.layers = []  # (kind, c_in, c_out, k, reduced) in call order

    def __getattr__(self, name):
        return getattr(_TF, name)

    def _run(self, fn, kind, x, w, b, k, stride, pad, dil, **kw):
        c_in, c_out = (w.shape[0], w.shape[1]) if kind == "convt" else (w.shape[1], w.shape[0])
        red = self.mode is not None and reduced_layer(kind, c_in, c_out, k, stride, dilation=dil, padding=pad,
                                                      pre_slope=0.0, fused=self.fused, resblock_type=int(str(self.h["resblock"])),
                                                      n_dil=self.n_dil)
        self.layers.append((kind, int(c_in), int(c_out), int(k), bool(red)))
        if self.mode is None:  # rounding off: torch's own op on the oracle's own tensors, bit for bit
            return fn(x, w, b, stride=stride, padding=pad, dilation=dil, **kw)
        if red:
            ws = f16_weight_scale(w) if self.mode == "f16" else 1.0
            x = round_operand(x, self.mode, F16_XS, self.rtz)
            w = round_operand(w, self.mode, ws, self.rtz)
        y = fn(x.to(self.acc), w.to(self.acc), None if b is None else b.to(self.acc), stride=stride, padding=pad, dilation=dil, **kw)
        return y.to(torch.float32)

    def conv1d(self, x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
        assert groups == 1
        k = int(w.shape[2])
        if not self.seen_pre:
            self.seen_pre, kind = True, "conv"                   # conv_pre
        elif self.stage_c is not None and w.shape[0] == w.shape[1] == self.stage_c:
            kind = "rb"                                          # a ResBlock conv of the current stage
        else:
            kind = "conv"                                        # conv_post
        return self._run(_TF.conv1d, kind, x, w, b, k, stride, padding, dilation)

    def conv_transpose1d(self, x, w, b=None, stride=1, padding=0, output_padding=0, groups=1, dilation=1):
        assert groups == 1 and output_padding == 0 and dilation == 1
        self.stage_c = int(w.shape[1])
        return self._run(_TF.conv_transpose1d, "convt", x, w, b, int(w.shape[2]), stride, padding, 1)


@contextlib.contextmanager
def reduced_functional(h: dict, mode: Optional[str], acc_dtype: torch.dtype = torch.float64, fused: int = 2, rtz: bool = False):
    """Swap ``oracle.parrot_oracle``'s ``F`` for a rounding one for the duration of the block (restored on exit)."""
    if mode is not None and mode not in MODES:
        raise ValueError(f"unknown reduced mode {mode!r}")
    saved = O.F
    O.F = _ReducedF(h, mode, acc_dtype, fused, rtz)
    try:
        yield O.F
    finally:
        O.F = saved


def code_generator_forward_reduced(sd, h, code, spkr, mode: Optional[str], acc_dtype: torch.dtype = torch.float64,
                                   stages: Optional[dict] = None, fused: int = 2, feats: Optional[dict] = None, rtz: bool = False):
    """``O.code_generator_forward`` with every reduced layer's operands rounded as the library rounds them in `mode`
    ("bf16" | "f16"; None: no rounding and torch's own ops -- bit-equal to the plain oracle) and every conv evaluated in
    `acc_dtype`.  `fused`: the handle's PARROT_FUSED mode (it decides whether the 16-channel ResBlocks are reduced)."""
    with torch.no_grad(), reduced_functional(h, mode, acc_dtype, fused, rtz):
        return O.code_generator_forward(sd, h, code, spkr, stages=stages, feats=feats)


def vocoder_layers(h: dict, fused: int = 2):
    """(kind, c_in, c_out, k, reduced) of every conv of the generator `h` in forward order, under `fused` (bf16 classes)."""
    from parrot_tts_amd import synth
    sd = synth.synth_voc_state_dict(h, seed=0)
    code = torch.zeros((1, 2), dtype=torch.int64)
    spkr = torch.zeros((1, 1), dtype=torch.int64)
    with torch.no_grad(), reduced_functional(h, "bf16", torch.float32, fused) as f:
        O.code_generator_forward(sd, h, code, spkr if h.get("multispkr") else None)
        return list(f.layers)


def generator_stage_reduced(sd, h, stage: str, x: torch.Tensor, mode: Optional[str], acc_dtype: torch.dtype = torch.float64,
                            fused: int = 2, rtz: bool = False) -> torch.Tensor:
    """One stage of ``O.generator_forward`` (models.py:95-111) from a given input, with the reduced-mode emulation of
    ``code_generator_forward_reduced``: "conv_pre" (from the embedding), "ups{i}" (leaky ReLU + ConvTranspose1d, from the
    previous stage), "mrf{i}" (the multi-receptive-field sum / n_kernels, from ``ups{i}``), "post" (leaky ReLU 0.01, conv_post,
    tanh, from the last ``mrf``).  Anchoring every stage at the library's own input of that stage keeps rounding flips of
    earlier stages -- which amplify, one operand ulp at a time, into as large a difference as the rounding itself -- out of
    the comparison."""
    w = O.fold_weight_norm(sd)
    nk = len(h["resblock_kernel_sizes"])
    with torch.no_grad(), reduced_functional(h, mode, acc_dtype, fused, rtz) as f:
        if stage == "conv_pre":
            return O.F.conv1d(x, w["conv_pre.weight"], w["conv_pre.bias"], padding=3)
        f.seen_pre = True
        if stage == "post":
            return torch.tanh(O.F.conv1d(O.F.leaky_relu(x), w["conv_post.weight"], w["conv_post.bias"], padding=3))
        i = int(stage[3:])
        u, k = h["upsample_rates"][i], h["upsample_kernel_sizes"][i]
        if stage.startswith("ups"):
            return O.F.conv_transpose1d(O.F.leaky_relu(x, O.LRELU_SLOPE), w[f"ups.{i}.weight"], w[f"ups.{i}.bias"], stride=u,
                                        padding=(k - u) // 2)
        assert stage.startswith("mrf")
        f.stage_c = int(w[f"ups.{i}.weight"].shape[1])
        rb = O.resblock1 if str(h["resblock"]) == "1" else O.resblock2
        xs = None
        for j in range(nk):  # (generator_forward's order: xs = r0; xs += r1; ...; / nk)
            r = rb(w, f"resblocks.{i * nk + j}.", x, h["resblock_kernel_sizes"][j], h["resblock_dilation_sizes"][j])
            xs = r if xs is None else xs + r
        return xs / nk
