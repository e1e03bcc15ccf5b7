"""Thin tensor-level wrappers over the single-op C-ABI entry points (conv plan, int16 cast, selftest, the TTE's attention cores,
LayerNorm and duration / length-regulator / argmax kernels on their own).

PyTorch is plumbing only: it owns device memory and the stream; all arithmetic happens in
libparrot_hip.so."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib

PRE_NONE, PRE_LRELU = 0, 1
ACT_NONE, ACT_RELU, ACT_TANH = 0, 1, 2
EPI_STORE, EPI_ADD, EPI_ADD_DIV = 0, 1, 2
PREC_F32, PREC_BF16X6, PREC_F16X3, PREC_BF16, PREC_F16 = 0, 1, 2, 3, 4
PREC_NAMES = {"f32": PREC_F32, "bf16x6": PREC_BF16X6, "f16x3": PREC_F16X3, "bf16": PREC_BF16, "f16": PREC_F16}
PREC_DEFAULT = PREC_F16X3
PREC_STR = {v: k for k, v in PREC_NAMES.items()}


def _prec_arg(precision) -> int:
    """A precision argument -- None, a name ("f16x3") or a PARROT_PREC_* code -- as the create calls take it (-1: library default)."""
    return -1 if precision is None else (PREC_NAMES[precision] if isinstance(precision, str) else int(precision))


def set_default_precision(prec: int) -> None:
    """Library-wide default for handles created afterwards (include/parrot_hip.h PARROT_PREC_*): PREC_F32 exact fp32
    MFMA, PREC_F16X3 (default) / PREC_BF16X6 split schemes with fp32-class error, PREC_BF16 / PREC_F16 single-MFMA
    reduced precision."""
    _lib.check(_lib.lib().parrot_set_default_precision(int(prec)))


def set_fused_resblocks(mode: int) -> None:
    """ResBlocks through the fused LDS-resident kernels: 0 off, 1 every eligible stage, 2 all but the exact-fp32
    32-channel kernel (library default).  Applies to handles created afterwards."""
    _lib.check(_lib.lib().parrot_set_fused_resblocks(int(mode)))


def set_tte_merge(on: bool) -> None:
    """FFT blocks: evaluate the back-to-back bias-free projections (quirk Q3) as their fp64-formed product (True, library
    default) or one after the other as the reference does.  Applies to handles created afterwards."""
    _lib.check(_lib.lib().parrot_set_tte_merge(int(bool(on))))


def range_fallback_default() -> bool:
    """PARROT_RANGE_FALLBACK (default on): a handle whose first forward reports a non-finite result under the default fp16x3
    scheme (|activation| >= 8190) is rebuilt in bf16x6 (fp32's range) and the batch re-run, with a warning."""
    import os
    return os.environ.get("PARROT_RANGE_FALLBACK", "1") not in ("", "0")


def stream_ptr(device=None) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def dptr(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


def _workspace(n_bytes, device, at_least: int = 1) -> torch.Tensor:
    """Scratch of ``n_bytes`` (what a ``*_workspace_bytes`` call returned) on ``device`` for one library call.  Never of size
    zero: an empty tensor's pointer is null, which the library takes for a missing argument."""
    return torch.empty(max(int(n_bytes), at_least), dtype=torch.uint8, device=device)


def require_cuda(t: torch.Tensor, name: str) -> None:
    if t.device.type != "cuda":
        raise RuntimeError(f"parrot_tts_amd: `{name}` must live on the GPU (got {t.device}); there is no CPU fallback")


def param_fingerprint(module) -> tuple:
    """Identity + version of every parameter / buffer of ``module``: changes whenever a tensor is replaced, moved or
    written in place (``load_state_dict`` through ANY parent module copies in place and bumps ``_version``).  The HIP
    handle caches packed copies of the weights, so the shims compare this before every forward and rebuild on mismatch."""
    # (a direct walk over the modules' own dicts: `module.parameters()` -- a generator over named_modules with name strings and a
    #  memo set -- cost 390-460 us per call on the full-size generator, on the host's critical path between the TTE's last launch and
    #  the vocoder's first at small batches; this is 130 us and sees the same tensors)
    out = []
    stack = [module]
    while stack:
        m = stack.pop()
        for t in m._parameters.values():
            if t is not None:
                out.append((id(t), t.data_ptr(), t._version))
        for t in m._buffers.values():
            if t is not None:
                out.append((id(t), t.data_ptr(), t._version))
        for c in m._modules.values():
            if c is not None:
                stack.append(c)
    return tuple(out)


def selftest() -> None:
    _lib.check(_lib.lib().parrot_selftest(stream_ptr()))


class ConvPlan:
    """One Conv1d / ConvTranspose1d layer packed for the MFMA implicit-GEMM kernel.

    ``weight`` / ``bias`` are CPU fp32 tensors in torch layout ((C_out,C_in,k), or (C_in,C_out,k) when
    ``transposed``).  ``__call__`` runs y = act(conv(pre(x)) + bias) (+ res) on (B, C, T) CUDA tensors."""

    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *, dilation: int = 1, padding: int = 0,
                 transposed: bool = False, stride: int = 1, pre_act: int = PRE_NONE, pre_slope: float = 0.0,
                 act: int = ACT_NONE, tile_cfg: int = -1, precision: int = -1):
        w = weight.detach().to("cpu", torch.float32).contiguous()
        b = None if bias is None else bias.detach().to("cpu", torch.float32).contiguous()
        c_in, c_out = (w.shape[0], w.shape[1]) if transposed else (w.shape[1], w.shape[0])
        self.c_in, self.c_out = int(c_in), int(c_out)
        d = _lib.ConvDesc(self.c_in, self.c_out, int(w.shape[2]), int(dilation), int(padding), int(bool(transposed)), int(stride),
                          int(pre_act), float(pre_slope), int(act), int(tile_cfg), int(precision))
        self._h = C.c_void_p()
        _lib.check(_lib.lib().parrot_conv_create(C.byref(self._h), C.byref(d), _lib.fptr(w), None if b is None else _lib.fptr(b)))

    def out_len(self, t_in: int) -> int:
        return int(_lib.lib().parrot_conv_out_len(self._h, int(t_in)))

    def __call__(self, x: torch.Tensor, res: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                 epilogue: int = EPI_STORE, div: float = 1.0) -> torch.Tensor:
        require_cuda(x, "x")
        assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 3 and x.shape[1] == self.c_in
        B, _, T = x.shape
        t_out = self.out_len(T)
        if out is None:
            assert epilogue == EPI_STORE
            out = torch.empty((B, self.c_out, t_out), device=x.device, dtype=torch.float32)
        assert out.is_contiguous() and tuple(out.shape) == (B, self.c_out, t_out)
        if res is not None:
            assert res.is_contiguous() and res.shape == out.shape
        _lib.check(_lib.lib().parrot_conv_run(self._h, dptr(x), dptr(res), dptr(out), B, T, int(epilogue), float(div), stream_ptr(x.device)))
        return out

    def __del__(self, _destroy=_lib.destroy):  # (bound here: module globals are already torn down at interpreter exit)
        h, self._h = getattr(self, "_h", None), None
        _destroy("parrot_conv_destroy", h)


def wav_to_int16(wav: torch.Tensor) -> torch.Tensor:
    """``(audio * 32768).astype('int16')`` of reference utils/vocoder/inference.py:71-73, on the GPU."""
    require_cuda(wav, "wav")
    w = wav.contiguous()
    out = torch.empty(w.shape, device=w.device, dtype=torch.int16)
    _lib.check(_lib.lib().parrot_wav_to_int16(dptr(w), dptr(out), w.numel(), stream_ptr(w.device)))
    return out


def length_regulator(seq: torch.Tensor, dur: torch.Tensor):
    """``length_regulator`` of reference modules/duration.py:6-24 on the HIP kernel the TTE decoder uses: seq (B,S,D) f32,
    dur (B,S) int64 -> (expanded (B,L,D) zero-padded to L = max row sum, tgt_mask (B,L) bool with the ``ids <= len`` rule
    of modules/data.py:18, out_lens list).  L is read back to the host like the reference does (duration.py:10)."""
    require_cuda(seq, "seq")
    seq = seq.to(torch.float32).contiguous()
    dur = dur.to(seq.device, torch.int64).contiguous()
    B, S, D = seq.shape
    L = int(torch.clamp(dur, min=0).sum(dim=1).max())  # the reference's own host sync
    if L <= 0:
        raise ValueError("length_regulator: every duration is zero (the reference fails downstream on an empty sequence)")
    lib = _lib.lib()
    ws = _workspace(lib.parrot_length_regulator_workspace_bytes(B, S, D, L), seq.device)
    out = torch.empty((B, L, D), dtype=torch.float32, device=seq.device)
    mask = torch.empty((B, L), dtype=torch.uint8, device=seq.device)
    lens = torch.empty((B,), dtype=torch.int32, device=seq.device)
    with torch.cuda.device(seq.device):
        _lib.check(lib.parrot_length_regulator(dptr(seq), dptr(dur), B, S, D, L, dptr(out), dptr(mask), dptr(lens), dptr(ws), ws.numel(),
                                               stream_ptr(seq.device)))
    return out, mask.bool(), lens.cpu().tolist()


ATTN_THREE_KERNEL, ATTN_FUSED, ATTN_FLASH = 0, 1, 2


def debug_attention(qkv: torch.Tensor, valid: torch.Tensor, heads: int, core: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One attention core of the TTE's FFT block on its own (tests; include/parrot_hip_debug.h): qkv (B, 3, D, T) f32 channel-first,
    valid (B, T) uint8 with non-zero = attend to this key -> ctx (B, D, T).  ``core``: ATTN_THREE_KERNEL, ATTN_FUSED or ATTN_FLASH;
    a core that does not take (D / heads, T) raises ParrotHipError with code -5."""
    require_cuda(qkv, "qkv")
    assert qkv.dtype == torch.float32 and qkv.is_contiguous() and qkv.dim() == 4 and qkv.shape[1] == 3
    B, _, D, T = qkv.shape
    assert D % heads == 0 and valid.dtype == torch.uint8 and valid.is_contiguous() and tuple(valid.shape) == (B, T)
    require_cuda(valid, "valid")
    if out is None:
        out = torch.empty((B, D, T), device=qkv.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (B, D, T)
    lib = _lib.lib()
    ws = _workspace(lib.parrot_debug_attention_workspace_bytes(B, T, heads, int(core)), qkv.device)
    with torch.cuda.device(qkv.device):
        _lib.check(lib.parrot_debug_attention(dptr(qkv), dptr(valid), dptr(out), B, T, heads, D // heads, int(core), dptr(ws), ws.numel(),
                                              stream_ptr(qkv.device)))
    return out


def debug_layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, relu_in: bool = False,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The TTE's LayerNorm over the channels of a channel-first (B, C, T) f32 tensor (of relu(x) when ``relu_in``), eps 1e-5, on its
    own (tests; include/parrot_hip_debug.h)."""
    require_cuda(x, "x")
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 3
    B, C_, T = x.shape
    for t in (gamma, beta):
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (C_,) and t.device == x.device
    if out is None:
        out = torch.empty_like(x)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == x.shape
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().parrot_debug_layernorm(dptr(x), dptr(gamma), dptr(beta), dptr(out), B, C_, T, int(bool(relu_in)),
                                                     stream_ptr(x.device)))
    return out


TIE_GUARD_MAX = 256  # guarded positions per decoder lane (csrc/tte_glue.h)


def _dev_arg(t: Optional[torch.Tensor], dtype, shape, dev, name: str) -> None:
    if t is not None:
        assert t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == tuple(shape) and t.device == dev, name


def debug_durations(ld_raw: torch.Tensor, src_valid: torch.Tensor, src_len: Optional[torch.Tensor] = None, out: Optional[dict] = None) -> dict:
    """duration_kernel on its own (tests; include/parrot_hip_debug.h): ld_raw (B, S) f32, src_valid (B, S) u8, src_len (B) i32 or None
    -> {"log_dur" (B, S) f32, "dur" (B, S) i64, "cum" (B, S) i32, "out_len" (B) i32, "status" (1) i32}.  ``out``: such a dict of
    caller-owned tensors to write into (``status`` is then not cleared first)."""
    require_cuda(ld_raw, "ld_raw")
    dev = ld_raw.device
    assert ld_raw.dim() == 2
    B, S = ld_raw.shape
    _dev_arg(ld_raw, torch.float32, (B, S), dev, "ld_raw")
    _dev_arg(src_valid, torch.uint8, (B, S), dev, "src_valid")
    _dev_arg(src_len, torch.int32, (B,), dev, "src_len")
    if out is None:
        out = {"log_dur": torch.empty((B, S), dtype=torch.float32, device=dev), "dur": torch.empty((B, S), dtype=torch.int64, device=dev),
               "cum": torch.empty((B, S), dtype=torch.int32, device=dev), "out_len": torch.empty((B,), dtype=torch.int32, device=dev),
               "status": torch.zeros((1,), dtype=torch.int32, device=dev)}
    for k, (dt, sh) in dict(log_dur=(torch.float32, (B, S)), dur=(torch.int64, (B, S)), cum=(torch.int32, (B, S)),
                            out_len=(torch.int32, (B,)), status=(torch.int32, (1,))).items():
        _dev_arg(out[k], dt, sh, dev, k)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().parrot_debug_durations(dptr(ld_raw), dptr(src_valid), dptr(src_len), B, S, dptr(out["log_dur"]), dptr(out["dur"]),
                                                     dptr(out["cum"]), dptr(out["out_len"]), dptr(out["status"]), stream_ptr(dev)))
    return out


def debug_length_regulate(enc: torch.Tensor, dur: torch.Tensor, pe: torch.Tensor, L: int, row_exact: bool = False,
                          src_len: Optional[torch.Tensor] = None, want_mask: bool = True, out: Optional[dict] = None) -> dict:
    """dur_prefix_kernel + length_regulate_kernel on their own (tests): enc (B, D, S) f32 channel-first, dur (B, S) i64, pe (P, D) f32
    -> {"y" (B, D, L), "tgt_mask" (B, L) u8 or None, "cum" (B, S) i32, "out_len" (B) i32, "status" (1) i32}."""
    require_cuda(enc, "enc")
    dev = enc.device
    assert enc.dim() == 3 and pe.dim() == 2
    B, D, S = enc.shape
    P = pe.shape[0]
    _dev_arg(enc, torch.float32, (B, D, S), dev, "enc")
    _dev_arg(dur, torch.int64, (B, S), dev, "dur")
    _dev_arg(pe, torch.float32, (P, D), dev, "pe")
    _dev_arg(src_len, torch.int32, (B,), dev, "src_len")
    if out is None:
        n = max(int(L), 1)
        out = {"y": torch.empty((B, D, n), dtype=torch.float32, device=dev),
               "tgt_mask": torch.empty((B, n), dtype=torch.uint8, device=dev) if want_mask else None,
               "cum": torch.empty((B, S), dtype=torch.int32, device=dev), "out_len": torch.empty((B,), dtype=torch.int32, device=dev),
               "status": torch.zeros((1,), dtype=torch.int32, device=dev)}
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().parrot_debug_length_regulate(dptr(enc), dptr(dur), dptr(src_len), dptr(pe), B, S, D, int(L), P, int(bool(row_exact)),
                                                           dptr(out["y"]), dptr(out["tgt_mask"]), dptr(out["cum"]), dptr(out["out_len"]),
                                                           dptr(out["status"]), stream_ptr(dev)))
    return out


def debug_argmax_guard(logits: torch.Tensor, guard: float, row0: int = 0, refine: Optional[dict] = None, gstat_start=None,
                       out: Optional[dict] = None) -> dict:
    """argmax_cf_kernel (+ tie_guard_refine_kernel when ``refine`` is given) on their own (tests): logits (B, V, L) f32 channel-first
    -> {"ids" (B, L) i64, "glist" (256, 2) i32, "gstat" (4) i32, "gref" (256, V) f32, "status" (1) i32}.  ``refine``: {"x" (B, D, L),
    "hwt" (D, V), "hb" (V) or None} and for the deep form also {"f" (B, F, L), "h" (B, D, L), "w2t" (F, D), "b2" (D) or None}.
    ``gstat_start``: four ints, what gstat holds before the launch (NULL: a restart)."""
    require_cuda(logits, "logits")
    dev = logits.device
    assert logits.dim() == 3
    B, V, L = logits.shape
    _dev_arg(logits, torch.float32, (B, V, L), dev, "logits")
    r = dict(refine or {})
    x, f = r.get("x"), r.get("f")
    D = int(x.shape[1]) if x is not None else 0
    F = int(f.shape[1]) if f is not None else 0
    for k, sh in dict(x=(B, D, L), hwt=(D, V), hb=(V,), f=(B, F, L), h=(B, D, L), w2t=(F, D), b2=(D,)).items():
        _dev_arg(r.get(k), torch.float32, sh, dev, k)
    if out is None:
        out = {"ids": torch.empty((B, L), dtype=torch.int64, device=dev), "glist": torch.zeros((TIE_GUARD_MAX, 2), dtype=torch.int32, device=dev),
               "gstat": torch.zeros((4,), dtype=torch.int32, device=dev), "gref": torch.zeros((TIE_GUARD_MAX, V), dtype=torch.float32, device=dev),
               "status": torch.zeros((1,), dtype=torch.int32, device=dev)}
    start = None if gstat_start is None else (C.c_int32 * 4)(*[int(v) for v in gstat_start])
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().parrot_debug_argmax_guard(dptr(logits), B, V, L, float(guard), int(row0), dptr(x), D, dptr(r.get("hwt")),
                                                        dptr(r.get("hb")), dptr(f), dptr(r.get("h")), dptr(r.get("w2t")), dptr(r.get("b2")), F,
                                                        start, dptr(out["ids"]), dptr(out["glist"]), dptr(out["gstat"]), dptr(out["gref"]),
                                                        dptr(out["status"]), stream_ptr(dev)))
    return out


# ---- the aligner's training kernels on their own (tests; include/parrot_hip_debug.h) --------------------------------------------------------
# A set ``p`` is a dict with the names of the kernel's parameter struct (tests/aligner_train_kernels_ref.py writes the model's own);
# ``x_base`` / ``c_base`` / ``y_base`` / per-tap ``a_off`` are element offsets into the flat buffers.  The *_desc functions only fill
# a descriptor and take any parrot_debug_buf (the refusal tests hand in made-up ones and call the library without a device).
def debug_buf(t: Optional[torch.Tensor], base: int = 0) -> _lib.DebugBuf:
    """A flat fp32 device tensor from element ``base`` on; None: the null buffer."""
    if t is None:
        return _lib.DebugBuf(None, 0)
    require_cuda(t, "buffer")
    assert t.dtype == torch.float32 and t.is_contiguous() and 0 <= base < t.numel()
    return _lib.DebugBuf(t.data_ptr() + 4 * base, t.numel() - base)


def _offset_buf(b: _lib.DebugBuf, base: int) -> _lib.DebugBuf:
    return _lib.DebugBuf((b.p or 0) + 4 * base if b.p else None, b.n - base)


def tap_gemm_desc(p: dict, A: _lib.DebugBuf, X: _lib.DebugBuf, Cb: _lib.DebugBuf, bias0=None, bias1=None) -> _lib.DebugTapGemmDesc:
    d = _lib.DebugTapGemmDesc()
    d.ntaps = p["ntaps"]
    for j in range(min(p["ntaps"], _lib.DEBUG_MAX_TAPS)):
        d.A[j] = _offset_buf(A, p["a_off"][j])
        d.x_off[j], d.shift[j] = p["x_off"][j], p["shift"][j]
    d.X, d.C = _offset_buf(X, p.get("x_base", 0)), _offset_buf(Cb, p.get("c_base", 0))
    d.bias0, d.bias1 = bias0 or _lib.DebugBuf(None, 0), bias1 or _lib.DebugBuf(None, 0)
    for k in ("M", "N", "K", "Z", "a_sm", "a_sk", "x_sz", "x_sk", "x_sn", "c_sz", "c_sm", "c_sn", "relu"):
        setattr(d, k, p[k])
    return d


def wgrad_desc(p: dict, dY: _lib.DebugBuf, X: _lib.DebugBuf, out: _lib.DebugBuf) -> _lib.DebugWgradDesc:
    d = _lib.DebugWgradDesc()
    d.dY, d.X, d.out = _offset_buf(dY, p.get("y_base", 0)), _offset_buf(X, p.get("x_base", 0)), out
    for j in range(min(p["ntaps"], _lib.DEBUG_MAX_TAPS)):
        d.shift[j] = p["shift"][j]
    for k in ("M", "K", "T", "R", "ntaps", "y_sz", "y_sm", "y_st", "x_sz", "x_sk", "x_st", "o_sm", "o_sk", "o_sj"):
        setattr(d, k, p[k])
    return d


def debug_tap_gemm(p: dict, A: torch.Tensor, X: torch.Tensor, Cb: torch.Tensor, bias0=None, bias1=None) -> torch.Tensor:
    """tap_gemm_kernel through launch_tap_gemm: writes the addressed elements of the flat ``Cb`` in place and returns it."""
    d = tap_gemm_desc(p, debug_buf(A), debug_buf(X), debug_buf(Cb), debug_buf(bias0), debug_buf(bias1))
    with torch.cuda.device(Cb.device):
        _lib.check(_lib.lib().parrot_debug_tap_gemm(C.byref(d), stream_ptr(Cb.device)))
    return Cb


def debug_wgrad(p: dict, dY: torch.Tensor, X: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """wgrad_kernel + wgrad_reduce_kernel as the model's wgrad() runs them; writes the addressed elements of the flat ``out``."""
    d = wgrad_desc(p, debug_buf(dY), debug_buf(X), debug_buf(out))
    lib = _lib.lib()
    ws = _workspace(lib.parrot_debug_wgrad_workspace_bytes(p["R"], p["ntaps"], p["M"], p["K"]), out.device)
    with torch.cuda.device(out.device):
        _lib.check(lib.parrot_debug_wgrad(C.byref(d), dptr(ws), ws.numel(), stream_ptr(out.device)))
    return out


def debug_colsum(src: torch.Tensor, R: int, M: int, ld: int, out0: torch.Tensor, out1: Optional[torch.Tensor] = None, base: int = 0):
    """colsum_part_kernel + colsum_final_kernel: out0[m] (and out1[m]) = sum_r src[base + r ld + m]."""
    d = _lib.DebugColsumDesc(debug_buf(src, base), debug_buf(out0), debug_buf(out1), R, M, ld)
    lib = _lib.lib()
    ws = _workspace(lib.parrot_debug_colsum_workspace_bytes(R, M), src.device)
    with torch.cuda.device(src.device):
        _lib.check(lib.parrot_debug_colsum(C.byref(d), dptr(ws), ws.numel(), stream_ptr(src.device)))
    return out0, out1


def debug_bn_train(x: torch.Tensor, y: torch.Tensor, gamma, beta, run_mean, run_var, mean, invstd, training: bool, eps: float) -> None:
    """bn_train_kernel on x (B, C, T): writes y, mean, invstd and -- training -- updates run_mean / run_var in place."""
    B, C_, T = x.shape
    d = _lib.DebugBnTrainDesc(*[debug_buf(t) for t in (x, y, gamma, beta, run_mean, run_var, mean, invstd)], B, C_, T, int(bool(training)), eps)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().parrot_debug_bn_train(C.byref(d), stream_ptr(x.device)))


def debug_bn_relu_bwd(dy: torch.Tensor, x: torch.Tensor, dx: torch.Tensor, gamma, mean, invstd, dgamma=None, dbeta=None) -> None:
    """bn_relu_bwd_kernel on (B, C, T): writes dx (which may be dy) and, when given, dgamma / dbeta."""
    B, C_, T = x.shape
    d = _lib.DebugBnBwdDesc(*[debug_buf(t) for t in (dy, x, dx, gamma, mean, invstd, dgamma, dbeta)], B, C_, T)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().parrot_debug_bn_relu_bwd(C.byref(d), stream_ptr(x.device)))


def debug_lstm(w_hh: torch.Tensor, xproj: torch.Tensor, kernel: int, h0: Optional[torch.Tensor] = None, c0: Optional[torch.Tensor] = None,
               n_steps: Optional[int] = None, out: Optional[torch.Tensor] = None) -> dict:
    """The aligner's LSTM recurrence on its own, through the step loop of the inference forward (``kernel`` 0, lstm_step_kernel) or of
    the training forward (1, lstm_train_step_kernel) (tests; include/parrot_hip_debug.h): w_hh (2, 4H, H), xproj (B, T, 8H), h0 / c0
    (2, B, H) or None for zeros -> {"out" (B, T, 2H), "h_n", "c_n" (2, B, H), and for kernel 1 "gates" (B, T, 8H), "c_all" (B, T, 2H)}.
    ``n_steps`` < T runs the first steps only; ``out``: a caller-filled tensor whose other frames are left alone."""
    require_cuda(xproj, "xproj")
    dev = xproj.device
    assert xproj.dim() == 3 and w_hh.dim() == 3
    B, T, H = int(xproj.shape[0]), int(xproj.shape[1]), int(w_hh.shape[2])
    _dev_arg(w_hh, torch.float32, (2, 4 * H, H), dev, "w_hh")
    _dev_arg(xproj, torch.float32, (B, T, 8 * H), dev, "xproj")
    _dev_arg(h0, torch.float32, (2, B, H), dev, "h0")
    _dev_arg(c0, torch.float32, (2, B, H), dev, "c0")
    if out is None:
        out = torch.empty((B, T, 2 * H), dtype=torch.float32, device=dev)
    _dev_arg(out, torch.float32, (B, T, 2 * H), dev, "out")
    res = {"out": out, "h_n": torch.empty((2, B, H), dtype=torch.float32, device=dev), "c_n": torch.empty((2, B, H), dtype=torch.float32, device=dev)}
    if kernel == 1:
        res["gates"] = torch.empty((B, T, 8 * H), dtype=torch.float32, device=dev)
        res["c_all"] = torch.empty((B, T, 2 * H), dtype=torch.float32, device=dev)
    lib = _lib.lib()
    n_ws = int(lib.parrot_debug_lstm_workspace_bytes(B, T, H, int(kernel)))
    ws = _workspace(n_ws, dev)
    with torch.cuda.device(dev):
        _lib.check(lib.parrot_debug_lstm(dptr(w_hh), dptr(xproj), dptr(h0), dptr(c0), B, T, H, T if n_steps is None else int(n_steps), int(kernel),
                                         dptr(out), dptr(res["h_n"]), dptr(res["c_n"]), dptr(res.get("gates")), dptr(res.get("c_all")), dptr(ws),
                                         n_ws, stream_ptr(dev)))
    return res
