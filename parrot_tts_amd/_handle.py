"""When a handle of packed weights must be rebuilt, and what happens when the fp16x3 scheme overflows: the one place that knows.

``PackedHandleModule`` is the base of the shims that hold parameters for a library handle (``Parrot``, ``CodeGenerator``,
``Aligner``): the handle caches packed copies of the weights, so it is dropped whenever they are reloaded, moved or written in
place, and rebuilt on the next forward.  ``RangeFallbackModule`` adds the range-safe fallback of the two shims that have one
(``Parrot``, ``CodeGenerator``)."""
from __future__ import annotations

import ctypes as C
import warnings
from typing import Optional

import torch
import torch.nn as nn

from . import _lib
from .ops import PREC_BF16X6, PREC_F16X3, PREC_STR, dptr, param_fingerprint, range_fallback_default, stream_ptr


def _attach(root: nn.Module, dotted: str, tensor: torch.Tensor, buffer: bool = False) -> None:
    """Register ``tensor`` under a dotted state_dict key, creating plain container modules on the way
    (numeric path parts are fine: nn.Module accepts '0' as a child name, as ModuleList does)."""
    parts = dotted.split(".")
    m = root
    for p in parts[:-1]:
        if p not in m._modules:
            m.add_module(p, nn.Module())
        m = m._modules[p]
    if buffer:
        m.register_buffer(parts[-1], tensor)
    else:
        m.register_parameter(parts[-1], nn.Parameter(tensor))


class PackedHandleModule(nn.Module):
    """A subclass names the library functions that destroy a handle and report its precision, and supplies ``_build(device)``,
    which creates the handle and sets ``_handle`` and ``_handle_device``."""

    _destroy_fn = _precision_fn = ""
    _handle: Optional[C.c_void_p] = None  # (class-level defaults: __del__ also runs on a module whose __init__ raised)
    _handle_device = None
    _handle_fp = None

    def __init__(self):
        super().__init__()
        # torch's load_state_dict recurses through _load_from_state_dict and never calls a CHILD's load_state_dict
        # override, so a reload through any wrapper (LitParrot, nn.Sequential ...) is caught here: the post hook runs
        # for every module of the tree, and _current_handle() also compares the parameters' version fingerprint.
        # (`_invalidate` is looked up on the instance when the hook runs.)
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._invalidate())

    # the two seams the CPU tests replace with recording fakes (and the only ones)
    def _destroy_handle(self, handle, _destroy=_lib.destroy) -> None:  # (bound here: __del__ runs at interpreter exit too,
        _destroy(self._destroy_fn, handle)                             #  when this module's globals are already torn down)

    def _handle_precision(self, handle) -> int:
        return int(getattr(_lib.lib(), self._precision_fn)(handle))

    def _weight_fingerprint(self) -> tuple:
        return param_fingerprint(self)

    def _invalidate(self):
        if self._handle is not None:
            self._destroy_handle(self._handle)
        self._handle = None

    def _current_handle(self, dev):
        """The packed-weight handle for ``dev``, rebuilt when any parameter was replaced, moved or written in place."""
        fp = self._weight_fingerprint()
        if self._handle is None or self._handle_device != dev or self._handle_fp != fp:
            self._invalidate()
            self._build(dev)
            self._handle_fp = fp
        return self._handle

    def _apply(self, fn, recurse=True):
        self._invalidate()
        return super()._apply(fn, recurse)

    def __del__(self):
        # (not _invalidate(): at interpreter exit nn.Module.__setattr__ no longer works, torch's globals being torn down as well)
        handle = self.__dict__.pop("_handle", None)
        if handle is not None:
            self._destroy_handle(handle)

    @property
    def precision_in_use(self) -> Optional[str]:
        """Precision of the live handle ("f16x3", "bf16x6", "f32", ...; None before the first forward): "bf16x6" after the
        range-safe fallback replaced a default-precision handle."""
        if self._handle is None:
            return None
        return PREC_STR.get(self._handle_precision(self._handle))


class RangeFallbackModule(PackedHandleModule):
    """Range-safe fallback: the default fp16x3 scheme needs |activation| < 8190, which no checkpoint format promises.  The FIRST
    run of every new handle is checked synchronously (one sync per handle lifetime); a non-finite result rebuilds the handle in
    bf16x6 (fp32's range), re-runs the batch and warns.  Later runs are covered by the asynchronous flag.

    A subclass names the library functions that peek at and fetch-and-clear the handle's device flag and the two pieces of the
    warning that are its own; its ``_build`` passes ``_precision_override`` on and sets ``_probe_pending`` for a handle it installs."""

    _peek_fn = _status_fn = ""
    _warn_name = ""                   # "parrot_tts_amd <name>: ..."
    _warn_cost = _warn_hint = ""      # the vocoder's: what bf16x6 costs, where to look

    def __init__(self):
        super().__init__()
        self.range_fallback = range_fallback_default()
        self._precision_override: Optional[int] = None  # PARROT_PREC_* this module's handles are created with (None: library default)
        self._fell_back = False  # the override above was set by the range-safe fallback (not by the caller)
        self._probe_pending = False
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._on_load())

    def _on_load(self):
        """New weights (the base's hook drops the packed handle): drop a bf16x6 override that the range-safe fallback set for the
        OLD weights (the new checkpoint gets the default scheme and its own first-run probe)."""
        if self._fell_back:
            self._precision_override, self._fell_back = None, False

    def _fall_back(self, why: str, stacklevel: int = 3) -> bool:
        """Switch this module to bf16x6 handles after a non-finite result under the fp16x3 scheme.  Returns False when there is
        nothing to fall back to (already fp32-range, or the fallback is switched off).  ``stacklevel``: the warning's, 3 = the
        caller of the shim method that calls this (from the first-run probe: that shim method itself)."""
        cur = None if self._handle is None else self._handle_precision(self._handle)
        if not self.range_fallback or cur != PREC_F16X3:
            return False
        warnings.warn(f"parrot_tts_amd {self._warn_name}: {why}: an activation left the fp16x3 scheme's range (|x| < 8190); rebuilding "
                      f"the handle in bf16x6 (fp32's range{self._warn_cost}) for this and all later batches.{self._warn_hint}",
                      RuntimeWarning, stacklevel=stacklevel)
        self._precision_override = PREC_BF16X6
        self._fell_back = True
        self._invalidate()
        return True

    def _first_run_overflowed(self, dev, why: str) -> bool:
        """After the FIRST run of a handle: one synchronous look at the device flag; True = the handle was replaced by a bf16x6
        one and the caller re-runs its batch.  With nothing to fall back to the device is not touched; a bad-id flag, or a
        non-finite result on such a handle, stays set for the regular reporting path (the check call / the status hook)."""
        if not self._probe_pending:
            return False
        self._probe_pending = False
        if not self.range_fallback or self._handle_precision(self._handle) != PREC_F16X3:
            return False
        lib = _lib.lib()
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            st = stream_ptr(dev)
            _lib.check(getattr(lib, self._peek_fn)(self._handle, dptr(flag), st))
            if int(flag.cpu()) != _lib.ST_NONFINITE:
                return False
            _lib.check(getattr(lib, self._status_fn)(self._handle, dptr(flag), st))  # handled here: clear it
        return self._fall_back(why)
