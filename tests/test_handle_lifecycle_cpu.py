"""CPU: the packed-handle lifecycle and the range-safe fallback the three shims share (parrot_tts_amd/_handle.py), driven on the
real ``Parrot``, ``CodeGenerator`` and ``Aligner`` classes: build, destroy and the precision query are recording fakes, and
``torch.device("cuda:N")`` objects stand in for devices -- nothing here touches a GPU or the library."""
import gc
import json
import warnings

import pytest
import torch

from parrot_tts_amd import _handle, _lib, ops, synth
from parrot_tts_amd.aligner import Aligner
from parrot_tts_amd.tte import Parrot
from parrot_tts_amd.vocoder import AttrDict, CodeGenerator

D0, D1 = torch.device("cuda:0"), torch.device("cuda:1")


def _parrot(tmp_path):
    d = tmp_path / "tte"
    d.mkdir(exist_ok=True)
    (d / "speakers.json").write_text(json.dumps({"a": 0, "b": 1}))
    return Parrot(synth.small_tte_config(str(d)), 30, 0)


def _generator(tmp_path):
    return CodeGenerator(AttrDict(synth.small_voc_config()))


def _aligner(tmp_path):
    return Aligner(80, 41, 32, 32)


ALL = [pytest.param(_parrot, Parrot, id="Parrot"), pytest.param(_generator, CodeGenerator, id="CodeGenerator"),
       pytest.param(_aligner, Aligner, id="Aligner")]
WITH_FALLBACK = ALL[:2]


class _Fakes:
    """What the library would have been asked to do, in order: ("build", device) / ("destroy", handle)."""

    def __init__(self):
        self.events, self.precision, self.n = [], ops.PREC_F16X3, 0


@pytest.fixture
def fakes(monkeypatch):
    f = _Fakes()

    def build(self, device, *args, **kwargs):  # what every real _build does on the module
        f.n += 1
        f.events.append(("build", device))
        self._handle, self._handle_device = f"handle{f.n}", device
        if isinstance(self, _handle.RangeFallbackModule):
            self._probe_pending = True

    for cls in (Parrot, CodeGenerator, Aligner):
        monkeypatch.setattr(cls, "_build", build)
    monkeypatch.setattr(_handle.PackedHandleModule, "_destroy_handle", lambda self, h: f.events.append(("destroy", h)))
    monkeypatch.setattr(_handle.PackedHandleModule, "_handle_precision", lambda self, h: f.precision)
    return f


def _reload_through_wrapper(m):
    torch.nn.Sequential(m).load_state_dict({"0." + k: v.clone() for k, v in m.state_dict().items()})


@pytest.mark.parametrize("make, cls", ALL)
def test_handle_is_built_once_and_rebuilt_when_weights_or_device_change(make, cls, fakes, tmp_path):
    m = make(tmp_path)
    assert isinstance(m, _handle.PackedHandleModule) and m.precision_in_use is None
    h1 = m._current_handle(D0)
    assert fakes.events == [("build", D0)] and m._handle == h1 and m._handle_device == D0
    assert m._current_handle(D0) == h1 and fakes.events == [("build", D0)]  # a second call builds nothing
    assert m.precision_in_use == "f16x3"
    with torch.no_grad():
        next(m.parameters()).add_(1.0)  # an in-place write to one parameter
    h2 = m._current_handle(D0)
    assert fakes.events[1:] == [("destroy", h1), ("build", D0)] and h2 != h1  # exactly one destroy, then one build
    assert m._current_handle(D0) == h2 and len(fakes.events) == 3
    _reload_through_wrapper(m)  # torch never calls a child's load_state_dict: the post hook must catch it
    assert m._handle is None and fakes.events[3:] == [("destroy", h2)]
    h3 = m._current_handle(D0)
    assert fakes.events[4:] == [("build", D0)]
    m.double()  # _apply
    assert m._handle is None and fakes.events[5:] == [("destroy", h3)]
    h4 = m._current_handle(D0)
    assert fakes.events[6:] == [("build", D0)]
    h5 = m._current_handle(D1)  # another device
    assert fakes.events[7:] == [("destroy", h4), ("build", D1)] and m._handle_device == D1
    assert m._current_handle(D1) == h5 and len(fakes.events) == 9


@pytest.mark.parametrize("make, cls", ALL)
def test_every_handle_is_destroyed_exactly_once(make, cls, fakes, tmp_path):
    m = make(tmp_path)
    m._invalidate()
    del m
    gc.collect()
    assert fakes.events == []  # a module that was never built destroys nothing
    m = make(tmp_path)
    h = m._current_handle(D0)
    m._invalidate()
    m._invalidate()
    assert fakes.events == [("build", D0), ("destroy", h)] and m._handle is None and m.precision_in_use is None
    h = m._current_handle(D0)
    del fakes.events[:]
    del m  # the last reference
    gc.collect()
    assert fakes.events == [("destroy", h)]


def test_aligner_step_is_no_weight(fakes, tmp_path):
    m = _aligner(tmp_path)
    h = m._current_handle(D0)
    m.step += 1  # what every forward does
    assert m._current_handle(D0) == h and fakes.events == [("build", D0)]
    assert m.get_step() == 2 and "step" in m.state_dict()  # (the fingerprint puts the buffer back)
    with torch.no_grad():
        m.lin.bias.add_(1.0)
    assert m._current_handle(D0) != h


def test_generator_invalidation_drops_its_workspace_cache(fakes, tmp_path):
    g = _generator(tmp_path)
    g._current_handle(D0)
    g._ws = {(1, 7): torch.zeros(4, dtype=torch.uint8)}
    g._invalidate()
    assert g._ws == {}
    g._current_handle(D0)
    g._ws = {(1, 7): torch.zeros(4, dtype=torch.uint8)}
    with torch.no_grad():
        g.conv_post.bias.add_(1.0)
    g._current_handle(D0)  # a rebuild: the cached workspace was sized by the old handle
    assert g._ws == {}


WARNINGS = {
    Parrot: "parrot_tts_amd TTE: why: an activation left the fp16x3 scheme's range (|x| < 8190); rebuilding the handle in bf16x6 "
            "(fp32's range) for this and all later batches.",
    CodeGenerator: "parrot_tts_amd vocoder: why: an activation left the fp16x3 scheme's range (|x| < 8190); rebuilding the handle in "
                   "bf16x6 (fp32's range, ~1.5x slower) for this and all later batches. CodeGenerator.activation_headroom() shows the "
                   "per-stage maxima.",
}


@pytest.mark.parametrize("make, cls", WITH_FALLBACK)
def test_fall_back_switches_an_f16x3_handle_to_bf16x6_and_nothing_else(make, cls, fakes, tmp_path):
    m = make(tmp_path)
    m.range_fallback = True  # (whatever PARROT_RANGE_FALLBACK says here)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # the three refusals are silent
        assert m._fall_back("why") is False  # no handle
        m._current_handle(D0)
        fakes.precision = ops.PREC_BF16X6
        assert m._fall_back("why") is False  # nothing to fall back to
        fakes.precision = ops.PREC_F16X3
        m.range_fallback = False
        assert m._fall_back("why") is False  # switched off
    assert m._precision_override is None and m._handle is not None and len(fakes.events) == 1
    m.range_fallback = True
    h = m._handle
    with pytest.warns(RuntimeWarning, match="bf16x6") as rec:
        assert m._fall_back("why") is True
    assert [str(w.message) for w in rec] == [WARNINGS[cls]]
    assert m._precision_override == ops.PREC_BF16X6 and m._handle is None and fakes.events[1:] == [("destroy", h)]


@pytest.mark.parametrize("make, cls", WITH_FALLBACK)
def test_reload_drops_the_fallbacks_override_and_keeps_the_callers(make, cls, fakes, tmp_path):
    m = make(tmp_path)
    m.range_fallback = True
    m._current_handle(D0)
    with pytest.warns(RuntimeWarning):
        assert m._fall_back("why")
    _reload_through_wrapper(m)
    assert m._precision_override is None  # the new weights get the default scheme again
    m._precision_override = ops.PREC_F32  # the caller's own choice
    m._current_handle(D0)
    _reload_through_wrapper(m)
    assert m._precision_override == ops.PREC_F32 and m._handle is None


class _RecordingLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *args: self.calls.append(name) or 0


@pytest.mark.parametrize("make, cls", WITH_FALLBACK)
def test_first_run_probe_leaves_the_device_alone_when_there_is_nothing_to_fall_back_to(make, cls, fakes, tmp_path, monkeypatch):
    lib = _RecordingLib()
    monkeypatch.setattr(_lib, "lib", lambda: lib)
    m = make(tmp_path)
    m.range_fallback = True
    assert m._first_run_overflowed(D0, "why") is False  # no new handle: no probe
    fakes.precision = ops.PREC_BF16X6
    m._current_handle(D0)
    assert m._probe_pending is True
    assert m._first_run_overflowed(D0, "why") is False and m._probe_pending is False
    m._invalidate()
    fakes.precision = ops.PREC_F16X3
    m.range_fallback = False
    m._current_handle(D0)
    assert m._first_run_overflowed(D0, "why") is False and m._probe_pending is False
    assert lib.calls == []  # neither the peek nor the fetch-and-clear was enqueued
    assert m._precision_override is None and m._handle is not None


def test_library_errors_translate_in_one_place():
    for code, exc in ((-2, IndexError), (-6, FloatingPointError)):
        e = _lib.ParrotHipError(code, "what the library said")
        with pytest.raises(exc) as info:
            _lib.reraise(e)
        assert str(info.value) == str(e) and info.value.__cause__ is None and info.value.__suppress_context__
    e = _lib.ParrotHipError(-4, "what the library said")
    with pytest.raises(_lib.ParrotHipError) as info:
        _lib.reraise(e)
    assert info.value is e and e.code == -4
    seen = []
    with pytest.raises(FloatingPointError):
        _lib.reraise(_lib.ParrotHipError(-6, "x"), on_nonfinite=lambda: seen.append("switched"))
    with pytest.raises(IndexError):
        _lib.reraise(_lib.ParrotHipError(-2, "x"), on_nonfinite=lambda: seen.append("no"))
    assert seen == ["switched"]
    assert _lib.ST_NONFINITE == 5


_EXIT_SCRIPT = """
import ctypes, os, sys
sys.path.insert(0, %r)
import torch
from parrot_tts_amd import _lib, ops, synth
from parrot_tts_amd.aligner import Aligner
from parrot_tts_amd.mel import MelSpectrogram
from parrot_tts_amd.vocoder import AttrDict, CodeGenerator


class FakeLib:  # stands for the loaded library: a live handle means there is one
    def __getattr__(self, name, _write=os.write):
        return lambda handle: _write(1, (name + "\\n").encode())


_lib._lib = FakeLib()
plan = ops.ConvPlan.__new__(ops.ConvPlan)
plan._h = ctypes.c_void_p(1)
aligner = Aligner(80, 41, 32, 32)
aligner._handle = ctypes.c_void_p(2)
generator = CodeGenerator(AttrDict(synth.small_voc_config()))
generator._handle = ctypes.c_void_p(3)
mel = MelSpectrogram.__new__(MelSpectrogram)
mel._handles = {0: ctypes.c_void_p(4)}
"""


def test_objects_alive_at_interpreter_exit_are_finalised_silently():
    """A script that keeps its models in module-level variables and ends: every ``__del__`` runs while module globals are being
    torn down (this package's and torch's), and none may raise -- Python would print 'Exception ignored in ...' for each."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", _EXIT_SCRIPT % root], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]
    # whatever was still destroyed went through the guarded destroy: each handle at most once
    assert sorted(set(out.stdout.split())) == sorted(out.stdout.split())
