#!/usr/bin/env python3
"""Generate tests/golden/mel_*.npz by running the REFERENCE's ``mel_spectrogram`` (utils/vocoder/dataset.py:43-69), imported at run
time from a reference checkout, on CPU in fp32.

The reference module imports ``soundfile``, ``amfm_decompy`` and ``librosa`` at the top; ``mel_spectrogram`` uses none of the
first two, and of librosa only ``librosa.filters.mel``.  Here the first two are bound to empty stub modules and
``librosa.filters.mel`` to ``parrot_tts_amd.mel.slaney_mel_basis_restated`` (librosa itself when it is installed) -- so the fixtures pin
the reference's SIGNAL PATH (reflect pad, torch.stft with its window handling, magnitude, projection, log-clamp) on a given
basis, and carry that basis.  Nothing from the reference is copied: a fixture holds the waveforms, the basis, the window, the
reference's fp32 output, the same formula evaluated in fp64 (tests/mel_ref.py on the fp32 window and basis), and in its meta
``d_ref = max |ref_fp32 - ref_fp64|``: the reference's own distance from the exact value, the unit of the GPU parity bound.

Also cross-checks tests/mel_ref.py (fp32) against the reference bit for bit, and the Conv1d formulation in fp64 within d_ref,
while the reference is at hand.

    python tools/make_mel_goldens.py [--reference DIR]
"""
import argparse
import importlib.util
import json
import math
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mel_ref as R  # noqa: E402
from parrot_tts_amd.mel import slaney_mel_basis_restated  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
SHIPPED = dict(n_fft=1024, num_mels=80, sampling_rate=16000, hop_size=256, win_size=1024, fmin=0, fmax=None)  # utils/vocoder/config.json, fmax_for_loss
CFG2 = dict(n_fft=400, num_mels=40, sampling_rate=16000, hop_size=160, win_size=320, fmin=0, fmax=8000)  # hop % 16 = 0, n_fft % hop != 0, win < n_fft


def load_reference(ref_dir):
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    stub("soundfile")
    stub("amfm_decompy", basic_tools=stub("amfm_decompy.basic_tools"), pYAAPT=stub("amfm_decompy.pYAAPT"))
    try:
        import librosa.filters  # noqa: F401
        import librosa.util  # noqa: F401
    except ImportError:
        def mel(*, sr, n_fft, n_mels, fmin, fmax):
            return slaney_mel_basis_restated(sr, n_fft, n_mels, fmin, fmax)
        stub("librosa", filters=stub("librosa.filters", mel=mel), util=stub("librosa.util", normalize=None))
    spec = importlib.util.spec_from_file_location("ref_vocoder_dataset", os.path.join(ref_dir, "utils", "vocoder", "dataset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def noise(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def fixtures():
    n = 8960  # h.segment_size: what the reference's default validation cuts
    yield "mel_noise", SHIPPED, 0.3 * noise((3, n), 11), "white noise x 0.3"
    yield "mel_tanh", SHIPPED, torch.tanh(2.0 * noise((3, n), 12)), "tanh(2 noise): near full scale"
    z = np.load(os.path.join(GOLD, "voc_full_u40.npz"))
    yield "mel_voc_u40", SHIPPED, torch.from_numpy(z["wav"][:, 0]), "the waveform of voc_full_u40.npz"
    t = torch.arange(n, dtype=torch.float64) / 16000.0
    tone = (0.9 * torch.sin(2 * math.pi * 220.0 * t)).to(torch.float32)
    yield "mel_tone", SHIPPED, tone[None, :] + 1e-4 * noise((3, n), 13), "220 Hz tone at 0.9 + 1e-4 noise: the dynamic-range stress case"
    yield "mel_cfg2", CFG2, 0.3 * noise((3, n), 14), "second config: centred window zero-padding and a partial last tap"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    a = ap.parse_args()
    ref = load_reference(a.reference)
    torch.set_num_threads(8)
    for name, c, wav, what in fixtures():
        with torch.no_grad():
            out = ref.mel_spectrogram(wav, c["n_fft"], c["num_mels"], c["sampling_rate"], c["hop_size"], c["win_size"], c["fmin"], c["fmax"], center=False)
        basis = ref.mel_basis[str(c["fmax"]) + "_cpu"]
        window = ref.hann_window["cpu"]
        args = (c["n_fft"], c["hop_size"], c["win_size"], basis, window)
        out64 = R.mel_ref(wav.double(), *args)
        d_ref = float((out.double() - out64).abs().max())
        mine = R.mel_ref(wav, *args)
        assert torch.equal(mine, out), f"{name}: tests/mel_ref.py differs from the reference by {float((mine - out).abs().max())}"
        d_conv64 = float((R.mel_conv_form(wav.double(), *args) - out64).abs().max())
        d_conv32 = float((R.mel_conv_form(wav, *args).double() - out64).abs().max())
        assert d_conv64 <= d_ref, f"{name}: the fp64 conv form is {d_conv64} from the fp64 reference (d_ref {d_ref})"
        meta = dict(c, what=what, d_ref=d_ref, d_conv_fp64=d_conv64, d_conv_fp32=d_conv32, frames=int(out.shape[-1]),
                    generator="tools/make_mel_goldens.py", torch=torch.__version__)
        np.savez_compressed(os.path.join(GOLD, name + ".npz"), wav=wav.numpy(), basis=basis.numpy(), window=window.numpy(),
                            mel_ref=out.numpy(), mel_ref64=out64.numpy(), meta=json.dumps(meta))
        print(name, tuple(out.shape), f"d_ref {d_ref:.3e} conv fp64 {d_conv64:.3e} conv fp32 {d_conv32:.3e} ({d_conv32 / d_ref:.2f} x d_ref)",
              os.path.getsize(os.path.join(GOLD, name + ".npz")), "bytes")


if __name__ == "__main__":
    main()
