#!/usr/bin/env python3
"""The mel of a B = 64 x 81 920 batch (the waveform of a full-size vocoder step) beside that vocoder step, in one process.

    python tools/mel_perf.py [--iters 30] [--precision f16x3|bf16x6|f32]     -> one JSON line

Run under `rocprofv3 --kernel-trace --stats` for the per-kernel times (profiles/mel.md): mel_frame_kernel reads and writes the
padded signal once (2 x 21 MB), mel_magnitude_kernel reads (B, 1026, 320) and writes (B, 528, 320) floats (84 + 43 MB).  The mel
calls rotate over --copies distinct waveforms; the whole working set of one call (21 + 21 + 84 + 43 + 6.5 MB) fits the 256 MiB
Infinity Cache, so what a kernel reads right after its producer wrote it may come from there -- the bytes-per-second figures of
profiles/mel.md are of traffic at the kernels' interface, not of HBM."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from parrot_tts_amd import synth  # noqa: E402
from parrot_tts_amd.mel import MelSpectrogram, mel_l1  # noqa: E402
from parrot_tts_amd.vocoder import AttrDict, CodeGenerator  # noqa: E402

MEL_H = dict(n_fft=1024, num_mels=80, sampling_rate=16000, hop_size=256, win_size=1024, fmin=0, fmax_for_loss=None)


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--copies", type=int, default=4)
    ap.add_argument("--precision", default=None, help="of the mel handle (default: f16x3)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    h = synth.default_voc_config()
    g = CodeGenerator(AttrDict(h))
    g.load_state_dict(synth.synth_voc_state_dict(h, seed=1234))
    g = g.eval().to(dev)
    b = synth.synth_voc_batch(64, 256, h, seed=3)
    code, spkr = b["code"].to(dev), b["spkr"].to(dev)
    mel = MelSpectrogram(MEL_H, precision=a.precision)
    wavs = [g(code=torch.roll(code, i, 0), spkr=spkr)[:, 0].contiguous() for i in range(a.copies)]
    g.check_inputs()
    for i in range(3):
        g(code=code, spkr=spkr)
        mel(wavs[i % len(wavs)], check=False)
    t_voc, t_mel = [], []
    for i in range(a.iters):  # interleaved: drift hits both alike
        t_voc.append(timed(lambda: g(code=code, spkr=spkr), dev))
        t_mel.append(timed(lambda i=i: mel(wavs[i % len(wavs)], check=False), dev))
    m0, m1 = mel(wavs[0], check=False), mel(wavs[1], check=False)
    t_l1 = [timed(lambda: mel_l1(m0, m1), dev) for _ in range(a.iters)]
    mel.check(dev)
    print(json.dumps({"B": 64, "N": 81920, "frames": int(m0.shape[-1]), "iters": a.iters, "precision": mel.precision_in_use(dev),
                      "vocoder_step_ms_median": statistics.median(t_voc), "vocoder_step_ms_min": min(t_voc),
                      "mel_ms_median": statistics.median(t_mel), "mel_ms_min": min(t_mel),
                      "mel_l1_ms_median": statistics.median(t_l1), "mel_l1_ms_min": min(t_l1),
                      "mel_spec_error_of_two_batches": float(mel_l1(m0, m1)[0]),
                      "note": "wall time per call incl. one host sync; kernel times: rocprofv3 --kernel-trace --stats"}))


if __name__ == "__main__":
    main()
