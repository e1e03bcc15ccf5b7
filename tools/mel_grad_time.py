#!/usr/bin/env python3
"""One timing of the mel L1 with its gradient at the reference trainer's shape: utils/vocoder/config.json's batch_size 16 rows of
segment_size 8960 samples (T = 35 frames of 80 mels, n_fft 1024, hop 256).  Two ways to the same gradient, both on the device,
both timed with device events around one call, 3 warm-up calls and `--runs` (>= 10) timed ones in alternation, the median reported
with the minimum and the maximum:

    device     parrot_mel_l1_grad (the forward, the L1 pair, five stages backwards), reduction "mean"
    torch_dev  torch's own: reflect pad, torch.stft, magnitude, matmul, log-clamp, F.l1_loss (fp32) and its backward to the waveform

    python tools/mel_grad_time.py [--runs 20] [--B 16 --N 8960] [--precision f16x3]   -> one JSON line

The line also carries each path's error against the fp64 host run of the same formula, max |g - g_64| / max |g_64| over the batch.
There is no threshold: this is not a measured hot path."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from parrot_tts_amd import _lib  # noqa: E402
from parrot_tts_amd import mel as M  # noqa: E402
from parrot_tts_amd.ops import dptr, stream_ptr  # noqa: E402

H = dict(n_fft=1024, num_mels=80, sampling_rate=16000, hop_size=256, win_size=1024, fmin=0, fmax_for_loss=None)


def torch_mel(y, basis, window):
    """dataset.py:55-67 with the basis and the window passed in, in y's dtype"""
    p = (H["n_fft"] - H["hop_size"]) // 2
    y = F.pad(y.unsqueeze(1), (p, p), mode="reflect").squeeze(1)
    spec = torch.stft(y, H["n_fft"], hop_length=H["hop_size"], win_length=H["win_size"], window=window.to(y.dtype), center=False, pad_mode="reflect",
                      normalized=False, onesided=True, return_complex=True)
    spec = torch.sqrt(torch.real(spec).pow(2) + torch.imag(spec).pow(2) + 1e-9)
    return torch.log(torch.clamp(torch.matmul(basis.to(y.dtype), spec), min=1e-5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--N", type=int, default=8960)
    ap.add_argument("--precision", default=None)
    a = ap.parse_args()
    if a.runs < 10:
        raise SystemExit("mel_grad_time: at least 10 timed runs")
    if not torch.cuda.is_available():
        raise SystemExit("mel_grad_time: no GPU; a timing taken elsewhere says nothing about the device")
    dev = torch.device("cuda:0")
    B, N = a.B, a.N
    g = torch.Generator().manual_seed(0)
    t = torch.arange(N, dtype=torch.float64) / 16000.0  # a voiced-like signal: harmonics of 140 Hz under a slow envelope, plus noise
    wav_h = sum(torch.sin(2 * torch.pi * 140.0 * (h + 1) * t + h) / (h + 1) for h in range(12))[None] * (0.3 + 0.2 * torch.rand(B, 1, generator=g, dtype=torch.float64))
    wav_h = (wav_h * 0.25 + 0.02 * torch.randn(B, N, generator=g, dtype=torch.float64)).to(torch.float32)
    mel = M.MelSpectrogram(H, precision=a.precision)
    basis_h, window_h = mel.basis, mel.window
    with torch.no_grad():
        ref64 = torch_mel(wav_h.double(), basis_h, window_h)
        u = 0.05 + 0.5 * torch.rand(ref64.shape, generator=g, dtype=torch.float64)
        target_h = (ref64 + u * (torch.randint(0, 2, ref64.shape, generator=g) * 2 - 1)).to(torch.float32)
    x64 = wav_h.double().requires_grad_()
    F.l1_loss(torch_mel(x64, basis_h, window_h), target_h.double()).backward()

    wav, target, basis, window = wav_h.to(dev), target_h.to(dev), basis_h.to(dev), window_h.to(dev)
    lib = _lib.lib()
    h = mel._handle(dev)
    out = torch.empty(2 * B, dtype=torch.float64, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    grad = torch.empty((B, N), dtype=torch.float32, device=dev)
    n_ws = int(lib.parrot_mel_l1_grad_workspace_bytes(h, B, N))
    ws = torch.empty(n_ws, dtype=torch.uint8, device=dev)
    leaf = wav.clone().requires_grad_()

    def device_call():
        _lib.check(lib.parrot_mel_l1_grad(h, dptr(wav), wav.stride(0), None, dptr(target), B, N, 0, 1.0, dptr(out), dptr(loss), dptr(grad), dptr(ws), n_ws,
                                          stream_ptr(dev)))

    def torch_dev_call():
        leaf.grad = None
        F.l1_loss(torch_mel(leaf, basis, window), target).backward()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    for _ in range(3):  # warm-up of both paths at the timed shape
        device_call()
        torch_dev_call()
    mel.check(dev)
    rel = lambda gr: float((gr.double().cpu() - x64.grad).abs().max() / x64.grad.abs().max())  # noqa: E731
    res = {"B": B, "N": N, "T": N // H["hop_size"], "precision": mel.precision_in_use(dev), "backward_gemms": "f32, DFT^T in 8 groups", "runs": a.runs,
           "workspace_bytes": n_ws, "loss": float(loss), "rel_err_vs_fp64": {"device": rel(grad), "torch_dev_fp32": rel(leaf.grad)}}
    times = {"device_ms": [], "torch_dev_ms": []}
    for _ in range(a.runs):  # in alternation
        times["device_ms"].append(timed(device_call))
        times["torch_dev_ms"].append(timed(torch_dev_call))
    for k, v in times.items():
        res[k] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
