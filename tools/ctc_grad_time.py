#!/usr/bin/env python3
"""One timing of the CTC loss with its gradient at an aligner-like shape: B = 16 rows of T = 800 frames and N = 100 tokens at V = 50
symbols, every row at full length.  The shape is an assumption, not a measured corpus.  Two ways to the same gradient, both on
the device, both timed with device events around one call, 3 warm-up calls and `--runs` (>= 10) timed ones, the median reported
with the minimum and the maximum:

    device     parrot_ctc_loss_grad (lse, alpha with its store, the token index, beta, the gradient), row weights of "mean"
    torch_dev  torch's own: log_softmax + F.ctc_loss (fp32, reduction "mean") and its backward to the logits

    python tools/ctc_grad_time.py [--runs 20] [--B 16 --T 800 --N 100 --V 50]   -> one JSON line

The line also carries each path's largest absolute distance from the fp64 host run of the same operator.  There is no threshold:
this is not a measured hot path."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from parrot_tts_amd import _lib  # noqa: E402
from parrot_tts_amd.aligner import ctc_reduction_weights  # noqa: E402
from parrot_tts_amd.ops import dptr, stream_ptr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--T", type=int, default=800)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--V", type=int, default=50)
    a = ap.parse_args()
    if a.runs < 10:
        raise SystemExit("ctc_grad_time: at least 10 timed runs")
    if not torch.cuda.is_available():
        raise SystemExit("ctc_grad_time: no GPU; a timing taken elsewhere says nothing about the device")
    dev = torch.device("cuda:0")
    B, T, N, V = a.B, a.T, a.N, a.V
    logits_h = torch.randn((B, T, V), generator=torch.Generator().manual_seed(0)) * 5.0
    tokens_h = torch.from_numpy(np.random.Generator(np.random.PCG64(0)).integers(1, V, size=(B, N)))
    ml_h, tl_h = torch.full((B,), T, dtype=torch.int64), torch.full((B,), N, dtype=torch.int64)
    logits, tokens = logits_h.to(dev), tokens_h.to(dev)
    ml, tl = ml_h.to(dev, torch.int32), tl_h.to(dev, torch.int32)
    ml64, tl64 = ml_h.to(dev), tl_h.to(dev)
    lib = _lib.lib()
    nll = torch.empty((B,), dtype=torch.float64, device=dev)
    grad = torch.empty((B, T, V), dtype=torch.float32, device=dev)
    w = ctc_reduction_weights(tl, "mean")
    n_ws = int(lib.parrot_ctc_grad_workspace_bytes(B, T, V, N))
    ws = torch.empty(n_ws, dtype=torch.uint8, device=dev)
    leaf = logits.clone().requires_grad_()

    def device_call():
        _lib.check(lib.parrot_ctc_loss_grad(dptr(logits), dptr(tokens), dptr(ml), dptr(tl), B, T, V, N, dptr(w), 0, dptr(nll), dptr(grad), dptr(ws),
                                            n_ws, stream_ptr(dev)))

    def torch_dev_call():
        leaf.grad = None
        F.ctc_loss(leaf.transpose(0, 1).log_softmax(2), tokens, ml64, tl64).backward()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    x64 = logits_h.double().requires_grad_()
    F.ctc_loss(x64.transpose(0, 1).log_softmax(2), tokens_h, ml_h, tl_h).backward()
    for _ in range(3):  # warm-up of both paths at the timed shape
        device_call()
        torch_dev_call()
    torch.cuda.synchronize(dev)
    assert int(ws[:4].view(torch.int32).item()) == 0
    dist = lambda g: float((g.double().cpu() - x64.grad).abs().max())  # noqa: E731
    out = {"B": B, "T": T, "N": N, "V": V, "runs": a.runs, "workspace_bytes": n_ws,
           "abs_err_vs_fp64": {"device": dist(grad), "torch_dev_fp32": dist(leaf.grad)}}
    times = {"device_ms": [], "torch_dev_ms": []}
    for _ in range(a.runs):  # in alternation
        times["device_ms"].append(timed(device_call))
        times["torch_dev_ms"].append(timed(torch_dev_call))
    for k, v in times.items():
        out[k] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
