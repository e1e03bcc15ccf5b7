#!/usr/bin/env python3
"""The aligner's CTC validation loss on one training batch of the reference's config: B = 16 rows of T = 2000 frames and N = 200
tokens at V = 41 symbols, every row at full length (the longest the batch can be).  Three ways to the same numbers:

    device     the library's kernel pair (parrot_ctc_loss: ctc_lse_kernel + ctc_alpha_kernel + the mean), device events around
               `--calls` back-to-back calls, no host synchronisation inside the window; `api_ms` is one `aligner.ctc_loss` call
               with its status read-back, by the host clock
    torch_cpu  log_softmax + torch.nn.functional.ctc_loss in fp32 on the host (the reference trainer's operator), host clock
    torch_dev  the same two torch operators on the device, device events

    python tools/ctc_bench.py [--rounds 7 --calls 20] [--B 16 --T 2000 --N 200 --V 41]   -> one JSON line

Every path is warmed up first; the three are measured in alternation, `--rounds` times, and the line carries the median and the
minimum / maximum of each, so that the spread can be seen beside the difference.  The line also carries each path's largest
relative distance from the fp64 host run of the same operator: a faster path that computes something else is not faster."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from parrot_tts_amd import _lib  # noqa: E402
from parrot_tts_amd.aligner import ctc_loss  # noqa: E402
from parrot_tts_amd.ops import dptr, stream_ptr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--T", type=int, default=2000)
    ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--V", type=int, default=41)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_bench: no GPU; a timing taken elsewhere says nothing about the device")
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
    mean = torch.empty((), dtype=torch.float32, device=dev)
    n_ws = int(lib.parrot_ctc_workspace_bytes(B, T, N))
    ws = torch.empty(n_ws, dtype=torch.uint8, device=dev)
    torch.set_num_threads(min(16, os.cpu_count() or 1))

    def device_call():
        _lib.check(lib.parrot_ctc_loss(dptr(logits), dptr(tokens), dptr(ml), dptr(tl), B, T, V, N, dptr(nll), dptr(mean), dptr(ws), n_ws, stream_ptr(dev)))

    def torch_dev_call():
        return F.ctc_loss(logits.transpose(0, 1).log_softmax(2), tokens, ml64, tl64, reduction="none")

    def torch_cpu_call(dtype=torch.float32):
        return F.ctc_loss(logits_h.to(dtype).transpose(0, 1).log_softmax(2), tokens_h, ml_h, tl_h, reduction="none")

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) / a.calls

    def host(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    y64 = torch_cpu_call(torch.float64)
    rel = lambda v: float(((v.double().cpu() - y64).abs() / y64.abs()).max())  # noqa: E731
    for _ in range(3):  # warm-up of every path at the timed shape
        device_call()
        torch_dev_call()
        ctc_loss(logits, tokens, ml, tl)
    torch_cpu_call()
    assert int(ws[:4].view(torch.int32).item()) == 0
    out = {"B": B, "T": T, "N": N, "V": V, "rounds": a.rounds, "calls_per_round": a.calls, "cpu_threads": torch.get_num_threads(),
           "rel_err_vs_fp64": {"device": rel(nll), "torch_cpu_fp32": rel(torch_cpu_call()), "torch_dev_fp32": rel(torch_dev_call())}}
    times = {"device_ms": [], "api_ms": [], "torch_dev_ms": [], "torch_cpu_ms": []}
    for _ in range(a.rounds):
        times["device_ms"].append(events(device_call))
        times["torch_dev_ms"].append(events(torch_dev_call))
        times["api_ms"].append(host(lambda: ctc_loss(logits, tokens, ml, tl)))
        times["torch_cpu_ms"].append(host(torch_cpu_call))
    for k, v in times.items():
        out[k] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    out["device_us_per_frame"] = out["device_ms"]["median"] * 1e3 / T
    print(json.dumps(out))


if __name__ == "__main__":
    main()
