#!/usr/bin/env python3
"""The aligner at the default config on a B = 8, T = 500 frames, N = 100 tokens batch: wall time of `align` and of its parts, the
recurrence with and without graph capture, and the same work by the CPU restatement (tests/aligner_ref.py) on this machine's CPUs.

    python tools/aligner_perf.py [--iters 20] [--B 8 --T 500 --N 100] [--precision f16x3|bf16x6|f32] [--no-cpu]   -> one JSON line
    python tools/aligner_perf.py --only forward|forward-graph|align --iters 5      only that loop: for a kernel trace

The wall times include one host synchronisation per call.  `forward_graph_ms` replays the forward -- T lstm_step_kernel launches
among some twenty others -- captured once as a graph; a capture that fails is an error, not a missing figure.
`forward_minus_graph_us_per_frame` is the whole forward's host-side saving per frame, NOT the time of a launch: the time per
lstm_step_kernel launch (kernel duration, and start-to-start period of consecutive launches) comes from a kernel trace of
`--only forward` and of `--only forward-graph` (`rocprofv3 --kernel-trace`), as do the shares of the convs, the input
projection, the recurrence and the DP (`--only align`).  No run of this tool on an MI355X is recorded yet: its figures belong in
profiles/aligner.md, which does not exist until then."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import aligner_ref as R  # noqa: E402
from parrot_tts_amd import synth  # noqa: E402
from parrot_tts_amd.aligner import Aligner, align_durations  # noqa: E402


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def med(fn, dev, iters):
    fn()
    return statistics.median(timed(fn, dev) for _ in range(iters))


def capture(model, mel, dev):
    """The forward captured once as a graph (after two runs on a side stream: handle, workspaces and the allocator are warm)."""
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):
            model(mel)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        g.captured = model(mel)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--T", type=int, default=500)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--V", type=int, default=61)
    ap.add_argument("--precision", default=None)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--only", choices=["forward", "forward-graph", "align"], default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = synth.default_aligner_config()
    sd = synth.synth_aligner_state_dict(cfg, a.V, seed=8, gain=14.0)
    model = Aligner(cfg["audio"]["n_mels"], a.V, **cfg["model"], precision=a.precision)
    model.load_state_dict(sd)
    model = model.eval().to(dev)
    rng = np.random.Generator(np.random.PCG64(0))
    mel_len = [a.T] + [int(v) for v in rng.integers(a.T // 2, a.T + 1, size=a.B - 1)]
    tokens_len = [a.N] + [int(v) for v in rng.integers(a.N // 2, a.N + 1, size=a.B - 1)]
    mel_h = synth.synth_aligner_mel(a.B, a.T, cfg["audio"]["n_mels"], mel_len, seed=1)
    tokens_h = torch.from_numpy(rng.integers(1, a.V, size=(a.B, a.N)))
    mel, tokens = mel_h.to(dev), tokens_h.to(dev)
    logits = model(mel)
    pred = model.softmax(logits, mel_len)
    out = {"B": a.B, "T": a.T, "N": a.N, "V": a.V, "iters": a.iters, "precision": model.precision_in_use}
    if a.only in ("forward", "align"):
        fn = (lambda: model(mel)) if a.only == "forward" else (lambda: model.align(mel, mel_len, tokens, tokens_len))
        out[a.only.replace("-", "_") + "_ms"] = med(fn, dev, a.iters)
        print(json.dumps(out))
        return
    if a.only == "forward-graph":
        out["forward_graph_ms"] = med(capture(model, mel, dev).replay, dev, a.iters)
        print(json.dumps(out))
        return
    out["align_ms"] = med(lambda: model.align(mel, mel_len, tokens, tokens_len), dev, a.iters)
    out["forward_ms"] = med(lambda: model(mel), dev, a.iters)
    out["softmax_ms"] = med(lambda: model.softmax(logits, mel_len, check=False), dev, a.iters)
    out["dp_ms"] = med(lambda: align_durations(pred, tokens, mel_len, tokens_len), dev, a.iters)
    out["dp_ms_per_utterance_alone"] = med(lambda: align_durations(pred[:1], tokens[:1], mel_len[:1], tokens_len[:1]), dev, a.iters)
    out["forward_ms_per_frame"] = out["forward_ms"] / a.T
    if not a.no_graph:
        g = capture(model, mel, dev)
        out["forward_graph_ms"] = med(g.replay, dev, a.iters)
        out["graph_equals_plain"] = bool(torch.equal(g.captured, logits))
        out["forward_minus_graph_us_per_frame"] = (out["forward_ms"] - out["forward_graph_ms"]) * 1e3 / a.T
    if not a.no_cpu:
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        with torch.no_grad():
            R.aligner_forward(sd, mel_h[:, :32])
            t0 = time.perf_counter()
            ref_logits, _ = R.aligner_forward(sd, mel_h)
            ref_pred = R.softmax_rows(ref_logits, mel_len)
            out["cpu_forward_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        for b in range(a.B):
            R.dp_durations(tokens_h[b, :tokens_len[b]].numpy(), ref_pred[b, :mel_len[b]].numpy())
        out["cpu_dp_ms"] = (time.perf_counter() - t0) * 1e3
        out["cpu_threads"] = torch.get_num_threads()
        out["cpu_over_gpu"] = (out["cpu_forward_ms"] + out["cpu_dp_ms"]) / out["align_ms"]
        out["cpu_over_gpu_forward"] = out["cpu_forward_ms"] / out["forward_ms"]
    out["note"] = "wall time per call incl. one host sync; kernel times: a kernel trace of --only forward / forward-graph / align"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
