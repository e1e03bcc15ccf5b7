#!/usr/bin/env python3
"""One timing of ModelLoss with its gradient at the benchmark's shape: N = 64 x 256 frames of V = 1000 logits, about 10 % of the
frames ignored, 64 x 60 log-durations.  Two ways to the same gradients, both on the device, both timed with device events around
one call, 3 warm-up calls and `--runs` (>= 10) timed ones in alternation, the median reported with the minimum and the maximum:

    device     parrot_tte_loss_grad (count + duration gradient, rows + logit gradient, reduce), unit weights
    torch_dev  torch's own: F.cross_entropy(ignore_index) + F.mse_loss (fp32) forward, and backward to the logits and log-durations

    python tools/tte_loss_grad_time.py [--runs 20] [--B 64 --L 256 --V 1000 --S 60]   -> one JSON line

The line also carries the algorithmic traffic of the logit pass, 8 N V bytes (the logits read once, the gradient written once), over
each path's median time, and each path's largest normalised distance from the fp64 host run (|delta| n_valid).  The rate is of the
whole call (three launches), not of one kernel.  There is no threshold: this is not a measured hot path."""
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
from parrot_tts_amd.ops import dptr, stream_ptr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--L", type=int, default=256)
    ap.add_argument("--V", type=int, default=1000)
    ap.add_argument("--S", type=int, default=60)
    a = ap.parse_args()
    if a.runs < 10:
        raise SystemExit("tte_loss_grad_time: at least 10 timed runs")
    if not torch.cuda.is_available():
        raise SystemExit("tte_loss_grad_time: no GPU; a timing taken elsewhere says nothing about the device")
    dev = torch.device("cuda:0")
    N, V, n_src = a.B * a.L, a.V, a.B * a.S
    gen = torch.Generator().manual_seed(0)
    logits_h = torch.randn((N, V), generator=gen) * 3.0
    codes_h = torch.randint(0, V, (N,), generator=gen)
    codes_h[torch.rand((N,), generator=gen) < 0.1] = V  # ~10 % ignored
    log_dur_h = torch.randn((n_src,), generator=gen)
    dur_h = torch.randint(0, 6, (n_src,), generator=gen)
    mask_h = torch.rand((n_src,), generator=gen) < 0.8
    logits, codes, log_dur, dur, mask = (t.to(dev) for t in (logits_h, codes_h, log_dur_h, dur_h, mask_h))
    src = mask.to(torch.uint8)
    lib = _lib.lib()
    sums = torch.empty(8, dtype=torch.float64, device=dev)
    losses = torch.empty(3, dtype=torch.float32, device=dev)
    g_logits, g_dur = torch.empty_like(logits), torch.empty_like(log_dur)
    n_ws = int(lib.parrot_tte_loss_grad_workspace_bytes(N))
    ws = torch.empty(n_ws, dtype=torch.uint8, device=dev)
    leaf, leaf_d = logits.clone().requires_grad_(), log_dur.clone().requires_grad_()
    target = torch.log(dur.float() + 1)

    def device_call():
        _lib.check(lib.parrot_tte_loss_grad(dptr(logits), dptr(codes), N, V, V, dptr(log_dur), dptr(dur), dptr(src), n_src, None, dptr(sums),
                                            dptr(losses), dptr(g_logits), dptr(g_dur), dptr(ws), n_ws, stream_ptr(dev)))

    def torch_dev_call():
        leaf.grad, leaf_d.grad = None, None
        loss = F.cross_entropy(leaf, codes, ignore_index=V) + F.mse_loss(leaf_d.masked_select(mask), target.masked_select(mask))
        loss.backward()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    x64 = logits_h.double().requires_grad_()
    F.cross_entropy(x64, codes_h, ignore_index=V).backward()
    n_valid = int((codes_h != V).sum())
    for _ in range(3):  # warm-up of both paths at the timed shape
        device_call()
        torch_dev_call()
    torch.cuda.synchronize(dev)
    assert int(sums[1]) == n_valid and int(sums[5]) == 0
    dist = lambda g: float((g.double().cpu() - x64.grad).abs().max()) * n_valid  # noqa: E731
    out = {"N": N, "V": V, "n_src": n_src, "n_valid": n_valid, "runs": a.runs, "workspace_bytes": n_ws, "algorithmic_bytes": 8 * N * V,
           "loss": [float(v) for v in losses.cpu()], "norm_err_vs_fp64": {"device": dist(g_logits), "torch_dev_fp32": dist(leaf.grad)}}
    times = {"device_ms": [], "torch_dev_ms": []}
    for _ in range(a.runs):  # in alternation
        times["device_ms"].append(timed(device_call))
        times["torch_dev_ms"].append(timed(torch_dev_call))
    for k, v in times.items():
        med = statistics.median(v)
        out[k] = {"median": med, "min": min(v), "max": max(v), "algorithmic_TB_per_s": 8 * N * V / (med * 1e-3) / 1e12}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
