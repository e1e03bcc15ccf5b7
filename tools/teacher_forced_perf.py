#!/usr/bin/env python3
"""Teacher-forced TTE forward vs the inference forward on the same B = 64 x S = 64 -> L = 256 batch (full-size model, forced
durations of 4), one after the other in one process, and the HIP ModelLoss on the (64, 256, 1000) logits.

    python tools/teacher_forced_perf.py [--iters 50] [--loss-iters 200]     -> one JSON line

Run under `rocprofv3 --kernel-trace --stats` for the loss kernels' own times (loss_rows_kernel reads N * V * 4 bytes once).  The
loss calls rotate over --loss-copies distinct copies of the logits (6 x 65.5 MB = 393 MB, more than the 256 MiB Infinity Cache), so
that each call reads its logits from HBM rather than from the cache the previous call filled."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from parrot_tts_amd import synth  # noqa: E402
from parrot_tts_amd.loss import ModelLoss  # noqa: E402
from parrot_tts_amd.tte import Parrot  # noqa: E402


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--loss-iters", type=int, default=200)
    ap.add_argument("--loss-copies", type=int, default=6)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = synth.default_tte_config(tempfile.mkdtemp())
    with open(os.path.join(cfg["path"]["root_path"], "speakers.json"), "w") as f:
        json.dump({"a": 0, "b": 1}, f)
    model = Parrot(cfg, 30, 0)
    model.load_state_dict(synth.synth_tte_state_dict(cfg, 30, 2, seed=9, forced_duration=4))
    model = model.eval().to(dev)
    batch = {k: v.to(dev) for k, v in synth.synth_tte_batch(64, 64, 30, 2, seed=6).items()}
    logits, _, mask, _ = model(batch, inference=True)
    tf = dict(batch, duration=model.infer_dense(batch)["dur"], tgt_mask=mask.clone())
    V = cfg["preprocess"]["hubert_codes"]
    tf["codes"] = torch.argmax(logits, -1)
    for _ in range(5):
        model(batch, inference=True)
        model(tf)
    t_inf, t_tf = [], []
    for _ in range(a.iters):  # interleaved: drift hits both alike
        t_inf.append(timed(lambda: model(batch, inference=True), dev))
        t_tf.append(timed(lambda: model(tf), dev))
    loss = ModelLoss(cfg)
    out, _, _, ld = model(tf)
    outs = [out.clone() for _ in range(a.loss_copies)]
    for i in range(5):
        loss(outs[i % len(outs)], ld, tf)
    t_loss = [timed(lambda i=i: loss(outs[i % len(outs)], ld, tf), dev) for i in range(a.loss_iters)]
    N = out.numel() // V
    print(json.dumps({"B": 64, "S": 64, "L": int(out.shape[1]), "V": V, "iters": a.iters,
                      "inference_forward_ms_median": statistics.median(t_inf), "teacher_forced_forward_ms_median": statistics.median(t_tf),
                      "inference_forward_ms_min": min(t_inf), "teacher_forced_forward_ms_min": min(t_tf),
                      "model_loss_call_ms_median": statistics.median(t_loss), "loss_logit_bytes": N * V * 4, "loss_copies": a.loss_copies,
                      "note": "wall time per call incl. the host sync of each call; loss kernel times: rocprofv3 --kernel-trace --stats"}))


if __name__ == "__main__":
    main()
