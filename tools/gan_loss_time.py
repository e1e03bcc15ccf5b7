#!/usr/bin/env python3
"""One timing of the vocoder's generator-step adversarial losses with their gradients at the reference trainer's shapes: the 62 terms
(5 period discriminators x 6 feature maps, 3 scale discriminators x 8, and 8 scores) for batch_size rows of segment_size samples
(tests/golden/vocoder_train_config.json: 16 x 8960), the shapes computed from the discriminators' layer constants
(tests/gan_loss_ref.py).  Three ways to the same gradients, all on the device, timed with device events around one whole step,
3 warm-up steps and `--runs` (>= 10) timed ones in alternation, the median reported with the minimum and the maximum:

    torch_eager   loss_gen_s + loss_gen_f + loss_fm_s + loss_fm_f as torch expressions (models.py:279-310), forward + backward
    autograd      parrot_tts_amd.gan_loss.generator_adversarial_loss forward + backward (two device calls)
    fused         generator_adversarial_loss_and_grad (one device call: values and gradients together)

and the last two once more with detach_real=True (no d/d fmap_r written; torch has no such form), and

    raw_fused     parrot_gan_loss itself on a table and buffers built beforehand, 10 calls back to back per timing: the two
                  launches without the Python side (allocation of 116 gradient tensors, the table, the re-nesting)

    python tools/gan_loss_time.py [--runs 20] [--B 16 --segment 8960]   -> one JSON line

The line also carries each path's algorithmic traffic -- every input read once per pass that needs it, every gradient written
once -- over its median time, as a share of the 6.29 TB/s copy ceiling.  The times are of the whole Python call (table building
included), not of one kernel.  There is no threshold."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import gan_loss_ref as R  # noqa: E402
from parrot_tts_amd import _lib, gan_loss  # noqa: E402
from parrot_tts_amd.ops import dptr, stream_ptr  # noqa: E402

COPY_CEILING = 6.29e12  # bytes / s, the measured copy rate of the MI355X


def main():
    with open(os.path.join(ROOT, "tests", "golden", "vocoder_train_config.json")) as f:
        cfg = json.load(f)
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--B", type=int, default=int(cfg["batch_size"]))
    ap.add_argument("--segment", type=int, default=int(cfg["segment_size"]))
    a = ap.parse_args()
    if a.runs < 10:
        raise SystemExit("gan_loss_time: at least 10 timed runs")
    if not torch.cuda.is_available():
        raise SystemExit("gan_loss_time: no GPU; a timing taken elsewhere says nothing about the device")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    mpd, msd = R.mpd_shapes(a.B, a.segment), R.msd_shapes(a.B, a.segment)
    mk = lambda s: torch.randn(s, device=dev).requires_grad_()  # noqa: E731
    fmap_f_r, fmap_f_g = [[mk(s) for s in d] for d in mpd], [[mk(s) for s in d] for d in mpd]
    fmap_s_r, fmap_s_g = [[mk(s) for s in d] for d in msd], [[mk(s) for s in d] for d in msd]
    y_df_hat_g, y_ds_hat_g = [mk(R.score_shape(d[-1])) for d in mpd], [mk(R.score_shape(d[-1])) for d in msd]
    args = (y_df_hat_g, y_ds_hat_g, fmap_f_r, fmap_f_g, fmap_s_r, fmap_s_g)
    leaves = [t for nest in args for d in nest for t in (d if isinstance(d, list) else [d])]
    n_l1 = sum(t.numel() for nest in (fmap_f_g, fmap_s_g) for d in nest for t in d)
    n_sq = sum(t.numel() for t in y_df_hat_g + y_ds_hat_g)

    def clear():
        for t in leaves:
            t.grad = None

    def torch_eager():
        clear()
        fm = lambda fr, fg: 2 * sum(torch.mean(torch.abs(rl - gl)) for dr, dg in zip(fr, fg) for rl, gl in zip(dr, dg))  # noqa: E731
        gl = lambda ys: sum(torch.mean((1 - dg) ** 2) for dg in ys)  # noqa: E731
        (gl(y_ds_hat_g) + gl(y_df_hat_g) + fm(fmap_s_r, fmap_s_g) + fm(fmap_f_r, fmap_f_g)).backward()

    def autograd(detach_real=False):
        clear()
        gan_loss.generator_adversarial_loss(*args, detach_real=detach_real)[0].backward()

    def fused(detach_real=False):
        return gan_loss.generator_adversarial_loss_and_grad(*args, detach_real=detach_real)

    # the C call alone: the table, the outputs and the workspace built once
    ops, flat, c, _ = gan_loss._generator_table(*args, False)
    dense = [t.detach() for t in flat]
    bufs = [torch.empty_like(t) for t in dense]
    terms = (_lib.GanTerm * len(ops))()
    i = 0
    for k, op in enumerate(ops):
        two = op == gan_loss.L1
        terms[k] = _lib.GanTerm(dense[i].data_ptr(), dense[i + 1].data_ptr() if two else 0, bufs[i].data_ptr(), bufs[i + 1].data_ptr() if two else 0,
                                dense[i].numel(), op, 0)
        i += 2 if two else 1
    lib = _lib.lib()
    wts = torch.tensor(c, dtype=torch.float64, device=dev)
    term_out, total = torch.empty(len(ops), dtype=torch.float64, device=dev), torch.empty((), dtype=torch.float32, device=dev)
    n_ws = int(lib.parrot_gan_loss_workspace_bytes(terms, len(ops)))
    ws = torch.empty(n_ws, dtype=torch.uint8, device=dev)
    RAW_CALLS = 10

    def raw_fused():
        for _ in range(RAW_CALLS):
            _lib.check(lib.parrot_gan_loss(terms, len(ops), dptr(wts), 1.0, dptr(term_out), dptr(total), dptr(ws), n_ws, stream_ptr(dev)))

    paths = {"raw_fused": raw_fused, "torch_eager": torch_eager, "autograd": autograd, "fused": fused, "autograd_detach_real": lambda: autograd(True),
             "fused_detach_real": lambda: fused(True)}
    # every input read once per pass (forward; backward), every gradient written once
    fwd, both, one = 8 * n_l1 + 4 * n_sq, 8 * n_l1 + 4 * n_sq, 4 * n_l1 + 4 * n_sq
    traffic = {"raw_fused": fwd + both, "torch_eager": 2 * fwd + both, "autograd": 2 * fwd + both, "fused": fwd + both, "autograd_detach_real": 2 * fwd + one,
               "fused_detach_real": fwd + one}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1)

    for _ in range(3):  # warm-up of every path at the timed shape
        for fn in paths.values():
            fn()
    torch.cuda.synchronize(dev)
    # the three agree: the eager gradients against the fused call's
    torch_eager()
    eager = [t.grad.clone() for t in leaves]
    loss, _, grads = fused()
    flat = [t for nest in grads for d in nest for t in (d if isinstance(d, list) else [d])]
    worst = max(float((x - y).abs().max() / y.abs().max().clamp_min(1e-30)) for x, y in zip(flat, eager))
    out = {"B": a.B, "segment": a.segment, "terms": 62, "l1_elements": n_l1, "square_elements": n_sq, "runs": a.runs, "loss": float(loss),
           "device": torch.cuda.get_device_name(dev), "worst_rel_gradient_distance_to_eager": worst,
           "workspace_bytes": n_ws}
    times = {k: [] for k in paths}
    for _ in range(a.runs):  # in alternation
        for k, fn in paths.items():
            times[k].append(timed(fn))
    for k, v in times.items():
        if k == "raw_fused":
            v = [t / RAW_CALLS for t in v]
        med = statistics.median(v)
        rate = traffic[k] / (med * 1e-3)
        out[k] = {"median_ms": med, "min_ms": min(v), "max_ms": max(v), "algorithmic_bytes": traffic[k], "TB_per_s": rate / 1e12,
                  "share_of_copy_ceiling": rate / COPY_CEILING}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
