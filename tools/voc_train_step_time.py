"""Time one generator training step (forward plus backward from a gradient at the waveform) at the reference's training shape --
the default config, batch 16, U = 28 units per row (segment_size 8960 / code_hop_size 320) -- for ``TrainableCodeGenerator`` and,
beside it on the same card, for torch eager autograd on the restatement of tests/voc_train_ref.py (the same graph from functional
ops, weight norm by torch._weight_norm).  A report, not a gate.

Method: host clock around ``--steps`` steps that end in a device synchronise, after ``--warmup`` steps, ``--rounds`` rounds alternating
the two cases; ours is also timed as forward alone and backward alone.  Every round's time per step is printed and written to
``--out`` with the library's saved / workspace bytes."""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--U", type=int, default=28)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import voc_train_ref as VR
    from parrot_tts_amd import _lib, synth
    from parrot_tts_amd.vocoder_train import TrainableCodeGenerator

    dev = "cuda:0"
    h = synth.default_voc_config()
    B, U = a.batch, a.U
    sd = synth.synth_voc_state_dict(h, seed=1234)
    batch = {k: v.to(dev) for k, v in synth.synth_voc_batch(B, U, h, seed=1234).items()}
    model = TrainableCodeGenerator(h)
    model.load_state_dict(sd)
    model = model.to(dev).train()
    c = model._cfg()
    sizes = {"saved_bytes": int(_lib.lib().parrot_voc_train_saved_bytes(ctypes.byref(c), B, U)),
             "workspace_bytes": int(_lib.lib().parrot_voc_train_workspace_bytes(ctypes.byref(c), B, U))}
    up = torch.randn((B, 1, model.out_samples(U)), device=dev)
    tsd = {k: v.to(dev).requires_grad_(True) for k, v in sd.items()}
    leaves = list(tsd.values())

    def ours():
        model.zero_grad(set_to_none=True)
        model(**batch).backward(up)

    def eager():
        wav, _ = VR.forward(tsd, h, batch)
        torch.autograd.grad(wav, leaves, up)

    res = {"ours_ms": [], "torch_eager_ms": [], "ours_forward_ms": [], "ours_backward_ms": []}
    for fn in (ours, eager):
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, fn in (("ours_ms", ours), ("torch_eager_ms", eager)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            torch.cuda.synchronize()
            res[name].append(1e3 * (time.perf_counter() - t0) / a.steps)
        fwd = bwd = 0.0
        for _ in range(a.steps):
            model.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            wav = model(**batch)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            wav.backward(up)
            torch.cuda.synchronize()
            fwd, bwd = fwd + t1 - t0, bwd + time.perf_counter() - t1
        res["ours_forward_ms"].append(1e3 * fwd / a.steps)
        res["ours_backward_ms"].append(1e3 * bwd / a.steps)
    rep = dict(shape={"B": B, "U": U, "samples": model.out_samples(U)}, steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0),
               **sizes, **res)
    print(json.dumps(rep))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rep, f, indent=1)


if __name__ == "__main__":
    main()
