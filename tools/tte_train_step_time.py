"""Time one TTE training step (forward, ModelLoss, backward) at the reference's training shape -- batch 6 of the full-size model, S = 128
phones and L = 1024 frames per row -- for ``TrainableParrot`` and, beside it on the same card, for torch eager autograd on the
restatement of tests/tte_train_ref.py (the same graph from functional ops, dropout by masks drawn on the device).  A report, not a gate.

Method: host clock around ``--steps`` steps that end in a device synchronise, after ``--warmup`` steps, ``--rounds`` rounds alternating
the two cases; every round's time per step is printed and written to ``--out`` with the library's saved / workspace bytes."""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--S", type=int, default=128)
    ap.add_argument("--L", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import tte_train_ref as TR
    from parrot_tts_amd import _lib, synth
    from parrot_tts_amd.loss import ModelLoss
    from parrot_tts_amd.tte_train import TrainableParrot

    dev = "cuda:0"
    root = tempfile.mkdtemp()
    with open(os.path.join(root, "speakers.json"), "w") as f:
        json.dump({"a": 0, "b": 1}, f)
    cfg = synth.default_tte_config(root)
    vocab, V, B, S, L = 80, cfg["preprocess"]["hubert_codes"], a.batch, a.S, a.L
    sd = synth.synth_tte_state_dict(cfg, vocab, 2, seed=1)
    g = torch.Generator().manual_seed(0)
    dur = torch.full((B, S), L // S, dtype=torch.int64)
    dur[:, 0] += L - int(dur[0].sum())
    batch = {"phones": torch.randint(1, vocab, (B, S), generator=g), "src_mask": torch.ones((B, S), dtype=torch.bool),
             "speaker": torch.randint(0, 2, (B,), generator=g), "duration": dur, "tgt_mask": torch.ones((B, L), dtype=torch.bool),
             "codes": torch.randint(0, V, (B, L), generator=g)}
    batch = {k: v.to(dev) for k, v in batch.items()}
    model = TrainableParrot(cfg, vocab, 0)
    model.load_state_dict(sd)
    model = model.to(dev).train()
    loss_fn = ModelLoss(cfg)
    c = model._cfg()
    sizes = {"saved_bytes": int(_lib.lib().parrot_tte_train_saved_bytes(ctypes.byref(c), B, S, L)),
             "workspace_bytes": int(_lib.lib().parrot_tte_train_workspace_bytes(ctypes.byref(c), B, S, L))}
    tsd = {k: v.to(dev).requires_grad_(k != "pos_emb.pe") for k, v in sd.items()}
    leaves = [tsd[k] for k in TR.param_keys(sd)]
    ns, ps = TR.site_sizes(cfg, B, S, L), TR.site_ps(cfg)

    def ours():
        model.zero_grad(set_to_none=True)
        out, _, _, ld = model(batch)
        loss_fn(out, ld, batch)[0].backward()

    def eager():
        masks = [(torch.rand(n, device=dev) >= p).to(torch.uint8) for n, p in zip(ns, ps)]
        logits, ld = TR.forward(tsd, cfg, batch, masks)
        loss = TR.model_loss(logits, ld, batch, V)[0]
        torch.autograd.grad(loss, leaves)

    res = {"ours_ms": [], "torch_eager_ms": []}
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
    rep = dict(shape={"B": B, "S": S, "L": L}, steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0), **sizes, **res)
    print(json.dumps(rep))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rep, f, indent=1)


if __name__ == "__main__":
    main()
