#!/usr/bin/env python3
"""Generate tests/golden/aligner_train_s1.npz, aligner_train_s2.npz and aligner_sampler_order.json by running the REFERENCE's aligner
in training (utils/aligner/model.py under ``model.train()``, the loss of utils/aligner/trainer.py:60-63, the sampler of
utils/aligner/dataset.py), imported at run time from a reference checkout, on the CPU.

Nothing from the reference is copied.  A model fixture holds the seeded state dict (``sd.<key>``), ``mel``, ``tokens`` and the
lengths (tests/aligner_train_ref.make_case), and from the reference module itself in ``.double()``: the train-mode logits, the
gradient of its CTC loss for all 19 parameters (``grad.<key>``), and the BatchNorm buffers after that one step (``after.<key>``).
Its meta records, per tensor, the distance of the reference's own fp32 run from those fp64 values relative to the tensor's
largest entry.  Cross-check while the reference is at hand: tests/aligner_train_ref.py in fp64 against the reference in fp64.

The sampler fixture is the index order the reference's ``BinnedLengthSampler`` yields over three epochs for the lengths and batch
size stored beside it.

    python tools/make_aligner_train_goldens.py [--reference DIR]
"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import aligner_train_ref as TR  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
MAX_BYTES = 1 << 20


def load_reference(ref_dir, name):
    sys.path.insert(0, os.path.join(ref_dir, "utils", "aligner"))  # (dataset.py imports its sibling utils.py by name)
    try:
        spec = importlib.util.spec_from_file_location("ref_aligner_" + name, os.path.join(ref_dir, "utils", "aligner", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.pop(0)
    return mod


def reference_step(ref_model, shape, sd, mel, tokens, ml, tl, dtype):
    B, T, n_mels, V, H, D, N = TR.SHAPES[shape]
    m = ref_model.Aligner(n_mels=n_mels, num_symbols=V, lstm_dim=H, conv_dim=D)
    m.load_state_dict(sd)
    m = m.to(dtype).train()
    logits = m(mel.to(dtype))
    loss = torch.nn.CTCLoss()(logits.transpose(0, 1).log_softmax(2), tokens, ml, tl)
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    after = {k: v.detach().clone() for k, v in m.state_dict().items() if k in TR.BUFFER_KEYS or k.endswith("num_batches_tracked") or k == "step"}
    return logits.detach(), loss.detach(), grads, after


def model_fixture(ref_model, shape, name):
    sd, mel, tokens, ml, tl = TR.make_case(shape)
    l64, loss64, g64, a64 = reference_step(ref_model, shape, sd, mel, tokens, ml, tl, torch.float64)
    l32, loss32, g32, a32 = reference_step(ref_model, shape, sd, mel, tokens, ml, tl, torch.float32)
    r64, rloss, rg, rb = TR.loss_and_grads(sd, mel, tokens, ml, tl, torch.float64)  # the restatement, while the reference is at hand
    assert float((r64 - l64).abs().max()) <= 1e-12 and abs(float(rloss - loss64)) <= 1e-12
    for k in TR.PARAM_KEYS:
        assert float((rg[k] - g64[k]).abs().max()) <= 1e-11 * max(1.0, float(g64[k].abs().max())), k
    for k in TR.BUFFER_KEYS:
        assert float((rb[k] - a64[k]).abs().max()) <= 1e-12, k
    rel = {k: float((g32[k].double() - g64[k]).abs().max() / g64[k].abs().max()) for k in TR.PARAM_KEYS}
    out = {"mel": mel.numpy(), "tokens": tokens.numpy(), "mel_len": ml.numpy(), "tokens_len": tl.numpy(), "logits64": l64.numpy(),
           "loss64": np.array(float(loss64))}
    out.update({"sd." + k: v.numpy() for k, v in sd.items()})
    out.update({"grad." + k: g64[k].numpy() for k in TR.PARAM_KEYS})
    out.update({"after." + k: v.numpy() for k, v in a64.items()})
    meta = {"shape": shape, "dims": list(TR.SHAPES[shape]), "loss64": float(loss64), "loss32": float(loss32),
            "logits_d_ref": float((l32.double() - l64).abs().max()), "grad_rel_d_ref_max": max(rel.values()), "grad_rel_d_ref": rel}
    path = os.path.join(GOLD, name + ".npz")
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **out)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    print(name, size, "bytes; fp32 gradients within", meta["grad_rel_d_ref_max"], "of fp64 relative to each tensor's largest entry")


def sampler_fixture(ref_dataset):
    rng = np.random.Generator(np.random.PCG64(4))
    lens = [int(v) for v in rng.integers(20, 400, size=23)]  # 23 items: three bins of 6 and a tail of 5
    batch_size = 2
    s = ref_dataset.BinnedLengthSampler(mel_lens=lens, batch_size=batch_size, bin_size=3 * batch_size)
    epochs = [[int(i) for i in iter(s)] for _ in range(3)]
    with open(os.path.join(GOLD, "aligner_sampler_order.json"), "w") as f:
        json.dump({"mel_lens": lens, "batch_size": batch_size, "epochs": epochs}, f)
    print("aligner_sampler_order", epochs[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("PARROT_REFERENCE"), help="a checkout of the reference (or $PARROT_REFERENCE)")
    args = ap.parse_args()
    if not args.reference:
        ap.error("give --reference DIR or set PARROT_REFERENCE")
    torch.manual_seed(0)
    ref_model = load_reference(args.reference, "model")
    model_fixture(ref_model, "S1", "aligner_train_s1")
    model_fixture(ref_model, "S2", "aligner_train_s2")
    sampler_fixture(load_reference(args.reference, "dataset"))


if __name__ == "__main__":
    main()
