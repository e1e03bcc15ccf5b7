"""Time the two multi-period-discriminator steps of the vocoder's trainer at the reference's training shape -- the default config,
batch 16, segments of 8960 samples, so 32 rows -- for ``TrainableMultiPeriodDiscriminator`` and, beside it on the same card, for torch
eager autograd on a torch-built MPD (the restatement of tests/mpd_ref.py: F.pad, torch._weight_norm, F.conv2d, F.leaky_relu) with the
same weights.  A report, not a gate.
  D step: forward on (y, y_hat.detach()), parameter gradients from random gradients at the ten scores.
  G step: forward on (y, y_hat), d y_hat from random gradients at the scores and at every map (parameters frozen, as a trainer that
          steps the generator alone would have them).

Method (tools/voc_train_step_time.py's): host clock around ``--steps`` steps that end in a device synchronise, after ``--warmup``
steps, ``--rounds`` rounds alternating the two implementations.  Every round's time per step is printed and written to ``--out`` with
the library's saved / workspace bytes."""
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
    ap.add_argument("--T", type=int, default=8960)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import mpd_ref as MR
    from parrot_tts_amd import _lib, synth
    from parrot_tts_amd.discriminator_train import TrainableMultiPeriodDiscriminator

    dev = "cuda:0"
    cfg = synth.default_mpd_config()
    B, T = a.batch, a.T
    sd = synth.synth_mpd_state_dict(cfg, seed=1234)
    y, y_hat = (t.to(dev) for t in synth.synth_mpd_batch(B, T, seed=1235))
    model = TrainableMultiPeriodDiscriminator()
    model.load_state_dict(sd)
    model = model.to(dev)
    c = model._cfg()
    sizes = {"saved_bytes": int(_lib.lib().parrot_mpd_train_saved_bytes(ctypes.byref(c), 2 * B, T)),
             "workspace_bytes": int(_lib.lib().parrot_mpd_train_workspace_bytes(ctypes.byref(c), 2 * B, T))}
    tsd = {k: v.to(dev) for k, v in sd.items()}
    with torch.no_grad():
        outs = MR.flat_outputs(*model(y, y_hat))
    ups = [torch.randn(o.shape, device=dev) for o in outs]
    is_score = [o.dim() == 2 for o in outs]
    sc_ups = [u for u, s in zip(ups, is_score) if s]

    def grad_mode(params_on):
        for p in model.parameters():
            p.requires_grad_(params_on)
        for v in tsd.values():
            v.requires_grad_(params_on)

    def ours_d():
        model.zero_grad(set_to_none=True)
        res = model(y, y_hat.detach())
        torch.autograd.backward([t for pair in zip(res[0], res[1]) for t in pair], sc_ups)

    def eager_d():
        res = MR.forward(tsd, cfg, y, y_hat.detach())
        torch.autograd.grad([t for pair in zip(res[0], res[1]) for t in pair], list(tsd.values()), sc_ups)

    def ours_g():
        yh = y_hat.detach().requires_grad_(True)
        torch.autograd.backward(MR.flat_outputs(*model(y, yh)), ups)
        return yh.grad

    def eager_g():
        yh = y_hat.detach().requires_grad_(True)
        pairs = [(o, u) for o, u in zip(MR.flat_outputs(*MR.forward(tsd, cfg, y, yh)[:4]), ups) if o.requires_grad]  # (the generated rows')
        return torch.autograd.grad([o for o, _ in pairs], [yh], [u for _, u in pairs])[0]

    res = {"ours_d_ms": [], "torch_eager_d_ms": [], "ours_g_ms": [], "torch_eager_g_ms": []}
    plan = ((True, (("ours_d_ms", ours_d), ("torch_eager_d_ms", eager_d))), (False, (("ours_g_ms", ours_g), ("torch_eager_g_ms", eager_g))))
    for params_on, fns in plan:
        grad_mode(params_on)
        for _, fn in fns:
            for _ in range(a.warmup):
                fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for params_on, fns in plan:
            grad_mode(params_on)
            for name, fn in fns:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    fn()
                torch.cuda.synchronize()
                res[name].append(1e3 * (time.perf_counter() - t0) / a.steps)
    rep = dict(shape={"B": B, "T": T, "rows": 2 * B}, steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0), **sizes, **res)
    print(json.dumps(rep))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rep, f, indent=1)


if __name__ == "__main__":
    main()
