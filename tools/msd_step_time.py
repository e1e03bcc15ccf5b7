"""Time the two multi-scale-discriminator steps of the vocoder's trainer at the reference's training shape -- the default config,
batch 16, segments of 8960 samples, so 32 rows -- for ``TrainableMultiScaleDiscriminator`` and, beside it on the same card, for torch
eager autograd on a torch-built MSD (the restatement of tests/msd_ref.py: F.conv1d with groups, torch._weight_norm, the hand-written
power iteration, F.avg_pool1d, F.leaky_relu) with the same weights, both in training mode.  A report, not a gate.
  D step: forward on (y, y_hat.detach()), parameter gradients from random gradients at the six scores.
  G step: forward on (y, y_hat), d y_hat from random gradients at the scores and at every map (parameters frozen, as a trainer that
          steps the generator alone would have them).
Then every grouped layer alone, at its shape inside scale 0 (32 rows): forward, data gradient and weight gradient of ours (the debug
entry points) against torch's grouped conv (F.conv1d, torch.nn.grad.conv1d_input, torch.nn.grad.conv1d_weight), with the fill of the
64-row tile (cout / g for forward and weight gradient, cin / g for the data gradient).

Method (tools/mpd_step_time.py's): host clock around ``--steps`` steps that end in a device synchronise, after ``--warmup`` steps,
``--rounds`` rounds alternating the two implementations.  Every round's time per step is printed and written to ``--out`` with the
library's saved / workspace bytes."""
import argparse
import ctypes
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

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
    import msd_ref as MR
    from parrot_tts_amd import _lib, synth
    from parrot_tts_amd.msd_train import TrainableMultiScaleDiscriminator
    from parrot_tts_amd.ops import dptr, stream_ptr

    dev = "cuda:0"
    cfg = synth.default_msd_config()
    B, T = a.batch, a.T
    sd = synth.synth_msd_state_dict(cfg, seed=1234)
    y, y_hat = (t.to(dev) for t in synth.synth_msd_batch(B, T, seed=1235))
    model = TrainableMultiScaleDiscriminator()
    model.load_state_dict(sd)
    model = model.to(dev)
    lib = _lib.lib()
    c = model._cfg()
    sizes = {"saved_bytes": int(lib.parrot_msd_train_saved_bytes(ctypes.byref(c), 2 * B, T)),
             "workspace_bytes": int(lib.parrot_msd_train_workspace_bytes(ctypes.byref(c), 2 * B, T))}
    tsd = {k: v.to(dev) for k, v in sd.items()}
    keys = MR.param_keys(sd)
    with torch.no_grad():
        outs = MR.flat_outputs(*model(y, y_hat))
    ups = [torch.randn(o.shape, device=dev) for o in outs]
    is_score = [o.dim() == 2 for o in outs]
    sc_ups = [u for u, s in zip(ups, is_score) if s]

    def grad_mode(params_on):
        for p in model.parameters():
            p.requires_grad_(params_on)
        for k in keys:
            tsd[k].requires_grad_(params_on)

    def ours_d():
        model.zero_grad(set_to_none=True)
        res = model(y, y_hat.detach())
        torch.autograd.backward([t for pair in zip(res[0], res[1]) for t in pair], sc_ups)

    def eager_d():
        res = MR.forward(tsd, cfg, y, y_hat.detach())
        torch.autograd.grad([t for pair in zip(res[0], res[1]) for t in pair], [tsd[k] for k in keys], sc_ups)
        tsd.update(res[5])  # (the buffers move on, as the module's do)

    def ours_g():
        yh = y_hat.detach().requires_grad_(True)
        torch.autograd.backward(MR.flat_outputs(*model(y, yh)), ups)
        return yh.grad

    def eager_g():
        yh = y_hat.detach().requires_grad_(True)
        res = MR.forward(tsd, cfg, y, yh)
        pairs = [(o, u) for o, u in zip(MR.flat_outputs(*res[:4]), ups) if o.requires_grad]  # (the generated rows')
        tsd.update(res[5])
        return torch.autograd.grad([o for o, _ in pairs], [yh], [u for _, u in pairs])[0]

    def clock(fn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps

    res = {"ours_d_ms": [], "torch_eager_d_ms": [], "ours_g_ms": [], "torch_eager_g_ms": []}
    plan = ((True, (("ours_d_ms", ours_d), ("torch_eager_d_ms", eager_d))), (False, (("ours_g_ms", ours_g), ("torch_eager_g_ms", eager_g))))
    for params_on, fns in plan:
        grad_mode(params_on)
        for _, fn in fns:
            for _ in range(a.warmup):
                fn()
    for _ in range(a.rounds):
        for params_on, fns in plan:
            grad_mode(params_on)
            for name, fn in fns:
                res[name].append(clock(fn, a.steps))

    # ---- the grouped layers alone, at their shapes inside scale 0 ---------------------------------------------------------------
    layers = []
    ch, L, N, k = [1] + cfg["channels"], T, 2 * B, 41
    st = stream_ptr(dev)
    for l in range(1, 6):
        cin, cout, g, s = ch[l], ch[l + 1], cfg["groups"][l], MR.STRIDES[l]
        Lo = (L - 1) // s + 1
        x, w = torch.randn(N, cin, L, device=dev), torch.randn(cout, cin // g, k, device=dev) / (cin // g * k) ** 0.5
        b, dy = torch.randn(cout, device=dev), torch.randn(N, cout, Lo, device=dev)
        yo, dx, dw = torch.empty(N, cout, Lo, device=dev), torch.empty_like(x), torch.empty_like(w)
        n_ws = int(lib.parrot_debug_msd_gconv_dw_workspace_bytes(N, cin, cout, g, k, s, L))
        ws = torch.empty(n_ws, dtype=torch.uint8, device=dev)
        fns = {"ours_fwd": lambda: _lib.check(lib.parrot_debug_msd_gconv_fwd(dptr(x), dptr(w), dptr(b), dptr(yo), N, cin, cout, g, k, s, L, 1, 0.1, st)),
               "torch_fwd": lambda: F.leaky_relu(F.conv1d(x, w, b, s, 20, 1, g), 0.1),
               "ours_dx": lambda: _lib.check(lib.parrot_debug_msd_gconv_dx(dptr(dy), dptr(w), None, dptr(x), 0.1, dptr(dx), N, cin, cout, g, k, s, L, st)),
               "torch_dx": lambda: torch.nn.grad.conv1d_input(x.shape, w, dy, s, 20, 1, g),
               "ours_dw": lambda: _lib.check(lib.parrot_debug_msd_gconv_dw(dptr(dy), dptr(x), dptr(dw), N, cin, cout, g, k, s, L, dptr(ws), n_ws, st)),
               "torch_dw": lambda: torch.nn.grad.conv1d_weight(x, w.shape, dy, s, 20, 1, g)}
        row = {"layer": f"convs[{l}] {cin}->{cout} g{g} s{s}", "L_in": L, "L_out": Lo, "fill_fwd_dw": min(1.0, cout // g / 64),
               "fill_dx": min(1.0, cin // g / 64)}
        for name, fn in fns.items():
            for _ in range(a.warmup):
                fn()
            row[name + "_ms"] = min(clock(fn, a.steps) for _ in range(a.rounds))
        layers.append(row)
        print(json.dumps(row))
        L = Lo
    rep = dict(shape={"B": B, "T": T, "rows": 2 * B}, steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0), **sizes, **res,
               grouped_layers=layers)
    print(json.dumps({k: v for k, v in rep.items() if k != "grouped_layers"}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rep, f, indent=1)


if __name__ == "__main__":
    main()
