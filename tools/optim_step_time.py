#!/usr/bin/env python3
"""Time the optimiser step alone on the vocoder's default-config parameter sets: the generator's (optim_g) and msd + mpd's (optim_d),
with random gradients.  Three contenders on the same box, interleaved round by round: parrot_tts_amd.optim.FusedAdamW,
torch.optim.AdamW as torch picks it (foreach: what a driver would otherwise call -- the yardstick) and torch.optim.AdamW(fused=True).

    python tools/optim_step_time.py [--rounds 7 --steps 50 --warmup 10] [--out profiles/optim_step_time.json]

Per contender and set: the median over rounds of (ms per step over `steps` back-to-back steps between two device synchronisations),
the min-max spread of the rounds, and the achieved GB/s at 28 bytes per element (read p, g, m, v; write p, m, v) beside the
6.3 TB/s achievable HBM bandwidth of the MI355X."""
import argparse
import itertools
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from parrot_tts_amd import synth  # noqa: E402
from parrot_tts_amd.cli.voc_train import build_models  # noqa: E402
from parrot_tts_amd.optim import FusedAdamW  # noqa: E402
from parrot_tts_amd.vocoder import AttrDict  # noqa: E402

PEAK_GBS = 6300.0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_step_time.json"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    h = AttrDict(synth.default_voc_config())
    torch.manual_seed(0)
    generator, mpd, msd = build_models(h, dev)
    sets = {"generator": list(generator.parameters()), "discriminators": list(itertools.chain(msd.parameters(), mpd.parameters()))}
    makers = {"fused_adamw": lambda ps: FusedAdamW(ps, 2e-4, betas=[0.8, 0.99]),
              "torch_default": lambda ps: torch.optim.AdamW(ps, 2e-4, betas=[0.8, 0.99]),
              "torch_fused": lambda ps: torch.optim.AdamW(ps, 2e-4, betas=[0.8, 0.99], fused=True)}
    result = {"device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "rounds": a.rounds, "steps": a.steps,
              "bytes_per_element": 28, "achievable_gbs": PEAK_GBS, "sets": {}}
    for set_name, params in sets.items():
        n = sum(p.numel() for p in params)
        for p in params:
            p.grad = torch.randn_like(p) * 1e-3
        opts = {k: make(params) for k, make in makers.items()}  # (each keeps its own state; they take turns on the same parameters)
        for o in opts.values():
            for _ in range(a.warmup):
                o.step()
        torch.cuda.synchronize()
        times = {k: [] for k in opts}
        for _ in range(a.rounds):
            for k, o in opts.items():  # interleaved
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    o.step()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) / a.steps * 1e3)
        entry = {"tensors": len(params), "elements": n}
        for k, ts in times.items():
            ts = sorted(ts)
            med = ts[len(ts) // 2]
            entry[k] = {"ms_per_step": med, "min_ms": ts[0], "max_ms": ts[-1], "gb_per_s": 28.0 * n / (med * 1e-3) / 1e9,
                        "fraction_of_achievable": 28.0 * n / (med * 1e-3) / 1e9 / PEAK_GBS}
        result["sets"][set_name] = entry
        for p in params:
            p.grad = None
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
