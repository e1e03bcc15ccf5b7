#!/usr/bin/env python3
"""Generate tests/golden/msd_default.npz by running the REFERENCE's own ``MultiScaleDiscriminator`` (utils/vocoder/models.py, imported
from the checkout given with --reference; CPU, fp32, one thread) in TRAIN mode under ``no_grad`` on the seeded default-config state
dict and a seeded pair of waveforms (B = 1, T = 400).  Train mode is what a training step runs: every call of the spectral-normed
discriminator 0 starts with a power iteration, so its real and generated rows see different sigmas and its buffers move.

Nothing of the reference is copied.  The fixture holds the two inputs, the six score tensors, per feature map its shape and its fp64
sum and sum of magnitudes, the updated ``weight_u`` / ``weight_v`` of discriminator 0, the list of state-dict keys with their shapes,
and a sha256 digest of the state dict: the weights themselves (118 MB) come back from the seed.

    python tools/make_msd_goldens.py --reference /path/to/reference
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from parrot_tts_amd import synth  # noqa: E402

SEED_W, SEED_IN, B, T = 1234, 1235, 1, 400


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="a checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "msd_default.npz"))
    a = ap.parse_args()
    # the vocoder directory first: its bare `utils.py` must win over the namespace package <reference>/utils
    sys.path.insert(0, os.path.join(a.reference, "utils", "vocoder"))
    import models as ref_models  # noqa
    torch.set_num_threads(1)
    cfg = synth.default_msd_config()
    sd = synth.synth_msd_state_dict(cfg, seed=SEED_W)
    y, y_hat = synth.synth_msd_batch(B, T, seed=SEED_IN)
    msd = ref_models.MultiScaleDiscriminator()
    res = msd.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert list(msd.state_dict()) == list(sd), "key order"
    msd.train()
    with torch.no_grad():
        y_d_rs, y_d_gs, fmap_rs, fmap_gs = msd(y, y_hat)
    after = msd.state_dict()
    out = {"y": y.numpy(), "y_hat": y_hat.numpy(), "digest": np.array(synth.state_digest(sd)), "seeds": np.array([SEED_W, SEED_IN]),
           "keys": np.array(list(sd)), "shapes": np.array([",".join(str(d) for d in v.shape) for v in sd.values()])}
    for i in range(cfg["n_scales"]):
        out[f"score_r{i}"], out[f"score_g{i}"] = y_d_rs[i].numpy(), y_d_gs[i].numpy()
        for l in range(8):
            for tag, m in (("r", fmap_rs[i][l]), ("g", fmap_gs[i][l])):
                out[f"map_{tag}{i}_{l}_shape"] = np.array(m.shape, dtype=np.int64)
                out[f"map_{tag}{i}_{l}_sums"] = np.array([float(m.double().sum()), float(m.double().abs().sum())], dtype=np.float64)
    n_buf = moved = 0
    for k, v in after.items():
        if k.startswith("discriminators.0.") and (k.endswith("weight_u") or k.endswith("weight_v")):
            moved += int(not torch.equal(v, sd[k]))
            out["after:" + k] = v.numpy().copy()
            n_buf += 1
    assert n_buf == 16 and moved >= 15  # (train mode moved them; conv_post's weight_u is one number, +1 or -1)
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
