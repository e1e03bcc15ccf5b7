#!/usr/bin/env python3
"""Record what the workspace size queries return into tests/golden/workspace_bytes.json (or the path given), for
tests/test_gpu_voc_workspace.py and tests/test_abi.py: a refactor of a workspace layout must return the same bytes.
    PARROT_HIP_LIB=<library of the commit whose sizes are to be held> python tools/make_workspace_goldens.py [OUT.json]
Default switches (no PARROT_MRF_STREAMS / PARROT_CHUNK_LANES / PARROT_PRECISION in the environment).  The vocoder handles
need a GPU; the length-regulator query does not."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from parrot_tts_amd import _lib, synth  # noqa: E402
from parrot_tts_amd.vocoder import AttrDict, CodeGenerator  # noqa: E402

DIRECT = [(1, 40), (8, 1024), (8, 1025), (3, 2731)]  # small config; either side of the B x U = 8192 branch-stream rule
CHUNKED = [("small", 2, 32), ("default", 40, 256)]   # (config, B, chunk_units), halo = the receptive field
LENGTH_REGULATOR = [(1, 1, 1, 0), (2, 7, 256, 0), (2, 7, 256, 33), (64, 64, 256, 2048)]  # (B, S, D, L)


def handle(h):
    g = CodeGenerator(AttrDict(h))
    g.load_state_dict(synth.synth_voc_state_dict(h, seed=1234, scale=1.0))
    g = g.eval().to("cuda:0")
    g._current_handle(torch.device("cuda:0"))
    return g


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "workspace_bytes.json")
    lib = _lib.lib()
    gens = {"small": handle(synth.small_voc_config()), "default": handle(synth.default_voc_config())}
    rec = {
        "voc_small": {f"{B}x{U}": lib.parrot_voc_workspace_bytes(gens["small"]._handle, B, U) for B, U in DIRECT},
        "voc_chunked": {f"{c}:{B}x{n}": lib.parrot_voc_chunked_workspace_bytes(gens[c]._handle, B, n, -1) for c, B, n in CHUNKED},
        "length_regulator": {f"{B},{S},{D},{L}": lib.parrot_length_regulator_workspace_bytes(B, S, D, L) for B, S, D, L in LENGTH_REGULATOR},
    }
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
