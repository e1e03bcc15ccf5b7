#!/usr/bin/env python3
"""Record what the workspace size queries return into tests/golden/workspace_bytes.json (or the path given), for
tests/test_gpu_voc_workspace.py and tests/test_abi.py: a refactor of a workspace layout must return the same bytes.
    PARROT_HIP_LIB=<library of the commit whose sizes are to be held> python tools/make_workspace_goldens.py [OUT.json]
Default switches (no PARROT_MRF_STREAMS / PARROT_CHUNK_LANES / PARROT_PRECISION in the environment).  The vocoder handles
need a GPU; the length-regulator query does not.
    PARROT_HIP_LIB=... python tools/make_workspace_goldens.py --train [OUT.json]
records parrot_{aligner,tte,voc}_train_{workspace,saved}_bytes into tests/golden/train_workspace_bytes.json instead, each case
with the config it was asked for (tests/test_abi.py rebuilds the structs from the file).  Needs no device."""
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

# ---- the training size queries.  The weight-gradient partial buffer of a layer of k taps of M x K floats over R = B T pairs is
# chunks x max(M K, min(k M K, FIT / chunks)) floats, chunks = ceil(R / 256), FIT = 64 MiB / 4 = 16 777 216 (train_gemm_host.h).
ALIGNER_CFGS = {"default": dict(n_mels=80, num_symbols=50, lstm_dim=512, conv_dim=512, bn_eps=1e-5),
                "small": dict(n_mels=16, num_symbols=30, lstm_dim=32, conv_dim=32, bn_eps=1e-5)}
# (config, B, T); the aligner sizes its buffer for all five taps, no budget.  The last is refused (B T > 13107 x 256): 0 bytes
ALIGNER_TRAIN = [("small", 3, 50), ("default", 1, 2), ("default", 2, 37), ("default", 4, 300), ("default", 16, 1000), ("default", 4096, 1000)]
# The workspace is the larger of the eval forward's (which holds a `saved` region) and the backward's (which holds the partial
# buffer): with the full depth the former wins and the partial rule does not show, so the budget cases use one layer per stack / one
# stage, where the backward's side decides (checked by rebuilding with another budget: these sizes moved, the full-depth ones did not).
_TTE = dict(d_model=256, n_filter_ffn=1024, ffn_k1=9, ffn_k2=1, max_len=3500, enc_layers=4, enc_heads=2, dec_layers=4, dec_heads=2,
            dp_filter=256, dp_kernel=3, vocab=80, n_speaker=1, n_codes=1000)
TTE_CFGS = {"default": _TTE, "shallow": dict(_TTE, enc_layers=1, dec_layers=1),
            "small": dict(_TTE, d_model=64, n_filter_ffn=128, max_len=400, enc_layers=2, dec_layers=2, dp_filter=64, vocab=40, n_speaker=4, n_codes=100)}
# (config, B, S, L).  The largest layer is the FFN's k = 9 conv: M K = 1024 x 256 = 262 144, all taps 2 359 296.
#   7 chunks (B max(S, L) = 1792): 7 x 2 359 296 = 16 515 072 <= FIT: the last size the budget does not cap;
#   8 chunks (2048): FIT / 8 = 2 097 152 < 2 359 296: capped, groups of 8 taps;
#   33 chunks (8320): FIT / 33 = 508 400 < 2 x 262 144: one tap per launch (32 chunks still fit two);  S > L once.
TTE_TRAIN = [("small", 2, 7, 11), ("small", 3, 33, 20), ("default", 6, 128, 1024), ("shallow", 7, 100, 256), ("shallow", 8, 100, 256),
             ("shallow", 16, 100, 520)]
_VOC = dict(num_embeddings=1000, embedding_dim=128, multispkr=1, n_spkr=4, model_in_dim=256, upsample_initial_channel=512, n_stages=5,
            upsample_rates=[5, 4, 4, 2, 2], upsample_kernel_sizes=[11, 8, 8, 4, 4], n_kernels=3, resblock_kernel_sizes=[3, 7, 11], n_dil=3,
            resblock_dilation_sizes=[[1, 3, 5]] * 3, resblock_type=1)
VOC_CFGS = {"default": _VOC,
            "small": dict(_VOC, num_embeddings=100, embedding_dim=16, model_in_dim=32, upsample_initial_channel=64),
            "one_stage": dict(_VOC, multispkr=0, model_in_dim=128, upsample_initial_channel=1024, n_stages=1, upsample_rates=[2],
                              upsample_kernel_sizes=[4], n_kernels=1, resblock_kernel_sizes=[11], n_dil=1, resblock_dilation_sizes=[[1]],
                              resblock_type=2)}
# (config, B, U).  one_stage: the largest layer is the 512-channel k = 11 resblock conv, M K = 262 144, all taps 2 883 584, over B x 2 U
# pairs:  5 chunks (B 2 U = 1200): 5 x 2 883 584 = 14 417 920 <= FIT, not capped;  10 chunks (2400): FIT / 10 < 2 883 584, capped;
# 38 chunks (9600): FIT / 38 = 441 505 < 2 x 262 144: one tap per launch;  75 chunks (19 200): FIT / 75 < M K: one tap per launch and a
# buffer of chunks x M K, beyond the budget.
VOC_TRAIN = [("small", 1, 8), ("small", 3, 37), ("default", 16, 28), ("one_stage", 2, 300), ("one_stage", 4, 300), ("one_stage", 8, 600),
             ("one_stage", 16, 600)]


def train_sizes(lib):
    import ctypes as C
    rec = {"aligner": [], "tte": [], "voc": []}
    for name, B, T in ALIGNER_TRAIN:
        cfg = _lib.AlignerCfg(**ALIGNER_CFGS[name])
        rec["aligner"].append({"cfg": ALIGNER_CFGS[name], "shape": [B, T], "workspace": lib.parrot_aligner_train_workspace_bytes(C.byref(cfg), B, T),
                               "saved": lib.parrot_aligner_train_saved_bytes(C.byref(cfg), B, T)})
    for name, B, S, L in TTE_TRAIN:
        cfg = _lib.TteTrainCfg(tte=_lib.TteCfg(**TTE_CFGS[name]), pad_idx=0, p_enc=0.1, p_dec=0.1, p_dp=0.5)
        rec["tte"].append({"cfg": TTE_CFGS[name], "shape": [B, S, L], "workspace": lib.parrot_tte_train_workspace_bytes(C.byref(cfg), B, S, L),
                           "saved": lib.parrot_tte_train_saved_bytes(C.byref(cfg), B, S, L)})
    for name, B, U in VOC_TRAIN:
        h = VOC_CFGS[name]
        cfg = _lib.VocCfg(**{k: tuple(tuple(r) if isinstance(r, list) else r for r in v) if isinstance(v, list) else v for k, v in h.items()})
        rec["voc"].append({"cfg": h, "shape": [B, U], "workspace": lib.parrot_voc_train_workspace_bytes(C.byref(cfg), B, U),
                           "saved": lib.parrot_voc_train_saved_bytes(C.byref(cfg), B, U)})
    return rec


def handle(h):
    g = CodeGenerator(AttrDict(h))
    g.load_state_dict(synth.synth_voc_state_dict(h, seed=1234, scale=1.0))
    g = g.eval().to("cuda:0")
    g._current_handle(torch.device("cuda:0"))
    return g


def main():
    if "--train" in sys.argv:
        sys.argv.remove("--train")
        out, rec = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "train_workspace_bytes.json"), train_sizes(_lib.lib())
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        return
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
