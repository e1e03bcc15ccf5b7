"""CPU: the yardstick of tests/test_gpu_tte_train.py is sound -- the restatement's gradients (tests/tte_train_ref.py) agree with
finite differences of its own fp64 forward, its dropout generator is Philox4x32-10 and keeps at the rate it should -- and the new
entry points are declared, exported and bound."""
import ctypes
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tte_train_ref as TR  # noqa: E402


def _masks(cfg, batch, seed=3, offset=1):
    B, S = batch["phones"].shape
    L = batch["tgt_mask"].shape[1]
    return [torch.from_numpy(TR.dropout_mask(seed, offset, site, n, p))
            for site, (n, p) in enumerate(zip(TR.site_sizes(cfg, B, S, L), TR.site_ps(cfg)))]


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10: zero counter and key, and all-ones."""
    assert int(TR.philox4x32_10_word0(0, 0, 0, 0, 0, 0)) == 0x6627E8D5
    f = 0xFFFFFFFF
    assert int(TR.philox4x32_10_word0(f, f, f, f, f, f)) == 0x408F276D


def test_reference_gradients_agree_with_finite_differences():
    """T3, fp64, with dropout masks in place: d loss / d theta along a random direction per parameter, central differences with
    h = 1e-6: the truncation error is O(h^2) and the rounding error about 1e-16 / h, so 1e-6 relative (and 1e-9 absolute) is ample."""
    cfg, sd, batch = TR.make_case("T3")
    masks = _masks(cfg, batch)
    _, _, g64, _ = TR.loss_and_grads(sd, cfg, batch, torch.float64, masks=masks)
    _, _, g32, _ = TR.loss_and_grads(sd, cfg, batch, torch.float32, masks=masks)
    V = cfg["preprocess"]["hubert_codes"]

    def loss(sdd):
        logits, log_dur = TR.forward(sdd, cfg, batch, masks)
        ld = log_dur.masked_select(batch["src_mask"])
        lt = torch.log(batch["duration"].double() + 1).masked_select(batch["src_mask"])
        return float(torch.nn.functional.cross_entropy(logits.reshape(-1, V), batch["codes"].reshape(-1), ignore_index=V)
                     + torch.nn.functional.mse_loss(ld, lt))

    sd64 = {k: v.double() for k, v in sd.items()}
    gen = torch.Generator().manual_seed(1)
    h = 1e-6
    for k in TR.param_keys(sd):
        u = torch.randn(sd[k].shape, generator=gen, dtype=torch.float64)
        if k == "tok_emb.weight":
            u[0] = 0  # the padding row gets no gradient by definition (nn.Embedding's padding_idx); here it is not even indexed
        up, dn = dict(sd64), dict(sd64)
        up[k], dn[k] = sd64[k] + h * u, sd64[k] - h * u
        fd = (loss(up) - loss(dn)) / (2 * h)
        an = float((g64[k] * u).sum())
        assert abs(fd - an) <= 1e-6 * abs(an) + 1e-9, (k, fd, an)
        # ... and the fp32 run is the same function: within 1e-3 of the fp64 gradient's largest magnitude
        assert float((g32[k].double() - g64[k]).abs().max()) <= 1e-3 * max(float(g64[k].abs().max()), 1e-6), k


def test_keep_rate_of_the_numpy_generator():
    n = 1 << 20
    for p in (0.1, 0.5):
        keep = TR.dropout_mask(42, 7, 1, n, p).mean()
        assert abs(keep - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / n), (p, keep)
    assert TR.dropout_mask(42, 7, 1, 1000, 0.0).all() and not TR.dropout_mask(42, 7, 1, 1000, 1.0).any()
    assert (TR.dropout_mask(42, 7, 1, 4096, 0.5) != TR.dropout_mask(42, 8, 1, 4096, 0.5)).any()
    assert (TR.dropout_mask(42, 7, 1, 4096, 0.5) != TR.dropout_mask(42, 7, 2, 4096, 0.5)).any()


def test_cli_schedule_is_the_reference_formula():
    """train.py:42-50 at steps 0, warm-up and total (and either side of them)."""
    import math
    from parrot_tts_amd.cli.tte_train import cosine_schedule_with_warmup as f
    W, N = 4000, 200000
    assert f(0, W, N) == 0.0 and f(1, W, N) == 1.0 / W and f(W - 1, W, N) == (W - 1) / W
    assert f(W, W, N) == 1.0 and f(N, W, N) == 0.0
    mid = (W + N) // 2
    assert f(mid, W, N) == max(0.0, 0.5 * (1.0 + math.cos(math.pi * 0.5 * 2.0 * (float(mid - W) / float(N - W)))))
    assert f(0, 0, 10) == 1.0  # no warm-up: the cosine from its top


def test_new_entry_points_are_declared_exported_and_bound():
    from parrot_tts_amd import _lib, build
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "parrot_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "parrot_hip_debug.h")).read()
    for name in ("parrot_tte_train_saved_bytes", "parrot_tte_train_workspace_bytes", "parrot_tte_train_forward", "parrot_tte_train_backward"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.SIGNATURES and hasattr(raw, name), name
    assert re.search(r"\bparrot_tte_train_dropout_mask\s*\(", dbg) and "parrot_tte_train_dropout_mask" in _lib.SIGNATURES
    assert hasattr(raw, "parrot_tte_train_dropout_mask")
    # the two structs of device pointers have the header's layout: 15 + 2 x 16 x 12 pointers; the configuration 14 ints + 1 + 3 floats
    assert ctypes.sizeof(_lib.TteDevPtrs) == (15 + 2 * _lib.TTE_TRAIN_MAX_LAYERS * 12) * ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(_lib.TteTrainCfg) == 18 * 4
    assert _lib.lib().parrot_abi_version() == 7
    # sizes need no device: 0 beyond the limits, positive inside
    from parrot_tts_amd.tte_train import TrainableParrot
    cfg, _, _ = TR.make_case("T3")
    c = TrainableParrot(cfg, 40, 0)._cfg()
    assert _lib.lib().parrot_tte_train_saved_bytes(ctypes.byref(c), 1, 3, 3) > 0
    assert _lib.lib().parrot_tte_train_workspace_bytes(ctypes.byref(c), 1, 3, 3) > _lib.lib().parrot_tte_train_saved_bytes(ctypes.byref(c), 1, 3, 3)
    assert _lib.lib().parrot_tte_train_saved_bytes(ctypes.byref(c), 0, 3, 3) == 0
    assert _lib.lib().parrot_tte_train_workspace_bytes(ctypes.byref(c), 1, 3, 0) == 0
