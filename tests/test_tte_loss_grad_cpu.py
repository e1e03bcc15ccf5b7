"""CPU: the host side of ModelLoss's gradient -- the two exported symbols and their argument validation, the fp64 restatement
tests/tte_loss_grad_ref.py against torch's fp64 autograd of the reference's own lines (modules/loss.py:12-21 as
tests/teacher_forced_ref.py::model_loss; train.py:72-85 calls backward on its first result), and the wrappers' refusals."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import tte_loss_grad_ref as R
from teacher_forced_ref import model_loss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from parrot_tts_amd.loss import ModelLoss  # noqa: E402


def test_grad_symbols_are_exported_and_the_header_is_c99(tmp_path):
    from parrot_tts_amd import _lib, build
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "parrot_hip.h")).read()
    for n in ("parrot_tte_loss_grad_workspace_bytes", "parrot_tte_loss_grad"):
        assert hasattr(raw, n) and n in _lib.SIGNATURES, n
        assert re.search(r"\b" + n + r"\s*\(", hdr), n
    assert "#define PARROT_ABI_VERSION 7" in hdr and "loss.py:5-21" in hdr and "train.py:72-85" in hdr and _lib.ABI_VERSION == 7
    lib = _lib.lib()
    q = lib.parrot_tte_loss_grad_workspace_bytes
    assert q(-1) == 0
    for N in (1, 16, 17, 16384):
        assert q(N) >= lib.parrot_tte_loss_workspace_bytes(N) > 0, N
    # argument validation happens before any HIP call
    buf = (ctypes.c_char * 4096)()
    p, p2, p3 = (ctypes.addressof(buf) + o for o in (0, 1024, 2048))
    assert lib.parrot_tte_loss_grad(None, None, 1, 4, 4, None, None, None, 1, None, None, None, None, None, None, 0, None) == -1
    assert b"null" in lib.parrot_last_error()
    assert lib.parrot_tte_loss_grad(p, p, 1, 4, 4, p, p, p, 1, None, p, None, None, None, p, 1024, None) == -1
    assert b"both gradients null" in lib.parrot_last_error()
    assert lib.parrot_tte_loss_grad(p, p, 1, 4, 4, p2, p, p, 1, None, p, None, p, p3, p, 1024, None) == -1  # grad_logits == logits
    assert b"alias" in lib.parrot_last_error()
    assert lib.parrot_tte_loss_grad(p, p, 0, 4, 4, p2, p, p, 1, None, p, None, p3, None, p, 1024, None) == -1  # empty logits
    assert b"empty" in lib.parrot_last_error()
    gcc = shutil.which("gcc")
    assert gcc is not None
    src = tmp_path / "hdr.c"
    src.write_text('#include "parrot_hip.h"\nsize_t (*ws)(int32_t) = parrot_tte_loss_grad_workspace_bytes;\n'
                   "int (*fn)(const float*, const int64_t*, int32_t, int32_t, int64_t, const float*, const int64_t*, const uint8_t*, int32_t,\n"
                   "          const double*, double*, float*, float*, float*, void*, size_t, void*) = parrot_tte_loss_grad;\n")
    subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def _ragged_batch():
    """B = 4, L = 7, V = 11, S = 6: an ignored tail, one fully ignored row, mask rows of different lengths, durations 0-5."""
    gen = torch.Generator().manual_seed(41)
    V = 11
    out = torch.randn((4, 7, V), generator=gen, dtype=torch.float64) * 2.0
    codes = torch.randint(0, V, (4, 7), generator=gen)
    codes[:, 5:] = V
    codes[2] = V
    batch = {"codes": codes, "src_mask": torch.arange(6)[None, :] < torch.tensor([6, 2, 5, 1])[:, None],
             "duration": torch.randint(0, 6, (4, 6), generator=gen)}
    log_dur = torch.randn((4, 6), generator=gen, dtype=torch.float64)
    return out, log_dur, batch, V


def _torch64(out, log_dur, batch, V, w):
    """model_loss in fp64 with autograd: (losses (3), d (w0 code + w1 dur) / d out, / d log_dur)."""
    x, ld = out.double().clone().requires_grad_(), log_dur.double().clone().requires_grad_()
    loss, code, dur = R.model_loss_typed(x, ld, batch, V)
    (w[0] * code + w[1] * dur).backward()
    return torch.stack([loss, code, dur]).detach().numpy(), x.grad.numpy(), ld.grad.numpy()


@pytest.mark.parametrize("w", [(1.0, 1.0), (0.7, -1.3)])
def test_ref_against_torch_fp64_autograd(w):
    out, log_dur, batch, V = _ragged_batch()
    losses, g_out, g_ld = _torch64(out, log_dur, batch, V, w)
    r = R.tte_loss_and_grad(out.reshape(-1, V).numpy(), batch["codes"].reshape(-1).numpy(), V, log_dur.numpy(), batch["duration"].numpy(),
                            batch["src_mask"].numpy(), w)
    assert (r["n_valid"], r["n_src"], r["n_bad"]) == (15, 14, 0)
    e_l = float(np.abs(r["losses"] - losses).max())
    e_g, e_d = float(np.abs(r["grad_logits"].reshape(g_out.shape) - g_out).max()), float(np.abs(r["grad_log_dur"] - g_ld).max())
    print(f"TTELOSSGRADREF w {w}: losses {losses.tolist()} err {e_l:.2e}, grad_logits err {e_g:.2e}, grad_log_dur err {e_d:.2e}")
    assert e_l <= 1e-12 and e_g <= 1e-12 and e_d <= 1e-12
    ign = (batch["codes"] == V).numpy()
    assert not r["grad_logits"].reshape(g_out.shape)[ign].any() and not g_out[ign].any()  # an ignored position: exactly 0, as torch's
    assert not r["grad_log_dur"][~batch["src_mask"].numpy()].any()
    assert float(np.abs(r["grad_logits"].sum(axis=1)).max()) <= 1e-15 * max(abs(w[0]), 1.0)  # softmax minus one-hot: every row sums to zero


def test_the_typed_model_loss_is_model_loss_in_fp32():
    out, log_dur, batch, V = _ragged_batch()
    grads = []
    for fn in (model_loss, R.model_loss_typed):
        x, ld = out.float().requires_grad_(), log_dur.float().requires_grad_()
        res = fn(x, ld, batch, V)
        res[0].backward()
        grads.append((torch.stack(res).detach(), x.grad, ld.grad))
    assert all(torch.equal(a, b) for a, b in zip(*grads))


def test_ref_nan_edge_cases_as_torch():
    """An all-ignored batch and an empty mask: NaN losses, all-zero gradients -- torch's fp64 autograd does the same."""
    out, log_dur, batch, V = _ragged_batch()
    empty = dict(batch, codes=torch.full_like(batch["codes"], V), src_mask=torch.zeros_like(batch["src_mask"]))
    losses, g_out, g_ld = _torch64(out, log_dur, empty, V, (1.0, 1.0))
    assert np.isnan(losses).all() and not g_out.any() and not g_ld.any()
    r = R.tte_loss_and_grad(out.reshape(-1, V).numpy(), empty["codes"].reshape(-1).numpy(), V, log_dur.numpy(), batch["duration"].numpy(),
                            empty["src_mask"].numpy())
    assert np.isnan(r["losses"]).all() and not r["grad_logits"].any() and not r["grad_log_dur"].any()
    assert (r["n_valid"], r["n_src"]) == (0, 0)
    # one of the two alone: the other loss and its gradient are untouched
    half = dict(batch, codes=empty["codes"])
    losses, g_out, g_ld = _torch64(out, log_dur, half, V, (1.0, 1.0))
    r = R.tte_loss_and_grad(out.reshape(-1, V).numpy(), half["codes"].reshape(-1).numpy(), V, log_dur.numpy(), batch["duration"].numpy(),
                            batch["src_mask"].numpy())
    assert np.isnan(r["losses"][:2]).all() and abs(r["losses"][2] - losses[2]) <= 1e-12 and not r["grad_logits"].any()
    assert float(np.abs(r["grad_log_dur"] - g_ld).max()) <= 1e-12
    # a target out of range (torch: IndexError): the row is NaN, the others are not
    codes = batch["codes"].reshape(-1).numpy().copy()
    codes[3] = V + 3
    r = R.tte_loss_and_grad(out.reshape(-1, V).numpy(), codes, V, log_dur.numpy(), batch["duration"].numpy(), batch["src_mask"].numpy())
    assert r["n_bad"] == 1 and np.isnan(r["grad_logits"][3]).all() and np.isfinite(np.delete(r["grad_logits"], 3, axis=0)).all()


def test_wrappers_refuse_cpu_tensors():
    out, log_dur, batch, V = _ragged_batch()
    loss = ModelLoss({"preprocess": {"hubert_codes": V}})
    with pytest.raises(RuntimeError, match="GPU"):  # no CPU path
        loss.loss_and_grad(out.float(), log_dur.float(), batch)
    with pytest.raises(RuntimeError, match="GPU"):
        loss(out.float().requires_grad_(), log_dur.float().requires_grad_(), batch)
    with pytest.raises(RuntimeError, match="GPU"):
        loss(out.float(), log_dur.float().requires_grad_(), batch)
    with pytest.raises(ValueError, match="Expected input batch_size"):
        loss.loss_and_grad(out.float(), log_dur.float(), dict(batch, codes=batch["codes"][:, :-1]))
