"""CPU: the host side of the CTC gradient -- the two exported symbols and their argument validation, the fp64 restatement
tests/ctc_grad_ref.py against torch's fp64 autograd of the reference trainer's own lines (utils/aligner/trainer.py:60-71) and
against central differences where torch's CPU backward is off (a row whose last token is the blank), the reduction weights, and
the wrappers' refusals."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctc_grad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from parrot_tts_amd import aligner as A  # noqa: E402


def test_grad_symbols_are_exported_and_the_header_is_c99(tmp_path):
    from parrot_tts_amd import _lib, build
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "parrot_hip.h")).read()
    for n in ("parrot_ctc_grad_workspace_bytes", "parrot_ctc_loss_grad"):
        assert hasattr(raw, n) and n in _lib.SIGNATURES, n
        assert re.search(r"\b" + n + r"\s*\(", hdr), n
    assert "#define PARROT_ABI_VERSION 7" in hdr and "trainer.py:60-71" in hdr and _lib.ABI_VERSION == 7
    lib = _lib.lib()
    q = lib.parrot_ctc_grad_workspace_bytes
    assert q(1, 10, 21, 2049) == 0 and q(1, 32769, 21, 4) == 0 and q(0, 10, 21, 4) == 0
    for B, T, V, N in ((2, 10, 21, 7), (3, 2300, 21, 2048), (16, 800, 50, 100)):
        assert q(B, T, V, N) >= 256 + B * T * 8 + B * T * (2 * N + 1) * 8, (B, T, V, N)
    big = q(1, 32768, 50, 2048)  # 1 GiB of alpha: no 32-bit product anywhere
    assert 256 + 32768 * 8 + 32768 * 4097 * 8 <= big < 2 ** 31
    assert q(65535, 32768, 50, 2048) >= 65535 * 32768 * 4097 * 8  # the largest shape the entry point takes
    # argument validation happens before any HIP call
    assert lib.parrot_ctc_loss_grad(None, None, None, None, 1, 1, 1, 1, None, 0, None, None, None, 0, None) == -1
    assert b"null" in lib.parrot_last_error()
    gcc = shutil.which("gcc")
    assert gcc is not None
    src = tmp_path / "hdr.c"
    src.write_text('#include "parrot_hip.h"\nsize_t (*ws)(int32_t, int32_t, int32_t, int32_t) = parrot_ctc_grad_workspace_bytes;\n'
                   "int (*fn)(const float*, const int64_t*, const int32_t*, const int32_t*, int32_t, int32_t, int32_t, int32_t, const double*,\n"
                   "          int32_t, double*, float*, void*, size_t, void*) = parrot_ctc_loss_grad;\n")
    subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def _torch64(logits, tokens, ml, tl, w=None, reduction="none"):
    """The trainer's own lines in fp64 with autograd: (loss, d (w . loss) / d logits)."""
    x = logits.double().clone().requires_grad_()
    loss = F.ctc_loss(x.transpose(0, 1).log_softmax(2), tokens, torch.tensor(ml), torch.tensor(tl), reduction=reduction)
    loss.backward(w if w is not None else torch.ones_like(loss))
    return loss.detach(), x.grad


def _ragged_batch():
    gen = torch.Generator().manual_seed(31)
    logits = torch.randn((4, 14, 9), generator=gen, dtype=torch.float64) * 2.0
    tokens = torch.tensor([[3, 5, 5, 7, 2], [4, 4, 4, 4, 4], [4, 0, 6, 1, 1], [2, 1, 1, 1, 1]])
    # a doubled token; an all-equal row (four 4s in 12 frames); a blank label that is not last; N_b = T_b = 1
    return logits, tokens, [14, 12, 10, 1], [5, 4, 4, 1]


def test_ref_against_torch_fp64_autograd():
    logits, tokens, ml, tl = _ragged_batch()
    w = torch.tensor([0.7, -1.3, 2.0, -0.4], dtype=torch.float64)  # both signs
    nll, grad = _torch64(logits, tokens, ml, tl, w)
    for b in range(4):
        n, g = R.ctc_nll_and_grad(logits[b, :ml[b]].numpy(), tokens[b, :tl[b]].numpy(), w[b].item())
        assert R.ctc_nll(logits[b, :ml[b]].numpy(), tokens[b, :tl[b]].numpy()) == n
        e_n, e_g = abs(n - nll[b].item()), float(np.abs(g - grad[b, :ml[b]].numpy()).max())
        print(f"CTCGRADREF row {b}: nll {n:.6f} err {e_n:.2e}, grad err {e_g:.2e}")
        assert e_n <= 1e-12 and e_g <= 1e-12, b
        assert float(np.abs(g.sum(axis=1)).max()) <= 1e-12  # softmax minus occupancy: every frame sums to zero
    # a row without a path: +inf and NaN
    n, g = R.ctc_nll_and_grad(logits[0, :5].numpy(), tokens[0].numpy())
    assert n == np.inf and np.isnan(g).all()


def test_ref_blank_last_against_central_differences():
    """The case torch's CPU backward gets wrong (it assigns the last token's term at the last frame, and so drops the final blank
    state's when that token is the blank): the restatement is held to central differences of its own nll instead."""
    x = (torch.randn((10, 9), generator=torch.Generator().manual_seed(32), dtype=torch.float64) * 2.0).numpy()
    tokens = np.array([4, 0, 6, 0])
    _, g = R.ctc_nll_and_grad(x, tokens)
    h, scale = 1e-6, float(np.abs(g).max())
    worst = 0.0
    for t in range(x.shape[0]):
        for v in range(x.shape[1]):
            hi, lo = x.copy(), x.copy()
            hi[t, v] += h
            lo[t, v] -= h
            worst = max(worst, abs((R.ctc_nll(hi, tokens) - R.ctc_nll(lo, tokens)) / (2 * h) - g[t, v]))
    print(f"CTCGRADREF blank-last: worst distance from central differences {worst:.2e}, largest gradient {scale:.3f}")
    assert worst <= 1e-5 * scale
    _, g_torch = _torch64(torch.from_numpy(x)[None], torch.from_numpy(tokens)[None], [10], [4])
    assert float(np.abs(g_torch[0].numpy() - g).max()) > 1e-3  # (torch differs there: the reason this test exists)


@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_reduction_weights_reproduce_torchs_gradients(reduction):
    logits, tokens, ml, tl = _ragged_batch()
    w = A.ctc_reduction_weights(torch.tensor(tl), reduction)
    assert w.dtype == torch.float64 and tuple(w.shape) == (4,)
    want = torch.ones(4, dtype=torch.float64) if reduction != "mean" else 1.0 / (torch.tensor(tl, dtype=torch.float64) * 4)
    assert bool(((w - want).abs() <= torch.from_numpy(np.spacing(want.numpy()))).all())
    _, g_red = _torch64(logits, tokens, ml, tl, reduction=reduction)       # torch's own reduction
    _, g_w = _torch64(logits, tokens, ml, tl, w)                           # reduction='none' weighted by the helper
    if reduction == "mean":
        assert bool(((g_red - g_w).abs() <= torch.from_numpy(np.spacing(g_red.abs().numpy()))).all())  # 1 ulp of fp64
    else:
        assert torch.equal(g_red, g_w)
    assert torch.equal(A.ctc_reduction_weights(torch.tensor([0, 3]), "mean"), torch.tensor([0.5, 1 / 6], dtype=torch.float64))  # max(N_b, 1)


def test_wrappers_refuse_what_they_do_not_compute():
    logits, tokens, ml, tl = _ragged_batch()
    x = logits.float()
    for fn in (A.ctc_loss_and_grad, A.ctc_loss_trainable):
        with pytest.raises(RuntimeError, match="GPU"):  # no CPU path
            fn(x, tokens, ml, tl)
        with pytest.raises(ValueError, match="reduction"):
            fn(x, tokens, ml, tl, reduction="batchmean")
    with pytest.raises(RuntimeError, match="GPU"):
        A.CTCLoss()(x.transpose(0, 1), tokens, ml, tl)
    with pytest.raises(ValueError, match="blank"):
        A.CTCLoss(blank=1)
    with pytest.raises(ValueError, match="reduction"):
        A.CTCLoss(reduction="batchmean")
    with pytest.raises(NotImplementedError, match="1-D"):
        A.CTCLoss()(x.transpose(0, 1), torch.cat([tokens[b, :tl[b]] for b in range(4)]), ml, tl)
    with pytest.raises(NotImplementedError, match="batched"):
        A.CTCLoss()(x[0], tokens[0], ml[:1], tl[:1])
    loss = A.CTCLoss(reduction="sum", zero_infinity=True)
    assert (loss.blank, loss.reduction, loss.zero_infinity) == (0, "sum", True)
