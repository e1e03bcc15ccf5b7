"""CPU: the host side of the vocoder's GAN losses (parrot_tts_amd.gan_loss over parrot_gan_loss) -- the fp64 restatement
tests/gan_loss_ref.py against torch's fp64 autograd of the plain expressions, the three exported symbols with their argument
validation (all of it before any HIP call: there is no device here), the workspace layout, and the wrappers' refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gan_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from parrot_tts_amd import _lib, gan_loss  # noqa: E402


def _nested(seed, dtype=torch.float64):
    """Two discriminators' feature maps (3 and 2 of them, odd shapes) and scores; one planted a == b element per pair."""
    gen = torch.Generator().manual_seed(seed)
    shapes = [[(2, 3, 7), (2, 5, 4, 3), (2, 1, 9)], [(2, 4, 5), (2, 1, 11)]]
    fr = [[torch.randn(s, generator=gen, dtype=dtype) for s in d] for d in shapes]
    fg = [[torch.randn(s, generator=gen, dtype=dtype) for s in d] for d in shapes]
    for dr, dg in zip(fr, fg):
        for rl, gl in zip(dr, dg):
            gl.reshape(-1)[3] = rl.reshape(-1)[3]
    yr = [torch.randn(2, 9, generator=gen, dtype=dtype), torch.randn(2, 11, generator=gen, dtype=dtype)]
    yg = [torch.randn(2, 9, generator=gen, dtype=dtype), torch.randn(2, 11, generator=gen, dtype=dtype)]
    return fr, fg, yr, yg


def _np(nest):
    return [[t.detach().numpy() for t in d] if isinstance(d, list) else d.detach().numpy() for d in nest]


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


@pytest.mark.parametrize("w", [1.0, -0.7])
def test_ref_against_torch_fp64_autograd(w):
    fr, fg, yr, yg = _nested(5)
    for t in [x for d in fr + fg for x in d] + yr + yg:
        t.requires_grad_()
    # the plain expressions
    fm = 2 * sum(torch.mean(torch.abs(rl - gl)) for dr, dg in zip(fr, fg) for rl, gl in zip(dr, dg))
    gen_terms = [torch.mean((1 - dg) ** 2) for dg in yg]
    disc_r, disc_g = [torch.mean((1 - dr) ** 2) for dr in yr], [torch.mean(dg ** 2) for dg in yg]
    (w * fm).backward()
    assert _rel(R.feature_loss(_np(fr), _np(fg)), fm.item()) <= 1e-12
    g_r, g_g = R.feature_loss_grad(_np(fr), _np(fg), w)
    for d_ref, d in zip(g_r + g_g, fr + fg):
        for got, t in zip(d_ref, d):
            assert _rel(got, t.grad.numpy()) <= 1e-12
            assert got.reshape(-1)[3] == 0.0 and t.grad.reshape(-1)[3] == 0.0  # a == b: exactly 0, as torch's sgn
    loss, ls = R.generator_loss(_np(yg))
    assert _rel(loss, sum(gen_terms).item()) <= 1e-12 and _rel(ls, [t.item() for t in gen_terms]) <= 1e-12
    (w * sum(gen_terms)).backward()
    for got, t in zip(R.generator_loss_grad(_np(yg), w), yg):
        assert _rel(got, t.grad.numpy()) <= 1e-12
        t.grad = None
    loss, rs, gs = R.discriminator_loss(_np(yr), _np(yg))
    assert _rel(loss, (sum(disc_r) + sum(disc_g)).item()) <= 1e-12
    assert _rel(rs, [t.item() for t in disc_r]) <= 1e-12 and _rel(gs, [t.item() for t in disc_g]) <= 1e-12
    (w * (sum(disc_r) + sum(disc_g))).backward()
    g_r, g_g = R.discriminator_loss_grad(_np(yr), _np(yg), w)
    for got, t in zip(g_r + g_g, yr + yg):
        assert _rel(got, t.grad.numpy()) <= 1e-12
    assert np.isnan(R.term(R.L1, np.zeros(0), np.zeros(0))) and bool(torch.isnan(torch.zeros(0).mean()))


def test_reference_shapes_from_the_layer_constants():
    """The 62 terms of a generator step: 5 x 6 + 3 x 8 feature maps and 8 scores; T = 2048 is no multiple of 3, 5, 7 or 11."""
    mpd, msd = R.mpd_shapes(2, 2048), R.msd_shapes(2, 2048)
    assert [len(d) for d in mpd] == [6] * 5 and [len(d) for d in msd] == [8] * 3
    assert mpd[0][0] == (2, 32, 342, 2) and mpd[1][0] == (2, 32, 228, 3) and mpd[4][-1] == (2, 1, 3, 11)
    assert msd[0][0] == (2, 128, 2048) and msd[1][0] == (2, 128, 1025) and msd[2][0] == (2, 128, 513) and msd[0][-1] == (2, 1, 32)
    assert sum(len(d) for d in mpd + msd) + len(mpd) + len(msd) == 62 <= _lib.GAN_MAX_TERMS


@pytest.fixture(scope="module")
def lib():
    from parrot_tts_amd import build
    build.build()
    return _lib.lib()


def _terms(specs):
    """[(op, a, b, grad_a, grad_b, n)] -> a GanTerm array."""
    arr = (_lib.GanTerm * max(len(specs), 1))()
    for k, (op, a, b, ga, gb, n) in enumerate(specs):
        arr[k] = _lib.GanTerm(a, b, ga, gb, n, op, 0)
    return arr


def test_symbols_struct_and_workspace(lib):
    hdr = open(os.path.join(ROOT, "include", "parrot_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("parrot_gan_loss_tile", "parrot_gan_loss_workspace_bytes", "parrot_gan_loss"):
        assert hasattr(raw, n) and n in _lib.SIGNATURES and re.search(r"\b" + n + r"\s*\(", hdr), n
    assert "#define PARROT_ABI_VERSION 7" in hdr and _lib.ABI_VERSION == 7 and lib.parrot_abi_version() == 7
    for name, val in (("L1", _lib.GAN_L1), ("SQ1", _lib.GAN_SQ1), ("SQ0", _lib.GAN_SQ0), ("MAX_TERMS", _lib.GAN_MAX_TERMS),
                      ("GRID_CAP", _lib.GAN_GRID_CAP)):
        assert re.search(rf"#define PARROT_GAN_{name} {val}\b", hdr), name
    assert _lib.GAN_MAX_TERMS >= 64
    assert ctypes.sizeof(_lib.GanTerm) == 48
    tile = lib.parrot_gan_loss_tile()
    assert tile > 0 and tile % 4 == 0
    q = lib.parrot_gan_loss_workspace_bytes
    assert q(None, 0) == 0 and q(_terms([]), 0) == 0 and q(None, 3) == 0
    assert q(_terms([(0, 8, 8, 0, 0, -1)]), 1) == 0
    ns = [1, tile, tile + 1, 0, 5 * tile + 3]
    specs = [(k % 3, 8, 8, 0, 0, n) for k, n in enumerate(ns)]
    base = q(_terms(specs), len(specs))
    assert base > 0 and base == q(_terms(specs[::-1]), len(specs)) == q(_terms(specs[2:] + specs[:2]), len(specs))
    # monotone in the number of tiles: 3 + 97 k tiles of one term
    sizes = [q(_terms([(0, 8, 8, 0, 0, (3 + 97 * k) * tile)]), 1) for k in range(8)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0] >= 8 * 3
    assert q(_terms([(0, 8, 8, 0, 0, 1000 * tile)]), 1) >= 8 * 1000
    # the same tiles in one term or in two: the same partial sums (one more mean)
    assert q(_terms([(0, 8, 8, 0, 0, 64 * tile)] * 2), 2) >= q(_terms([(0, 8, 8, 0, 0, 128 * tile)]), 1)


def test_refusals_happen_before_any_device_call(lib):
    buf = (ctypes.c_char * 4096)()
    p, p2, p3, p4 = (ctypes.addressof(buf) + o for o in (0, 1024, 2048, 3072))
    ws_n = 4096

    def call(specs, K=None, term_out=p3, total=None, n_ws=ws_n):
        return lib.parrot_gan_loss(_terms(specs) if specs is not None else None, len(specs) if K is None else K, None, 1.0, term_out, total, p4, n_ws, None)

    def refused(code, word, *a, **kw):
        assert call(*a, **kw) == code
        msg = lib.parrot_last_error()
        assert msg and word in msg, (msg, word)

    refused(-1, b"null", None, K=2)                                       # a null table with K > 0
    refused(-1, b"unknown op", [(3, p, p2, 0, 0, 4)])
    refused(-1, b"unknown op", [(-1, p, p2, 0, 0, 4)])
    refused(-1, b"negative n", [(0, p, p2, 0, 0, -1)])
    refused(-1, b"null a", [(1, 0, 0, 0, 0, 4)])
    refused(-1, b"null b", [(0, p, 0, 0, 0, 4)])
    refused(-1, b"grad_b on a squares term", [(1, p, 0, 0, p2, 4)])
    refused(-1, b"grad_b on a squares term", [(2, p, 0, 0, p2, 4)])
    refused(-1, b"alias", [(0, p, p2, p, 0, 4)])                          # grad_a == a
    refused(-1, b"alias", [(0, p, p2, p2, 0, 4)])                         # grad_a == b
    refused(-1, b"alias", [(0, p, p2, 0, p2, 4)])                         # grad_b == b
    refused(-1, b"alias", [(0, p, p2, 0, p, 4)])                          # grad_b == a
    refused(-1, b"alias", [(2, p, 0, p, 0, 4)])
    refused(-1, b"neither values", [(0, p, p2, 0, 0, 4)], term_out=None)  # no term_out, no total, no gradient
    refused(-1, b"neither values", [], term_out=None)
    refused(-4, b"workspace", [(0, p, p2, 0, 0, 4)], n_ws=8)
    refused(-4, b"workspace", [(0, p, p2, 0, 0, 4)], term_out=None, total=p3, n_ws=8)
    # the second term is the bad one: the message names it
    refused(-1, b"term 1", [(0, p, p2, 0, 0, 4), (0, p, 0, 0, 0, 4)])


def test_shims_refuse_before_touching_a_device():
    fr, fg, yr, yg = _nested(7, torch.float32)
    with pytest.raises(RuntimeError, match="GPU"):
        gan_loss.feature_loss(fr, fg)
    with pytest.raises(RuntimeError, match="GPU"):
        gan_loss.generator_loss([t.requires_grad_() for t in yg])
    with pytest.raises(RuntimeError, match="GPU"):
        gan_loss.discriminator_loss(yr, yg)
    with pytest.raises(RuntimeError, match="GPU"):
        gan_loss.generator_adversarial_loss(yg, yg, fr, fg, fr, fg)
    with pytest.raises(RuntimeError, match="GPU"):
        gan_loss.discriminator_adversarial_loss_and_grad(yr, yg, yr, yg)
    with pytest.raises(ValueError, match="discriminators"):
        gan_loss.feature_loss(fr, fg[:1])
    with pytest.raises(ValueError, match="feature maps"):
        gan_loss.feature_loss(fr, [fg[0][:2], fg[1]])
    with pytest.raises(ValueError, match="shapes"):
        gan_loss.feature_loss(fr, [fg[0], [fg[1][0], fg[1][1][:, :, :5]]])
    with pytest.raises(ValueError, match="real and 1 generated"):
        gan_loss.discriminator_loss(yr, yg[:1])
    with pytest.raises(ValueError, match="fmap_s_r"):
        gan_loss.generator_adversarial_loss_and_grad(yg, yg, fr, fg, fr, fg[:1])
    with pytest.raises(ValueError, match="y_ds_hat_r"):
        gan_loss.discriminator_adversarial_loss(yr, yg, yr[:1], yg)
    # empty lists: the reference's own values, no device call
    assert gan_loss.feature_loss([], []) == 0 and gan_loss.generator_loss([]) == (0, []) and gan_loss.discriminator_loss([], []) == (0, [], [])
    assert gan_loss.feature_loss([[], []], [[], []]) == 0


def test_dropin_exports_the_reference_names():
    from parrot_tts_amd.dropin.utils.vocoder import models
    for n in ("CodeGenerator", "feature_loss", "generator_loss", "discriminator_loss"):
        assert callable(getattr(models, n)), n
    assert models.feature_loss is gan_loss.feature_loss
