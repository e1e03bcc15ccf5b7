"""GPU: the TTE's training kernels (csrc/tte_train.h) alone, through the parrot_debug_tte_* entry points, at their tile edges; and
conv_dw's tap-group path, which a weight gradient takes when its partials exceed the workspace bound.

Bit-exact on small-integer data (every sum is exact in fp32 and fp64 alike): the length regulator's backward and the two embedding
gradients.  Within a bound derived from the arithmetic, against fp64 on the same fp32 inputs: the masked softmax with dropout, forward
and backward, and LayerNorm backward.  eps = 2^-24 (half an fp32 ulp, relative) throughout."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tte_train_ref as TR  # noqa: E402
from parrot_tts_amd import _lib  # noqa: E402
from parrot_tts_amd.ops import dptr, stream_ptr  # noqa: E402

DEV = "cuda:0"
EPS = 2.0 ** -24
SEED, OFFSET, SITE = 42, 3, 5


_alive = []


def _d(t):
    """Device pointer of a copy of ``t`` on the GPU; the copy lives until the next ``_call`` has finished."""
    if t is None:
        return dptr(None)
    t = t.to(DEV).contiguous()
    _alive.append(t)
    return dptr(t)


def _call(name, *args):
    with torch.cuda.device(DEV):
        _lib.check(getattr(_lib.lib(), name)(*args, stream_ptr(DEV)))
        torch.cuda.synchronize()
    _alive.clear()


def _ints(gen, shape, lo=-8, hi=9):
    return torch.randint(lo, hi, shape, generator=gen).to(torch.float32)


# ---- bit-exact on small integers --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 70, 300])  # 300: a thread's second channel
def test_length_regulator_backward_is_exact(D):
    g = torch.Generator().manual_seed(D)
    B, S, L = 3, 6, 70
    dur = torch.tensor([[10, 0, 25, 0, 0, 35], [0, 0, 3, 1, 0, 0], [0, 0, 0, 0, 0, 0]])  # fills L; short with empty ends; all empty
    dy, add = _ints(g, (B, L, D)), _ints(g, (B, S, D))
    want = torch.zeros((B, S, D), dtype=torch.float64)
    for b in range(B):
        t = 0
        for s in range(S):
            want[b, s] = dy[b, t: t + int(dur[b, s])].double().sum(dim=0)
            t += int(dur[b, s])
    for with_add in (False, True):
        denc = torch.full((B, S, D), float("nan"), device=DEV)
        cum = torch.empty((B, S + 1), dtype=torch.int32, device=DEV)
        a = add if with_add else None
        _call("parrot_debug_tte_lr_bwd", _d(dy), _d(dur), _d(a), dptr(denc), dptr(cum), B, S, L, D)
        assert torch.equal(denc.cpu().double(), want + (add.double() if with_add else 0))
        assert cum.cpu().tolist() == [[0, 10, 10, 35, 35, 35, 70], [0, 0, 0, 3, 4, 4, 4], [0] * 7]
        if not with_add:  # an empty segment is +0, not a rounding of anything
            assert torch.equal(denc.cpu()[2].view(torch.int32), torch.zeros((S, D), dtype=torch.int32))


@pytest.mark.parametrize("D", [1, 70, 300])  # 300: the second block of channels
def test_embedding_gradients_are_exact(D):
    g = torch.Generator().manual_seed(D + 1)
    V, B, S = 11, 4, 13
    ids = torch.randint(0, V - 2, (B * S,), generator=g)  # rows 9, 10 are never used; id 0 is the padding
    ids[:3] = 0
    dx = _ints(g, (B * S, D))
    want = torch.zeros((V, D), dtype=torch.float64).index_add_(0, ids, dx.double())
    want[0] = 0
    dtab = torch.full((V, D), float("nan"), device=DEV)
    _call("parrot_debug_tte_embed_grad", _d(ids), _d(dx), dptr(dtab), B * S, 1, D, V, 0)
    assert torch.equal(dtab.cpu().double(), want)
    assert torch.equal(dtab.cpu()[[0, 9, 10]].view(torch.int32), torch.zeros((3, D), dtype=torch.int32))  # padding and unused rows: +0
    # the speaker table: one id per batch row, every position of the row counts; no padding row
    spk = torch.tensor([2, 0, 2, 1])
    want = torch.zeros((3, D), dtype=torch.float64).index_add_(0, spk.repeat_interleave(S), dx.double())
    dtab = torch.full((3, D), float("nan"), device=DEV)
    _call("parrot_debug_tte_embed_grad", _d(spk), _d(dx), dptr(dtab), B * S, S, D, 3, -1)
    assert torch.equal(dtab.cpu().double(), want)


# ---- dropout ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_dropout_apply(n):
    g = torch.Generator().manual_seed(n)
    x = torch.randn((n,), generator=g)
    x[0] = float("nan")
    if n > 4:
        x[1], x[2], x[3] = float("inf"), -0.0, 1e-42  # (a denormal stays what it is)
    y = torch.full((n,), 7.0, device=DEV)
    _call("parrot_debug_tte_dropout", _d(x), dptr(y), n, 0.0, SEED, OFFSET, SITE)
    assert torch.equal(y.cpu().view(torch.int32), x.view(torch.int32))  # p = 0 leaves x bit-equal
    x = torch.randn((n,), generator=g)  # (normals from here on: the product of a NaN or a denormal is not pinned to its bits)
    for p in (0.1, 0.5):
        keep = torch.from_numpy(TR.dropout_mask(SEED, OFFSET, SITE, n, p)).bool()
        want = torch.where(keep, x * TR.drop_scale(p, torch.float32), torch.zeros(()))
        _call("parrot_debug_tte_dropout", _d(x), dptr(y), n, p, SEED, OFFSET, SITE)
        assert torch.equal(y.cpu().view(torch.int32), want.view(torch.int32)), p  # a survivor: one fp32 product; the rest +0
    _call("parrot_debug_tte_dropout", _d(x), dptr(y), n, 1.0, SEED, OFFSET, SITE)
    assert torch.equal(y.cpu().view(torch.int32), torch.zeros((n,), dtype=torch.int32))


# ---- masked softmax with dropout --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("T", [1, 64, 65, 130])
def test_softmax_dropout_forward_and_backward(T, p):
    """Forward, relative to the fp64 P of the same fp32 scores: the exponent's argument s - max is rounded once (|s - max| < 16: 8 eps
    of relative error in e), expf 2 eps; the row sum carries its terms' 10 eps and ceil(T / 64) + 6 additions; the quotient 1 eps; the
    dropout's scale is rounded once and multiplied once: 2 eps.  10 + 19 + 1 + 2 = 32 eps.  A masked key is exactly 0, a dropped
    element exactly 0.
    Backward, from the same fp32 P and upstream: g = dP scale (2 eps), A = sum_k |g_k| P_k; the row sum of g_k P_k carries 2 eps A from g
    and ceil(T / 64) + 6 <= 9 additions (FMA: the products are not rounded): 11 eps A, 12 with its own use; d = g - sum adds eps |d|, and the
    product with P eps more: |error| <= eps P (2 |d| + 3 |g| + 12 A)."""
    B, H = 2, 2
    g = torch.Generator().manual_seed(T)
    s = torch.randn((B, H, T, T), generator=g) * 2
    valid = torch.ones((B, T), dtype=torch.bool)
    if T > 1:
        valid[1, T - T // 3:] = False  # a fully masked tail in the second batch row
    n = B * H * T * T
    keep = torch.from_numpy(TR.dropout_mask(SEED, OFFSET, SITE, n, p)).view(B, H, T, T).bool() if p else torch.ones((B, H, T, T), dtype=torch.bool)
    scale = TR.drop_scale(p, torch.float64) if p else torch.ones((), dtype=torch.float64)
    kv = valid.view(B, 1, 1, T).expand(B, H, T, T)
    P64 = torch.softmax(s.double().masked_fill(~kv, float("-inf")), dim=-1)
    P = s.to(DEV).clone()
    pd = torch.full((B, H, T, T), float("nan"), device=DEV)
    _call("parrot_debug_tte_softmax_drop_fwd", dptr(P), dptr(pd), _d(valid.to(torch.uint8)), B, H, T, p, SEED, OFFSET, SITE)
    P, pd = P.cpu(), pd.cpu()
    assert bool(((P.double() - P64).abs() <= 32 * EPS * P64).all()), float(((P.double() - P64).abs() / P64.clamp_min(1e-300)).max() / EPS)
    assert bool((P[~kv] == 0).all()) and bool((pd[~keep] == 0).all())
    assert bool(((pd.double() - P64 * scale * keep).abs() <= 32 * EPS * P64 * scale).all())
    assert torch.equal(pd[keep], (P * TR.drop_scale(p, torch.float32))[keep] if p else P[keep])  # Pd is P's own bits, scaled once
    # backward
    up = torch.randn((B, H, T, T), generator=g)
    g64 = up.double() * scale * keep
    A = (g64.abs() * P.double()).sum(dim=-1, keepdim=True)
    d64 = g64 - (g64 * P.double()).sum(dim=-1, keepdim=True)
    dS = up.to(DEV).clone()
    _call("parrot_debug_tte_softmax_drop_bwd", _d(P), dptr(dS), B, H, T, p, SEED, OFFSET, SITE)
    err = (dS.cpu().double() - P.double() * d64).abs()
    bound = EPS * P.double() * (2 * d64.abs() + 3 * g64.abs() + 12 * A)
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
    assert bool((dS.cpu()[~kv] == 0).all())


# ---- LayerNorm backward -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu_res", [False, True])
@pytest.mark.parametrize("C_", [64, 96, 160])
def test_layernorm_backward(C_, relu_res):
    """mean and rstd (kept by the forward) are fp64 sums rounded once: within half an ulp (+ 1e-6 of it for the fp64 sums).  The
    backward against the fp64 formula evaluated with those same fp32 statistics, on the same fp32 inputs.  With xh = (x - m) r (2 eps),
    g = dy gamma (1 eps), s1 = mean g and s2 = mean g xh summed in fp64 and rounded once (their terms' errors: eps mean|g|, 3 eps
    mean|g xh|), the bracket (g - s1) - xh s2 is off by at most eps (|g| + 1.5 mean|g| + 6 |xh| mean|g xh|) from its inputs and 2 eps of
    its partial results from the two subtractions; the product with r adds eps of the whole (4, 5 and 9 eps on the three terms):
    |error| <= 10 eps r (|g| + mean|g| + |xh| mean|g xh|),
    plus eps of the result when the residual is added.  dy xh: 3 eps, 4 allowed.  Where relu_mask is set and x <= 0: exactly 0."""
    rows = 7
    g = torch.Generator().manual_seed(C_)
    x, dy, res = torch.randn((rows, C_), generator=g) + 0.3, torch.randn((rows, C_), generator=g), torch.randn((rows, C_), generator=g)
    gamma, beta = 1 + 0.1 * torch.randn((C_,), generator=g), 0.1 * torch.randn((C_,), generator=g)
    y, mean, rstd = (torch.full(sh, float("nan"), device=DEV) for sh in ((rows, C_), (rows,), (rows,)))
    _call("parrot_debug_tte_ln_fwd", _d(x), _d(gamma), _d(beta), dptr(y), dptr(mean), dptr(rstd), rows, C_)
    m64 = x.double().mean(dim=1)
    r64 = 1.0 / torch.sqrt(x.double().var(dim=1, unbiased=False) + 1e-5)
    for got, want in ((mean.cpu(), m64), (rstd.cpu(), r64)):
        assert bool(((got.double() - want).abs() <= 0.5 * (1 + 1e-6) * torch.from_numpy(np.spacing(want.abs().float().numpy())).double()).all())
    y64 = torch.nn.functional.layer_norm(x.double(), (C_,), gamma.double(), beta.double())
    assert float((y.cpu().double() - y64).abs().max()) <= 8 * EPS * float(y64.abs().max())
    m, r = mean.cpu().double().unsqueeze(1), rstd.cpu().double().unsqueeze(1)
    xh, gg = (x.double() - m) * r, dy.double() * gamma.double()
    want = r * ((gg - gg.mean(dim=1, keepdim=True)) - xh * (gg * xh).mean(dim=1, keepdim=True))
    bound = 10 * EPS * r * (gg.abs() + gg.abs().mean(dim=1, keepdim=True) + xh.abs() * (gg * xh).abs().mean(dim=1, keepdim=True))
    if relu_res:
        want = want + res.double()
        bound = bound + EPS * want.abs()
        want = torch.where(x > 0, want, torch.zeros((), dtype=torch.float64))
    dx, dyxh = torch.full((rows, C_), float("nan"), device=DEV), torch.full((rows, C_), float("nan"), device=DEV)
    _call("parrot_debug_tte_ln_bwd", _d(dy), _d(x), _d(gamma), dptr(mean), dptr(rstd),
          _d(res) if relu_res else dptr(None), dptr(dx), dptr(dyxh), rows, C_, int(relu_res))
    err = (dx.cpu().double() - want).abs()
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
    if relu_res:
        assert bool((dx.cpu()[x <= 0] == 0).all())
    assert bool(((dyxh.cpu().double() - dy.double() * xh).abs() <= 4 * EPS * (dy.double() * xh).abs()).all())


# ---- the weight gradient, a few taps at a time ------------------------------------------------------------------------------------
def _conv_dw(dY, X, cout, cin, kk, pad, B, T, group):
    lib = _lib.lib()
    n_ws = int(lib.parrot_debug_tte_conv_dw_workspace_bytes(cout, cin, kk, B, T, group))
    assert n_ws == ((B * T + 255) // 256) * group * cout * cin * 4
    ws = torch.empty((n_ws,), dtype=torch.uint8, device=DEV)
    dW = torch.full((cout, cin, kk), float("nan"), device=DEV)
    _call("parrot_debug_tte_conv_dw", dptr(dY), dptr(X), dptr(dW), cout, cin, kk, pad, B, T, group, dptr(ws), n_ws)
    return dW.cpu()


@pytest.mark.parametrize("cout, cin, kk, pad, B, T", [(70, 65, 9, 4, 2, 150), (33, 70, 3, 1, 3, 100), (5, 7, 9, 4, 1, 3)])
def test_weight_gradient_in_tap_groups(cout, cin, kk, pad, B, T):
    """conv_dw with the partial buffer sized for 1, 2 and all taps: B T = 300 is two reduction chunks, the first ending inside batch row
    1; group = 2 on k = 9 is five launches, the last with one tap, each reduced into its own taps of dW.  A tap's arithmetic does not
    depend on its group, so the three results are the same bits; against fp64 (torch.autograd of conv1d) each element is a sum of
    at most 256 fp32 products per chunk accumulated in fp32, the chunks then added in fp64: |error| <= (256 + 1) eps sum |dY| |X|."""
    g = torch.Generator().manual_seed(kk * T)
    dY, X = torch.randn((B, T, cout), generator=g), torch.randn((B, T, cin), generator=g)
    W = torch.zeros((cout, cin, kk), dtype=torch.float64, requires_grad=True)

    def wgrad(dy, x):
        out = torch.nn.functional.conv1d(x.double().transpose(1, 2), W, padding=pad)
        return torch.autograd.grad(out, W, dy.double().transpose(1, 2))[0]

    want, mag = wgrad(dY, X), wgrad(dY.abs(), X.abs())
    dYd, Xd = dY.to(DEV), X.to(DEV)
    got = {grp: _conv_dw(dYd, Xd, cout, cin, kk, pad, B, T, grp) for grp in sorted({1, 2, kk})}
    for grp, dW in got.items():
        err = (dW.double() - want).abs()
        assert bool((err <= 257 * EPS * mag + 1e-30).all()), (grp, float((err / (EPS * mag).clamp_min(1e-300)).max()))
        assert torch.equal(dW, got[kk]), grp


def test_argument_errors():
    lib = _lib.lib()
    x = torch.zeros((8,), device=DEV)
    assert lib.parrot_debug_tte_dropout(dptr(x), dptr(x), 8, 1.5, 0, 0, 0, stream_ptr(DEV)) == -1
    assert lib.parrot_debug_tte_dropout(dptr(x), dptr(None), 8, 0.5, 0, 0, 0, stream_ptr(DEV)) == -1
    assert lib.parrot_debug_tte_conv_dw_workspace_bytes(4, 4, 10, 1, 8, 1) == 0 and lib.parrot_debug_tte_conv_dw_workspace_bytes(4, 4, 9, 1, 8, 10) == 0
    assert lib.parrot_debug_tte_conv_dw(dptr(x), dptr(x), dptr(x), 1, 1, 3, 1, 1, 8, 1, dptr(x), 3, stream_ptr(DEV)) == -1  # workspace too small
    assert lib.parrot_debug_tte_lr_bwd(dptr(x), dptr(x), dptr(None), dptr(x), dptr(x), 1, 0, 8, 1, stream_ptr(DEV)) == -1
