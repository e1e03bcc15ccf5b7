"""GPU: the pieces of the vocoder's training alone, through the debug entry points (include/parrot_hip_debug.h): one transposed or
dilated conv of the training path -- forward, data gradient, weight gradient -- the weight norm, and the embedding scatters.

Convs: small-integer data (|x| <= 3, |w| <= 2), on which every fp32 product and every sum, in any order, is exact (the largest sum
here is below 65 x 11 x 6 x 3 x 65 < 2^24), so the comparison with torch's own conv in fp64 on the CPU is equality.
Weight norm: on normals, against the fp64 formula within a bound derived at each check."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from parrot_tts_amd import _lib  # noqa: E402
from parrot_tts_amd.ops import dptr, stream_ptr  # noqa: E402

DEV = "cuda:0"


def _ints(shape, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-hi, hi + 1, shape, generator=g).to(torch.float32)


def _conv_case(B, cin, cout, k, dil, u, transposed, T, seed):
    """-> x, w, bias, dy (integers) and the fp64 results (y, dx, dw) of torch's conv on the CPU."""
    x = _ints((B, cin, T), 3, seed)
    w = _ints((cin, cout, k) if transposed else (cout, cin, k), 2, seed + 1)
    bias = _ints((cout,), 3, seed + 2)
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    if transposed:
        y = F.conv_transpose1d(xd, wd, bias.double(), stride=u, padding=(k - u) // 2)
    else:
        y = F.conv1d(xd, wd, bias.double(), padding=dil * (k - 1) // 2, dilation=dil)
    dy = _ints(tuple(y.shape), 3, seed + 3)
    dx, dw = torch.autograd.grad(y, [xd, wd], dy.double())
    return x, w, bias, dy, y.detach(), dx, dw


def _run_conv(B, cin, cout, k, dil, u, transposed, T, seed=0):
    lib = _lib.lib()
    x, w, bias, dy, y64, dx64, dw64 = _conv_case(B, cin, cout, k, dil, u, transposed, T, seed)
    xg, wg, bg, dyg = (t.to(DEV) for t in (x, w, bias, dy))
    y = torch.full(tuple(y64.shape), float("nan"), device=DEV)
    dx = torch.full(tuple(x.shape), float("nan"), device=DEV)
    dw = torch.full(tuple(w.shape), float("nan"), device=DEV)
    n_ws = int(lib.parrot_debug_voc_conv_dw_workspace_bytes(B, cin, cout, k, T))
    assert n_ws > 0
    ws = torch.empty(n_ws, dtype=torch.uint8, device=DEV)
    args = (B, cin, cout, k, dil, u, int(transposed), T)
    with torch.cuda.device(DEV):
        _lib.check(lib.parrot_debug_voc_conv_fwd(dptr(xg), dptr(wg), dptr(bg), dptr(y), *args, stream_ptr(DEV)))
        _lib.check(lib.parrot_debug_voc_conv_dx(dptr(dyg), dptr(wg), dptr(dx), *args, stream_ptr(DEV)))
        _lib.check(lib.parrot_debug_voc_conv_dw(dptr(dyg), dptr(xg), dptr(dw), *args, dptr(ws), n_ws, stream_ptr(DEV)))
    assert torch.equal(y.cpu().double(), y64), "forward"
    assert torch.equal(dx.cpu().double(), dx64), "data gradient"
    assert torch.equal(dw.cpu().double(), dw64), "weight gradient"


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [1, 13, 65])
@pytest.mark.parametrize("cin,cout", [(65, 33), (4, 2)])
@pytest.mark.parametrize("u,k", [(2, 4), (5, 11), (2, 5), (4, 9)])
def test_transposed_conv_forward_and_both_gradients(u, k, cin, cout, T, B):
    """(2, 5) and (4, 9) have odd k - u: T u + 1 samples, and the last one is a real sample of the strided operand."""
    _run_conv(B, cin, cout, k, 1, u, True, T, seed=u * 100 + k)


@pytest.mark.parametrize("C_", [1, 16, 65])
@pytest.mark.parametrize("k,d,T", [(11, 5, 7), (11, 5, 64), (11, 5, 65), (3, 1, 7), (3, 1, 65)])
def test_dilated_conv_forward_and_both_gradients(k, d, T, C_):
    """k = 11, d = 5 at T = 7 puts every outer tap outside."""
    _run_conv(2, C_, C_, k, d, 1, False, T, seed=k * 10 + d)


def test_conv_limits_are_refused_before_any_launch():
    lib = _lib.lib()
    buf = torch.zeros(4096, device=DEV)
    for args in ((1, 4, 4, 13, 1, 1, 0, 8), (1, 4, 4, 4, 1, 1, 0, 8), (1, 4, 4, 3, 1, 4, 1, 8), (0, 4, 4, 3, 1, 1, 0, 8), (1, 4, 4, 3, 1, 1, 0, 0)):
        assert lib.parrot_debug_voc_conv_fwd(dptr(buf), dptr(buf), None, dptr(buf), *args, stream_ptr(DEV)) == -1, args
    assert lib.parrot_debug_voc_conv_dw_workspace_bytes(1, 4, 4, 13, 8) == 0


@pytest.mark.parametrize("rows", [1, 5, 64, 65])
@pytest.mark.parametrize("shape", [(7,), (64, 4), (257,), (512, 11)])
def test_weight_norm_forward_and_backward(rows, shape):
    """Row lengths 7, 256, 257 and 5632; (rows, a, k) is a Conv1d's (C_out, C_in, k) as well as a ConvTranspose1d's (C_in, C_out, k):
    the rows are dim 0 either way.  Bounds (u = 2^-24): the norm is an fp64 sum rounded once, so w = v (g / norm) carries three
    roundings: 3 u |w|, 4 u with the reference's own.  dg = s / norm: s is exact to fp64, norm carries u, the quotient's rounding u:
    2 u |dg| + u sum|dw v| / norm for the cancellation in s.  dv: 4 u (|ratio dw| + |c v|)."""
    lib = _lib.lib()
    g_ = torch.Generator().manual_seed(rows * 1000 + shape[0])
    v = torch.randn((rows,) + shape, generator=g_)
    g = torch.rand((rows,) + (1,) * len(shape), generator=g_) + 0.5
    dw = torch.randn(v.shape, generator=g_)
    length = v[0].numel()
    vg, gg, dwg = v.to(DEV), g.to(DEV), dw.to(DEV)
    w, norm = torch.empty_like(vg), torch.empty(rows, device=DEV)
    dv, dg = torch.empty_like(vg), torch.empty(rows, device=DEV)
    with torch.cuda.device(DEV):
        _lib.check(lib.parrot_debug_voc_wn_fwd(dptr(vg), dptr(gg), dptr(w), dptr(norm), rows, length, stream_ptr(DEV)))
        _lib.check(lib.parrot_debug_voc_wn_bwd(dptr(dwg), dptr(vg), dptr(gg), dptr(norm), dptr(dv), dptr(dg), rows, length, stream_ptr(DEV)))
    u = 2.0 ** -24
    v64, g64, dw64 = v.double().flatten(1), g.double().flatten(), dw.double().flatten(1)
    n64 = v64.norm(dim=1)
    assert bool(((norm.cpu().double() - n64).abs() <= u * n64).all())  # an fp64 sum, rounded to fp32 once
    w64 = v64 * (g64 / n64)[:, None]
    assert bool(((w.cpu().double().flatten(1) - w64).abs() <= 4 * u * w64.abs() + 1e-45).all())
    s = (dw64 * v64).sum(dim=1)
    dg64 = s / n64
    assert bool(((dg.cpu().double() - dg64).abs() <= 2 * u * dg64.abs() + u * (dw64 * v64).abs().sum(dim=1) / n64 * 2).all())
    ratio, c = (g64 / n64)[:, None], (g64 * s / n64 ** 3)[:, None]
    dv64 = ratio * dw64 - c * v64
    assert bool(((dv.cpu().double().flatten(1) - dv64).abs() <= 4 * u * ((ratio * dw64).abs() + (c * v64).abs()) + 1e-45).all())
    # both torch's own forward and autograd agree with the formula (so the formula is the reference's)
    vt, gt = v.double().requires_grad_(True), g.double().requires_grad_(True)
    wt = torch._weight_norm(vt, gt, 0)
    tv, tg = torch.autograd.grad(wt, [vt, gt], dw.double())
    assert torch.allclose(wt.detach().flatten(1), w64, rtol=1e-12, atol=0) and torch.allclose(tv.flatten(1), dv64, rtol=1e-9, atol=1e-12)
    assert torch.allclose(tg.flatten(), dg64, rtol=1e-9, atol=1e-12)


def test_weight_norm_of_a_zero_row_is_torchs():
    lib = _lib.lib()
    v = torch.randn((3, 5))
    v[1] = 0
    g = torch.ones((3, 1))
    vg, gg = v.to(DEV), g.to(DEV)
    w, norm = torch.empty_like(vg), torch.empty(3, device=DEV)
    with torch.cuda.device(DEV):
        _lib.check(lib.parrot_debug_voc_wn_fwd(dptr(vg), dptr(gg), dptr(w), dptr(norm), 3, 5, stream_ptr(DEV)))
    want = torch._weight_norm(v, g, 0)
    assert bool(torch.isnan(want[1]).all()) and bool(torch.isnan(w.cpu()[1]).all())  # 0 x (1 / 0): nothing is clamped
    assert bool(torch.isfinite(w.cpu()[[0, 2]]).all())


def _embed_grad(ids, dx, per, V):
    lib = _lib.lib()
    rows, D = dx.shape
    out = torch.full((V, D), float("nan"), device=DEV)
    ids_g, dx_g = ids.to(DEV), dx.to(DEV)  # (held until the result is back: a temporary's block would be handed to the next one)
    with torch.cuda.device(DEV):
        _lib.check(lib.parrot_debug_tte_embed_grad(dptr(ids_g), dptr(dx_g), dptr(out), rows, per, D, V, -1, stream_ptr(DEV)))
    return out.cpu()


def test_embedding_gradients_dict_with_repeats_and_spkr_with_shared_rows():
    """The two scatters of the backward, as it launches them: d dict over rows (b, u) with repeated codes, d spkr over the frames
    and over the batch rows that share a speaker (per = U).  Integer data: exact."""
    B, U, E = 3, 5, 36
    dx = _ints((B * U, E), 3, 9)
    code = torch.tensor([[4, 4, 7, 0, 4], [7, 7, 7, 1, 0], [2, 4, 0, 0, 9]])
    want = torch.zeros((10, E), dtype=torch.float64).index_add_(0, code.flatten(), dx.double())
    assert torch.equal(_embed_grad(code.flatten(), dx, 1, 10).double(), want)
    spkr = torch.tensor([6, 2, 6])
    want = torch.zeros((10, E), dtype=torch.float64).index_add_(0, spkr.repeat_interleave(U), dx.double())
    assert torch.equal(_embed_grad(spkr, dx, U, 10).double(), want)
