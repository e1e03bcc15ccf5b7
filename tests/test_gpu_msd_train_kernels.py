"""GPU: the new forms of the multi-scale discriminator's training alone, through the debug entry points (parrot_debug_msd_*), on small
integers: |x| <= 3, |w| <= 2, |dy| <= 2, so every sum here is an integer below 2^24 and the comparison with torch's fp64 conv on the
CPU is EQUALITY for forward, data gradient and weight gradient.  The leaky ReLU's slope is 0.5, which keeps the values exact.

    gconv_*  one grouped conv of 41 taps, padding 20, stride 1, 2 or 4: per-group widths on both sides of the 32-row wave tile and the
             64-row block, input lengths that give one output column, every phase of the stride, a window wholly inside the padding,
             and both sides of the 64-column tile; N = 3 lets a 256-pair weight-gradient chunk straddle two rows; cin / g x 41 > 256
             from cin / g = 7 on, so the accumulator flush is crossed
    first_*  convs[0], 15 taps
    pool_*   AvgPool1d(4, 2, padding=2): forward on multiples of 4, backward on integers read as quarters
    sn_*     spectral norm: fold and backward on values exact in fp32, the power iteration on normals against fp64"""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from parrot_tts_amd import _lib
from parrot_tts_amd.ops import dptr, stream_ptr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SLOPE = 0.5
LENGTHS = (1, 2, 5, 63, 64, 65, 129, 257, 4 * 64 + 3)
R, R_SMALL = 8.0, 256.0


def _ints(gen, shape, lim):
    return torch.randint(-lim, lim + 1, shape, generator=gen).to(torch.float64)


def _dev(t):
    return t.to(torch.float32).contiguous().to(DEV)


def _lrelu(x):
    return torch.where(x > 0, x, SLOPE * x)


def _ws(n):
    return torch.empty(max(int(n), 1), dtype=torch.uint8, device=DEV)


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


@pytest.mark.parametrize("stride", [1, 2, 4])
@pytest.mark.parametrize("cing,coutg,g", [(1, 1, 3), (3, 5, 2), (8, 16, 2), (7, 33, 1), (33, 65, 2)])
def test_grouped_conv_forward_data_and_weight_gradient_are_exact(stride, cing, coutg, g):
    lib, k = _lib.lib(), 41
    cin, cout = cing * g, coutg * g
    gen = torch.Generator().manual_seed(1000 * stride + 10 * cing + g)
    for T, N in itertools.product(LENGTHS, (1, 3)):
        x = _ints(gen, (N, cin, T), 3).requires_grad_(True)
        w = _ints(gen, (cout, cing, k), 2).requires_grad_(True)
        b = _ints(gen, (cout,), 2)
        y = F.conv1d(x, w, b, stride, padding=20, groups=g)
        To = y.shape[2]
        assert To == (T - 1) // stride + 1
        dy = _ints(gen, y.shape, 2)
        dx, dw = torch.autograd.grad(y, [x, w], dy)
        pre, mask = _ints(gen, x.shape, 3), _ints(gen, x.shape, 1)
        dxm = torch.where(mask > 0, pre + dx, SLOPE * (pre + dx))
        tag = (stride, cing, coutg, g, T, N)
        xs, ws_, bs, dys = _dev(x.detach()), _dev(w.detach()), _dev(b), _dev(dy)
        for act in (0, 1):
            out = _nan(N, cout, To)
            _lib.check(lib.parrot_debug_msd_gconv_fwd(dptr(xs), dptr(ws_), dptr(bs), dptr(out), N, cin, cout, g, k, stride, T, act, SLOPE,
                                                      stream_ptr(DEV)))
            want = _lrelu(y.detach()) if act else y.detach()
            assert torch.equal(out.cpu().double(), want), ("fwd", act) + tag
        out = _nan(N, cin, T)
        _lib.check(lib.parrot_debug_msd_gconv_dx(dptr(dys), dptr(ws_), None, None, SLOPE, dptr(out), N, cin, cout, g, k, stride, T, stream_ptr(DEV)))
        assert torch.equal(out.cpu().double(), dx), ("dx",) + tag
        out.fill_(float("nan"))
        pres, masks = _dev(pre), _dev(mask)
        _lib.check(lib.parrot_debug_msd_gconv_dx(dptr(dys), dptr(ws_), dptr(pres), dptr(masks), SLOPE, dptr(out), N, cin, cout, g, k, stride, T,
                                                 stream_ptr(DEV)))
        assert torch.equal(out.cpu().double(), dxm), ("dx, pre and mask",) + tag
        n_ws = lib.parrot_debug_msd_gconv_dw_workspace_bytes(N, cin, cout, g, k, stride, T)
        assert n_ws > 0
        wsb, out = _ws(n_ws), _nan(cout, cing, k)
        _lib.check(lib.parrot_debug_msd_gconv_dw(dptr(dys), dptr(xs), dptr(out), N, cin, cout, g, k, stride, T, dptr(wsb), n_ws, stream_ptr(DEV)))
        assert torch.equal(out.cpu().double(), dw), ("dw",) + tag


@pytest.mark.parametrize("c1", [1, 16, 33])
def test_first_layer_is_exact(c1):
    lib, k = _lib.lib(), 15
    gen = torch.Generator().manual_seed(c1)
    for T, N in itertools.product(LENGTHS, (1, 3)):
        x = _ints(gen, (N, 1, T), 3).requires_grad_(True)
        w = _ints(gen, (c1, 1, k), 2).requires_grad_(True)
        b = _ints(gen, (c1,), 2)
        y = F.conv1d(x, w, b, 1, padding=7)
        dy = _ints(gen, y.shape, 2)
        dx, dw = torch.autograd.grad(y, [x, w], dy)
        xs, ws_, bs, dys = _dev(x.detach()), _dev(w.detach()), _dev(b), _dev(dy)
        out = _nan(N, c1, T)
        _lib.check(lib.parrot_debug_msd_first_fwd(dptr(xs), dptr(ws_), dptr(bs), dptr(out), N, T, c1, SLOPE, stream_ptr(DEV)))
        assert torch.equal(out.cpu().double(), _lrelu(y.detach())), ("fwd", c1, T, N)
        out = _nan(N, 1, T)
        _lib.check(lib.parrot_debug_msd_first_dx(dptr(dys), dptr(ws_), dptr(out), N, T, c1, stream_ptr(DEV)))
        assert torch.equal(out.cpu().double(), dx), ("dx", c1, T, N)
        n_ws = lib.parrot_debug_msd_first_dw_workspace_bytes(N, T, c1)
        assert n_ws > 0
        wsb, out = _ws(n_ws), _nan(c1, 1, k)
        _lib.check(lib.parrot_debug_msd_first_dw(dptr(dys), dptr(xs), dptr(out), N, T, c1, dptr(wsb), n_ws, stream_ptr(DEV)))
        assert torch.equal(out.cpu().double(), dw), ("dw", c1, T, N)


def test_pool_forward_and_backward_are_exact():
    lib = _lib.lib()
    gen = torch.Generator().manual_seed(4)
    for T in (1, 2, 3, 8, 65, 257, 1000):
        x = (4 * _ints(gen, (3, 1, T), 50)).requires_grad_(True)  # (multiples of 4: every window sum and its quarter are exact)
        y = F.avg_pool1d(x, 4, 2, 2)
        To = y.shape[2]
        assert To == T // 2 + 1
        out = _nan(3, 1, To)
        _lib.check(lib.parrot_debug_msd_pool_fwd(dptr(_dev(x.detach())), dptr(out), 3, T, stream_ptr(DEV)))
        assert torch.equal(out.cpu().double(), y.detach()), ("fwd", T)
        dy = _ints(gen, y.shape, 50)
        dx, = torch.autograd.grad(y, [x], dy)
        out = _nan(3, 1, T)
        _lib.check(lib.parrot_debug_msd_pool_bwd(dptr(_dev(dy)), dptr(out), 3, T, stream_ptr(DEV)))
        assert torch.equal(out.cpu().double(), dx), ("bwd", T)


def _sn_fold(w, u, v, iterate):
    lib = _lib.lib()
    rows, cols = w.shape
    wd, ud, vd = _dev(w), _dev(u), _dev(v)
    wf, sig = _nan(rows, cols), _nan(1)
    n_ws = 4 * (rows + cols)
    _lib.check(lib.parrot_debug_msd_sn_fold(dptr(wd), dptr(ud), dptr(vd), rows, cols, iterate, dptr(wf), dptr(sig), dptr(_ws(n_ws)), n_ws,
                                            stream_ptr(DEV)))
    return wf.cpu(), sig.cpu(), ud.cpu(), vd.cpu()


@pytest.mark.parametrize("rows,cols", [(1, 3), (5, 7), (65, 300), (130, 2049)])
def test_spectral_fold_and_sigma_gradient_are_exact_on_one_hot_vectors(rows, cols):
    """u = a e_i and v = b e_j with a, b powers of two: sigma = a b W[i][j] exactly, a power of two when W[i][j] is one, so W / sigma is
    exact too; the backward's <G, W> is an integer and every term a dyadic rational far inside fp32."""
    lib = _lib.lib()
    gen = torch.Generator().manual_seed(rows)
    w = _ints(gen, (rows, cols), 2)
    halves = []
    for (i, j, a, b, wij) in ((rows - 1, cols // 2, 0.5, 0.25, 2.0), (0, cols - 1, 2.0, 0.5, -1.0)):
        w[i, j] = wij
        u, v = torch.zeros(rows, dtype=torch.float64), torch.zeros(cols, dtype=torch.float64)
        u[i], v[j] = a, b
        halves.append((u, v))
    for u, v in halves:
        sigma = float(u @ (w @ v))
        wf, sig, u2, v2 = _sn_fold(w, u, v, 0)
        assert float(sig) == sigma and torch.equal(wf.double(), w / sigma)
        assert torch.equal(u2.double(), u) and torch.equal(v2.double(), v)  # (no iteration: the buffers are read only)
    (ua, va), (ub, vb) = halves
    sa, sb = float(ua @ (w @ va)), float(ub @ (w @ vb))
    ga, gb = _ints(gen, (rows, cols), 2), _ints(gen, (rows, cols), 2)
    term = lambda g, u, v, s: g / s - ((g * w).sum() / s ** 2) * torch.outer(u, v)  # noqa: E731
    n_ws = lib.parrot_debug_msd_sn_bwd_workspace_bytes(rows, cols)
    assert n_ws > 0
    dev = [_dev(t) for t in (ga, gb, w, ua, va, torch.tensor([sa]), ub, vb, torch.tensor([sb]))]
    for two in (True, False):
        out = _nan(rows, cols)
        args = [dptr(t) for t in dev]
        if not two:
            args[1] = args[6] = args[7] = args[8] = None
        _lib.check(lib.parrot_debug_msd_sn_bwd(*args, dptr(out), rows, cols, dptr(_ws(n_ws)), n_ws, stream_ptr(DEV)))
        want = term(ga, ua, va, sa) + (term(gb, ub, vb, sb) if two else 0)
        assert torch.equal(out.cpu().double(), want), two


@pytest.mark.parametrize("rows,cols", [(4, 15), (128, 1312), (1024, 2624)])
def test_power_iteration_on_normals_is_held_to_fp64(rows, cols):
    """One iteration, sigma and the fold against fp64 under the project's rule: the yardstick is the same computation in fp32 on the
    CPU (torch's mv, normalize, dot), ours within R = 8 of it with a floor of half an ulp of the largest magnitude."""
    gen = torch.Generator().manual_seed(cols)
    w = (torch.randn((rows, cols), generator=gen, dtype=torch.float64) / cols ** 0.5).float()
    u = F.normalize(torch.randn(rows, generator=gen, dtype=torch.float64), dim=0).float()
    v = F.normalize(torch.randn(cols, generator=gen, dtype=torch.float64), dim=0).float()

    def ref(dt):
        W, uu = w.to(dt), u.to(dt)
        vv = F.normalize(torch.mv(W.t(), uu), dim=0, eps=1e-12)
        uu = F.normalize(torch.mv(W, vv), dim=0, eps=1e-12)
        sigma = torch.dot(uu, torch.mv(W, vv))
        return W / sigma, sigma.reshape(1), uu, vv

    r64, r32 = ref(torch.float64), ref(torch.float32)
    ours = _sn_fold(w, u, v, 1)
    bad = []
    for name, o, a32, a64 in zip(("fold", "sigma", "u", "v"), ours, r32, r64):
        yard = float((a32.double() - a64).abs().max())
        floor = float(np.spacing(np.float32(a64.abs().max().item()))) / 2
        err = float((o.double() - a64).abs().max())
        r = R if a64.numel() >= 8 else R_SMALL
        print(f"sn {rows}x{cols} {name}: err {err:.3e}  yardstick {yard:.3e}  ratio {err / yard if yard else 0:.2f}  floor {floor:.3e}")
        if not err <= max(r * yard, floor):
            bad.append((name, err, yard, floor))
    assert not bad, bad
