"""GPU: the new forms of the multi-period discriminator's training alone, through the debug entry points (parrot_debug_mpd_*), on small
integers: |x| <= 3, |w| <= 2, |dy| <= 2, so every sum here is an integer below 2^24 and the comparison with torch's fp64 conv on the
CPU is EQUALITY for forward, data gradient and weight gradient.  The leaky ReLU's slope is 0.5, which keeps the values exact.

    conv_*   one strided tap conv (k = 5, padding 2, stride 3 and the fifth layer's stride 1) on Z = B p independent rows
    first_*  convs[0] fused with the reflect pad and the fold; d wav includes the reflected samples, which receive two contributions
    post_*   conv_post: the per-column reduction, the outer product, the two-level weight gradient"""
import itertools

import pytest
import torch
import torch.nn.functional as F

from parrot_tts_amd import _lib
from parrot_tts_amd.ops import dptr, stream_ptr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SLOPE = 0.5


def _ints(gen, shape, lim):
    return torch.randint(-lim, lim + 1, shape, generator=gen).to(torch.float64)


def _dev(t):
    return t.to(torch.float32).contiguous().to(DEV)


def _rows(t):
    """torch's (B, C, H, p) -> the library's rows (B p, C, H)"""
    B, C, H, p = t.shape
    return t.permute(0, 3, 1, 2).reshape(B * p, C, H)


def _unrows(t, B, p):
    """(B p, C, H) -> (B, C, H, p)"""
    Z, C, H = t.shape
    return t.view(B, p, C, H).permute(0, 2, 3, 1)


def _lrelu(x):
    return torch.where(x > 0, x, SLOPE * x)


def _ws(n):
    return torch.empty(max(int(n), 1), dtype=torch.uint8, device=DEV)


@pytest.mark.parametrize("stride", [3, 1])
@pytest.mark.parametrize("cin,cout", [(4, 2), (65, 33)])
def test_strided_conv_forward_data_and_weight_gradient_are_exact(stride, cin, cout):
    lib, k = _lib.lib(), 5
    gen = torch.Generator().manual_seed(100 * stride + cin)
    for H, p, B in itertools.product((1, 2, 3, 4, 64, 65, 193), (1, 2, 11), (1, 3)):
        x = _ints(gen, (B, cin, H, p), 3).requires_grad_(True)
        w = _ints(gen, (cout, cin, k, 1), 2).requires_grad_(True)
        b = _ints(gen, (cout,), 2)
        y = F.conv2d(x, w, b, (stride, 1), padding=(2, 0))
        Ho, Z = y.shape[2], B * p
        dy = _ints(gen, y.shape, 2)
        dx, dw = torch.autograd.grad(y, [x, w], dy)
        pre, mask = _ints(gen, x.shape, 3), _ints(gen, x.shape, 1)
        dxm = torch.where(mask > 0, pre + dx, SLOPE * (pre + dx))
        tag = (stride, cin, cout, H, p, B)
        xs, ws_, bs, dys = _dev(_rows(x.detach())), _dev(w.detach()), _dev(b), _dev(_rows(dy))
        for act in (0, 1):
            out = torch.full((Z, cout, Ho), float("nan"), device=DEV)
            _lib.check(lib.parrot_debug_mpd_conv_fwd(dptr(xs), dptr(ws_), dptr(bs), dptr(out), Z, cin, cout, k, stride, H, act, SLOPE, stream_ptr(DEV)))
            want = _lrelu(y.detach()) if act else y.detach()
            assert torch.equal(_unrows(out, B, p).cpu().double(), want), ("fwd", act) + tag
        out = torch.full((Z, cin, H), float("nan"), device=DEV)
        _lib.check(lib.parrot_debug_mpd_conv_dx(dptr(dys), dptr(ws_), None, None, SLOPE, dptr(out), Z, cin, cout, k, stride, H, stream_ptr(DEV)))
        assert torch.equal(_unrows(out, B, p).cpu().double(), dx), ("dx",) + tag
        out.fill_(float("nan"))
        pres, masks = _dev(_rows(pre)), _dev(_rows(mask))
        _lib.check(lib.parrot_debug_mpd_conv_dx(dptr(dys), dptr(ws_), dptr(pres), dptr(masks), SLOPE, dptr(out), Z, cin, cout, k, stride, H,
                                                stream_ptr(DEV)))
        assert torch.equal(_unrows(out, B, p).cpu().double(), dxm), ("dx, pre and mask",) + tag
        n_ws = lib.parrot_debug_mpd_conv_dw_workspace_bytes(Z, cin, cout, k, stride, H)
        assert n_ws > 0
        wsb, out = _ws(n_ws), torch.full((cout, cin, k), float("nan"), device=DEV)
        _lib.check(lib.parrot_debug_mpd_conv_dw(dptr(dys), dptr(xs), dptr(out), Z, cin, cout, k, stride, H, dptr(wsb), n_ws, stream_ptr(DEV)))
        assert torch.equal(out.cpu().double(), dw[..., 0]), ("dw",) + tag


@pytest.mark.parametrize("c1", [1, 4, 33])
def test_first_layer_with_fold_and_reflect_pad_is_exact(c1):
    lib, k, s, N = _lib.lib(), 5, 3, 2
    gen = torch.Generator().manual_seed(c1)
    for T, p in ((22, 11), (23, 11), (32, 11), (12, 11), (13, 2), (64, 1)):  # no pad, the longest pad (10), pad 1, pad 10 of 12, pad 1, p = 1
        wav = _ints(gen, (N, 1, T), 3).requires_grad_(True)
        w = _ints(gen, (c1, 1, k, 1), 2).requires_grad_(True)
        b = _ints(gen, (c1,), 2)
        x = wav
        if T % p:
            x = F.pad(x, (0, p - T % p), "reflect")
        x = x.view(N, 1, x.shape[-1] // p, p)
        y = _lrelu(F.conv2d(x, w, b, (s, 1), padding=(2, 0)))
        H1 = y.shape[2]
        dy = _ints(gen, y.shape, 2) * 2  # (even: the mask's slope 0.5 keeps the restatement's gradient integral)
        dwav, dw = torch.autograd.grad(y, [wav, w], dy)
        tag = (c1, T, p)
        wavs, ws_, bs = _dev(wav.detach()), _dev(w.detach()), _dev(b)
        out = torch.full((N, p, c1, H1), float("nan"), device=DEV)
        _lib.check(lib.parrot_debug_mpd_first_fwd(dptr(wavs), dptr(ws_), dptr(bs), dptr(out), N, T, p, c1, k, s, SLOPE, stream_ptr(DEV)))
        assert torch.equal(out.permute(0, 2, 3, 1).cpu().double(), y.detach()), ("fwd",) + tag
        # the gradient at the conv's output, past the mask, in the library's layout
        g = torch.where(y.detach() > 0, dy, SLOPE * dy)
        gs = _dev(g.permute(0, 3, 1, 2))
        out = torch.full((N, 1, T), float("nan"), device=DEV)
        _lib.check(lib.parrot_debug_mpd_first_dx(dptr(gs), dptr(ws_), dptr(out), N, T, p, c1, k, s, stream_ptr(DEV)))
        assert torch.equal(out.cpu().double(), dwav), ("d wav",) + tag
        n_ws = lib.parrot_debug_mpd_first_dw_workspace_bytes(N, T, p, c1, k, s)
        assert n_ws > 0
        wsb, out = _ws(n_ws), torch.full((c1, k), float("nan"), device=DEV)
        _lib.check(lib.parrot_debug_mpd_first_dw(dptr(gs), dptr(wavs), dptr(out), N, T, p, c1, k, s, dptr(wsb), n_ws, stream_ptr(DEV)))
        assert torch.equal(out.cpu().double(), dw[:, 0, :, 0]), ("dw",) + tag


@pytest.mark.parametrize("C", [1, 65, 1024])
def test_conv_post_is_exact(C):
    lib, Z = _lib.lib(), 2
    gen = torch.Generator().manual_seed(C)
    for H in (1, 63, 65):
        x = _ints(gen, (Z, C, H), 3).requires_grad_(True)
        w = _ints(gen, (1, C, 3), 2).requires_grad_(True)
        b = _ints(gen, (1,), 2)
        y = F.conv1d(x, w, b, padding=1)
        dy = _ints(gen, y.shape, 2)
        dx, dw = torch.autograd.grad(y, [x, w], dy)
        pre, mask = _ints(gen, x.shape, 3), _ints(gen, x.shape, 1)
        xs, ws_, bs, dys = _dev(x.detach()), _dev(w.detach()), _dev(b), _dev(dy)
        out = torch.full((Z, H), float("nan"), device=DEV)
        _lib.check(lib.parrot_debug_mpd_post_fwd(dptr(xs), dptr(ws_), dptr(bs), dptr(out), Z, C, H, stream_ptr(DEV)))
        assert torch.equal(out.cpu().double(), y.detach()[:, 0]), ("fwd", C, H)
        out = torch.full((Z, C, H), float("nan"), device=DEV)
        _lib.check(lib.parrot_debug_mpd_post_dx(dptr(dys), dptr(ws_), None, None, SLOPE, dptr(out), Z, C, H, stream_ptr(DEV)))
        assert torch.equal(out.cpu().double(), dx), ("dx", C, H)
        out.fill_(float("nan"))
        pres, masks = _dev(pre), _dev(mask)
        _lib.check(lib.parrot_debug_mpd_post_dx(dptr(dys), dptr(ws_), dptr(pres), dptr(masks), SLOPE, dptr(out), Z, C, H, stream_ptr(DEV)))
        assert torch.equal(out.cpu().double(), torch.where(mask > 0, pre + dx, SLOPE * (pre + dx))), ("dx, pre and mask", C, H)
        n_ws = lib.parrot_debug_mpd_post_dw_workspace_bytes(Z, C, H)
        assert n_ws > 0
        wsb, out = _ws(n_ws), torch.full((C, 3), float("nan"), device=DEV)
        _lib.check(lib.parrot_debug_mpd_post_dw(dptr(dys), dptr(xs), dptr(out), Z, C, H, dptr(wsb), n_ws, stream_ptr(DEV)))
        assert torch.equal(out.cpu().double(), dw[0]), ("dw", C, H)


def test_limits_are_refused_before_any_launch():
    lib = _lib.lib()
    a = torch.zeros(64, device=DEV)
    p, s = dptr(a), stream_ptr(DEV)
    for code in (lib.parrot_debug_mpd_conv_fwd(p, p, p, p, 1, 4, 2, 4, 3, 8, 1, 0.1, s),       # even k
                 lib.parrot_debug_mpd_conv_fwd(p, p, p, p, 1, 4, 2, 13, 3, 64, 1, 0.1, s),     # k > 11
                 lib.parrot_debug_mpd_conv_dx(p, p, None, None, 0.1, p, 1, 4, 2, 3, 5, 8, s),  # stride > k
                 lib.parrot_debug_mpd_conv_dw(p, p, p, 1, 4, 2, 5, 3, 8, p, 0, s),             # workspace too small
                 lib.parrot_debug_mpd_first_fwd(p, p, p, p, 1, 5, 11, 4, 5, 3, 0.1, s),        # T <= n_pad
                 lib.parrot_debug_mpd_first_dx(p, p, p, 1, 2, 4, 4, 5, 3, s),                  # T == n_pad
                 lib.parrot_debug_mpd_first_dw(p, p, p, 1, 12, 11, 4, 5, 3, p, 0, s),          # workspace too small
                 lib.parrot_debug_mpd_post_fwd(p, p, p, p, 0, 4, 4, s),                        # Z = 0
                 lib.parrot_debug_mpd_post_dw(p, p, p, 1, 4, 4, p, 0, s)):                     # workspace too small
        assert code == -1
    torch.cuda.synchronize()
    assert bool((a == 0).all())
