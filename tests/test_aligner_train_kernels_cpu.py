"""CPU: tests/aligner_train_kernels_ref.py (the numpy restatement of the aligner's training kernels that
tests/test_gpu_aligner_train_kernels.py holds the device to) pinned against torch in fp64, with the very parameter sets
host_aligner_train.hip builds; and the refusals of the parrot_debug_* entry points of those kernels, which all happen on the host
before any launch -- so they are exercised here on made-up pointers, without a device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import aligner_train_kernels_ref as K  # noqa: E402

B, T, NM, D, H, V = 3, 11, 7, 6, 4, 5  # (n_mels is NM here)
TG = K.host_tap_gemm_sets(B, T, NM, D, H, V)
WG = K.host_wgrad_sets(B, T, NM, D, H, V)


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _close(got, want, name):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, name
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), name


def _tg(p, A, X, b0=None, b1=None):
    """The set on fp64 data -> the addressed (Z, M, N) block read back through the set's own C strides."""
    out = K.tap_gemm(p, A.ravel(), X.ravel(), np.zeros(p["c_size"]), b0, b1)
    z, m, n = np.arange(p["Z"]), np.arange(p["M"]), np.arange(p["N"])
    return out, out[p["c_base"] + z[:, None, None] * p["c_sz"] + m[None, :, None] * p["c_sm"] + n[None, None, :] * p["c_sn"]]


@pytest.mark.parametrize("first", [True, False])
def test_conv_sets_are_conv1d_and_its_autograd(first):
    rng = _rng(1 + first)
    cin = NM if first else D
    w = torch.from_numpy(rng.standard_normal((D, cin, 5))).requires_grad_(True)
    x = torch.from_numpy(rng.standard_normal((B, cin, T))).requires_grad_(True)
    y = F.relu(F.conv1d(x, w, None, padding=2))
    g = torch.from_numpy(rng.standard_normal((B, D, T)))
    # forward: the mel is (B, T, n_mels) in memory, later inputs channel-first
    xmem = x.detach().numpy().transpose(0, 2, 1).copy() if first else x.detach().numpy()
    p = TG["conv0" if first else "conv1"]
    assert p["a_size"] == w.numel() and p["x_size"] == x.numel() and p["c_size"] == y.numel()
    full, blk = _tg(p, w.detach().numpy(), xmem)
    _close(blk, y.detach().numpy(), "conv forward")
    _close(full.reshape(B, D, T), y.detach().numpy(), "conv forward, layout")
    # weight gradient of conv (no ReLU in between: dY is the gradient at the conv's output)
    y2 = F.conv1d(x, w, None, padding=2)
    gw, gx = torch.autograd.grad(y2, (w, x), g)
    q = WG["conv0" if first else "conv1"]
    assert q["o_size"] == w.numel() and q["y_size"] == g.numel() and q["x_size"] == x.numel()
    _close(K.wgrad(q, g.numpy().ravel(), xmem.ravel(), np.zeros(q["o_size"])).reshape(D, cin, 5), gw.numpy(), "conv weight gradient")
    if not first:  # (the mel gets no gradient)
        _close(_tg(TG["dgrad"], w.detach().numpy(), g.numpy())[1], gx.numpy(), "conv data gradient")


def test_lstm_and_linear_sets_are_the_matrix_products():
    rng = _rng(3)
    y2 = rng.standard_normal((B, D, T))
    w_ih, b_ih, b_hh = rng.standard_normal((2, 4 * H, D)), rng.standard_normal((2, 4 * H)), rng.standard_normal((2, 4 * H))
    xproj = np.zeros(TG["xproj0"]["c_size"])
    for d in (0, 1):
        xproj = K.tap_gemm(TG[f"xproj{d}"], w_ih[d].ravel(), y2.ravel(), xproj, b_ih[d], b_hh[d])
    want = np.concatenate([np.einsum("mk,bkt->btm", w_ih[d], y2) + b_ih[d] + b_hh[d] for d in (0, 1)], axis=-1)
    _close(xproj.reshape(B, T, 8 * H), want, "xproj")
    h, lin_w, lin_b = rng.standard_normal((B, T, 2 * H)), rng.standard_normal((V, 2 * H)), rng.standard_normal(V)
    _close(_tg(TG["linear"], lin_w, h, lin_b)[0].reshape(B, T, V), h @ lin_w.T + lin_b, "linear")
    gl = rng.standard_normal((B, T, V))
    _close(_tg(TG["dlstm"], lin_w, gl)[0].reshape(B, T, 2 * H), gl @ lin_w, "dlstm")
    dg = rng.standard_normal((B, T, 8 * H))
    want = sum(np.einsum("mk,btm->bkt", w_ih[d], dg[..., d * 4 * H:(d + 1) * 4 * H]) for d in (0, 1))
    _close(_tg(TG["dy2"], w_ih, dg)[0].reshape(B, D, T), want, "dy2")
    z = np.zeros
    _close(K.wgrad(WG["linear"], gl.ravel(), h.ravel(), z(V * 2 * H)).reshape(V, 2 * H), np.einsum("btm,btk->mk", gl, h), "d lin_w")
    for d in (0, 1):
        dgd = dg[..., d * 4 * H:(d + 1) * 4 * H]
        _close(K.wgrad(WG[f"w_ih{d}"], dg.ravel(), y2.ravel(), z(4 * H * D)).reshape(4 * H, D), np.einsum("btm,bkt->mk", dgd, y2), f"d w_ih{d}")
        hd = h[..., d * H:(d + 1) * H]
        hprev = np.zeros_like(hd)  # h at the step before t: t - 1 forward, t + 1 backward, h_0 = 0
        if d:
            hprev[:, :-1] = hd[:, 1:]
        else:
            hprev[:, 1:] = hd[:, :-1]
        _close(K.wgrad(WG[f"w_hh{d}"], dg.ravel(), h.ravel(), z(4 * H * H)).reshape(4 * H, H), np.einsum("btm,btk->mk", dgd, hprev), f"d w_hh{d}")


def test_integer_data_is_summed_in_int64_and_untouched_elements_keep_their_value():
    rng = _rng(4)
    p = K.tg_xproj(5, 3, 7, 2, 1)
    A, X = rng.integers(-4, 5, p["a_size"]), rng.integers(-4, 5, p["x_size"])
    out = K.tap_gemm(p, A, X, np.full(p["c_size"], -7777, np.int64), rng.integers(-4, 5, 5), rng.integers(-4, 5, 5))
    assert out.dtype == np.int64
    out = out.reshape(2, 3, 10)
    assert (out[..., :5] == -7777).all() and (out[..., 5:] != -7777).all()
    assert K.colsum(rng.integers(-4, 5, 60), 6, 4, 10, base=3).dtype == np.int64
    assert K.passes(K.tg_conv(1, 1, 112, 1, False)) == 20 and K.passes(K.tg_linear(1, 1, 272, 1)) == 9
    triples = K.sample_triples()
    assert len(triples) == 40 and len(set(triples)) == 40
    for pos in range(3):
        assert sorted({t[pos] for t in triples}) == sorted(K.SIZES)


@pytest.mark.parametrize("n_b, n_t", [(2, 1), (3, 17)])
def test_batchnorm_pair_is_batch_norm_training_and_its_autograd(n_b, n_t):
    rng = _rng(5)
    Cn, eps = 3, 1e-5
    x = torch.from_numpy(np.maximum(rng.standard_normal((n_b, Cn, n_t)), 0.0)).requires_grad_(True)  # a ReLU's output
    gamma = torch.from_numpy(rng.standard_normal(Cn)).requires_grad_(True)
    beta = torch.from_numpy(rng.standard_normal(Cn)).requires_grad_(True)
    rm, rv = torch.from_numpy(rng.standard_normal(Cn)), torch.from_numpy(rng.uniform(0.5, 2.0, Cn))
    rm0, rv0 = rm.numpy().copy(), rv.numpy().copy()
    y = F.batch_norm(x, rm, rv, gamma, beta, training=True, momentum=0.1, eps=eps)
    got = K.bn_train(x.detach().numpy(), gamma.detach().numpy(), beta.detach().numpy(), rm0, rv0, eps, True, np.float64)
    _close(got["y"], y.detach().numpy(), "y")
    _close(got["run_mean"], rm.numpy(), "running_mean")
    _close(got["run_var"], rv.numpy(), "running_var")
    ev = K.bn_train(x.detach().numpy(), gamma.detach().numpy(), beta.detach().numpy(), rm0, rv0, eps, False, np.float64)
    _close(ev["y"], F.batch_norm(x, torch.from_numpy(rm0), torch.from_numpy(rv0), gamma, beta, training=False, eps=eps).detach().numpy(), "eval y")
    assert np.array_equal(ev["run_mean"], rm0) and np.array_equal(ev["run_var"], rv0)
    # backward through BatchNorm and the ReLU in front of it: the gradient at the conv's output
    pre = torch.from_numpy(np.where(x.detach().numpy() > 0, x.detach().numpy(), -1.0)).requires_grad_(True)
    y = F.batch_norm(F.relu(pre), torch.from_numpy(rm0), torch.from_numpy(rv0), gamma, beta, training=True, momentum=0.1, eps=eps)
    dy = torch.from_numpy(rng.standard_normal(tuple(y.shape)))
    gpre, gg, gb = torch.autograd.grad(y, (pre, gamma, beta), dy)
    bw = K.bn_relu_bwd(dy.numpy(), x.detach().numpy(), gamma.detach().numpy(), got["mean"], got["invstd"], np.float64)
    _close(bw["dx"], gpre.numpy(), "dx")
    _close(bw["dgamma"], gg.numpy(), "dgamma")
    _close(bw["dbeta"], gb.numpy(), "dbeta")
    assert (bw["dx"][x.detach().numpy() == 0] == 0).all()


# =========================================================================================================================================
# refusals: every one before a launch, so no device is needed (tests/test_gpu_aligner_train_kernels.py repeats them on real buffers)
# =========================================================================================================================================
E_INVALID, E_UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def lib():
    from parrot_tts_amd import build, _lib
    build.build()
    return _lib.lib()


def fake(n, p=0x10000):
    from parrot_tts_amd import _lib
    return _lib.DebugBuf(p, n)


def tap_gemm_refusals():
    """(name, set, {buffer: count override}, code): each a change to the valid conv set of the table above."""
    base = TG["conv1"]
    ch = lambda **kw: dict(base, **kw)  # noqa: E731
    return [("null A", base, dict(A=None), E_INVALID), ("empty X", base, dict(X=0), E_INVALID), ("null C", base, dict(C=None), E_INVALID),
            ("M = 0", ch(M=0), {}, E_INVALID), ("N < 0", ch(N=-3), {}, E_INVALID), ("K = 0", ch(K=0), {}, E_INVALID), ("Z = 0", ch(Z=0), {}, E_INVALID),
            ("no taps", ch(ntaps=0), {}, E_INVALID), ("six taps", ch(ntaps=6), {}, E_UNSUPPORTED),
            ("A one short", base, dict(A=base["a_size"] - 1), E_INVALID), ("X one short", base, dict(X=base["x_size"] - 1), E_INVALID),
            ("C one short", base, dict(C=base["c_size"] - 1), E_INVALID),
            ("negative A stride", ch(a_sk=-5), {}, E_INVALID), ("negative C stride", ch(c_sm=-T), {}, E_INVALID),
            ("negative x_off", ch(x_off=[0, 0, -1, 0, 0]), {}, E_INVALID), ("x_off past the end", ch(x_off=[0, 0, 0, 0, 1]), {}, E_INVALID),
            ("bias short", base, dict(bias0=D - 1), E_INVALID), ("bias1 alone", base, dict(bias1=D), E_INVALID),
            ("Z beyond the grid", ch(Z=65536, x_sz=0, c_sz=0), {}, E_UNSUPPORTED)]


def wgrad_refusals():
    base = WG["conv1"]
    ch = lambda **kw: dict(base, **kw)  # noqa: E731
    return [("null dY", base, dict(dY=None), E_INVALID), ("empty out", base, dict(out=0), E_INVALID), ("M = 0", ch(M=0), {}, E_INVALID),
            ("T = 0", ch(T=0), {}, E_INVALID), ("R no multiple of T", ch(R=B * T + 1), {}, E_INVALID), ("six taps", ch(ntaps=6), {}, E_UNSUPPORTED),
            ("dY one short", base, dict(dY=base["y_size"] - 1), E_INVALID), ("X one short", base, dict(X=base["x_size"] - 1), E_INVALID),
            ("out one short", base, dict(out=base["o_size"] - 1), E_INVALID), ("negative out stride", ch(o_sj=-1), {}, E_INVALID),
            ("workspace one byte short", base, dict(ws=-1), E_INVALID), ("null workspace", base, dict(ws=None), E_INVALID),
            ("chunks x taps beyond the grid", ch(T=1, R=13108 * 256, y_sz=0, x_sz=0), {}, E_UNSUPPORTED)]


def call_tap_gemm(lib, mk, p, over):
    from parrot_tts_amd import ops
    n = dict(A=p["a_size"], X=p["x_size"], C=p["c_size"], bias0=None, bias1=None)
    n.update(over)
    b = {k: mk(k, v) for k, v in n.items()}
    return lib.parrot_debug_tap_gemm(C.byref(ops.tap_gemm_desc(p, b["A"], b["X"], b["C"], b["bias0"], b["bias1"])), None)


def call_wgrad(lib, mk, p, over):
    from parrot_tts_amd import ops
    need = lib.parrot_debug_wgrad_workspace_bytes(p["R"], min(p["ntaps"], 5), max(p["M"], 1), p["K"])
    n = dict(dY=p["y_size"], X=p["x_size"], out=p["o_size"], ws=0)
    n.update(over)
    ws_bytes = need + (n["ws"] or 0)
    ws = mk("ws", None if n["ws"] is None else max(ws_bytes // 4, 1))
    b = {k: mk(k, n[k]) for k in ("dY", "X", "out")}
    return lib.parrot_debug_wgrad(C.byref(ops.wgrad_desc(p, b["dY"], b["X"], b["out"])), ws.p, ws_bytes, None)


def _fake_mk(name, n):
    from parrot_tts_amd import _lib
    return _lib.DebugBuf(None, 0) if n is None else fake(n)


@pytest.mark.parametrize("case", tap_gemm_refusals(), ids=lambda c: c[0])
def test_tap_gemm_refuses(lib, case):
    name, p, over, code = case
    assert call_tap_gemm(lib, _fake_mk, p, over) == code, lib.parrot_last_error()
    assert b"debug_tap_gemm" in lib.parrot_last_error()


@pytest.mark.parametrize("case", wgrad_refusals(), ids=lambda c: c[0])
def test_wgrad_refuses(lib, case):
    name, p, over, code = case
    assert call_wgrad(lib, _fake_mk, p, over) == code, lib.parrot_last_error()
    assert b"debug_wgrad" in lib.parrot_last_error()


def colsum_refusals():
    """(name, R, M, ld, src count, out0 count, out1 count or None, workspace bytes beyond the need or None, code)"""
    return [("src short", 6, 4, 10, 53, 4, None, 0, E_INVALID), ("out0 short", 6, 4, 10, 54, 3, None, 0, E_INVALID),
            ("out1 short", 6, 4, 10, 54, 4, 3, 0, E_INVALID), ("R = 0", 0, 4, 10, 54, 4, None, 0, E_INVALID),
            ("M = 0", 6, 0, 10, 54, 4, None, 0, E_INVALID), ("negative ld", 6, 4, -10, 54, 4, None, 0, E_INVALID),
            ("workspace short", 6, 4, 10, 54, 4, None, -1, E_INVALID), ("null workspace", 6, 4, 10, 54, 4, None, None, E_INVALID),
            ("chunks beyond the grid", 65536 * 256, 1, 0, 1, 1, None, 0, E_UNSUPPORTED)]


def call_colsum(lib, mk, R, M, ld, n_src, n_out0, n_out1, ws_extra):
    from parrot_tts_amd import _lib
    need = lib.parrot_debug_colsum_workspace_bytes(max(R, 1), max(M, 1))
    ws_bytes = need + (ws_extra or 0)
    ws = mk("ws", None if ws_extra is None else max(ws_bytes // 4, 1))
    d = _lib.DebugColsumDesc(mk("src", n_src), mk("out0", n_out0), mk("out1", n_out1), R, M, ld)
    return lib.parrot_debug_colsum(C.byref(d), ws.p, ws_bytes, None)


@pytest.mark.parametrize("case", colsum_refusals(), ids=lambda c: c[0])
def test_colsum_refuses(lib, case):
    assert call_colsum(lib, _fake_mk, *case[1:-1]) == case[-1], lib.parrot_last_error()
    assert b"debug_colsum" in lib.parrot_last_error()


BN_BUFS = ("x", "y", "gamma", "beta", "run_mean", "run_var", "mean", "invstd")
BWD_BUFS = ("dy", "x", "dx", "gamma", "mean", "invstd", "dgamma", "dbeta")


def bn_refusals():
    """(name, backward?, B, C, T, training, {buffer: count}, code)"""
    out = [("x short", False, 2, 3, 5, 1, dict(x=29), E_INVALID), ("y null", False, 2, 3, 5, 1, dict(y=None), E_INVALID),
           ("one value per channel", False, 1, 3, 1, 1, {}, E_INVALID), ("C = 0", False, 2, 0, 5, 1, {}, E_INVALID),
           ("T < 0", False, 2, 3, -5, 0, {}, E_INVALID), ("dx short", True, 2, 3, 5, 1, dict(dx=29), E_INVALID),
           ("dgamma short", True, 2, 3, 5, 1, dict(dgamma=2), E_INVALID), ("B = 0", True, 0, 3, 5, 1, {}, E_INVALID)]
    out += [(f"{k} short", False, 2, 3, 5, 1, {k: 2}, E_INVALID) for k in BN_BUFS[2:]]
    out += [(f"bwd {k} null", True, 2, 3, 5, 1, {k: None}, E_INVALID) for k in BWD_BUFS[:6]]
    return out


def call_bn(lib, mk, bwd, nb, nc, nt, training, over):
    from parrot_tts_amd import _lib
    names = BWD_BUFS if bwd else BN_BUFS
    full = max(nb * nc * nt, 1)
    n = {k: (full if k in ("x", "y", "dy", "dx") else max(nc, 1)) for k in names}
    n.update(over)
    bufs = [mk(k, n[k]) for k in names]
    if bwd:
        return lib.parrot_debug_bn_relu_bwd(C.byref(_lib.DebugBnBwdDesc(*bufs, nb, nc, nt)), None)
    return lib.parrot_debug_bn_train(C.byref(_lib.DebugBnTrainDesc(*bufs, nb, nc, nt, training, 1e-5)), None)


@pytest.mark.parametrize("case", bn_refusals(), ids=lambda c: c[0])
def test_batchnorm_entry_points_refuse(lib, case):
    assert call_bn(lib, _fake_mk, *case[1:-1]) == case[-1], lib.parrot_last_error()
    assert b"debug_bn" in lib.parrot_last_error()


def test_null_descriptors_and_workspace_queries(lib):
    for fn in (lib.parrot_debug_tap_gemm, lib.parrot_debug_bn_train, lib.parrot_debug_bn_relu_bwd):
        assert fn(None, None) == E_INVALID
    assert lib.parrot_debug_wgrad(None, 0x10000, 64, None) == E_INVALID and lib.parrot_debug_colsum(None, 0x10000, 64, None) == E_INVALID
    assert lib.parrot_debug_wgrad_workspace_bytes(600, 5, 33, 65) == 3 * 5 * 33 * 65 * 4
    assert lib.parrot_debug_wgrad_workspace_bytes(256, 1, 1, 1) == 4 and lib.parrot_debug_wgrad_workspace_bytes(257, 1, 1, 1) == 8
    for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 6, 1, 1), (1, 1, 0, 1), (1, 1, 1, -1)):
        assert lib.parrot_debug_wgrad_workspace_bytes(*bad) == 0, bad
    assert lib.parrot_debug_colsum_workspace_bytes(1000, 300) == 4 * 300 * 8
    assert lib.parrot_debug_colsum_workspace_bytes(0, 3) == 0 and lib.parrot_debug_colsum_workspace_bytes(3, 0) == 0
