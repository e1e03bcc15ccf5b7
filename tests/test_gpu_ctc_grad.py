"""GPU: the gradient of the aligner's CTC loss on the device (parrot_tts_amd.aligner.ctc_loss_and_grad / ctc_loss_trainable / CTCLoss
over parrot_ctc_loss_grad).

The yardstick is the reference's own operator (utils/aligner/trainer.py:60-71) on the CPU in fp64, through autograd:
``x64.requires_grad_(); F.ctc_loss(x64.transpose(0, 1).log_softmax(2), tokens, ml, tl, reduction='none')`` and a backward with row
weights w.  Per case, e_case is the error of torch's CPU fp32 gradient against that fp64 run (unit weights; the largest absolute
difference over the real frames of the rows that have a path), and the device stays within max(2 e_case, FLOOR) max|w_b| on every
element.  2: the margin of tests/test_gpu_ctc.py (device expf / logf an ulp off the host's, another sum order).  FLOOR = 4e-6 is
the one error the fp64 recursion does not remove, the fp32 log-sum-exp per frame: a shift d of a frame's lp cancels in the
occupancy and scales exp(lp) by e^-d, and one ulp of logf(s), s <= V <= 100, plus a few ulps of relative error in the fp32 sum give
d <~ 2e-6 for the logits used here (|x| <~ 25).  torch's CPU backward is off for a row whose LAST token is the blank (it assigns the
last token's term at the last frame and so drops the final blank state's): no such row where torch is the yardstick; that case is
held to tests/ctc_grad_ref.py instead.  Measured (MI355X): DESIGN.md section 3.

The whole file also passes under PARROT_POISON_WS=nan (workspace and outputs filled with NaN at the top of the entry point)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctc_grad_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from parrot_tts_amd import _lib  # noqa: E402
from parrot_tts_amd import aligner as A  # noqa: E402

DEV = "cuda:0"
FLOOR = 4e-6


# ---- the generators of tests/test_gpu_ctc.py -----------------------------------------------------------------------------------
def _tokens(rng, B, N, V, no_repeat_rows=()):
    tokens = rng.integers(1, V, size=(B, N))
    for b in no_repeat_rows:
        for j in range(1, N):
            if tokens[b, j] == tokens[b, j - 1]:
                tokens[b, j] = tokens[b, j] % (V - 1) + 1
    return torch.from_numpy(tokens)


def _case(seed, B, T, V, N, gain, mel_len=None, tokens_len=None, no_repeat_rows=()):
    gen = torch.Generator().manual_seed(seed)
    logits = torch.randn((B, T, V), generator=gen) * gain
    tokens = _tokens(np.random.Generator(np.random.PCG64(seed)), B, N, V, no_repeat_rows)
    return logits, tokens, list(mel_len or [T] * B), list(tokens_len or [N] * B)


def _doubled(mel_len_row1):
    logits, tokens, ml, tl = _case(21, 3, 12, 21, 6, 2.0, mel_len=(12, mel_len_row1, 9), tokens_len=(6, 6, 4))
    tokens[1] = torch.tensor([3, 5, 5, 7, 2, 9])  # one repeat: 7 frames at least
    return logits, tokens, ml, tl


def _blank(last):
    logits, tokens, ml, tl = _case(22, 2, 14, 21, 5, 2.0, mel_len=(14, 11))
    tokens[0] = torch.tensor([4, 0, 0, 7, 0] if last else [4, 0, 0, 7, 3])  # the blank as a label, doubled; last or not
    return logits, tokens, ml, tl


# no row ends in the blank: the generators draw tokens from [1, V)
CASES = {
    "smallest": lambda: _case(4, 1, 1, 21, 1, 1.0),
    "b3t23": lambda: _case(1, 3, 23, 21, 5, 1.0),
    "b3t23_peaky": lambda: _case(1, 3, 23, 21, 5, 6.0),
    "ragged_t_eq_n": lambda: _case(2, 4, 60, 21, 9, 3.0, mel_len=(60, 23, 41, 9), tokens_len=(9, 4, 7, 9), no_repeat_rows=(3,)),
    "doubled_feasible": lambda: _doubled(7),       # mel_len = tokens_len + 1 with one repeat
    "blank_middle": lambda: _blank(False),
    "s257": lambda: _case(5, 2, 300, 41, 128, 4.0),
    "s601_v100": lambda: _case(6, 2, 700, 100, 300, 4.0),
    # more than one state per thread: K = 2 (the second row with idle threads at the end), then K = 5, 3, 4 with 226 MB of alpha
    "k2": lambda: _case(8, 2, 760, 41, 600, 4.0, mel_len=(760, 700), tokens_len=(600, 513), no_repeat_rows=(0, 1)),
    "k345": lambda: _case(9, 3, 2300, 21, 2048, 3.0, mel_len=(2300, 1250, 1800), tokens_len=(2048, 1100, 1600), no_repeat_rows=(0, 1, 2)),
}
_cache = {}


def _weights(B, seed):
    rng = np.random.Generator(np.random.PCG64(100 + seed))
    w = rng.uniform(0.5, 1.5, size=B) * np.where(np.arange(B) % 2 == 0, -1.0, 1.0)  # both signs (B = 1: negative)
    return torch.from_numpy(w)


def _yardstick(logits, tokens, ml, tl, weights, dtype=torch.float64, reduction="none"):
    """The trainer's own lines on the CPU: -> (loss, [d (w . loss) / d logits for w in weights]) as fp64."""
    x = logits.to(dtype).clone().requires_grad_()
    loss = F.ctc_loss(x.transpose(0, 1).log_softmax(2), tokens, torch.tensor(ml), torch.tensor(tl), reduction=reduction)
    grads = []
    for w in weights:
        x.grad = None
        loss.backward(torch.ones_like(loss) if w is None else w.to(dtype).reshape(loss.shape), retain_graph=True)
        grads.append(x.grad.double().clone())
    return loss.detach().double(), grads


def _real(ml, T, rows=None):
    """(B, T) bool: the real frames, of ``rows`` only when given."""
    m = torch.arange(T)[None, :] < torch.tensor(ml)[:, None]
    if rows is not None:
        m = m & rows[:, None]
    return m


def _e_case(logits, tokens, ml, tl):
    """(e_case, the fp64 nll, the fp64 unit-weight gradient)"""
    y64, (g64,) = _yardstick(logits, tokens, ml, tl, [None])
    _, (g32,) = _yardstick(logits, tokens, ml, tl, [None], torch.float32)
    real = _real(ml, logits.shape[1], torch.isfinite(y64))
    return float((g32 - g64)[real].abs().max()), y64, g64


def _device(logits, tokens, ml, tl, w=None, reduction="none", zero_infinity=False):
    """(loss, gradient of the leaf logits) on the device through autograd, with grad_output w."""
    x = logits.to(DEV).requires_grad_()
    loss = A.ctc_loss_trainable(x, tokens, ml, tl, reduction=reduction, zero_infinity=zero_infinity)
    loss.backward(torch.ones_like(loss) if w is None else w.to(DEV).to(loss.dtype).reshape(loss.shape))
    assert x.grad.dtype == torch.float32 and x.grad.shape == x.shape
    return loss.detach().cpu(), x.grad.cpu()


def _results(name):
    """One case once: inputs, the yardsticks, and the device's results.  Shared and left unchanged."""
    if name not in _cache:
        logits, tokens, ml, tl = CASES[name]()
        w = _weights(len(ml), list(CASES).index(name))
        e_case, y64, g64 = _e_case(logits, tokens, ml, tl)
        _, (g64w,) = _yardstick(logits, tokens, ml, tl, [w])
        dl = logits.to(DEV)
        nll, g1 = A.ctc_loss_and_grad(dl, tokens, ml, tl, reduction="none")
        loss_w, gw = _device(logits, tokens, ml, tl, w)
        _cache[name] = dict(logits=logits, tokens=tokens, ml=ml, tl=tl, w=w, e_case=e_case, y64=y64, g64=g64, g64w=g64w, nll=nll.cpu(), g1=g1.cpu(),
                            loss_w=loss_w, gw=gw, nll_fwd=A.ctc_loss(dl, tokens, ml, tl, reduction="none").cpu())
    return _cache[name]


@pytest.mark.parametrize("name", list(CASES))
def test_gradient_against_the_fp64_yardstick(name):
    r = _results(name)
    ml, w, T = r["ml"], r["w"], r["logits"].shape[1]
    assert torch.isfinite(r["y64"]).all()  # every row of these cases has a path
    for b, n in enumerate(r["tl"]):
        assert int(r["tokens"][b, n - 1]) != 0  # torch is the yardstick: no row ends in the blank
    real = _real(ml, T)
    bound = max(2 * r["e_case"], FLOOR)
    e1 = float((r["g1"].double() - r["g64"])[real].abs().max())
    ew = float((r["gw"].double() - r["g64w"])[real].abs().max())
    wmax = float(w.abs().max())
    sums1 = r["g1"].double().sum(2)[real].abs().max().item()
    sumsw = (r["gw"].double().sum(2) / w[:, None])[real].abs().max().item()
    print(f"CTCGRAD {name}: device max abs err {e1:.3e} (unit weights), {ew / wmax:.3e} x max|w| (weights {w.tolist()}); torch fp32 e_case "
          f"{r['e_case']:.3e}, floor {FLOOR:.1e}, bound {bound:.3e}; largest |frame sum| / |w| {max(sums1, sumsw):.3e}")
    # nll: the bits of the forward-only entry point, from both routes
    assert r["nll"].dtype == torch.float64 and r["nll"].numpy().tobytes() == r["nll_fwd"].numpy().tobytes()
    assert r["loss_w"].numpy().tobytes() == r["nll_fwd"].numpy().tobytes()
    # the gradient, element by element
    assert e1 <= bound, (name, e1, bound)
    assert ew <= bound * wmax, (name, ew, bound * wmax)
    # padding frames: exactly zero
    for g in (r["g1"], r["gw"]):
        assert not torch.isnan(g).any()
        assert torch.equal(g[~real], torch.zeros_like(g[~real]))
    # a real frame's gradient sums to zero: softmax minus occupancy
    assert sums1 <= FLOOR and sumsw <= FLOOR


def test_blank_last_row_against_the_restatement():
    """The row torch's CPU backward gets wrong: held to tests/ctc_grad_ref.py on the device's own inputs (the fp32 logits), within
    FLOOR; the other row of the batch too."""
    logits, tokens, ml, tl = _blank(True)
    nll, grad = A.ctc_loss_and_grad(logits.to(DEV), tokens, ml, tl, reduction="none")
    nll, grad = nll.cpu(), grad.cpu()
    for b in range(2):
        n, g = R.ctc_nll_and_grad(logits[b, :ml[b]].numpy(), tokens[b, :tl[b]].numpy())
        err = float(np.abs(grad[b, :ml[b]].double().numpy() - g).max())
        print(f"CTCGRAD blank_last row {b}: device max abs err against the fp64 restatement {err:.3e} (floor {FLOOR:.1e}), nll {n:.6f}")
        assert err <= FLOOR and abs(nll[b].item() - n) <= 1e-6 * abs(n)
        assert torch.equal(grad[b, ml[b]:], torch.zeros_like(grad[b, ml[b]:]))
    _, (g_torch,) = _yardstick(logits, tokens, ml, tl, [None])
    assert float((g_torch[0] - grad[0].double()).abs().max()) > 1e-3  # (and torch is indeed elsewhere on that row)


@pytest.mark.parametrize("name", ["ragged_t_eq_n", "k2"])
def test_determinism_and_nothing_beyond_the_lengths(name):
    r = _results(name)
    logits, tokens, ml, tl = r["logits"].clone(), r["tokens"].clone(), r["ml"], r["tl"]
    B, V = len(ml), logits.shape[2]
    for b in range(B):  # what lies beyond a row's lengths is never read
        logits[b, ml[b]:] = float("nan")
        tokens[b, tl[b]:] = torch.tensor([V + 5, -1] * tokens.shape[1])[:tokens.shape[1] - tl[b]]
    dl = logits.to(DEV)
    nll, grad = A.ctc_loss_and_grad(dl, tokens, ml, tl, reduction="none")
    assert torch.equal(grad.cpu(), r["g1"]) and nll.cpu().numpy().tobytes() == r["nll"].numpy().tobytes()
    nll2, grad2 = A.ctc_loss_and_grad(dl, tokens, ml, tl, reduction="none")  # two calls are bit-equal
    assert torch.equal(grad2, grad) and torch.equal(nll2, nll)
    for b in range(B):  # a row alone, at the same T, is that row of the batch
        _, alone = A.ctc_loss_and_grad(dl[b:b + 1], tokens[b:b + 1], ml[b:b + 1], tl[b:b + 1], reduction="none")
        assert torch.equal(alone[0], grad[b]), b
    perm = [2, 0, 3, 1] if B == 4 else [1, 0]  # the rows beside a row do not matter, nor does its place
    _, gp = A.ctc_loss_and_grad(dl[perm], tokens[perm], [ml[i] for i in perm], [tl[i] for i in perm], reduction="none")
    assert torch.equal(gp, grad[perm])
    # the weighted route: the same bits again
    _, gw = _device(r["logits"], r["tokens"], ml, tl, r["w"])
    assert torch.equal(gw, r["gw"])


def test_row_without_a_path():
    feas, (logits, tokens, ml, tl) = _results("doubled_feasible"), _doubled(6)
    dl = logits.to(DEV)
    T = logits.shape[1]
    nll, grad = A.ctc_loss_and_grad(dl, tokens, ml, tl, reduction="none")
    nll, grad = nll.cpu(), grad.cpu()
    assert nll[1].item() == math.inf
    assert torch.isnan(grad[1, :6]).all() and torch.equal(grad[1, 6:], torch.zeros((T - 6, 21)))  # NaN exactly on the real frames
    _, (g_torch,) = _yardstick(logits, tokens, ml, tl, [None])
    assert torch.isnan(g_torch[1, :6]).all() and not g_torch[1, 6:].any()  # (as torch's CPU backward)
    _, without = A.ctc_loss_and_grad(dl[[0, 2]], tokens[[0, 2]], [ml[0], ml[2]], [tl[0], tl[2]], reduction="none")
    for i, b in enumerate((0, 2)):  # the other rows: the bits of the batch without it, and of the batch in which it has a path
        assert torch.equal(grad[b], without[i].cpu()) and torch.equal(grad[b], feas["g1"][b]), b
        assert nll[b].numpy().tobytes() == feas["nll"][b].numpy().tobytes()
    mean, _ = A.ctc_loss_and_grad(dl, tokens, ml, tl)
    assert mean.item() == math.inf
    # zero_infinity: the row counts 0 and its gradient is 0 throughout
    nll0, grad0 = A.ctc_loss_and_grad(dl, tokens, ml, tl, reduction="none", zero_infinity=True)
    assert nll0[1].item() == 0.0 and torch.equal(nll0.cpu()[[0, 2]], nll[[0, 2]])
    assert torch.equal(grad0[1].cpu(), torch.zeros((T, 21))) and torch.equal(grad0.cpu()[[0, 2]], grad[[0, 2]])
    mean0, gmean0 = A.ctc_loss_and_grad(dl, tokens, ml, tl, zero_infinity=True)
    want = (nll[0].item() / tl[0] + 0.0 + nll[2].item() / tl[2]) / 3
    assert mean0.dtype == torch.float32 and math.isfinite(mean0.item()) and np.float32(mean0.item()).tobytes() == np.float32(want).tobytes()
    assert torch.isfinite(gmean0).all() and torch.equal(gmean0[1].cpu(), torch.zeros((T, 21)))
    loss_t, g_t = _device(logits, tokens, ml, tl, None, "mean", True)  # the autograd route agrees
    assert torch.equal(loss_t, mean0.cpu()) and torch.equal(g_t, gmean0.cpu())
    y0, (g0,) = _yardstick(logits, tokens, ml, tl, [None], reduction="mean")  # (torch without zero_infinity: inf / NaN)
    assert not math.isfinite(y0.item())


def test_reductions_bit_equal_the_forward():
    r = _results("ragged_t_eq_n")
    dl = r["logits"].to(DEV)
    for red in ("mean", "sum", "none"):
        want = A.ctc_loss(dl, r["tokens"], r["ml"], r["tl"], reduction=red)
        got, grad = A.ctc_loss_and_grad(dl, r["tokens"], r["ml"], r["tl"], reduction=red)
        x = dl.clone().requires_grad_()
        tr = A.ctc_loss_trainable(x, r["tokens"], r["ml"], r["tl"], reduction=red)
        assert tr.requires_grad
        for v in (got, tr.detach()):
            assert v.dtype == want.dtype and v.shape == want.shape and v.device == want.device and torch.equal(v, want), red
        w = A.ctc_reduction_weights(torch.tensor(r["tl"]), red)
        err = float((grad.cpu().double() - r["g64"] * w[:, None, None]).abs().max())
        assert err <= max(2 * r["e_case"], FLOOR) * float(w.max()), (red, err)


@pytest.mark.parametrize("name", ["b3t23", "ragged_t_eq_n"])
def test_autograd_the_trainers_lines(name):
    """trainer.py:61-63 and 69 on the device with A.CTCLoss() and torch's log_softmax, against the same lines on the CPU in fp64 with
    torch.nn.CTCLoss(); then ctc_loss_trainable under every reduction with a random grad_output.  All of it inside
    torch.use_deterministic_algorithms(True), where torch's own device CTC backward raises."""
    r = _results(name)
    logits, tokens, ml, tl = r["logits"], r["tokens"], r["ml"], r["tl"]
    B = len(ml)
    bound = max(2 * r["e_case"], FLOOR)
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        x64 = logits.double().requires_grad_()
        pred64 = x64.transpose(0, 1).log_softmax(2)
        loss64 = torch.nn.CTCLoss()(pred64, tokens, torch.tensor(ml), torch.tensor(tl))
        loss64.backward()
        x = logits.to(DEV).requires_grad_()
        pred = x.transpose(0, 1).log_softmax(2)
        loss = A.CTCLoss()(pred, tokens.to(DEV), torch.tensor(ml, device=DEV), torch.tensor(tl, device=DEV))
        assert loss.dtype == torch.float32 and loss.dim() == 0 and not torch.isnan(loss) and not torch.isinf(loss)
        loss.backward()
        wmax = 1.0 / (min(tl) * B)
        err = float((x.grad.cpu().double() - x64.grad).abs().max())
        print(f"CTCGRAD trainer lines {name}: loss {loss.item():.6f} (fp64 {loss64.item():.6f}), leaf gradient max abs err {err:.3e}, bound "
              f"{bound * wmax:.3e}")
        assert abs(loss.item() - loss64.item()) <= 1e-5 * abs(loss64.item()) and err <= bound * wmax
        for i, red in enumerate(("mean", "sum", "none")):
            go = _weights(B, 50 + i) if red == "none" else _weights(1, 50 + i).reshape(())
            _, (want,) = _yardstick(logits, tokens, ml, tl, [go], reduction=red)
            _, got = _device(logits, tokens, ml, tl, go, red)
            w_eff = A.ctc_reduction_weights(torch.tensor(tl), red) * go
            err = float((got.double() - want).abs().max())
            print(f"CTCGRAD trainable {name} {red}: max abs err {err:.3e}, bound {bound * float(w_eff.abs().max()):.3e}")
            assert err <= bound * float(w_eff.abs().max()), (red, err)
    finally:
        torch.use_deterministic_algorithms(was)


def _raw(dl, tokens, ml, tl, w=None, zero_infinity=0):
    """parrot_ctc_loss_grad itself -> (status, nll, grad)"""
    lib = _lib.lib()
    B, T, V = dl.shape
    N = tokens.shape[1]
    nll = torch.empty(B, dtype=torch.float64, device=DEV)
    grad = torch.empty((B, T, V), dtype=torch.float32, device=DEV)
    n_ws = int(lib.parrot_ctc_grad_workspace_bytes(B, T, V, N))
    ws = torch.empty(n_ws, dtype=torch.uint8, device=DEV)
    td, mld, tld = tokens.to(DEV), torch.tensor(ml, dtype=torch.int32, device=DEV), torch.tensor(tl, dtype=torch.int32, device=DEV)
    wd = None if w is None else w.to(DEV, torch.float64)
    _lib.check(lib.parrot_ctc_loss_grad(A.dptr(dl), A.dptr(td), A.dptr(mld), A.dptr(tld), B, T, V, N, A.dptr(wd), zero_infinity, A.dptr(nll),
                                        A.dptr(grad), A.dptr(ws), n_ws, A.stream_ptr(torch.device(DEV))))
    return int(ws[:4].view(torch.int32).item()), nll.cpu(), grad.cpu()


def test_errors():
    """No fault is produced on purpose: every case is one of the forward's status paths, refused before a kernel could read
    through the bad value."""
    r = _results("b3t23")
    logits, tokens, ml, tl = r["logits"], r["tokens"], r["ml"], r["tl"]
    V, T = 21, 23
    dl = logits.to(DEV)
    bad = tokens.clone()
    bad[1, 2] = V  # a token == V inside the length
    for fn in (A.ctc_loss_and_grad, A.ctc_loss_trainable):
        with pytest.raises(ValueError, match="token"):
            fn(dl, bad, ml, tl)
        with pytest.raises(ValueError, match="mel_len"):
            fn(dl, tokens, [23, T + 1, 23], tl)
        x = dl.clone()
        x[2, 22, 7] = float("nan")  # the last real frame of row 2
        with pytest.raises(FloatingPointError, match="logit"):
            fn(x, tokens, ml, tl)
        with pytest.raises(_lib.ParrotHipError) as e:  # N over the limit
            fn(dl[:1], torch.ones((1, A.MAX_TOKENS + 1), dtype=torch.int64), [23], [3])
        assert e.value.code == -5
    # the entry point itself: a null row_weight is all ones; the bad row alone is NaN throughout, the call's other rows are computed
    status, nll, grad = _raw(dl, tokens, ml, tl)
    assert status == 0 and torch.equal(grad, r["g1"]) and nll.numpy().tobytes() == r["nll"].numpy().tobytes()
    status, nll, grad = _raw(dl, tokens, ml, tl, r["w"])
    assert status == 0 and torch.equal(grad, r["gw"])
    for zi in (0, 1):
        status, nll, grad = _raw(dl, bad, ml, tl, None, zi)
        assert status == 9 and math.isnan(nll[1].item()) and torch.isnan(grad[1]).all()
        assert torch.equal(grad[[0, 2]], r["g1"][[0, 2]]) and torch.equal(nll[[0, 2]], r["nll"][[0, 2]])
    status, nll, grad = _raw(dl, tokens, [23, 0, 23], tl)  # a bad length: that row is NaN throughout, the length is not used
    assert status == 9 and torch.isnan(grad[1]).all() and torch.equal(grad[[0, 2]], r["g1"][[0, 2]])
    lib = _lib.lib()
    assert lib.parrot_ctc_loss_grad(A.dptr(dl), None, None, None, 3, T, V, 5, None, 0, None, None, None, 0, None) == -1
    # and the library is fine afterwards
    _, again = A.ctc_loss_and_grad(dl, tokens, ml, tl, reduction="none")
    assert torch.equal(again.cpu(), r["g1"])


def test_whole_file_under_poison():
    """This file once more in a child process under PARROT_POISON_WS=nan: a kernel reading a byte of the workspace or of an
    output that nobody wrote would turn a gradient into NaN there, and an element of the gradient that nobody wrote stays NaN (the
    tests above compare the positions of the expected NaNs of a row without a path exactly, so poison cannot hide there)."""
    if os.environ.get("PARROT_POISON_WS"):
        return  # (already a poisoned run: the tests above were it)
    env = dict(os.environ, PARROT_POISON_WS="nan")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", os.path.abspath(__file__), "-k", "not whole_file"], cwd=ROOT,
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
