"""GPU: ModelLoss's gradient on the device (parrot_tts_amd.loss.ModelLoss.loss_and_grad / forward with a graph, over
parrot_tte_loss_grad).

The yardstick is the reference's own operator (modules/loss.py:12-21 as tests/teacher_forced_ref.py::model_loss) on the CPU in fp64,
through autograd, backward of w_code code_loss + w_dur dur_loss.  Errors are measured in normalised units, in which the gradient is
softmax - onehot and the log-duration difference: |delta| n_valid / |w_code| for grad_logits and |delta| n_src / (2 |w_dur|) for
grad_log_dur.  Per case e_case is the error of torch's CPU fp32 autograd against that fp64 run in the same units (unit weights),
and the device stays within

    grad_logits:   max(2 e_case, 2^-24 (32 + D_case)),   D_case the largest max - min of a row of the case's logits
    grad_log_dur:  max(2 e_case, 2^-22 (1 + max |log_dur| + max log(dur + 1)))

The second term is the worst case of the fp32 evaluation: rounding x - m costs 2^-24 D in the exponent, and expf (2 ulp), the
16-term lane sum with the 6-level tree (22 ulp), the reciprocal, the scale and the final rounding stay under 32 ulp of a
probability <= 1.  For the durations: one rounding each of logf, the subtraction and the product, relative to the magnitudes
subtracted.  Measured (MI355X): DESIGN.md section 3, "ModelLoss gradient".

The whole file also passes under PARROT_POISON_WS=nan (workspace and outputs filled with NaN at the top of the entry point)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import tte_loss_grad_ref as R
from teacher_forced_ref import model_loss

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from parrot_tts_amd import _lib  # noqa: E402
from parrot_tts_amd.loss import ModelLoss, _loss_call  # noqa: E402
from parrot_tts_amd.ops import dptr, stream_ptr  # noqa: E402

DEV = "cuda:0"
WEIGHTS = ((1.0, 1.0), (0.7, -1.3), (0.0, 2.0))
REF_WEIGHTS = WEIGHTS + ((2.0, 0.5),)  # (test_autograd's second backward: 2 code + 0.5 dur)


def _make(seed, N, V, gain, src_lens, S, ignored=(), equal_row=None):
    """-> dict(out (N, V) f32, batch {codes (N), src_mask / duration (len(src_lens), S)}, log_dur, V), on the CPU."""
    gen = torch.Generator().manual_seed(seed)
    out = torch.randn((N, V), generator=gen) * gain
    if equal_row is not None:
        out[equal_row] = 0.5  # every logit equal: p = 1 / V
    codes = torch.randint(0, V, (N,), generator=gen)
    for lo, hi in ignored:
        codes[lo:hi] = V
    batch = {"codes": codes, "src_mask": torch.arange(S)[None, :] < torch.tensor(src_lens)[:, None],
             "duration": torch.randint(0, 6, (len(src_lens), S), generator=gen)}
    return {"out": out, "batch": batch, "log_dur": torch.randn((len(src_lens), S), generator=gen), "V": V}


def _v1000():
    # B = 5, L = 37 flattened (tests/test_gpu_teacher_forced.py's shape): each row's tail from 30, row 1 from 5, and the whole
    # third 16-row block (32 .. 47) ignored
    ign = [(b * 37 + 30, (b + 1) * 37) for b in range(5)] + [(37 + 5, 74), (32, 48)]
    return _make(1, 185, 1000, 3.0, [9, 4, 7, 1, 8], 9, ign, equal_row=3)


CASES = {
    "v1000": _v1000,                                                                      # vector path, the last chunk partial
    "v1024": lambda: _make(2, 17, 1024, 1.0, [3, 5], 5, [(4, 7)]),                          # all four chunks full; the second block holds one row
    "v4": lambda: _make(3, 16, 4, 6.0, [2, 1, 4], 4, [(0, 1), (9, 12)]),                    # one float4, 63 idle lanes, exactly one block
    "v37": lambda: _make(4, 12, 37, 3.0, [4, 2], 4, [(10, 12)], equal_row=1),               # generic path, odd V
    "v1028": lambda: _make(5, 33, 1028, 6.0, [6, 1, 3], 6, [(15, 18), (32, 33)]),           # V % 4 == 0 but over the register path
    "offset": lambda: _make(6, 20, 1000, 20.0, [5, 2], 5, [(0, 3), (19, 20)]),              # base not 16-byte aligned; gain 20: most p underflow
    "single": lambda: _make(7, 1, 1000, 1.0, [3], 4),                                       # a single row
}


def _gpu(c):
    """The case on the device; "offset": the logits are a view one float into their storage."""
    out = c["out"].to(DEV)
    if c.get("offset"):
        buf = torch.empty(out.numel() + 1, device=DEV)
        buf[1:].copy_(out.reshape(-1))
        out = buf[1:].view(out.shape)
        assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out, c["log_dur"].to(DEV), {k: v.to(DEV) for k, v in c["batch"].items()}


def _autograd(c, dtype, w):
    x, ld = c["out"].clone().to(dtype).requires_grad_(), c["log_dur"].clone().to(dtype).requires_grad_()
    _, code, dur = R.model_loss_typed(x, ld, c["batch"], c["V"])  # (model_loss itself in fp32; see there for fp64)
    (w[0] * code + w[1] * dur).backward()
    return x.grad.double(), ld.grad.double()


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case, torch's fp64 gradients per weight pair, and the two bounds (computed once, shared, never modified)."""
    c = CASES[name]()
    c["offset"] = name == "offset"
    c["n_valid"] = int((c["batch"]["codes"] != c["V"]).sum())
    c["n_src"] = int(c["batch"]["src_mask"].sum())
    c["ref"] = {w: _autograd(c, torch.float64, w) for w in REF_WEIGHTS}
    g32, d32 = _autograd(c, torch.float32, WEIGHTS[0])
    e_logits = float((g32 - c["ref"][WEIGHTS[0]][0]).abs().max()) * c["n_valid"]
    e_dur = float((d32 - c["ref"][WEIGHTS[0]][1]).abs().max()) * c["n_src"] / 2.0
    D = float((c["out"].max(dim=1).values - c["out"].min(dim=1).values).max())
    c["e_case"] = (e_logits, e_dur)
    c["bound_logits"] = max(2.0 * e_logits, 2.0 ** -24 * (32.0 + D))
    c["bound_dur"] = max(2.0 * e_dur, 2.0 ** -22 * (1.0 + float(c["log_dur"].abs().max())
                                                    + float(torch.log(c["batch"]["duration"].float() + 1).max())))
    return c


def _loss(c):
    return ModelLoss({"preprocess": {"hubert_codes": c["V"]}})


def _raw(c, w=None, grad_logits=True, grad_log_dur=True, codes=None):
    """parrot_tte_loss_grad (or, without a gradient, parrot_tte_loss) on the case -> (sums, losses, grad_logits, grad_log_dur)."""
    out, log_dur, batch = _gpu(c)
    if codes is not None:
        batch = dict(batch, codes=codes.to(DEV))
    a = _loss(c)._args(out, log_dur, batch)
    assert a[0].data_ptr() == out.data_ptr()  # (no copy: the offset case keeps its misaligned base)
    wt = None if w is None else torch.tensor(w, dtype=torch.float64, device=DEV)
    return _loss_call(a, wt, grad_logits, grad_log_dur)


def _errors(c, w, g_logits, g_dur):
    """The two errors against torch's fp64 autograd, each already multiplied out so that it compares with bound x |w|."""
    ref_g, ref_d = c["ref"][w]
    return (float((g_logits.double().cpu() - ref_g).abs().max()) * c["n_valid"],
            float((g_dur.double().cpu() - ref_d).abs().max()) * c["n_src"] / 2.0)


@pytest.mark.parametrize("name", list(CASES))
def test_gradients_against_torch_fp64_autograd(name):
    c = _case(name)
    for w in WEIGHTS:
        _, _, g, d = _raw(c, w)
        assert g.dtype == torch.float32 and g.shape == c["out"].shape and d.shape == c["log_dur"].shape
        e_g, e_d = _errors(c, w, g, d)
        print(f"TTELOSSGRAD {name} N {c['out'].shape[0]} V {c['V']} w {w}: grad_logits err {e_g:.3e} (bound {c['bound_logits'] * abs(w[0]):.3e}, "
              f"e_case {c['e_case'][0]:.3e}), grad_log_dur err {e_d:.3e} (bound {c['bound_dur'] * abs(w[1]):.3e}, e_case {c['e_case'][1]:.3e})")
        assert e_g <= c["bound_logits"] * abs(w[0]), (name, w)   # (w_code = 0: a zero gradient, exactly)
        assert e_d <= c["bound_dur"] * abs(w[1]), (name, w)
    # the numpy restatement says the same as torch
    r = R.tte_loss_and_grad(c["out"].numpy(), c["batch"]["codes"].numpy(), c["V"], c["log_dur"].numpy(), c["batch"]["duration"].numpy(),
                            c["batch"]["src_mask"].numpy(), WEIGHTS[1])
    assert float(np.abs(r["grad_logits"] - c["ref"][WEIGHTS[1]][0].numpy()).max()) <= 1e-12


@pytest.mark.parametrize("name", list(CASES))
def test_bits(name):
    """The forward's bits, two calls, ignored rows and masked durations exactly 0, and each output alone."""
    c = _case(name)
    w = WEIGHTS[1]
    sums0, losses0, _, _ = _raw(c, None, False, False)  # parrot_tte_loss
    sums, losses, g, d = _raw(c, w)
    assert torch.equal(sums, sums0) and torch.equal(losses, losses0)
    assert int(sums[1]) == c["n_valid"] and int(sums[4]) == c["n_src"] and int(sums[5]) == 0
    sums2, losses2, g2, d2 = _raw(c, w)
    assert torch.equal(sums2, sums) and torch.equal(losses2, losses) and torch.equal(g2, g) and torch.equal(d2, d)
    ign = (c["batch"]["codes"] == c["V"]).to(DEV)
    assert not g[ign].any() and bool(torch.isfinite(g).all())
    assert (c["out"].shape[0] <= 4) == (int(ign.sum()) == 0)  # every case with N > 4 has ignored rows
    assert not d[~c["batch"]["src_mask"].to(DEV)].any()
    sums3, losses3, g3, none = _raw(c, w, True, False)
    assert none is None and torch.equal(g3, g) and torch.equal(sums3, sums) and torch.equal(losses3, losses)
    sums4, losses4, none, d4 = _raw(c, w, False, True)
    assert none is None and torch.equal(d4, d) and torch.equal(sums4, sums) and torch.equal(losses4, losses)


def test_a_rows_bits_do_not_depend_on_the_rows_beside_it():
    c = _case("v1000")
    _, _, g, _ = _raw(c, WEIGHTS[1])
    perm = torch.randperm(185, generator=torch.Generator().manual_seed(9))
    p = dict(c, out=c["out"][perm], batch=dict(c["batch"], codes=c["batch"]["codes"][perm]))
    sums, _, gp, _ = _raw(p, WEIGHTS[1])
    assert int(sums[1]) == c["n_valid"]
    assert torch.equal(gp, g[perm.to(DEV)])


def test_nothing_valid_gives_nan_losses_and_zero_gradients():
    c = _case("v37")
    out, log_dur, batch = _gpu(c)
    loss = _loss(c)
    empty = dict(batch, codes=torch.full_like(batch["codes"], c["V"]), src_mask=torch.zeros_like(batch["src_mask"]))
    res, g, d = loss.loss_and_grad(out, log_dur, empty)
    assert all(bool(torch.isnan(v)) for v in res) and not g.any() and not d.any()
    assert loss.last_stats["n_valid"] == 0 and loss.last_stats["n_src"] == 0
    # one of the two alone: the other half is as before
    full, g_full, d_full = loss.loss_and_grad(out, log_dur, batch)
    res, g, d = loss.loss_and_grad(out, log_dur, dict(batch, codes=empty["codes"]))
    assert bool(torch.isnan(res[0])) and bool(torch.isnan(res[1])) and torch.equal(res[2], full[2]) and not g.any() and torch.equal(d, d_full)
    res, g, d = loss.loss_and_grad(out, log_dur, dict(batch, src_mask=empty["src_mask"]))
    assert bool(torch.isnan(res[0])) and bool(torch.isnan(res[2])) and torch.equal(res[1], full[1]) and not d.any() and torch.equal(g, g_full)


@pytest.mark.parametrize("name", ["v1000", "v37"])
def test_a_target_out_of_range(name):
    c = _case(name)
    out, log_dur, batch = _gpu(c)
    row = 7  # a valid row of both cases
    assert int(c["batch"]["codes"][row]) != c["V"]
    bad = c["batch"]["codes"].clone()
    bad[row] = c["V"] + 3
    with pytest.raises(IndexError, match=f"Target {c['V'] + 3} is out of bounds"):
        _loss(c).loss_and_grad(out, log_dur, dict(batch, codes=bad.to(DEV)))
    sums, _, g, d = _raw(c, None, codes=bad)
    assert int(sums[5]) == 1 and int(sums[6]) == c["V"] + 3 and int(sums[1]) == c["n_valid"] - 1
    assert bool(torch.isnan(g[row]).all())
    others = torch.arange(g.shape[0], device=DEV) != row
    assert bool(torch.isfinite(g[others]).all()) and bool(torch.isfinite(d).all())
    neg = c["batch"]["codes"].clone()
    neg[row] = -1
    sums, _, g, _ = _raw(c, None, codes=neg)
    assert int(sums[5]) == 1 and bool(torch.isnan(g[row]).all()) and bool(torch.isfinite(g[others]).all())


def _check_autograd(c, got_out, got_dur, w, what):
    e_g, e_d = _errors(c, w, got_out.reshape(c["out"].shape), got_dur)
    print(f"TTELOSSGRAD autograd {what}: grad_logits err {e_g:.3e}, grad_log_dur err {e_d:.3e}")
    assert e_g <= c["bound_logits"] * abs(w[0]) and e_d <= c["bound_dur"] * abs(w[1]), what


@pytest.mark.parametrize("deterministic", [False, True])
def test_autograd(deterministic):
    c = _case("v1000")
    out, log_dur, batch = _gpu(c)
    out3 = out.reshape(5, 37, c["V"])  # (B, L, V), as Parrot.forward returns it
    batch = dict(batch, codes=batch["codes"].reshape(5, 37))
    loss = _loss(c)
    torch.use_deterministic_algorithms(deterministic)
    try:
        plain = loss(out3, log_dur, batch)
        assert all(not v.requires_grad and v.grad_fn is None for v in plain)
        x, ld = out3.clone().requires_grad_(), log_dur.clone().requires_grad_()
        res = loss(x, ld, batch)
        assert all(v.requires_grad and v.dim() == 0 and v.dtype == torch.float32 for v in res)
        assert all(torch.equal(a.detach(), b) for a, b in zip(res, plain))
        res[0].backward()
        assert x.grad.shape == x.shape and x.grad.dtype == torch.float32 and ld.grad.shape == ld.shape
        _check_autograd(c, x.grad, ld.grad, (1.0, 1.0), "loss.backward()")
        first = x.grad.clone()
        x.grad, ld.grad = None, None
        _, code, dur = loss(x, ld, batch)
        (2 * code + 0.5 * dur).backward()
        _check_autograd(c, x.grad, ld.grad, (2.0, 0.5), "(2 code + 0.5 dur).backward()")
        _, g_direct, d_direct = loss.loss_and_grad(out3, log_dur, batch)
        assert torch.equal(g_direct, first) and g_direct.shape == out3.shape and d_direct.shape == log_dur.shape
        with torch.no_grad():  # grad mode off: the plain path whatever the inputs require
            assert all(not v.requires_grad for v in loss(x, ld, batch))
        # only log_dur requires grad: out gets none (and the kernel a null pointer)
        x2, ld2 = out3.clone(), log_dur.clone().requires_grad_()
        loss(x2, ld2, batch)[0].backward()
        assert x2.grad is None and torch.equal(ld2.grad, d_direct)
        x3, ld3 = out3.clone().requires_grad_(), log_dur.clone()
        loss(x3, ld3, batch)[0].backward()
        assert ld3.grad is None and torch.equal(x3.grad, first)
        # bf16 inputs give bf16 gradients: the fp32 gradient of the bf16 values, rounded once
        xb, lb = out3.to(torch.bfloat16).requires_grad_(), log_dur.to(torch.bfloat16).requires_grad_()
        loss(xb, lb, batch)[0].backward()
        assert xb.grad.dtype == torch.bfloat16 and lb.grad.dtype == torch.bfloat16 and xb.grad.shape == xb.shape
        _, g_b, d_b = loss.loss_and_grad(xb.detach().float(), lb.detach().float(), batch)
        assert torch.equal(xb.grad, g_b.to(torch.bfloat16)) and torch.equal(lb.grad, d_b.to(torch.bfloat16))
    finally:
        torch.use_deterministic_algorithms(False)


def test_a_torch_built_head_trains_on_it():
    """nn.Linear heads over random features: one backward through ModelLoss, one through torch's model_loss.  1e-5 relative to the
    parameter's largest gradient entry: 40 times the normalised per-element bound above, for the fp32 matmul backward both share."""
    torch.manual_seed(11)
    V = 40
    feats, enc = torch.randn(2, 9, 16, device=DEV), torch.randn(2, 5, 16, device=DEV)
    head, dp = nn.Linear(16, V).to(DEV), nn.Linear(16, 1).to(DEV)
    codes = torch.randint(0, V, (2, 9), device=DEV)
    codes[1, 6:] = V
    batch = {"codes": codes, "src_mask": (torch.arange(5)[None, :] < torch.tensor([5, 3])[:, None]).to(DEV),
             "duration": torch.randint(0, 6, (2, 5), device=DEV)}
    params = list(head.parameters()) + list(dp.parameters())
    grads = []
    for fn in (ModelLoss({"preprocess": {"hubert_codes": V}}), lambda o, d, b: model_loss(o, d, b, V)):
        for p in params:
            p.grad = None
        loss = fn(head(feats), dp(enc).squeeze(-1), batch)[0]
        loss.backward()
        grads.append([p.grad.clone() for p in params])
    for ours, want in zip(*grads):
        err, scale = float((ours - want).abs().max()), float(want.abs().max())
        print(f"TTELOSSGRAD head parameter {tuple(want.shape)}: err {err:.3e}, largest entry {scale:.3e}")
        assert err <= 1e-5 * scale


def test_raw_call_refusals():
    c = _case("v4")
    out, log_dur, batch = _gpu(c)
    a = _loss(c)._args(out, log_dur, batch)
    lib = _lib.lib()
    sums, ws = torch.empty(8, dtype=torch.float64, device=DEV), torch.empty(4096, dtype=torch.uint8, device=DEV)
    call = lambda g, d, n_ws: lib.parrot_tte_loss_grad(dptr(a[0]), dptr(a[1]), 16, 4, 4, dptr(a[2]), dptr(a[3]), dptr(a[4]), a[4].numel(), None,  # noqa: E731
                                                       dptr(sums), None, dptr(g), dptr(d), dptr(ws), n_ws, stream_ptr(torch.device(DEV)))
    assert call(None, None, 4096) == -1
    assert call(a[0], None, 4096) == -1  # grad_logits aliases logits
    assert call(torch.empty_like(a[0]), None, 8) == -4 and b"workspace" in lib.parrot_last_error()
    assert call(torch.empty_like(a[0]), torch.empty_like(a[2]), 4096) == 0  # and the library is fine afterwards


def test_whole_file_under_poison():
    """This file once more in a child process under PARROT_POISON_WS=nan: a kernel reading a byte of the workspace or of an output
    that nobody wrote would turn a result into NaN there, and an element of a gradient that nobody wrote stays NaN (the tests above
    require the zeros of ignored rows exactly and every other element finite, so poison cannot hide)."""
    if os.environ.get("PARROT_POISON_WS"):
        return  # (already a poisoned run: the tests above were it)
    env = dict(os.environ, PARROT_POISON_WS="nan")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", os.path.abspath(__file__), "-k", "not whole_file"], cwd=ROOT,
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
