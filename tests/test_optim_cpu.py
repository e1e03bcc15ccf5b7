"""CPU: the fused AdamW's specification and host side -- the fp32 rule of tests/adamw_ref.py against its fp64 restatement and
against torch.optim.AdamW(foreach=False), the host half of the rule (parrot_tts_amd.optim.step_scalars), the C entry point's
refusals (all of them before any HIP call: there is no device here), and FusedAdamW's construction, state-dict interchange with
torch.optim.AdamW and refusals."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import adamw_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from parrot_tts_amd import _lib, optim  # noqa: E402

N, STEPS = 200_000, 10


@pytest.mark.parametrize("lr,b1,b2,wd", R.HYPER)
def test_fp32_rule_against_fp64_and_torch(lr, b1, b2, wd):
    """After every step the largest absolute error of the rule's parameters against fp64 is at most twice torch's own: the two are
    roundings of one formula in different orders, so the factor is margin.  exp_avg and exp_avg_sq are held to the number format (torch
    may form exp_avg with a fused multiply-add, one rounding where the rule has two, so twice its error is no bound there)."""
    p0, gs = R.problem(N, 11, STEPS)
    p, m, v = p0.copy(), np.zeros(N, R.F), np.zeros(N, R.F)
    p64, m64, v64 = p0.astype(np.float64), np.zeros(N), np.zeros(N)
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.AdamW([tp], lr=lr, betas=(b1, b2), eps=R.EPS, weight_decay=wd, foreach=False)
    G = max(float(np.abs(g).max()) for g in gs)
    for k, g in enumerate(gs, 1):
        p, m, v = R.step(p, g, m, v, lr, b1, b2, R.EPS, wd, k)
        p64, m64, v64 = R.step64(p64, g, m64, v64, lr, b1, b2, R.EPS, wd, k)
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        st = opt.state[tp]
        for name, ours, ref, theirs in (("p", p, p64, tp.detach().numpy()), ("m", m, m64, st["exp_avg"].numpy()),
                                        ("v", v, v64, st["exp_avg_sq"].numpy())):
            e_ours, e_torch = np.abs(ours - ref).max(), np.abs(theirs.astype(np.float64) - ref).max()
            print(f"step {k} {name}: ours {e_ours:.3e} torch {e_torch:.3e}")
            if name == "p":
                assert e_ours <= 2 * e_torch, (k, name, e_ours, e_torch)
            else:  # from the number format: three (four) roundings a step of values <= 2 G (G^2), each at most 2^-24 relative
                assert e_ours <= (3 * 2 * G if name == "m" else 4 * G * G) * k * 2.0 ** -24, (k, name, e_ours)
    assert np.isfinite(p).all() and (v >= 0).all()


def test_step_scalars_are_the_reference_scalars():
    for lr, b1, b2, wd in R.HYPER + [(0.0, 0.0, 0.0, 0.0), (3e-4, 0.5, 0.9, 0.3)]:
        for step in (1, 2, 3, 10, 1000, 123456):
            got, want = optim.step_scalars(lr, b1, b2, R.EPS, wd, step), R.scalars(lr, b1, b2, R.EPS, wd, step)
            assert len(got) == 7 and all(type(x) is np.float32 for x in got)
            assert [x.tobytes() for x in got] == [x.tobytes() for x in want], (lr, b1, b2, wd, step)
    decay, w1, b2_, w2, e, ns, rs = optim.step_scalars(2e-4, 0.8, 0.99, 1e-8, 0.01, 1)
    assert decay == np.float32(1 - 2e-6) and w1 == np.float32(1 - 0.8) and b2_ == np.float32(0.99) and e == np.float32(1e-8)
    assert ns == np.float32(-2e-4 / (1 - 0.8)) and rs == np.float32(np.sqrt(1 - 0.99))


@pytest.fixture(scope="module")
def lib():
    from parrot_tts_amd import build
    build.build()
    return _lib.lib()


def test_symbols_struct_and_constants(lib):
    hdr = open(os.path.join(ROOT, "include", "parrot_hip.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("parrot_adamw_step", "parrot_adamw_chunk", "parrot_adamw_max_tensors"):
        assert hasattr(raw, n) and n in _lib.SIGNATURES and re.search(r"\b" + n + r"\s*\(", hdr), n
    assert "#define PARROT_ABI_VERSION 7" in hdr and _lib.ABI_VERSION == 7 and lib.parrot_abi_version() == 7
    assert ctypes.sizeof(_lib.AdamwTensor) == 48
    C, M = lib.parrot_adamw_chunk(), lib.parrot_adamw_max_tensors()
    assert C > 0 and C % 4 == 0
    # the by-value table (48 bytes a tensor and a 4-byte chunk prefix, the scalars, 64 bytes to spare) fills the 4 KB kernel argument
    assert 64 <= M and M * 52 <= 4096 < (M + 3) * 52


def _table(specs):
    arr = (_lib.AdamwTensor * max(len(specs), 1))()
    for k, s in enumerate(specs):
        arr[k] = _lib.AdamwTensor(*s)
    return arr


def test_refusals_happen_before_any_device_call(lib):
    buf = (ctypes.c_char * 4096)()
    p, g, m, v = (ctypes.addressof(buf) + o for o in (0, 1024, 2048, 3072))
    good = (p, g, m, v, 4, 1)
    hyper = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01)

    def call(specs, K=None, **kw):
        h = dict(hyper, **kw)
        return lib.parrot_adamw_step(_table(specs) if specs is not None else None, len(specs) if K is None else K, h["lr"], h["b1"], h["b2"],
                                     h["eps"], h["wd"], None)

    def refused(word, *a, **kw):
        assert call(*a, **kw) == -1
        msg = lib.parrot_last_error()
        assert msg and word in msg, (msg, word)

    refused(b"null tensor table", None, K=2)
    refused(b"negative K", [good], K=-1)
    for i in range(4):
        bad = list(good)
        bad[i] = 0
        refused(b"null pointer", [tuple(bad)])
    refused(b"negative n", [(p, g, m, v, -1, 1)])
    refused(b"step below 1", [(p, g, m, v, 4, 0)])
    refused(b"step below 1", [(p, g, m, v, 4, -3)])
    refused(b"negative lr", [good], lr=-1e-3)
    refused(b"negative eps", [good], eps=-1e-8)
    refused(b"negative weight_decay", [good], wd=-0.01)
    for name in ("b1", "b2"):
        for val in (-0.1, 1.0, 1.5, float("nan")):
            refused(b"beta" + name[1:].encode() + b" outside", [good], **{name: val})
    for i in range(4):
        for j in range(i + 1, 4):
            bad = list(good)
            bad[j] = bad[i]
            refused(b"alias", [tuple(bad)])
    # the second tensor is the bad one: the message names it; n == 0 does not excuse a null pointer
    refused(b"tensor 1", [good, (p, g, m, 0, 0, 1)])
    # nothing to do is not an error and needs no device: an empty table, and tensors without elements
    assert call([], K=0) == 0 and call(None, K=0) == 0
    assert call([(p, g, m, v, 0, 1), (p, g, m, v, 0, 7)]) == 0


def _params():
    gen = torch.Generator().manual_seed(3)
    return [torch.nn.Parameter(torch.randn(s, generator=gen)) for s in [(3, 5), (7,), ()]]


def test_constructs_on_cpu_with_torchs_keys_and_defaults():
    ours, theirs = optim.FusedAdamW(_params()), torch.optim.AdamW(_params())
    go, gt = ours.param_groups[0], theirs.param_groups[0]
    assert list(go) == list(gt)
    assert {k: v for k, v in go.items() if k != "params"} == {k: v for k, v in gt.items() if k != "params"}
    assert ours.defaults == theirs.defaults
    ours = optim.FusedAdamW([{"params": _params()[:1], "lr": 5e-4, "weight_decay": 0.0}, {"params": _params()[1:]}], 2e-4, betas=[0.8, 0.99])
    assert [g["lr"] for g in ours.param_groups] == [5e-4, 2e-4] and [g["weight_decay"] for g in ours.param_groups] == [0.0, 1e-2]
    assert ours.param_groups[1]["betas"] == torch.optim.AdamW(_params(), 2e-4, betas=[0.8, 0.99]).param_groups[0]["betas"]
    assert tuple(ours.param_groups[1]["betas"]) == (0.8, 0.99)
    with pytest.raises(ValueError):
        optim.FusedAdamW(_params(), lr=-1.0)
    with pytest.raises(ValueError):
        optim.FusedAdamW(_params(), betas=(0.9, 1.0))


def test_refusals_of_the_class():
    for kw in ({"amsgrad": True}, {"maximize": True}, {"capturable": True}, {"differentiable": True}, {"lr": torch.tensor(1e-3)}):
        with pytest.raises(NotImplementedError):
            optim.FusedAdamW(_params(), **kw)
    ps = _params()
    opt = optim.FusedAdamW(ps)
    for p in ps:
        p.grad = torch.ones_like(p)
    before = [p.detach().clone() for p in ps]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    assert all(torch.equal(a, p) for a, p in zip(before, ps)) and len(opt.state) == 0


def test_state_dicts_go_both_ways():
    # torch -> ours: two torch steps on the CPU, then the state loads with keys, dtypes and the step tensor as torch writes them
    ps_t = _params()
    theirs = torch.optim.AdamW(ps_t, 2e-4, betas=[0.8, 0.99], foreach=False)
    for _ in range(2):
        for p in ps_t:
            p.grad = torch.full_like(p, 0.25)
        theirs.step()
    sd = theirs.state_dict()
    ours = optim.FusedAdamW(_params(), 1e-3)
    ours.load_state_dict(sd)
    assert ours.param_groups[0]["lr"] == 2e-4 and tuple(ours.param_groups[0]["betas"]) == (0.8, 0.99)
    back = ours.state_dict()
    assert back["param_groups"] == sd["param_groups"]
    assert sorted(back["state"]) == sorted(sd["state"]) == [0, 1, 2]
    for k in sd["state"]:
        a, b = sd["state"][k], back["state"][k]
        assert list(a) == list(b) == ["step", "exp_avg", "exp_avg_sq"]
        for name in a:
            assert a[name].dtype == b[name].dtype == torch.float32 and a[name].device == b[name].device and torch.equal(a[name], b[name])
        assert b["step"].dim() == 0 and b["step"].device.type == "cpu" and float(b["step"]) == 2.0
    # ours -> torch: the reloaded optimiser goes on exactly as the original
    again = torch.optim.AdamW(_params(), 1e-3, foreach=False)
    again.load_state_dict(copy.deepcopy(back))  # (load_state_dict shares the tensors it is given)
    ps_a = again.param_groups[0]["params"]
    with torch.no_grad():
        for a, t in zip(ps_a, ps_t):
            a.copy_(t)
    for opt, ps in ((theirs, ps_t), (again, ps_a)):
        for p in ps:
            p.grad = torch.full_like(p, -0.5)
        opt.step()
    assert all(torch.equal(a, t) for a, t in zip(ps_a, ps_t))
    assert all(float(again.state[p]["step"]) == 3.0 for p in ps_a)


def test_lr_scheduler_drives_it():
    opt = optim.FusedAdamW(_params(), 2e-4)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.999)
    ref = torch.optim.AdamW(_params(), 2e-4)
    sched_ref = torch.optim.lr_scheduler.ExponentialLR(ref, gamma=0.999)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (scheduler.step() before optimizer.step(): nothing steps on the CPU)
        for _ in range(3):
            sched.step()
            sched_ref.step()
    assert opt.param_groups[0]["lr"] == ref.param_groups[0]["lr"] != 2e-4
    assert sched.get_last_lr() == sched_ref.get_last_lr()
