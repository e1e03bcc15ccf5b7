"""GPU: the fused multi-tensor AdamW (parrot_tts_amd.optim.FusedAdamW over parrot_adamw_step).

The kernel's yardstick is tests/adamw_ref.py, the update rule in numpy float32 op by op: p, exp_avg and exp_avg_sq are equal to it
BIT FOR BIT, at every size around the chunk, across the launch boundary of a group with more tensors than one launch's table
holds, for views at any 4-byte offset (with sentinels on both sides), with subnormal, huge, zero, inf and nan gradients.  Against
torch.optim.AdamW(foreach=False) on the device the rule is the CPU test's: the parameters' largest absolute error against the fp64
restatement is at most twice torch's own (two roundings of one formula in different orders; the factor is margin); exp_avg and
exp_avg_sq, bit-equal to the rule already, are held to a bound from the number format."""
import functools

import numpy as np
import pytest
import torch

import adamw_ref as R

pytestmark = pytest.mark.gpu

from parrot_tts_amd import _lib  # noqa: E402
from parrot_tts_amd.optim import FusedAdamW  # noqa: E402

DEV = "cuda:0"
GROUP_A = dict(lr=2e-4, betas=(0.8, 0.99), eps=R.EPS, weight_decay=0.01)
GROUP_B = dict(lr=1e-3, betas=(0.9, 0.999), eps=R.EPS, weight_decay=0.0)


@functools.lru_cache(maxsize=None)
def _consts():
    lib = _lib.lib()
    return int(lib.parrot_adamw_chunk()), int(lib.parrot_adamw_max_tensors())


def _bits(x):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x
    return np.ascontiguousarray(x, dtype=np.float32).reshape(-1).view(np.uint32)


def _grad(rng, n, special=True):
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 0, n)).astype(np.float32)
    g[::7] = 0
    if special and n >= 3:
        g[1], g[2] = 1e-41, 1e18  # a subnormal and a square near the top of the range
    return g


class _Ref:
    """adamw_ref over a list of tensors with torch's bookkeeping: a tensor without a gradient is untouched and its step lags."""

    def __init__(self, p0, hyper):
        self.p = [x.copy() for x in p0]
        self.m = [np.zeros_like(x) for x in p0]
        self.v = [np.zeros_like(x) for x in p0]
        self.step = [0] * len(p0)
        self.hyper = hyper  # per tensor

    def update(self, grads, lr_scale=1.0):
        for i, g in enumerate(grads):
            if g is None:
                continue
            self.step[i] += 1
            h = self.hyper[i]
            self.p[i], self.m[i], self.v[i] = R.step(self.p[i], g, self.m[i], self.v[i], h["lr"] * lr_scale, *h["betas"], h["eps"],
                                                      h["weight_decay"], self.step[i])


def _assert_state_bits(opt, params, ref, where=""):
    for i, p in enumerate(params):
        st = opt.state[p]
        if ref.step[i] == 0:
            assert len(st) == 0, (where, i)
            assert np.array_equal(_bits(p), _bits(ref.p[i])), (where, i, "p untouched")
            continue
        assert float(st["step"]) == ref.step[i] and st["step"].device.type == "cpu" and st["step"].dtype == torch.float32, (where, i)
        for name, got, want in (("p", p, ref.p[i]), ("m", st["exp_avg"], ref.m[i]), ("v", st["exp_avg_sq"], ref.v[i])):
            assert np.array_equal(_bits(got), _bits(want)), (where, i, name, p.numel())


def test_bit_equal_to_the_rule_over_sizes_groups_and_launches():
    C, M = _consts()
    rng = np.random.default_rng(5)
    sizes_a = [1, 2, 3, 4, 5, C - 1, C, C + 1, 2 * C + 3]
    sizes_b = [1 + (k % 9) for k in range(M)] + [C + 5]  # M + 1 tensors: two launches, the chunk-crossing one in the second
    assert len(sizes_b) == M + 1
    shapes = [(n,) for n in sizes_a + sizes_b]
    shapes[8], shapes[3] = (2 * C + 3, 1), (2, 1, 2)
    p0 = [(rng.standard_normal(s) * 10.0 ** rng.uniform(-3, 0, s)).astype(np.float32) for s in shapes]
    params = [torch.nn.Parameter(torch.from_numpy(x.copy()).to(DEV)) for x in p0]
    na = len(sizes_a)
    opt = FusedAdamW([dict(params=params[:na], **GROUP_A), dict(params=params[na:], **GROUP_B)])
    ref = _Ref([x.reshape(-1) for x in p0], [GROUP_A] * na + [GROUP_B] * len(sizes_b))
    lagging = (6, na + 3)  # a tensor of each group has no gradient in steps 2 and 3
    for k in range(1, 6):
        grads = [None if (i in lagging and k in (2, 3)) else _grad(rng, x.size) for i, x in enumerate(p0)]
        for p, g in zip(params, grads):
            p.grad = None if g is None else torch.from_numpy(g.copy()).to(DEV).reshape(p.shape)
        opt.step()
        torch.cuda.synchronize()
        ref.update(grads)
        _assert_state_bits(opt, params, ref, where=f"step {k}")
        for p, g in zip(params, grads):  # g is read only
            assert g is None or np.array_equal(_bits(p.grad), _bits(g))
    assert [ref.step[i] for i in lagging] == [3, 3] and ref.step[0] == 5


def test_gradient_before_first_step_missing_and_nonfinite_gradients():
    C, _ = _consts()
    rng = np.random.default_rng(6)
    sizes = [7, C + 9, 33]
    p0 = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    params = [torch.nn.Parameter(torch.from_numpy(x.copy()).to(DEV)) for x in p0]
    opt = FusedAdamW(params, **GROUP_A)
    ref = _Ref(p0, [GROUP_A] * 3)
    for k in range(1, 4):
        grads = [_grad(rng, n) for n in sizes]
        if k == 1:
            grads[2] = None  # never stepped so far: no state yet
        if k == 2:
            grads[0][4], grads[1][C + 2], grads[1][17] = np.inf, np.nan, -np.inf
        for p, g in zip(params, grads):
            p.grad = None if g is None else torch.from_numpy(g.copy()).to(DEV)
        opt.step()
        torch.cuda.synchronize()
        ref.update(grads)
        for i, p in enumerate(params):
            if ref.step[i] == 0:
                assert len(opt.state[p]) == 0 and np.array_equal(_bits(p), _bits(p0[i]))
                continue
            st = opt.state[p]
            for name, got, want in (("p", p, ref.p[i]), ("m", st["exp_avg"], ref.m[i]), ("v", st["exp_avg_sq"], ref.v[i])):
                got = got.detach().cpu().numpy()
                fin = np.isfinite(want)
                assert np.array_equal(np.isfinite(got), fin), (k, i, name)  # the same elements non-finite as in the reference
                assert np.array_equal(_bits(got[fin]), _bits(want[fin])), (k, i, name)
    bad = ~np.isfinite(ref.p[0])
    assert bad.sum() == 1 and bad[4] and (~np.isfinite(ref.p[1])).sum() == 2


OFFSETS = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 2, 0, 0), (0, 0, 3, 0), (0, 0, 0, 1), (1, 2, 3, 1), (3, 3, 3, 3), (2, 1, 0, 3)]
SENTINEL = 12345.678


def test_views_at_any_offset_touch_nothing_outside_and_agree_with_the_aligned_run():
    """p, g, exp_avg and exp_avg_sq are views at element offsets 0 .. 3 of larger buffers filled with a sentinel: the results are
    those of the aligned run (and of the rule) bit for bit, every sentinel and every gradient is unchanged."""
    C, _ = _consts()
    rng = np.random.default_rng(7)
    sizes = [5, C + 3, 2 * C + 1, 4 * 5, C]
    pad = 8
    results = []
    for offs in OFFSETS:
        rng_run = np.random.default_rng(70)
        bufs = [[torch.full((n + 2 * pad,), SENTINEL, device=DEV) for n in sizes] for _ in range(4)]  # p, g, m, v
        view = lambda which, i: bufs[which][i][offs[which]:offs[which] + sizes[i]]  # noqa: E731
        p0 = [rng_run.standard_normal(n).astype(np.float32) for n in sizes]
        params = []
        for i, n in enumerate(sizes):
            view(0, i).copy_(torch.from_numpy(p0[i]))
            view(2, i).zero_()
            view(3, i).zero_()
            params.append(torch.nn.Parameter(view(0, i)))
            assert params[-1].data_ptr() == bufs[0][i].data_ptr() + 4 * offs[0]
        opt = FusedAdamW(params, **GROUP_A)
        for i, p in enumerate(params):
            opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": view(2, i), "exp_avg_sq": view(3, i)}
        ref = _Ref(p0, [GROUP_A] * len(sizes))
        for k in range(1, 4):
            grads = [_grad(rng_run, n) for n in sizes]
            for i, p in enumerate(params):
                view(1, i).copy_(torch.from_numpy(grads[i]))
                p.grad = view(1, i)
            opt.step()
            torch.cuda.synchronize()
            ref.update(grads)
            for i in range(len(sizes)):
                assert np.array_equal(_bits(view(1, i)), _bits(grads[i])), (offs, k, i, "gradient changed")
        _assert_state_bits(opt, params, ref, where=str(offs))
        for which in range(4):
            for i, n in enumerate(sizes):
                b, o = bufs[which][i], offs[which]
                assert bool((b[:o] == SENTINEL).all()) and bool((b[o + n:] == SENTINEL).all()), (offs, which, i, "sentinel overwritten")
        results.append([np.concatenate([_bits(view(w, i)) for w in (0, 2, 3)]) for i in range(len(sizes))])
    for offs, res in zip(OFFSETS[1:], results[1:]):
        for a, b in zip(results[0], res):
            assert np.array_equal(a, b), offs
    del rng


def _errs(params, states, ref64):
    """max |x - fp64| of p, exp_avg, exp_avg_sq."""
    p64, m64, v64 = ref64
    f = lambda t: t.detach().cpu().numpy().astype(np.float64).reshape(-1)  # noqa: E731
    return [float(np.abs(f(a) - b).max()) for a, b in ((params, p64), (states["exp_avg"], m64), (states["exp_avg_sq"], v64))]


def _assert_moments_within_format_bound(errs, gs):
    """exp_avg and exp_avg_sq after len(gs) steps against fp64, from the number format alone (the 2 x torch rule is for p: torch
    forms exp_avg with one fused rounding where the rule has two, so its error there can be legitimately half of ours).  With
    G = max |g| over the steps, |m| <= G and v <= G^2; a step of m is three roundings of values <= 2 G (subtract, multiply, add), a
    step of v four of values <= G^2, each at most 2^-24 relative; beta < 1 does not grow what was there."""
    G, k = max(float(np.abs(g).max()) for g in gs), len(gs)
    assert errs[1] <= 3 * k * 2.0 ** -24 * 2 * G, errs[1]
    assert errs[2] <= 4 * k * 2.0 ** -24 * G * G, errs[2]


@pytest.mark.parametrize("lr,b1,b2,wd", R.HYPER)
def test_against_torch_on_the_device_with_a_scheduler(lr, b1, b2, wd):
    n, gamma = 100_003, 0.9
    p0, gs = R.problem(n, 21, 5)
    ours_p, torch_p = (torch.nn.Parameter(torch.from_numpy(p0.copy()).to(DEV)) for _ in range(2))
    ours = FusedAdamW([ours_p], lr, betas=(b1, b2), eps=R.EPS, weight_decay=wd)
    theirs = torch.optim.AdamW([torch_p], lr, betas=(b1, b2), eps=R.EPS, weight_decay=wd, foreach=False)
    scheds = [torch.optim.lr_scheduler.ExponentialLR(o, gamma=gamma) for o in (ours, theirs)]
    ref64 = (p0.astype(np.float64), np.zeros(n), np.zeros(n))
    epoch = 0
    for k, g in enumerate(gs, 1):
        lr_now = ours.param_groups[0]["lr"]
        assert lr_now == theirs.param_groups[0]["lr"] and lr_now == pytest.approx(lr * gamma ** epoch, rel=1e-12)
        for o, p in ((ours, ours_p), (theirs, torch_p)):
            p.grad = torch.from_numpy(g.copy()).to(DEV)
            o.step()
        ref64 = R.step64(*ref64[:1], g, *ref64[1:], lr_now, b1, b2, R.EPS, wd, k)
        e_ours, e_torch = _errs(ours_p, ours.state[ours_p], ref64), _errs(torch_p, theirs.state[torch_p], ref64)
        print(f"step {k} lr {lr_now:.3e}: ours {e_ours} torch {e_torch}")
        assert e_ours[0] <= 2 * e_torch[0], (k, e_ours[0], e_torch[0])
        _assert_moments_within_format_bound(e_ours, gs[:k])
        if k <= 3:  # three "epochs"
            for s in scheds:
                s.step()
            epoch += 1
    assert epoch == 3 and ours.param_groups[0]["lr"] == pytest.approx(lr * gamma ** 3, rel=1e-12)


@pytest.mark.parametrize("first", ["torch", "ours"])
def test_state_interchange(first):
    """Two steps of one class, state_dict -> load_state_dict of the other, two more steps: held against four torch steps by the
    same rule."""
    lr, b1, b2, wd = R.HYPER[0]
    n = 50_001
    p0, gs = R.problem(n, 22, 4)
    kw = dict(lr=lr, betas=(b1, b2), eps=R.EPS, weight_decay=wd)
    make = {"torch": lambda p: torch.optim.AdamW([p], foreach=False, **kw), "ours": lambda p: FusedAdamW([p], **kw)}
    second = "ours" if first == "torch" else "torch"

    def run(p, opt, grads):
        for g in grads:
            p.grad = torch.from_numpy(g.copy()).to(DEV)
            opt.step()

    p_mixed = torch.nn.Parameter(torch.from_numpy(p0.copy()).to(DEV))
    opt1 = make[first](p_mixed)
    run(p_mixed, opt1, gs[:2])
    opt2 = make[second](p_mixed)
    opt2.load_state_dict(opt1.state_dict())
    st = opt2.state[p_mixed]
    assert float(st["step"]) == 2.0 and st["step"].device.type == "cpu" and st["exp_avg"].device.type == "cuda"
    run(p_mixed, opt2, gs[2:])
    assert float(opt2.state[p_mixed]["step"]) == 4.0
    p_torch = torch.nn.Parameter(torch.from_numpy(p0.copy()).to(DEV))
    opt_t = make["torch"](p_torch)
    run(p_torch, opt_t, gs)
    ref64 = (p0.astype(np.float64), np.zeros(n), np.zeros(n))
    for k, g in enumerate(gs, 1):
        ref64 = R.step64(*ref64[:1], g, *ref64[1:], lr, b1, b2, R.EPS, wd, k)
    e_mixed, e_torch = _errs(p_mixed, opt2.state[p_mixed], ref64), _errs(p_torch, opt_t.state[p_torch], ref64)
    print(f"{first} then {second}: {e_mixed} torch {e_torch}")
    assert e_mixed[0] <= 2 * e_torch[0], (e_mixed[0], e_torch[0])
    _assert_moments_within_format_bound(e_mixed, gs)


def _one_run(deterministic):
    C, M = _consts()
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(deterministic)
    try:
        rng = np.random.default_rng(31)
        sizes = [3, C + 1, 3 * C + 2] + [11] * M
        params = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(DEV)) for n in sizes]
        opt = FusedAdamW(params, **GROUP_A)
        for _ in range(3):
            for p in params:
                p.grad = torch.from_numpy(_grad(rng, p.numel())).to(DEV)
            opt.step()
        torch.cuda.synchronize()
        return [np.concatenate([_bits(p), _bits(opt.state[p]["exp_avg"]), _bits(opt.state[p]["exp_avg_sq"])]) for p in params]
    finally:
        torch.use_deterministic_algorithms(prev)


def test_two_runs_agree_bit_for_bit_also_in_deterministic_mode():
    a, b, c = _one_run(False), _one_run(False), _one_run(True)
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and np.array_equal(x, z)


def test_noncontiguous_gradient_sparse_gradient_and_wrong_parameters():
    p = torch.nn.Parameter(torch.randn(6, 5, device=DEV))
    q = torch.nn.Parameter(p.detach().clone())
    g = torch.randn(5, 6, device=DEV).t()
    assert not g.is_contiguous()
    a, b = FusedAdamW([p], **GROUP_A), FusedAdamW([q], **GROUP_A)
    p.grad, q.grad = g, g.contiguous()
    a.step()
    b.step()
    assert torch.equal(p, q) and torch.equal(p.grad, g)
    s = torch.nn.Parameter(torch.randn(4, 3, device=DEV))
    s.grad = torch.zeros(4, 3, device=DEV).to_sparse()
    with pytest.raises(RuntimeError, match="sparse"):
        FusedAdamW([s]).step()
    h = torch.nn.Parameter(torch.randn(4, device=DEV, dtype=torch.float16))
    h.grad = torch.zeros_like(h)
    with pytest.raises(RuntimeError, match="fp32"):
        FusedAdamW([h]).step()
    nc = torch.nn.Parameter(torch.randn(5, 6, device=DEV).t())
    nc.grad = torch.zeros_like(nc)
    with pytest.raises(RuntimeError, match="contiguous"):
        FusedAdamW([nc]).step()
