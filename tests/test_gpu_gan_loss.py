"""GPU: the vocoder's adversarial losses on the device (parrot_tts_amd.gan_loss over parrot_gan_loss).

The yardstick is torch on the CPU in fp64 on the same fp32 inputs: the plain expressions mean |a - b|, mean (1 - a)^2, mean a^2 and
their autograd.  Bounds:

    term_out[k]      |err| <= (n_k + 4) 2^-52 ref: each fp64 contribution carries at most 3 roundings and a sum of n non-negative fp64
                     values in any order is within n 2^-53 relative
    total            == np.float32(scale * sum of term_out in table order), bit for bit
    L1 gradients     one magnitude per term, bit for bit, within 2^-23 relative of |w_k| / n_k; the sign exactly sgn(b - a), exactly 0
                     where a == b; grad_a == -grad_b bit for bit
    square gradients |err| <= 2^-23 |ref| per element: one fp32 rounding of an fp64 product whose operand order may differ from
                     torch's by an fp64 ulp

Measured (MI355X): DESIGN.md section 3, "GAN losses".  The whole file also passes under PARROT_POISON_WS=nan (workspace, term_out,
total and every gradient buffer filled with NaN at the top of the entry point)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import gan_loss_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from parrot_tts_amd import _lib, gan_loss  # noqa: E402
from parrot_tts_amd.gan_loss import L1, SQ0, SQ1, _call  # noqa: E402
from parrot_tts_amd.ops import dptr, stream_ptr  # noqa: E402

DEV = "cuda:0"
MIXED = (0.7, -1.3, 0.0, 2.0, -0.25)  # term k gets MIXED[k % 5]: both signs and a zero


@functools.lru_cache(maxsize=None)
def _tile():
    return int(_lib.lib().parrot_gan_loss_tile())


def _term(gen, op, n, shape=None, offset=False, equal=()):
    """One term on the CPU: dict(op, a, b (None for the squares), offset).  ``equal``: flat indices where b is set to a."""
    shape = (n,) if shape is None else shape
    a = torch.randn(shape, generator=gen) * 1.5
    b = None
    if op == L1:
        b = torch.randn(shape, generator=gen)
        for i in equal:
            b.reshape(-1)[i] = a.reshape(-1)[i]
    return {"op": op, "a": a, "b": b, "offset": offset}


def _shapes_case():
    T = _tile()
    gen = torch.Generator().manual_seed(101)
    terms = [_term(gen, op, n) for n in (1, 3, 4, 5, T - 1, T, T + 1, 3 * T + 5) for op in (L1, SQ1, SQ0)]
    terms.append(_term(gen, L1, T + 7, offset=True))          # a is a view one float into its storage
    terms.append(_term(gen, SQ0, 2 * T + 2, offset=True))
    terms.append(_term(gen, L1, 1000, equal=(0, 1, 7, 500, 998, 999)))
    return terms


def _reference_case(B=2, T=2048):
    """The 62 terms of a generator step at the discriminators' shapes, in generator_adversarial_loss's order."""
    gen = torch.Generator().manual_seed(202)
    mpd, msd = R.mpd_shapes(B, T), R.msd_shapes(B, T)
    assert T % 3 and T % 5 and T % 7 and T % 11  # (the reflect-padded period lengths)
    terms = [_term(gen, SQ1, 0, R.score_shape(d[-1])) for d in msd] + [_term(gen, SQ1, 0, R.score_shape(d[-1])) for d in mpd]
    terms += [_term(gen, L1, 0, s, equal=(0,)) for d in msd + mpd for s in d]
    assert len(terms) == 62
    return terms


def _split_case():
    """PARROT_GAN_MAX_TERMS + 6 terms: the call splits into two launches."""
    T = _tile()
    gen = torch.Generator().manual_seed(303)
    ns = (T + 1, 5, 2 * T, 1, 777, T - 1, 4)
    return [_term(gen, (L1, SQ1, SQ0)[k % 3], ns[k % len(ns)]) for k in range(_lib.GAN_MAX_TERMS + 6)]


def _stride_case():
    """One term of (grid cap + 1) tiles: the stride loop runs twice for workgroup 0."""
    gen = torch.Generator().manual_seed(404)
    return [_term(gen, L1, (_lib.GAN_GRID_CAP + 1) * _tile(), equal=(5, 4097))]


def _single_case():
    gen = torch.Generator().manual_seed(505)
    return [_term(gen, SQ1, 2 * _tile() + 3)]


CASES = {"shapes": _shapes_case, "reference62": _reference_case, "split": _split_case, "stride": _stride_case, "single": _single_case}


def _ref_term(t, w):
    """torch CPU fp64 on the fp32 inputs -> (value, grad_a, grad_b) of w * term."""
    x = t["a"].double().requires_grad_()
    y = t["b"].double().requires_grad_() if t["op"] == L1 else None
    v = (x - y).abs().mean() if t["op"] == L1 else (((1 - x) ** 2).mean() if t["op"] == SQ1 else (x ** 2).mean())
    (w * v).backward()
    return float(v.detach()), x.grad, None if y is None else y.grad


def _fp32_value(t):
    a, b = t["a"], t["b"]
    return float((a - b).abs().mean() if t["op"] == L1 else (((1 - a) ** 2).mean() if t["op"] == SQ1 else (a ** 2).mean()))


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case with its device tensors and torch's fp64 values (computed once, shared, never modified)."""
    terms = CASES[name]()
    for t in terms:
        for key in ("a", "b"):
            src = t[key]
            if src is None:
                t[key + "_dev"] = None
                continue
            if t["offset"] and key == "a":
                buf = torch.empty(src.numel() + 1, device=DEV)
                buf[1:].copy_(src.reshape(-1))
                t["a_dev"] = buf[1:].view(src.shape)
                assert t["a_dev"].data_ptr() % 16 == 4 and t["a_dev"].is_contiguous()
            else:
                t[key + "_dev"] = src.to(DEV)
        t["n"] = t["a"].numel()
        t["ref"] = _ref_term(t, 1.0)[0]
    return terms


def _flat(terms):
    return [x for t in terms for x in ((t["a_dev"], t["b_dev"]) if t["op"] == L1 else (t["a_dev"],))]


def _raw(terms, w="ones", scale=1.0, values=True, grads=True):
    """One parrot_gan_loss call -> (term_out, total, [(grad_a, grad_b)] per term).  w: "ones", "mixed" or None (a null pointer)."""
    ops = [t["op"] for t in terms]
    flat = _flat(terms)
    wt = None
    if w == "ones":
        wt = torch.ones(len(ops), dtype=torch.float64, device=DEV)
    elif w == "mixed":
        wt = torch.tensor([MIXED[k % 5] for k in range(len(ops))], dtype=torch.float64, device=DEV)
    term_out, total, g = _call(ops, flat, [True] * len(flat) if grads else None, wt, scale, values)
    it = iter(g)
    return term_out, total, [(next(it), next(it) if t["op"] == L1 else None) for t in terms]


def _bits(x):
    return x.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[x.element_size()])


def _same(x, y):
    """Bit for bit (NaN == NaN, +0 != -0)."""
    return x.shape == y.shape and x.dtype == y.dtype and bool(torch.equal(_bits(x), _bits(y)))


def _check_values(name, terms, term_out, total, scale):
    got = term_out.cpu().numpy()
    worst = 0.0
    for k, t in enumerate(terms):
        ref = t["ref"]
        err, bound = abs(got[k] - ref), (t["n"] + 4) * 2.0 ** -52 * ref
        e32 = abs(_fp32_value(t) - ref)
        if k < 6 or err > bound:
            print(f"GANLOSS {name} term {k} op {t['op']} n {t['n']}: {got[k]:.17g} err {err:.3e} (bound {bound:.3e}); torch fp32 err {e32:.3e}")
        worst = max(worst, err / ref)
        assert err <= bound, (name, k)
    print(f"GANLOSS {name}: K {len(terms)}, worst relative value error {worst:.3e}")
    want = np.float32(scale * sum(got.tolist()))
    assert total.dtype == torch.float32 and total.dim() == 0
    assert np.float32(total.item()).tobytes() == want.tobytes(), (name, total.item(), want)


def _check_grads(name, terms, grads, w):
    worst_l1, worst_sq = 0.0, 0.0
    for k, (t, (ga, gb)) in enumerate(zip(terms, grads)):
        wk = 1.0 if w in ("ones", None) else MIXED[k % 5]
        assert ga.dtype == torch.float32 and ga.shape == t["a"].shape
        if t["op"] == L1:
            a, b, g = t["a"].double(), t["b"].double(), gb.cpu()
            assert _same(ga, -gb), (name, k)                                  # grad_a == -grad_b, bit for bit
            sign = torch.sign(b - a)
            mags = torch.unique(g[sign != 0].abs())
            if wk == 0.0:
                assert not g.any() and not ga.any(), (name, k)                # that term's gradient is exactly 0
                continue
            assert bool((g[sign == 0] == 0).all()), (name, k)                 # a == b: exactly 0
            if not bool((sign != 0).any()):
                continue
            assert mags.numel() == 1, (name, k, mags)                         # one magnitude per term
            want = abs(wk) / t["n"]
            rel = abs(float(mags[0].double()) - want) / want
            worst_l1 = max(worst_l1, rel)
            assert rel <= 2.0 ** -23, (name, k, rel)
            assert bool(torch.equal(g.double(), sign * float(mags[0]) * (1.0 if wk > 0 else -1.0))), (name, k)  # the sign: sgn(b - a)
        else:
            assert gb is None
            _, ref, _ = _ref_term(t, wk)
            d = (ga.cpu().double() - ref).abs()
            if wk == 0.0:
                assert not ga.any(), (name, k)
                continue
            ok = d <= 2.0 ** -23 * ref.abs()
            worst_sq = max(worst_sq, float((d / ref.abs().clamp_min(1e-300)).max()))
            assert bool(ok.all()), (name, k, float(d.max()))
    print(f"GANLOSS {name} w {w}: worst L1 magnitude error {worst_l1:.3e}, worst squares element error {worst_sq:.3e} (bound {2.0 ** -23:.3e}, relative)")


@pytest.mark.parametrize("name", list(CASES))
def test_values_and_gradients_against_torch_fp64(name):
    terms = _case(name)
    for w, scale in (("ones", 1.0), ("mixed", 2.0), (None, 0.5)):
        if name == "stride" and w == "mixed":
            continue  # (one term: MIXED[0] alone adds nothing to "ones" at 130 MB a call)
        term_out, total, grads = _raw(terms, w, scale)
        _check_values(name, terms, term_out, total, scale)
        _check_grads(name, terms, grads, w)
        assert all(bool(torch.isfinite(g).all()) for pair in grads for g in pair if g is not None)


@pytest.mark.parametrize("name", ["shapes", "reference62", "split", "single"])
def test_bits(name):
    """Two calls; values-only, gradients-only and fused calls; the table reversed and permuted."""
    terms = _case(name)
    term_out, total, grads = _raw(terms, "mixed", 2.0)
    t2, tot2, g2 = _raw(terms, "mixed", 2.0)
    assert _same(t2, term_out) and _same(tot2, total)
    assert all(_same(x, y) for p, q in zip(g2, grads) for x, y in zip(p, q) if x is not None)
    tv, totv, gv = _raw(terms, "mixed", 2.0, values=True, grads=False)
    assert _same(tv, term_out) and _same(totv, total) and all(x is None for p in gv for x in p)
    tn, totn, gn = _raw(terms, "mixed", 2.0, values=False, grads=True)
    assert tn is None and totn is None
    assert all(_same(x, y) for p, q in zip(gn, grads) for x, y in zip(p, q) if x is not None)
    # a term's bits do not depend on its place in the table: same weight, another position
    K = len(terms)
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(9)).tolist()
    for order in (list(range(K))[::-1], perm):
        sub = [terms[k] for k in order]
        wt = torch.tensor([MIXED[k % 5] for k in order], dtype=torch.float64, device=DEV)
        flat = _flat(sub)
        to, _, g = _call([t["op"] for t in sub], flat, [True] * len(flat), wt, 2.0, True)
        it = iter(g)
        for pos, k in enumerate(order):
            assert _same(to[pos], term_out[k]), (name, k)
            assert _same(next(it), grads[k][0]), (name, k)
            if terms[k]["op"] == L1:
                assert _same(next(it), grads[k][1]), (name, k)


def test_a_term_alone_has_the_bits_it_has_among_the_62():
    terms = _case("reference62")
    term_out, _, grads = _raw(terms, "mixed", 1.0)
    for k, t in enumerate(terms):
        wt = torch.tensor([MIXED[k % 5]], dtype=torch.float64, device=DEV)
        flat = _flat([t])
        to, total, g = _call([t["op"]], flat, [True] * len(flat), wt, 1.0, True)
        assert _same(to[0], term_out[k]) and _same(g[0], grads[k][0]), k
        assert t["op"] != L1 or _same(g[1], grads[k][1]), k
        assert np.float32(total.item()).tobytes() == np.float32(to[0].item()).tobytes()


def test_an_empty_term_is_nan_and_leaves_the_others_alone():
    terms = _case("shapes")[:9]
    term_out, _, grads = _raw(terms, "mixed", 1.0)
    empty = {"op": SQ0, "a_dev": torch.empty(0, device=DEV), "b_dev": None, "a": torch.empty(0), "b": None}
    with_empty = terms[:4] + [empty] + terms[4:]
    ops = [t["op"] for t in with_empty]
    flat = _flat(with_empty)
    wt = torch.tensor([MIXED[k % 5] for k in range(4)] + [1.0] + [MIXED[k % 5] for k in range(4, 9)], dtype=torch.float64, device=DEV)
    to, total, g = _call(ops, flat, [True] * len(flat), wt, 1.0, True)
    assert bool(torch.isnan(to[4])) and bool(torch.isnan(total))
    assert _same(torch.cat([to[:4], to[5:]]), term_out)
    it = iter(g)
    for k, t in enumerate(with_empty):
        ga = next(it)
        gb = next(it) if t["op"] == L1 else None
        if k == 4:
            assert ga.numel() == 0
            continue
        want = grads[k if k < 4 else k - 1]
        assert _same(ga, want[0]) and (gb is None or _same(gb, want[1]))
    # through the public functions: torch's mean of nothing
    loss, ls = gan_loss.generator_loss([terms[1]["a_dev"], torch.empty(0, device=DEV)])
    assert bool(torch.isnan(loss)) and bool(torch.isnan(ls[1])) and bool(torch.isfinite(ls[0]))


def test_nonfinite_inputs_propagate_as_in_torch():
    gen = torch.Generator().manual_seed(606)
    a, b = torch.randn(300, generator=gen), torch.randn(300, generator=gen)
    a[7], b[9], a[11] = float("nan"), float("inf"), float("-inf")
    terms = [{"op": L1, "a": a, "b": b, "a_dev": a.to(DEV), "b_dev": b.to(DEV)}, {"op": SQ1, "a": b, "b": None, "a_dev": b.to(DEV), "b_dev": None},
             {"op": SQ0, "a": a[20:], "b": None, "a_dev": a[20:].to(DEV), "b_dev": None}]
    term_out, total, grads = _raw(terms, "ones", 1.0)
    assert bool(torch.isnan(term_out[0])) and bool(torch.isinf(term_out[1])) and bool(torch.isfinite(term_out[2])) and bool(torch.isnan(total))
    _, ga, gb = _ref_term(terms[0], 1.0)  # torch: sgn(NaN) = 0, sgn(+-inf) = +-1
    assert bool(torch.equal(grads[0][0].cpu().double(), ga.float().double())) and bool(torch.equal(grads[0][1].cpu().double(), gb.float().double()))
    _, ga, _ = _ref_term(terms[1], 1.0)
    assert bool(torch.equal(torch.isinf(grads[1][0].cpu()), torch.isinf(ga))) and float(grads[1][0][9]) == float("inf")


# ---------------------------------------------------------------------------------------------
# the public functions
# ---------------------------------------------------------------------------------------------
def _nested(dtype=torch.float32, seed=77):
    """Two "period" and two "scale" discriminators' outputs at small odd shapes, on the device."""
    gen = torch.Generator().manual_seed(seed)
    mk = lambda s: torch.randn(s, generator=gen).to(DEV, dtype)  # noqa: E731
    f_shapes = [[(2, 3, 7, 2), (2, 5, 4, 2), (2, 1, 9, 2)], [(2, 4, 5, 3), (2, 1, 11, 3)]]
    s_shapes = [[(2, 8, 33), (2, 1, _tile() + 3)], [(2, 6, 17), (2, 1, 9)]]
    d = {}
    for key, shapes in (("f", f_shapes), ("s", s_shapes)):
        d[f"fmap_{key}_r"] = [[mk(s) for s in dd] for dd in shapes]
        d[f"fmap_{key}_g"] = [[mk(s) for s in dd] for dd in shapes]
        d[f"y_d{key}_hat_r"] = [mk(R.score_shape(dd[-1])) for dd in shapes]
        d[f"y_d{key}_hat_g"] = [mk(R.score_shape(dd[-1])) for dd in shapes]
    return d


def _req(nest):
    return [[t.clone().requires_grad_() for t in d] if isinstance(d, list) else d.clone().requires_grad_() for d in nest]


def _leaves(nest):
    return [t for d in nest for t in (d if isinstance(d, list) else [d])]


def _raw_grads(ops, flat, w):
    """The raw gradients-only call with every weight w[k] -> gradients in ``flat``'s order."""
    dense = [t.detach().float().contiguous() for t in flat]
    wt = torch.tensor(w, dtype=torch.float64, device=DEV)
    return _call(ops, dense, [True] * len(dense), wt, 1.0, False)[2]


UP = float(np.float32(0.37))  # a non-unit upstream gradient, as the fp32 value autograd carries


@pytest.mark.parametrize("deterministic", [False, True])
def test_autograd(deterministic):
    d = _nested()
    torch.use_deterministic_algorithms(deterministic)
    try:
        # --- feature_loss
        plain = gan_loss.feature_loss(d["fmap_f_r"], d["fmap_f_g"])
        assert plain.dim() == 0 and plain.dtype == torch.float32 and not plain.requires_grad and plain.grad_fn is None
        pairs = [(r, g) for dr, dg in zip(d["fmap_f_r"], d["fmap_f_g"]) for r, g in zip(dr, dg)]
        flat = [t for p in pairs for t in p]
        for up in (1.0, UP):
            fr, fg = _req(d["fmap_f_r"]), _req(d["fmap_f_g"])
            loss = gan_loss.feature_loss(fr, fg)
            assert loss.requires_grad and loss.grad_fn is not None and _same(loss.detach(), plain)
            (loss if up == 1.0 else up * loss).backward()
            want = _raw_grads([L1] * len(pairs), flat, [2.0 * up] * len(pairs))
            got = [t.grad for p in zip(_leaves(fr), _leaves(fg)) for t in p]
            assert all(_same(x, y.reshape(x.shape)) for x, y in zip(got, want)), up
        with torch.no_grad():
            assert not gan_loss.feature_loss(_req(d["fmap_f_r"]), _req(d["fmap_f_g"])).requires_grad
        fr, fg = _req(d["fmap_f_r"]), _req(d["fmap_f_g"])
        gan_loss.feature_loss(fr, fg, detach_real=True).backward()
        assert all(t.grad is None for t in _leaves(fr)) and all(t.grad is not None for t in _leaves(fg))
        unit = _raw_grads([L1] * len(pairs), flat, [2.0] * len(pairs))
        assert all(_same(t.grad, w.reshape(t.shape)) for t, w in zip(_leaves(fg), unit[1::2]))
        # only the real side requires grad: the generated side gets none
        fr = _req(d["fmap_f_r"])
        gan_loss.feature_loss(fr, d["fmap_f_g"]).backward()
        assert all(_same(t.grad, w.reshape(t.shape)) for t, w in zip(_leaves(fr), unit[0::2]))
        # --- generator_loss
        ys = d["y_df_hat_g"] + d["y_ds_hat_g"]
        plain, ls = gan_loss.generator_loss(ys)
        assert not plain.requires_grad and len(ls) == len(ys) and all(v.dim() == 0 and v.dtype == torch.float32 and not v.requires_grad for v in ls)
        for up in (1.0, UP):
            yq = _req(ys)
            loss, ls_q = gan_loss.generator_loss(yq)
            assert loss.requires_grad and _same(loss.detach(), plain) and all(not v.requires_grad and _same(v, u) for v, u in zip(ls_q, ls))
            (loss if up == 1.0 else up * loss).backward()
            want = _raw_grads([SQ1] * len(ys), ys, [up] * len(ys))
            assert all(_same(t.grad, w.reshape(t.shape)) for t, w in zip(yq, want)), up
        with torch.no_grad():
            assert not gan_loss.generator_loss(_req(ys))[0].requires_grad
        # --- discriminator_loss
        plain, r_l, g_l = gan_loss.discriminator_loss(d["y_df_hat_r"], d["y_df_hat_g"])
        assert not plain.requires_grad and all(type(v) is float for v in r_l + g_l) and len(r_l) == len(g_l) == 2
        for up in (1.0, UP):
            yr, yg = _req(d["y_df_hat_r"]), _req(d["y_df_hat_g"])
            loss, r_q, g_q = gan_loss.discriminator_loss(yr, yg)
            assert loss.requires_grad and _same(loss.detach(), plain) and r_q == r_l and g_q == g_l
            (loss if up == 1.0 else up * loss).backward()
            flat_d = [t for p in zip(d["y_df_hat_r"], d["y_df_hat_g"]) for t in p]
            want = _raw_grads([SQ1, SQ0] * 2, flat_d, [up] * 4)
            got = [t.grad for p in zip(yr, yg) for t in p]
            assert all(_same(x, y.reshape(x.shape)) for x, y in zip(got, want)), up
        with torch.no_grad():
            assert not gan_loss.discriminator_loss(_req(d["y_df_hat_r"]), _req(d["y_df_hat_g"]))[0].requires_grad
        # --- generator_adversarial_loss
        keys = ("y_df_hat_g", "y_ds_hat_g", "fmap_f_r", "fmap_f_g", "fmap_s_r", "fmap_s_g")
        plain, parts = gan_loss.generator_adversarial_loss(*[d[k] for k in keys])
        assert plain.dim() == 0 and plain.dtype == torch.float32 and not plain.requires_grad
        assert sorted(parts) == ["loss_fm_f", "loss_fm_s", "loss_gen_f", "loss_gen_s"] and all(not v.requires_grad and v.dim() == 0 for v in parts.values())
        fused, parts_f, g_fused = gan_loss.generator_adversarial_loss_and_grad(*[d[k] for k in keys])
        assert _same(fused, plain) and all(_same(parts_f[k], parts[k]) for k in parts) and len(g_fused) == 6
        for up in (1.0, UP):
            args = [_req(d[k]) for k in keys]
            loss, parts_q = gan_loss.generator_adversarial_loss(*args)
            assert loss.requires_grad and _same(loss.detach(), plain) and all(not v.requires_grad and _same(v, parts[k]) for k, v in parts_q.items())
            (loss if up == 1.0 else up * loss).backward()
            ops, flat_g, c, _ = gan_loss._generator_table(*[d[k] for k in keys], False)
            want = _raw_grads(ops, flat_g, [up * ck for ck in c])
            _, flat_q, _, _ = gan_loss._generator_table(*args, False)
            assert all(_same(t.grad, w.reshape(t.shape)) for t, w in zip(flat_q, want)), up
            if up == 1.0:
                for nest_q, nest_g in zip(args, g_fused):
                    assert all(_same(t.grad, g) for t, g in zip(_leaves(nest_q), _leaves(nest_g)))
        args = [_req(d[k]) for k in keys]
        gan_loss.generator_adversarial_loss(*args, detach_real=True)[0].backward()
        assert all(t.grad is None for k, a in zip(keys, args) if k.endswith("_r") for t in _leaves(a))
        assert all(_same(t.grad, g) for k, a, gs in zip(keys, args, g_fused) if not k.endswith("_r") for t, g in zip(_leaves(a), _leaves(gs)))
        _, _, g_det = gan_loss.generator_adversarial_loss_and_grad(*[d[k] for k in keys], detach_real=True)
        assert g_det[2] is None and g_det[4] is None and all(_same(x, y) for i in (0, 1, 3, 5) for x, y in zip(_leaves(g_det[i]), _leaves(g_fused[i])))
        with torch.no_grad():
            assert not gan_loss.generator_adversarial_loss(*[_req(d[k]) for k in keys])[0].requires_grad
        # --- discriminator_adversarial_loss
        keys = ("y_df_hat_r", "y_df_hat_g", "y_ds_hat_r", "y_ds_hat_g")
        plain, parts = gan_loss.discriminator_adversarial_loss(*[d[k] for k in keys])
        assert plain.dim() == 0 and not plain.requires_grad and sorted(parts) == ["loss_disc_f", "loss_disc_s"]
        fused, parts_f, g_fused = gan_loss.discriminator_adversarial_loss_and_grad(*[d[k] for k in keys])
        assert _same(fused, plain) and all(_same(parts_f[k], parts[k]) for k in parts) and len(g_fused) == 4
        for up in (1.0, UP):
            args = [_req(d[k]) for k in keys]
            loss, _ = gan_loss.discriminator_adversarial_loss(*args)
            assert loss.requires_grad and _same(loss.detach(), plain)
            (loss if up == 1.0 else up * loss).backward()
            ops, flat_d, c, _ = gan_loss._discriminator_table(*[d[k] for k in keys])
            want = _raw_grads(ops, flat_d, [up] * len(ops))
            _, flat_q, _, _ = gan_loss._discriminator_table(*args)
            assert all(_same(t.grad, w.reshape(t.shape)) for t, w in zip(flat_q, want)), up
            if up == 1.0:
                for nest_q, nest_g in zip(args, g_fused):
                    assert all(_same(t.grad, g) for t, g in zip(nest_q, nest_g))
        with torch.no_grad():
            assert not gan_loss.discriminator_adversarial_loss(*[_req(d[k]) for k in keys])[0].requires_grad
        # --- bf16 inputs give bf16 gradients: the fp32 gradient of the upcast values, rounded once
        fr = [[t.to(torch.bfloat16).requires_grad_() for t in dd] for dd in d["fmap_f_r"]]
        fg = [[t.to(torch.bfloat16).requires_grad_() for t in dd] for dd in d["fmap_f_g"]]
        yb = [t.to(torch.bfloat16).requires_grad_() for t in ys]
        (gan_loss.feature_loss(fr, fg) + gan_loss.generator_loss(yb)[0]).backward()
        flat_b = [t for p in zip(_leaves(fr), _leaves(fg)) for t in p]
        want = _raw_grads([L1] * len(pairs), flat_b, [2.0] * len(pairs))
        assert all(t.grad.dtype == torch.bfloat16 and t.grad.shape == t.shape and _same(t.grad, w.reshape(t.shape).to(torch.bfloat16)) for t, w in zip(flat_b, want))
        want = _raw_grads([SQ1] * len(yb), yb, [1.0] * len(yb))
        assert all(t.grad.dtype == torch.bfloat16 and _same(t.grad, w.reshape(t.shape).to(torch.bfloat16)) for t, w in zip(yb, want))
    finally:
        torch.use_deterministic_algorithms(False)


class _TinyDisc(nn.Module):
    """A small Conv1d / leaky-ReLU stack in the reference discriminators' pattern: forward -> (score, fmaps).  No biases and no
    parameter under 192 entries: see test_a_torch_built_discriminator_trains_on_it."""

    def __init__(self):
        super().__init__()
        self.convs = nn.ModuleList([nn.Conv1d(1, 32, 15, 1, padding=7, bias=False), nn.Conv1d(32, 64, 21, 2, groups=4, padding=10, bias=False),
                                    nn.Conv1d(64, 64, 5, 2, padding=2, bias=False)])
        self.conv_post = nn.Conv1d(64, 1, 3, 1, padding=1, bias=False)

    def forward(self, x):
        fmap = []
        for layer in self.convs:
            x = F.leaky_relu(layer(x), 0.1)
            fmap.append(x)
        x = self.conv_post(x)
        fmap.append(x)
        return torch.flatten(x, 1, -1), fmap


def _plain_feature_loss(fmap_r, fmap_g):
    return 2 * sum(torch.mean(torch.abs(rl - gl)) for dr, dg in zip(fmap_r, fmap_g) for rl, gl in zip(dr, dg))


def _plain_generator_loss(outs):
    return sum(torch.mean((1 - dg) ** 2) for dg in outs)


def _plain_discriminator_loss(real, gen):
    return sum(torch.mean((1 - dr) ** 2) + torch.mean(dg ** 2) for dr, dg in zip(real, gen))


def test_a_torch_built_discriminator_trains_on_it():
    """One backward of the generator-step sum and one of the discriminator-step sum through this module and through the plain torch
    expressions, on a tiny generator (one Conv1d) and two tiny discriminators.  Per parameter, e_case is the largest error of torch's
    own fp32 run against the same net on the CPU in fp64; this module's run stays within 2 e_case of that fp64 gradient.
    Both runs share torch's fp32 convolutions, whose backward is not reproducible from run to run on the device: for a parameter of a
    few entries (a bias, an 8 x 1 x 5 weight) e_case itself was seen to move by a factor of 3.7 between two runs, so a ratio of two
    such maxima says nothing.  The nets therefore have no bias and no parameter under 192 entries, over which the largest error is a
    stable figure.  Measured (MI355X): DESIGN.md section 3, "GAN losses"."""
    torch.manual_seed(13)
    gen64 = nn.Conv1d(8, 1, 31, padding=15, bias=False).double()
    discs64 = nn.ModuleList([_TinyDisc(), _TinyDisc()]).double()
    feats64, wav64 = torch.randn(4, 8, 6000, dtype=torch.float64), torch.randn(4, 1, 6000, dtype=torch.float64) * 0.5

    def step(gen, discs, feats, wav, which, ours):
        for p in list(gen.parameters()) + list(discs.parameters()):
            p.grad = None
        y_hat = torch.tanh(gen(feats))
        if which == "generator":
            outs = [(disc(wav), disc(y_hat)) for disc in discs]
            y_g, f_r, f_g = [o[1][0] for o in outs], [o[0][1] for o in outs], [o[1][1] for o in outs]
            if ours:
                loss = gan_loss.generator_adversarial_loss(y_g[:1], y_g[1:], f_r[:1], f_g[:1], f_r[1:], f_g[1:])[0]
            else:
                loss = _plain_generator_loss(y_g[1:]) + _plain_generator_loss(y_g[:1]) + _plain_feature_loss(f_r[1:], f_g[1:]) + _plain_feature_loss(f_r[:1], f_g[:1])
            params = list(gen.parameters()) + list(discs.parameters())
        else:
            outs = [(disc(wav)[0], disc(y_hat.detach())[0]) for disc in discs]
            y_r, y_g = [o[0] for o in outs], [o[1] for o in outs]
            if ours:
                loss = gan_loss.discriminator_adversarial_loss(y_r[:1], y_g[:1], y_r[1:], y_g[1:])[0]
            else:
                loss = _plain_discriminator_loss(y_r[1:], y_g[1:]) + _plain_discriminator_loss(y_r[:1], y_g[:1])
            params = list(discs.parameters())
        loss.backward()
        return float(loss.detach()), [p.grad.detach().double().cpu().clone() for p in params]

    import copy
    gen32, discs32 = copy.deepcopy(gen64).float().to(DEV), copy.deepcopy(discs64).float().to(DEV)
    feats32, wav32 = feats64.float().to(DEV), wav64.float().to(DEV)
    torch.use_deterministic_algorithms(True)  # (the convolutions' backward too: the figures below repeat from run to run)
    try:
        for which in ("generator", "discriminator"):
            l64, g64 = step(gen64, discs64, feats64, wav64, which, False)
            l32, g32 = step(gen32, discs32, feats32, wav32, which, False)
            lo, go = step(gen32, discs32, feats32, wav32, which, True)
            print(f"GANLOSS train {which}: loss fp64 {l64:.9g}, torch fp32 {l32:.9g}, this module {lo:.9g}")
            for i, (ref, t32, ours) in enumerate(zip(g64, g32, go)):
                assert ref.numel() >= 192
                e_case, e_ours = float((t32 - ref).abs().max()), float((ours - ref).abs().max())
                print(f"GANLOSS train {which} parameter {i} {tuple(ref.shape)}: e_case {e_case:.3e}, this module {e_ours:.3e}, largest entry {float(ref.abs().max()):.3e}")
                assert e_ours <= 2.0 * e_case, (which, i)
    finally:
        torch.use_deterministic_algorithms(False)


def test_raw_call_refusals():
    terms = _case("single")
    a = terms[0]["a_dev"]
    lib = _lib.lib()
    arr = (_lib.GanTerm * 1)()
    term_out, ws = torch.empty(1, dtype=torch.float64, device=DEV), torch.empty(4096, dtype=torch.uint8, device=DEV)
    g = torch.empty_like(a)

    def call(op, pa, pb, ga, gb, n, out=term_out, n_ws=4096):
        arr[0] = _lib.GanTerm(pa, pb, ga, gb, n, op, 0)
        return lib.parrot_gan_loss(arr, 1, None, 1.0, dptr(out), None, dptr(ws), n_ws, stream_ptr(torch.device(DEV)))

    assert call(7, a.data_ptr(), 0, 0, 0, a.numel()) == -1 and b"unknown op" in lib.parrot_last_error()
    assert call(SQ1, a.data_ptr(), 0, 0, 0, -3) == -1
    assert call(SQ1, 0, 0, 0, 0, a.numel()) == -1
    assert call(L1, a.data_ptr(), 0, 0, 0, a.numel()) == -1
    assert call(SQ1, a.data_ptr(), 0, 0, g.data_ptr(), a.numel()) == -1
    assert call(SQ1, a.data_ptr(), 0, a.data_ptr(), 0, a.numel()) == -1 and b"alias" in lib.parrot_last_error()
    assert call(SQ1, a.data_ptr(), 0, 0, 0, a.numel(), out=None) == -1 and b"neither" in lib.parrot_last_error()
    assert call(SQ1, a.data_ptr(), 0, g.data_ptr(), 0, a.numel(), n_ws=8) == -4 and b"workspace" in lib.parrot_last_error()
    assert lib.parrot_gan_loss(None, 1, None, 1.0, dptr(term_out), None, dptr(ws), 4096, stream_ptr(torch.device(DEV))) == -1
    assert call(SQ1, a.data_ptr(), 0, g.data_ptr(), 0, a.numel()) == 0  # and the library is fine afterwards
    want, _, grads = _raw(terms, None, 1.0)
    assert _same(term_out, want) and _same(g, grads[0][0])


def test_whole_file_under_poison():
    """This file once more in a child process under PARROT_POISON_WS=nan: a kernel reading a byte of the workspace or of an output
    that nobody wrote would turn a result into NaN there, and a gradient element that nobody wrote stays NaN (the tests above
    require the exact zeros and every other element finite, so poison cannot hide)."""
    if os.environ.get("PARROT_POISON_WS"):
        return  # (already a poisoned run: the tests above were it)
    env = dict(os.environ, PARROT_POISON_WS="nan")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", os.path.abspath(__file__), "-k", "not whole_file"], cwd=ROOT,
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
