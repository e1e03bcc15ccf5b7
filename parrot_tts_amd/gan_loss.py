"""The vocoder's adversarial losses -- ``feature_loss``, ``generator_loss`` and ``discriminator_loss`` of reference
utils/vocoder/models.py:279-310 -- backed by libparrot_hip.so (``parrot_gan_loss``), with the reference's signatures and return shapes.

Every mean of a call is one TERM of one device call: a launch that reads each tensor once (fp64 contributions from the fp32 values,
fixed-order fp64 sums: two calls agree bit for bit, also under ``torch.use_deterministic_algorithms(True)``) and a single-workgroup
reduction.  The losses are differentiable with respect to every tensor that requires grad: the backward is ONE gradients-only launch
with the upstream gradients formed on the device (no host synchronisation, no double backward).  ``generator_adversarial_loss``
and ``discriminator_adversarial_loss`` are the reference trainer's sums (train.py:161-165 without the mel term, train.py:142-148)
as one call each -- 62 terms for the generator step -- and their ``*_and_grad`` forms return values and gradients from a single
fused call.  The inputs may come from torch-built discriminators or from ``discriminator_train.TrainableMultiPeriodDiscriminator``,
whose maps are permuted views: every input is made dense once (``_dense``)."""
from __future__ import annotations

import torch

from . import _lib
from .ops import _workspace, dptr, require_cuda, stream_ptr

L1, SQ1, SQ0 = _lib.GAN_L1, _lib.GAN_SQ1, _lib.GAN_SQ0


def _dense(t: torch.Tensor) -> torch.Tensor:
    """The kernel's view of an input: dense fp32, detached (no copy when it already is)."""
    return t.detach().to(torch.float32).contiguous()


def _flat_check(ops, flat):
    """The flat tensor list of a table (a, then b for an L1 term) lives on one GPU -> that device."""
    assert len(flat) == sum(2 if op == L1 else 1 for op in ops)
    for t in flat:
        require_cuda(t, "loss input")
    dev = flat[0].device
    if any(t.device != dev for t in flat):
        raise RuntimeError("parrot_tts_amd: the tensors of one GAN loss call must live on one device")
    return dev


def _call(ops, dense, want, weights, scale: float, values: bool):
    """One parrot_gan_loss call over the table ``ops`` with the dense fp32 tensors ``dense`` (a, then b for an L1 term, term by term)
    -> (term_out (K) fp64 or None, total 0-dim fp32 or None, the gradients in ``dense``'s order: fp32 in the tensor's shape where
    ``want`` says so, else None).  ``weights``: (K) fp64 device tensor, the gradient arriving at each term's mean (None: ones)."""
    K, dev = len(ops), dense[0].device
    lib = _lib.lib()
    terms = (_lib.GanTerm * K)()
    grads = [torch.empty_like(t) if w else None for t, w in zip(dense, want)] if want is not None else [None] * len(dense)
    spare = None  # (an empty tensor's pointer is null, which the library takes for a missing array: n = 0 reads nothing)
    i = 0
    for k, op in enumerate(ops):
        a, ga = dense[i], grads[i]
        b, gb = (dense[i + 1], grads[i + 1]) if op == L1 else (None, None)
        i += 2 if op == L1 else 1
        if a.numel() == 0:
            spare = torch.empty(1, dtype=torch.float32, device=dev) if spare is None else spare
            a, b, ga, gb = spare, (spare if op == L1 else None), None, None
        terms[k] = _lib.GanTerm(a.data_ptr(), 0 if b is None else b.data_ptr(), 0 if ga is None else ga.data_ptr(),
                                0 if gb is None else gb.data_ptr(), dense[i - 1].numel(), op, 0)
    term_out = torch.empty(K, dtype=torch.float64, device=dev) if values else None
    total = torch.empty((), dtype=torch.float32, device=dev) if values else None
    with torch.cuda.device(dev):
        ws = _workspace(lib.parrot_gan_loss_workspace_bytes(terms, K), dev) if values else None
        _lib.check(lib.parrot_gan_loss(terms, K, dptr(weights), float(scale), dptr(term_out), dptr(total), dptr(ws),
                                       0 if ws is None else ws.numel(), stream_ptr(dev)))
    return term_out, total, grads


class _GanLossFn(torch.autograd.Function):
    """(ops, scale, *tensors) -> (total, term_out).  The forward is the values-only call; the backward is one gradients-only call
    with w_k = scale * g_total + g_terms[k], formed on the device, writing a gradient only for the tensors that need one."""

    @staticmethod
    def forward(ctx, ops, scale, *tensors):
        dense = [_dense(t) for t in tensors]
        ctx.save_for_backward(*dense)
        ctx.ops, ctx.scale = ops, scale
        ctx.meta = [(t.shape, t.dtype) for t in tensors]
        term_out, total, _ = _call(ops, dense, None, None, scale, True)
        return total, term_out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_total, g_terms):
        dense, need = ctx.saved_tensors, ctx.needs_input_grad[2:]
        if not any(need):
            return (None,) * (2 + len(dense))
        w = (g_total.to(torch.float64) * ctx.scale + g_terms.to(torch.float64)).contiguous()
        _, _, grads = _call(ctx.ops, dense, need, w, ctx.scale, False)
        return (None, None) + tuple(None if g is None else g.reshape(shape).to(dtype) for g, (shape, dtype) in zip(grads, ctx.meta))


def _run(ops, flat, scale: float):
    """-> (total, term_out) of the table: with a graph when grad mode is on and a tensor requires grad, else the plain call."""
    _flat_check(ops, flat)
    if torch.is_grad_enabled() and any(t.requires_grad for t in flat):
        return _GanLossFn.apply(tuple(ops), float(scale), *flat)
    with torch.no_grad():
        term_out, total, _ = _call(ops, [_dense(t) for t in flat], None, None, scale, True)
    return total, term_out


def _fused(ops, flat, weights, scale: float):
    """Values and every gradient from one call -> (total, term_out, gradients in ``flat``'s order, shapes and dtypes)."""
    _flat_check(ops, flat)
    term_out, total, grads = _call(ops, [_dense(t) for t in flat], [True] * len(flat), weights, scale, True)
    return total, term_out, [g.reshape(t.shape).to(t.dtype) for g, t in zip(grads, flat)]


def _pairs(fmap_r, fmap_g, what="fmap_r / fmap_g"):
    """The (real, generated) feature-map pairs of two nested lists, in the reference's loop order; ValueError on a mismatch."""
    if len(fmap_r) != len(fmap_g):
        raise ValueError(f"{what}: {len(fmap_r)} and {len(fmap_g)} discriminators")
    out = []
    for i, (dr, dg) in enumerate(zip(fmap_r, fmap_g)):
        if len(dr) != len(dg):
            raise ValueError(f"{what}: discriminator {i} has {len(dr)} and {len(dg)} feature maps")
        for j, (rl, gl) in enumerate(zip(dr, dg)):
            if rl.shape != gl.shape:
                raise ValueError(f"{what}: feature map {j} of discriminator {i} has shapes {tuple(rl.shape)} and {tuple(gl.shape)}")
            out.append((rl, gl))
    return out


def _l1_flat(pairs, detach_real: bool):
    return [t for rl, gl in pairs for t in ((rl.detach() if detach_real else rl), gl)]


def feature_loss(fmap_r, fmap_g, detach_real: bool = False):
    """models.py:279-285: ``2 * sum over every pair of mean |rl - gl|`` -> a 0-dim fp32 tensor (the int 0 for empty lists, as the
    reference).  Gradients flow to the tensors that require grad.  ``detach_real=True`` treats ``fmap_r`` as constants and spares
    the write of d/d fmap_r: the reference's generator step computes that gradient (the real branch reaches the discriminators'
    weights) and discards it with ``optim_g.step()``, which updates the generator alone."""
    pairs = _pairs(fmap_r, fmap_g)
    if not pairs:
        return 0
    return _run([L1] * len(pairs), _l1_flat(pairs, detach_real), 2.0)[0]


def generator_loss(disc_outputs):
    """models.py:302-310: ``(sum_k mean (1 - dg_k)^2, [the K means])`` -> (0-dim fp32 tensor, list of 0-dim fp32 tensors: detached
    views of the term vector).  ``(0, [])`` for an empty list, as the reference."""
    outs = list(disc_outputs)
    if not outs:
        return 0, []
    total, term_out = _run([SQ1] * len(outs), outs, 1.0)
    return total, list(term_out.detach().to(torch.float32).unbind(0))


def _disc_flat(real, generated, what):
    real, generated = list(real), list(generated)
    if len(real) != len(generated):
        raise ValueError(f"{what}: {len(real)} real and {len(generated)} generated outputs")
    return [t for pair in zip(real, generated) for t in pair]


def discriminator_loss(disc_real_outputs, disc_generated_outputs):
    """models.py:288-299: ``(sum_k mean (1 - dr_k)^2 + mean dg_k^2, r_losses, g_losses)`` -> (0-dim fp32 tensor, two lists of Python
    floats, as the reference's ``.item()``s -- read back with ONE transfer of the term vector).  ``(0, [], [])`` for empty lists."""
    flat = _disc_flat(disc_real_outputs, disc_generated_outputs, "disc_real_outputs / disc_generated_outputs")
    if not flat:
        return 0, [], []
    total, term_out = _run([SQ1, SQ0] * (len(flat) // 2), flat, 1.0)
    vals = term_out.detach().to(torch.float32).tolist()
    return total, vals[0::2], vals[1::2]


_WEIGHTS: dict = {}


def _weights(c, dev) -> torch.Tensor:
    """The constant per-term factors of a step-level sum as a (K) fp64 device tensor (uploaded once per table and device)."""
    key = (tuple(c), dev)
    if key not in _WEIGHTS:
        _WEIGHTS[key] = torch.tensor(c, dtype=torch.float64, device=dev)
    return _WEIGHTS[key]


def _generator_table(y_df_hat_g, y_ds_hat_g, fmap_f_r, fmap_f_g, fmap_s_r, fmap_s_g, detach_real):
    """train.py:161-165's terms in the order of its sum, loss_gen_s + loss_gen_f + loss_fm_s + loss_fm_f."""
    gen_s, gen_f = list(y_ds_hat_g), list(y_df_hat_g)
    fm_s, fm_f = _pairs(fmap_s_r, fmap_s_g, "fmap_s_r / fmap_s_g"), _pairs(fmap_f_r, fmap_f_g, "fmap_f_r / fmap_f_g")
    ops = [SQ1] * (len(gen_s) + len(gen_f)) + [L1] * (len(fm_s) + len(fm_f))
    flat = gen_s + gen_f + _l1_flat(fm_s, detach_real) + _l1_flat(fm_f, detach_real)
    c = [1.0] * (len(gen_s) + len(gen_f)) + [2.0] * (len(fm_s) + len(fm_f))  # (feature_loss's factor 2)
    names = ("loss_gen_s", "loss_gen_f", "loss_fm_s", "loss_fm_f")
    return ops, flat, c, dict(zip(names, (len(gen_s), len(gen_f), len(fm_s), len(fm_f))))


def _weighted(term_out, c, groups):
    """(sum_k c_k term_out[k] as fp32, {group: its detached share}): a small fp64 expression on the device."""
    wt = term_out * _weights(c, term_out.device)
    parts, k = {}, 0
    for name, n in groups.items():
        parts[name] = wt[k:k + n].sum().to(torch.float32).detach()
        k += n
    return wt.sum().to(torch.float32), parts


def generator_adversarial_loss(y_df_hat_g, y_ds_hat_g, fmap_f_r, fmap_f_g, fmap_s_r, fmap_s_g, detach_real: bool = False):
    """train.py:161-165 without the mel term: ``loss_gen_s + loss_gen_f + loss_fm_s + loss_fm_f`` with every term (62 for the
    reference's discriminators) in ONE device call -> (loss, parts): a 0-dim fp32 tensor and a dict of the four detached sums.
    ``detach_real``: as ``feature_loss``."""
    ops, flat, c, groups = _generator_table(y_df_hat_g, y_ds_hat_g, fmap_f_r, fmap_f_g, fmap_s_r, fmap_s_g, detach_real)
    if not ops:
        return 0, {name: 0 for name in groups}
    return _weighted(_run(ops, flat, 1.0)[1], c, groups)


def _discriminator_table(y_df_hat_r, y_df_hat_g, y_ds_hat_r, y_ds_hat_g):
    """train.py:142-148's terms in the order of its sum, loss_disc_s + loss_disc_f."""
    s, f = _disc_flat(y_ds_hat_r, y_ds_hat_g, "y_ds_hat_r / y_ds_hat_g"), _disc_flat(y_df_hat_r, y_df_hat_g, "y_df_hat_r / y_df_hat_g")
    flat = s + f
    return [SQ1, SQ0] * (len(flat) // 2), flat, [1.0] * len(flat), {"loss_disc_s": len(s), "loss_disc_f": len(f)}


def discriminator_adversarial_loss(y_df_hat_r, y_df_hat_g, y_ds_hat_r, y_ds_hat_g):
    """train.py:142-148: ``loss_disc_s + loss_disc_f`` in one device call -> (loss, parts): a 0-dim fp32 tensor and a dict of the
    two detached sums."""
    ops, flat, c, groups = _discriminator_table(y_df_hat_r, y_df_hat_g, y_ds_hat_r, y_ds_hat_g)
    if not ops:
        return 0, {name: 0 for name in groups}
    return _weighted(_run(ops, flat, 1.0)[1], c, groups)


def _renest(grads, *nests):
    """The flat gradient list back into lists shaped like ``nests`` (each a list of tensors or a list of lists), in order."""
    it = iter(grads)
    return tuple([[next(it) for _ in sub] if isinstance(sub, (list, tuple)) else next(it) for sub in nest] for nest in nests)


@torch.no_grad()
def generator_adversarial_loss_and_grad(y_df_hat_g, y_ds_hat_g, fmap_f_r, fmap_f_g, fmap_s_r, fmap_s_g, detach_real: bool = False):
    """``generator_adversarial_loss`` and its gradient from one fused call (values and gradients together) -> (loss, parts, grads):
    ``grads`` is a tuple nested like the six inputs, each gradient in its tensor's shape and dtype.  ``detach_real=True``: the two
    ``fmap_*_r`` entries are None and their gradients are not written."""
    ops, flat, c, groups = _generator_table(y_df_hat_g, y_ds_hat_g, fmap_f_r, fmap_f_g, fmap_s_r, fmap_s_g, False)
    if not ops:
        return 0, {name: 0 for name in groups}, ([], [], [], [], [], [])
    dev = _flat_check(ops, flat)
    n_sq = groups["loss_gen_s"] + groups["loss_gen_f"]
    want = [True] * n_sq + [not detach_real, True] * (len(ops) - n_sq)
    term_out, _, grads = _call(ops, [_dense(t) for t in flat], want, _weights(c, dev), 1.0, True)
    grads = [None if g is None else g.reshape(t.shape).to(t.dtype) for g, t in zip(grads, flat)]
    loss, parts = _weighted(term_out, c, groups)
    n_s, n_f, p_s = groups["loss_gen_s"], groups["loss_gen_f"], 2 * groups["loss_fm_s"]
    l1_s, l1_f = grads[n_sq:n_sq + p_s], grads[n_sq + p_s:]
    g_s_r, g_s_g = _renest(l1_s[0::2], fmap_s_r) + _renest(l1_s[1::2], fmap_s_g)
    g_f_r, g_f_g = _renest(l1_f[0::2], fmap_f_r) + _renest(l1_f[1::2], fmap_f_g)
    if detach_real:
        g_s_r = g_f_r = None
    return loss, parts, (grads[n_s:n_s + n_f], grads[:n_s], g_f_r, g_f_g, g_s_r, g_s_g)


@torch.no_grad()
def discriminator_adversarial_loss_and_grad(y_df_hat_r, y_df_hat_g, y_ds_hat_r, y_ds_hat_g):
    """``discriminator_adversarial_loss`` and its gradient from one fused call -> (loss, parts, grads): ``grads`` is a tuple of four
    lists like the inputs."""
    ops, flat, c, groups = _discriminator_table(y_df_hat_r, y_df_hat_g, y_ds_hat_r, y_ds_hat_g)
    if not ops:
        return 0, {name: 0 for name in groups}, ([], [], [], [])
    _, term_out, grads = _fused(ops, flat, None, 1.0)
    loss, parts = _weighted(term_out, c, groups)
    n_s = groups["loss_disc_s"]
    return loss, parts, (grads[n_s + 0::2], grads[n_s + 1::2], grads[0:n_s:2], grads[1:n_s:2])
