"""CPU restatement of the reference's ``CodeGenerator.forward`` (utils/vocoder/models.py:153-169) for training: it runs
``oracle.parrot_oracle.code_generator_forward`` under autograd, in fp32 or fp64, on leaves made from the state dict, with ONE change:
every leaky ReLU is ``where(mask, x, slope * x)``.  ``mask`` is ``x > 0``, or a list of masks handed in and consumed in site order
(the reference's execution order: per stage the one before ups[i], then per resblock and dilation the one before convs1[m] and the
one before convs2[m]; last the one before conv_post).

Why masks are handed in: at these sizes an fp32 evaluation flips the sign of some lrelu input with probability of order one, and one
flip moves a bias gradient by tens of thousands of times the reference's own fp32-vs-fp64 error.  So the reference is handed the
masks the device applied, as tests/tte_train_ref.py is handed the dropout masks, and the masks themselves are tested separately."""
import contextlib

import torch
import torch.nn.functional as F

from oracle import parrot_oracle as O
from parrot_tts_amd import synth

SEED = 1234


def _configs():
    small = synth.small_voc_config
    v2 = small()
    v2.update(upsample_initial_channel=160, embedding_dim=36, model_in_dim=72, upsample_rates=[2, 3], upsample_kernel_sizes=[4, 7],
              resblock_kernel_sizes=[3, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 2, 4]])
    v4 = small()
    v4.update(resblock="2", multispkr=None, model_in_dim=16)
    # name -> (config, B, U)
    return {"V1": (small(), 2, 3),                      # five stages, T = 15 .. 960 across the 64-column tile edge, channels 32 .. 2, 96 sites
            "V2": (v2, 3, 23),                          # M = 160 / 80 / 40, K = 72 across the 64-row tile edge; B T = 414: two chunks; k = 11
            "V3": (synth.corner_voc_config(), 1, 2),    # odd k - u: T u + 1 lengths; uneven dilation lists
            "V4": (v4, 1, 1),                           # ResBlock2, no speaker table, one unit: T = 5 at stage 0
            "V5": (synth.default_voc_config(), 1, 3)}   # the real widths, 512 .. 16 channels


CASES = ("V1", "V2", "V3", "V4", "V5")


def make_case(name: str):
    """-> (h, state dict (fp32, weight norm attached), batch {code (B, U), spkr (B, 1)}), seeded."""
    h, B, U = _configs()[name]
    return h, synth.synth_voc_state_dict(h, seed=SEED), synth.synth_voc_batch(B, U, h, seed=SEED)


class _Functional:
    """torch.nn.functional with the one change: the leaky ReLU takes its mask from a list (or from x > 0) and records its input."""

    def __init__(self, masks):
        self.masks, self.inputs = masks, []

    def __getattr__(self, name):
        return getattr(F, name)

    def leaky_relu(self, x, negative_slope=0.01):
        site = len(self.inputs)
        self.inputs.append(x.detach())
        m = (x > 0) if self.masks is None else self.masks[site].to(x.device).view(x.shape).bool()
        return torch.where(m, x, negative_slope * x)


@contextlib.contextmanager
def _patched(masks):
    shim, keep = _Functional(masks), O.F
    O.F = shim
    try:
        yield shim
    finally:
        O.F = keep


def forward(sd, h, batch, masks=None):
    """-> (wav (B, 1, T), the lrelu inputs in site order).  ``sd`` in the dtype to run in."""
    with _patched(masks) as shim:
        wav = O.code_generator_forward(sd, h, batch["code"], batch.get("spkr") if h.get("multispkr") else None)
    if masks is not None:
        assert len(shim.inputs) == len(masks)
    return wav, shim.inputs


_own = {}


def own_inputs(name: str):
    """The lrelu inputs of the restatement run on its own (masks x > 0 of the run itself) in fp64 and in fp32: what the mask tests
    take x64 and e_site from.  Computed once, on ONE thread: e_site is a maximum of fp32 rounding errors, and torch's CPU convs sum
    in an order that depends on the thread count, so on more threads the band, and the number of elements inside it, would depend on
    the machine (V1, site 82: 2 elements of 3840 inside on 1 - 8 threads, 4 on 16, against a cap of 3.84)."""
    if name not in _own:
        h, sd, batch = make_case(name)
        keep = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            with torch.no_grad():
                _own[name] = (forward({k: v.double() for k, v in sd.items()}, h, batch)[1], forward(sd, h, batch)[1])
        finally:
            torch.set_num_threads(keep)
    return _own[name]


def n_sites(h) -> int:
    per = (6 if str(h["resblock"]) == "1" else 2) * len(h["resblock_kernel_sizes"])
    return len(h["upsample_rates"]) * (1 + per) + 1


def param_keys(sd):
    return list(sd)


def loss_and_grads(sd, h, batch, dtype, upstream, masks=None):
    """-> (wav, {key -> gradient}, lrelu inputs, loss or None) in ``dtype``.  upstream: a gradient (B, 1, T) at the waveform, or
    ("mse", target): the gradient of F.mse_loss(wav, target)."""
    sdt = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    wav, inputs = forward(sdt, h, batch, masks)
    keys = param_keys(sd)
    loss = None
    if isinstance(upstream, tuple):
        loss = F.mse_loss(wav, upstream[1].to(dtype))
        grads = torch.autograd.grad(loss, [sdt[k] for k in keys])
        loss = float(loss.detach())
    else:
        grads = torch.autograd.grad(wav, [sdt[k] for k in keys], upstream.to(dtype))
    return wav.detach(), dict(zip(keys, (g.detach() for g in grads))), inputs, loss


def folded(sd):
    """The state dict after remove_weight_norm(): plain ``weight`` keys (fp64 fold, rounded to fp32 once)."""
    return {k: v.to(torch.float32) for k, v in O.fold_weight_norm({k: v.double() for k, v in sd.items()}).items()}


def excluded(inputs64, inputs32, masks, band=8.0):
    """Per site: (elements inside the band |x64| <= band * e_site, elements of the site, mismatches of ``masks`` against x64 > 0
    outside the band).  e_site: the fp32-vs-fp64 max error of the site's input.  masks None: the fp32 run's own x > 0."""
    out = []
    for s, (x64, x32) in enumerate(zip(inputs64, inputs32)):
        e = float((x32.double() - x64).abs().max())
        inside = x64.abs() <= band * e
        m = (x32 > 0) if masks is None else masks[s].cpu().view(x64.shape).bool()
        wrong = ((m != (x64 > 0)) & ~inside).sum()
        out.append((int(inside.sum()), x64.numel(), int(wrong)))
    return out


def check_caps(counts):
    """The caps on what the band leaves out: in total at most 1e-4 of all lrelu elements of the case, per site at most the larger of
    one element and 1e-3 of the site; and no mismatch outside the band.  -> (excluded share, worst site share)."""
    total_in, total = sum(c[0] for c in counts), sum(c[1] for c in counts)
    assert all(c[2] == 0 for c in counts), [(s, c) for s, c in enumerate(counts) if c[2]]
    assert total_in <= 1e-4 * total, (total_in, total)
    for s, (inside, n, _) in enumerate(counts):
        assert inside <= max(1, 1e-3 * n), (s, inside, n)
    return total_in / total, max(c[0] / c[1] for c in counts)
