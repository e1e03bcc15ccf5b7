"""CPU restatement of the reference's ``MultiPeriodDiscriminator.forward`` (utils/vocoder/models.py:171-225) for training, from
plain torch calls -- ``F.pad(..., "reflect")``, ``torch._weight_norm(v, g, 0)``, ``F.conv2d`` -- in fp32 or fp64 on leaves made from
the state dict, with the ONE change tests/voc_train_ref.py makes: every leaky ReLU is ``where(mask, x, slope * x)``.  ``mask`` is
``x > 0``, or a list of masks handed in in site order (period-major, then layer: five sites per period), each over all N = 2 B rows,
real rows first; the lrelu inputs are recorded in the same order and shape (N, C, H, p).  As the reference does, a period runs the
real rows and the generated rows as two calls.

Outputs are flat lists in ONE order, used for upstream gradients too: per period the six maps as (real, generated) pairs, then the
two scores: 14 tensors per period (``flat_outputs``)."""
import torch
import torch.nn.functional as F

from parrot_tts_amd import synth
from voc_train_ref import check_caps, excluded  # noqa: F401  (the mask band and its caps are the generator's)

SLOPE = 0.1
SEED_W, SEED_IN = 1234, 1235
NARROW = [4, 8, 33, 65]


def _cfg(**kw):
    c = synth.default_mpd_config()
    c.update(kw)
    return c


# name -> (config, B, T)
_CASES = {"M1": (_cfg(channels=NARROW), 2, 2311),   # T mod p = 1 for every p: the longest pad; H = 1156 -> 386 -> 129 -> 43 -> 15 at p = 2
          "M2": (_cfg(channels=NARROW), 3, 2310),   # 2 3 5 7 11: no pad anywhere; several 256-pair chunks
          "M3": (_cfg(), 1, 400),                   # the real widths
          "M4": (_cfg(channels=NARROW), 1, 12),     # p = 11 pads 10 of 12, H = 2, last maps H = 1
          "M5": (_cfg(periods=[1, 4], channels=[3, 5, 7, 9]), 1, 131)}  # p = 1: the fold is the identity; central differences
CASES = tuple(_CASES)
_made = {}


def make_case(name: str):
    """-> (cfg, state dict (fp32, weight norm attached), y (B, 1, T), y_hat (B, 1, T)), seeded; made once."""
    if name not in _made:
        cfg, B, T = _CASES[name]
        _made[name] = (cfg, synth.synth_mpd_state_dict(cfg, seed=SEED_W)) + synth.synth_mpd_batch(B, T, seed=SEED_IN)
    return _made[name]


def n_sites(cfg) -> int:
    return 5 * len(cfg["periods"])


def _weight(sd, prefix):
    if prefix + ".weight" in sd:
        return sd[prefix + ".weight"]
    return torch._weight_norm(sd[prefix + ".weight_v"], sd[prefix + ".weight_g"], 0)


def _disc_p(sd, cfg, i, x, site_masks):
    """DiscriminatorP.forward (models.py:184-203) of period index i on x (b, 1, t) -> (score, the six maps, the five lrelu inputs)."""
    p, s = cfg["periods"][i], cfg["stride"]
    b, c, t = x.shape
    if t % p != 0:
        n_pad = p - (t % p)
        x = F.pad(x, (0, n_pad), "reflect")
        t = t + n_pad
    x = x.view(b, c, t // p, p)
    fmap, inputs = [], []
    for l in range(5):
        pre = f"discriminators.{i}.convs.{l}"
        x = F.conv2d(x, _weight(sd, pre), sd[pre + ".bias"], (s if l < 4 else 1, 1), padding=(2, 0))
        inputs.append(x.detach())
        if site_masks is None:
            x = F.leaky_relu(x, SLOPE)
        else:
            x = torch.where(site_masks[l].view(x.shape).bool(), x, SLOPE * x)
        fmap.append(x)
    pre = f"discriminators.{i}.conv_post"
    x = F.conv2d(x, _weight(sd, pre), sd[pre + ".bias"], 1, padding=(1, 0))
    fmap.append(x)
    return torch.flatten(x, 1, -1), fmap, inputs


def forward(sd, cfg, y, y_hat, masks=None):
    """-> (y_d_rs, y_d_gs, fmap_rs, fmap_gs, lrelu inputs in site order, each (2 B, C, H, p)).  ``sd`` and the waveforms in the dtype
    to run in.  masks None: the reference's own F.leaky_relu (no change at all)."""
    B = y.shape[0]
    y_d_rs, y_d_gs, fmap_rs, fmap_gs, inputs = [], [], [], [], []
    for i in range(len(cfg["periods"])):
        m = None if masks is None else masks[5 * i:5 * i + 5]
        r, fr, ir = _disc_p(sd, cfg, i, y, None if m is None else [t[:B] for t in m])
        g, fg, ig = _disc_p(sd, cfg, i, y_hat, None if m is None else [t[B:] for t in m])
        y_d_rs.append(r); y_d_gs.append(g); fmap_rs.append(fr); fmap_gs.append(fg)
        inputs += [torch.cat(pair, 0) for pair in zip(ir, ig)]
    if masks is not None:
        assert len(masks) == len(inputs)
    return y_d_rs, y_d_gs, fmap_rs, fmap_gs, inputs


def flat_outputs(y_d_rs, y_d_gs, fmap_rs, fmap_gs):
    out = []
    for r, g, fr, fg in zip(y_d_rs, y_d_gs, fmap_rs, fmap_gs):
        for a, b in zip(fr, fg):
            out += [a, b]
        out += [r, g]
    return out


def output_names(cfg):
    out = []
    for p in cfg["periods"]:
        for l in range(6):
            out += [f"p{p} map{l} real", f"p{p} map{l} gen"]
        out += [f"p{p} score real", f"p{p} score gen"]
    return out


def random_upstream(outs, seed=17):
    """A seeded normal gradient at every output, fp64 draws rounded to fp32."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(o.shape, generator=g, dtype=torch.float64).to(torch.float32) for o in outs]


def d_loss(y_d_rs, y_d_gs):
    """discriminator_loss (models.py:288-299) without the .item()s"""
    loss = 0
    for dr, dg in zip(y_d_rs, y_d_gs):
        loss = loss + (torch.mean((1 - dr) ** 2) + torch.mean(dg ** 2))
    return loss


def g_loss(y_d_gs, fmap_rs, fmap_gs):
    """generator_loss + feature_loss (models.py:279-285, :302-310; train.py:159-165 for one discriminator family)"""
    gen = 0
    for dg in y_d_gs:
        gen = gen + torch.mean((1 - dg) ** 2)
    fm = 0
    for dr, dg in zip(fmap_rs, fmap_gs):
        for rl, gl in zip(dr, dg):
            fm = fm + torch.mean(torch.abs(rl - gl))
    return gen + fm * 2


def loss_and_grads(sd, cfg, y, y_hat, dtype, upstream, masks):
    """-> (flat outputs, {key -> gradient}, d y_hat or None, lrelu inputs, loss or None) in ``dtype``.  upstream: a flat list of
    gradients (``flat_outputs`` order), "d" (the discriminator step: y_hat detached, no d y_hat) or "g" (the generator step)."""
    sdt = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    yh = y_hat.detach().to(dtype).clone().requires_grad_(upstream != "d")
    res = forward(sdt, cfg, y.to(dtype), yh, masks)
    outs = flat_outputs(*res[:4])
    keys = list(sd)
    leaves = [sdt[k] for k in keys] + ([] if upstream == "d" else [yh])
    if upstream == "d":
        loss = d_loss(res[0], res[1])
    elif upstream == "g":
        loss = g_loss(res[1], res[2], res[3])
    else:
        loss = sum((o * u.to(dtype)).sum() for o, u in zip(outs, upstream))
    grads = [g.detach() for g in torch.autograd.grad(loss, leaves)]
    dyh = None if upstream == "d" else grads[-1]
    return [o.detach() for o in outs], dict(zip(keys, grads)), dyh, res[4], (float(loss.detach()) if isinstance(upstream, str) else None)


_own = {}


def own_inputs(name: str):
    """The lrelu inputs of the restatement run on its own (its own x > 0) in fp64 and in fp32, on ONE thread (voc_train_ref.own_inputs
    says why): what the mask tests take x64 and e_site from."""
    if name not in _own:
        cfg, sd, y, y_hat = make_case(name)
        keep = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            with torch.no_grad():
                _own[name] = (forward({k: v.double() for k, v in sd.items()}, cfg, y.double(), y_hat.double())[4], forward(sd, cfg, y, y_hat)[4])
        finally:
            torch.set_num_threads(keep)
    return _own[name]


def folded(sd):
    """The state dict after remove_weight_norm(): plain ``weight`` keys (fp64 fold, rounded to fp32 once)."""
    out = {}
    for k, v in sd.items():
        if k.endswith(".weight_v"):
            pre = k[:-len(".weight_v")]
            out[pre + ".weight"] = torch._weight_norm(v.double(), sd[pre + ".weight_g"].double(), 0).to(torch.float32)
        elif not k.endswith(".weight_g"):
            out[k] = v
    return out
