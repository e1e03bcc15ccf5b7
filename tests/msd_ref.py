"""CPU restatement of the reference's ``MultiScaleDiscriminator.forward`` (utils/vocoder/models.py:228-276) for training, from plain
torch calls -- ``F.conv1d(..., groups=)``, ``torch._weight_norm(v, g, 0)``, ``F.avg_pool1d(x, 4, 2, 2)`` and a hand-written power
iteration, sigma and fold as ``torch.nn.utils.spectral_norm`` computes them -- in fp32 or fp64 on leaves made from the state dict,
with the ONE change tests/mpd_ref.py makes: every leaky ReLU is ``where(mask, x, slope * x)``.  ``mask`` is ``x > 0``, or a list of
masks handed in in site order (scale-major, then layer: seven sites per scale), each over all N = 2 B rows, real rows first; the
lrelu inputs are recorded in the same order and shape (N, C, L).

As the reference does, a scale runs the real rows and the generated rows as two calls, and in training mode every call of the
spectral-normed discriminator 0 starts with one power iteration (under no_grad; u and v are constants of the graph): the real rows
see ``weight_orig / sigma_1``, the generated rows ``weight_orig / sigma_2``, and the buffers end two iterations on.  ``forward`` returns
them.  With ``train=False`` nothing iterates and both calls use one sigma.

Outputs are flat lists in ONE order, used for upstream gradients too: per scale the eight maps as (real, generated) pairs, then the
two scores: 18 tensors per scale (``flat_outputs``)."""
import torch
import torch.nn.functional as F

from parrot_tts_amd import synth
from voc_train_ref import check_caps, excluded  # noqa: F401  (the mask band and its caps are the generator's)

SLOPE = 0.1
EPS = 1e-12
SEED_W, SEED_IN = 1234, 1235
KERNELS = (15, 41, 41, 41, 41, 41, 5)
STRIDES = (1, 2, 2, 4, 4, 1, 1)
NARROW = [16, 16, 32, 64, 128, 128, 65]


def _cfg(**kw):
    c = synth.default_msd_config()
    c.update(kw)
    return c


# name -> (config, B, T)
_CASES = {"S1": (_cfg(channels=NARROW), 2, 2311),   # odd lengths at every scale (pooled 1156, 579); cin / g = 4, 1, 2, 4, 8
          "S2": (_cfg(channels=[6, 9, 15, 15, 33, 33, 7], groups=[1, 3, 3, 3, 3, 3, 1]), 3, 2310),  # per-group widths 2, 3, 5, 11
          "S3": (_cfg(), 1, 400),                   # the real widths
          "S4": (_cfg(channels=NARROW), 1, 12),     # lengths 12 -> 6 -> 3 -> 1 -> 1; pooled 7, 4; most taps in the padding
          "S5": (_cfg(channels=[2, 4, 4, 4, 4, 4, 3], groups=[1, 2, 2, 2, 2, 2, 1]), 1, 37)}  # central differences
CASES = tuple(_CASES)
_made = {}


def make_case(name: str):
    """-> (cfg, state dict (fp32), y (B, 1, T), y_hat (B, 1, T)), seeded; made once."""
    if name not in _made:
        cfg, B, T = _CASES[name]
        _made[name] = (cfg, synth.synth_msd_state_dict(cfg, seed=SEED_W)) + synth.synth_msd_batch(B, T, seed=SEED_IN)
    return _made[name]


def n_sites(cfg) -> int:
    return 7 * cfg["n_scales"]


def pool(x):
    """AvgPool1d(4, 2, padding=2): count_include_pad is torch's default, so every window divides by 4."""
    return F.avg_pool1d(x, 4, 2, 2)


def power_iteration(w_mat, u, v):
    """One iteration as torch.nn.utils.spectral_norm runs it: v = normalize(W^T u), u = normalize(W v)."""
    v = F.normalize(torch.mv(w_mat.t(), u), dim=0, eps=EPS)
    u = F.normalize(torch.mv(w_mat, v), dim=0, eps=EPS)
    return u, v


def spectral_weight(w_orig, u, v):
    """weight_orig / sigma with sigma = u^T (W v), u and v constants."""
    sigma = torch.dot(u, torch.mv(w_orig.flatten(1), v))
    return w_orig / sigma


class _State:
    """The weights one call of a discriminator runs on.  A spectral layer's u and v live here between the two calls."""

    def __init__(self, sd, i, train):
        self.sd, self.i, self.train = sd, i, train
        self.uv = {}

    def weight(self, prefix):
        sd = self.sd
        if prefix + ".weight" in sd:
            return sd[prefix + ".weight"]
        if prefix + ".weight_orig" in sd:
            w = sd[prefix + ".weight_orig"]
            u, v = self.uv.get(prefix, (sd[prefix + ".weight_u"].detach(), sd[prefix + ".weight_v"].detach()))
            if self.train:
                with torch.no_grad():
                    u, v = power_iteration(w.detach().flatten(1), u, v)
            self.uv[prefix] = (u, v)
            return spectral_weight(w, u, v)
        return torch._weight_norm(sd[prefix + ".weight_v"], sd[prefix + ".weight_g"], 0)


def _disc_s(st, cfg, x, site_masks):
    """DiscriminatorS.forward (models.py:240-250) of scale st.i on x (b, 1, t) -> (score, the eight maps, the seven lrelu inputs)."""
    fmap, inputs = [], []
    for l in range(7):
        pre = f"discriminators.{st.i}.convs.{l}"
        x = F.conv1d(x, st.weight(pre), st.sd[pre + ".bias"], STRIDES[l], padding=(KERNELS[l] - 1) // 2, groups=cfg["groups"][l])
        inputs.append(x.detach())
        if site_masks is None:
            x = F.leaky_relu(x, SLOPE)
        else:
            x = torch.where(site_masks[l].view(x.shape).bool(), x, SLOPE * x)
        fmap.append(x)
    pre = f"discriminators.{st.i}.conv_post"
    x = F.conv1d(x, st.weight(pre), st.sd[pre + ".bias"], 1, padding=1)
    fmap.append(x)
    return torch.flatten(x, 1, -1), fmap, inputs


def forward(sd, cfg, y, y_hat, masks=None, train=True):
    """-> (y_d_rs, y_d_gs, fmap_rs, fmap_gs, lrelu inputs in site order, each (2 B, C, L), {key -> updated weight_u / weight_v}).
    ``sd`` and the waveforms in the dtype to run in.  masks None: the reference's own F.leaky_relu (no change at all)."""
    B = y.shape[0]
    y_d_rs, y_d_gs, fmap_rs, fmap_gs, inputs, new = [], [], [], [], [], {}
    for i in range(cfg["n_scales"]):
        if i != 0:
            y, y_hat = pool(y), pool(y_hat)
        m = None if masks is None else masks[7 * i:7 * i + 7]
        st = _State(sd, i, train)
        r, fr, ir = _disc_s(st, cfg, y, None if m is None else [t[:B] for t in m])
        g, fg, ig = _disc_s(st, cfg, y_hat, None if m is None else [t[B:] for t in m])
        y_d_rs.append(r); y_d_gs.append(g); fmap_rs.append(fr); fmap_gs.append(fg)
        inputs += [torch.cat(pair, 0) for pair in zip(ir, ig)]
        for pre, (u, v) in st.uv.items():
            new[pre + ".weight_u"], new[pre + ".weight_v"] = u.detach(), v.detach()
    if masks is not None:
        assert len(masks) == len(inputs)
    return y_d_rs, y_d_gs, fmap_rs, fmap_gs, inputs, new


def flat_outputs(y_d_rs, y_d_gs, fmap_rs, fmap_gs):
    out = []
    for r, g, fr, fg in zip(y_d_rs, y_d_gs, fmap_rs, fmap_gs):
        for a, b in zip(fr, fg):
            out += [a, b]
        out += [r, g]
    return out


def output_names(cfg):
    out = []
    for i in range(cfg["n_scales"]):
        for l in range(8):
            out += [f"s{i} map{l} real", f"s{i} map{l} gen"]
        out += [f"s{i} score real", f"s{i} score gen"]
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


def param_keys(sd):
    """The keys that are parameters: everything but a spectral layer's buffers (weight_u, and weight_v beside a weight_orig)."""
    return [k for k in sd if not (k.endswith(".weight_u") or (k.endswith(".weight_v") and k[:-len("weight_v")] + "weight_orig" in sd))]


def loss_and_grads(sd, cfg, y, y_hat, dtype, upstream, masks, train=True):
    """-> (flat outputs, {parameter key -> gradient}, d y_hat or None, lrelu inputs, loss or None, updated buffers) in ``dtype``.
    upstream: a flat list of gradients (``flat_outputs`` order), "d" (the discriminator step: y_hat detached, no d y_hat) or "g" (the
    generator step)."""
    keys = param_keys(sd)
    sdt = {k: v.detach().to(dtype).clone().requires_grad_(k in keys) for k, v in sd.items()}
    yh = y_hat.detach().to(dtype).clone().requires_grad_(upstream != "d")
    res = forward(sdt, cfg, y.to(dtype), yh, masks, train)
    outs = flat_outputs(*res[:4])
    leaves = [sdt[k] for k in keys] + ([] if upstream == "d" else [yh])
    if upstream == "d":
        loss = d_loss(res[0], res[1])
    elif upstream == "g":
        loss = g_loss(res[1], res[2], res[3])
    else:
        loss = sum((o * u.to(dtype)).sum() for o, u in zip(outs, upstream))
    grads = [g.detach() for g in torch.autograd.grad(loss, leaves)]
    dyh = None if upstream == "d" else grads[-1]
    return ([o.detach() for o in outs], dict(zip(keys, grads)), dyh, res[4], (float(loss.detach()) if isinstance(upstream, str) else None),
            res[5])


_own = {}


def own_inputs(name: str):
    """The lrelu inputs of the restatement run on its own (its own x > 0, training mode) in fp64 and in fp32, on ONE thread
    (voc_train_ref.own_inputs says why): what the mask tests take x64 and e_site from."""
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
    """The state dict after remove_weight_norm(): plain ``weight`` keys on the weight-normed scales (fp64 fold, rounded to fp32
    once); the spectral scale keeps its keys."""
    out = {}
    for k, v in sd.items():
        pre = k[:-len("weight_v")]
        if k.endswith(".weight_v") and pre + "weight_g" in sd:
            out[pre + "weight"] = torch._weight_norm(v.double(), sd[pre + "weight_g"].double(), 0).to(torch.float32)
        elif not k.endswith(".weight_g"):
            out[k] = v
    return out
