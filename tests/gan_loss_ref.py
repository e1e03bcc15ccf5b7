"""A numpy fp64 restatement of the vocoder's adversarial losses and their gradients (parrot_tts_amd.gan_loss over parrot_gan_loss),
written from the formulas of include/parrot_hip.h:

    L1   mean |a - b|      d/db = sgn(b - a) / n,  d/da = -d/db
    SQ1  mean (1 - a)^2    d/da = -2 (1 - a) / n
    SQ0  mean a^2          d/da = 2 a / n

feature_loss = 2 sum of L1 terms over every (real, generated) feature-map pair; generator_loss = sum of SQ1 terms;
discriminator_loss = sum of (SQ1 of the real output + SQ0 of the generated one).  Shared by the CPU and the GPU tests; also the
table of the reference discriminators' layer constants and the shapes of their 62 generator-step terms."""
import numpy as np

L1, SQ1, SQ0 = 0, 1, 2


def term(op, a, b=None):
    """-> the term's mean (fp64; NaN for an empty array, numpy's and torch's mean of nothing)."""
    a = np.asarray(a, dtype=np.float64)
    if a.size == 0:
        return np.float64("nan")
    if op == L1:
        return np.abs(a - np.asarray(b, dtype=np.float64)).mean()
    return ((1.0 - a) ** 2).mean() if op == SQ1 else (a ** 2).mean()


def term_grad(op, a, b=None, w=1.0):
    """-> (grad_a, grad_b) of w * term (grad_b None for the squares), fp64 in a's shape."""
    a = np.asarray(a, dtype=np.float64)
    n = a.size
    if op == L1:
        gb = np.sign(np.asarray(b, dtype=np.float64) - a) * (w / n)
        return -gb, gb
    return (-2.0 * (1.0 - a) * w / n if op == SQ1 else 2.0 * a * w / n), None


def feature_loss(fmap_r, fmap_g):
    return 2.0 * sum(term(L1, rl, gl) for dr, dg in zip(fmap_r, fmap_g) for rl, gl in zip(dr, dg))


def feature_loss_grad(fmap_r, fmap_g, w=1.0):
    """-> (grads like fmap_r, grads like fmap_g) of w * feature_loss."""
    g = [[term_grad(L1, rl, gl, 2.0 * w) for rl, gl in zip(dr, dg)] for dr, dg in zip(fmap_r, fmap_g)]
    return [[p[0] for p in d] for d in g], [[p[1] for p in d] for d in g]


def generator_loss(disc_outputs):
    ls = [term(SQ1, dg) for dg in disc_outputs]
    return sum(ls), ls


def generator_loss_grad(disc_outputs, w=1.0):
    return [term_grad(SQ1, dg, None, w)[0] for dg in disc_outputs]


def discriminator_loss(disc_real_outputs, disc_generated_outputs):
    r = [term(SQ1, dr) for dr in disc_real_outputs]
    g = [term(SQ0, dg) for dg in disc_generated_outputs]
    return sum(a + b for a, b in zip(r, g)), r, g


def discriminator_loss_grad(disc_real_outputs, disc_generated_outputs, w=1.0):
    return ([term_grad(SQ1, dr, None, w)[0] for dr in disc_real_outputs], [term_grad(SQ0, dg, None, w)[0] for dg in disc_generated_outputs])


# ---------------------------------------------------------------------------------------------
# The reference discriminators' feature-map shapes (utils/vocoder/models.py:171-276), from their layer constants.
# ---------------------------------------------------------------------------------------------
PERIODS = (2, 3, 5, 7, 11)
# DiscriminatorP: Conv2d over (T / period, period) with kernel (k, 1): (c_out, k, stride, pad); the last row is conv_post
MPD_LAYERS = ((32, 5, 3, 2), (128, 5, 3, 2), (512, 5, 3, 2), (1024, 5, 3, 2), (1024, 5, 1, 2), (1, 3, 1, 1))
# DiscriminatorS: Conv1d (c_out, k, stride, pad, groups); the last row is conv_post
MSD_LAYERS = ((128, 15, 1, 7, 1), (128, 41, 2, 20, 4), (256, 41, 2, 20, 16), (512, 41, 4, 20, 16), (1024, 41, 4, 20, 16), (1024, 41, 1, 20, 16),
              (1024, 5, 1, 2, 1), (1, 3, 1, 1, 1))
MSD_POOL = (4, 2, 2)  # AvgPool1d(kernel, stride, padding) before the second and the third scale discriminator


def _conv_len(t, k, stride, pad):
    return (t + 2 * pad - k) // stride + 1


def mpd_shapes(B, T):
    """-> per period discriminator, the shapes of its 6 feature maps for a (B, 1, T) waveform (reflect-padded to the period)."""
    out = []
    for p in PERIODS:
        h = (T + p - 1) // p
        maps = []
        for c, k, s, pad in MPD_LAYERS:
            h = _conv_len(h, k, s, pad)
            maps.append((B, c, h, p))
        out.append(maps)
    return out


def msd_shapes(B, T):
    """-> per scale discriminator, the shapes of its 8 feature maps."""
    out = []
    t = T
    for i in range(3):
        if i:
            t = _conv_len(t, MSD_POOL[0], MSD_POOL[1], MSD_POOL[2])
        maps, u = [], t
        for c, k, s, pad, _ in MSD_LAYERS:
            u = _conv_len(u, k, s, pad)
            maps.append((B, c, u))
        out.append(maps)
    return out


def score_shape(fmap_shape):
    """The discriminator's score: its last feature map flattened from dim 1."""
    return (fmap_shape[0], int(np.prod(fmap_shape[1:])))
