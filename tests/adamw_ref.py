"""The specification of the fused AdamW step (include/parrot_hip.h, csrc/optim.h) in numpy float32, op by op: every line is one
correctly rounded fp32 operation, as numpy performs it on float32 arrays, and nothing is contracted.  ``scalars`` is the host half
(Python doubles, each rounded to fp32 once); ``step64`` restates the same formula in float64 with the unrounded hyperparameters --
the yardstick both this rule and torch's AdamW are measured against."""
import math

import numpy as np

F = np.float32


def scalars(lr, beta1, beta2, eps, wd, step):
    """-> (decay, w1, b2, w2, e, ns, rs) as float32; step is the count after this update (>= 1)."""
    lr, beta1, beta2, eps, wd = float(lr), float(beta1), float(beta2), float(eps), float(wd)
    assert step >= 1
    decay, w1, b2, w2, e = 1.0 - lr * wd, 1.0 - beta1, beta2, 1.0 - beta2, eps
    ns = -lr / (1.0 - beta1 ** step)
    rs = math.sqrt(1.0 - beta2 ** step)
    return tuple(F(x) for x in (decay, w1, b2, w2, e, ns, rs))


def step(p, g, m, v, lr, beta1, beta2, eps, wd, step_no):
    """One update of float32 arrays -> new (p, m, v); the inputs are left as they are."""
    assert p.dtype == g.dtype == m.dtype == v.dtype == F
    decay, w1, b2, w2, e, ns, rs = scalars(lr, beta1, beta2, eps, wd, step_no)
    with np.errstate(all="ignore"):
        p = p * decay
        m = m + (g - m) * w1
        v = v * b2 + (g * w2) * g
        d = np.sqrt(v) / rs + e
        p = p + ns * (m / d)
    assert p.dtype == m.dtype == v.dtype == F
    return p, m, v


def step64(p, g, m, v, lr, beta1, beta2, eps, wd, step_no):
    """The same formula in float64 with the hyperparameters as given (g is taken as it is: the fp32 gradient, exactly)."""
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    with np.errstate(all="ignore"):
        p = p * (1.0 - lr * wd)
        m = m + (g - m) * (1.0 - beta1)
        v = v * beta2 + (g * (1.0 - beta2)) * g
        d = np.sqrt(v) / math.sqrt(1.0 - beta2 ** step_no) + eps
        p = p + (-lr / (1.0 - beta1 ** step_no)) * (m / d)
    return p, m, v


HYPER = [(2e-4, 0.8, 0.99, 0.01), (1e-3, 0.9, 0.999, 0.01), (1e-4, 0.9, 0.999, 0.0)]  # (lr, beta1, beta2, wd)
EPS = 1e-8


def problem(n, seed, steps):
    """p ~ N(0,1) 10^U(-3,0), g ~ N(0,1) 10^U(-8,0) with every 7th gradient zero -> (p0 (n), [g_1 .. g_steps]) float32."""
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 0, n)).astype(F)
    gs = []
    for _ in range(steps):
        g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 0, n)).astype(F)
        g[::7] = 0
        gs.append(g)
    return p, gs
