"""numpy fp64 restatement of ``ModelLoss`` (reference modules/loss.py:5-21) with its gradient, as parrot_tte_loss_grad defines it
(include/parrot_hip.h): the three losses, d (w_code code_loss + w_dur dur_loss) / d logits and / d log_dur.

    code_loss = sum over valid rows of (logsumexp(x[n]) - x[n, t_n]) / n_valid          (valid: t_n != ignore_index)
    dur_loss  = sum over set mask bytes of (log_dur[i] - log(dur[i] + 1))^2 / n_src
    grad_logits[n, v] = (w_code / n_valid) (softmax(x[n])[v] - [v == t_n])               0 for an ignored row
    grad_log_dur[i]   = (2 w_dur / n_src) (log_dur[i] - log(dur[i] + 1))                 0 outside the mask

Nothing valid (every row ignored / no mask byte set): that loss is NaN (0 / 0) and its gradient all zeros, as torch's autograd
gives.  A target outside [0, V) that is not the ignore index (torch raises IndexError) makes its row NaN and counts in n_bad."""
import numpy as np
import torch
import torch.nn.functional as F


def model_loss_typed(out, log_dur_preds, batch, num_codes: int):
    """tests/teacher_forced_ref.py::model_loss (modules/loss.py:12-21) with the duration target in the predictions' dtype, so that
    it also runs, and differentiates, in fp64 (``duration.float()`` makes an fp32 target, which F.mse_loss's backward refuses beside
    fp64 predictions).  In fp32 it is model_loss itself, operation for operation."""
    ld = log_dur_preds.masked_select(batch["src_mask"])
    lt = torch.log(batch["duration"].to(log_dur_preds.dtype) + 1).masked_select(batch["src_mask"])
    code_loss = F.cross_entropy(out.reshape(-1, num_codes), batch["codes"].reshape(-1), ignore_index=num_codes)
    dur_loss = F.mse_loss(ld, lt)
    return code_loss + dur_loss, code_loss, dur_loss


def tte_loss_and_grad(logits, targets, ignore_index, log_dur, dur, src_mask, weights=(1.0, 1.0)):
    """logits (N, V), targets (N) int, log_dur / dur / src_mask of one shape -> dict(losses (3) = {total, code, dur}, grad_logits
    (N, V), grad_log_dur (log_dur's shape), n_valid, n_src, n_bad), everything fp64."""
    x = np.asarray(logits, dtype=np.float64)
    t = np.asarray(targets).astype(np.int64)
    N, V = x.shape
    bad = (t != ignore_index) & ((t < 0) | (t >= V))
    valid = (t != ignore_index) & ~bad
    n_valid = int(valid.sum())
    m = x.max(axis=1, keepdims=True)
    e = np.exp(x - m)
    s = e.sum(axis=1, keepdims=True)
    nll = np.log(s[:, 0]) - (x[np.arange(N), np.where(valid, t, 0)] - m[:, 0])
    onehot = np.zeros((N, V))
    onehot[np.arange(N)[valid], t[valid]] = 1.0
    with np.errstate(invalid="ignore", divide="ignore"):
        code = np.float64(nll[valid].sum()) / np.float64(n_valid)
        g = np.zeros((N, V))
        if n_valid:
            g[valid] = (np.float64(weights[0]) / n_valid) * (e / s - onehot)[valid]
        g[bad] = np.nan
        ld = np.asarray(log_dur, dtype=np.float64)
        mask = np.asarray(src_mask).astype(bool)
        d = ld - np.log(np.asarray(dur).astype(np.float64) + 1.0)  # log(duration + 1), loss.py:14
        n_src = int(mask.sum())
        durl = np.float64((d[mask] ** 2).sum()) / np.float64(n_src)
        gd = np.zeros(ld.shape)
        if n_src:
            gd[mask] = (2.0 * np.float64(weights[1]) / n_src) * d[mask]
    return {"losses": np.array([code + durl, code, durl]), "grad_logits": g, "grad_log_dur": gd, "n_valid": n_valid, "n_src": n_src,
            "n_bad": int(bad.sum())}
