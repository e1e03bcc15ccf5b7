"""CPU yardsticks for the gradient of the mel L1 with respect to the waveform (parrot_mel_l1_grad):

    autograd_loss_and_grad   torch's autograd through tests/mel_ref.py (``mel_ref`` or ``mel_conv_form``), in the dtype asked for --
                             fp64: the yardstick; fp32: what the reference's trainer computes (train.py:157, loss_gen_all.backward())
    staged_loss_and_grad     a hand-written restatement of the five backward stages in the library's formulation (polyphase view,
                             transposed convs, gather-form frame adjoint with ragged n_samples), no autograd
    make_target              the tests' target: the fp64 log-mel plus an offset that keeps sgn away from the forward's rounding

Ragged batches: row b is its first n_samples[b] samples run alone (the reflection at its own end), n_samples[b] // hop frames."""
import numpy as np
import torch
import torch.nn.functional as F

import mel_ref as R


def _rows(wav, n_samples):
    B, N = wav.shape
    return [N] * B if n_samples is None else [int(n) for n in n_samples]


def make_target(logmel64: torch.Tensor, seed: int) -> torch.Tensor:
    """logmel64 + s u, u uniform in [0.05, 0.55], s = +-1, seeded; rounded to fp32."""
    g = torch.Generator().manual_seed(seed)
    u = 0.05 + 0.5 * torch.rand(logmel64.shape, generator=g, dtype=torch.float64)
    s = torch.randint(0, 2, logmel64.shape, generator=g).to(torch.float64) * 2 - 1
    return (logmel64.to(torch.float64) + s * u).to(torch.float32)


def autograd_loss_and_grad(fn, wav, target, n_samples, n_fft, hop, win, basis, window, reduction="mean", dtype=torch.float64):
    """-> (loss, grad (B, N), row_sums (B)) in ``dtype``: sum over rows of sum |fn(wav[b, :n_b]) - target[b, :, :n_b // hop]|, divided
    by the number of real elements for "mean"; grad is exactly 0 at and beyond n_b."""
    wav = wav.to(dtype).clone().requires_grad_(True)
    target = target.to(dtype)
    lens = _rows(wav, n_samples)
    sums, count = [], 0
    for b, n in enumerate(lens):
        t = n // hop
        mel = fn(wav[b: b + 1, :n], n_fft, hop, win, basis, window)
        assert mel.shape[-1] == t
        sums.append((mel - target[b: b + 1, :, :t]).abs().sum())
        count += mel.shape[1] * t
    total = torch.stack(sums).sum()
    loss = total / count if reduction == "mean" else total
    loss.backward()
    return loss.detach(), wav.grad.detach(), torch.stack(sums).detach()


def staged_forward(wav, n_samples, n_fft, hop, win, basis, window):
    """The library's forward on a ragged batch, in wav's dtype -> dict(x, W, re, im, mag, mel, logmel, frames, F, k, pad)."""
    B, N = wav.shape
    dt = wav.dtype
    F_, k, T, p = n_fft // 2 + 1, -(-n_fft // hop), N // hop, (n_fft - hop) // 2
    Tc = T + k - 1
    lens = _rows(wav, n_samples)
    x = torch.zeros(B, hop, Tc, dtype=dt)
    for b, n in enumerate(lens):  # mel_frame_kernel: x[b][c][j] = padded_b[j hop + c] for j < frames + k - 1, positions < n + 2 p
        fr = n // hop
        if fr == 0:
            continue
        pad = F.pad(wav[b, :n][None, None], (p, p), mode="reflect")[0, 0]
        need = (fr + k - 1) * hop
        pad = F.pad(pad, (0, max(0, need - pad.numel())))[:need]
        x[b, :, : fr + k - 1] = pad.reshape(fr + k - 1, hop).T
    W = R.dft_conv_weights(n_fft, hop, win, window).to(torch.float32).to(dt)
    spec = F.conv1d(x, W)
    re, im = spec[:, :F_], spec[:, F_:]
    mag = torch.sqrt(re.pow(2) + im.pow(2) + 1e-9)
    mel = F.conv1d(mag, basis.to(dt).unsqueeze(-1))
    frames = torch.tensor([n // hop for n in lens])
    live = (torch.arange(T)[None, :] < frames[:, None])[:, None, :]
    logmel = torch.where(live, torch.log(torch.clamp(mel, min=1e-5)), torch.zeros((), dtype=dt))
    return dict(x=x, W=W, re=re, im=im, mag=mag, mel=mel, logmel=logmel, live=live, lens=lens, F=F_, k=k, pad=p, T=T, Tc=Tc)


def staged_loss_and_grad(wav, target, n_samples, n_fft, hop, win, basis, window, reduction="mean", scale=1.0):
    """The five backward stages as the library runs them, in wav's dtype, no autograd -> (loss, grad (B, N))."""
    B, N = wav.shape
    dt = wav.dtype
    s = staged_forward(wav, n_samples, n_fft, hop, win, basis, window)
    k, p, Tc, lens = s["k"], s["pad"], s["Tc"], s["lens"]
    target = target.to(dt)
    d = torch.where(s["live"], s["logmel"] - target, torch.zeros((), dtype=dt))
    count = basis.shape[0] * sum(n // hop for n in lens)
    total = d.abs().sum()
    loss = total / count if reduction == "mean" else total
    # 1. head: sgn(d) [mel >= 1e-5] / mel on real frames, unit weight
    g_mel = torch.where(s["live"] & (s["mel"] >= 1e-5), torch.sign(d) / s["mel"], torch.zeros((), dtype=dt))
    # 2. mel projection transposed (1x1 conv with basis^T)
    g_mag = F.conv1d(g_mel, basis.to(dt).T.contiguous().unsqueeze(-1))
    # 3. magnitude backwards
    g_spec = torch.cat([g_mag * s["re"] / s["mag"], g_mag * s["im"] / s["mag"]], 1)
    # 4. framed DFT transposed: Wt[c][o][j'] = W[o][c][k - 1 - j'], padding k - 1
    g_poly = F.conv1d(g_spec, s["W"].permute(1, 0, 2).flip(2).contiguous(), padding=k - 1)
    assert g_poly.shape == (B, hop, Tc)
    # 5. frame adjoint, gather form: own position, left mirror, right mirror about n_b - 1, in that order; then the scale
    factor = scale / count if reduction == "mean" else scale
    grad = torch.zeros(B, N, dtype=dt)
    for b, n in enumerate(lens):
        fr = n // hop
        if n <= p or fr == 0:
            continue
        flat = g_poly[b].T.reshape(-1).numpy()  # flat[j hop + c]
        plim = min(n + 2 * p, (fr - 1) * hop + n_fft)
        i = np.arange(n)

        def at(q, ok):
            ok = ok & (q < plim) & (q >= 0)
            return np.where(ok, flat[np.where(ok, q, 0)], 0.0)

        v = at(i + p, np.ones(n, dtype=bool))
        v = v + at(p - i, (i >= 1) & (i <= p))
        v = v + at(2 * (n - 1) - i + p, (i <= n - 2) & (i >= n - 1 - p))
        grad[b, :n] = torch.from_numpy(v * factor)
    return loss, grad
