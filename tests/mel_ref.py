"""CPU restatement of the reference's ``mel_spectrogram`` (utils/vocoder/dataset.py:43-69, center=False) -- the same torch ops in
the same order -- with the mel basis and the window passed in, in the tensor's own dtype (fp32: what the reference computes;
fp64: the yardstick the goldens carry), and the Conv1d formulation the library evaluates (polyphase view + DFT-weight conv)."""
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

# tests/golden fixtures written by tools/make_mel_goldens.py
GOLDENS = ["mel_noise", "mel_tanh", "mel_voc_u40", "mel_tone", "mel_cfg2"]


def load_golden(golden_dir: str, name: str):
    """-> (npz, meta): wav (B, N), basis, window, mel_ref (the reference, fp32), mel_ref64 (the same formula in fp64)."""
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    return z, json.loads(str(z["meta"]))


def mel_ref(y: torch.Tensor, n_fft: int, hop: int, win: int, basis: torch.Tensor, window: torch.Tensor) -> torch.Tensor:
    """dataset.py:55-67 on y (B, N); basis (n_mels, n_fft // 2 + 1) and window (win,) are cast to y's dtype, so an fp64 ``y``
    evaluates the formula in fp64 FROM THE fp32 WINDOW AND BASIS the reference holds."""
    basis, window = basis.to(y.dtype), window.to(y.dtype)
    p = int((n_fft - hop) / 2)
    y = F.pad(y.unsqueeze(1), (p, p), mode="reflect").squeeze(1)
    spec = torch.stft(y, n_fft, hop_length=hop, win_length=win, window=window, center=False, pad_mode="reflect", normalized=False,
                      onesided=True, return_complex=True)
    spec = torch.sqrt(torch.real(spec).pow(2) + torch.imag(spec).pow(2) + (1e-9))
    spec = torch.matmul(basis, spec)
    return torch.log(torch.clamp(spec, min=1e-5))


def dft_conv_weights(n_fft: int, hop: int, win: int, window: torch.Tensor) -> torch.Tensor:
    """(2 (n_fft / 2 + 1), hop, ceil(n_fft / hop)) fp64: W[o][c][j] = w[n] cos(2 pi f n / n_fft) for the real rows, -w[n] sin(...)
    for the imaginary rows, n = j hop + c, zero where n >= n_fft; w = the fp32 window zero-padded, centred, to n_fft (torch.stft);
    the angle is reduced as (f n) mod n_fft before cos / sin."""
    F_, k = n_fft // 2 + 1, -(-n_fft // hop)
    w = torch.zeros(n_fft, dtype=torch.float64)
    left = (n_fft - win) // 2
    w[left: left + win] = window.to(torch.float32).to(torch.float64)
    n = torch.arange(k * hop, dtype=torch.int64)
    f = torch.arange(F_, dtype=torch.int64)
    ang = 2.0 * math.pi * ((f[:, None] * n[None, :]) % n_fft).to(torch.float64) / n_fft
    wn = torch.cat([w, torch.zeros(k * hop - n_fft, dtype=torch.float64)])
    W = torch.cat([wn * torch.cos(ang), -wn * torch.sin(ang)], 0)  # (2F, k hop), zero beyond n_fft through wn
    return W.reshape(2 * F_, k, hop).permute(0, 2, 1).contiguous()


def mel_conv_form(y: torch.Tensor, n_fft: int, hop: int, win: int, basis: torch.Tensor, window: torch.Tensor) -> torch.Tensor:
    """The library's formulation in y's dtype: reflect pad -> polyphase view x[c][t] = padded[t hop + c] of shape
    (hop, T + k - 1) -> Conv1d(hop -> 2F, k) with ``dft_conv_weights`` rounded to fp32 -> magnitude -> 1x1 mel conv -> log-clamp."""
    B, N = y.shape
    F_, k, T = n_fft // 2 + 1, -(-n_fft // hop), N // hop
    p = int((n_fft - hop) / 2)
    pad = F.pad(y.unsqueeze(1), (p, p), mode="reflect").squeeze(1)
    cols = T + k - 1
    need = cols * hop
    pad = F.pad(pad, (0, max(0, need - pad.shape[1])))[:, :need]
    x = pad.reshape(B, cols, hop).transpose(1, 2)
    W = dft_conv_weights(n_fft, hop, win, window).to(torch.float32).to(y.dtype)
    spec = F.conv1d(x, W)
    mag = torch.sqrt(spec[:, :F_].pow(2) + spec[:, F_:].pow(2) + 1e-9)
    mel = F.conv1d(mag, basis.to(y.dtype).unsqueeze(-1))
    return torch.log(torch.clamp(mel, min=1e-5))
