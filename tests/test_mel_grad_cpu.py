"""CPU: the yardsticks of the mel-L1 gradient (tests/mel_grad_ref.py).  The hand-written restatement of the library's five backward
stages against torch's autograd through tests/mel_ref.py and against central differences, in fp64; and the host-side argument
checks of the Python entry points."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mel_grad_ref as G  # noqa: E402
import mel_ref as R  # noqa: E402
from parrot_tts_amd import mel as M  # noqa: E402

# a tiny configuration: k = 4 taps, 33 bins, reflect pad 24
TINY = dict(n_fft=64, hop=16, win=64, n_mels=8, N=160)


def _tiny():
    """3 rows: noise; noise with a silent stretch (whole frames of zeros: the clamp acts there); a ragged row of 100 samples."""
    c = TINY
    g = torch.Generator().manual_seed(5)
    wav = 0.1 * torch.randn(3, c["N"], generator=g, dtype=torch.float64)
    wav[1, 40:150] = 0.0
    lens = [c["N"], c["N"], 100]
    basis = torch.from_numpy(M.slaney_mel_basis_restated(16000, c["n_fft"], c["n_mels"], 0, 8000))
    window = torch.hann_window(c["win"])
    args = (c["n_fft"], c["hop"], c["win"], basis, window)
    ref = torch.zeros(3, c["n_mels"], c["N"] // c["hop"], dtype=torch.float64)
    for b, n in enumerate(lens):
        ref[b, :, : n // c["hop"]] = R.mel_ref(wav[b: b + 1, :n], *args)[0]
    return wav, lens, args, G.make_target(ref, 11).double()


@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_staged_restatement_equals_autograd_on_the_tiny_config(reduction):
    wav, lens, args, target = _tiny()
    assert float(R.mel_ref(wav[1:2], *args).min()) == pytest.approx(np.log(1e-5))  # the silent frames sit on the clamp
    loss_a, grad_a, _ = G.autograd_loss_and_grad(R.mel_ref, wav, target, lens, *args, reduction=reduction)
    loss_c, grad_c, _ = G.autograd_loss_and_grad(R.mel_conv_form, wav, target, lens, *args, reduction=reduction)
    loss_s, grad_s = G.staged_loss_and_grad(wav, target, lens, *args, reduction=reduction)
    scale = float(grad_a.abs().max())
    # fp64 against fp64: the DFT weights of the conv form are rounded to fp32 (2^-24 relative), torch.stft's are not
    assert scale > 0 and abs(float(loss_c - loss_a)) <= 1e-6 * float(loss_a) and abs(float(loss_s - loss_c)) <= 1e-12 * float(loss_c)
    assert float((grad_c - grad_a).abs().max()) <= 1e-5 * scale
    assert float((grad_s - grad_c).abs().max()) <= 1e-11 * scale
    assert torch.all(grad_s[2, lens[2]:] == 0) and torch.all(grad_a[2, lens[2]:] == 0)
    assert torch.isfinite(grad_s).all()
    # scale is a plain factor
    _, grad_45 = G.staged_loss_and_grad(wav, target, lens, *args, reduction=reduction, scale=45.0)
    assert float((grad_45 - 45.0 * grad_s).abs().max()) <= 1e-12 * 45 * scale


def test_staged_restatement_against_central_differences():
    """d loss / d wav[b, i] by central differences of the staged forward's own loss (h = 1e-6: the loss is piecewise smooth, and
    the target's offset keeps every |.| away from its kink; the clamp's kink sits 0.79 of the threshold away from the silent
    frames' bins), every sample of every row."""
    wav, lens, args, target = _tiny()
    _, grad = G.staged_loss_and_grad(wav, target, lens, *args, reduction="sum")

    def row_losses(w, n, tgt):  # every row of w is one utterance of n samples with the same target
        s = G.staged_forward(w, [n] * w.shape[0], *args)
        return torch.where(s["live"], s["logmel"] - tgt, torch.zeros((), dtype=torch.float64)).abs().sum(dim=(1, 2))

    h, worst = 1e-6, 0.0
    scale = float(grad.abs().max())
    N = wav.shape[1]
    for b, n in enumerate(lens):
        step = h * torch.eye(N, dtype=torch.float64)
        fd = (row_losses(wav[b] + step, n, target[b]) - row_losses(wav[b] - step, n, target[b])) / (2 * h)
        assert torch.all(fd[n:] == 0) and torch.all(grad[b, n:] == 0)
        worst = max(worst, float((fd - grad[b]).abs().max()))
    print(f"MELGRAD-FD worst |fd - grad| {worst:.3e}, max |grad| {scale:.3e}")
    assert worst <= 1e-5 * scale


@pytest.mark.parametrize("name", ["mel_cfg2", "mel_tanh"])
def test_staged_restatement_equals_autograd_on_a_golden(golden_dir, name):
    """k = 3 with a zero tap and a window shorter than n_fft (mel_cfg2), k = 4 (mel_tanh); the forward tests' ragged lengths."""
    z, m = R.load_golden(golden_dir, name)
    wav = torch.from_numpy(z["wav"]).double()
    N = wav.shape[1]
    lens = [N, N * 5 // 9, m["n_fft"] + 1]
    args = (m["n_fft"], m["hop_size"], m["win_size"], torch.from_numpy(z["basis"]), torch.from_numpy(z["window"]))
    target = G.make_target(torch.from_numpy(z["mel_ref64"]), 3).double()
    loss_a, grad_a, _ = G.autograd_loss_and_grad(R.mel_conv_form, wav, target, lens, *args)
    loss_s, grad_s = G.staged_loss_and_grad(wav, target, lens, *args)
    for b in range(3):
        assert float((grad_s[b] - grad_a[b]).abs().max()) <= 1e-10 * float(grad_a[b].abs().max())
        assert torch.all(grad_s[b, lens[b]:] == 0)
    assert abs(float(loss_s - loss_a)) <= 1e-12 * float(loss_a)


def test_python_entry_points_validate_on_the_host():
    mel = M.MelSpectrogram(n_fft=1024, num_mels=80, sampling_rate=16000, hop_size=256, win_size=1024, fmin=0, fmax=8000)
    wav, target = torch.zeros(2, 8960), torch.zeros(2, 80, 35)
    with pytest.raises(ValueError, match="reduction"):
        mel.l1_loss_and_grad(wav, target, reduction="none")
    with pytest.raises(ValueError, match="reduction"):
        M.mel_l1_trainable(mel, wav, target, reduction="none")
    with pytest.raises(ValueError, match="reduction"):
        M.MelL1Loss(dict(n_fft=1024, num_mels=80, sampling_rate=16000, hop_size=256, win_size=1024, fmin=0), reduction="batchmean")
    for call in (lambda: mel.l1_loss_and_grad(wav, target), lambda: M.mel_l1_trainable(mel, wav, target),
                 lambda: M.mel_l1_trainable(mel, wav.requires_grad_(True), target)):
        with pytest.raises((RuntimeError, ValueError), match="GPU|cuda|CUDA|device"):  # there is no CPU path
            call()
