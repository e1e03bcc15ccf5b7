"""GPU: the mel L1 and its gradient with respect to the waveform on the device (parrot_mel_l1_grad; MelSpectrogram.l1_loss_and_grad,
mel_l1_trainable, MelL1Loss in parrot_tts_amd/mel.py).

The parity rule.  The yardstick is torch's autograd through tests/mel_ref.py in fp64; the metric, per row, is
max |g_dev - g_64| / max |g_64|.  The allowance is not a constant: torch's CPU fp32 autograd of the same loss is evaluated twice in
the test, through ``mel_ref`` (torch.stft) and through ``mel_conv_form`` (the Conv1d formulation), and the device may err by 2 x the
larger of the two errors on that fixture and row -- the margin the CTC tests give over torch's own fp32.  The targets are the fp64
log-mel plus a seeded offset of magnitude in [0.05, 0.55], so that no sgn hangs on the forward's rounding.
Measured (MI355X): see DESIGN.md section 4.

The whole file also passes under PARROT_POISON_WS=nan (workspace and outputs filled with NaN at the top of the entry point)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mel_grad_ref as G  # noqa: E402
import mel_ref as R  # noqa: E402
from parrot_tts_amd import _lib  # noqa: E402
from parrot_tts_amd import mel as M  # noqa: E402

DEV = "cuda:0"
GOLDEN = os.path.join(ROOT, "tests", "golden")
LOG_FLOOR = float(np.log(1e-5))


def _mel_of(z, m, precision=None):
    return M.MelSpectrogram(n_fft=m["n_fft"], num_mels=m["num_mels"], sampling_rate=m["sampling_rate"], hop_size=m["hop_size"],
                            win_size=m["win_size"], fmin=m["fmin"], fmax=m["fmax"], precision=precision, basis=z["basis"],
                            window=torch.from_numpy(z["window"]))


def _args(z, m):
    return m["n_fft"], m["hop_size"], m["win_size"], torch.from_numpy(z["basis"]), torch.from_numpy(z["window"])


def _rel(got, want):
    """per row: max |got - want| / max |want|"""
    return [float((got[b].double() - want[b]).abs().max() / want[b].abs().max()) for b in range(want.shape[0])]


def _yardstick(wav, target, lens, args, reduction="mean"):
    """-> (g64, tol (per row), loss64, row_sums64): the fp64 gradient and 2 x the larger error of torch's two fp32 evaluations."""
    loss64, g64, sums64 = G.autograd_loss_and_grad(R.mel_ref, wav, target, lens, *args, reduction=reduction)
    e_ref = _rel(G.autograd_loss_and_grad(R.mel_ref, wav, target, lens, *args, reduction=reduction, dtype=torch.float32)[1], g64)
    e_conv = _rel(G.autograd_loss_and_grad(R.mel_conv_form, wav, target, lens, *args, reduction=reduction, dtype=torch.float32)[1], g64)
    return g64, [2 * max(a, b) for a, b in zip(e_ref, e_conv)], loss64, sums64


_cache = {}


def _fixture(name):
    """One golden with its target and the yardstick of the dense batch under "mean": computed once, shared, never changed."""
    if name not in _cache:
        z, m = R.load_golden(GOLDEN, name)
        wav = torch.from_numpy(z["wav"])
        ref64 = torch.from_numpy(z["mel_ref64"])
        target = G.make_target(ref64, 1000 + R.GOLDENS.index(name))
        # what the targets rest on: no |d| near 0 (sgn is the same in every precision), no element on the clamp
        assert float((ref64 - target.double()).abs().min()) >= 0.0499 and float(ref64.min()) > LOG_FLOOR + 1e-3
        g64, tol, loss64, _ = _yardstick(wav, target, None, _args(z, m))
        _cache[name] = dict(z=z, m=m, wav=wav, target=target, g64=g64, tol=tol, loss64=loss64)
    return _cache[name]


@pytest.mark.parametrize("precision", [None, "f32"])
@pytest.mark.parametrize("name", ["mel_noise", "mel_tanh", "mel_voc_u40", "mel_cfg2", "mel_tone"])
def test_golden_parity(name, precision):
    """Every row within 2 x torch's fp32 error of the fp64 gradient (the default f16x3 handle, and the exact-fp32 one with its grouped
    DFT: 8 groups at hop 256, 5 at hop 160); the loss equals mel_l1 of the forward bit for bit; two calls agree bit for bit."""
    f = _fixture(name)
    mel = _mel_of(f["z"], f["m"], precision)
    wav, target = f["wav"].to(DEV), f["target"].to(DEV)
    loss, grad = mel.l1_loss_and_grad(wav, target)
    assert mel.precision_in_use(DEV) == (precision or "f16x3")
    assert loss.dtype == torch.float32 and loss.dim() == 0 and grad.dtype == torch.float32 and grad.shape == wav.shape
    err = _rel(grad.cpu(), f["g64"])
    for b, (e, t) in enumerate(zip(err, f["tol"])):
        print(f"MELGRAD {name} {precision or 'f16x3'} row {b}: device {e:.3e}, allowed {t:.3e} (2 x torch fp32), max |g| {float(f['g64'][b].abs().max()):.3e}")
    want, _ = M.mel_l1(mel(wav), target)
    assert torch.equal(loss, want)
    assert abs(float(loss) - float(f["loss64"])) <= 4 * f["m"]["d_ref"]  # (every element of the forward is within 4 x d_ref)
    loss2, grad2 = mel.l1_loss_and_grad(wav, target)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
    assert all(e <= t for e, t in zip(err, f["tol"])), (err, f["tol"])


def test_sum_and_scale():
    """"sum": the loss is the fp64 row sums added in row order; the gradient is the mean's times the count (one rounding each);
    ``scale`` is a plain factor; (B, 1, N) is taken as the forward takes it."""
    f = _fixture("mel_tanh")
    mel = _mel_of(f["z"], f["m"])
    wav, target = f["wav"].to(DEV), f["target"].to(DEV)
    loss, grad = mel.l1_loss_and_grad(wav, target, reduction="sum")
    assert loss.dtype == torch.float64 and loss.dim() == 0
    out = mel(wav)
    n_row = out.shape[1] * out.shape[2]
    rows = (out.double() - target.double()).abs().sum(dim=(1, 2))  # (torch's order of summation)
    assert abs(float(loss) - float(rows.sum())) <= 2.0 ** -36 * float(loss)
    # bit for bit: the entry point's own fp64 row sums, added in row order
    B, N = wav.shape
    lib = _lib.lib()
    from parrot_tts_amd.ops import dptr, stream_ptr
    dev = torch.device(DEV)
    o64 = torch.empty(2 * B, dtype=torch.float64, device=DEV)
    l64 = torch.empty((), dtype=torch.float64, device=DEV)
    g = torch.empty_like(wav)
    h = mel._handle(dev)
    ws = torch.empty(int(lib.parrot_mel_l1_grad_workspace_bytes(h, B, N)), dtype=torch.uint8, device=DEV)
    _lib.check(lib.parrot_mel_l1_grad(h, dptr(wav), wav.stride(0), None, dptr(target), B, N, 1, 1.0, dptr(o64), dptr(l64), dptr(g), dptr(ws),
                                      ws.numel(), stream_ptr(dev)))
    mel.check(DEV)
    tot = 0.0
    for b in range(B):
        tot += float(o64[b])
    assert float(l64) == tot == float(loss) and torch.equal(g, grad)
    assert o64[B:].tolist() == [float(n_row)] * B
    _, g_mean = mel.l1_loss_and_grad(wav, target)
    assert float((grad.double() / (B * n_row) - g_mean.double()).abs().max()) <= 2.0 ** -22 * float(g_mean.abs().max())
    g45 = torch.empty_like(wav)  # the entry point's `scale` (the Python functions pass 1)
    _lib.check(lib.parrot_mel_l1_grad(h, dptr(wav), wav.stride(0), None, dptr(target), B, N, 1, 45.0, dptr(o64), dptr(l64), dptr(g45), dptr(ws),
                                      ws.numel(), stream_ptr(dev)))
    mel.check(DEV)
    assert float(l64) == float(loss)
    assert float((g45.double() - 45.0 * grad.double()).abs().max()) <= 2.0 ** -23 * 45.0 * float(grad.abs().max())
    loss3, grad3 = mel.l1_loss_and_grad(wav.unsqueeze(1), target, reduction="sum")
    assert torch.equal(loss3, loss) and torch.equal(grad3, grad)


@pytest.mark.parametrize("name,precision", [("mel_tanh", None), ("mel_cfg2", "f32")])
def test_ragged_batch(name, precision):
    """n_samples = [N, N * 5 // 9, n_fft + 1] with a NaN tail that must never be read.  "sum": a row's gradient equals that utterance
    run alone bit for bit and is exactly 0 beyond its end.  "mean": every row within the allowance of the fp64 gradient, which
    carries the batch's count."""
    f = _fixture(name)
    z, m = f["z"], f["m"]
    mel, hop = _mel_of(z, m, precision), m["hop_size"]
    clean = f["wav"]
    N = clean.shape[1]
    lens = [N, N * 5 // 9, m["n_fft"] + 1]
    wav = clean.clone()
    for b, n in enumerate(lens):
        wav[b, n:] = float("nan")
    # the target of a ragged row comes from that row's OWN fp64 mel (its last frames see the reflection at its end)
    ref = [R.mel_ref(clean[b: b + 1, :n].double(), *_args(z, m)) for b, n in enumerate(lens)]
    target_cpu = torch.zeros_like(f["target"])
    for b, n in enumerate(lens):
        target_cpu[b, :, : n // hop] = G.make_target(ref[b], 50 + b)[0]
        assert float((ref[b][0] - target_cpu[b, :, : n // hop].double()).abs().min()) >= 0.0499 and float(ref[b].min()) > LOG_FLOOR + 1e-3
    target = target_cpu.to(DEV)
    loss, grad = mel.l1_loss_and_grad(wav.to(DEV), target, lens, reduction="sum")
    total = 0.0
    for b, n in enumerate(lens):
        l1, g1 = mel.l1_loss_and_grad(clean[b: b + 1, :n].contiguous().to(DEV), target[b: b + 1, :, : n // hop].contiguous(), reduction="sum")
        assert torch.equal(grad[b, :n], g1[0]), b
        assert torch.all(grad[b, n:] == 0), b
        total += float(l1)
    assert float(loss) == total
    # "mean": against fp64
    g64, tol, loss64, _ = _yardstick(clean, target_cpu, lens, _args(z, m))
    loss_m, grad_m = mel.l1_loss_and_grad(wav.to(DEV), target, torch.tensor(lens, device=DEV))
    want, _ = M.mel_l1(mel(wav.to(DEV), lens), target, [n // hop for n in lens])
    assert torch.equal(loss_m, want) and abs(float(loss_m) - float(loss64)) <= 4 * m["d_ref"]
    err = _rel(grad_m.cpu(), g64)
    for b, (e, t) in enumerate(zip(err, tol)):
        print(f"MELGRAD ragged {name} {precision or 'f16x3'} row {b} (n = {lens[b]}): device {e:.3e}, allowed {t:.3e}")
    for b, n in enumerate(lens):
        assert torch.all(grad_m[b, n:] == 0)
    assert all(e <= t for e, t in zip(err, tol)), (err, tol)


def test_silence():
    """0.1-amplitude noise with a zero stretch longer than 3 n_fft: every mel bin of an all-silent frame is ~2e-6, 0.79 of the
    threshold below the clamp, so the clamp blocks its gradient in fp32 and fp64 alike.  The gradient is finite everywhere and
    exactly 0 at the samples that only all-silent frames cover."""
    f = _fixture("mel_noise")
    z, m = f["z"], f["m"]
    n_fft, hop, N = m["n_fft"], m["hop_size"], 8960
    pad = (n_fft - hop) // 2
    g = torch.Generator().manual_seed(77)
    wav = 0.1 * torch.randn(1, N, generator=g)
    z0, z1 = 2000, 2000 + 3 * n_fft + 128
    wav[0, z0:z1] = 0.0
    ref64 = R.mel_ref(wav.double(), *_args(z, m))
    T = N // hop
    start = np.arange(T) * hop - pad  # frame t reads samples [start, start + n_fft) (away from the ends: no mirror inside the stretch)
    silent = (start >= z0) & (start + n_fft <= z1)
    pre = G.staged_forward(wav.double(), None, *_args(z, m))["mel"][0][:, torch.from_numpy(silent)]  # the pre-clamp mel
    assert silent.sum() >= 3 and 1e-6 < float(pre.min()) and float(pre.max()) < 0.3e-5
    i = np.arange(N)
    covered_by_live = np.zeros(N, dtype=bool)
    for t in np.nonzero(~silent)[0]:
        covered_by_live |= (i >= start[t]) & (i < start[t] + n_fft)
    only_silent = ~covered_by_live
    only_silent[: pad + 1] = False  # (the mirrored ends belong to live frames)
    only_silent[N - pad - 1:] = False
    assert only_silent.sum() >= n_fft
    target = G.make_target(ref64, 5)
    mel = _mel_of(z, m)
    loss, grad = mel.l1_loss_and_grad(wav.to(DEV), target.to(DEV))
    grad = grad.cpu()
    assert torch.isfinite(grad).all() and torch.isfinite(loss)
    assert torch.all(grad[0, torch.from_numpy(only_silent)] == 0)
    assert float(grad[0, torch.from_numpy(~only_silent)].abs().max()) > 0
    # and it is the gradient: the same allowance as on the goldens
    live = torch.from_numpy(~silent)
    assert float((ref64[0][:, live] - target.double()[0][:, live]).abs().min()) >= 0.0499
    g64, tol, _, _ = _yardstick(wav, target, None, _args(z, m))
    err = _rel(grad, g64)
    print(f"MELGRAD silence: device {err[0]:.3e}, allowed {tol[0]:.3e}")
    assert err[0] <= tol[0]


def test_autograd_through_a_small_conv():
    """train.py:157 as it would read: a small torch Conv1d produces (B, 1, N), ``MelL1Loss(h)(y, y_mel) * 45`` is backpropagated.
    The parameter gradients against the same graph with torch's device ops for the mel chain (in fp64); the allowance, per
    parameter, is 2 x the error of torch's CPU fp32 autograd of that graph against its fp64 evaluation (the larger of ``mel_ref`` and
    ``mel_conv_form``) -- the rule of the parity test, on the loss times 45.  This is an ABSOLUTE allowance per parameter
    tensor, formed the way the parity test forms its own, where the issue words it as the parity test's per-row relative tolerance
    scaled by 45: a per-row tolerance on d loss / d wav does not carry over to a sum over rows and samples without the Conv1d's
    Jacobian, so the same construction (2 x torch's own fp32 error against fp64) is applied to the quantity compared.  Runs under
    torch.use_deterministic_algorithms(True); the target gets no gradient."""
    f = _fixture("mel_tanh")
    z, m = f["z"], f["m"]
    args = _args(z, m)
    x = f["wav"].unsqueeze(1)
    torch.manual_seed(3)
    conv = torch.nn.Conv1d(1, 1, 5, padding=2)
    with torch.no_grad():
        conv.weight.mul_(0.2)
        conv.weight[0, 0, 2] += 0.9
        conv.bias.mul_(0.01)
    names = [n for n, _ in conv.named_parameters()]
    with torch.no_grad():
        y_mel64 = R.mel_ref(conv.double()(x.double())[:, 0], *args)
    conv.float()
    y_mel = G.make_target(y_mel64, 21)
    assert float((y_mel64 - y_mel.double()).abs().min()) >= 0.0499 and float(y_mel64.min()) > LOG_FLOOR + 1e-3

    def torch_graph(fn, conv_dtype, mel_dtype, device):
        c = torch.nn.Conv1d(1, 1, 5, padding=2)
        c.load_state_dict(conv.state_dict())
        c = c.to(device, conv_dtype)
        basis, window = args[3].to(device), args[4].to(device)
        y = c(x.to(device, conv_dtype))[:, 0].to(mel_dtype)
        loss = torch.nn.functional.l1_loss(fn(y, args[0], args[1], args[2], basis, window), y_mel.to(device, mel_dtype)) * 45
        loss.backward()
        return {n: p.grad.detach().cpu().double() for n, p in c.named_parameters()}, float(loss.detach())

    # the yardstick: the network as it is trained (fp32, torch's device conv), the mel chain by torch's device ops in fp64
    want, loss64 = torch_graph(R.mel_ref, torch.float32, torch.float64, DEV)
    cpu64, _ = torch_graph(R.mel_ref, torch.float64, torch.float64, "cpu")
    e = [torch_graph(fn, torch.float32, torch.float32, "cpu")[0] for fn in (R.mel_ref, R.mel_conv_form)]
    tol = {n: 2 * max(float((g[n] - cpu64[n]).abs().max()) for g in e) for n in names}

    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        net = torch.nn.Conv1d(1, 1, 5, padding=2)
        net.load_state_dict(conv.state_dict())
        net = net.to(DEV)
        crit = M.MelL1Loss(precision=None, basis=z["basis"], window=torch.from_numpy(z["window"]), n_fft=m["n_fft"], num_mels=m["num_mels"],
                           sampling_rate=m["sampling_rate"], hop_size=m["hop_size"], win_size=m["win_size"], fmin=m["fmin"], fmax=m["fmax"])
        tgt = y_mel.to(DEV).requires_grad_(True)
        y = net(x.to(DEV))
        assert y.shape[1] == 1
        loss = crit(y, tgt) * 45
        loss.backward()
    finally:
        torch.use_deterministic_algorithms(was)
    assert tgt.grad is None
    assert abs(float(loss) - loss64) <= 45 * 4 * m["d_ref"]
    for n, p in net.named_parameters():
        err = float((p.grad.cpu().double() - want[n]).abs().max())
        print(f"MELGRAD autograd {n}: max abs err {err:.3e}, allowed {tol[n]:.3e}, max |grad| {float(want[n].abs().max()):.3e}")
    for n, p in net.named_parameters():
        assert float((p.grad.cpu().double() - want[n]).abs().max()) <= tol[n], n
    # without a gradient to compute, the value is the same
    with torch.no_grad():
        assert torch.equal(crit(y.detach(), y_mel.to(DEV)) * 45, loss.detach())


def test_errors():
    """No fault is produced on purpose: each case is one of the forward's status paths or a host-side check."""
    f = _fixture("mel_noise")
    mel = _mel_of(f["z"], f["m"])
    wav, target = f["wav"].to(DEV), f["target"].to(DEV)
    good_loss, good = mel.l1_loss_and_grad(wav, target)
    bad = wav.clone()
    bad[1, 4000] = float("nan")
    for fn in (lambda w, n=None: mel.l1_loss_and_grad(w, target, n), lambda w, n=None: M.mel_l1_trainable(mel, w.clone().requires_grad_(True), target, n)):
        with pytest.raises(_lib.ParrotHipError) as e:  # status 5: nothing is returned
            fn(bad)
        assert e.value.code == -6
        with pytest.raises(_lib.ParrotHipError) as e:  # a row no longer than the reflect pad (384)
            fn(wav, [8960, 384, 8960])
        assert e.value.code == -1 and "reflect pad" in str(e.value)
        for counts in ([8960, 8961, 8960], [8960, -1, 8960], [28, 28]):
            with pytest.raises(ValueError, match="n_samples"):
                fn(wav, counts)
    for shape in ((3, 80, 34), (2, 80, 35), (3, 35, 80), (3, 80 * 35)):
        with pytest.raises(ValueError, match="target"):
            mel.l1_loss_and_grad(wav, torch.zeros(shape, device=DEV))
    with pytest.raises(ValueError):
        M.mel_l1_trainable(mel, wav, torch.zeros((3, 80, 34), device=DEV))  # (no gradient asked for: mel_l1's own check)
    with pytest.raises(RuntimeError, match="GPU"):
        mel.l1_loss_and_grad(wav.cpu(), target)
    with pytest.raises(RuntimeError, match="GPU"):
        mel.l1_loss_and_grad(wav, target.cpu())
    with pytest.raises(ValueError, match="reduction"):
        mel.l1_loss_and_grad(wav, target, reduction="none")
    lib = _lib.lib()
    assert lib.parrot_mel_l1_grad(mel._handle(torch.device(DEV)), None, 0, None, None, 3, 8960, 0, 1.0, None, None, None, None, 0, None) == -1
    assert int(lib.parrot_mel_l1_grad_workspace_bytes(mel._handle(torch.device(DEV)), 0, 8960)) == 0
    # and the handle is fine afterwards, in both directions
    loss, grad = mel.l1_loss_and_grad(wav, target)
    assert torch.equal(loss, good_loss) and torch.equal(grad, good)
    assert float((mel(wav).cpu().double() - torch.from_numpy(f["z"]["mel_ref64"])).abs().max()) <= 4 * f["m"]["d_ref"]


def test_whole_file_under_poison():
    """This file once more in a child process under PARROT_POISON_WS=nan: a kernel reading a byte of the workspace or of an output
    that nobody wrote would turn a gradient into NaN, and a sample of the gradient that nobody wrote stays NaN."""
    if os.environ.get("PARROT_POISON_WS"):
        return  # (already a poisoned run: the tests above were it)
    env = dict(os.environ, PARROT_POISON_WS="nan")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", os.path.abspath(__file__), "-k", "not whole_file"], cwd=ROOT,
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
