"""GPU: the log-mel spectrogram and the mel L1 on the device (parrot_tts_amd/mel.py over parrot_mel_forward / parrot_mel_l1) and
the voc_eval driver.

The parity rule: every element of the device mel is within 4 x d_ref of the reference formula evaluated in fp64, where d_ref is
the distance of the reference's OWN fp32 result from that fp64 value on the same input (the fixture's meta; computed in the test
for the full-size batch) and 4 is the project's allowance for a different fp32 summation order ("split <= 4x
exact").  No element is excluded."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from scipy.io import wavfile

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mel_ref as R  # noqa: E402
from parrot_tts_amd import _lib, data, synth  # noqa: E402
from parrot_tts_amd import mel as M  # noqa: E402
from parrot_tts_amd.cli import voc_eval  # noqa: E402
from parrot_tts_amd.vocoder import AttrDict, CodeGenerator  # noqa: E402

DEV = "cuda:0"
# two fp64 sums of the same n <= 25 600 exact terms in different orders differ by at most n x 2^-53 = 2.8e-12 relative < 2^-36
FP64_ORDER = 2.0 ** -36
MEL_H = dict(n_fft=1024, num_mels=80, sampling_rate=16000, hop_size=256, win_size=1024, fmin=0, fmax=8000, fmax_for_loss=None)


def _mel_of(z, m, precision=None):
    return M.MelSpectrogram(n_fft=m["n_fft"], num_mels=m["num_mels"], sampling_rate=m["sampling_rate"], hop_size=m["hop_size"],
                            win_size=m["win_size"], fmin=m["fmin"], fmax=m["fmax"], precision=precision, basis=z["basis"],
                            window=torch.from_numpy(z["window"]))


@pytest.mark.parametrize("precision", ["f16x3", "bf16x6", "f32"])
@pytest.mark.parametrize("name", R.GOLDENS)
def test_golden_parity(golden_dir, name, precision):
    """max |gpu - ref_fp64| <= 4 x d_ref of the fixture, every element.  Measured (MI355X): see DESIGN.md section 4."""
    z, m = R.load_golden(golden_dir, name)
    mel = _mel_of(z, m, precision)
    out = mel(torch.from_numpy(z["wav"]).to(DEV))
    assert mel.precision_in_use(DEV) == precision and tuple(out.shape) == z["mel_ref"].shape
    d = float((out.cpu().double() - torch.from_numpy(z["mel_ref64"])).abs().max())
    d32 = float((out.cpu() - torch.from_numpy(z["mel_ref"])).abs().max())
    print(f"MELPARITY {name} {precision}: gpu-fp64 {d:.3e} = {d / m['d_ref']:.2f} x d_ref ({m['d_ref']:.3e}); gpu-ref_fp32 {d32:.3e}")
    assert d <= 4 * m["d_ref"]


def test_reference_signature_and_handle_cache(golden_dir):
    z, m = R.load_golden(golden_dir, "mel_noise")
    wav = torch.from_numpy(z["wav"]).to(DEV)
    a = M.mel_spectrogram(wav, 1024, 80, 16000, 256, 1024, 0, None)
    n = len(M._cache)
    b = M.mel_spectrogram(wav, 1024, 80, 16000, 256, 1024, 0, None, center=False)
    assert len(M._cache) == n and torch.equal(a, b)
    assert float((a.cpu().double() - torch.from_numpy(z["mel_ref64"])).abs().max()) <= 4 * m["d_ref"]
    c = M.mel_spectrogram(wav, 1024, 80, 16000, 256, 1024, 0, 8000)  # sr / 2 spelled out: the same basis
    assert torch.equal(a, c)
    assert torch.equal(M.MelSpectrogram(MEL_H)(wav.unsqueeze(1)), a)   # the generator's (B, 1, N)
    assert torch.equal(M.MelSpectrogram(MEL_H)(torch.cat([wav, wav], 1)[:, :8960]), a)  # a strided view: row_stride


@pytest.fixture(scope="module")
def full_batch():
    h = synth.default_voc_config()
    g = CodeGenerator(AttrDict(h))
    g.load_state_dict(synth.synth_voc_state_dict(h, seed=1234))
    g = g.eval().to(DEV)
    b = synth.synth_voc_batch(64, 256, h, seed=3)
    wav = g(code=b["code"].to(DEV), spkr=b["spkr"].to(DEV))
    g.check_inputs()
    assert tuple(wav.shape) == (64, 1, 81920)
    return wav[:, 0].contiguous()


def test_full_size_batch(full_batch):
    """B = 64 x 81 920, the waveform of a synthesised batch; eight rows against the restatement in fp64, d_ref from the fp32
    restatement of the same rows."""
    mel = M.MelSpectrogram(MEL_H)
    out = mel(full_batch)
    assert tuple(out.shape) == (64, 80, 320)
    rows = [0, 9, 18, 27, 36, 45, 54, 63]
    w = full_batch[rows].cpu()
    args = (1024, 256, 1024, mel.basis, mel.window)
    ref64 = R.mel_ref(w.double(), *args)
    worst = 0.0
    for i, r in enumerate(rows):
        d_ref = float((R.mel_ref(w[i: i + 1], *args).double() - ref64[i: i + 1]).abs().max())
        d = float((out[r].cpu().double() - ref64[i]).abs().max())
        print(f"MELFULL row {r}: gpu-fp64 {d:.3e} = {d / d_ref:.2f} x d_ref ({d_ref:.3e}); peak |wav| {float(w[i].abs().max()):.3f}")
        worst = max(worst, d / d_ref)
        assert d <= 4 * d_ref, (r, d, d_ref)
    # every row of the batch equals that row alone (dense rows: no n_samples needed)
    assert torch.equal(mel(full_batch[63:64]), out[63:64])


def test_ragged_batch_rows_equal_their_own_run(golden_dir):
    z, m = R.load_golden(golden_dir, "mel_tanh")
    mel = _mel_of(z, m)
    lens = [8960, 5000, 2049]  # 35, 19 (5000 = 19 * 256 + 136) and 8 (2049 = 8 * 256 + 1) frames
    wav = torch.from_numpy(z["wav"]).clone()
    for b, n in enumerate(lens):
        wav[b, n:] = float("nan")  # the padding is poison: it must never be read
    out = mel(wav.to(DEV), lens)
    z2 = torch.from_numpy(z["wav"])
    for b, n in enumerate(lens):
        alone = mel(z2[b: b + 1, :n].contiguous().to(DEV))
        assert alone.shape[-1] == n // 256 == mel.frames(n)
        assert torch.equal(out[b: b + 1, :, : n // 256], alone), b
        assert torch.all(out[b, :, n // 256:] == 0)
        ref64 = R.mel_ref(z2[b: b + 1, :n].double(), m["n_fft"], m["hop_size"], m["win_size"], torch.from_numpy(z["basis"]), torch.from_numpy(z["window"]))
        assert float((alone.cpu().double() - ref64).abs().max()) <= 4 * m["d_ref"]  # (reflection at the row's own end)
    # frames beyond n // hop do not enter mel_l1
    other = _mel_of(z, m)(torch.from_numpy(np.load(os.path.join(golden_dir, "mel_noise.npz"))["wav"]).to(DEV))
    nf = [n // 256 for n in lens]
    mean, rows = M.mel_l1(out, other, nf)
    dirty = other.clone()
    for b, t in enumerate(nf):
        dirty[b, :, t:] = float("nan")
    mean2, rows2 = M.mel_l1(out, dirty, nf)
    assert torch.equal(mean, mean2) and torch.equal(rows, rows2)
    want_rows = torch.stack([(out[b, :, :t].double() - other[b, :, :t].double()).abs().mean() for b, t in enumerate(nf)])
    want_sum = sum(float((out[b, :, :t].double() - other[b, :, :t].double()).abs().sum()) for b, t in enumerate(nf))
    assert float(((rows - want_rows).abs() / want_rows).max()) <= FP64_ORDER
    assert abs(float(mean) - want_sum / (80 * sum(nf))) <= 2.0 ** -23 * want_sum / (80 * sum(nf))
    # a row's value does not depend on the width it is padded to
    _, rows_alone = M.mel_l1(out[1:2, :, : nf[1]].contiguous(), other[1:2, :, : nf[1]].contiguous())
    assert torch.equal(rows_alone[0], rows[1])


@pytest.mark.parametrize("name", ["mel_tanh", "mel_cfg2"])
def test_f32_grouped_dft_ragged(golden_dir, name):
    """f32 runs the framed DFT as a grouped conv whose partial sums the magnitude kernel adds (8 groups at hop 256, 5 at hop
    160): the unit_lens rule and the parity rule hold there as well, with a NaN tail and a frame count that is no multiple of 4."""
    z, m = R.load_golden(golden_dir, name)
    mel, hop = _mel_of(z, m, "f32"), m["hop_size"]
    clean = torch.from_numpy(z["wav"])
    N = clean.shape[1]
    lens = [N, N * 5 // 9, m["n_fft"] + 1]
    wav = clean.clone()
    for b, n in enumerate(lens):
        wav[b, n:] = float("nan")
    out = mel(wav.to(DEV), lens)
    assert torch.equal(out[0], mel(clean.to(DEV))[0])
    for b, n in enumerate(lens):
        alone = mel(clean[b: b + 1, :n].contiguous().to(DEV))
        assert torch.equal(out[b: b + 1, :, : n // hop], alone) and torch.all(out[b, :, n // hop:] == 0), b
        ref64 = R.mel_ref(clean[b: b + 1, :n].double(), m["n_fft"], hop, m["win_size"], torch.from_numpy(z["basis"]), torch.from_numpy(z["window"]))
        assert float((alone.cpu().double() - ref64).abs().max()) <= 4 * m["d_ref"]


def test_mel_l1_against_torch_fp64(golden_dir, full_batch):
    """An exact-order fp64 sum rounded once to fp32: relative error <= 2^-23 against torch's fp64 value on the same device mels;
    two calls agree bit for bit; F.l1_loss semantics for rows of one length."""
    mel = M.MelSpectrogram(MEL_H)
    a = mel(full_batch)
    b = mel(torch.roll(full_batch, 1, 0) * 0.7)
    for x, y in ((a, b), (a[:3, :, :35].contiguous(), b[:3, :, :35].contiguous()), (a[:1, :, :1].contiguous(), b[:1, :, :1].contiguous())):
        mean, rows = M.mel_l1(x, y)
        want = float(F.l1_loss(x.double(), y.double()))
        rel = abs(float(mean) - want) / want
        print(f"MELL1 {tuple(x.shape)}: mean {float(mean):.9g} torch fp64 {want:.12g} rel {rel:.2e}")
        assert mean.dtype == torch.float32 and mean.dim() == 0 and rel <= 2.0 ** -23
        want_rows = (x.double() - y.double()).abs().mean(dim=(1, 2))
        assert rows.dtype == torch.float64 and float(((rows - want_rows).abs() / want_rows).max()) <= FP64_ORDER
        mean2, rows2 = M.mel_l1(x, y)
        assert torch.equal(mean, mean2) and torch.equal(rows, rows2)
    assert float(M.mel_l1(a, a)[0]) == 0.0


def test_device_status(golden_dir):
    z, m = R.load_golden(golden_dir, "mel_noise")
    mel = _mel_of(z, m)
    wav = torch.from_numpy(z["wav"]).to(DEV)
    good = mel(wav)
    with pytest.raises(_lib.ParrotHipError) as e:  # a row no longer than the reflect pad (384): the reference's F.pad raises
        mel(wav, [8960, 384, 8960])
    assert e.value.code == -1 and "reflect pad" in str(e.value)
    assert torch.equal(mel(wav), good)  # the flag was cleared by the check that reported it
    assert torch.equal(mel(wav, [8960, 385, 8960])[0], good[0])  # one sample more than the pad is enough
    with pytest.raises(RuntimeError, match="Padding size"):
        mel(wav[:, :384].contiguous())
    for bad_counts in ([8960, 8961, 8960], [8960, -1, 8960], [28, 28, 28, 28]):  # host counts: beyond the row, negative, one too many
        with pytest.raises(ValueError, match="n_samples"):
            mel(wav, bad_counts)
    bad = wav.clone()
    bad[1, 4000] = float("nan")
    with pytest.raises(_lib.ParrotHipError) as e:
        mel(bad)
    assert e.value.code == -6
    bad[1, 4000] = float("inf")
    with pytest.raises(_lib.ParrotHipError) as e:
        mel(bad)
    assert e.value.code == -6
    assert torch.equal(mel(wav), good)
    # the status without a synchronisation
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    mel(bad, check=False)
    from parrot_tts_amd.ops import dptr, stream_ptr
    _lib.check(_lib.lib().parrot_mel_status_async(mel._handle(torch.device(DEV)), dptr(st), stream_ptr(torch.device(DEV))))
    assert int(st) == 5
    mel.check(DEV)  # cleared by the async read
    with pytest.raises(_lib.ParrotHipError) as e:  # the reduced-precision operating points are not offered
        M.MelSpectrogram(MEL_H, precision="bf16")(wav)
    assert e.value.code == -5


_PROBE = r"""
import hashlib, os, sys, numpy as np, torch
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import mel_ref as R
from parrot_tts_amd import mel as M
dev = "cuda:0"
def digest(*ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()[:16]
for name in R.GOLDENS:
    z, m = R.load_golden(os.path.join("tests", "golden"), name)
    mel = M.MelSpectrogram(n_fft=m["n_fft"], num_mels=m["num_mels"], sampling_rate=m["sampling_rate"], hop_size=m["hop_size"], win_size=m["win_size"],
                           fmin=m["fmin"], fmax=m["fmax"], basis=z["basis"], window=torch.from_numpy(z["window"]))
    wav = torch.from_numpy(z["wav"]).to(dev)
    out = mel(wav)
    lens = [wav.shape[1], wav.shape[1] * 5 // 9]
    rag = mel(wav[:2], lens)
    nf = [n // m["hop_size"] for n in lens]
    mean, rows = M.mel_l1(out[:2], rag, nf)
    print(name, mel.precision_in_use(dev), digest(out), digest(rag), digest(mean, rows))
# the exact-fp32 handle: the grouped DFT's padded rows and the partial sums the magnitude kernel reads back (hop 256: 8 groups; 160: 5)
for name in ("mel_tanh", "mel_cfg2"):
    z, m = R.load_golden(os.path.join("tests", "golden"), name)
    mel = M.MelSpectrogram(n_fft=m["n_fft"], num_mels=m["num_mels"], sampling_rate=m["sampling_rate"], hop_size=m["hop_size"], win_size=m["win_size"],
                           fmin=m["fmin"], fmax=m["fmax"], basis=z["basis"], window=torch.from_numpy(z["window"]), precision="f32")
    wav = torch.from_numpy(z["wav"]).to(dev)
    print(name, mel.precision_in_use(dev), digest(mel(wav)), digest(mel(wav[:2], [wav.shape[1], wav.shape[1] * 5 // 9])))
"""


def _probe(env):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", _PROBE], capture_output=True, text=True, env=e, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(R.GOLDENS) + 2
    return lines


@pytest.fixture(scope="module")
def plain_probe():
    return _probe({"PARROT_POISON_WS": "0", "PARROT_PRECISION": "f16x3"})


def test_poison_mode_leaves_the_results_unchanged(plain_probe):
    """Workspace, outputs and L1 partials filled with NaN at the top of every entry point: a kernel reading a byte nobody wrote
    would change the digests (the magnitude kernel's pad channels, the frames beyond a ragged row's end)."""
    assert _probe({"PARROT_POISON_WS": "nan", "PARROT_PRECISION": "f16x3"}) == plain_probe


def test_mel_does_not_move_with_the_vocoders_operating_point(plain_probe):
    """PARROT_PRECISION=bf16 (the reduced-precision operating point of the generator): the mel handle is built in f16x3 and its
    output is bit-identical to the default run."""
    got = _probe({"PARROT_POISON_WS": "0", "PARROT_PRECISION": "bf16"})
    assert got == plain_probe and [line.split()[1] for line in got] == ["f16x3"] * len(R.GOLDENS) + ["f32"] * 2
    assert _probe({"PARROT_POISON_WS": "0", "PARROT_PRECISION": "f16"}) == plain_probe


def test_voc_eval_end_to_end(tmp_path, capsys):
    """The driver on a temporary manifest of ragged items (some without a wav) with a small generator.  mel_spec_error against the
    per-item value computed on the CPU in fp64 (tests/mel_ref.py) from the waveform the generator returns for that item ALONE --
    the float waveform, as the reference's validation loop takes it (train.py:208-213), not the int16 PCM -- and from the
    dataset's ground truth.  The bound follows from the element rule: two mels each within 4 x d_ref of their fp64 values move a
    mean absolute difference by at most 4 (d_ref(ground truth) + d_ref(generated)); for the mean over items, the mean of these.
    Batched and one-row-per-batch runs print the same line, bit for bit."""
    h = synth.small_voc_config()
    h.update(MEL_H)
    cfg = tmp_path / "config.json"
    cfg.write_text(json.dumps(h))
    vsd = synth.synth_voc_state_dict(h, seed=41)
    torch.save({"generator": vsd}, tmp_path / "g_00000001")
    rng = np.random.Generator(np.random.PCG64(9))
    (tmp_path / "wavs").mkdir()
    recs, n_audio = [], [9, 23, 0, 5, 14, 2, 0, 31, 17]  # units of ground truth per item; 0: no wav
    for i, n in enumerate(n_audio):
        wav = tmp_path / "wavs" / f"{('hi_f', 'gu_m', 'en_f')[i % 3]}_{i:04d}.wav"
        if n:
            t = np.arange(320 * n + 13 * i)
            wavfile.write(str(wav), 16000, (3000 * np.sin(0.02 * (i + 1) * t) + 800 * rng.standard_normal(t.size)).astype(np.int16))
        recs.append({"audio": str(wav), "hubert": " ".join(map(str, rng.integers(0, 100, max(n, 4) + (i % 2) * 3))), "duration": 0.1})
    man = tmp_path / "val.txt"
    man.write_text("".join(data.format_dict_line(r) for r in recs))
    base = ["--checkpoint_file", str(tmp_path / "g_00000001"), "--config", str(cfg), "--input_code_file", str(man), "--per_item"]
    res = voc_eval.main(base + ["--batch_rows", "4", "--batch_units", "100"])
    line_batched = capsys.readouterr().out.strip().splitlines()[-1]
    res1 = voc_eval.main(base + ["--batch_rows", "1"])
    line_single = capsys.readouterr().out.strip().splitlines()[-1]
    assert line_batched == line_single and res == res1 and json.loads(line_batched) == res
    assert res["n_utterances"] == 7 and res["n_skipped_no_audio"] == 2 and res["precision"] == "f16x3"
    # item by item on the CPU
    g = CodeGenerator(AttrDict(h))
    g.load_state_dict(vsd)
    g = g.eval().to(DEV)
    ds = data.CodeDataset(data.parse_manifest(man), -1, 320, multispkr="_")
    basis, window = torch.from_numpy(M.slaney_mel_basis(16000, 1024, 80, 0, None)), torch.hann_window(1024)
    args = (1024, 256, 1024, basis, window)
    want, bound = [], []
    for i, n in enumerate(n_audio):
        feats, gt, filename, _ = ds[i]
        if gt is None:
            continue
        assert feats["code"].size == n and gt.shape == (1, 320 * n)
        spk = data.VOCODER_SPEAKERS[data.parse_speaker(filename, "_")]
        w = g(code=torch.from_numpy(feats["code"])[None].to(DEV), spkr=torch.tensor([[spk]], device=DEV))[:, 0].cpu()
        a64, b64 = R.mel_ref(gt.double(), *args), R.mel_ref(w.double(), *args)
        want.append(float((a64 - b64).abs().mean()))
        bound.append(4 * (float((R.mel_ref(gt, *args).double() - a64).abs().max()) + float((R.mel_ref(w, *args).double() - b64).abs().max())))
        name = os.path.splitext(os.path.basename(filename))[0]
        print(f"MELEVAL {name}: driver {res['items'][name]:.9g} cpu fp64 {want[-1]:.9g} diff {abs(res['items'][name] - want[-1]):.2e} bound {bound[-1]:.2e}")
        assert abs(res["items"][name] - want[-1]) <= bound[-1]
    g.check_inputs()
    assert len(want) == 7 and abs(res["mel_spec_error"] - float(np.mean(want))) <= float(np.mean(bound))
    assert res["mel_spec_error"] == float(np.mean([res["items"][k] for k in res["items"]]))
