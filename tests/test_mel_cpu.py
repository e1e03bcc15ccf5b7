"""CPU: the host side of the mel metric (parrot_tts_amd/mel.py, cli/voc_eval.py) and the yardsticks the GPU tests use -- the torch
restatement tests/mel_ref.py against the reference's own outputs (tests/golden/mel_*.npz, tools/make_mel_goldens.py), the Conv1d
formulation the library evaluates, the Slaney mel basis, and the driver's batching / aggregation against a stub generator."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mel_ref as R  # noqa: E402
from parrot_tts_amd import mel as M  # noqa: E402
from parrot_tts_amd.cli import voc_eval  # noqa: E402


def _args(z, m):
    return m["n_fft"], m["hop_size"], m["win_size"], torch.from_numpy(z["basis"]), torch.from_numpy(z["window"])


@pytest.mark.parametrize("name", R.GOLDENS)
def test_restatement_equals_the_reference_bit_for_bit(golden_dir, name):
    """tests/mel_ref.py (fp32) against what the reference's mel_spectrogram returned: the same torch ops in the same order, so
    the same bits (checked to hold for 1, 2, 8 and 16 CPU threads); its fp64 evaluation equals the stored one, and the
    stored d_ref is the distance of the two."""
    z, m = R.load_golden(golden_dir, name)
    wav = torch.from_numpy(z["wav"])
    out = R.mel_ref(wav, *_args(z, m))
    assert out.dtype == torch.float32 and tuple(out.shape) == z["mel_ref"].shape == (wav.shape[0], m["num_mels"], wav.shape[1] // m["hop_size"])
    assert torch.equal(out, torch.from_numpy(z["mel_ref"]))
    out64 = R.mel_ref(wav.double(), *_args(z, m))
    assert float((out64 - torch.from_numpy(z["mel_ref64"])).abs().max()) <= 1e-12
    d_ref = float((torch.from_numpy(z["mel_ref"]).double() - torch.from_numpy(z["mel_ref64"])).abs().max())
    assert d_ref == m["d_ref"] and 0 < d_ref < 1e-2
    assert m["frames"] == wav.shape[1] // m["hop_size"]


@pytest.mark.parametrize("name", R.GOLDENS)
def test_conv_formulation_in_fp64_is_within_d_ref(golden_dir, name):
    """Reflect pad -> polyphase view -> Conv1d with the DFT weights formed in fp64 from the fp32 window and rounded to fp32 ->
    magnitude -> 1x1 mel conv -> log-clamp, evaluated in fp64: within d_ref of the fp64 reference (what is left is the rounding
    of the weights)."""
    z, m = R.load_golden(golden_dir, name)
    out = R.mel_conv_form(torch.from_numpy(z["wav"]).double(), *_args(z, m))
    d = float((out - torch.from_numpy(z["mel_ref64"])).abs().max())
    print(f"{name}: fp64 conv form {d:.3e}, d_ref {m['d_ref']:.3e}")
    assert d <= m["d_ref"]


def test_conv_weights_layout_and_partial_last_tap():
    W = R.dft_conv_weights(400, 160, 320, torch.hann_window(320))
    assert tuple(W.shape) == (2 * 201, 160, 3)
    n = (torch.arange(3)[None, :] * 160 + torch.arange(160)[:, None])  # n = j hop + c
    assert torch.all(W[:, n >= 400] == 0)                                # the partial last tap
    assert torch.all(W[:, n < 40] == 0) and torch.all(W[:, (n >= 360) & (n < 400)] == 0)  # window zero-padded, centred: 40 + 320 + 40
    assert torch.equal(W[0][n == 200], torch.hann_window(320)[160:161].double())  # f = 0: the fp32 window itself
    assert torch.all(W[201] == 0)                                        # -sin(0)


@pytest.mark.parametrize("sr,n_fft,n_mels,fmin,fmax", [(16000, 1024, 80, 0, None), (16000, 1024, 80, 0, 8000), (16000, 400, 40, 0, 8000),
                                                       (22050, 1024, 80, 55.0, 7600.0)])
def test_slaney_mel_basis_properties(sr, n_fft, n_mels, fmin, fmax):
    B = M.slaney_mel_basis_restated(sr, n_fft, n_mels, fmin, fmax)
    n_freq = n_fft // 2 + 1
    assert B.shape == (n_mels, n_freq) and B.dtype == np.float32 and np.all(B >= 0) and np.all(np.isfinite(B))
    top = sr / 2 if fmax is None else fmax
    edges = M.mel_to_hz(np.linspace(M.hz_to_mel(fmin), M.hz_to_mel(top), n_mels + 2))
    bin_hz = (sr / 2) / (n_freq - 1)
    for i in range(n_mels):
        nz = np.nonzero(B[i])[0]
        assert nz.size > 0 and np.all(np.diff(nz) == 1)                    # one contiguous support ...
        k = int(np.argmax(B[i]))
        assert np.all(np.diff(B[i, nz[0]: k + 1]) >= 0) and np.all(np.diff(B[i, k: nz[-1] + 1]) <= 0)  # ... rising then falling: one triangle
        freqs = nz * bin_hz
        assert freqs[0] > edges[i] - 1e-6 and freqs[-1] < edges[i + 2] + 1e-6  # between its own edges
        # Slaney norm: a triangle of height 2 / (f_hi - f_lo) has area 1 in Hz, so the samples sum to 1 / bin_hz = 2 (bin rate) /
        # bandwidth x (bandwidth / 2) -- within the discretisation: sampling a triangle of base w on a grid of step h misses its
        # area by at most one sample of its peak, h * height
        width = edges[i + 2] - edges[i]
        assert abs(B[i].sum() * bin_hz - 1.0) <= 2.0 * bin_hz / width + 1e-6
    # the scale: 200/3 Hz per mel below 1 kHz, 27 mels per factor 6.4 above
    assert np.allclose(M.hz_to_mel([0, 200, 1000]), [0, 3, 15]) and np.allclose(M.hz_to_mel(6400.0), 15 + 27)
    assert np.allclose(M.mel_to_hz(M.hz_to_mel([10.0, 999.0, 1000.0, 1001.0, 7999.0])), [10.0, 999.0, 1000.0, 1001.0, 7999.0])
    lin = edges[edges < 1000.0]
    if lin.size > 2:
        assert np.allclose(np.diff(lin), np.diff(lin)[0])                  # linear below 1 kHz
    log = edges[edges > 1000.0]
    if log.size > 2:
        assert np.allclose(log[1:] / log[:-1], log[1] / log[0])            # logarithmic above
    try:                                                                   # the one place the restatement can be pinned:
        from librosa.filters import mel as librosa_mel                     # against librosa itself, where it is installed
    except ImportError:
        return
    L = np.asarray(librosa_mel(sr=sr, n_fft=n_fft, n_mels=n_mels, fmin=fmin, fmax=float(sr) / 2 if fmax is None else fmax))
    assert L.shape == B.shape and np.allclose(L, B, rtol=1e-6, atol=1e-9)  # (float32 values formed from the same fp64 ramps)
    assert np.array_equal(M.slaney_mel_basis(sr, n_fft, n_mels, fmin, fmax), L.astype(np.float32))


def test_golden_basis_is_the_restated_one(golden_dir):
    z, m = R.load_golden(golden_dir, "mel_noise")
    assert np.array_equal(z["basis"], M.slaney_mel_basis_restated(16000, 1024, 80, 0, None))
    assert np.array_equal(z["window"], torch.hann_window(1024).numpy())


def test_frame_counts_and_cpu_tensors_raise():
    m = M.MelSpectrogram(dict(n_fft=1024, num_mels=80, sampling_rate=16000, hop_size=256, win_size=1024, fmin=0, fmax=8000, fmax_for_loss=None))
    assert m.fmax == 8000.0 and m.pad == 384 and m.n_freq == 513   # fmax_for_loss null = sr / 2, not h.fmax
    assert [m.frames(n) for n in (0, 255, 256, 8960, 81920, 81921)] == [0, 0, 1, 35, 320, 320]
    assert M.MelSpectrogram(dict(n_fft=400, num_mels=40, sampling_rate=16000, hop_size=160, win_size=320, fmin=0), fmax=8000).frames(8000) == 50
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.mel_spectrogram(torch.zeros(1, 8960), 1024, 80, 16000, 256, 1024, 0, 8000)
    with pytest.raises(NotImplementedError):
        M.mel_spectrogram(torch.zeros(1, 8960), 1024, 80, 16000, 256, 1024, 0, 8000, center=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(2, 8960))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.mel_l1(torch.zeros(1, 80, 4), torch.zeros(1, 80, 4))
    with pytest.raises(ValueError):
        M.MelSpectrogram(dict(n_fft=1024))
    with pytest.raises(ValueError):
        M.MelSpectrogram(dict(n_fft=1024, num_mels=80, sampling_rate=16000, hop_size=256, win_size=1024, fmin=0), basis=np.zeros((80, 512), np.float32))


def test_mel_entry_points_validate_before_any_device_call():
    import ctypes as C
    from parrot_tts_amd import _lib, build
    build.build()
    lib = _lib.lib()
    assert lib.parrot_mel_forward(None, None, 0, None, 1, 1024, None, None, 0, None) == -1 and b"null" in lib.parrot_last_error()
    assert lib.parrot_mel_l1(None, None, None, 1, 80, 4, None, None, None, 0, None) == -1
    assert lib.parrot_mel_create(None, None, None, None) == -1
    assert lib.parrot_mel_workspace_bytes(None, 1, 1024) == 0
    assert lib.parrot_mel_l1_workspace_bytes(3, 80, 35) >= 3 * 8 and lib.parrot_mel_l1_workspace_bytes(0, 80, 35) == 0
    assert C.sizeof(_lib.MelCfg) == 4 * 4


# ---- the driver against a stub generator ----------------------------------------------------------------------------------
class _StubGen:
    """A 'vocoder' on the CPU: sample t of a row is a fixed function of the unit it falls in."""
    multispkr = True
    hop = 320

    def out_samples(self, units):
        return units * self.hop

    def __call__(self, code, spkr, unit_lens):
        t = torch.arange(code.shape[1] * self.hop)
        u = code[:, t // self.hop].float()
        return (0.5 * torch.sin(0.01 * (u + 1 + spkr.float()) * (t % self.hop)[None, :])).unsqueeze(1)


class _StubMel:
    """tests/mel_ref.py row by row with each row's own length (what the device mel computes for a ragged batch)."""
    hop_size = 256
    pad = 384

    def __init__(self):
        self.basis = torch.from_numpy(M.slaney_mel_basis_restated(16000, 1024, 80, 0, None))
        self.window = torch.hann_window(1024)
        self.checked = 0

    def __call__(self, wav, n_samples, check=True):
        out = torch.zeros(wav.shape[0], 80, wav.shape[1] // 256)
        for b, n in enumerate(n_samples.tolist()):
            out[b, :, : n // 256] = R.mel_ref(wav[b: b + 1, :n], 1024, 256, 1024, self.basis, self.window)[0]
        return out

    def check(self, dev):
        self.checked += 1


def _stub_l1(a, b, n_frames):
    rows = torch.stack([(a[r, :, :n].double() - b[r, :, :n].double()).abs().mean() for r, n in enumerate(n_frames.tolist())])
    return None, rows


def test_voc_eval_names_an_utterance_no_longer_than_the_reflect_pad():
    """One 320-sample unit is shorter than the 384-sample reflect pad: the reference's F.pad would raise in the middle of the
    loop; the driver says which item before any batch runs."""
    rows = [(np.arange(9), 6, torch.zeros(9 * 320), "hi_f_0000"), (np.arange(1), 5, torch.zeros(320), "gu_m_0001")]
    mel = _StubMel()
    with pytest.raises(ValueError, match="gu_m_0001"):
        voc_eval.evaluate(_StubGen(), mel, rows, "cpu")
    assert mel.checked == 0


def test_voc_eval_aggregation_with_a_stub_generator(tmp_path, monkeypatch):
    from scipy.io import wavfile
    from parrot_tts_amd import data
    rng = np.random.Generator(np.random.PCG64(7))
    (tmp_path / "wavs").mkdir()
    recs, n_units = [], [9, 4, 13, 6, 2]
    for i, n in enumerate(n_units):
        wav = tmp_path / "wavs" / f"{('hi_f', 'gu_m')[i % 2]}_{i:04d}.wav"
        if i != 3:  # item 3 has no ground truth
            wavfile.write(str(wav), 16000, (rng.standard_normal(320 * n + 17 * i) * 3000).astype(np.int16))
        recs.append({"audio": str(wav), "hubert": " ".join(map(str, rng.integers(0, 100, n + (3 if i == 2 else 0)))), "duration": 0.1})
    man = tmp_path / "val.txt"
    man.write_text("".join(data.format_dict_line(r) for r in recs))
    h = {"multispkr": "_", "code_hop_size": 320, "sampling_rate": 16000}
    ns = type("A", (), dict(code_file=None, input_code_file=str(man), pad=None))
    ds = voc_eval.build_dataset(ns, voc_eval.AttrDict(h))
    rows, skipped = voc_eval.collect_rows(ds, h)
    assert skipped == 1 and [r[3] for r in rows] == ["hi_f_0000", "gu_m_0001", "hi_f_0002", "hi_f_0004"]
    assert [r[0].size for r in rows] == [9, 4, 13, 2] and [r[2].numel() for r in rows] == [9 * 320, 4 * 320, 13 * 320, 2 * 320]  # trimmed to whole units
    assert [r[1] for r in rows] == [6, 5, 6, 6]                                                                          # the fixed speaker table
    assert voc_eval.collect_rows(ds, h, n=2)[1] == 0 and len(voc_eval.collect_rows(ds, h, n=2)[0]) == 2
    monkeypatch.setattr(voc_eval, "mel_l1", _stub_l1)
    gen, mel = _StubGen(), _StubMel()
    batched = voc_eval.evaluate(gen, mel, rows, "cpu", max_rows=3, max_units=10000)
    single = voc_eval.evaluate(gen, mel, rows, "cpu", max_rows=1)
    assert mel.checked == 2 + 4
    assert np.array_equal(batched, single) and np.all(np.isfinite(batched)) and np.all(batched > 0)
    # each row is its own utterance: the value of row 1 (padded to 13 units in its batch) computed directly
    code = torch.from_numpy(rows[1][0])[None]
    w = gen(code, torch.tensor([[rows[1][1]]]), None)[:, 0]
    want = (R.mel_ref(rows[1][2][None], 1024, 256, 1024, mel.basis, mel.window).double() - R.mel_ref(w, 1024, 256, 1024, mel.basis, mel.window).double()).abs().mean()
    assert batched[1] == float(want)
    res = voc_eval.summarise(batched, [r[3] for r in rows], skipped, "f16x3", per_item=True)
    assert res["mel_spec_error"] == float(np.mean(batched)) and res["n_utterances"] == 4 and res["n_skipped_no_audio"] == 1
    assert res["precision"] == "f16x3" and list(res["items"]) == [r[3] for r in rows]
    assert "items" not in voc_eval.summarise(batched, [r[3] for r in rows], skipped, "f16x3")
    assert np.isnan(voc_eval.summarise(np.zeros(0), [], 2, "f16x3")["mel_spec_error"])
    with pytest.raises(SystemExit):
        voc_eval.main(["--input_code_file", str(man)])  # --checkpoint_file is required
