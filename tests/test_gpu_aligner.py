"""GPU: the forced aligner on the device (parrot_tts_amd/aligner.py over parrot_aligner_forward / parrot_align_softmax /
parrot_align_durations) and the align_durations driver.

The parity rule is the mel's: every element of every tapped stage, of the logits and of pred is within 4 x d_ref of the reference
formula evaluated in fp64, where d_ref is the distance of the reference's OWN fp32 result from that fp64 value on the same input
(per stage, in the fixture's meta) and 4 is the project's allowance for a different fp32 summation order.  Frames in the padding
are included: the reference runs the network over them (utils/aligner/model.py:41-48) and so does the library.

Durations: exact.  The dynamic programme is held to the reference's durations wherever the cheapest path is unique, to the stored
fp64 cost bit for bit everywhere, and on tied rows to the documented rule (tests/aligner_ref.py).

The whole file also passes under PARROT_POISON_WS=nan (workspaces and outputs filled with NaN at the top of every entry point)."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import aligner_ref as R  # noqa: E402
from parrot_tts_amd import _lib, synth  # noqa: E402
from parrot_tts_amd import aligner as A  # noqa: E402
from parrot_tts_amd.cli import align_durations as CLI  # noqa: E402

DEV = "cuda:0"
PRECISIONS = ["f16x3", "bf16x6", "f32"]
_models = {}


def _cfg_of(m):
    cfg = synth.default_aligner_config()
    cfg["audio"]["n_mels"] = m["n_mels"]
    cfg["model"].update(lstm_dim=m["lstm_dim"], conv_dim=m["conv_dim"])
    return cfg


def _model(golden_dir, name, precision=None):
    """One model per (fixture, precision) for the whole module: the weights are rebuilt from the fixture's seed (and proven by its
    digest), packed once."""
    key = (name, precision)
    if key not in _models:
        z, m = R.load_golden(golden_dir, name)
        sd = synth.synth_aligner_state_dict(_cfg_of(m), m["num_symbols"], seed=m["seed"], gain=m["gain"])
        assert synth.state_digest(sd) == m["digest"]
        model = A.Aligner(m["n_mels"], m["num_symbols"], m["lstm_dim"], m["conv_dim"], precision=precision)
        model.load_state_dict(sd)
        _models[key] = model.eval().to(DEV)
    return _models[key]


def _ratio(got, want64, d_ref):
    return float((got.cpu().double() - torch.from_numpy(np.asarray(want64))).abs().max()) / d_ref


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", R.MODEL_GOLDENS)
def test_stage_and_logit_parity(golden_dir, name, precision):
    """Each tapped stage, the logits and pred within 4 x their own d_ref of the fp64 value, every element of every row, padding
    frames included.  Measured (MI355X): DESIGN.md section 4."""
    z, m = R.load_golden(golden_dir, name)
    model = _model(golden_dir, name, precision)
    mel = torch.from_numpy(z["mel"]).to(DEV)
    logits, st = model(mel, stages=True)
    assert model.precision_in_use == precision and tuple(logits.shape) == z["logits"].shape
    ratios = {}
    if "bn3" in z.files:
        ratios["bn3"] = _ratio(st["bn3"], z["bn364"], m["d_ref"]["bn3"])
    if "lstm" in z.files:
        got = st["lstm"][..., torch.from_numpy(z["lstm_channels"]).long().to(DEV)] if "lstm_channels" in z.files else st["lstm"]
        ratios["lstm"] = _ratio(got, z["lstm64"], m["d_ref"]["lstm"])
    ratios["logits"] = _ratio(logits, z["logits64"], m["d_ref"]["logits"])
    if "pred" in z.files:
        pred = model.softmax(logits, z["mel_len"].tolist())
        ratios["pred"] = _ratio(pred, z["pred64"], m["d_ref"]["pred"])
        for b, n in enumerate(z["mel_len"]):
            assert not pred[b, int(n):].any()  # frames at or beyond mel_len are written as zero
    print(f"ALIGNPARITY {name} {precision}: " + " ".join(f"{k} {v:.2f} x d_ref ({m['d_ref'][k]:.2e})" for k, v in ratios.items()))
    for k, v in ratios.items():
        assert v <= 4.0, (k, v)


def test_padding_quirk(golden_dir):
    """The shortest row of aligner_small inside its batch matches the fixture; run alone (B = 1, its own length) it matches
    logits_alone; the two differ by far more than the tolerance, so neither comparison can pass for the other."""
    z, m = R.load_golden(golden_dir, "aligner_small")
    model = _model(golden_dir, "aligner_small")
    b, n = m["alone_row"], int(z["mel_len"][m["alone_row"]])
    mel = torch.from_numpy(z["mel"]).to(DEV)
    inside = model(mel)[b, :n]
    alone = model(mel[b:b + 1, :n])[0]
    assert _ratio(inside, z["logits64"][b, :n], m["d_ref"]["logits"]) <= 4.0
    assert _ratio(alone, z["logits_alone64"], m["d_ref"]["logits_alone"]) <= 4.0
    gap = float((inside - alone).abs().max())
    assert gap > 100 * max(m["d_ref"]["logits"], m["d_ref"]["logits_alone"]), gap
    assert float(np.abs(z["logits"][b, :n] - z["logits_alone"]).max()) > 100 * m["d_ref"]["logits"]


def _dp_cases(golden_dir):
    """(name, tokens (N,), pred (T, V), reference durations, fp64 cost, unique) of align_dp and of the model fixtures' own pred."""
    z, m = R.load_golden(golden_dir, R.DP_GOLDEN)
    cases = [(c, z[c + "_tokens"], z[c + "_pred"], z[c + "_durations"], float(z[c + "_cost"]), m["unique"][c]) for c in m["cases"]]
    for name in ("aligner_small", "aligner_full"):
        zz, mm = R.load_golden(golden_dir, name)
        for b in range(len(zz["mel_len"])):
            T, N = int(zz["mel_len"][b]), int(zz["tokens_len"][b])
            cases.append((f"{name}[{b}]", zz["tokens"][b, :N], zz["pred"][b, :T], zz["durations"][b, :N], float(zz["cost"][b]), mm["unique"][b]))
    return cases


def _bits(x):
    return np.float64(x).tobytes()


def test_dp_on_the_references_own_pred(golden_dir):
    cases = _dp_cases(golden_dir)
    assert sum(1 for c in cases if not c[5]) >= 2 and sum(1 for c in cases if c[5]) >= 4
    single = []
    for name, tokens, pred, dur_ref, cost, unique in cases:
        T, N = pred.shape[0], tokens.shape[0]
        dur, c = A.align_durations(torch.from_numpy(pred).to(DEV)[None], torch.from_numpy(tokens)[None], [T], [N])
        dur, c = dur[0].cpu().numpy(), float(c[0])
        single.append(dur)
        assert _bits(c) == _bits(cost), (name, c, cost)          # bit-equal to the fp64 DP / scipy's Dijkstra distance, every row
        assert int(dur.sum()) == T, name
        pc = R.path_cost(dur, tokens, pred)
        assert abs(pc - cost) <= (T + N) * 2.0 ** -53 * cost, (name, pc, cost)
        assert np.array_equal(dur, R.dp_durations(tokens, pred)), name  # the documented tie rule: tied and tie-free rows alike
        if unique:
            assert np.array_equal(dur, dur_ref), (name, dur, dur_ref)     # exactly the reference's
        assert np.array_equal(A.extract_durations_with_dijkstra(tokens, pred), dur), name  # the numpy drop-in
    # all cases packed into one ragged call (pred zero-padded to the longest T, the widest V) equal the one-at-a-time calls
    B, T, N, V = len(cases), max(c[2].shape[0] for c in cases), max(c[1].shape[0] for c in cases), max(c[2].shape[1] for c in cases)
    pred = np.zeros((B, T, V), np.float32)
    tokens = np.zeros((B, N), np.int64)
    for b, (_, tk, p, _, _, _) in enumerate(cases):
        pred[b, :p.shape[0], :p.shape[1]] = p
        tokens[b, :tk.shape[0]] = tk
    dur, c = A.align_durations(torch.from_numpy(pred).to(DEV), torch.from_numpy(tokens), [x[2].shape[0] for x in cases], [x[1].shape[0] for x in cases])
    dur, c = dur.cpu().numpy(), c.cpu().numpy()
    for b, (name, tk, _, _, cost, _) in enumerate(cases):
        assert np.array_equal(dur[b, :tk.shape[0]], single[b]) and not dur[b, tk.shape[0]:].any(), name
        assert _bits(c[b]) == _bits(cost), name


@pytest.mark.parametrize("name", ["aligner_small", "aligner_full"])
def test_end_to_end_align(golden_dir, name):
    z, m = R.load_golden(golden_dir, name)
    model = _model(golden_dir, name)
    mel_len, tokens_len = z["mel_len"].tolist(), z["tokens_len"].tolist()
    dur, cost, pred = model.align(torch.from_numpy(z["mel"]).to(DEV), mel_len, torch.from_numpy(z["tokens"]).to(DEV), tokens_len)
    dur, pred_h = dur.cpu().numpy(), pred.cpu().numpy()
    held, left_out = [], []
    for b, (T, N) in enumerate(zip(mel_len, tokens_len)):
        want = R.dp_durations(z["tokens"][b, :N], pred_h[b, :T])  # the DP on the device's OWN pred: exact, every row
        assert np.array_equal(dur[b, :N], want) and not dur[b, N:].any() and int(dur[b].sum()) == T, b
        if m["unique"][b] and m["stable"][b]:
            assert np.array_equal(dur[b, :N], z["durations"][b, :N]), (b, dur[b, :N], z["durations"][b, :N])
            held.append(b)
        else:
            left_out.append(b)
    print(f"ALIGNE2E {name}: rows held to the reference's durations {held}, left out (tied or unstable) {left_out}")
    assert held, "no row of the fixture is both unique and stable"


def test_determinism(golden_dir):
    z, m = R.load_golden(golden_dir, "aligner_small")
    model = _model(golden_dir, "aligner_small")
    args = (torch.from_numpy(z["mel"]).to(DEV), z["mel_len"].tolist(), torch.from_numpy(z["tokens"]).to(DEV), z["tokens_len"].tolist())
    a, b = model.align(*args), model.align(*args)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert torch.equal(model(args[0]), model(args[0]))
    assert model.get_step() >= 5  # step counts forwards, in eval too


def test_refusals(golden_dir):
    """No fault is produced on purpose: every case is refused before a kernel could read through the bad value."""
    z, m = R.load_golden(golden_dir, "aligner_small")
    model = _model(golden_dir, "aligner_small")
    V = m["num_symbols"]
    pred = torch.full((1, 4, V), 1.0 / V, device=DEV)
    with pytest.raises(_lib.ParrotHipError) as e:      # N over the limit
        A.align_durations(pred, torch.ones((1, A.MAX_TOKENS + 1), dtype=torch.int64), [4], [3])
    assert e.value.code == -5
    lib = _lib.lib()
    assert lib.parrot_align_workspace_bytes(1, A.MAX_FRAMES + 1, 4) == 0 and lib.parrot_align_workspace_bytes(1, 4, A.MAX_TOKENS + 1) == 0
    one = torch.zeros(8, device=DEV)
    p = lambda t: A.dptr(t)  # noqa: E731
    assert lib.parrot_align_durations(p(one), p(one), p(one), p(one), 1, A.MAX_FRAMES + 1, V, 4, p(one), p(one), p(one), 8, None) == -5  # T over the limit
    assert lib.parrot_aligner_workspace_bytes(model._current_handle(torch.device(DEV)), 1, A.MAX_FRAMES + 1) == 0
    bad = A.Aligner(16, V, 24, 32).to(DEV)              # lstm_dim = 24
    with pytest.raises(_lib.ParrotHipError) as e:
        bad(torch.zeros((1, 8, 16), device=DEV))
    assert e.value.code == -5
    with pytest.raises(_lib.ParrotHipError) as e:      # the operating-point precisions are not offered
        A.Aligner(16, V, 32, 32, precision="bf16").to(DEV)(torch.zeros((1, 8, 16), device=DEV))
    assert e.value.code == -5
    tokens = torch.tensor([[1, 2, V, 3]])               # a token == V: the new status, durations are not returned
    with pytest.raises(ValueError, match="token"):
        A.align_durations(pred, tokens, [4], [4])
    with pytest.raises(ValueError, match="token"):     # ... device-side lengths out of range likewise, nothing read through them
        A.align_durations(pred, torch.tensor([[1, 2, 3, 4]]), torch.tensor([9], device=DEV), torch.tensor([4], device=DEV))
    with pytest.raises(ValueError, match="mel_len"):   # mel_len > T: a host error
        model.predict(torch.from_numpy(z["mel"]).to(DEV), [61, 41, 23])
    with pytest.raises(RuntimeError, match="GPU"):
        model(torch.from_numpy(z["mel"]))
    mel = torch.from_numpy(z["mel"]).to(DEV).clone()
    mel[1, 3, 2] = float("nan")                         # a non-finite logit: status 5
    with pytest.raises(_lib.ParrotHipError) as e:
        model.predict(mel, z["mel_len"].tolist())
    assert e.value.code == -6
    dur, _ = A.align_durations(pred, torch.tensor([[1, 2, 3, 4]]), [4], [4])  # and the library is fine afterwards
    assert int(dur.sum()) == 4


def test_softmax_in_place_and_device_side_status(golden_dir):
    """parrot_align_softmax may run in place; a device-side mel_len out of range sets status 9 in the softmax too (clamped, nothing
    read through it); a NaN probability of a real frame handed to the dynamic programme sets status 5: no durations come back."""
    z, m = R.load_golden(golden_dir, "aligner_small")
    model = _model(golden_dir, "aligner_small")
    mel = torch.from_numpy(z["mel"]).to(DEV)
    lens = z["mel_len"].tolist()
    logits = model(mel)
    pred = model.softmax(logits, lens)
    B, T, V = logits.shape
    ml = torch.tensor(lens, dtype=torch.int32, device=DEV)
    buf = logits.clone()
    _lib.check(_lib.lib().parrot_align_softmax(model._current_handle(torch.device(DEV)), A.dptr(buf), A.dptr(ml), B, T, A.dptr(buf), A.stream_ptr(torch.device(DEV))))
    assert torch.equal(buf, pred)
    for bad_len in ([T + 1, 41, 23], [60, 0, 23]):
        with pytest.raises(ValueError, match="mel_len"):
            model.predict(mel, torch.tensor(bad_len, device=DEV))
    assert torch.equal(model.predict(mel, ml), pred)       # the flag was cleared
    tokens = torch.from_numpy(z["tokens"])
    tl = z["tokens_len"].tolist()
    dur, cost = A.align_durations(pred, tokens, lens, tl)
    for val in (float("nan"), float("inf")):
        p = pred.clone()
        p[1, 40, int(tokens[1, 3])] = val                   # the last real frame of row 1, a column the row's tokens gather
        with pytest.raises(FloatingPointError, match="pred"):
            A.align_durations(p, tokens, lens, tl)
    p = pred.clone()
    p[1, 41:] = float("nan")                                # beyond mel_len: never read
    d2, c2 = A.align_durations(p, tokens, lens, tl)
    assert torch.equal(d2, dur) and torch.equal(c2, cost)


def _corpus(tmp_path, method="dijkstra"):
    cfg = synth.small_aligner_config(str(tmp_path / "data"))
    cfg["durations"]["method"] = method
    symbols = [chr(ord("a") + i) for i in range(20)]
    V = len(symbols) + 1
    data = tmp_path / "data"
    for d in ("mels", "tokens", "checkpoints"):
        (data / d).mkdir(parents=True, exist_ok=True)
    rng = np.random.Generator(np.random.PCG64(5))
    lens = [(37, 9), (52, 14), (20, 25), (45, 6), (31, 8)]
    dataset = []
    for i, (T, N) in enumerate(lens):
        item = f"utt{i:02d}"
        np.save(data / "mels" / f"{item}.npy", synth.synth_aligner_mel(1, T, 16, seed=20 + i)[0].numpy(), allow_pickle=False)
        np.save(data / "tokens" / f"{item}.npy", rng.integers(1, V, size=N), allow_pickle=False)
        dataset.append({"item_id": item, "mel_len": T, "tokens_len": N})
    with open(data / "dataset.pkl", "wb") as f:
        pickle.dump(dataset, f)
    with open(data / "symbols.pkl", "wb") as f:
        pickle.dump(symbols, f)
    sd = synth.synth_aligner_state_dict(cfg, V, seed=3, gain=14.0)
    torch.save({"config": cfg, "symbols": symbols, "model": sd}, data / "checkpoints" / "latest_model.pt")
    import yaml
    with open(tmp_path / "config.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    return cfg, dataset, sd, V, data


def test_cli_end_to_end(tmp_path, capsys):
    cfg, dataset, sd, V, data = _corpus(tmp_path)
    CLI.main(["--config", str(tmp_path / "config.yaml"), "--target", "out", "--batch_size", "2"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["n_items"] == 5 and line["n_written"] == 5 and line["n_failed"] == 0 and line["n_batches"] == 3
    assert sorted(os.listdir(data / "out")) == ["durations", "predictions"]   # the reference's layout
    model = A.Aligner(16, V, 32, 32)
    model.load_state_dict(sd)
    model = model.eval().to(DEV)
    for idx in ([0, 1], [2, 3], [4]):  # the same batches, directly
        items = [dataset[i] for i in idx]
        mel_len, tokens_len = [it["mel_len"] for it in items], [it["tokens_len"] for it in items]
        mel = torch.zeros((len(idx), max(mel_len), 16))
        tokens = torch.zeros((len(idx), max(tokens_len)), dtype=torch.int64)
        for b, it in enumerate(items):
            mel[b, :mel_len[b]] = torch.from_numpy(np.load(data / "mels" / f"{it['item_id']}.npy"))
            tokens[b, :tokens_len[b]] = torch.from_numpy(np.load(data / "tokens" / f"{it['item_id']}.npy"))
        dur, _, pred = model.align(mel.to(DEV), mel_len, tokens.to(DEV), tokens_len)
        for b, it in enumerate(items):
            p = np.load(data / "out" / "predictions" / f"{it['item_id']}.npy")
            d = np.load(data / "out" / "durations" / f"{it['item_id']}.npy")
            assert p.dtype == np.float32 and p.shape == (mel_len[b], V) and np.array_equal(p, pred[b, :mel_len[b]].cpu().numpy())
            assert d.dtype == np.int32 and d.shape == (tokens_len[b],) and np.array_equal(d, dur[b, :tokens_len[b]].cpu().numpy())
            assert int(d.sum()) == mel_len[b]


def test_cli_refuses_beam(tmp_path):
    _corpus(tmp_path, method="beam")
    r = subprocess.run([sys.executable, "-m", "parrot_tts_amd.cli.align_durations", "--config", str(tmp_path / "config.yaml")], cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode != 0 and "beam" in r.stderr


def test_whole_file_under_poison():
    """This file once more in a child process under PARROT_POISON_WS=nan: a kernel reading a byte nobody wrote would turn a parity
    ratio, a cost or a duration into NaN / garbage there."""
    if os.environ.get("PARROT_POISON_WS"):
        return  # (already a poisoned run: the tests above were it)
    env = dict(os.environ, PARROT_POISON_WS="nan")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", os.path.abspath(__file__), "-k", "not whole_file"], cwd=ROOT,
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
