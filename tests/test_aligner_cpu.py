"""CPU: the host side of the aligner (parrot_tts_amd/aligner.py, cli/align_durations.py) and the yardsticks the GPU tests use -- the
restatement tests/aligner_ref.py against the reference's own outputs (tests/golden/aligner_*.npz, align_dp.npz, written by
tools/make_aligner_goldens.py), the state-dict surface, the exported symbols, and the driver's argument / config / dataset handling
against a stub model."""
import ctypes
import json
import os
import pickle
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import aligner_ref as R  # noqa: E402
from parrot_tts_amd import aligner as A  # noqa: E402
from parrot_tts_amd import synth  # noqa: E402
from parrot_tts_amd.cli import align_durations as CLI  # noqa: E402


def _sd(m):
    cfg = synth.default_aligner_config()
    cfg["audio"]["n_mels"] = m["n_mels"]
    cfg["model"].update(lstm_dim=m["lstm_dim"], conv_dim=m["conv_dim"])
    sd = synth.synth_aligner_state_dict(cfg, m["num_symbols"], seed=m["seed"], gain=m["gain"])
    assert synth.state_digest(sd) == m["digest"]  # the weights regenerate bit for bit from the seed
    return sd


@pytest.mark.parametrize("name", R.MODEL_GOLDENS)
def test_restatement_against_the_fixtures(golden_dir, name):
    """tests/aligner_ref.py in fp64 equals the reference run in fp64 (logits64, stages) to 1e-12; the stored d_ref is the distance
    of the reference's fp32 result from it; the fp32 restatement is within 4 x d_ref itself (it is another fp32 summation order)."""
    z, m = R.load_golden(golden_dir, name)
    sd = _sd(m)
    mel = torch.from_numpy(z["mel"])
    out64, st64 = R.aligner_forward(sd, mel.double())
    assert float((out64 - torch.from_numpy(z["logits64"])).abs().max()) <= 1e-12
    d_ref = float((torch.from_numpy(z["logits"]).double() - torch.from_numpy(z["logits64"])).abs().max())
    assert d_ref == m["d_ref"]["logits"] and 0 < d_ref < 1e-3
    assert 12 <= m["logit_max"] <= 23  # a peaky softmax
    for k in ("bn3", "lstm"):
        if k in z.files:
            got = st64[k][..., torch.from_numpy(z["lstm_channels"]).long()] if (k == "lstm" and "lstm_channels" in z.files) else st64[k]
            assert float((got - torch.from_numpy(z[k + "64"])).abs().max()) <= 1e-12
            assert float((torch.from_numpy(z[k]).double() - torch.from_numpy(z[k + "64"])).abs().max()) == m["d_ref"][k]
    if name != "aligner_full":  # (the full-size fp32 loop is the slow one; its fp64 run above is what the GPU is held to)
        out32, _ = R.aligner_forward(sd, mel)
        assert float((out32.double() - torch.from_numpy(z["logits64"])).abs().max()) <= 4 * d_ref
    if "pred" in z.files:
        pred = R.softmax_rows(torch.from_numpy(z["logits"]), z["mel_len"])
        assert torch.equal(pred, torch.from_numpy(z["pred"]))
        p64 = R.softmax_rows(torch.from_numpy(z["logits64"]), z["mel_len"])
        assert float((p64 - torch.from_numpy(z["pred64"])).abs().max()) <= 1e-15
        assert any(u and s for u, s in zip(m["unique"], m["stable"]))
    if "logits_alone" in z.files:  # the padding quirk is in the fixture: the row alone is another result
        b, n = m["alone_row"], int(z["mel_len"][m["alone_row"]])
        alone64, _ = R.aligner_forward(sd, mel[b:b + 1, :n].double())
        assert float((alone64[0] - torch.from_numpy(z["logits_alone64"])).abs().max()) <= 1e-12
        assert float(np.abs(z["logits"][b, :n] - z["logits_alone"]).max()) > 100 * d_ref


def _dp_cases(golden_dir):
    z, m = R.load_golden(golden_dir, R.DP_GOLDEN)
    cases = [(c, z[c + "_tokens"], z[c + "_pred"], z[c + "_durations"], float(z[c + "_cost"]), m["unique"][c], m["tied"][c]) for c in m["cases"]]
    for name in ("aligner_small", "aligner_full"):
        zz, mm = R.load_golden(golden_dir, name)
        for b in range(len(zz["mel_len"])):
            T, N = int(zz["mel_len"][b]), int(zz["tokens_len"][b])
            cases.append((f"{name}[{b}]", zz["tokens"][b, :N], zz["pred"][b, :T], zz["durations"][b, :N], float(zz["cost"][b]), mm["unique"][b], False))
    return cases


def test_dp_restatement_against_the_reference(golden_dir):
    """dp_durations == the reference's durations on every unique row; the cost is bit-equal to the stored one (scipy's Dijkstra
    distance, asserted by the generator) on every row; the tied cases are tied; path_cost of the reference's own durations is
    that cost: its path is as cheap, whichever it chose."""
    cases = _dp_cases(golden_dir)
    assert {c[0] for c in cases} >= {"t150n30", "t64n64", "t23n30", "t97n33_repeats", "t40n12_saturated", "t17n1"}
    for name, tokens, pred, dur_ref, cost, unique, tied in cases:
        dur, c, u = R.dp_durations(tokens, pred, with_info=True)
        assert np.float64(c).tobytes() == np.float64(cost).tobytes(), name
        assert u == unique and (not tied or not unique), name
        assert int(dur.sum()) == pred.shape[0] == int(dur_ref.sum()), name
        if unique:
            assert np.array_equal(dur, dur_ref), name
        for d in (dur, dur_ref):
            pc = R.path_cost(d, tokens, pred)
            assert abs(pc - cost) <= (pred.shape[0] + len(tokens)) * 2.0 ** -53 * cost, (name, pc, cost)
    by = {c[0]: c for c in cases}
    assert by["t23n30"][1].shape[0] > by["t23n30"][2].shape[0] and (by["t23n30"][3] == 0).any()  # N > T: tokens passed by right moves get 0
    assert by["t17n1"][3].tolist() == [17]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_lstm_steps_is_lstm_direction_from_a_zero_state(dtype):
    """``lstm_steps`` -- what tests/test_gpu_aligner_kernels.py holds the two LSTM step kernels to -- from a zero state with
    n_steps = T is ``lstm_direction`` / the "lstm" tap of ``aligner_forward`` EXACTLY, in both dtypes, once bias_hh is folded into
    the input projection as the library folds it (bias_hh = 0 here, so both add the same two numbers); with the fixture's own
    bias_hh, which ``lstm_direction`` adds to h W_hh^T first, the two agree to rounding.  A run stopped after n_steps and resumed
    from its state is the full run; frames no step owns stay zero."""
    m = dict(n_mels=24, lstm_dim=48, conv_dim=32, num_symbols=13)
    cfg = synth.default_aligner_config()
    cfg["audio"]["n_mels"] = m["n_mels"]
    cfg["model"].update(lstm_dim=m["lstm_dim"], conv_dim=m["conv_dim"])
    sd = synth.synth_aligner_state_dict(cfg, m["num_symbols"], seed=21, gain=2.0)
    mel = synth.synth_aligner_mel(3, 11, m["n_mels"], seed=22).to(dtype)
    H = m["lstm_dim"]

    def xproj_of(sd):
        bn3 = R.aligner_forward(sd, mel)[1]["bn3"]
        return torch.cat([bn3 @ sd["rnn.weight_ih_l0" + s].to(dtype).t() + sd["rnn.bias_ih_l0" + s].to(dtype) + sd["rnn.bias_hh_l0" + s].to(dtype)
                          for s in ("", "_reverse")], dim=-1)

    w_hh = torch.stack([sd["rnn.weight_hh_l0"], sd["rnn.weight_hh_l0_reverse"]])
    folded = dict(sd)
    for s in ("", "_reverse"):
        folded["rnn.bias_hh_l0" + s] = torch.zeros_like(sd["rnn.bias_hh_l0" + s])
    assert any(bool(sd["rnn.bias_ih_l0" + s].abs().max() > 0) for s in ("", "_reverse"))
    want = R.aligner_forward(folded, mel)[1]["lstm"]
    out, h_n, c_n, gates, c_all = R.lstm_steps(w_hh, xproj_of(folded), None, None, None, dtype)
    assert out.dtype == dtype and torch.equal(out, want)
    assert torch.equal(h_n[0], out[:, -1, :H]) and torch.equal(h_n[1], out[:, 0, H:])
    assert torch.equal(c_n[0], c_all[:, -1, :H]) and torch.equal(c_n[1], c_all[:, 0, H:])
    o_ = torch.cat([gates[..., 3 * H:4 * H], gates[..., 7 * H:]], dim=-1)
    assert torch.equal(out, o_ * torch.tanh(c_all))
    # the fixture's own bias_hh: another order of the same three-term sum
    want = R.aligner_forward(sd, mel)[1]["lstm"]
    full = R.lstm_steps(w_hh, xproj_of(sd), None, None, None, dtype)
    assert float((full[0] - want).abs().max()) <= (1e-12 if dtype == torch.float64 else 1e-5)
    # stopped after 4 steps and resumed: the forward direction continues on frames 4 .., the backward one on frames .. T - 5
    xp = xproj_of(sd)
    T = xp.shape[1]
    first = R.lstm_steps(w_hh, xp, None, None, 4, dtype)
    assert not first[0][:, 4:, :H].any() and not first[0][:, :T - 4, H:].any()
    assert torch.equal(first[0][:, :4, :H], full[0][:, :4, :H]) and torch.equal(first[0][:, T - 4:, H:], full[0][:, T - 4:, H:])
    rest = torch.cat([xp[:, 4:, :4 * H], xp[:, :T - 4, 4 * H:]], dim=-1)
    second = R.lstm_steps(w_hh, rest, first[1], first[2], None, dtype)
    assert torch.equal(second[0][..., :H], full[0][:, 4:, :H]) and torch.equal(second[0][..., H:], full[0][:, :T - 4, H:])
    assert torch.equal(second[1], full[1]) and torch.equal(second[2], full[2])
    pre = R.lstm_preactivations(w_hh, rest, first[1], dtype)
    assert torch.equal(torch.sigmoid(pre[0][:, :H]), second[3][:, 0, :H]) and torch.equal(torch.tanh(pre[1][:, 2 * H:3 * H]), second[3][:, -1, 6 * H:7 * H])


def _fast_dp_seeded_cases():
    """(name, tokens, pred): (1, 9), (9, 1), (40, 33) uniform (every cell tied), (50, 20) saturated (w exactly 0 or 1)."""
    rng = np.random.Generator(np.random.PCG64(31))
    V = 11
    soft = lambda T: torch.softmax(torch.from_numpy(rng.standard_normal((T, V)) * 3), -1).numpy().astype(np.float32)  # noqa: E731
    cases = [("t1n9", rng.integers(0, V, 9), soft(1)), ("t9n1", rng.integers(0, V, 1), soft(9)),
             ("t40n33_uniform", rng.integers(0, V, 33), np.full((40, V), 1.0 / V, np.float32))]
    sat = np.zeros((50, V), np.float32)
    sat[np.arange(50), rng.integers(0, V, 50)] = 1.0
    cases.append(("t50n20_saturated", rng.integers(0, V, 20), sat))
    return cases


def test_fast_dp_is_the_slow_dp(golden_dir):
    """``dp_durations_fast`` (the anti-diagonal sweep the GPU tests use at 2100 x 2048) gives ``dp_durations``' durations and its cost
    bit for bit: on every case of align_dp.npz, on single-frame and single-token grids, with every cell tied, and saturated."""
    z, m = R.load_golden(golden_dir, R.DP_GOLDEN)
    cases = [(c, z[c + "_tokens"], z[c + "_pred"]) for c in m["cases"]] + _fast_dp_seeded_cases()
    assert len(cases) >= 10
    for name, tokens, pred in cases:
        dur, cost, _ = R.dp_durations(tokens, pred, with_info=True)
        fdur, fcost = R.dp_durations_fast(tokens, pred)
        assert fdur.dtype == np.int32 and np.array_equal(fdur, dur), name
        assert np.float64(fcost).tobytes() == np.float64(cost).tobytes(), name
        assert int(fdur.sum()) == pred.shape[0], name
    w = R.path_weights(cases[-1][1], cases[-1][2])
    assert set(np.unique(w).tolist()) <= {0.0, 1.0}


def test_state_dict_round_trip_and_from_checkpoint():
    cfg = synth.small_aligner_config()
    symbols = list("abcdefghijklmnopqrst")
    sd = synth.synth_aligner_state_dict(cfg, len(symbols) + 1, seed=3)
    model = A.Aligner.from_checkpoint({"config": cfg, "symbols": symbols, "model": sd})
    assert (model.n_mels, model.num_symbols, model.lstm_dim, model.conv_dim) == (16, 21, 32, 32)
    got = model.state_dict()
    assert sorted(got) == sorted(sd) and all(torch.equal(got[k], sd[k]) and got[k].dtype == sd[k].dtype for k in sd)
    assert {"step", "convs.0.bnorm.num_batches_tracked", "convs.2.bnorm.running_var", "rnn.weight_hh_l0_reverse", "lin.bias"} <= set(got)
    assert model.get_step() == 1 and isinstance(model.get_step(), int)
    assert synth.state_digest(got) == synth.state_digest(sd)
    assert synth.state_digest(synth.synth_aligner_state_dict(cfg, 21, seed=4)) != synth.state_digest(sd)
    missing = {k: v for k, v in sd.items() if k != "rnn.bias_hh_l0"}
    with pytest.raises(RuntimeError, match="Missing key"):
        A.Aligner(16, 21, 32, 32).load_state_dict(missing)
    with pytest.raises(RuntimeError, match="Unexpected key"):
        A.Aligner(16, 21, 32, 32).load_state_dict(dict(sd, extra=torch.zeros(1)))
    with pytest.raises(RuntimeError, match="size mismatch"):
        A.Aligner(16, 22, 32, 32).load_state_dict(sd)
    with pytest.raises(RuntimeError, match="GPU"):  # no CPU path
        model(torch.zeros(1, 8, 16))
    full = synth.default_aligner_config()
    assert (full["audio"]["n_mels"], full["model"]["lstm_dim"], full["model"]["conv_dim"]) == (80, 512, 512)


def test_new_symbols_are_exported_and_the_header_is_c99(tmp_path):
    from parrot_tts_amd import _lib, build
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    names = ["parrot_aligner_create", "parrot_aligner_create_ex", "parrot_aligner_destroy", "parrot_aligner_precision",
             "parrot_aligner_workspace_bytes", "parrot_aligner_forward", "parrot_aligner_check", "parrot_aligner_status_async",
             "parrot_align_softmax", "parrot_align_workspace_bytes", "parrot_align_durations", "parrot_aligner_debug_stages"]
    hdr = open(os.path.join(ROOT, "include", "parrot_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "parrot_hip_debug.h")).read()
    for n in names:
        assert hasattr(raw, n) and n in _lib.SIGNATURES, n
        assert re.search(r"\b" + n + r"\s*\(", dbg if "debug" in n else hdr), n
    assert "#define PARROT_ABI_VERSION 7" in hdr
    assert ctypes.sizeof(_lib.AlignerCfg) == 5 * 4 and ctypes.sizeof(_lib.AlignerWeights) == (5 * 3 + 4 * 2 + 2) * ctypes.sizeof(ctypes.c_void_p)
    # argument validation happens before any HIP call
    lib = _lib.lib()
    assert lib.parrot_align_workspace_bytes(1, 10, 2049) == 0 and lib.parrot_align_workspace_bytes(2, 10, 7) == 256 + 256
    assert lib.parrot_align_durations(None, None, None, None, 1, 1, 1, 1, None, None, None, 0, None) == -1
    gcc = shutil.which("gcc")
    assert gcc is not None
    src = tmp_path / "hdr.c"
    src.write_text('#include "parrot_hip.h"\n#include "parrot_hip_debug.h"\nparrot_aligner_cfg c; parrot_aligner_weights w;\n')
    subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


class _StubModel:
    """The surface the driver uses, on the CPU: pred is a softmax of a fixed projection of the mel; durations by tests/aligner_ref.py."""

    def __init__(self, V):
        self.V, self.batches, self.precision_in_use = V, [], "stub"

    def get_step(self):
        return 7

    def predict(self, mel, mel_len):
        self.batches.append((tuple(mel.shape), list(mel_len)))
        w = torch.linspace(-1, 1, mel.shape[2] * self.V).reshape(mel.shape[2], self.V)
        return R.softmax_rows(mel @ w * 3, mel_len)

    def durations(self, pred, tokens, mel_len, tokens_len):
        out = torch.zeros(tokens.shape, dtype=torch.int32)
        for b, (T, N) in enumerate(zip(mel_len, tokens_len)):
            if int(tokens[b, :N].max()) >= self.V:
                raise ValueError("a token outside [0, V)")
            out[b, :N] = torch.from_numpy(R.dp_durations(tokens[b, :N].numpy(), pred[b, :T].numpy()))
        return out


def _corpus(tmp_path, method="dijkstra", bad_token_item=None, ckpt_symbols=None):
    import yaml
    cfg = synth.small_aligner_config(str(tmp_path / "data"))
    cfg["durations"]["method"] = method
    symbols = list("abcdefghijklmnopqrst")
    data = tmp_path / "data"
    for d in ("mels", "tokens", "checkpoints"):
        (data / d).mkdir(parents=True, exist_ok=True)
    rng = np.random.Generator(np.random.PCG64(5))
    dataset = []
    for i, (T, N) in enumerate([(37, 9), (52, 14), (20, 25), (45, 6), (31, 8)]):
        item = f"utt{i:02d}"
        np.save(data / "mels" / f"{item}.npy", synth.synth_aligner_mel(1, T + 3, 16, seed=20 + i)[0].numpy())  # (stored longer than mel_len)
        tokens = rng.integers(1, 21, size=N)
        if item == bad_token_item:
            tokens[2] = 21
        if i != 3:
            np.save(data / "tokens" / f"{item}.npy", tokens)  # utt03 has no token file: reported and skipped
        dataset.append({"item_id": item, "mel_len": T, "tokens_len": N})
    pickle.dump(dataset, open(data / "dataset.pkl", "wb"))
    pickle.dump(symbols, open(data / "symbols.pkl", "wb"))
    torch.save({"config": cfg, "symbols": ckpt_symbols or symbols, "model": {}}, data / "checkpoints" / "latest_model.pt")
    yaml.safe_dump(cfg, open(tmp_path / "config.yaml", "w"))
    return data


def test_cli_arguments_config_and_dataset_handling(tmp_path, capsys):
    args = CLI.parse_args([])
    assert (args.config, args.model, args.target, args.batch_size) == ("utils/aligner/aligner_train_config.yaml", None, "outputs", 8)
    args = CLI.parse_args(["-c", "x.yaml", "-m", "ckpt.pt", "-t", "out", "-b", "3", "-w", "5"])
    assert (args.config, args.model, args.target, args.batch_size) == ("x.yaml", "ckpt.pt", "out", 3)
    assert CLI.plan_batches(5, 2) == [[0, 1], [2, 3], [4]] and CLI.plan_batches(0, 4) == []
    data = _corpus(tmp_path, bad_token_item="utt01")
    stub = _StubModel(21)
    out = CLI.run(CLI.parse_args(["--config", str(tmp_path / "config.yaml"), "--target", "out", "--batch_size", "2"]),
                  model_loader=lambda ckpt, dev: stub, device="cpu")
    err = capsys.readouterr().err
    assert out["n_items"] == 5 and out["n_batches"] == 3 and out["n_written"] == 3 and out["n_failed"] == 2 and out["step"] == 7
    assert "utt03" in err and "utt01" in err  # a failing item is reported and skipped
    # dataset order, each batch padded to ITS OWN longest mel (only the loadable rows ride in it)
    assert stub.batches == [((2, 52, 16), [37, 52]), ((1, 20, 16), [20]), ((1, 31, 16), [31])]
    assert sorted(os.listdir(data / "out" / "durations")) == ["utt00.npy", "utt02.npy", "utt04.npy"]
    assert sorted(os.listdir(data / "out" / "predictions")) == ["utt00.npy", "utt01.npy", "utt02.npy", "utt04.npy"]
    d, p = np.load(data / "out" / "durations" / "utt02.npy"), np.load(data / "out" / "predictions" / "utt02.npy")
    assert d.dtype == np.int32 and d.shape == (25,) and int(d.sum()) == 20 and p.dtype == np.float32 and p.shape == (20, 21)
    json.dumps(out)


def test_cli_checks_symbols_and_refuses_beam(tmp_path):
    _corpus(tmp_path, ckpt_symbols=list("abc"))
    with pytest.raises(AssertionError, match="Symbols from dataset do not match"):
        CLI.run(CLI.parse_args(["--config", str(tmp_path / "config.yaml")]), model_loader=lambda c, d: _StubModel(21), device="cpu")
    _corpus(tmp_path, method="beam")
    with pytest.raises(SystemExit) as e:
        CLI.run(CLI.parse_args(["--config", str(tmp_path / "config.yaml")]), model_loader=lambda c, d: _StubModel(21), device="cpu")
    assert "beam" in str(e.value) and e.value.code != 0


def test_dropin_reexports():
    sys.path.insert(0, os.path.join(ROOT, "parrot_tts_amd", "dropin"))
    try:
        for k in [k for k in sys.modules if k == "utils" or k.startswith("utils.")]:
            del sys.modules[k]
        from utils.aligner.duration_extraction import extract_durations_with_dijkstra
        from utils.aligner.model import Aligner
        assert Aligner is A.Aligner and extract_durations_with_dijkstra is A.extract_durations_with_dijkstra
    finally:
        sys.path.remove(os.path.join(ROOT, "parrot_tts_amd", "dropin"))
        for k in [k for k in sys.modules if k == "utils" or k.startswith("utils.")]:
            del sys.modules[k]
