"""CPU: the host side of the aligner's CTC validation loss -- the two exported symbols, their argument validation, and the
aligner_eval driver (parrot_tts_amd/cli/aligner_eval.py) end to end against a stub model on a tmp corpus, with the losses from
torch's CPU ``ctc_loss`` in fp64 (the operator of reference utils/aligner/trainer.py:60-63)."""
import ctypes
import json
import math
import os
import pickle
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from parrot_tts_amd import synth  # noqa: E402
from parrot_tts_amd.cli import aligner_eval as CLI  # noqa: E402

V = 21


def test_ctc_symbols_are_exported_and_the_header_is_c99(tmp_path):
    from parrot_tts_amd import _lib, build
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "parrot_hip.h")).read()
    for n in ("parrot_ctc_workspace_bytes", "parrot_ctc_loss"):
        assert hasattr(raw, n) and n in _lib.SIGNATURES, n
        assert re.search(r"\b" + n + r"\s*\(", hdr), n
    assert "#define PARROT_ABI_VERSION 7" in hdr and "trainer.py:60-63" in hdr
    lib = _lib.lib()
    # the limits of the module: beyond them the workspace query answers 0
    assert lib.parrot_ctc_workspace_bytes(1, 10, 2049) == 0 and lib.parrot_ctc_workspace_bytes(1, 32769, 4) == 0
    assert lib.parrot_ctc_workspace_bytes(0, 10, 4) == 0
    assert lib.parrot_ctc_workspace_bytes(2, 10, 7) == 256 + 256  # the status word, then 20 fp64 rounded up to 256 bytes
    assert lib.parrot_ctc_workspace_bytes(1, 32768, 2048) == 256 + 32768 * 8
    # argument validation happens before any HIP call
    assert lib.parrot_ctc_loss(None, None, None, None, 1, 1, 1, 1, None, None, None, 0, None) == -1
    assert b"null" in lib.parrot_last_error()
    gcc = shutil.which("gcc")
    assert gcc is not None
    src = tmp_path / "hdr.c"
    src.write_text('#include "parrot_hip.h"\nsize_t (*ws)(int32_t, int32_t, int32_t) = parrot_ctc_workspace_bytes;\n'
                   "int (*fn)(const float*, const int64_t*, const int32_t*, const int32_t*, int32_t, int32_t, int32_t, int32_t, double*, float*, void*,\n"
                   "          size_t, void*) = parrot_ctc_loss;\n")
    subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


class _StubModel:
    """The surface the driver uses, on the CPU: the logits are a fixed projection of the mel."""

    def __init__(self):
        self.batches, self.precision_in_use = [], "stub"

    def get_step(self):
        return 7

    def __call__(self, mel):
        self.batches.append(tuple(mel.shape))
        w = torch.linspace(-1, 1, mel.shape[2] * V).reshape(mel.shape[2], V)
        return torch.sin(mel @ w * 3) * 4


def _torch_loss(logits, tokens, mel_len, tokens_len):
    """nll (B) fp64 by the reference's own operator; a token outside the table is refused, as the device refuses it."""
    for b, n in enumerate(tokens_len):
        if int(tokens[b, :n].max()) >= V or int(tokens[b, :n].min()) < 0:
            raise ValueError("a token outside [0, V)")
    return F.ctc_loss(logits.double().transpose(0, 1).log_softmax(2), tokens, torch.tensor(mel_len), torch.tensor(tokens_len), reduction="none")


LENS = [(37, 9), (52, 14), (20, 25), (45, 6), (31, 8), (28, 5)]  # utt02 is infeasible: fewer frames than tokens


def _corpus(tmp_path, ckpt_symbols=None):
    import yaml
    cfg = synth.small_aligner_config(str(tmp_path / "data"))
    symbols = list("abcdefghijklmnopqrst")
    data = tmp_path / "data"
    for d in ("mels", "tokens", "checkpoints"):
        (data / d).mkdir(parents=True, exist_ok=True)
    rng = np.random.Generator(np.random.PCG64(5))
    dataset, tokens_of = [], {}
    for i, (T, N) in enumerate(LENS):
        item = f"utt{i:02d}"
        np.save(data / "mels" / f"{item}.npy", synth.synth_aligner_mel(1, T + 3, 16, seed=20 + i)[0].numpy())  # (stored longer than mel_len)
        tokens = rng.integers(1, V, size=N)
        if i == 1:
            tokens[2] = V  # utt01 holds a token outside the symbol table: reported and skipped
        if i != 3:
            np.save(data / "tokens" / f"{item}.npy", tokens)  # utt03 has no token file: reported and skipped
        tokens_of[item] = tokens
        dataset.append({"item_id": item, "mel_len": T, "tokens_len": N})
    with open(data / "dataset.pkl", "wb") as f:
        pickle.dump(dataset, f)
    with open(data / "symbols.pkl", "wb") as f:
        pickle.dump(symbols, f)
    torch.save({"config": cfg, "symbols": ckpt_symbols or symbols, "model": {}}, data / "checkpoints" / "latest_model.pt")
    with open(tmp_path / "config.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    return data, tokens_of


def test_driver_end_to_end_against_a_stub_model(tmp_path, capsys):
    args = CLI.parse_args([])
    assert (args.config, args.model, args.batch_size, args.per_item) == ("utils/aligner/aligner_train_config.yaml", None, 8, False)
    data, tokens_of = _corpus(tmp_path)
    stub = _StubModel()
    argv = ["--config", str(tmp_path / "config.yaml"), "--batch_size", "2"]
    out = CLI.run(CLI.parse_args(argv + ["--per_item"]), model_loader=lambda ckpt, dev: stub, loss_fn=_torch_loss, device="cpu")
    err = capsys.readouterr().err
    assert set(out) == {"ctc_loss", "n_items", "n_infeasible", "n_failed", "n_batches", "step", "precision", "items"}
    assert out["n_items"] == 6 and out["n_batches"] == 3 and out["n_failed"] == 2 and out["n_infeasible"] == 1 and out["step"] == 7
    assert "utt03" in err and "utt01" in err  # a failing item is reported and skipped
    # dataset order, each batch padded to ITS OWN longest mel (only the loadable rows ride in it)
    assert stub.batches == [(2, 52, 16), (1, 20, 16), (2, 31, 16)]
    # the same batches, directly
    want = {}
    for idx in ([0, 1], [2], [4, 5]):
        T = max(LENS[i][0] for i in idx)
        mel = torch.zeros((len(idx), T, 16))
        for b, i in enumerate(idx):
            mel[b, :LENS[i][0]] = torch.from_numpy(np.load(data / "mels" / f"utt{i:02d}.npy"))[:LENS[i][0]]
        logits = _StubModel()(mel)
        for b, i in enumerate(idx):
            if i == 1:
                continue
            tk = torch.from_numpy(tokens_of[f"utt{i:02d}"])[None]
            want[f"utt{i:02d}"] = float(_torch_loss(logits[b:b + 1], tk, [LENS[i][0]], [LENS[i][1]])[0]) / LENS[i][1]
    assert sorted(out["items"]) == sorted(want) == ["utt00", "utt02", "utt04", "utt05"]
    assert out["items"]["utt02"] == math.inf == want["utt02"]  # counted, and left out of the mean
    for k in want:
        assert out["items"][k] == pytest.approx(want[k], rel=1e-12), k
    finite = [want[k] for k in ("utt00", "utt04", "utt05")]
    assert out["ctc_loss"] == pytest.approx(sum(finite) / 3, rel=1e-12)
    line = json.loads(json.dumps(out))
    assert line["items"]["utt02"] == math.inf
    out2 = CLI.run(CLI.parse_args(argv), model_loader=lambda ckpt, dev: _StubModel(), loss_fn=_torch_loss, device="cpu")
    assert "items" not in out2 and out2["ctc_loss"] == out["ctc_loss"]


def test_driver_checks_symbols(tmp_path):
    _corpus(tmp_path, ckpt_symbols=list("abc"))
    with pytest.raises(AssertionError, match="Symbols from dataset do not match"):
        CLI.run(CLI.parse_args(["--config", str(tmp_path / "config.yaml")]), model_loader=lambda c, d: _StubModel(), loss_fn=_torch_loss, device="cpu")
