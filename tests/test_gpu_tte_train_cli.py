"""GPU: ``python -m parrot_tts_amd.cli.tte_train`` -- four optimiser steps on a synthetic dataset write a checkpoint that
``cli.tte_eval`` scores."""
import json
import os
import pickle

import pytest
import torch
import yaml

from parrot_tts_amd import checkpoint, data, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dataset(tmp_path):
    root = tmp_path / "tte"
    root.mkdir()
    (root / "speakers.json").write_text(json.dumps({"bho_f": 0, "en_m": 1}))
    symbols = ["a", " ", "b", "c", "d"]
    with open(root / "symbols.pkl", "wb") as f:
        pickle.dump(symbols, f)
    cfg = synth.small_tte_config(str(root))
    cfg["path"]["alignment_path"] = str(root)
    cfg["path"]["wav_path"] = str(tmp_path / "audio")
    cfg["optimizer"] = {"init_lr": 1e-3, "weight_decay": 0.01}
    cfg["train"] = {"batch_size": 2, "grad_acc_steps": 2, "grad_clip": 1.0, "warmup_steps": 2, "total_steps": 4, "val_every": 2, "save_every": 4,
                    "log_every": 1}
    recs = [{"audio": "/x/bho_f_001.wav", "speaker": "bho_f", "characters": "a sil b c", "hubert": "1 2 3 4 5 6", "duration": "1 2 0 3"},
            {"audio": "/x/en_m_002.wav", "speaker": "en_m", "characters": "d a", "hubert": "7 8 9", "duration": "1 2"},
            {"audio": "/x/bho_f_003.wav", "speaker": "bho_f", "characters": "c c sil a b d", "hubert": "3 3 4 99 0", "duration": "1 1 0 1 1 1"}]
    (root / "train.txt").write_text("".join(data.format_dict_line(r) for r in recs))
    (root / "val.txt").write_text("".join(data.format_dict_line(r) for r in recs[:2]))
    ycfg = tmp_path / "cfg.yaml"
    ycfg.write_text(yaml.safe_dump(cfg))
    return root, cfg, ycfg


def test_four_steps_write_a_checkpoint_that_tte_eval_scores(tmp_path, capsys):
    from parrot_tts_amd.cli import tte_eval, tte_train
    root, cfg, ycfg = _dataset(tmp_path)
    res = tte_train.main(["--config", str(ycfg), "--device", DEV])
    lines = [json.loads(x) for x in capsys.readouterr().out.strip().splitlines()]
    assert res["steps"] == 4 and [r["step"] for r in lines] == [1, 2, 3, 4] and lines == res["records"]
    # the schedule: warm-up 0, 1/2, then the cosine from 1 (train.py:42-50); the learning rate logged is the one the step used
    assert [r["lr"] for r in lines] == pytest.approx([0.0, 5e-4, 1e-3, 5e-4])
    assert all({"train_total_loss", "train_code_loss", "train_dur_loss"} <= set(r) for r in lines)
    assert "val_total_loss" in lines[1] and "val_total_loss" in lines[3] and "val_total_loss" not in lines[0]
    assert lines[3]["val_total_loss"] < lines[1]["val_total_loss"]
    ck = res["checkpoint"]
    assert ck == lines[3]["checkpoint"] == os.path.join(str(root), "ckpt", "parrot_model-step=4.ckpt") and os.path.isfile(ck)
    ev = tte_eval.main(["--config", str(ycfg), "--checkpoint_pth", ck, "--device", DEV, "--batch_size", "2"])
    assert ev["n_utterances"] == 2 and torch.isfinite(torch.tensor(ev["val_total_loss"]))
    # tte_eval runs the inference Parrot on the trained weights; the driver's last validation ran TrainableParrot in eval mode on them
    assert ev["val_total_loss"] == pytest.approx(lines[3]["val_total_loss"], abs=2e-4)
    assert set(checkpoint.LitParrot.load_from_checkpoint(ck).state_dict()) == set(torch.load(ck, weights_only=True)["state_dict"])
