"""CPU: the host side of cli.voc_train -- checkpoint names and keys, the epoch / learning-rate arithmetic, the batch order with the
dropped last batch, the resume bookkeeping from a hand-made g_ / do_ pair whose optimiser entries torch.optim.AdamW wrote, the
speaker-table rule, and the refusal to run without a GPU.  (tests/test_voc_train_cpu.py is the generator's training module.)"""
import json
import os

import pytest
import torch

from parrot_tts_amd import data
from parrot_tts_amd.cli import voc_train
from parrot_tts_amd.optim import FusedAdamW


def test_checkpoint_names_and_resume_scan(tmp_path):
    g, do = voc_train.checkpoint_pair(str(tmp_path), 2)
    assert os.path.basename(g) == "g_00000002" and os.path.basename(do) == "do_00000002"
    assert voc_train.checkpoint_pair("d", 12345678) == (os.path.join("d", "g_12345678"), os.path.join("d", "do_12345678"))
    assert voc_train.find_resume(str(tmp_path / "absent")) is None and voc_train.find_resume(str(tmp_path)) is None
    torch.save({"generator": {}}, g)
    assert voc_train.find_resume(str(tmp_path)) is None  # a g_ alone is no resume (train.py:59)
    for step in (2, 10):
        torch.save({"steps": step, "epoch": 1}, voc_train.checkpoint_pair(str(tmp_path), step)[1])
    torch.save({"generator": {}}, voc_train.checkpoint_pair(str(tmp_path), 10)[0])
    (tmp_path / "g_final").write_bytes(b"")  # not eight characters: the training scripts' glob passes it over
    assert voc_train.find_resume(str(tmp_path)) == voc_train.checkpoint_pair(str(tmp_path), 10)


def test_epoch_and_learning_rate_arithmetic():
    lr0, decay = 2e-4, 0.999
    p = torch.nn.Parameter(torch.zeros(3))
    opt = FusedAdamW([p], lr0, betas=[0.8, 0.99])
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=decay, last_epoch=-1)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for epoch in range(5):
            assert opt.param_groups[0]["lr"] == pytest.approx(voc_train.lr_at(lr0, decay, epoch), rel=1e-12)
            sched.step()
    assert voc_train.lr_at(lr0, decay, 0) == lr0 and voc_train.lr_at(lr0, decay, 3) == lr0 * decay ** 3


def test_batch_order_and_dropped_last_batch():
    assert voc_train.epoch_batches(3, 2) == [[0, 1]]
    assert voc_train.epoch_batches(7, 3) == [[0, 1, 2], [3, 4, 5]]
    assert voc_train.epoch_batches(4, 2) == [[0, 1], [2, 3]]
    assert voc_train.epoch_batches(1, 2) == [] and voc_train.epoch_batches(0, 16) == []
    import numpy as np
    items = [({"code": np.arange(3) + k, "spkr": np.asarray([k])}, torch.full((6,), float(k)), f"f{k}", None) for k in range(2)]
    x, y = voc_train.collate(items, "cpu")
    assert x["code"].tolist() == [[0, 1, 2], [1, 2, 3]] and x["code"].dtype == torch.int64 and x["spkr"].tolist() == [[0], [1]]
    assert tuple(y.shape) == (2, 1, 6) and y.dtype == torch.float32 and y[1, 0, 0] == 1.0


def test_resume_bookkeeping_from_a_torch_written_pair(tmp_path):
    """train.py:68-69, 84-89: steps + 1, last_epoch = epoch, the optimiser entries load into FusedAdamW, and the scheduler built with
    last_epoch goes on from the stored rate as it does over torch's own AdamW."""
    lr0, decay = 2e-4, 0.9

    def make(cls):
        gen = torch.Generator().manual_seed(0)
        ps = [torch.nn.Parameter(torch.randn(4, 3, generator=gen)), torch.nn.Parameter(torch.randn(5, generator=gen))]
        return ps, cls(ps, lr0, betas=[0.8, 0.99])

    ps, opt = make(torch.optim.AdamW)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=decay, last_epoch=-1)
    for _ in range(3):  # three one-step epochs; the pair is written inside the third (epoch 2), before its scheduler step
        for p in ps:
            p.grad = torch.ones_like(p)
        opt.step()
        if _ < 2:
            sched.step()
    g, do = voc_train.checkpoint_pair(str(tmp_path), 2)
    torch.save({"generator": {}}, g)
    torch.save({"mpd": {}, "msd": {}, "optim_g": opt.state_dict(), "optim_d": opt.state_dict(), "steps": 2, "epoch": 2}, do)
    sd = torch.load(voc_train.find_resume(str(tmp_path))[1], weights_only=True)
    assert sorted(sd) == ["epoch", "mpd", "msd", "optim_d", "optim_g", "steps"]  # no segment_rng_state: a reference-written file
    steps, last_epoch = voc_train.resume_bookkeeping(sd)
    assert (steps, last_epoch) == (3, 2)
    resumed = {}
    for name, cls in (("ours", FusedAdamW), ("torch", torch.optim.AdamW)):
        ps2, opt2 = make(cls)
        opt2.load_state_dict(sd["optim_g"])
        assert opt2.param_groups[0]["lr"] == pytest.approx(lr0 * decay ** 2, rel=1e-12) and opt2.param_groups[0]["initial_lr"] == lr0
        assert all(float(opt2.state[p]["step"]) == 3.0 for p in ps2)
        s2 = torch.optim.lr_scheduler.ExponentialLR(opt2, gamma=decay, last_epoch=last_epoch)
        resumed[name] = (opt2.param_groups[0]["lr"], s2.last_epoch)
    assert resumed["ours"] == resumed["torch"]
    assert list(range(max(0, last_epoch), 5)) == [2, 3, 4] and list(range(max(0, -1), 2)) == [0, 1]


def test_speaker_table_rule():
    files = ["a/en_f_001.wav", "a/hi_m_7.wav", "b/en_f_002.wav"]
    table, fixed = voc_train.speaker_table(files, "_")
    assert fixed and table == data.VOCODER_SPEAKERS and table is not data.VOCODER_SPEAKERS
    table, fixed = voc_train.speaker_table(files + ["c/xx_y_1.wav"], "_")
    assert not fixed and table == {"en_f": 0, "hi_m": 1, "xx_y": 2}  # the reference's sorted table
    assert voc_train.speaker_table(files, None) == (None, True)
    assert voc_train.speaker_table(files, "single")[1] is False  # 'A' is no name of the fixed table


def test_refuses_to_run_without_a_gpu(tmp_path):
    cfg = tmp_path / "config.json"
    cfg.write_text(json.dumps({"seed": 1}))
    if torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="needs a GPU"):
            voc_train.main(["--config", str(cfg), "--checkpoint_path", str(tmp_path / "ck"), "--device", "cpu"])
    else:
        with pytest.raises(RuntimeError, match="needs a GPU"):
            voc_train.main(["--config", str(cfg), "--checkpoint_path", str(tmp_path / "ck")])
    assert not (tmp_path / "ck").exists()
    with pytest.raises(ValueError):
        voc_train.build_optimizers(None, None, None, None, "sgd")
