"""GPU: python -m parrot_tts_amd.cli.voc_train end to end on a reduced vocoder -- synth.small_voc_config() with the mel keys of the
reference's config.json, narrow discriminators through the "mpd" / "msd" keys, segment_size 8960, batch_size 2, three synthetic wavs
(one shorter than a segment, two speakers), four one-step epochs with a checkpoint and a validation every second step."""
import itertools
import json
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from mpd_ref import NARROW as MPD_NARROW
from msd_ref import NARROW

pytestmark = pytest.mark.gpu

from parrot_tts_amd import data, synth  # noqa: E402
from parrot_tts_amd.cli import voc_eval, voc_train  # noqa: E402
from parrot_tts_amd.vocoder import AttrDict  # noqa: E402

DEV = "cuda:0"
LR0, DECAY = 2e-4, 0.999
KEYS = {"step", "epoch", "lr", "gen_loss_total", "mel_spec_error", "disc_loss_total", "s_per_batch"}


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    root = tmp_path_factory.mktemp("voc_train")
    rng = np.random.default_rng(3)
    lines = []
    for name, n in (("en_f_0.wav", 6400), ("hi_m_1.wav", 12800 + 77), ("en_f_2.wav", 19200)):
        t = np.arange(n) / 16000.0
        x = (np.sin(2 * np.pi * 220.0 * t * (1 + len(lines))) * 6000 + rng.standard_normal(n) * 1500).astype(np.int16)
        wavfile.write(str(root / name), 16000, x)
        units = " ".join(str(v) for v in rng.integers(0, 100, n // 320))
        lines.append(str({"audio": str(root / name), "hubert": units}))
    manifest = root / "train.txt"
    manifest.write_text("\n".join(lines) + "\n")
    h = synth.small_voc_config()
    h.update(input_training_file=str(manifest), input_validation_file=str(manifest), batch_size=2, learning_rate=LR0, adam_b1=0.8,
             adam_b2=0.99, lr_decay=DECAY, segment_size=8960, num_mels=80, num_freq=1025, n_fft=1024, hop_size=256, win_size=1024,
             fmin=0, fmax=8000, fmax_for_loss=None, num_gpus=0, mpd={"channels": MPD_NARROW}, msd={"channels": NARROW})
    cfg = root / "config.json"
    cfg.write_text(json.dumps(h))
    return root, cfg, AttrDict(h)


def _run(cfg, ckpt, steps, extra=()):
    """One run of the driver -> the records it printed (main returns them as well)."""
    res = voc_train.main(["--config", str(cfg), "--checkpoint_path", str(ckpt), "--training_steps", str(steps), "--checkpoint_interval", "2",
                          "--validation_interval", "2", "--stdout_interval", "1", "--device", DEV, *extra])
    return res["records"]


@pytest.fixture(scope="module")
def first_run(setup):
    root, cfg, h = setup
    return _run(cfg, root / "ck_a", 4), root / "ck_a"


def _load(path):
    return torch.load(path, map_location="cpu", weights_only=True)


def _same(a, b):
    if isinstance(a, torch.Tensor):
        if not isinstance(b, torch.Tensor) or a.dtype != b.dtype or a.shape != b.shape:
            return False
        return torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))  # (bits: a NaN equals itself)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def test_json_lines_checkpoints_and_keys(setup, first_run):
    _, _, h = setup
    recs, ck = first_run
    assert [r["step"] for r in recs] == [0, 1, 2, 3] and [r["epoch"] for r in recs] == [0, 1, 2, 3]
    for r in recs:
        assert KEYS <= set(r) <= KEYS | {"val_mel_spec_error", "checkpoint"}
        assert r["lr"] == pytest.approx(LR0 * DECAY ** r["epoch"], rel=1e-12)
        assert all(np.isfinite(r[k]) for k in r if k != "checkpoint") and r["s_per_batch"] > 0
    assert ["val_mel_spec_error" in r for r in recs] == [True, False, True, False]
    assert ["checkpoint" in r for r in recs] == [False, False, True, True]
    assert sorted(os.listdir(ck)) == ["do_00000002", "do_00000003", "g_00000002", "g_00000003"]
    g, do = _load(ck / "g_00000003"), _load(ck / "do_00000003")
    assert list(g) == ["generator"]
    assert set(do) == {"mpd", "msd", "optim_g", "optim_d", "steps", "epoch", "segment_rng_state"} and do["steps"] == 3 and do["epoch"] == 3
    assert _load(ck / "do_00000002")["steps"] == 2
    generator, mpd, msd = voc_train.build_models(h, "cpu")
    generator.load_state_dict(g["generator"], strict=True)
    mpd.load_state_dict(do["mpd"], strict=True)
    msd.load_state_dict(do["msd"], strict=True)
    for params, key in ((itertools.chain(msd.parameters(), mpd.parameters()), "optim_d"), (generator.parameters(), "optim_g")):
        opt = torch.optim.AdamW(params, LR0, betas=[0.8, 0.99])
        opt.load_state_dict(do[key])
        st = next(iter(opt.state.values()))
        assert float(st["step"]) == 4.0 and opt.param_groups[0]["lr"] == pytest.approx(LR0 * DECAY ** 3, rel=1e-12)


def test_last_validation_equals_voc_eval_on_the_written_checkpoint(setup, first_run, capsys):
    _, cfg, h = setup
    recs, ck = first_run
    res = voc_eval.main(["--checkpoint_file", str(ck / "g_00000002"), "--config", str(cfg), "--input_code_file", h.input_validation_file])
    assert res["n_utterances"] == 3 and res["mel_spec_error"] == recs[2]["val_mel_spec_error"]


def _first_batch(h, dev):
    """The set-up of main() up to its first batch."""
    torch.manual_seed(h.seed)
    torch.cuda.manual_seed(h.seed)
    generator, mpd, msd = voc_train.build_models(h, dev)
    files = data.parse_manifest(h.input_training_file)
    table, _ = voc_train.speaker_table(files[0], h.multispkr)
    ds = data.SegmentCodeDataset(files, h.segment_size, h.code_hop_size, sampling_rate=h.sampling_rate, multispkr=h.multispkr, spkr_to_id=table)
    x, y = voc_train.collate([ds[j] for j in voc_train.epoch_batches(len(ds), h.batch_size)[0]], dev)
    for m in (generator, mpd, msd):
        m.train()
    return generator, mpd, msd, x, y


def test_step_one_losses_equal_a_composition_of_the_parts(setup, first_run):
    """The reference's order (train.py:131-165) written out over the parts.  disc_loss_total is formed before any update;
    gen_loss_total sees the discriminators after their first update (train.py:151, 159-160), so the composition makes that update too:
    it is deterministic."""
    from parrot_tts_amd.gan_loss import discriminator_adversarial_loss, generator_adversarial_loss
    from parrot_tts_amd.mel import MelL1Loss, MelSpectrogram
    _, _, h = setup
    recs, _ = first_run
    generator, mpd, msd, x, y = _first_batch(h, torch.device(DEV))
    _, optim_d = voc_train.build_optimizers(h, generator, mpd, msd)
    y_g_hat = generator(**x)
    y_mel = MelSpectrogram(h)(y[:, 0])
    optim_d.zero_grad()
    y_df_hat_r, y_df_hat_g, _, _ = mpd(y, y_g_hat.detach())
    y_ds_hat_r, y_ds_hat_g, _, _ = msd(y, y_g_hat.detach())
    loss_disc_all, _ = discriminator_adversarial_loss(y_df_hat_r, y_df_hat_g, y_ds_hat_r, y_ds_hat_g)
    assert float(loss_disc_all) == recs[0]["disc_loss_total"]
    loss_disc_all.backward()
    optim_d.step()
    loss_mel = MelL1Loss(h)(y_g_hat, y_mel) * 45
    y_df_hat_r, y_df_hat_g, fmap_f_r, fmap_f_g = mpd(y, y_g_hat)
    y_ds_hat_r, y_ds_hat_g, fmap_s_r, fmap_s_g = msd(y, y_g_hat)
    loss_adv, _ = generator_adversarial_loss(y_df_hat_g, y_ds_hat_g, fmap_f_r, fmap_f_g, fmap_s_r, fmap_s_g)
    assert float(loss_adv + loss_mel) == recs[0]["gen_loss_total"]
    assert float(loss_mel) / 45 == recs[0]["mel_spec_error"]


def test_generator_gradients_with_frozen_discriminators_are_those_with_them_unfrozen(setup):
    from parrot_tts_amd.mel import MelL1Loss
    _, _, h = setup
    grads = []
    for freeze in (True, False):
        generator, mpd, msd, x, y = _first_batch(h, torch.device(DEV))
        optim_g, optim_d = voc_train.build_optimizers(h, generator, mpd, msd)
        voc_train.train_step(generator, mpd, msd, optim_g, optim_d, MelL1Loss(h), x, y, freeze_discriminators=freeze, update=False)
        assert all(p.requires_grad for p in itertools.chain(msd.parameters(), mpd.parameters()))  # restored
        grads.append([p.grad.clone() for p in generator.parameters()])
        assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads[-1]) and any(bool(g.abs().sum() > 0) for g in grads[-1])
    assert len(grads[0]) == len(grads[1]) > 10
    for a, b in zip(*grads):
        assert torch.equal(a, b)


def test_a_second_identical_run_writes_identical_checkpoints(setup, first_run):
    root, cfg, _ = setup
    recs, ck = first_run
    again = _run(cfg, root / "ck_b", 4)
    for name in sorted(os.listdir(ck)):
        assert _same(_load(ck / name), _load(root / "ck_b" / name)), name
    drop = lambda r: {k: v for k, v in r.items() if k not in ("s_per_batch", "checkpoint")}  # noqa: E731
    assert [drop(r) for r in again] == [drop(r) for r in recs]


def test_a_stopped_run_resumes(setup, capsys):
    """train.py:68-69, 88-89: steps + 1, the epoch loop from the stored epoch, schedulers built with last_epoch on the stored rate."""
    root, cfg, _ = setup
    ck = root / "ck_c"
    capsys.readouterr()
    first = _run(cfg, ck, 2)
    printed = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert printed == first and all(KEYS <= set(r) for r in printed)  # one JSON line per logged step
    assert [r["step"] for r in first] == [0, 1] and sorted(os.listdir(ck)) == ["do_00000001", "g_00000001"]
    do = _load(ck / "do_00000001")
    assert do["steps"] == 1 and do["epoch"] == 1 and do["optim_g"]["param_groups"][0]["lr"] == pytest.approx(LR0 * DECAY, rel=1e-12)
    # what the reference's calls give: AdamW with the stored groups, ExponentialLR(last_epoch=stored epoch)
    p = torch.nn.Parameter(torch.zeros(1))
    probe = torch.optim.AdamW([p], LR0)
    probe.param_groups[0].update(lr=do["optim_g"]["param_groups"][0]["lr"], initial_lr=do["optim_g"]["param_groups"][0]["initial_lr"])
    sched = torch.optim.lr_scheduler.ExponentialLR(probe, gamma=DECAY, last_epoch=do["epoch"])
    lr_resumed = probe.param_groups[0]["lr"]
    resumed = _run(cfg, ck, 4)
    assert [r["step"] for r in resumed] == [2, 3] and [r["epoch"] for r in resumed] == [1, 2]
    assert resumed[0]["lr"] == lr_resumed
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sched.step()
    assert resumed[1]["lr"] == probe.param_groups[0]["lr"]
    assert all(np.isfinite(r["gen_loss_total"]) and np.isfinite(r["disc_loss_total"]) for r in resumed)
    assert {"do_00000002", "g_00000002", "do_00000003", "g_00000003"} <= set(os.listdir(ck))
    end = _load(ck / "do_00000003")
    assert end["steps"] == 3 and end["epoch"] == 2
    assert float(next(iter(end["optim_d"]["state"].values()))["step"]) == 4.0
