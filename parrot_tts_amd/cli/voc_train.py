#!/usr/bin/env python3
"""Train the unit vocoder on one GPU: the reference's ``utils/vocoder/train.py`` over the five device parts --
``TrainableCodeGenerator``, ``TrainableMultiPeriodDiscriminator`` / ``TrainableMultiScaleDiscriminator``, ``MelL1Loss`` and the fused
adversarial losses -- with both AdamW updates on the fused multi-tensor kernel (``optim.FusedAdamW``).

    python -m parrot_tts_amd.cli.voc_train --config utils/vocoder/config.json --checkpoint_path runs/vocoder/checkpoints \
        [--training_epochs 4000 --training_steps 800000 --stdout_interval 5 --checkpoint_interval 10000 --validation_interval 1000]
        [--device cuda:0] [--optimizer fused|torch]

``config.json`` carries the reference's keys; two optional ones, ``"mpd": {...}`` and ``"msd": {...}``, hold constructor arguments of
the two discriminators (absent: the reference's hard-coded widths).  The step (``train_step``) follows train.py:125-168 in their
order: the generator's forward, the discriminator step on ``y_g_hat.detach()``, then the generator step through ``45 * MelL1Loss`` plus
the adversarial and feature-matching terms on the UPDATED discriminators.  During the generator step the discriminators' parameters
do not require grad: their weight-gradient kernels are skipped (``optim_d.zero_grad()`` would discard those gradients in any case) and
the generator's gradients do not change by a bit.  The mel target of the batch's real audio is formed per batch on the device.
Batches are ``h.batch_size`` items in manifest order, no shuffle, the last short batch dropped (train.py:99-100); segments come from
``data.SegmentCodeDataset``; two ``ExponentialLR(gamma=h.lr_decay)`` are stepped once per epoch.

One JSON line per logged step: ``step``, ``epoch``, ``lr``, ``gen_loss_total``, ``mel_spec_error``, ``disc_loss_total``,
``s_per_batch``, and ``val_mel_spec_error`` / ``checkpoint`` when that step validated / saved.  Validation loads the generator's
current weights into the inference ``CodeGenerator`` and scores WHOLE utterances of ``input_validation_file`` with ``voc_eval``'s
``collect_rows`` / ``evaluate`` (the stance of voc_eval's docstring against the reference's random-segment number).  Checkpoints are
the reference's: ``g_%08d`` = {'generator'}, ``do_%08d`` = {'mpd', 'msd', 'optim_g', 'optim_d', 'steps', 'epoch'} plus
``segment_rng_state`` (the dataset's ``Random.getstate()``, which the reference ignores), every ``--checkpoint_interval`` steps (not
at step 0) and at the end.  When ``--checkpoint_path`` holds both a ``g_`` and a ``do_`` the run resumes as train.py:54-69, 84-89:
weights, both optimiser states, ``steps + 1``, the epoch loop from ``max(0, last_epoch)``, schedulers with ``last_epoch``, and the
segment RNG state when the key is there.

Two deliberate departures from the reference's ``main``: the checkpoint directory is never deleted (the reference's
``shutil.rmtree`` makes its own resume unreachable), and reaching ``--training_steps`` ends the run (the reference's ``break`` leaves
only the inner loop).  When every speaker of the training manifest is in ``data.VOCODER_SPEAKERS`` those ids are used, so that
``voc_eval`` / ``voc_infer`` read the checkpoint with the same table; otherwise the reference's sorted table is used and one warning
line says so.  Single GPU only (no DDP, no TensorBoard, no f0); without a GPU it fails loudly."""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np
import torch

from ..checkpoint import scan_checkpoint
from ..data import VOCODER_SPEAKERS, CodeDataset, SegmentCodeDataset, parse_manifest, parse_speaker
from ..vocoder import AttrDict

MEL_WEIGHT = 45  # train.py:157


def lr_at(lr0: float, decay: float, epoch: int) -> float:
    """The learning rate of a fresh run's epoch (0-based): ExponentialLR stepped once per epoch."""
    return lr0 * decay ** epoch


def epoch_batches(n_items: int, batch_size: int):
    """train.py:99-100: manifest order, no shuffle, the last short batch dropped -> index lists."""
    return [list(range(s, s + batch_size)) for s in range(0, n_items - batch_size + 1, batch_size)]


def speaker_table(audio_files, multispkr):
    """-> (spkr_to_id or None, fixed): ``data.VOCODER_SPEAKERS`` when it holds every speaker of the manifest (fixed = True), else the
    reference's table sorted from the manifest's names (dataset.py:170-175)."""
    if not multispkr:
        return None, True
    names = sorted({parse_speaker(f, multispkr) for f in audio_files})
    if all(n in VOCODER_SPEAKERS for n in names):
        return dict(VOCODER_SPEAKERS), True
    return {k: v for v, k in enumerate(names)}, False


def checkpoint_pair(cp_dir, steps: int):
    return os.path.join(cp_dir, "g_{:08d}".format(steps)), os.path.join(cp_dir, "do_{:08d}".format(steps))


def find_resume(cp_dir):
    """train.py:54-61: the newest ``g_`` and ``do_`` of the directory, or None unless both exist."""
    if not os.path.isdir(cp_dir):
        return None
    cp_g, cp_do = scan_checkpoint(cp_dir, "g_"), scan_checkpoint(cp_dir, "do_")
    return None if cp_g is None or cp_do is None else (cp_g, cp_do)


def resume_bookkeeping(state_dict_do):
    """train.py:68-69 -> (steps, last_epoch)."""
    return int(state_dict_do["steps"]) + 1, int(state_dict_do["epoch"])


def require_gpu(device: str) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError(f"parrot_tts_amd: voc_train needs a GPU (got --device {device}, torch.cuda.is_available() = "
                           f"{torch.cuda.is_available()}); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def build_models(h, dev):
    from ..discriminator_train import TrainableMultiPeriodDiscriminator
    from ..msd_train import TrainableMultiScaleDiscriminator
    from ..vocoder_train import TrainableCodeGenerator
    generator = TrainableCodeGenerator(h).to(dev)
    mpd = TrainableMultiPeriodDiscriminator(**dict(h.get("mpd") or {})).to(dev)
    msd = TrainableMultiScaleDiscriminator(**dict(h.get("msd") or {})).to(dev)
    return generator, mpd, msd


def build_optimizers(h, generator, mpd, msd, kind: str = "fused"):
    """train.py:80-82; ``kind``: 'fused' (optim.FusedAdamW) or 'torch' (torch.optim.AdamW, for A/B)."""
    if kind == "fused":
        from ..optim import FusedAdamW as cls
    elif kind == "torch":
        cls = torch.optim.AdamW
    else:
        raise ValueError(f"--optimizer must be 'fused' or 'torch', got {kind!r}")
    optim_g = cls(generator.parameters(), h.learning_rate, betas=[h.adam_b1, h.adam_b2])
    optim_d = cls(itertools.chain(msd.parameters(), mpd.parameters()), h.learning_rate, betas=[h.adam_b1, h.adam_b2])
    return optim_g, optim_d


def collate(items, dev):
    """The default collate of the reference's DataLoader over ``(feats, audio, filename, None)`` -> (x, y (B, 1, N)) on the device."""
    x = {"code": torch.from_numpy(np.stack([np.asarray(it[0]["code"], dtype=np.int64) for it in items])).to(dev)}
    if "spkr" in items[0][0]:
        x["spkr"] = torch.from_numpy(np.stack([it[0]["spkr"] for it in items])).to(dev)
    y = torch.stack([it[1] for it in items]).to(dev).unsqueeze(1)
    return x, y


def train_step(generator, mpd, msd, optim_g, optim_d, mel_loss, x, y, freeze_discriminators: bool = True, update: bool = True):
    """train.py:131-168 -> {'gen_loss_total', 'disc_loss_total', 'loss_mel'} (0-dim device tensors) and 'y_g_hat' / 'y_mel'.
    ``update=False`` forms losses and gradients and leaves the parameters alone; ``freeze_discriminators=False`` lets the generator
    step compute the discriminators' weight gradients as the reference does (they are discarded either way)."""
    from ..gan_loss import discriminator_adversarial_loss, generator_adversarial_loss
    y_g_hat = generator(**x)
    assert y_g_hat.shape == y.shape, f"Mismatch in vocoder output shape - {y_g_hat.shape} != {y.shape}"
    with torch.no_grad():
        y_mel = mel_loss.mel(y[:, 0])
    # discriminators (train.py:138-151)
    optim_d.zero_grad()
    y_df_hat_r, y_df_hat_g, _, _ = mpd(y, y_g_hat.detach())
    y_ds_hat_r, y_ds_hat_g, _, _ = msd(y, y_g_hat.detach())
    loss_disc_all, _ = discriminator_adversarial_loss(y_df_hat_r, y_df_hat_g, y_ds_hat_r, y_ds_hat_g)
    loss_disc_all.backward()
    if update:
        optim_d.step()
    # generator (train.py:154-168)
    optim_g.zero_grad()
    disc_params = [p for p in itertools.chain(msd.parameters(), mpd.parameters()) if p.requires_grad] if freeze_discriminators else []
    for p in disc_params:
        p.requires_grad_(False)
    try:
        loss_mel = mel_loss(y_g_hat, y_mel) * MEL_WEIGHT
        y_df_hat_r, y_df_hat_g, fmap_f_r, fmap_f_g = mpd(y, y_g_hat)
        y_ds_hat_r, y_ds_hat_g, fmap_s_r, fmap_s_g = msd(y, y_g_hat)
        loss_adv, _ = generator_adversarial_loss(y_df_hat_g, y_ds_hat_g, fmap_f_r, fmap_f_g, fmap_s_r, fmap_s_g)
        loss_gen_all = loss_adv + loss_mel
        loss_gen_all.backward()
    finally:
        for p in disc_params:
            p.requires_grad_(True)
    if update:
        optim_g.step()
    return {"gen_loss_total": loss_gen_all.detach(), "disc_loss_total": loss_disc_all.detach(), "loss_mel": loss_mel.detach(),
            "y_g_hat": y_g_hat.detach(), "y_mel": y_mel}


def validation_rows(h, table, fixed: bool):
    """The whole utterances of ``input_validation_file`` as voc_eval's rows (speaker ids from the run's own table)."""
    from .voc_eval import collect_rows
    ds = CodeDataset(parse_manifest(h.input_validation_file), -1, h.code_hop_size, sampling_rate=h.sampling_rate,
                     multispkr=h.get("multispkr", None))
    if fixed:
        return collect_rows(ds, h)
    rows, skipped = [], 0  # (collect_rows with the manifest's own table)
    for item in range(len(ds)):
        feats, gt_audio, filename, _ = ds[item]
        code = np.asarray(feats["code"], dtype=np.int64).reshape(-1)
        if gt_audio is None or code.size == 0:
            skipped += 1
            continue
        rows.append((code, table[parse_speaker(filename, h["multispkr"])], gt_audio.reshape(-1).to(torch.float32), os.path.splitext(
            os.path.basename(filename))[0]))
    return rows, skipped


def validate(generator, h, mel, rows, dev) -> float:
    """train.py:198-227 over whole utterances: the generator's current weights in the inference ``CodeGenerator``."""
    from ..vocoder import CodeGenerator
    from .voc_eval import evaluate
    g = CodeGenerator(h)
    g.load_state_dict({k: v.detach().cpu() for k, v in generator.state_dict().items()})
    g.eval()
    g.remove_weight_norm()
    g = g.to(dev)
    with torch.no_grad():
        errs = evaluate(g, mel, rows, dev)
    g.check_inputs()
    return float(np.mean(errs)) if len(errs) else float("nan")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--group_name", default=None)
    ap.add_argument("--checkpoint_path", default="runs/vocoder/checkpoints")
    ap.add_argument("--config", default="")
    ap.add_argument("--training_epochs", default=4000, type=int)
    ap.add_argument("--training_steps", default=800000, type=int)
    ap.add_argument("--stdout_interval", default=5, type=int)
    ap.add_argument("--checkpoint_interval", default=10000, type=int)
    ap.add_argument("--summary_interval", default=100, type=int, help="accepted and unused: there is no TensorBoard")
    ap.add_argument("--validation_interval", default=1000, type=int)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--optimizer", default="fused", choices=("fused", "torch"), help="fused: optim.FusedAdamW; torch: torch.optim.AdamW")
    a = ap.parse_args(argv)
    dev = require_gpu(a.device)
    with open(a.config) as f:
        h = AttrDict(json.load(f))
    from ..mel import MelL1Loss

    os.makedirs(a.checkpoint_path, exist_ok=True)  # (never deleted: see the docstring)
    torch.manual_seed(h.seed)
    torch.cuda.manual_seed(h.seed)
    generator, mpd, msd = build_models(h, dev)
    steps, last_epoch, state_dict_do = 0, -1, None
    found = find_resume(a.checkpoint_path)
    if found is not None:
        state_dict_g = torch.load(found[0], map_location=dev, weights_only=True)
        state_dict_do = torch.load(found[1], map_location=dev, weights_only=True)
        generator.load_state_dict(state_dict_g["generator"])
        mpd.load_state_dict(state_dict_do["mpd"])
        msd.load_state_dict(state_dict_do["msd"])
        steps, last_epoch = resume_bookkeeping(state_dict_do)
    optim_g, optim_d = build_optimizers(h, generator, mpd, msd, a.optimizer)
    if state_dict_do is not None:
        optim_g.load_state_dict(state_dict_do["optim_g"])
        optim_d.load_state_dict(state_dict_do["optim_d"])
    scheduler_g = torch.optim.lr_scheduler.ExponentialLR(optim_g, gamma=h.lr_decay, last_epoch=last_epoch)
    scheduler_d = torch.optim.lr_scheduler.ExponentialLR(optim_d, gamma=h.lr_decay, last_epoch=last_epoch)

    training_filelist = parse_manifest(h.input_training_file)
    table, fixed = speaker_table(training_filelist[0], h.get("multispkr", None))
    if not fixed:
        print(f"voc_train: warning: speakers outside data.VOCODER_SPEAKERS; using the manifest's sorted table {table} "
              "(voc_eval / voc_infer read checkpoints with the fixed table)", file=sys.stderr, flush=True)
    trainset = SegmentCodeDataset(training_filelist, h.segment_size, h.code_hop_size, sampling_rate=h.sampling_rate,
                                  multispkr=h.get("multispkr", None), spkr_to_id=table)
    if state_dict_do is not None and "segment_rng_state" in state_dict_do:
        trainset.set_rng_state(state_dict_do["segment_rng_state"])
    batches = epoch_batches(len(trainset), h.batch_size)
    mel_loss = MelL1Loss(h)
    val_rows = None

    def save(step, epoch):
        cp_g, cp_do = checkpoint_pair(a.checkpoint_path, step)
        torch.save({"generator": generator.state_dict()}, cp_g)
        torch.save({"mpd": mpd.state_dict(), "msd": msd.state_dict(), "optim_g": optim_g.state_dict(), "optim_d": optim_d.state_dict(),
                    "steps": step, "epoch": epoch, "segment_rng_state": trainset.rng_state()}, cp_do)
        return cp_g

    generator.train()
    mpd.train()
    msd.train()
    records, done = [], steps >= a.training_steps
    for epoch in range(max(0, last_epoch), a.training_epochs):
        if done:
            break
        for i, idx in enumerate(batches):
            start_b = time.time()
            x, y = collate([trainset[j] for j in idx], dev)
            lr = optim_g.param_groups[0]["lr"]
            out = train_step(generator, mpd, msd, optim_g, optim_d, mel_loss, x, y)
            final = steps + 1 >= a.training_steps or (epoch == a.training_epochs - 1 and i == len(batches) - 1)
            rec = None
            if steps % a.stdout_interval == 0 or final:
                rec = {"step": steps, "epoch": epoch, "lr": lr, "gen_loss_total": float(out["gen_loss_total"]),
                       "mel_spec_error": float(out["loss_mel"]) / MEL_WEIGHT, "disc_loss_total": float(out["disc_loss_total"]),
                       "s_per_batch": time.time() - start_b}
            extra = {}
            if (steps % a.checkpoint_interval == 0 and steps != 0) or final:
                extra["checkpoint"] = save(steps, epoch)
            if steps % a.validation_interval == 0:
                if val_rows is None:
                    val_rows = validation_rows(h, table, fixed)[0]
                extra["val_mel_spec_error"] = validate(generator, h, mel_loss.mel, val_rows, dev)
            if extra and rec is None:
                rec = {"step": steps, "epoch": epoch, "lr": lr, "gen_loss_total": float(out["gen_loss_total"]),
                       "mel_spec_error": float(out["loss_mel"]) / MEL_WEIGHT, "disc_loss_total": float(out["disc_loss_total"]),
                       "s_per_batch": time.time() - start_b}
            if rec is not None:
                rec.update(extra)
                print(json.dumps(rec), flush=True)
                records.append(rec)
            steps += 1
            if steps >= a.training_steps:
                done = True
                break
        scheduler_g.step()
        scheduler_d.step()
    return {"steps": steps, "records": records}


if __name__ == "__main__":
    main()
