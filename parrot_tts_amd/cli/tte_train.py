#!/usr/bin/env python3
"""Train the TTE on one GPU: the reference's ``train.py`` without Lightning -- ``LitParrot.training_step`` on a ``TrainableParrot``
(the HIP training forward and backward), AdamW with the config's ``optimizer.init_lr`` and ``weight_decay`` (torch's default betas:
train.py:99-103 passes none), ``get_cosine_schedule_with_warmup`` stepped once per optimiser step, ``train.grad_acc_steps``,
``clip_grad_norm_(train.grad_clip)``, validation every ``train.val_every`` steps through ``validation_step``, a checkpoint every
``train.save_every`` steps (and at the end) in the layout ``tte_eval`` / ``tte_infer`` read back.

    python -m parrot_tts_amd.cli.tte_train --config utils/TTE/TTE_config.yaml [--checkpoint_pth CKPT] [--max_steps N] [--seed 42]

Prints one JSON line per logged step (``train.log_every``): step, lr, the three training losses, and the validation losses when that
step validated.  Runs under ``torch.use_deterministic_algorithms(True)`` (the reference trains with deterministic=True) after
``torch.manual_seed(seed)`` (the reference: ``seed_everything(42)``), which also seeds the dropout.  Single GPU only: DDP and multi-GPU
training are out of scope.  ``--checkpoint_pth`` starts from a checkpoint's WEIGHTS and is not a resume: the optimiser and schedule
state and the dropout offset begin again at step 0 (the checkpoints hold the model only, as ``tte_eval`` / ``tte_infer`` read them)."""
import argparse
import json
import math
import os

import torch
import yaml

from ..checkpoint import LitParrot, save_lightning_style
from ..data import ParrotDataset
from .tte_eval import evaluate


def cosine_schedule_with_warmup(step: int, num_warmup_steps: int, num_training_steps: int, num_cycles: float = 0.5) -> float:
    """The factor ``get_cosine_schedule_with_warmup`` (train.py:13-52) applies to the initial learning rate at ``step``."""
    if step < num_warmup_steps:
        return float(step) / float(max(1, num_warmup_steps))
    progress = float(step - num_warmup_steps) / float(max(1, num_training_steps - num_warmup_steps))
    return max(0.0, 0.5 * (1.0 + math.cos(math.pi * float(num_cycles) * 2.0 * progress)))


def _batches(ds, batch_size: int, gen: torch.Generator):
    """Shuffled epochs without end, collated like the reference's training DataLoader (shuffle=True, the last batch kept)."""
    while True:
        order = torch.randperm(len(ds), generator=gen).tolist()
        for s in range(0, len(order), batch_size):
            yield ds.collate_fn([ds[i] for i in order[s: s + batch_size]])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", type=str, required=True)
    ap.add_argument("--checkpoint_pth", type=str, default=None, help="start from this checkpoint's weights")
    ap.add_argument("--max_steps", type=int, default=None, help="stop after this many optimiser steps (default: train.total_steps)")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--device", type=str, default="cuda:0")
    a = ap.parse_args(argv)
    cfg = yaml.load(open(a.config, "r"), Loader=yaml.FullLoader)
    tc, oc = cfg["train"], cfg["optimizer"]
    torch.manual_seed(a.seed)
    train_ds, val_ds = ParrotDataset("train", data_config=cfg), ParrotDataset("val", data_config=cfg)
    lit = LitParrot(cfg, train_ds.src_vocab_size, train_ds.src_pad_idx, trainable=True)
    if a.checkpoint_pth:
        lit.load_state_dict(torch.load(a.checkpoint_pth, map_location="cpu", weights_only=True)["state_dict"], strict=True)
    lit = lit.to(a.device)
    optim = torch.optim.AdamW(lit.parrot.parameters(), lr=oc["init_lr"], weight_decay=oc["weight_decay"])
    sched = torch.optim.lr_scheduler.LambdaLR(optim, lambda k: cosine_schedule_with_warmup(k, tc["warmup_steps"], tc["total_steps"]))
    total = tc["total_steps"] if a.max_steps is None else min(a.max_steps, tc["total_steps"])
    acc, ckpt_dir = max(1, int(tc["grad_acc_steps"])), os.path.join(cfg["path"]["root_path"], "ckpt")
    os.makedirs(ckpt_dir, exist_ok=True)
    batches = _batches(train_ds, tc["batch_size"], torch.Generator().manual_seed(a.seed))
    records, last = [], None

    def save(step):
        path = os.path.join(ckpt_dir, f"parrot_model-step={step}.ckpt")
        save_lightning_style(path, {k: v.detach().cpu() for k, v in lit.parrot.state_dict().items()}, cfg, train_ds.src_vocab_size,
                             train_ds.src_pad_idx)
        return path

    torch.use_deterministic_algorithms(True)
    try:
        for step in range(1, total + 1):
            lit.train()
            optim.zero_grad()
            for micro in range(acc):  # Lightning's accumulate_grad_batches: every micro-batch's loss is divided by their number
                batch = next(batches)
                gpu = {k: (v.to(a.device) if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
                loss = lit.training_step(gpu, (step - 1) * acc + micro)
                (loss / acc).backward()
            torch.nn.utils.clip_grad_norm_(lit.parrot.parameters(), tc["grad_clip"])
            lr = optim.param_groups[0]["lr"]
            optim.step()
            sched.step()
            rec = {"step": step, "lr": lr}
            rec.update({k: float(v.detach()) for k, v in lit.logged.items() if k.startswith("train_")})
            if tc["val_every"] and step % tc["val_every"] == 0:
                with torch.no_grad():
                    rec.update(evaluate(lit, val_ds, tc["batch_size"], a.device))
            if tc["save_every"] and step % tc["save_every"] == 0:
                last = save(step)
                rec["checkpoint"] = last
            if step % max(1, int(tc.get("log_every", 1))) == 0 or "checkpoint" in rec or "val_total_loss" in rec or step == total:
                print(json.dumps(rec), flush=True)
                records.append(rec)
        if total and (last is None or not last.endswith(f"step={total}.ckpt")):
            last = save(total)
    finally:
        torch.use_deterministic_algorithms(False)
    return {"steps": total, "checkpoint": last, "records": records}


if __name__ == "__main__":
    main()
