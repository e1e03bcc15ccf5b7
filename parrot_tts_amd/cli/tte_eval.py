#!/usr/bin/env python3
"""Validation loss of a TTE checkpoint: the reference's ``LitParrot.validation_step`` (train.py:87-95: the teacher-forced
``Parrot.forward`` and ``ModelLoss``) over <root_path>/<split>.txt, on the GPU.

    python -m parrot_tts_amd.cli.tte_eval --config utils/TTE/TTE_config.yaml --checkpoint_pth CKPT [--split val] [--batch_size 1]

Prints one JSON line: val_total_loss / val_code_loss / val_dur_loss (the mean of the per-batch values, weighted by batch size,
as Lightning averages a validation epoch), unit_accuracy (argmax == target over the non-padded code positions) and
n_utterances.  Batches are collated in file order like the reference's validation DataLoader."""
import argparse
import json

import torch
import yaml

from ..checkpoint import LitParrot
from ..data import ParrotDataset


def evaluate(model: LitParrot, ds: ParrotDataset, batch_size: int, device) -> dict:
    model.eval()
    tot = {"val_total_loss": 0.0, "val_code_loss": 0.0, "val_dur_loss": 0.0}
    n_utt = n_valid = n_correct = 0
    for s in range(0, len(ds), batch_size):
        batch = ds.collate_fn([ds[i] for i in range(s, min(len(ds), s + batch_size))])
        gpu = {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
        model.validation_step(gpu, s // batch_size)
        b = len(batch["ids"])
        for k in tot:
            tot[k] += float(model.logged[k]) * b
        n_utt += b
        n_valid += model.loss_fn.last_stats["n_valid"]
        n_correct += model.loss_fn.last_stats["n_correct"]
    res = {k: v / max(n_utt, 1) for k, v in tot.items()}
    res["unit_accuracy"] = n_correct / n_valid if n_valid else float("nan")
    res["n_utterances"] = n_utt
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=str, required=True)
    ap.add_argument("--checkpoint_pth", type=str, required=True)
    ap.add_argument("--split", type=str, default="val")
    ap.add_argument("--batch_size", type=int, default=1)
    ap.add_argument("--device", type=str, default="cuda:0")
    a = ap.parse_args(argv)
    cfg = yaml.load(open(a.config, "r"), Loader=yaml.FullLoader)
    ds = ParrotDataset(a.split, data_config=cfg)
    model = LitParrot.load_from_checkpoint(a.checkpoint_pth, weights_only=True).to(a.device)
    with torch.no_grad():
        res = evaluate(model, ds, a.batch_size, a.device)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
