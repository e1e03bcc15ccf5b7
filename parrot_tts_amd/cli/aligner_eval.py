#!/usr/bin/env python3
"""Validation metric of an aligner checkpoint: the CTC loss the reference trains on (utils/aligner/trainer.py:60-63), on the GPU.

    python -m parrot_tts_amd.cli.aligner_eval --config utils/aligner/aligner_train_config.yaml [--model CKPT] [--batch_size 8]
        [--per_item]

It reads what ``align_durations`` reads (and through the same code): ``paths.data_dir`` of the config holds ``dataset.pkl``,
``symbols.pkl``, ``mels/ID.npy`` and ``tokens/ID.npy``; the checkpoint (default ``<data_dir>/checkpoints/latest_model.pt``) must
carry the dataset's symbols.  Nothing is written.

Batches are formed in dataset order and zero-padded to the batch's own longest mel; the network runs over the padding as the
reference's does, so a row's logits -- and with them its loss -- depend on the batch it rides in: compare checkpoints at the
same ``--batch_size``.  An item's loss is ``nll / tokens_len``, the term torch's ``reduction='mean'`` averages.  An item that has
no alignment at all (``mel_len < tokens_len + repeated neighbours``; the reference's trainer skips such a step, trainer.py:67) is
``+inf``: it is counted and left out of the mean.  A failing item (a missing file, a token outside the symbol table, a
non-finite logit) is reported and skipped.

Prints one JSON line: ``ctc_loss`` (the mean of ``nll / tokens_len`` over the finite items; null when there is none), ``n_items``,
``n_infeasible``, ``n_failed``, ``n_batches``, ``step``, ``precision``, and with --per_item ``items``: {item_id: nll / tokens_len}."""
import argparse
import json
import math
import sys

import torch

from .align_durations import load_batch, load_model, open_corpus, plan_batches, read_config


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="CTC validation loss of an aligner checkpoint (GPU).")
    ap.add_argument("--config", "-c", default="utils/aligner/aligner_train_config.yaml", type=str, help="Points to the config file.")
    ap.add_argument("--model", "-m", default=None, type=str, help="Points to the a model file to restore.")
    ap.add_argument("--batch_size", "-b", default=8, type=int, help="Batch size.")
    ap.add_argument("--per_item", action="store_true", help="Also report every item's loss.")
    return ap.parse_args(argv)


def device_ctc_loss(logits, tokens, mel_len, tokens_len):
    from ..aligner import ctc_loss
    return ctc_loss(logits, tokens, mel_len, tokens_len, reduction="none")


def run(args, model_loader=load_model, loss_fn=device_ctc_loss, device=None) -> dict:
    """``loss_fn(logits, tokens, mel_len, tokens_len) -> nll (B)``: the device's ``ctc_loss`` (tests on a host pass torch's)."""
    config = read_config(args.config)
    device = torch.device("cuda") if device is None else torch.device(device)
    _, model, dataset, n_mels, mel_dir, token_dir = open_corpus(config, args.model, model_loader, device)
    batches = plan_batches(len(dataset), max(1, int(args.batch_size)))
    items_out = {}
    n_failed = 0
    for idx in batches:
        items, mel, tokens, mel_len, tokens_len, failed = load_batch(dataset, idx, mel_dir, token_dir, n_mels)
        n_failed += failed
        if not items:
            continue
        try:
            logits = model(mel.to(device))
        except Exception as e:
            print(f"Error processing {[it['item_id'] for it in items]}: {e}", file=sys.stderr)
            n_failed += len(items)
            continue
        tokens = tokens.to(device)
        try:
            nll = loss_fn(logits, tokens, mel_len, tokens_len).cpu().tolist()
        except Exception:  # one bad item fails the call: find it row by row, on the same logits
            nll = None
        for b, item in enumerate(items):
            try:
                v = nll[b] if nll is not None else float(loss_fn(logits[b:b + 1], tokens[b:b + 1], mel_len[b:b + 1], tokens_len[b:b + 1]).cpu()[0])
                if math.isnan(v):
                    raise FloatingPointError("the loss is NaN")
                items_out[item["item_id"]] = v / tokens_len[b]
            except Exception as e:
                print(f"Error processing {item['item_id']}: {e}", file=sys.stderr)
                n_failed += 1
    finite = [v for v in items_out.values() if math.isfinite(v)]
    out = {"ctc_loss": math.fsum(finite) / len(finite) if finite else None, "n_items": len(dataset), "n_infeasible": len(items_out) - len(finite),
           "n_failed": n_failed, "n_batches": len(batches), "step": int(model.get_step()), "precision": getattr(model, "precision_in_use", None)}
    if args.per_item:
        out["items"] = items_out
    return out


def main(argv=None):
    print(json.dumps(run(parse_args(argv))))


if __name__ == "__main__":
    main()
