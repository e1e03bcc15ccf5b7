#!/usr/bin/env python3
"""Duration extraction with a trained aligner, on the GPU: the reference's utils/aligner/extract_durations.py.

    python -m parrot_tts_amd.cli.align_durations --config utils/aligner/aligner_train_config.yaml [--model CKPT] [--target outputs]
        [--batch_size 8]

The same flags and the same inputs: ``paths.data_dir`` of the config holds ``dataset.pkl`` (a list of ``{item_id, mel_len,
tokens_len}``), ``symbols.pkl``, ``mels/ID.npy`` ((mel_len, n_mels) float) and ``tokens/ID.npy``; the checkpoint (default
``<data_dir>/checkpoints/latest_model.pt``) is a dict with ``config``, ``symbols`` and ``model``, and its symbols must equal the
dataset's (extract_durations.py:73-74).  Written under ``<data_dir>/<target>``: ``predictions/ID.npy`` ((mel_len, num_symbols) fp32
softmax) and ``durations/ID.npy`` ((tokens_len,) int32), as the reference does.

Batches are formed in dataset order and zero-padded to the batch's own longest mel; the network runs over the padding as the
reference's does (a row's prediction depends on the batch it rides in -- the reference's binned, shuffled batches are not
reproduced, so neither are its bits for rows shorter than their batch).  A failing item is reported and skipped
(extract_durations.py:43-45).  ``durations.method: beam`` is not covered and exits with a message.  ``--num_workers`` is accepted
and ignored: the dynamic programme runs on the GPU, one workgroup per utterance.

Prints one JSON line: ``n_items``, ``n_written``, ``n_failed``, ``n_batches``, ``step``, ``precision``, ``target``."""
import argparse
import json
import pickle
import sys
from pathlib import Path

import numpy as np
import torch


def read_config(path):
    import yaml
    with open(path, "r") as f:
        return yaml.safe_load(f)


def unpickle(path):
    with open(str(path), "rb") as f:
        return pickle.load(f)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Duration extraction with a trained aligner (GPU).")
    ap.add_argument("--config", "-c", default="utils/aligner/aligner_train_config.yaml", type=str, help="Points to the config file.")
    ap.add_argument("--model", "-m", default=None, type=str, help="Points to the a model file to restore.")
    ap.add_argument("--target", "-t", default="outputs", type=str, help="Target path")
    ap.add_argument("--batch_size", "-b", default=8, type=int, help="Batch size for inference.")
    ap.add_argument("--num_workers", "-w", metavar="N", type=int, default=0, help="Accepted for compatibility; unused.")
    return ap.parse_args(argv)


def load_model(checkpoint: dict, device):
    from ..aligner import Aligner
    return Aligner.from_checkpoint(checkpoint).eval().to(device)


def plan_batches(n_items: int, batch_size: int):
    """Dataset order, ``batch_size`` items each."""
    return [list(range(i, min(i + batch_size, n_items))) for i in range(0, n_items, batch_size)]


def load_item(item, mel_dir: Path, token_dir: Path, n_mels: int):
    """-> (mel (mel_len, n_mels) float32, tokens (tokens_len,) int64) as extract_durations.py:30-33 and dataset.py:23-31 read them."""
    mel = np.load(str(mel_dir / f"{item['item_id']}.npy"), allow_pickle=False)
    tokens = np.load(str(token_dir / f"{item['item_id']}.npy"), allow_pickle=False).astype(np.int64)
    if mel.ndim != 2 or mel.shape[1] != n_mels:
        raise ValueError(f"mel of shape {mel.shape}, expected (frames, {n_mels})")
    mel_len, tokens_len = int(item["mel_len"]), int(item["tokens_len"])
    if not (1 <= mel_len <= mel.shape[0]) or not (1 <= tokens_len <= tokens.shape[0]):
        raise ValueError(f"mel_len {mel_len} / tokens_len {tokens_len} outside the stored arrays ({mel.shape[0]}, {tokens.shape[0]})")
    return mel.astype(np.float32), tokens[:tokens_len]


def open_corpus(config: dict, model_path, model_loader, device):
    """What the aligner's drivers read (extract_durations.py:60-84): the checkpoint (default
    ``<data_dir>/checkpoints/latest_model.pt``) with its symbols assertion, ``dataset.pkl``, and where the mels and tokens lie.
    -> (data_dir, model, dataset, n_mels, mel_dir, token_dir)"""
    data_dir = Path(config["paths"]["data_dir"])
    model_path = Path(model_path) if model_path else data_dir / "checkpoints" / "latest_model.pt"
    checkpoint = torch.load(model_path, map_location=torch.device("cpu"), weights_only=False)
    symbols = unpickle(data_dir / "symbols.pkl")
    assert symbols == checkpoint["symbols"], "Symbols from dataset do not match symbols from model checkpoint!"
    model = model_loader(checkpoint, device)
    dataset = unpickle(data_dir / "dataset.pkl")
    return data_dir, model, dataset, int(checkpoint["config"]["audio"]["n_mels"]), data_dir / "mels", data_dir / "tokens"


def load_batch(dataset, idx, mel_dir: Path, token_dir: Path, n_mels: int):
    """The loadable items of one batch, zero-padded to the batch's own longest mel and token row.  A failing item is reported and
    left out (extract_durations.py:43-45).  -> (items, mel (B, T, n_mels) fp32, tokens (B, N) int64, mel_len, tokens_len, n_failed),
    the tensors on the host; ``items`` is empty when nothing loaded."""
    rows, n_failed = [], 0
    for i in idx:
        try:
            rows.append((dataset[i],) + load_item(dataset[i], mel_dir, token_dir, n_mels))
        except Exception as e:
            print(f"Error processing {dataset[i].get('item_id')}: {e}", file=sys.stderr)
            n_failed += 1
    if not rows:
        return [], None, None, [], [], n_failed
    mel_len = [int(r[0]["mel_len"]) for r in rows]
    tokens_len = [int(r[2].shape[0]) for r in rows]
    mel = torch.zeros((len(rows), max(mel_len), n_mels), dtype=torch.float32)
    tokens = torch.zeros((len(rows), max(tokens_len)), dtype=torch.int64)
    for b, (_, m, t) in enumerate(rows):
        mel[b, :mel_len[b]] = torch.from_numpy(m[:mel_len[b]])
        tokens[b, :tokens_len[b]] = torch.from_numpy(t)
    return [r[0] for r in rows], mel, tokens, mel_len, tokens_len, n_failed


def run(args, model_loader=load_model, device=None) -> dict:
    config = read_config(args.config)
    method = config.get("durations", {}).get("method", "dijkstra")
    if method == "beam":
        raise SystemExit("align_durations: durations.method 'beam' is not covered (INTEGRATION.md); use 'dijkstra'")
    device = torch.device("cuda") if device is None else torch.device(device)
    target = Path(config["paths"]["data_dir"]) / args.target
    dur_dir, pred_dir = target / "durations", target / "predictions"
    dur_dir.mkdir(parents=True, exist_ok=True)
    pred_dir.mkdir(parents=True, exist_ok=True)
    data_dir, model, dataset, n_mels, mel_dir, token_dir = open_corpus(config, args.model, model_loader, device)
    batches = plan_batches(len(dataset), max(1, int(args.batch_size)))
    n_written = n_failed = 0
    for idx in batches:
        items, mel, tokens, mel_len, tokens_len, failed = load_batch(dataset, idx, mel_dir, token_dir, n_mels)
        n_failed += failed
        if not items:
            continue
        try:
            pred = model.predict(mel.to(device), mel_len)
        except Exception as e:
            print(f"Error processing {[it['item_id'] for it in items]}: {e}", file=sys.stderr)
            n_failed += len(items)
            continue
        try:
            dur = model.durations(pred, tokens.to(device), mel_len, tokens_len).cpu().numpy()
        except Exception:  # one bad item (a token outside the symbol table ...) fails the call: find it row by row, same pred
            dur = None
        pred_h = pred.cpu().numpy()
        for b, item in enumerate(items):
            try:
                np.save(pred_dir / f"{item['item_id']}.npy", pred_h[b, :mel_len[b]], allow_pickle=False)  # (kept when the durations fail, as the reference's)
                d_b = dur[b] if dur is not None else model.durations(pred[b:b + 1], tokens[b:b + 1].to(device), mel_len[b:b + 1],
                                                                     tokens_len[b:b + 1]).cpu().numpy()[0]
                np.save(dur_dir / f"{item['item_id']}.npy", d_b[:tokens_len[b]].astype(np.int32), allow_pickle=False)
                n_written += 1
            except Exception as e:
                print(f"Error processing {item['item_id']}: {e}", file=sys.stderr)
                n_failed += 1
    return {"n_items": len(dataset), "n_written": n_written, "n_failed": n_failed, "n_batches": len(batches), "step": int(model.get_step()),
            "precision": getattr(model, "precision_in_use", None), "target": str(target)}


def main(argv=None):
    print(json.dumps(run(parse_args(argv))))


if __name__ == "__main__":
    main()
