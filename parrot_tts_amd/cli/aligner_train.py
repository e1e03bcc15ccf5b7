#!/usr/bin/env python3
"""Train the forced aligner on the GPU: the reference's utils/aligner/train.py with the loop of utils/aligner/trainer.py:28-88.

    python -m parrot_tts_amd.cli.aligner_train --config utils/aligner/aligner_train_config.yaml [--checkpoint CKPT] [--max_steps N]

It reads what ``align_durations`` reads (and through the same code): ``paths.data_dir`` of the config holds ``dataset.pkl``,
``symbols.pkl``, ``mels/ID.npy`` and ``tokens/ID.npy``.  It restores ``--checkpoint``, else ``<data_dir>/checkpoints/latest_model.pt``,
else initialises a ``TrainableAligner`` from ``audio.n_mels`` and ``model`` of the config with ``Adam(lr=1e-4)``; the learning rate
is then set from ``training.learning_rate``.  Batches follow the reference's ``BinnedLengthSampler`` (``bin_size = 3 x
batch_size``, seed 42; utils/aligner/dataset.py:38-60), zero-padded to their own longest row.  Every step is the reference's:

    pred = model(mel); pred = pred.transpose(0, 1).log_softmax(2); loss = ctc_loss(pred, tokens, mel_len, tokens_len)
    if the loss is finite: optim.zero_grad(); loss.backward(); clip_grad_norm_(model.parameters(), 1.0); optim.step()

with ``parrot_tts_amd.aligner.CTCLoss`` as the loss; Adam and the clipping are torch's.  A step whose loss is NaN / inf is skipped
and counted.  An item that cannot be loaded (a missing or malformed mel / token file) ends the run with an error, as the reference's
DataLoader does: the corpus never shrinks silently.  ``model_step_{k}k.pt`` is written every ``training.checkpoint_steps`` steps and ``latest_model.pt`` after every
epoch, both with the reference's keys (``model``, ``optim``, ``config``, ``symbols``), so ``align_durations`` / ``aligner_eval``
and the reference's own tools read them.  ``--max_steps N`` ends the run after N steps (``latest_model.pt`` is still written).

Left out: the TensorBoard scalars and the plot texts (trainer.py:73-75, 82-83, 90-116), and the progress bar.

Prints one JSON line per epoch: ``epoch``, ``step``, ``mean_loss`` (over the steps that were taken; null when there is none),
``n_skipped``."""
import argparse
import json
import math
from pathlib import Path
from random import Random

import numpy as np
import torch

from .align_durations import load_batch, read_config, unpickle


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Training of the aligner (GPU).")
    ap.add_argument("--config", "-c", default="utils/aligner/aligner_train_config.yaml", help="Points to the config file.")
    ap.add_argument("--checkpoint", "-cp", default=None, help="Points to the a model file to restore.")
    ap.add_argument("--max_steps", type=int, default=None, help="Stop after this many steps.")
    return ap.parse_args(argv)


class BinnedLengthOrder:
    """The index order of the reference's ``BinnedLengthSampler``: items sorted by length, shuffled inside bins of ``bin_size``, the
    bins shuffled, the remainder shuffled at the end.  As there, one ``Random(seed)`` lives as long as the sampler and every
    shuffle works on the sorted index array IN PLACE, so an epoch starts from what the epoch before left."""

    def __init__(self, mel_lens, batch_size: int, bin_size: int, seed: int = 42) -> None:
        assert bin_size % batch_size == 0
        self.idx = torch.sort(torch.tensor(mel_lens))[1].numpy()
        self.bin_size = bin_size
        self.random = Random(seed)

    def epoch(self):
        idx, n = self.idx, self.bin_size
        bins = []
        for i in range(len(idx) // n):
            part = idx[i * n:(i + 1) * n]  # (a view: the shuffle below reorders idx itself)
            self.random.shuffle(part)
            bins.append(part)
        self.random.shuffle(bins)
        order = np.stack(bins).reshape(-1) if bins else np.zeros((0,), dtype=idx.dtype)
        if len(order) < len(idx):
            tail = idx[len(order):]
            self.random.shuffle(tail)
            order = np.concatenate([order, tail])
        return [int(i) for i in order]


def checkpoint_dict(model, optim, config, symbols) -> dict:
    return {"model": model.state_dict(), "optim": optim.state_dict(), "config": config, "symbols": symbols}


def open_run(config: dict, checkpoint_path, device):
    """-> (model on ``device``, optimiser, symbols, checkpoint directory): train.py:24-45 and trainer.py:43-48."""
    from ..aligner import TrainableAligner
    data_dir = Path(config["paths"]["data_dir"])
    symbols = unpickle(data_dir / "symbols.pkl")
    ckpt_dir = data_dir / "checkpoints"
    ckpt_dir.mkdir(parents=True, exist_ok=True)
    path = Path(checkpoint_path) if checkpoint_path else ckpt_dir / "latest_model.pt"
    if checkpoint_path or path.exists():
        checkpoint = torch.load(path, map_location=torch.device("cpu"), weights_only=False)
        assert checkpoint["symbols"] == symbols, "Symbols from data do not match symbols from model!"
        model = TrainableAligner.from_checkpoint(checkpoint).to(device)
        optim = torch.optim.Adam(model.parameters())
        optim.load_state_dict(checkpoint["optim"])
    else:
        model = TrainableAligner(n_mels=config["audio"]["n_mels"], num_symbols=len(symbols) + 1, **config["model"]).to(device)
        optim = torch.optim.Adam(model.parameters(), lr=1e-4)
    for g in optim.param_groups:
        g["lr"] = config["training"]["learning_rate"]
    return model.train(), optim, symbols, ckpt_dir


def train_step(model, optim, ctc_loss, mel, tokens, mel_len, tokens_len):
    """trainer.py:60-71.  -> (loss as a float, whether the step was taken)"""
    pred = model(mel)
    pred = pred.transpose(0, 1).log_softmax(2)
    loss = ctc_loss(pred, tokens, mel_len, tokens_len)
    taken = bool(not torch.isnan(loss) and not torch.isinf(loss))
    if taken:
        optim.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        optim.step()
    return float(loss.detach()), taken


def run(args, device=None) -> list:
    from ..aligner import CTCLoss
    config = read_config(args.config)
    tp = config["training"]
    device = torch.device("cuda") if device is None else torch.device(device)
    model, optim, symbols, ckpt_dir = open_run(config, args.checkpoint, device)
    data_dir = Path(config["paths"]["data_dir"])
    dataset = unpickle(data_dir / "dataset.pkl")
    n_mels = int(config["audio"]["n_mels"])
    batch_size = int(tp["batch_size"])
    order = BinnedLengthOrder([d["mel_len"] for d in dataset], batch_size, 3 * batch_size)
    n_batches = max(1, math.ceil(len(dataset) / batch_size))
    ctc_loss = CTCLoss()
    report, n_steps = [], 0
    for epoch in range(model.get_step() // n_batches + 1, int(tp["epochs"]) + 1):
        idx = order.epoch()
        losses, n_skipped = [], 0
        for i in range(0, len(idx), batch_size):
            items, mel, tokens, mel_len, tokens_len, n_failed = load_batch(dataset, idx[i:i + batch_size], data_dir / "mels", data_dir / "tokens", n_mels)
            if n_failed:  # (load_batch has named each item on stderr; the reference's DataLoader raises here too)
                raise RuntimeError(f"aligner_train: {n_failed} item(s) of a batch could not be loaded; training on a silently smaller corpus is refused")
            loss, taken = train_step(model, optim, ctc_loss, mel.to(device), tokens.to(device), torch.tensor(mel_len, device=device),
                                     torch.tensor(tokens_len, device=device))
            if taken:
                losses.append(loss)
            else:
                n_skipped += 1
            n_steps += 1
            if model.get_step() % int(tp["checkpoint_steps"]) == 0:
                torch.save(checkpoint_dict(model, optim, config, symbols), ckpt_dir / f"model_step_{model.get_step() // 1000}k.pt")
            if args.max_steps is not None and n_steps >= args.max_steps:
                break
        torch.save(checkpoint_dict(model, optim, config, symbols), ckpt_dir / "latest_model.pt")
        line = {"epoch": epoch, "step": int(model.get_step()), "mean_loss": math.fsum(losses) / len(losses) if losses else None,
                "n_skipped": n_skipped}
        print(json.dumps(line), flush=True)
        report.append(line)
        if args.max_steps is not None and n_steps >= args.max_steps:
            break
    return report


def main(argv=None):
    run(parse_args(argv))


if __name__ == "__main__":
    main()
