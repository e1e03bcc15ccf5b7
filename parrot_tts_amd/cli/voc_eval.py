#!/usr/bin/env python3
"""Validation metric of a vocoder checkpoint: the reference's ``validation/mel_spec_error`` (utils/vocoder/train.py:198-227) over
a unit manifest, on the GPU.

    python -m parrot_tts_amd.cli.voc_eval --checkpoint_file CKPT_OR_DIR --config utils/vocoder/config.json \
        --input_code_file runs/vocoder/val.txt [--batch_rows 64 --batch_units 16384] [--per_item]

For every manifest item whose ground-truth wav exists: the ground truth is peak-normalised x 0.95 and trimmed to whole units
(``CodeDataset``, dataset.py:212-223), the units are vocoded under the item's own speaker, both waveforms go through
``mel_spectrogram`` with ``h.fmax_for_loss`` (``null`` = sampling_rate / 2) and the item's error is the mean absolute difference
of the two log-mels (``F.l1_loss``, train.py:213).  Items are vocoded as the length-bucketed padded batches of ``voc_infer``
with per-row lengths through every stage -- generator, both mels, the L1 -- so a row's value is that utterance's own,
whatever batch it rides in.

Prints one JSON line: ``mel_spec_error`` (the mean of the per-utterance errors), ``n_utterances``, ``n_skipped_no_audio`` (items
without a ground-truth wav: nothing to compare against), ``precision`` (of the mel; the generator's is what PARROT_PRECISION
selects -- the point of the metric is to compare such modes), and with --per_item ``items``: {name: error}.

``mel_spec_error`` equals the reference's validation loop run with ``batch_size 1`` and ``segment_size -1`` (whole utterances).
The reference's DEFAULT validates something else: its validation set is built with ``h.segment_size`` (8 960 samples) and
``split=True``, i.e. one RANDOM 8 960-sample segment per utterance (train.py:88-92, dataset.py:182-202, 226-235), so its logged
number moves from run to run and is not reproduced here."""
import argparse
import json
from pathlib import Path

import numpy as np
import torch

from .. import dist as pdist
from ..checkpoint import load_generator
from ..data import VOCODER_SPEAKERS, parse_speaker
from ..mel import MelSpectrogram, mel_l1
from ..vocoder import AttrDict
from .voc_infer import build_dataset, plan_batches


def collect_rows(dataset, h, n=-1):
    """-> (rows, n_skipped): rows = [(units int64 array, speaker id or None, ground truth (n,) float32 tensor, name)] for the
    items whose ground-truth wav exists (and that hold at least one whole unit of it)."""
    multi = bool(h.get("multispkr"))
    rows, skipped = [], 0
    for item in range(len(dataset) if n < 0 else min(n, len(dataset))):
        feats, gt_audio, filename, _ = dataset[item]
        code = np.asarray(feats["code"], dtype=np.int64).reshape(-1)
        if gt_audio is None or code.size == 0:
            skipped += 1
            continue
        spk = VOCODER_SPEAKERS[parse_speaker(filename, h["multispkr"])] if multi else None
        rows.append((code, spk, gt_audio.reshape(-1).to(torch.float32), Path(filename).stem))
    return rows, skipped


def evaluate(gen, mel, rows, dev, max_rows=64, max_units=16384):
    """Per-row mel errors (fp64 numpy, in the order of ``rows``) of ``gen`` -- any callable with the shim generator's surface:
    ``gen(code=, spkr=, unit_lens=) -> (B, 1, samples)``, ``out_samples(units)``, ``multispkr`` -- under the mel ``mel``."""
    errs = np.full(len(rows), np.nan, dtype=np.float64)
    lengths = [int(r[0].size) for r in rows]
    # the reference's F.pad raises on such an utterance (dataset.py:55) in the middle of its loop: say which one before any batch runs
    short = [r[3] for r, n in zip(rows, lengths) if min(int(gen.out_samples(n)), r[2].numel()) <= mel.pad]
    if short:
        raise ValueError(f"voc_eval: {len(short)} utterance(s) no longer than the mel's reflect pad ({mel.pad} samples): {short[:8]}")
    multi = bool(gen.multispkr)
    for idx in plan_batches(lengths, max_rows, max_units):
        lens = [lengths[i] for i in idx]
        U = max(lens)
        n_samples = [int(gen.out_samples(n)) for n in lens]
        code_h = torch.zeros((len(idx), U), dtype=torch.int64)
        gt_h = torch.zeros((len(idx), int(gen.out_samples(U))), dtype=torch.float32)
        for r, i in enumerate(idx):
            code_h[r, : lens[r]] = torch.from_numpy(rows[i][0])
            n = min(n_samples[r], rows[i][2].numel())  # (the ground truth holds lens[r] * code_hop_size samples)
            n_samples[r] = n
            gt_h[r, :n] = rows[i][2][:n]
        spk = torch.tensor([[rows[i][1]] for i in idx], device=dev) if multi else None
        wav = gen(code=code_h.to(dev), spkr=spk, unit_lens=torch.tensor(lens, dtype=torch.int32, device=dev))
        ns = torch.tensor(n_samples, dtype=torch.int32, device=dev)
        mel_hat = mel(wav[:, 0], ns, check=False)
        mel_gt = mel(gt_h.to(dev), ns, check=False)
        _, row_means = mel_l1(mel_gt, mel_hat, ns // mel.hop_size)
        errs[np.asarray(idx)] = row_means.cpu().numpy()
        mel.check(dev)  # (the stream is idle after the copy: a row shorter than the reflect pad / a non-finite mel fails here)
    return errs


def summarise(errs, names, n_skipped, precision, per_item=False) -> dict:
    res = {"mel_spec_error": float(np.mean(errs)) if len(errs) else float("nan"), "n_utterances": int(len(errs)),
           "n_skipped_no_audio": int(n_skipped), "precision": precision}
    if per_item:
        res["items"] = {n: float(e) for n, e in zip(names, errs)}
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--input_code_file", default="runs/vocoder/val.txt")
    ap.add_argument("--checkpoint_file", required=True)
    ap.add_argument("--config", default="utils/vocoder/config.json")
    ap.add_argument("--pad", default=None, type=int)
    ap.add_argument("-n", type=int, default=-1, help="number of items (default: all)")
    ap.add_argument("--batch_rows", type=int, default=64, help="rows per vocoder batch")
    ap.add_argument("--batch_units", type=int, default=16384, help="padded units (rows x longest row) per vocoder batch")
    ap.add_argument("--per_item", action="store_true", help="add the per-utterance errors to the JSON line")
    a = ap.parse_args(argv)
    a.code_file = None  # (a 'name|units' list carries no audio path: nothing to validate against)
    _, _, local = pdist.init_from_env()
    dev = pdist.local_device(local)
    with open(a.config) as f:
        h = AttrDict(json.load(f))
    gen = load_generator(h, a.checkpoint_file, dev)
    mel = MelSpectrogram(h)
    rows, skipped = collect_rows(build_dataset(a, h), h, a.n)
    errs = evaluate(gen, mel, rows, dev, a.batch_rows, a.batch_units)
    gen.check_inputs()
    res = summarise(errs, [r[3] for r in rows], skipped, mel.precision_in_use(dev), a.per_item)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
