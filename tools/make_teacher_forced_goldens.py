#!/usr/bin/env python3
"""Generate tests/golden/tte_{small,full}_teacher_forced.npz by running the REFERENCE's teacher-forced forward
(modules/parrot.py:90-110: ``Parrot(batch)`` with inference=False, eval mode, no_grad) and its ``ModelLoss``
(modules/loss.py:5-21), imported at run time from a reference checkout (CPU fp32), on seeded synthetic checkpoints.

Nothing from the reference is copied: the fixtures hold plain input / output arrays plus a sha256 digest of the synthetic
state_dict, so that tests can prove they regenerated the same weights.  Inputs: a ragged batch, durations with zeros, a nonzero
duration at a padded source position (row ``pad_row``), one row whose codes are shorter than its sum of durations (row
``short_row``: its mask is not the sum prefix), codes padded with V.  Outputs: log_dur, top-1 ids, top-2 margins and some logits
rows of the padded batch, the ModelLoss triple, and -- for the row-exact mode -- each row's own B = 1 teacher-forced run (its
unpadded tokens, its durations cut at its length, a mask of width sum(dur) that is all True; ``pad_row`` left out).

Also cross-checks the CPU restatement (tests/teacher_forced_ref.py) against the reference while it is at hand.

    python tools/make_teacher_forced_goldens.py [--reference DIR]
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from parrot_tts_amd import synth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
torch.set_num_threads(8)


def tf_batch(B, S, vocab, n_spk, V, seed, max_dur, full_row_dur=None):
    """The teacher-forced inputs (see the module docstring); ``full_row_dur``: row 0 (unpadded) gets that duration everywhere,
    which pins L = S * full_row_dur."""
    b = synth.synth_tte_batch(B, S, vocab, n_spk, seed=seed, ragged=True)
    g = torch.Generator().manual_seed(seed + 1000)
    real = b["src_mask"]
    dur = torch.randint(0, max_dur + 1, (B, S), generator=g) * real
    dur[:, 0] = dur[:, 0].clamp(min=1)  # every row expands to something: no all-masked row
    if full_row_dur is not None:
        assert bool(real[0].all())
        dur[0] = full_row_dur
    pad_row = next(r for r in range(1, B) if not bool(real[r].all()))
    dur[pad_row, int((~real[pad_row]).nonzero()[0])] = 2
    sums = dur.sum(1)
    short_row = next(r for r in range(1, B) if r != pad_row and int(sums[r]) > 3)
    L = int(sums.max())
    code_len = sums.clone()
    code_len[short_row] = int(sums[short_row]) - 3
    codes = torch.full((B, L), V, dtype=torch.int64)
    for r in range(B):
        codes[r, : int(code_len[r])] = torch.randint(0, V, (int(code_len[r]),), generator=g)
    b.update(duration=dur, codes=codes, tgt_mask=codes != V)
    return b, pad_row, short_row


def top2(logits):
    v, i = torch.topk(logits, 2, dim=-1)
    return i[..., 0], v[..., 0] - v[..., 1]


def maxdiff(a, b):
    return float((a.double() - b.double()).abs().max()) if a.numel() else 0.0


def case(name, cfg, vocab, n_spk, B, S, seed_w, seed_in, max_dur, RefParrot, RefModelLoss, full_row_dur=None, logits_rows=None):
    from teacher_forced_ref import model_loss, tte_forward_tf

    V = cfg["preprocess"]["hubert_codes"]
    sd = synth.synth_tte_state_dict(cfg, vocab, n_spk, seed=seed_w)
    batch, pad_row, short_row = tf_batch(B, S, vocab, n_spk, V, seed_in, max_dur, full_row_dur)
    tmp = tempfile.mkdtemp()
    with open(os.path.join(tmp, "speakers.json"), "w") as f:
        json.dump({f"spk{i}": i for i in range(n_spk)}, f)
    rcfg = synth.clone_config(cfg)
    rcfg["path"]["root_path"] = tmp
    model = RefParrot(rcfg, vocab, 0)
    res = model.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    model.eval()
    with torch.no_grad():
        logits, _, tgt_mask, log_dur = model(batch)  # inference=False: teacher forced
        loss = RefModelLoss(rcfg)(logits, log_dur, batch)
        mine = tte_forward_tf(sd, cfg, batch)
        mine_loss = model_loss(mine["logits"], mine["log_dur"], batch, V)
    assert tgt_mask is batch["tgt_mask"]
    L = logits.shape[1]
    ids, margin = top2(logits)
    print(f"[{name}] B={B} S={S} L={L} restatement-vs-ref: logits {maxdiff(mine['logits'], logits):.3g} log_dur "
          f"{maxdiff(mine['log_dur'], log_dur):.3g} loss {[maxdiff(a, b) for a, b in zip(mine_loss, loss)]}")
    # row-exact: every row as its own B = 1 teacher-forced run (pad_row has no such reading)
    re_ids = np.full((B, L), -1, dtype=np.int16)
    re_margin = np.full((B, L), np.nan, dtype=np.float32)
    pe_idx = {S, L}
    re_diff = 0.0
    for r in range(B):
        if r == pad_row:
            continue
        n = int(batch["src_mask"][r].sum())
        d = batch["duration"][r: r + 1, :n]
        Lr = int(d.sum())
        one = {"phones": batch["phones"][r: r + 1, :n], "src_mask": batch["src_mask"][r: r + 1, :n],
               "speaker": batch["speaker"][r: r + 1], "duration": d, "tgt_mask": torch.ones((1, Lr), dtype=torch.bool)}
        with torch.no_grad():
            lg1 = model(one)[0][0]
            if r < 4:
                re_diff = max(re_diff, maxdiff(tte_forward_tf(sd, cfg, one)["logits"][0], lg1))
        i1, m1 = top2(lg1)
        re_ids[r, :Lr] = i1.numpy()
        re_margin[r, :Lr] = m1.numpy()
        pe_idx |= {n, Lr}
    print(f"[{name}] row-exact runs: restatement-vs-ref logits {re_diff:.3g} (rows 0-3)")
    pe_idx = np.array(sorted(pe_idx))
    extra = {}
    if logits_rows is None:
        extra["logits"] = logits.numpy()
    else:  # a few (b, t) positions of the full logits
        pos = np.array(logits_rows, dtype=np.int64)
        extra["logits_pos"] = pos
        extra["logits_rows"] = logits[pos[:, 0], pos[:, 1]].numpy()
    np.savez_compressed(
        os.path.join(GOLD, name + ".npz"),
        digest=np.array(synth.state_digest(sd)),
        meta=np.array(json.dumps(dict(vocab=vocab, n_spk=n_spk, B=B, S=S, seed_w=seed_w, seed_in=seed_in, max_dur=max_dur,
                                      full_row_dur=full_row_dur, pad_row=pad_row, short_row=short_row))),
        phones=batch["phones"].numpy(), src_mask=batch["src_mask"].numpy(), speaker=batch["speaker"].numpy(),
        duration=batch["duration"].numpy(), codes=batch["codes"].numpy().astype(np.int16), tgt_mask=batch["tgt_mask"].numpy(),
        log_dur=log_dur.numpy(), ids=ids.numpy().astype(np.int16), margin=margin.numpy(),
        loss=np.array([float(v) for v in loss], dtype=np.float32),
        re_ids=re_ids, re_margin=re_margin,
        pe_idx=pe_idx, pe_rows=sd["pos_emb.pe"][torch.from_numpy(pe_idx)].numpy(),
        **extra,
    )
    print(f"[{name}] wrote {os.path.getsize(os.path.join(GOLD, name + '.npz'))} bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("PARROT_REFERENCE", "/root/reference"),
                    help="checkout of the reference repository (its modules/ package is imported, never copied)")
    a = ap.parse_args()
    sys.path.insert(1, a.reference)
    from modules.loss import ModelLoss as RefModelLoss  # noqa: E402
    from modules.parrot import Parrot as RefParrot  # noqa: E402

    # small model, 3 ragged rows; full logits kept
    case("tte_small_teacher_forced", synth.small_tte_config(), vocab=30, n_spk=2, B=3, S=11, seed_w=5, seed_in=3, max_dur=3,
         RefParrot=RefParrot, RefModelLoss=RefModelLoss)
    # full model at the bench shape: B = 64 x S = 64, row 0 pins L = 256; a few logits rows kept
    case("tte_full_teacher_forced", synth.default_tte_config(), vocab=60, n_spk=2, B=64, S=64, seed_w=0, seed_in=1, max_dur=4,
         RefParrot=RefParrot, RefModelLoss=RefModelLoss, full_row_dur=4,
         logits_rows=[(0, 0), (0, 255), (1, 7), (5, 100), (17, 3), (33, 200), (63, 1), (63, 150)])


if __name__ == "__main__":
    main()
