"""CPU restatement of the reference's teacher-forced ``Parrot.forward(batch)`` (modules/parrot.py:90-110 with inference=False)
and of ``ModelLoss`` (modules/loss.py:5-21), built from the oracle's blocks: the caller's durations expand the encoder output
(duration.py:6-24, every position counts) and the caller's tgt_mask is the decoder's key mask."""
import json
import os
from typing import Dict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import parrot_oracle as O
from parrot_tts_amd import synth

# tests/golden fixtures of the reference's teacher-forced Parrot(batch) + ModelLoss (tools/make_teacher_forced_goldens.py)
GOLDENS = {"tte_small_teacher_forced": synth.small_tte_config, "tte_full_teacher_forced": synth.default_tte_config}


def load_golden(golden_dir: str, name: str):
    """-> (npz, meta, cfg, state_dict (digest-checked, pe rows patched), the batch the reference ran)."""
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    m = json.loads(str(z["meta"]))
    cfg = GOLDENS[name]()
    sd = synth.synth_tte_state_dict(cfg, m["vocab"], m["n_spk"], seed=m["seed_w"])
    assert synth.state_digest(sd) == str(z["digest"]), "synthetic weights did not regenerate identically"
    synth.patch_pe_rows(sd, z["pe_idx"], z["pe_rows"])
    batch = {k: torch.from_numpy(z[k]) for k in ("phones", "src_mask", "speaker", "duration", "tgt_mask")}
    batch["codes"] = torch.from_numpy(z["codes"].astype(np.int64))
    return z, m, cfg, sd, batch


def row_alone(batch: dict, r: int) -> dict:
    """Row r as its own B = 1 teacher-forced batch: unpadded tokens, durations cut at its length, an all-True mask."""
    n = int(batch["src_mask"][r].sum())
    d = batch["duration"][r: r + 1, :n]
    return {"phones": batch["phones"][r: r + 1, :n], "src_mask": batch["src_mask"][r: r + 1, :n], "speaker": batch["speaker"][r: r + 1],
            "duration": d, "tgt_mask": torch.ones((1, int(d.sum())), dtype=torch.bool)}


def tte_forward_tf(sd: Dict[str, torch.Tensor], cfg: dict, batch: dict) -> dict:
    """-> dict(logits (B,L,V), log_dur (B,S), tgt_mask (the caller's), lens)."""
    tr = cfg["transformer"]
    ks = tr["conv_kernel_sizes"]
    src_kpm = ~batch["src_mask"]
    out = O.pos_emb(sd["pos_emb.pe"], F.embedding(batch["phones"], sd["tok_emb.weight"]))
    for n in range(tr["encoder"]["n_layer"]):
        out = O.fft_block(sd, f"encoder_layers.{n}.", out, tr["encoder"]["n_head"], ks, src_kpm)
    if "speaker_emb.weight" in sd:
        out = out + F.embedding(batch["speaker"], sd["speaker_emb.weight"]).unsqueeze(1)
    log_dur = O.duration_predictor(sd, out, src_kpm, cfg["duration_predictor"]["kernel_size"])
    dur, tgt_mask = batch["duration"], batch["tgt_mask"]
    assert tgt_mask.shape[1] == int(dur.sum(dim=1).max())  # duration.py:12
    out, _, lens = O.length_regulator(out, dur)
    out = O.pos_emb(sd["pos_emb.pe"], out)
    for n in range(tr["decoder"]["n_layer"]):
        out = O.fft_block(sd, f"decoder_layers.{n}.", out, tr["decoder"]["n_head"], ks, ~tgt_mask)
    logits = F.linear(out, sd["head.weight"], sd["head.bias"])
    return {"logits": logits, "log_dur": log_dur, "tgt_mask": tgt_mask, "lens": lens}


def model_loss(out, log_dur_preds, batch, num_codes: int):
    """modules/loss.py:12-21 in torch: (loss, code_loss, dur_loss)."""
    ld = log_dur_preds.masked_select(batch["src_mask"])
    lt = torch.log(batch["duration"].float() + 1).masked_select(batch["src_mask"])
    code_loss = F.cross_entropy(out.reshape(-1, num_codes), batch["codes"].reshape(-1), ignore_index=num_codes)
    dur_loss = F.mse_loss(ld, lt)
    return code_loss + dur_loss, code_loss, dur_loss
