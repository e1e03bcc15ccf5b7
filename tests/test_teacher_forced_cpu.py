"""CPU: the teacher-forced restatement (tests/teacher_forced_ref.py) against the oracle's inference forward, the restated
ModelLoss against torch's modules, and argument validation of the new entry points (before any HIP call)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from teacher_forced_ref import GOLDENS, load_golden, model_loss, row_alone, tte_forward_tf  # noqa: E402
from oracle import parrot_oracle as O  # noqa: E402
from parrot_tts_amd import synth  # noqa: E402


def _same(got, want, what):
    """Bit equality with the reference's golden -- or, on a host whose CPU makes torch pick another fp32 summation order than the
    golden's host did, agreement within that evaluation-order noise (the bound of tests/test_oracle_golden.py)."""
    got, want = np.asarray(got), np.asarray(want)
    if np.array_equal(got, want):
        return
    d = float(np.abs(got - want).max())
    assert d <= 2e-5 * max(1.0, float(np.abs(want).max())), f"{what}: differs from the golden by {d:.2e}"


@pytest.mark.parametrize("name", list(GOLDENS))
def test_restatement_matches_reference_teacher_forced_golden(golden_dir, name):
    """The reference's teacher-forced Parrot(batch) and ModelLoss on the golden's inputs: ragged rows, zero durations, a nonzero
    duration at a padded source position, a row whose codes are shorter than its sum of durations, codes padded with V."""
    z, m, cfg, sd, batch = load_golden(golden_dir, name)
    V = cfg["preprocess"]["hubert_codes"]
    with torch.no_grad():
        r = tte_forward_tf(sd, cfg, batch)
        loss = model_loss(r["logits"], r["log_dur"], batch, V)
    _same(r["log_dur"].numpy(), z["log_dur"], "log_dur")
    if "logits" in z.files:
        _same(r["logits"].numpy(), z["logits"], "logits")
    else:
        pos = z["logits_pos"]
        _same(r["logits"][pos[:, 0], pos[:, 1]].numpy(), z["logits_rows"], "logits rows")
    top = torch.topk(r["logits"], 2, dim=-1)
    sure = torch.from_numpy(z["margin"] > 1e-4)
    assert torch.equal(top.indices[..., 0][sure], torch.from_numpy(z["ids"].astype(np.int64))[sure])
    _same(np.array([float(v) for v in loss], dtype=np.float32), z["loss"], "loss triple")
    # row-exact: the B = 1 runs (the padded-duration row has none); the full golden: its first rows (CPU time)
    for row in [b for b in range(min(m["B"], 4)) if b != m["pad_row"]]:
        one = row_alone(batch, row)
        with torch.no_grad():
            lg = tte_forward_tf(sd, cfg, one)["logits"][0]
        Lr = lg.shape[0]
        sure = torch.from_numpy(z["re_margin"][row, :Lr] > 1e-4)
        assert torch.equal(torch.argmax(lg, -1)[sure], torch.from_numpy(z["re_ids"][row, :Lr].astype(np.int64))[sure]), row


@pytest.fixture(scope="module")
def lib():
    from parrot_tts_amd import build, _lib
    build.build()
    return _lib.lib()


def test_restatement_with_predicted_durations_is_the_inference_forward():
    """duration = the predicted durations, tgt_mask = t <= len (quirk Q2): the teacher-forced forward IS the inference one."""
    cfg = synth.small_tte_config()
    sd = synth.synth_tte_state_dict(cfg, 30, 2, seed=5)
    batch = synth.synth_tte_batch(3, 11, 30, 2, seed=3, ragged=True)
    with torch.no_grad():
        inf = O.tte_forward(sd, cfg, batch)
        tf = tte_forward_tf(sd, cfg, dict(batch, duration=inf["dur"], tgt_mask=inf["tgt_mask"]))
    assert torch.equal(tf["logits"], inf["logits"]) and torch.equal(tf["log_dur"], inf["log_dur"])
    with pytest.raises(AssertionError):  # duration.py:12
        tte_forward_tf(sd, cfg, dict(batch, duration=inf["dur"], tgt_mask=inf["tgt_mask"][:, :-1]))


def test_restated_loss_is_the_reference_modules():
    torch.manual_seed(1)
    V = 50
    out = torch.randn(2, 7, V)
    codes = torch.randint(0, V, (2, 7))
    codes[1, 4:] = V
    batch = {"codes": codes, "src_mask": torch.tensor([[1, 1, 1, 0], [1, 1, 0, 0]], dtype=torch.bool),
             "duration": torch.randint(0, 5, (2, 4))}
    ld = torch.randn(2, 4)
    got = model_loss(out, ld, batch, V)
    code = nn.CrossEntropyLoss(ignore_index=V)(out.reshape(-1, V), codes.reshape(-1))
    dur = nn.MSELoss()(ld.masked_select(batch["src_mask"]), torch.log(batch["duration"].float() + 1).masked_select(batch["src_mask"]))
    assert torch.equal(got[1], code) and torch.equal(got[2], dur) and torch.equal(got[0], code + dur)


def test_new_entry_points_reject_null_arguments(lib):
    buf = (C.c_char * 1024)()
    p = C.cast(buf, C.c_void_p)
    assert lib.parrot_tte_set_durations(None, p, 1, 1, None, p, p, 1024, None) == -1
    assert b"null" in lib.parrot_last_error()
    assert lib.parrot_tte_decode_masked(None, 1, 1, 1, 0, p, p, None, p, 1024, p, 1024, None) == -1
    assert b"null" in lib.parrot_last_error()
    assert lib.parrot_tte_loss(None, p, 1, 4, 4, p, p, p, 1, p, None, p, 1024, None) == -1
    assert b"null" in lib.parrot_last_error()
    assert lib.parrot_tte_loss(p, p, 0, 4, 4, p, p, p, 1, p, None, p, 1024, None) == -1  # empty logits
    assert lib.parrot_tte_loss_workspace_bytes(-1) == 0 and lib.parrot_tte_loss_workspace_bytes(16384) > 0
