"""GPU: the teacher-forced TTE forward (reference modules/parrot.py:90-110 with inference=False: the caller's durations and
target mask), ``infer(durations=...)``, the HIP ``ModelLoss`` (modules/loss.py) and the consumers built on them
(LitParrot.validation_step, SynthesisPipeline, tte_eval, tte_infer --teacher_forced)."""
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from teacher_forced_ref import GOLDENS, load_golden, model_loss, tte_forward_tf  # noqa: E402
from parrot_tts_amd import checkpoint, data, ops, synth  # noqa: E402
from parrot_tts_amd.loss import ModelLoss  # noqa: E402
from parrot_tts_amd.pipeline import SynthesisPipeline  # noqa: E402
from parrot_tts_amd.tte import Parrot  # noqa: E402
from parrot_tts_amd.vocoder import AttrDict, CodeGenerator  # noqa: E402

DEV = "cuda:0"
VOCAB, NSPK = 30, 2


@pytest.fixture(params=["f32", "bf16x6", "f16x3"])
def prec(request):
    ops.set_default_precision(ops.PREC_NAMES[request.param])
    yield request.param
    ops.set_default_precision(ops.PREC_DEFAULT)


def _parrot(cfg, sd, tmp_path, n_spk=NSPK, vocab=VOCAB):
    cfg = synth.clone_config(cfg)
    cfg["path"]["root_path"] = str(tmp_path)
    with open(os.path.join(str(tmp_path), "speakers.json"), "w") as f:
        json.dump({f"s{i}": i for i in range(n_spk)}, f)
    m = Parrot(cfg, vocab, 0)
    m.load_state_dict(sd)
    return m.eval().to(DEV)


V_SMALL = synth.small_tte_config()["preprocess"]["hubert_codes"]


def _tf_batch(seed=3):
    """Ragged batch; durations with zeros and a nonzero one at a padded source position (row 1); row 2's codes are shorter
    than its sum of durations (its mask is not the sum prefix); codes padded with V like collate does."""
    b = synth.synth_tte_batch(3, 11, VOCAB, NSPK, seed=seed, ragged=True)
    g = torch.Generator().manual_seed(seed)
    dur = torch.randint(0, 4, b["phones"].shape, generator=g) * b["src_mask"]
    dur[:, 0] = 2
    pad_pos = (~b["src_mask"][1]).nonzero()
    assert len(pad_pos), "row 1 must be padded"
    dur[1, int(pad_pos[0])] = 3
    sums = dur.sum(1)
    L = int(sums.max())
    code_len = sums.clone()
    code_len[2] = max(1, int(sums[2]) - 3)
    V = V_SMALL
    codes = torch.full((3, L), V, dtype=torch.int64)
    for r in range(3):
        codes[r, : code_len[r]] = torch.randint(0, V, (int(code_len[r]),), generator=g)
    b.update(duration=dur, codes=codes, tgt_mask=codes != V)
    return b


def _margin(logits):
    top = torch.topk(logits, 2, dim=-1).values
    return top[..., 0] - top[..., 1]


@pytest.mark.parametrize("name", list(GOLDENS))
def test_teacher_forced_matches_reference_golden(golden_dir, tmp_path, name, prec):
    """model(batch) against the reference's teacher-forced Parrot(batch) + ModelLoss (tests/golden), and row-exact
    infer(durations=...) against each row's own B = 1 reference run."""
    z, m, cfg, sd, batch = load_golden(golden_dir, name)
    model = _parrot(cfg, sd, tmp_path, n_spk=m["n_spk"], vocab=m["vocab"])
    gpu = {k: v.to(DEV) for k, v in batch.items()}
    logits, _, tgt_mask, log_dur = model(gpu)
    assert tgt_mask is gpu["tgt_mask"]
    lg = logits.cpu()
    msk = batch["tgt_mask"]
    if "logits" in z.files:
        assert float((lg[msk] - torch.from_numpy(z["logits"])[msk]).abs().max()) <= 1e-4
    else:
        pos = torch.from_numpy(z["logits_pos"])
        assert float((lg[pos[:, 0], pos[:, 1]] - torch.from_numpy(z["logits_rows"])).abs().max()) <= 1e-4
    sm = batch["src_mask"]
    assert float((log_dur.cpu()[sm] - torch.from_numpy(z["log_dur"])[sm]).abs().max()) <= 2e-5
    sure = msk & torch.from_numpy(z["margin"] > 1e-4)
    assert torch.equal(torch.argmax(lg, -1)[sure], torch.from_numpy(z["ids"].astype(np.int64))[sure])
    got = ModelLoss(cfg)(logits, log_dur, gpu)  # the full path: HIP logits -> HIP loss
    for a, g in zip(got, z["loss"]):
        assert abs(float(a) - float(g)) <= 2e-4 * max(1.0, abs(float(g)))
    # row-exact: the padded-duration row has no row-alone reading (its duration there is dropped here, and left out)
    dur = batch["duration"] * batch["src_mask"]
    rows = model.infer(gpu, row_exact=True, durations=dur.to(DEV))
    for r in range(m["B"]):
        if r == m["pad_row"]:
            continue
        Lr = int(dur[r].sum())
        assert len(rows[r]) == Lr
        sure = torch.from_numpy(z["re_margin"][r, :Lr] > 1e-4)
        assert torch.equal(torch.tensor(rows[r])[sure], torch.from_numpy(z["re_ids"][r, :Lr].astype(np.int64))[sure]), r


def test_teacher_forced_forward_matches_restatement(tmp_path, prec):
    cfg = synth.small_tte_config()
    sd = synth.synth_tte_state_dict(cfg, VOCAB, NSPK, seed=5)
    model = _parrot(cfg, sd, tmp_path)
    batch = _tf_batch()
    with torch.no_grad():
        ref = tte_forward_tf(sd, cfg, batch)
    gpu = {k: v.to(DEV) for k, v in batch.items()}
    logits, src_mask, tgt_mask, log_dur = model(gpu)
    assert tgt_mask is gpu["tgt_mask"] and src_mask is gpu["src_mask"]
    m = batch["tgt_mask"]
    lg = logits.cpu()
    assert lg.shape == ref["logits"].shape
    assert float((lg[m] - ref["logits"][m]).abs().max()) <= 1e-4
    sm = batch["src_mask"]
    assert float((log_dur.cpu()[sm] - ref["log_dur"][sm]).abs().max()) <= 2e-5
    ids = torch.argmax(lg, -1)
    want = torch.argmax(ref["logits"], -1)
    sure = m & (_margin(ref["logits"]) > 1e-4)
    assert torch.equal(ids[sure], want[sure])
    # the loss on these logits: within 2e-4 of the restated reference's loss on its own logits
    got = ModelLoss(cfg)(logits, log_dur, gpu)
    with torch.no_grad():
        exp = model_loss(ref["logits"], ref["log_dur"], batch, V_SMALL)
    for a, b in zip(got, exp):
        assert abs(float(a) - float(b)) <= 2e-4 * max(1.0, abs(float(b)))


def test_row_exact_infer_with_durations_matches_single_rows(tmp_path, prec):
    cfg = synth.small_tte_config()
    sd = synth.synth_tte_state_dict(cfg, VOCAB, NSPK, seed=5)
    model = _parrot(cfg, sd, tmp_path)
    batch = _tf_batch()
    batch["duration"][1] *= batch["src_mask"][1]  # (a nonzero duration at a padded position has no row-alone reading)
    gpu = {k: v.to(DEV) for k, v in batch.items()}
    rows = model.infer(gpu, row_exact=True, durations=gpu["duration"])
    for r in range(3):
        n = int(batch["src_mask"][r].sum())
        d = batch["duration"][r: r + 1, :n]
        L = int(d.sum())
        one = {"phones": batch["phones"][r: r + 1, :n], "src_mask": batch["src_mask"][r: r + 1, :n], "speaker": batch["speaker"][r: r + 1],
               "duration": d, "tgt_mask": torch.ones((1, L), dtype=torch.bool)}
        with torch.no_grad():
            ref = tte_forward_tf(sd, cfg, one)
        want = torch.argmax(ref["logits"][0], -1)
        got = torch.tensor(rows[r])
        assert got.shape == (L,)
        sure = _margin(ref["logits"][0]) > 1e-4
        assert torch.equal(got[sure], want[sure]), r


def _bitwise_vs_inference(model, batch):
    gpu = {k: v.to(DEV) for k, v in batch.items()}
    lg_i, _, mask_i, ld_i = model(gpu, inference=True)
    dur = model.infer_dense(gpu)["dur"]  # the predicted durations
    tf = dict(gpu, duration=dur, tgt_mask=mask_i.clone())
    lg_t, _, mask_t, ld_t = model(tf)
    assert mask_t is tf["tgt_mask"]
    assert torch.equal(lg_t, lg_i) and torch.equal(ld_t, ld_i)


def test_teacher_forced_equals_inference_bit_for_bit_small(tmp_path, prec):
    cfg = synth.small_tte_config()
    sd = synth.synth_tte_state_dict(cfg, VOCAB, NSPK, seed=8)
    _bitwise_vs_inference(_parrot(cfg, sd, tmp_path), synth.synth_tte_batch(4, 13, VOCAB, NSPK, seed=4, ragged=True))


def test_teacher_forced_equals_inference_bit_for_bit_full_size(tmp_path, prec):
    cfg = synth.default_tte_config()
    sd = synth.synth_tte_state_dict(cfg, VOCAB, NSPK, seed=9, forced_duration=4)
    batch = synth.synth_tte_batch(64, 64, VOCAB, NSPK, seed=6)
    model = _parrot(cfg, sd, tmp_path)
    gpu = {k: v.to(DEV) for k, v in batch.items()}
    assert model(gpu, inference=True)[0].shape[1] == 256
    _bitwise_vs_inference(model, batch)


def test_infer_with_durations_emits_sum_ids_equal_to_forward_argmax(tmp_path, prec):
    cfg = synth.small_tte_config()
    sd = synth.synth_tte_state_dict(cfg, VOCAB, NSPK, seed=5)
    model = _parrot(cfg, sd, tmp_path)
    batch = _tf_batch(seed=11)
    gpu = {k: v.to(DEV) for k, v in batch.items()}
    before = model.infer(gpu)  # a batch's own `duration` entry is never used implicitly
    assert before == model.infer({k: v for k, v in gpu.items() if k not in ("duration", "codes", "tgt_mask")})
    rows = model.infer(gpu, durations=gpu["duration"])
    sums = batch["duration"].sum(1)
    L = int(sums.max())
    prefix = torch.arange(L)[None, :] < sums[:, None]
    logits = model(dict(gpu, tgt_mask=prefix.to(DEV)))[0].cpu()
    for r in range(3):
        assert len(rows[r]) == int(sums[r])
        want = torch.argmax(logits[r, : int(sums[r])], -1)
        sure = _margin(logits[r, : int(sums[r])]) > 1e-4
        assert torch.equal(torch.tensor(rows[r])[sure], want[sure])
    dense = model.infer_dense(gpu, durations=gpu["duration"])
    assert torch.equal(dense["tgt_mask"].cpu(), prefix)


def test_model_loss_matches_torch_formula_and_repeats_bitwise():
    torch.manual_seed(0)
    B, L, S, V = 5, 37, 9, 1000
    cfg = {"preprocess": {"hubert_codes": V}}
    out = (torch.randn(B, L, V) * 3).to(DEV)
    codes = torch.randint(0, V, (B, L))
    codes[:, 30:] = V
    codes[1, 5:] = V
    batch = {"codes": codes.to(DEV), "src_mask": (torch.arange(S)[None, :] < torch.tensor([9, 4, 7, 1, 8])[:, None]).to(DEV),
             "duration": torch.randint(0, 6, (B, S)).to(DEV)}
    log_dur = torch.randn(B, S).to(DEV)
    loss = ModelLoss(cfg)
    got = loss(out, log_dur, batch)
    again = loss(out, log_dur, batch)
    want = model_loss(out, log_dur, batch, V)
    for a, a2, w in zip(got, again, want):
        assert a.dim() == 0 and a.dtype == torch.float32 and a.device.type == "cuda"
        assert torch.equal(a, a2)
        assert abs(float(a) - float(w)) <= 1e-5 * abs(float(w))
    valid = codes != V
    acc = (torch.argmax(out.cpu(), -1) == codes)[valid].sum()
    assert loss.last_stats["n_valid"] == int(valid.sum()) and loss.last_stats["n_correct"] == int(acc)
    # odd vocabulary (the kernel's generic path) and the NaN edge cases of torch
    V2 = 37
    o2 = torch.randn(3, 4, V2).to(DEV)
    c2 = torch.randint(0, V2, (3, 4)).to(DEV)
    b2 = dict(batch, codes=c2, src_mask=batch["src_mask"][:3, :4], duration=batch["duration"][:3, :4])
    g2 = ModelLoss({"preprocess": {"hubert_codes": V2}})(o2, log_dur[:3, :4], b2)
    w2 = model_loss(o2, log_dur[:3, :4], b2, V2)
    assert all(abs(float(a) - float(w)) <= 1e-5 * abs(float(w)) for a, w in zip(g2, w2))
    ign = loss(out, log_dur, dict(batch, codes=torch.full_like(batch["codes"], V), src_mask=torch.zeros_like(batch["src_mask"])))
    assert all(bool(torch.isnan(v)) for v in ign)


def test_teacher_forced_errors(tmp_path):
    cfg = synth.small_tte_config()
    sd = synth.synth_tte_state_dict(cfg, VOCAB, NSPK, seed=5)
    model = _parrot(cfg, sd, tmp_path)
    gpu = {k: v.to(DEV) for k, v in _tf_batch().items()}
    neg = gpu["duration"].clone()
    neg[0, 1] = -1
    with pytest.raises(RuntimeError, match="repeats can not be negative"):
        model(dict(gpu, duration=neg))
    with pytest.raises(AssertionError):  # duration.py:12
        model(dict(gpu, tgt_mask=gpu["tgt_mask"][:, :-1]))
    big = gpu["duration"].clone()
    big[0, 0] = cfg["transformer"]["max_len"] + 100  # (one duration alone beyond max_len: the width check still sees the true sum)
    with pytest.raises(IndexError):  # pe[T] out of range, fft.py:18
        model(dict(gpu, duration=big, tgt_mask=torch.ones((3, int(big.sum(1).max())), dtype=torch.bool, device=DEV)))
    with pytest.raises(AssertionError):  # parrot.py:92
        model({k: v for k, v in gpu.items() if k != "duration"})
    empty = gpu["tgt_mask"].clone()
    empty[1] = False
    with pytest.raises(ValueError):
        model(dict(gpu, tgt_mask=empty))
    logits, _, _, log_dur = model(gpu)
    bad = gpu["codes"].clone()
    bad[2, 0] = V_SMALL + 5
    with pytest.raises(IndexError, match=f"Target {V_SMALL + 5} is out of bounds"):
        ModelLoss(cfg)(logits, log_dur, dict(gpu, codes=bad))
    with pytest.raises(ValueError, match="Expected input batch_size"):
        ModelLoss(cfg)(logits, log_dur, dict(gpu, codes=gpu["codes"][:, :-1]))
    model.train()
    with pytest.raises(NotImplementedError):
        model(gpu)
    model.eval()
    assert model.infer(gpu, durations=gpu["duration"])  # the handle is usable after every error


def test_c_side_check_reports_bad_durations(tmp_path):
    """parrot_tte_check itself -- the shim decodes the status word in Python (_raise_status) and never gets there: status 6 and 7 of
    parrot_tte_set_durations come back as PARROT_E_INVALID with the library's own messages, and reporting clears the flag."""
    from parrot_tts_amd import _lib
    from parrot_tts_amd.ops import dptr, stream_ptr
    cfg = synth.small_tte_config()
    model = _parrot(cfg, synth.synth_tte_state_dict(cfg, VOCAB, NSPK, seed=5), tmp_path)
    gpu = {k: v.to(DEV) for k, v in _tf_batch().items()}
    model(gpu)  # (builds the handle)
    lib, h, st = _lib.lib(), model._handle, stream_ptr(torch.device(DEV))
    B, S = gpu["duration"].shape
    state = torch.empty(lib.parrot_tte_state_bytes(h, B, S), dtype=torch.uint8, device=DEV)
    out_lens = torch.empty(B, dtype=torch.int32, device=DEV)
    assert lib.parrot_tte_check(h, st) == 0
    neg = gpu["duration"].clone()
    neg[0, 1] = -1
    assert lib.parrot_tte_set_durations(h, dptr(neg), B, S, None, dptr(out_lens), dptr(state), state.numel(), st) == 0
    assert lib.parrot_tte_check(h, st) == -1  # PARROT_E_INVALID
    assert b"tte: repeats can not be negative (a negative duration, duration.py:14)" in lib.parrot_last_error()
    assert lib.parrot_tte_check(h, st) == 0
    src_len = gpu["src_mask"].sum(1).to(torch.int32)  # (_tf_batch: row 1 has a nonzero duration at a padded position)
    assert lib.parrot_tte_set_durations(h, dptr(gpu["duration"]), B, S, dptr(src_len), dptr(out_lens), dptr(state), state.numel(), st) == 0
    assert lib.parrot_tte_check(h, st) == -1
    assert b"tte: row-exact durations: a nonzero duration at a padded source position" in lib.parrot_last_error()
    assert lib.parrot_tte_check(h, st) == 0


def test_pipeline_with_durations_vocodes_the_emitted_ids(tmp_path):
    cfg, h = synth.small_tte_config(), synth.small_voc_config()
    sd = synth.synth_tte_state_dict(cfg, VOCAB, NSPK, seed=5)
    gen = CodeGenerator(AttrDict(h))
    gen.load_state_dict(synth.synth_voc_state_dict(h, seed=2))
    gen = gen.eval().to(DEV)
    pipe = SynthesisPipeline(_parrot(cfg, sd, tmp_path), gen)
    gpu = {k: v.to(DEV) for k, v in _tf_batch().items()}
    out = pipe(gpu, durations=gpu["duration"])
    sums = gpu["duration"].sum(1)
    assert torch.equal(out["n_samples"].cpu(), gen.out_samples(sums.cpu()))
    spkr = gpu["speaker"].reshape(-1, 1) if gen.multispkr else None
    with torch.no_grad():
        ref = gen(code=out["ids"], spkr=spkr, unit_lens=sums.to(torch.int32))
    for r in range(3):
        n = int(out["n_samples"][r])
        assert torch.equal(out["wav"][r, :, :n], ref[r, :, :n]), r


def _dataset(tmp_path):
    root = tmp_path / "tte"
    root.mkdir()
    (root / "speakers.json").write_text(json.dumps({"bho_f": 0, "en_m": 1}))
    symbols = ["a", " ", "b", "c", "d"]
    with open(root / "symbols.pkl", "wb") as f:
        pickle.dump(symbols, f)
    cfg = synth.small_tte_config(str(root))
    cfg["path"]["alignment_path"] = str(root)
    cfg["path"]["wav_path"] = str(tmp_path / "audio")
    recs = [{"audio": "/x/bho_f_001.wav", "speaker": "bho_f", "characters": "a sil b c", "hubert": "1 2 3 4 5 6", "duration": "1 2 0 3"},
            {"audio": "/x/en_m_002.wav", "speaker": "en_m", "characters": "d a", "hubert": "7 8 9", "duration": "1 2"},
            {"audio": "/x/bho_f_003.wav", "speaker": "bho_f", "characters": "c c sil a b d", "hubert": "3 3 4 99 0",
             "duration": "1 1 0 1 1 1"}]
    (root / "val.txt").write_text("".join(data.format_dict_line(r) for r in recs))
    vocab = len(symbols) + 2
    sd = synth.synth_tte_state_dict(cfg, vocab, 2, seed=17)
    ck = tmp_path / "parrot.ckpt"
    checkpoint.save_lightning_style(ck, sd, cfg, vocab, 0)
    ycfg = tmp_path / "cfg.yaml"
    ycfg.write_text(yaml.safe_dump(cfg))
    return root, cfg, ck, ycfg, recs


def test_tte_eval_reports_validation_step_losses(tmp_path, capsys):
    from parrot_tts_amd.cli import tte_eval
    root, cfg, ck, ycfg, recs = _dataset(tmp_path)
    res = tte_eval.main(["--config", str(ycfg), "--checkpoint_pth", str(ck), "--device", DEV, "--batch_size", "2"])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == res
    assert res["n_utterances"] == 3 and 0.0 <= res["unit_accuracy"] <= 1.0
    model = checkpoint.LitParrot.load_from_checkpoint(ck).to(DEV).eval()
    ds = data.ParrotDataset("val", cfg)
    want = {"val_total_loss": 0.0, "val_code_loss": 0.0, "val_dur_loss": 0.0}
    for s, idx in enumerate(([0, 1], [2])):
        batch = ds.collate_fn([ds[i] for i in idx])
        gpu = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
        total = model.validation_step(gpu, s)
        assert torch.equal(total, model.logged["val_total_loss"])
        for k in want:
            want[k] += float(model.logged[k]) * len(idx)
    for k in want:
        assert res[k] == pytest.approx(want[k] / 3, rel=1e-6)


def test_tte_infer_teacher_forced_writes_sum_durations_ids(tmp_path):
    from parrot_tts_amd.cli import tte_infer
    root, cfg, ck, ycfg, recs = _dataset(tmp_path)
    for extra in ([], ["--row_exact", "--batch_size", "3"]):
        tte_infer.main(["--config", str(ycfg), "--checkpoint_pth", str(ck), "--device", DEV, "--teacher_forced"] + extra)
        lines = (root / "predictions.txt").read_text().splitlines()
        assert len(lines) == 3
        for line, rec in zip(lines, recs):
            n = sum(int(v) for v in rec["duration"].split(" "))
            assert len(data.parse_dict_line(line)["hubert"].split(" ")) == n
