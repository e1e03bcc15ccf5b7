"""CPU: the oracle (oracle/parrot_oracle.py) must reproduce, BIT-EXACTLY, the vectors captured from
the reference implementation by tools/make_goldens.py (tests/golden/*.npz), after regenerating
the same seeded synthetic checkpoints (digest-checked)."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import parrot_oracle as O
from parrot_tts_amd import synth

torch.set_num_threads(8)


def _load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    meta = json.loads(str(z["meta"])) if "meta" in z.files else {}
    return z, meta


TTE_CASES = {
    "tte_full_ragged": synth.default_tte_config,
    "tte_full_forced": synth.default_tte_config,
    "tte_small_ragged": synth.small_tte_config,
    "tte_small_multi": synth.small_tte_config,
}


@pytest.mark.parametrize("name", list(TTE_CASES))
def test_tte_oracle_matches_reference(golden_dir, name):
    z, m = _load(golden_dir, name)
    cfg = TTE_CASES[name]()
    sd = synth.synth_tte_state_dict(cfg, m["vocab"], m["n_spk"], seed=m["seed_w"], forced_duration=m["forced"], gain=m["gain"])
    assert synth.state_digest(sd) == str(z["digest"]), "synthetic weights did not regenerate identically"
    synth.patch_pe_rows(sd, z["pe_idx"], z["pe_rows"])
    batch = {"phones": torch.from_numpy(z["phones"]), "src_mask": torch.from_numpy(z["src_mask"]),
             "speaker": torch.from_numpy(z["speaker"])}
    gen = synth.synth_tte_batch(m["B"], m["S"], m["vocab"], m["n_spk"], seed=m["seed_in"], ragged=m["ragged"])
    assert torch.equal(gen["phones"], batch["phones"])
    with torch.no_grad():
        r = O.tte_forward(sd, cfg, batch)
        ids_ragged = O.tte_infer(sd, cfg, batch)
    assert np.array_equal(r["log_dur"].numpy(), z["log_dur"])
    assert np.array_equal(r["dur"].numpy(), z["dur"])
    assert np.array_equal(r["tgt_mask"].numpy(), z["tgt_mask"])
    assert np.array_equal(torch.argmax(r["logits"], -1).numpy(), z["ids"])
    n = z["logits_head"].shape[0]
    assert np.array_equal(r["logits"][:n].numpy(), z["logits_head"])
    for b, row in enumerate(ids_ragged):
        ln = int(z["ids_ragged_len"][b])
        assert row == z["ids_ragged"][b, :ln].tolist()
    # quirk Q2: every row emits len+1 ids except rows of maximal length
    L = r["logits"].shape[1]
    for b, row in enumerate(ids_ragged):
        assert len(row) == min(r["lens"][b] + 1, L)


def test_tte_blocks(golden_dir):
    z, _ = _load(golden_dir, "tte_blocks")
    cfg = synth.default_tte_config()
    sd = synth.synth_tte_state_dict(cfg, 50, 2, seed=7)
    assert synth.state_digest(sd) == str(z["digest"])
    x, kpm = torch.from_numpy(z["x"]), torch.from_numpy(z["kpm"])
    with torch.no_grad():
        y = O.fft_block(sd, "decoder_layers.1.", x, 2, [9, 1], kpm)
        ld = O.duration_predictor(sd, x, kpm, 3)
        ex, tm, _ = O.length_regulator(torch.from_numpy(z["lr_seq"]), torch.from_numpy(z["lr_dur"]))
    assert np.array_equal(y.numpy(), z["fft_out"])
    assert np.array_equal(ld.numpy(), z["log_dur"])
    assert np.array_equal(ex.numpy(), z["lr_out"])
    assert np.array_equal(tm.numpy(), z["lr_mask"])


def _voc_cfg(name):
    if name.startswith("voc_full"):
        return synth.default_voc_config()
    if name == "voc_small_corners":  # odd k - u upsampling stages (T u + 1 samples), dilation lists of unequal length
        return synth.corner_voc_config()
    h = synth.small_voc_config()
    if name == "voc_small_singlespk":
        h["multispkr"] = None
        h["model_in_dim"] = h["embedding_dim"]
    if name == "voc_small_resblock2":
        h["resblock"] = "2"
        h["resblock_dilation_sizes"] = [[1, 3], [1, 3], [1, 3]]
    return h


def _equal_or_within_evaluation_order_noise(y, name, golden_wav):
    """Bit equality with the committed golden -- or, on a host whose CPU makes torch pick another fp32 summation order than the
    golden's host did (conv blocking follows the cache sizes / vector ISA: the same reference code then differs from its own
    golden by a few 1e-6, as it does between thread counts), the golden within that evaluation-order noise; the caller then
    holds the int16 waveform and every stage to the same noise."""
    if np.array_equal(y, golden_wav):
        return "golden"
    d = float(np.abs(y - golden_wav).max())
    assert d <= 2e-5, f"{name}: oracle differs from the golden by {d:.2e}: more than fp32 evaluation-order noise"
    print(f"{name}: this host evaluates the fp32 convs in another order than the golden's host (max diff {d:.1e})")
    return "noise"


VOC_CASES = ["voc_full_stages", "voc_full_u40", "voc_full_u40_hot", "voc_small", "voc_small_singlespk",
             "voc_small_resblock2", "voc_full_u256", "voc_small_corners"]


@pytest.mark.parametrize("name", VOC_CASES)
def test_vocoder_oracle_matches_reference(golden_dir, name):
    z, m = _load(golden_dir, name)
    h = _voc_cfg(name)
    sd = synth.synth_voc_state_dict(h, seed=m["seed_w"], scale=m["scale"])
    assert synth.state_digest(sd) == str(z["digest"])
    code, spkr = torch.from_numpy(z["code"]), torch.from_numpy(z["spkr"])
    st = {}
    with torch.no_grad():
        y = O.code_generator_forward(sd, h, code, spkr, stages=st)
        y_folded = O.code_generator_forward(O.fold_weight_norm(sd), h, code, spkr)
    n_out = m["U"]
    for u, k in zip(h["upsample_rates"], h["upsample_kernel_sizes"]):
        n_out = (n_out - 1) * u - 2 * ((k - u) // 2) + k  # ConvTranspose1d (models.py:80-83): T u, + 1 for odd k - u
    assert y.shape == (m["B"], 1, n_out)
    pinned_by = _equal_or_within_evaluation_order_noise(y.numpy(), name, z["wav"])
    assert np.array_equal(y_folded.numpy(), y.numpy()), "weight_g/weight_v and folded checkpoints must agree"
    if pinned_by == "golden":
        assert np.array_equal(O.to_int16(y.squeeze(1)), z["wav_int16"])
    else:  # (another summation order moves samples by a few 1e-6: at most one int16 step at a rounding boundary)
        assert int(np.abs(O.to_int16(y.squeeze(1)).astype(np.int32) - z["wav_int16"].astype(np.int32)).max()) <= 1
    for k in z.files:
        if k.startswith("stage_"):
            if pinned_by == "golden":
                assert np.array_equal(st[k[6:]].numpy(), z[k]), k
            else:  # (a host that sums the fp32 convs in another order than the golden's: the same evaluation-order noise per stage)
                assert float(np.abs(st[k[6:]].numpy() - z[k]).max()) <= 2e-5 * max(1.0, float(np.abs(z[k]).max())), k
    if "wav_fp64" in z.files:  # the reference's own fp32 round-off at realistic scale
        assert np.abs(z["wav"] - z["wav_fp64"]).max() < 5e-5


def test_vocoder_extra_conditioning_streams_match_reference(golden_dir):
    """CodeGenerator.forward with extra keyword tensors (models.py:162-167): oracle == reference golden, bit for bit."""
    z = np.load(os.path.join(golden_dir, "voc_small_feats.npz"))
    m = json.loads(str(z["meta"]))
    h = synth.clone_config(synth.small_voc_config())
    h["model_in_dim"] += m["extra_channels"]
    sd = synth.synth_voc_state_dict(h, seed=m["seed_w"])
    assert synth.state_digest(sd) == str(z["digest"])
    feats = {"f0": torch.from_numpy(z["f0"]), "energy": torch.from_numpy(z["energy"]), "style": torch.from_numpy(z["style"])}
    with torch.no_grad():
        y = O.code_generator_forward(sd, h, torch.from_numpy(z["code"]), torch.from_numpy(z["spkr"]), feats=feats)
    assert np.array_equal(y.numpy(), z["wav"])
    with pytest.raises(NotImplementedError):  # 20 = 2 * 7 + 6: the remainder check of models.py:146-148 fires
        O.upsample_condition(torch.zeros(2, 1, 7), 20)
    with pytest.raises(RuntimeError):         # 20 = 6 * 3 + 2: passes that check and fails in .view(), as the reference does
        O.upsample_condition(torch.zeros(2, 1, 3), 20)


def test_reference_logits_depend_on_its_own_thread_count():
    """What "bit-exact unit ids" can mean.  The reference's fp32 logits (restated bit-for-bit by the oracle) move by ~1e-5 when
    nothing but the number of CPU threads changes (BLAS blocking -> another fp32 summation order; the residual stream is ~10, so
    one ulp is ~1e-6 and eight blocks of them add up).  An id whose top-2 margin is below that noise is not determined by the
    reference itself; the HIP path is therefore required to match every id with a margin above 1e-4 (tests/test_gpu_*.py) and
    reports how many positions fall below (Parrot.guard_stats)."""
    cfg = synth.default_tte_config()
    vocab, n_spk = 300, 10
    sd = synth.synth_tte_state_dict(cfg, vocab, n_spk, seed=42, forced_duration=4)
    batch = synth.synth_tte_batch(4, 64, vocab, n_spk, seed=0)
    n0 = torch.get_num_threads()
    try:
        outs = []
        for nt in (1, 4):
            torch.set_num_threads(nt)
            with torch.no_grad():
                outs.append(O.tte_forward(sd, cfg, batch)["logits"])
    finally:
        torch.set_num_threads(n0)
    d = float((outs[0] - outs[1]).abs().max())
    print(f"reference logits, 1 vs 4 CPU threads: max |diff| = {d:.3e}")  # (recorded: 1.2e-5 on the build container)
    # the upper bound is the claim (thread noise stays far below the 1e-4 margin the HIP path is held to); a host with one
    # usable core, or a BLAS that blocks identically for both thread counts, legitimately shows d == 0
    assert 0.0 <= d < 1e-4, d
    import bench
    if bench.cpu_quota() >= 4 and d == 0.0:
        pytest.skip("this host's BLAS gives identical sums for 1 and 4 threads: nothing to record")
