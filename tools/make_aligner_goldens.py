#!/usr/bin/env python3
"""Generate tests/golden/aligner_*.npz and align_dp.npz by running the REFERENCE's aligner (utils/aligner/model.py,
utils/aligner/duration_extraction.py), imported at run time from a reference checkout, on CPU in fp32.

Nothing from the reference is copied: a fixture holds the inputs (mel, tokens, lengths; the weights as a seed and a digest of
``parrot_tts_amd.synth.synth_aligner_state_dict``), the reference's fp32 outputs, the same formula evaluated in fp64 (the reference
module itself in ``.double()``), and in its meta, per stage, ``d_ref = max |ref_fp32 - ref_fp64|``: the reference's own distance from
the exact value, the unit of the GPU parity bound (4 x d_ref).  Per row it also stores
  unique: no exact tie between the two smallest predecessor distances at any cell of the fp64 DP's path
  stable: the reference's durations are unchanged for pred taken from the fp64 logits and under 16 seeded perturbations of
          +-4 d_ref(pred).
Cross-checks while the reference is at hand: tests/aligner_ref.py in fp64 against the reference in fp64 (1e-12), the fp64 DP's cost
against scipy's Dijkstra distance bit for bit, its durations against the reference's on every unique row.

    python tools/make_aligner_goldens.py [--reference DIR]
"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import aligner_ref as R  # noqa: E402
from parrot_tts_amd import synth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
MAX_BYTES = 1752383  # the largest golden already there


def load_reference(ref_dir):
    mods = []
    for name in ("model", "duration_extraction"):
        spec = importlib.util.spec_from_file_location("ref_aligner_" + name, os.path.join(ref_dir, "utils", "aligner", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mods.append(mod)
    return mods


def scipy_cost(ref_dx, tokens, pred):
    from scipy.sparse.csgraph import dijkstra
    w = np.float32(1.0) - pred[:, tokens]
    assert w.dtype == np.float32
    if w.size == 1:
        return 0.0
    dist = dijkstra(csgraph=ref_dx.to_adj_matrix(w), directed=True, indices=0)
    return float(dist[-1])


def dp_row(ref_dx, tokens, pred):
    """-> reference durations, fp64 DP cost (== scipy's, asserted), unique flag, DP durations."""
    dur_ref = ref_dx.extract_durations_with_dijkstra(tokens, pred).astype(np.int32) if pred[:, tokens].size > 1 else np.array([pred.shape[0]], np.int32)
    dur_dp, cost, unique = R.dp_durations(tokens, pred, with_info=True)
    sc = scipy_cost(ref_dx, tokens, pred)
    assert np.float64(cost).tobytes() == np.float64(sc).tobytes(), (cost, sc)
    assert int(dur_ref.sum()) == pred.shape[0] and int(dur_dp.sum()) == pred.shape[0]
    if unique:
        assert np.array_equal(dur_ref, dur_dp), (dur_ref, dur_dp)
    pc = R.path_cost(dur_ref, tokens, pred)
    assert abs(pc - cost) <= (pred.shape[0] + len(tokens)) * 2.0 ** -53 * cost, (pc, cost)
    return dur_ref, cost, unique, dur_dp


def tokens_for(rng, V, n, repeats=False):
    t = rng.integers(1, V, size=n)
    if not repeats:
        for j in range(1, n):
            while t[j] == t[j - 1]:
                t[j] = rng.integers(1, V)
    return t.astype(np.int64)


def model_fixture(name, ref_model, ref_dx, cfg, V, mel_len, tokens_len, seed, gain, stages=(), lstm_channels=None, with_dp=True, alone=None):
    B, T = len(mel_len), max(mel_len)
    sd = synth.synth_aligner_state_dict(cfg, V, seed=seed, gain=gain)
    n_mels = cfg["audio"]["n_mels"]
    mel = synth.synth_aligner_mel(B, T, n_mels, mel_len, seed=seed + 1)
    m = ref_model.Aligner(n_mels=n_mels, num_symbols=V, **cfg["model"])
    m.load_state_dict(sd)
    m.eval()
    taps = {}
    m.convs[2].register_forward_hook(lambda mod, i, o: taps.__setitem__("bn3", o.detach().clone()))
    m.rnn.register_forward_hook(lambda mod, i, o: taps.__setitem__("lstm", o[0].detach().clone()))
    with torch.no_grad():
        logits = m(mel)
        t32 = dict(taps)
        logits_alone = m(mel[alone:alone + 1, :mel_len[alone]])[0] if alone is not None else None
        m64 = m.double()
        logits64 = m64(mel.double())
        t64 = dict(taps)
        alone64 = m64(mel[alone:alone + 1, :mel_len[alone]].double())[0] if alone is not None else None
        # the restatement, while the reference is at hand
        r64, rs64 = R.aligner_forward(sd, mel.double())
        assert float((r64 - logits64).abs().max()) <= 1e-12, float((r64 - logits64).abs().max())
        for k in ("bn3", "lstm"):
            assert float((rs64[k] - t64[k]).abs().max()) <= 1e-12
    pred = R.softmax_rows(logits, mel_len)
    pred64 = R.softmax_rows(logits64, mel_len)
    out = {"mel": mel.numpy(), "mel_len": np.array(mel_len, np.int32), "logits": logits.numpy(), "logits64": logits64.numpy()}
    d_ref = {"logits": float((logits.double() - logits64).abs().max())}
    meta = {"n_mels": n_mels, "num_symbols": V, "lstm_dim": cfg["model"]["lstm_dim"], "conv_dim": cfg["model"]["conv_dim"], "seed": seed,
            "gain": gain, "digest": synth.state_digest(sd), "logit_max": float(logits.max())}
    if with_dp:
        out["pred"], out["pred64"] = pred.numpy(), pred64.numpy()
        d_ref["pred"] = float((pred.double() - pred64).abs().max())
    for k in stages:
        a32, a64 = t32[k], t64[k]
        if k == "lstm" and lstm_channels is not None:
            a32, a64 = a32[..., lstm_channels], a64[..., lstm_channels]
            out["lstm_channels"] = np.array(lstm_channels, np.int32)
        out[k], out[k + "64"] = a32.numpy(), a64.numpy()
        d_ref[k] = float((a32.double() - a64).abs().max())
    if alone is not None:
        out["logits_alone"], out["logits_alone64"] = logits_alone.numpy(), alone64.numpy()
        d_ref["logits_alone"] = float((logits_alone.double() - alone64).abs().max())
        meta["alone_row"] = alone
        meta["alone_gap"] = float((logits[alone, :mel_len[alone]] - logits_alone).abs().max())
    if with_dp:
        rng = np.random.Generator(np.random.PCG64(seed + 2))
        N = max(tokens_len)
        tokens = np.zeros((B, N), np.int64)
        durs = np.zeros((B, N), np.int32)
        costs, uniq, stab = [], [], []
        pn, pn64 = pred.numpy(), pred64.numpy()
        for b in range(B):
            tk = tokens_for(rng, V, tokens_len[b])
            tokens[b, :tokens_len[b]] = tk
            p = pn[b, :mel_len[b]]
            dur_ref, cost, unique, _ = dp_row(ref_dx, tk, p)
            durs[b, :tokens_len[b]] = dur_ref
            costs.append(cost)
            uniq.append(unique)
            ok = np.array_equal(ref_dx.extract_durations_with_dijkstra(tk, pn64[b, :mel_len[b]].astype(np.float32)), dur_ref)
            prng = np.random.Generator(np.random.PCG64(1000 + b))
            for _ in range(16):
                q = (p.astype(np.float64) + prng.uniform(-1, 1, size=p.shape) * 4 * d_ref["pred"]).clip(0, 1).astype(np.float32)
                ok = ok and np.array_equal(ref_dx.extract_durations_with_dijkstra(tk, q), dur_ref)
            stab.append(bool(ok))
        out.update(tokens=tokens, tokens_len=np.array(tokens_len, np.int32), durations=durs, cost=np.array(costs, np.float64))
        meta.update(unique=uniq, stable=stab)
        assert any(u and s for u, s in zip(uniq, stab)), (name, uniq, stab)
    meta["d_ref"] = d_ref
    save(name, out, meta)


def save(name, out, meta):
    path = os.path.join(GOLD, name + ".npz")
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **out)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    print(name, size, "bytes", json.dumps(meta))


def planted_pred(rng, T, N, V, tokens, boost, saturate=False):
    """pred (T, V) fp32 around a planted monotonic alignment: frame i belongs to token a(i)."""
    cuts = np.sort(rng.choice(np.arange(1, T), size=min(N, T) - 1, replace=False)) if min(N, T) > 1 else np.array([], int)
    a = np.searchsorted(cuts, np.arange(T), side="right")
    if N > T:  # more tokens than frames: some tokens are passed by right moves
        a = np.sort(rng.choice(np.arange(N), size=T, replace=False))
        a[-1] = N - 1
    logits = rng.standard_normal(size=(T, V))
    logits[np.arange(T), tokens[a]] += boost
    if saturate:  # p == 1.0f on the planted token, w == 1.0f everywhere else; a few frames belong to symbol 0, which no token
        logits[np.arange(T), tokens[a]] += 40.0  # carries (silence): their whole row costs exactly 1, whichever neighbour takes them
        for i in range(5, T - 1, 9):
            logits[i, 0] += 90.0
    x = torch.from_numpy(logits.astype(np.float32))
    return torch.softmax(x, dim=-1).numpy()


def dp_fixture(ref_dx):
    V = 40
    cases = [("t150n30", 150, 30, 5.0, False, False, 11), ("t64n64", 64, 64, 5.0, False, False, 12), ("t23n30", 23, 30, 5.0, False, False, 13),
             ("t97n33_repeats", 97, 33, 5.0, True, False, 14), ("t40n12_saturated", 40, 12, 5.0, False, True, 15), ("t17n1", 17, 1, 5.0, False, False, 16)]
    out, meta = {}, {"cases": [], "V": V, "unique": {}, "tied": {}}
    for name, T, N, boost, repeats, saturate, seed in cases:
        rng = np.random.Generator(np.random.PCG64(seed))
        tokens = tokens_for(rng, V, N)
        if repeats:  # doubled letters: identical adjacent columns, exact ties
            for j in range(2, N, 3):
                tokens[j] = tokens[j - 1]
        pred = planted_pred(rng, T, N, V, tokens, boost, saturate)
        dur_ref, cost, unique, dur_dp = dp_row(ref_dx, tokens, pred)
        if repeats or saturate:
            assert not unique, name + ": meant to be tied"
        elif N > 1:
            assert unique, name + ": meant to be tie-free"
        out[name + "_tokens"], out[name + "_pred"], out[name + "_durations"] = tokens, pred, dur_ref
        out[name + "_cost"] = np.array(cost, np.float64)
        meta["cases"].append(name)
        meta["unique"][name] = unique
        meta["tied"][name] = bool(repeats or saturate)
    save("align_dp", out, meta)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("PARROT_REFERENCE", "/root/reference"))
    ap.add_argument("--gain", type=float, default=14.0)  # logit max 14 - 20: a peaky softmax that does not saturate
    args = ap.parse_args()
    torch.manual_seed(0)
    ref_model, ref_dx = load_reference(args.reference)
    small, full = synth.small_aligner_config(), synth.default_aligner_config()
    dp_fixture(ref_dx)
    model_fixture("aligner_small", ref_model, ref_dx, small, 21, [60, 41, 23], [12, 9, 30], seed=7, gain=args.gain, stages=("bn3", "lstm"), alone=2)
    H = full["model"]["lstm_dim"]
    chans = sorted(set(range(0, 2 * H, 2 * H // 64)))
    model_fixture("aligner_full", ref_model, ref_dx, full, 61, [48, 29], [10, 7], seed=8, gain=args.gain, stages=("lstm",), lstm_channels=chans)
    model_fixture("aligner_small_long", ref_model, ref_dx, small, 21, [601, 350], None, seed=9, gain=args.gain, with_dp=False)


if __name__ == "__main__":
    main()
