"""Synthetic configs, checkpoints and inputs in the reference's exact on-disk layouts.

No reference checkpoint is available offline (demo.ipynb cell 4 downloads them), so every
golden vector, parity test and bench run uses seeded synthetic weights laid out exactly like
the reference's ``state_dict``s:

* TTE  : keys of ``Parrot.state_dict()``            (reference modules/parrot.py:13-65)
* vocoder: keys of ``CodeGenerator.state_dict()`` with weight-norm attached
           (``weight_g``/``weight_v``; reference utils/vocoder/models.py:69-130)
* aligner: keys of ``Aligner.state_dict()``          (reference utils/aligner/model.py:24-40)

Weights come from ``numpy.random.Generator(PCG64(seed))`` so they regenerate bit-identically
on the GPU box (same image, same numpy); ``state_digest`` lets tests prove that.
"""
from __future__ import annotations

import copy
import hashlib
import math
from typing import Dict, Optional

import numpy as np
import torch


# --------------------------------------------------------------------------------------
# configs (same keys/values as utils/TTE/TTE_config.yaml and utils/vocoder/config.json)
# --------------------------------------------------------------------------------------
def default_tte_config(root_path: str = "runs/TTE") -> dict:
    """Model-relevant part of utils/TTE/TTE_config.yaml:1-30."""
    return {
        "path": {"root_path": root_path, "alignment_path": "runs/aligner"},
        "preprocess": {"val_size": 100, "hubert_codes": 1000, "speaker": "_"},
        "transformer": {
            "encoder": {"n_layer": 4, "n_head": 2, "dropout_p": 0.1},
            "decoder": {"n_layer": 4, "n_head": 2, "dropout_p": 0.1},
            "d_model": 256,
            "conv_n_filter": 1024,
            "conv_kernel_sizes": [9, 1],
            "max_len": 3500,
        },
        "duration_predictor": {"n_filter": 256, "kernel_size": 3, "dropout_p": 0.5},
    }


def default_voc_config() -> dict:
    """Model-relevant part of utils/vocoder/config.json:5-32."""
    return {
        "resblock": "1",
        "seed": 1234,
        "upsample_rates": [5, 4, 4, 2, 2],
        "upsample_kernel_sizes": [11, 8, 8, 4, 4],
        "upsample_initial_channel": 512,
        "resblock_kernel_sizes": [3, 7, 11],
        "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5], [1, 3, 5]],
        "num_embeddings": 1000,
        "embedding_dim": 128,
        "model_in_dim": 256,
        "code_hop_size": 320,
        "multispkr": "_",
        "sampling_rate": 16000,
    }


def small_tte_config(root_path: str = "runs/TTE") -> dict:
    """A reduced TTE (same graph, smaller dims) for fast CPU goldens / smoke tests."""
    cfg = default_tte_config(root_path)
    cfg["transformer"].update(d_model=64, conv_n_filter=128, max_len=400)
    cfg["transformer"]["encoder"]["n_layer"] = 2
    cfg["transformer"]["decoder"]["n_layer"] = 2
    cfg["duration_predictor"]["n_filter"] = 64
    cfg["preprocess"]["hubert_codes"] = 100
    return cfg


def small_voc_config() -> dict:
    """A reduced generator (same graph: 5 stages, 3x3 MRF) for fast CPU goldens / smoke tests."""
    h = default_voc_config()
    h.update(upsample_initial_channel=64, embedding_dim=16, model_in_dim=32, num_embeddings=100)
    return h


def corner_voc_config() -> dict:
    """Config corners the reference accepts: odd ``upsample_kernel_size - upsample_rate`` (ConvTranspose1d then
    yields T u + 1 samples, reference utils/vocoder/models.py:80-83) and dilation lists of different lengths per kernel size
    (ResBlock1 reads the first three entries only, models.py:17-22).  Golden: tests/golden/voc_small_corners.npz."""
    h = small_voc_config()
    h["upsample_rates"], h["upsample_kernel_sizes"] = [4, 2, 2], [9, 4, 5]       # k - u = 5, 2, 3: two odd stages
    h["resblock_dilation_sizes"] = [[1, 2, 3], [1, 3, 5, 7], [2, 1, 4, 9, 11]]    # entries beyond the third are never read
    return h


# --------------------------------------------------------------------------------------
# helpers
# --------------------------------------------------------------------------------------
def _rng(seed: int) -> np.random.Generator:
    return np.random.Generator(np.random.PCG64(seed))


def _normal(rng, shape, std):
    # .clone(): torch-owned (64-byte aligned) storage, like nn.Parameter copies in the reference --
    # CPU BLAS picks alignment-dependent code paths, so this keeps oracle == reference bit-exact.
    return torch.from_numpy((rng.standard_normal(size=shape) * std).astype(np.float32)).clone()


def sinusoid_table(max_len: int, d_model: int) -> torch.Tensor:
    """The (max_len, d_model) buffer ``pos_emb.pe`` (reference modules/fft.py:21-38).

    Real checkpoints carry this buffer in their state_dict; synthetic ones rebuild it with
    the same formula (sin on even columns, cos on odd, 10000^(-2i/d))."""
    pe = torch.zeros(max_len, d_model)
    position = torch.arange(0, max_len).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d_model, 2, dtype=torch.float) * -(math.log(10000.0) / d_model))
    pe[:, 0::2] = torch.sin(position.float() * div_term)
    pe[:, 1::2] = torch.cos(position.float() * div_term)
    return pe


def patch_pe_rows(sd: Dict[str, torch.Tensor], idx, rows) -> None:
    """Overwrite rows ``idx`` of ``pos_emb.pe`` with the exact values a golden run used (only rows S and L
    are ever read: reference quirk Q1)."""
    for i, r in zip(idx, rows):
        sd["pos_emb.pe"][int(i)] = torch.as_tensor(r)


def state_digest(sd: Dict[str, torch.Tensor]) -> str:
    """sha256 over (key, shape, raw bytes) of every tensor, in sorted key order.

    ``pos_emb.pe`` is skipped: it is rebuilt with torch.sin/cos/exp, whose last bit depends on the
    host CPU's vector ISA; goldens carry the two rows they used instead (``patch_pe_rows``)."""
    hsh = hashlib.sha256()
    for k in sorted(sd):
        if k == "pos_emb.pe":
            continue
        t = sd[k].detach().cpu().contiguous()
        hsh.update(k.encode())
        hsh.update(str(tuple(t.shape)).encode())
        hsh.update(t.numpy().tobytes())
    return hsh.hexdigest()


# --------------------------------------------------------------------------------------
# TTE
# --------------------------------------------------------------------------------------
def synth_tte_state_dict(cfg: dict, src_vocab_size: int, n_speaker: int, seed: int = 42,
                         forced_duration: Optional[int] = None, gain: float = 1.0) -> Dict[str, torch.Tensor]:
    """Seeded weights with the key set of ``Parrot.state_dict()``.

    ``forced_duration=d`` zeroes ``duration_predictor.proj.weight`` and sets its bias to
    ``ln(d+1)`` so every valid token gets duration ``d`` (L = d*S exactly).
    """
    rng = _rng(seed)
    tr = cfg["transformer"]
    D, F = tr["d_model"], tr["conv_n_filter"]
    k1, k2 = tr["conv_kernel_sizes"]
    dp = cfg["duration_predictor"]
    NF, DK = dp["n_filter"], dp["kernel_size"]
    V = cfg["preprocess"]["hubert_codes"]
    sd: Dict[str, torch.Tensor] = {}
    sd["pos_emb.pe"] = sinusoid_table(tr["max_len"], D)
    sd["tok_emb.weight"] = _normal(rng, (src_vocab_size, D), 1.0)
    if n_speaker > 1:
        sd["speaker_emb.weight"] = _normal(rng, (n_speaker, D), 0.5)
    for idx, (cin, cout) in ((0, (D, NF)), (4, (NF, NF))):
        sd[f"duration_predictor.layers.{idx}.conv.weight"] = _normal(rng, (cout, cin, DK), gain / math.sqrt(cin * DK))
        sd[f"duration_predictor.layers.{idx}.conv.bias"] = _normal(rng, (cout,), 0.05)
    for idx in (2, 6):
        sd[f"duration_predictor.layers.{idx}.weight"] = 1.0 + _normal(rng, (NF,), 0.1)
        sd[f"duration_predictor.layers.{idx}.bias"] = _normal(rng, (NF,), 0.05)
    sd["duration_predictor.proj.weight"] = _normal(rng, (1, NF), 1.0 / math.sqrt(NF))
    sd["duration_predictor.proj.bias"] = torch.full((1,), 1.0)
    for side in ("encoder", "decoder"):
        for n in range(tr[side]["n_layer"]):
            p = f"{side}_layers.{n}."
            sd[p + "attention.qkv.weight"] = _normal(rng, (3 * D, D), gain / math.sqrt(D))
            sd[p + "attention.mha.in_proj_weight"] = _normal(rng, (3 * D, D), gain / math.sqrt(D))
            sd[p + "attention.mha.out_proj.weight"] = _normal(rng, (D, D), gain / math.sqrt(D))
            sd[p + "attention.wo.weight"] = _normal(rng, (D, D), gain / math.sqrt(D))
            sd[p + "convlayer.conv1.weight"] = _normal(rng, (F, D, k1), gain / math.sqrt(D * k1))
            sd[p + "convlayer.conv1.bias"] = _normal(rng, (F,), 0.05)
            sd[p + "convlayer.conv2.weight"] = _normal(rng, (D, F, k2), gain / math.sqrt(F * k2))
            sd[p + "convlayer.conv2.bias"] = _normal(rng, (D,), 0.05)
            for nm in ("attn_norm", "conv_norm"):
                sd[p + nm + ".weight"] = 1.0 + _normal(rng, (D,), 0.1)
                sd[p + nm + ".bias"] = _normal(rng, (D,), 0.05)
    sd["head.weight"] = _normal(rng, (V, D), 1.0 / math.sqrt(D))
    sd["head.bias"] = _normal(rng, (V,), 0.05)
    if forced_duration is not None:
        sd["duration_predictor.proj.weight"] = torch.zeros(1, NF)
        sd["duration_predictor.proj.bias"] = torch.full((1,), math.log(forced_duration + 1.0))
    return sd


def synth_tte_batch(B: int, S: int, vocab: int, n_speaker: int, seed: int = 0, ragged: bool = False) -> dict:
    """A collated inference batch like ``ParrotDataset.collate_fn`` makes (modules/data.py:102-120):
    ``phones`` (B,S) int64 right-padded with 0, ``src_mask`` (B,S) bool True=valid, ``speaker`` (B,)."""
    rng = _rng(seed)
    phones = rng.integers(2, vocab, size=(B, S), dtype=np.int64)
    lens = np.full((B,), S, dtype=np.int64)
    if ragged and B > 1:
        lens = rng.integers(max(1, S // 2), S + 1, size=(B,), dtype=np.int64)
        lens[0] = S  # pad_sequence pads to the longest row
        for b in range(B):
            phones[b, lens[b]:] = 0
    speaker = rng.integers(0, max(1, n_speaker), size=(B,), dtype=np.int64)
    phones_t = torch.from_numpy(phones)
    return {"phones": phones_t, "src_mask": phones_t != 0, "speaker": torch.from_numpy(speaker),
            "src_lens": torch.from_numpy(lens)}


# --------------------------------------------------------------------------------------
# vocoder
# --------------------------------------------------------------------------------------
def voc_layer_shapes(h: dict):
    """(name, kind, cin, cout, k, stride) for every weight-normed layer, in state_dict order."""
    c0 = h["upsample_initial_channel"]
    out = [("conv_pre", "conv", h.get("model_in_dim", 128), c0, 7, 1)]
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        out.append((f"ups.{i}", "convT", c0 // (2 ** i), c0 // (2 ** (i + 1)), k, u))
    nk = len(h["resblock_kernel_sizes"])
    for i in range(len(h["upsample_rates"])):
        ch = c0 // (2 ** (i + 1))
        for j, k in enumerate(h["resblock_kernel_sizes"]):
            n_conv = 3 if str(h["resblock"]) == "1" else 2  # what the reference constructors build (models.py:17-22,51-54), whatever the list length
            for m in range(n_conv):
                if str(h["resblock"]) == "1":
                    out.append((f"resblocks.{i * nk + j}.convs1.{m}", "conv", ch, ch, k, 1))
                    out.append((f"resblocks.{i * nk + j}.convs2.{m}", "conv", ch, ch, k, 1))
                else:
                    out.append((f"resblocks.{i * nk + j}.convs.{m}", "conv", ch, ch, k, 1))
    out.append(("conv_post", "conv", c0 // (2 ** len(h["upsample_rates"])), 1, 7, 1))
    return out


def synth_voc_state_dict(h: dict, seed: int = 1234, scale: float = 1.0, jitter_g: bool = True) -> Dict[str, torch.Tensor]:
    """Seeded generator checkpoint body (what sits under ``['generator']`` in ``g_%08d`` files,
    reference utils/vocoder/train.py:183-186) with weight-norm attached.

    Recipe from SURVEY §8c: ``weight_v ~ N(0, scale/sqrt(fan_in))`` with fan_in = C_in*k
    (Conv1d) or C_in*k/u (ConvTranspose1d); ``weight_g = ||v|| * U(1,1.3)``; ``bias ~ N(0,0.02)``.
    Conv1d ``weight_v`` is (C_out,C_in,k) with g per out-channel; ConvTranspose1d ``weight_v`` is
    (C_in,C_out,k) with g per *in*-channel (both: norm over dims != 0)."""
    rng = _rng(seed)
    sd: Dict[str, torch.Tensor] = {}
    for name, kind, cin, cout, k, u in voc_layer_shapes(h):
        if kind == "conv":
            v = _normal(rng, (cout, cin, k), scale / math.sqrt(cin * k))
        else:
            v = _normal(rng, (cin, cout, k), scale / math.sqrt(cin * k / u))
        norm = v.flatten(1).norm(dim=1).reshape(-1, 1, 1)
        g = norm.clone()
        if jitter_g:
            g = g * torch.from_numpy(rng.uniform(1.0, 1.3, size=tuple(g.shape)).astype(np.float32))
        sd[name + ".bias"] = _normal(rng, (cout,), 0.02)
        sd[name + ".weight_g"] = g
        sd[name + ".weight_v"] = v
    sd["dict.weight"] = _normal(rng, (h["num_embeddings"], h["embedding_dim"]), 1.0)
    if h.get("multispkr"):
        sd["spkr.weight"] = _normal(rng, (10, h["embedding_dim"]), 1.0)
    return sd


def synth_voc_batch(B: int, U: int, h: dict, seed: int = 0) -> dict:
    """``code`` (B,U) int64 in [0,num_embeddings), ``spkr`` (B,1) int64 in [0,10)."""
    rng = _rng(seed)
    code = torch.from_numpy(rng.integers(0, h["num_embeddings"], size=(B, U), dtype=np.int64))
    spkr = torch.from_numpy(rng.integers(0, 10, size=(B, 1), dtype=np.int64))
    return {"code": code, "spkr": spkr}


# --------------------------------------------------------------------------------------
# aligner
# --------------------------------------------------------------------------------------
def default_aligner_config(data_dir: str = "runs/aligner/data") -> dict:
    """Model-relevant part of utils/aligner/aligner_train_config.yaml."""
    return {
        "paths": {"dataset_dir": None, "data_dir": data_dir, "symbols_path": None, "metadata_path": "wavs", "dur_path": None},
        "audio": {"sample_rate": 16000, "n_filters": 1024, "n_mels": 80, "win_length": 1024, "hop_length": 320, "fmin": 0, "fmax": 8000,
                  "power": 1},
        "model": {"lstm_dim": 512, "conv_dim": 512},
        "durations": {"method": "dijkstra"},
    }


def small_aligner_config(data_dir: str = "runs/aligner/data") -> dict:
    """A reduced aligner (same graph, smaller dims) for fast CPU goldens / smoke tests."""
    cfg = default_aligner_config(data_dir)
    cfg["audio"]["n_mels"] = 16
    cfg["model"].update(lstm_dim=32, conv_dim=32)
    return cfg


def synth_aligner_state_dict(cfg: dict, num_symbols: int, seed: int = 7, gain: float = 1.0) -> Dict[str, torch.Tensor]:
    """Seeded weights with the key set of the reference ``Aligner.state_dict()`` (utils/aligner/model.py:24-40): ``step``, three
    bias-free k = 5 convs with BatchNorm parameters AND running statistics (the mean positive: it follows a ReLU), the
    bidirectional LSTM, the Linear.  ``gain`` scales ``lin.weight``: large values make the softmax peaky, as a trained aligner's."""
    rng = _rng(seed)
    n_mels, D, H = cfg["audio"]["n_mels"], cfg["model"]["conv_dim"], cfg["model"]["lstm_dim"]
    sd: Dict[str, torch.Tensor] = {"step": torch.tensor(1, dtype=torch.int)}
    for i in range(3):
        cin = n_mels if i == 0 else D
        p = f"convs.{i}."
        sd[p + "conv.weight"] = _normal(rng, (D, cin, 5), 1.4 / math.sqrt(cin * 5))
        sd[p + "bnorm.weight"] = 1.0 + _normal(rng, (D,), 0.1)
        sd[p + "bnorm.bias"] = _normal(rng, (D,), 0.05)
        sd[p + "bnorm.running_mean"] = torch.from_numpy(rng.uniform(0.2, 0.6, size=(D,)).astype(np.float32)).clone()
        sd[p + "bnorm.running_var"] = torch.from_numpy(rng.uniform(0.3, 1.0, size=(D,)).astype(np.float32)).clone()
        sd[p + "bnorm.num_batches_tracked"] = torch.tensor(1000, dtype=torch.long)
    for sfx in ("", "_reverse"):
        sd["rnn.weight_ih_l0" + sfx] = _normal(rng, (4 * H, D), 1.0 / math.sqrt(D))
        sd["rnn.weight_hh_l0" + sfx] = _normal(rng, (4 * H, H), 1.0 / math.sqrt(H))
        sd["rnn.bias_ih_l0" + sfx] = _normal(rng, (4 * H,), 0.1)
        sd["rnn.bias_hh_l0" + sfx] = _normal(rng, (4 * H,), 0.1)
    sd["lin.weight"] = _normal(rng, (num_symbols, 2 * H), gain / math.sqrt(2 * H))
    sd["lin.bias"] = _normal(rng, (num_symbols,), 0.05)
    return sd


def synth_aligner_mel(B: int, T: int, n_mels: int, mel_len=None, seed: int = 0) -> torch.Tensor:
    """A padded mel batch (B, T, n_mels) as ``collate_dataset`` makes it (utils/aligner/dataset.py:66-75): smooth seeded log-mel-like
    values, zero beyond ``mel_len[b]``."""
    rng = _rng(seed)
    x = rng.standard_normal(size=(B, T + 4, n_mels))
    x = (x[:, :-4] + x[:, 1:-3] + x[:, 2:-2] + x[:, 3:-1] + x[:, 4:]) * 0.8 - 1.0
    mel = torch.from_numpy(x.astype(np.float32)).clone()
    if mel_len is not None:
        for b, n in enumerate(mel_len):
            mel[b, int(n):] = 0.0
    return mel


def clone_config(cfg: dict) -> dict:
    return copy.deepcopy(cfg)


# --------------------------------------------------------------------------------------
# multi-period discriminator
# --------------------------------------------------------------------------------------
def default_mpd_config() -> dict:
    """What reference utils/vocoder/models.py:171-210 hard-codes."""
    return {"periods": [2, 3, 5, 7, 11], "channels": [32, 128, 512, 1024], "kernel_size": 5, "stride": 3}


def mpd_layer_shapes(cfg: dict):
    """(key prefix, cout, cin, k) of every conv in state_dict order: per period convs.0 .. convs.4, then conv_post."""
    c = [1] + list(cfg["channels"]) + [cfg["channels"][-1]]
    out = []
    for i in range(len(cfg["periods"])):
        out += [(f"discriminators.{i}.convs.{l}", c[l + 1], c[l], cfg["kernel_size"]) for l in range(5)]
        out.append((f"discriminators.{i}.conv_post", 1, c[5], 3))
    return out


def synth_mpd_state_dict(cfg: dict = None, seed: int = 1234) -> Dict[str, torch.Tensor]:
    """Seeded ``mpd`` entry of a ``do_%08d`` checkpoint (reference utils/vocoder/train.py:187-192) with weight norm attached, the
    reference's key order (bias, weight_g, weight_v).  fp64 draws n ~ N(0, 1) from one ``torch.Generator``, rounded to fp32:
    ``weight_v = n / sqrt(cin k)``, ``weight_g = ||v|| (1 + 0.1 n)``, ``bias = 0.1 n``; conv_post has ``g = ||v||`` and a zero bias, so
    scores stay of order one.  The default config's dict is 164 MB."""
    cfg = cfg or default_mpd_config()
    gen = torch.Generator().manual_seed(seed)
    draw = lambda *shape: torch.randn(shape, generator=gen, dtype=torch.float64)  # noqa: E731
    sd: Dict[str, torch.Tensor] = {}
    for name, cout, cin, k in mpd_layer_shapes(cfg):
        post = name.endswith("conv_post")
        v = (draw(cout, cin, k, 1) / math.sqrt(cin * k)).to(torch.float32)
        norm = v.double().flatten(1).norm(dim=1).reshape(-1, 1, 1, 1)
        g = norm if post else norm * (1 + 0.1 * draw(cout, 1, 1, 1))
        sd[name + ".bias"] = torch.zeros(cout) if post else (0.1 * draw(cout)).to(torch.float32)
        sd[name + ".weight_g"] = g.to(torch.float32)
        sd[name + ".weight_v"] = v
    return sd


def synth_mpd_batch(B: int, T: int, seed: int = 1235):
    """``(y, y_hat)``, each (B, 1, T) fp32: 0.3 n, fp64 draws rounded to fp32."""
    gen = torch.Generator().manual_seed(seed)
    y, y_hat = (0.3 * torch.randn((B, 1, T), generator=gen, dtype=torch.float64) for _ in range(2))
    return y.to(torch.float32), y_hat.to(torch.float32)


def default_msd_config() -> dict:
    """What reference utils/vocoder/models.py:228-258 hard-codes: the widths and group counts of convs[0 .. 7) of every DiscriminatorS
    (kernel sizes 15, 41 x 5, 5 and strides 1, 2, 2, 4, 4, 1, 1 are fixed), three scales, spectral norm on the first."""
    return {"channels": [128, 128, 256, 512, 1024, 1024, 1024], "groups": [1, 4, 16, 16, 16, 16, 1], "n_scales": 3}


MSD_KERNELS = (15, 41, 41, 41, 41, 41, 5)


def msd_layer_shapes(cfg: dict):
    """(key prefix, cout, cin / groups, k) of every conv in state_dict order: per scale convs.0 .. convs.6, then conv_post."""
    c = [1] + list(cfg["channels"])
    out = []
    for i in range(cfg["n_scales"]):
        out += [(f"discriminators.{i}.convs.{l}", c[l + 1], c[l] // cfg["groups"][l], MSD_KERNELS[l]) for l in range(7)]
        out.append((f"discriminators.{i}.conv_post", 1, c[7], 3))
    return out


def synth_msd_state_dict(cfg: dict = None, seed: int = 1234) -> Dict[str, torch.Tensor]:
    """Seeded ``msd`` entry of a ``do_%08d`` checkpoint (reference utils/vocoder/train.py:187-192), the reference's key order.
    fp64 draws n ~ N(0, 1) from one ``torch.Generator``, rounded to fp32.  Discriminator 0 (spectral norm): ``bias = 0.1 n``,
    ``weight_orig = n / sqrt(cin_g k)``, ``weight_u`` and ``weight_v`` unit-norm normals FAR FROM CONVERGED, as a fresh constructor
    leaves them, so that sigma after one power iteration and after two differ visibly; conv_post has a zero bias.  Discriminators 1
    and up (weight norm): as ``synth_mpd_state_dict``.  The default config's dict is 118 MB."""
    cfg = cfg or default_msd_config()
    gen = torch.Generator().manual_seed(seed)
    draw = lambda *shape: torch.randn(shape, generator=gen, dtype=torch.float64)  # noqa: E731
    sd: Dict[str, torch.Tensor] = {}
    for name, cout, cin, k in msd_layer_shapes(cfg):
        post = name.endswith("conv_post")
        w = (draw(cout, cin, k) / math.sqrt(cin * k)).to(torch.float32)
        sd[name + ".bias"] = torch.zeros(cout) if post else (0.1 * draw(cout)).to(torch.float32)
        if name.startswith("discriminators.0."):
            u, v = draw(cout), draw(cin * k)
            sd[name + ".weight_orig"] = w
            sd[name + ".weight_u"] = (u / u.norm()).to(torch.float32)
            sd[name + ".weight_v"] = (v / v.norm()).to(torch.float32)
        else:
            norm = w.double().flatten(1).norm(dim=1).reshape(-1, 1, 1)
            sd[name + ".weight_g"] = (norm if post else norm * (1 + 0.1 * draw(cout, 1, 1))).to(torch.float32)
            sd[name + ".weight_v"] = w
    return sd


def synth_msd_batch(B: int, T: int, seed: int = 1235):
    """``(y, y_hat)``, each (B, 1, T) fp32: 0.3 n, fp64 draws rounded to fp32."""
    return synth_mpd_batch(B, T, seed)
