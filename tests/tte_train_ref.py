"""CPU restatement of the reference's ``Parrot.forward(batch)`` under ``model.train()`` (modules/parrot.py:90-110 with
inference=False) with ``ModelLoss`` (modules/loss.py), in torch, fp32 or fp64, gradients by ``torch.autograd``.  Built from the
oracle's blocks (oracle/parrot_oracle.py); its own are the attention, which multiplies the softmax probabilities by a GIVEN keep mask
and 1 / (1 - p) (nn.MultiheadAttention's dropout, fft.py:49), and the duration predictor, which takes the two masks of its dropouts
(duration.py:33,37).  Also a numpy restatement of the dropout generator of csrc/tte_train.h (Philox4x32-10)."""
import json
import math
import os
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

from oracle import parrot_oracle as O
from parrot_tts_amd import synth
from teacher_forced_ref import model_loss

# name -> (D, F, NF, V, n_speaker, B, src lens, L, src vocab)
SHAPES = {
    "T1": (64, 128, 64, 100, 3, 3, (7, 5, 4), 70, 40),   # a 64-wide tile edge is crossed; padded target rows
    "T2": (96, 160, 80, 70, 3, 2, (9, 9), 130, 40),      # no multiple of 64; three column blocks; B L > 256
    "T3": (64, 128, 64, 100, 1, 1, (3,), 3, 40),         # every tap of the k = 9 conv partly outside; no speaker_emb
    "T4": (64, 128, 64, 100, 1, 1, (1,), 1, 40),         # S = 1, L = 1
}
_roots = {}


def root_path(n_speaker: int) -> str:
    """A directory with the speakers.json the constructors read (parrot.py:24-26)."""
    if n_speaker not in _roots:
        d = tempfile.mkdtemp(prefix="tte_train_ref_")
        with open(os.path.join(d, "speakers.json"), "w") as f:
            json.dump({f"spk{i}": i for i in range(n_speaker)}, f)
        _roots[n_speaker] = d
    return _roots[n_speaker]


def make_case(shape: str, seed: int = 5):
    """-> (cfg, state dict (fp32), batch with codes), seeded."""
    D, Fn, NF, V, nspk, B, lens, L, vocab = SHAPES[shape]
    cfg = synth.small_tte_config(root_path(nspk))
    cfg["transformer"].update(d_model=D, conv_n_filter=Fn)
    cfg["duration_predictor"]["n_filter"] = NF
    cfg["preprocess"]["hubert_codes"] = V
    sd = synth.synth_tte_state_dict(cfg, vocab, nspk, seed=seed)
    sd["tok_emb.weight"][0] = 0.0  # padding_idx = 0 (nn.Embedding zeroes that row)
    rng = np.random.default_rng(seed)
    S = max(lens)
    phones = np.zeros((B, S), dtype=np.int64)
    dur = np.zeros((B, S), dtype=np.int64)
    for b, n in enumerate(lens):
        phones[b, :n] = rng.integers(1, vocab, size=n)
        total = L if b == 0 else max(n, int(L * (0.55 + 0.15 * b)))
        cuts = np.sort(rng.integers(0, total + 1, size=n - 1)) if n > 1 else np.zeros(0, dtype=np.int64)
        d = np.diff(np.concatenate([[0], cuts, [total]]))
        if n >= 3 and shape == "T1":  # a 0 inside the row
            d[1] += d[2]
            d[2] = 0
        dur[b, :n] = d
    sums = dur.sum(axis=1)
    assert sums.max() == L
    tgt_mask = np.arange(L)[None, :] < sums[:, None]
    codes = rng.integers(0, V, size=(B, L))
    codes[~tgt_mask] = V  # ignore_index beyond the row (data.py's padding)
    batch = {"phones": torch.from_numpy(phones), "src_mask": torch.from_numpy(phones != 0), "speaker": torch.from_numpy(rng.integers(0, nspk, size=B)),
             "duration": torch.from_numpy(dur), "tgt_mask": torch.from_numpy(tgt_mask), "codes": torch.from_numpy(codes)}
    return cfg, sd, batch


# ---- the dropout generator -------------------------------------------------------------------------------------------------------
def philox4x32_10_word0(c0, c1, c2, c3, k0, k1):
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1, m32 = np.uint64(k0), np.uint64(k1), np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return c0


def dropout_mask(seed: int, offset: int, site: int, n: int, p: float) -> np.ndarray:
    """uint8 (n): 1 where element i of ``site`` is kept under (seed, offset) -- the rule of csrc/tte_train.h."""
    i = np.arange(n, dtype=np.uint64)
    w = philox4x32_10_word0(i & np.uint64(0xFFFFFFFF), i >> np.uint64(32), offset & 0xFFFFFFFF, ((offset >> 32) & 0xFFFFFF) | (site << 24),
                            seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    thr = np.uint64(math.floor(float(np.float32(p)) * 16777216.0 + 0.5))
    return ((w >> np.uint64(8)) >= thr).astype(np.uint8)


def drop_scale(p: float, dtype) -> torch.Tensor:
    """1 / (1 - p) as the kernels form it: the fp32 quotient."""
    return torch.tensor(float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))), dtype=dtype)


def site_sizes(cfg: dict, B: int, S: int, L: int):
    """Elements of every dropout site, in site order: 2 of the duration predictor, the encoder blocks, the decoder blocks."""
    tr = cfg["transformer"]
    n = [B * S * cfg["duration_predictor"]["n_filter"]] * 2
    n += [B * tr["encoder"]["n_head"] * S * S] * tr["encoder"]["n_layer"]
    n += [B * tr["decoder"]["n_head"] * L * L] * tr["decoder"]["n_layer"]
    return n


def site_ps(cfg: dict):
    tr = cfg["transformer"]
    return [cfg["duration_predictor"]["dropout_p"]] * 2 + [tr["encoder"]["dropout_p"]] * tr["encoder"]["n_layer"] \
        + [tr["decoder"]["dropout_p"]] * tr["decoder"]["n_layer"]


# ---- the model -------------------------------------------------------------------------------------------------------------------
def _drop(x, mask, p):
    """mask: flat keep mask (uint8 tensor) of x's elements, or None for no dropout."""
    if mask is None:
        return x
    return x * mask.view(x.shape).to(x.dtype) * drop_scale(p, x.dtype)


def attention(sd, p, x, n_head, key_padding_mask, mask, drop_p):
    """O.attention with the dropout of nn.MultiheadAttention on the softmax probabilities (F.multi_head_attention_forward)."""
    B, T, E = x.shape
    hd = E // n_head
    q, k, v = F.linear(x, sd[p + "qkv.weight"]).split(E, dim=2)
    w_q, w_k, w_v = sd[p + "mha.in_proj_weight"].chunk(3)
    q, k, v = (F.linear(t.transpose(1, 0).contiguous(), w) for t, w in ((q, w_q), (k, w_k), (v, w_v)))
    q, k, v = (t.view(T, B * n_head, hd).transpose(0, 1) for t in (q, k, v))
    m = torch.zeros(key_padding_mask.shape, dtype=x.dtype, device=x.device).masked_fill_(key_padding_mask, float("-inf"))
    m = m.view(B, 1, 1, T).expand(-1, n_head, -1, -1).reshape(B * n_head, 1, T)
    w = F.softmax(torch.baddbmm(m, q * math.sqrt(1.0 / float(hd)), k.transpose(-2, -1)), dim=-1)
    w = _drop(w, mask, drop_p)
    o = torch.bmm(w, v).transpose(0, 1).contiguous().view(T * B, E)
    o = F.linear(o, sd[p + "mha.out_proj.weight"]).view(T, B, E).transpose(1, 0)
    return F.linear(o.contiguous(), sd[p + "wo.weight"])


def fft_block(sd, p, x, n_head, ks, kpm, mask, drop_p):
    D = x.shape[-1]
    h = x + attention(sd, p + "attention.", F.layer_norm(x, (D,), sd[p + "attn_norm.weight"], sd[p + "attn_norm.bias"]), n_head, kpm, mask, drop_p)
    return h + O.conv_layer(sd, p + "convlayer.", F.layer_norm(h, (D,), sd[p + "conv_norm.weight"], sd[p + "conv_norm.bias"]), ks)


def duration_predictor(sd, x, kpm, kernel_size, masks, drop_p):
    p = "duration_predictor."
    NF = sd[p + "layers.0.conv.weight"].shape[0]
    o = F.conv1d(x.transpose(1, 2), sd[p + "layers.0.conv.weight"], sd[p + "layers.0.conv.bias"], padding=(kernel_size - 1) // 2).transpose(1, 2)
    o = _drop(F.layer_norm(F.relu(o), (NF,), sd[p + "layers.2.weight"], sd[p + "layers.2.bias"]), masks[0], drop_p)
    o = F.conv1d(o.transpose(1, 2), sd[p + "layers.4.conv.weight"], sd[p + "layers.4.conv.bias"], padding=1).transpose(1, 2)
    o = _drop(F.layer_norm(F.relu(o), (NF,), sd[p + "layers.6.weight"], sd[p + "layers.6.bias"]), masks[1], drop_p)
    return F.linear(o, sd[p + "proj.weight"], sd[p + "proj.bias"]).squeeze(-1).masked_fill(kpm, 0.0)


def forward(sd, cfg, batch, masks=None):
    """-> (logits (B, L, V), log_dur (B, S)).  masks: one flat keep mask per dropout site (site order), or None: no dropout."""
    tr = cfg["transformer"]
    ks, ne, nd = tr["conv_kernel_sizes"], tr["encoder"]["n_layer"], tr["decoder"]["n_layer"]
    ps = site_ps(cfg)
    masks = [None] * (2 + ne + nd) if masks is None else masks
    src_kpm = ~batch["src_mask"]
    out = O.pos_emb(sd["pos_emb.pe"], F.embedding(batch["phones"], sd["tok_emb.weight"], padding_idx=0))  # parrot.py:21
    for n in range(ne):
        out = fft_block(sd, f"encoder_layers.{n}.", out, tr["encoder"]["n_head"], ks, src_kpm, masks[2 + n], ps[2 + n])
    if "speaker_emb.weight" in sd:
        out = out + F.embedding(batch["speaker"], sd["speaker_emb.weight"]).unsqueeze(1)
    log_dur = duration_predictor(sd, out, src_kpm, cfg["duration_predictor"]["kernel_size"], masks[:2], ps[0])
    assert batch["tgt_mask"].shape[1] == int(batch["duration"].sum(dim=1).max())  # duration.py:12
    out, _, _ = O.length_regulator(out, batch["duration"])
    out = O.pos_emb(sd["pos_emb.pe"], out)
    for n in range(nd):
        out = fft_block(sd, f"decoder_layers.{n}.", out, tr["decoder"]["n_head"], ks, ~batch["tgt_mask"], masks[2 + ne + n], ps[2 + ne + n])
    return F.linear(out, sd["head.weight"], sd["head.bias"]), log_dur


def param_keys(sd):
    return [k for k in sd if k != "pos_emb.pe"]


def loss_and_grads(sd, cfg, batch, dtype, upstream=None, masks=None):
    """-> (logits, log_dur, {key -> gradient}, (loss, code_loss, dur_loss)) in ``dtype``.  upstream: None = ModelLoss's gradient, or
    (grad_logits, grad_log_dur)."""
    sdt = {k: v.detach().to(dtype).clone().requires_grad_(k != "pos_emb.pe") for k, v in sd.items()}
    logits, log_dur = forward(sdt, cfg, batch, masks)
    V = cfg["preprocess"]["hubert_codes"]
    b = dict(batch)
    b["duration"] = batch["duration"].to(dtype)
    ld = log_dur.masked_select(batch["src_mask"])
    lt = torch.log(b["duration"] + 1).masked_select(batch["src_mask"])
    code_loss = F.cross_entropy(logits.reshape(-1, V), batch["codes"].reshape(-1), ignore_index=V)
    dur_loss = F.mse_loss(ld, lt)
    losses = (code_loss + dur_loss, code_loss, dur_loss)
    keys = param_keys(sd)
    if upstream is None:
        grads = torch.autograd.grad(losses[0], [sdt[k] for k in keys])
    else:
        grads = torch.autograd.grad([logits, log_dur], [sdt[k] for k in keys], [upstream[0].to(dtype), upstream[1].to(dtype)])
    return logits.detach(), log_dur.detach(), dict(zip(keys, (g.detach() for g in grads))), tuple(float(x.detach()) for x in losses)


__all__ = ["SHAPES", "make_case", "dropout_mask", "forward", "loss_and_grads", "model_loss"]
