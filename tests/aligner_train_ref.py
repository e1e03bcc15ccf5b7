"""CPU restatement of the reference's aligner in TRAINING (utils/aligner/model.py:5-48 under ``model.train()``, the loss of
utils/aligner/trainer.py:60-63): torch functional ops in the tensors' own dtype (fp32: what the reference computes; fp64: the
yardstick), differentiable by torch's CPU autograd.  Needs no file of the reference at run time; tools/make_aligner_train_goldens.py
holds it to the reference itself."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

BN_EPS = 1e-5
MOMENTUM = 0.1
TRAIN_GOLDENS = ["aligner_train_s1", "aligner_train_s2"]

# name: (B, T, n_mels, V, lstm_dim, conv_dim, N)
SHAPES = {
    "S1": (3, 37, 24, 13, 32, 32, 5),
    "S2": (9, 70, 24, 13, 48, 32, 7),
    "S3": (1, 2, 24, 13, 32, 32, 1),
    "S4": (2, 33, 80, 13, 32, 32, 4),
    "S5": (17, 5, 24, 13, 32, 32, 2),  # more rows than one 16-row batch pass of the LSTM step kernels
    # three trips of both LSTM k-loops with only some lanes in the last (128 + 4q < 144, 512 + 4q < 576); two block rows and a partial
    # K pass in every conv and its gradients; 20 staging passes in the convs, 36 in dy_2
    "S6": (2, 9, 24, 13, 144, 112, 3),
    "S7": (3, 130, 24, 70, 32, 32, 6),  # three column blocks, the last 2 wide; a chunk boundary inside a batch row (B T = 390); V > 64
    "S8": (3, 1, 24, 13, 32, 32, 1),    # T = 1: every side tap outside, one step of the recurrence
}

PARAM_KEYS = ([f"convs.{i}.conv.weight" for i in range(3)] + [f"convs.{i}.bnorm.weight" for i in range(3)]
              + [f"convs.{i}.bnorm.bias" for i in range(3)]
              + [f"rnn.{k}_l0{sfx}" for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh") for sfx in ("", "_reverse")]
              + ["lin.weight", "lin.bias"])
BUFFER_KEYS = [f"convs.{i}.bnorm.{k}" for i in range(3) for k in ("running_mean", "running_var")]


def load_golden(golden_dir: str, name: str):
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    return z, json.loads(str(z["meta"]))


def golden_state_dict(z) -> dict:
    sd = {k[3:]: torch.from_numpy(z[k]).clone() for k in z.files if k.startswith("sd.")}
    return sd


def case_config(shape: str) -> dict:
    B, T, n_mels, V, H, D, N = SHAPES[shape]
    return {"audio": {"n_mels": n_mels}, "model": {"lstm_dim": H, "conv_dim": D}}


def make_case(shape: str, seed: int = 0):
    """Seeded state dict, mel, tokens and lengths of a shape of the table above (parrot_tts_amd.synth).  S1: row 0's mel is zero from
    frame 25 on.  Tokens never repeat, so every row has a path when mel_len >= tokens_len."""
    from parrot_tts_amd import synth
    B, T, n_mels, V, H, D, N = SHAPES[shape]
    sd = synth.synth_aligner_state_dict(case_config(shape), V, seed=100 + seed, gain=2.0)
    mel_len = [T] * B
    if shape == "S1":
        mel_len[0] = 25
    mel = synth.synth_aligner_mel(B, T, n_mels, mel_len, seed=200 + seed)
    rng = np.random.Generator(np.random.PCG64(300 + seed))
    tokens = np.zeros((B, N), np.int64)
    tokens_len = [max(1, N - (b % 3)) for b in range(B)]
    for b in range(B):
        t = rng.integers(1, V, size=tokens_len[b])
        for j in range(1, len(t)):
            while t[j] == t[j - 1]:
                t[j] = rng.integers(1, V)
        tokens[b, :tokens_len[b]] = t
    return sd, mel, torch.from_numpy(tokens), torch.tensor(mel_len, dtype=torch.int64), torch.tensor(tokens_len, dtype=torch.int64)


def lstm_direction(x, w_ih, w_hh, b_ih, b_hh, reverse: bool):
    """One direction of a one-layer nn.LSTM, batch_first: x (B, T, D) -> (B, T, H); gates i, f, g, o; h_0 = c_0 = 0."""
    B, T, _ = x.shape
    H = w_hh.shape[1]
    h = x.new_zeros(B, H)
    c = x.new_zeros(B, H)
    outs = [None] * T
    xp = x @ w_ih.t() + b_ih
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        g = xp[:, t] + (h @ w_hh.t() + b_hh)
        i_, f_, g_, o_ = g[:, :H], g[:, H:2 * H], g[:, 2 * H:3 * H], g[:, 3 * H:]
        c = torch.sigmoid(f_) * c + torch.sigmoid(i_) * torch.tanh(g_)
        h = torch.sigmoid(o_) * torch.tanh(c)
        outs[t] = h
    return torch.stack(outs, dim=1)


def forward(P: dict, mel: torch.Tensor, training: bool = True):
    """P: state_dict key -> tensor (parameters may require grad; buffers are read).  mel (B, T, n_mels) -> (logits (B, T, V),
    {buffer key -> value after this forward}), everything in mel's dtype.  training: BatchNorm over all B T values of the padded
    batch (nothing masked), biased variance for the normalisation, unbiased for the running update."""
    dt = mel.dtype
    x = mel
    new_buffers = {}
    for i in range(3):
        p = f"convs.{i}."
        y = F.relu(F.conv1d(x.transpose(1, 2), P[p + "conv.weight"].to(dt), None, padding=2))
        rm, rv = P[p + "bnorm.running_mean"].to(dt), P[p + "bnorm.running_var"].to(dt)
        if training:
            n = y.shape[0] * y.shape[2]
            if n == 1:
                raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(y.shape)}")
            mean = y.mean(dim=(0, 2))
            var = ((y - mean[None, :, None]) ** 2).mean(dim=(0, 2))
            new_buffers[p + "bnorm.running_mean"] = ((1 - MOMENTUM) * rm + MOMENTUM * mean).detach()
            new_buffers[p + "bnorm.running_var"] = ((1 - MOMENTUM) * rv + MOMENTUM * var * n / (n - 1)).detach()
        else:
            mean, var = rm, rv
            new_buffers[p + "bnorm.running_mean"], new_buffers[p + "bnorm.running_var"] = rm, rv
        y = (y - mean[None, :, None]) * torch.rsqrt(var + BN_EPS)[None, :, None] * P[p + "bnorm.weight"].to(dt)[None, :, None] \
            + P[p + "bnorm.bias"].to(dt)[None, :, None]
        x = y.transpose(1, 2)
    R = lambda k: P[k].to(dt)  # noqa: E731
    fwd = lstm_direction(x, R("rnn.weight_ih_l0"), R("rnn.weight_hh_l0"), R("rnn.bias_ih_l0"), R("rnn.bias_hh_l0"), False)
    bwd = lstm_direction(x, R("rnn.weight_ih_l0_reverse"), R("rnn.weight_hh_l0_reverse"), R("rnn.bias_ih_l0_reverse"),
                         R("rnn.bias_hh_l0_reverse"), True)
    logits = torch.cat([fwd, bwd], dim=-1) @ R("lin.weight").t() + R("lin.bias")
    return logits, new_buffers


def ctc(logits, tokens, mel_len, tokens_len):
    """trainer.py:60-63: CTCLoss()(logits.transpose(0, 1).log_softmax(2), tokens, mel_len, tokens_len)."""
    return F.ctc_loss(logits.transpose(0, 1).log_softmax(2), tokens, mel_len, tokens_len)


def leaf_params(sd: dict, dtype) -> dict:
    """sd -> tensors of ``dtype``; the 19 parameters as fresh leaves that require grad."""
    P = {}
    for k, v in sd.items():
        if v.dim() == 0:
            continue
        P[k] = v.detach().to(dtype).clone()
        if k in PARAM_KEYS:
            P[k].requires_grad_(True)
    return P


def loss_and_grads(sd: dict, mel, tokens, mel_len, tokens_len, dtype, grad_logits=None):
    """One training step's numbers in ``dtype`` -> (logits, loss or None, {param key -> gradient}, buffers after the step).  The
    upstream gradient is the CTC loss's, or ``grad_logits`` (B, T, V) when given."""
    P = leaf_params(sd, dtype)
    logits, bufs = forward(P, mel.to(dtype), True)
    if grad_logits is None:
        loss = ctc(logits, tokens, mel_len, tokens_len)
        loss.backward()
    else:
        loss = None
        logits.backward(grad_logits.to(dtype))
    return logits.detach(), (None if loss is None else loss.detach()), {k: P[k].grad for k in PARAM_KEYS}, bufs
