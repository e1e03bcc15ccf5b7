"""CPU restatement of the reference's aligner stage: ``Aligner.forward`` (utils/aligner/model.py:24-48) in the tensor's own dtype
(fp32: what the reference computes; fp64: the yardstick the goldens carry), the softmax of utils/aligner/extract_durations.py:91-93,
and ``extract_durations_with_dijkstra`` (utils/aligner/duration_extraction.py:52-85) as the fp64 dynamic programme it is, with the
library's documented tie rule (diagonal, then previous frame, then previous token)."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

# tests/golden fixtures written by tools/make_aligner_goldens.py
MODEL_GOLDENS = ["aligner_small", "aligner_full", "aligner_small_long"]
DP_GOLDEN = "align_dp"
BN_EPS = 1e-5


def load_golden(golden_dir: str, name: str):
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    return z, json.loads(str(z["meta"]))


def lstm_direction(x, w_ih, w_hh, b_ih, b_hh, reverse: bool):
    """One direction of a one-layer nn.LSTM, batch_first: x (B, T, D) -> (B, T, H); gates i, f, g, o; h_0 = c_0 = 0."""
    B, T, _ = x.shape
    H = w_hh.shape[1]
    h = x.new_zeros(B, H)
    c = x.new_zeros(B, H)
    out = x.new_zeros(B, T, H)
    xp = x @ w_ih.t() + b_ih
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        g = xp[:, t] + (h @ w_hh.t() + b_hh)
        i_, f_, g_, o_ = g[:, :H], g[:, H:2 * H], g[:, 2 * H:3 * H], g[:, 3 * H:]
        c = torch.sigmoid(f_) * c + torch.sigmoid(i_) * torch.tanh(g_)
        h = torch.sigmoid(o_) * torch.tanh(c)
        out[:, t] = h
    return out


def lstm_steps(w_hh, xproj, h0=None, c0=None, n_steps=None, dtype=torch.float64):
    """The recurrence of ``lstm_direction`` for both directions at once, started from a given state and stopped after ``n_steps``:
    w_hh (2, 4H, H) [forward, backward], xproj (B, T, 8H) = W_ih x + b_ih + b_hh of both directions, h0 / c0 (2, B, H) or None for
    zeros -> out (B, T, 2H), h_n, c_n (2, B, H), gates (B, T, 8H) = sigmoid(i), sigmoid(f), tanh(g), sigmoid(o) per direction, c_all
    (B, T, 2H), all in ``dtype``.  The forward direction takes frames 0 .. n_steps - 1, the backward one T - 1 .. T - n_steps; frames
    no step owns are zero.  The pre-activation is xproj[:, t] + h W_hh^T: ``lstm_direction``'s with b_hh already inside xproj."""
    w_hh, xproj = torch.as_tensor(w_hh).to(dtype), torch.as_tensor(xproj).to(dtype)
    B, T, H = xproj.shape[0], xproj.shape[1], w_hh.shape[2]
    n_steps = T if n_steps is None else int(n_steps)
    assert w_hh.shape == (2, 4 * H, H) and xproj.shape == (B, T, 8 * H) and 1 <= n_steps <= T
    h_n = xproj.new_zeros(2, B, H) if h0 is None else torch.as_tensor(h0).to(dtype).clone()
    c_n = xproj.new_zeros(2, B, H) if c0 is None else torch.as_tensor(c0).to(dtype).clone()
    out, c_all, gates = xproj.new_zeros(B, T, 2 * H), xproj.new_zeros(B, T, 2 * H), xproj.new_zeros(B, T, 8 * H)
    for d in range(2):
        h, c = h_n[d], c_n[d]
        for step in range(n_steps):
            t = T - 1 - step if d else step
            g = xproj[:, t, d * 4 * H:(d + 1) * 4 * H] + (h @ w_hh[d].t())
            i_, f_, g_, o_ = torch.sigmoid(g[:, :H]), torch.sigmoid(g[:, H:2 * H]), torch.tanh(g[:, 2 * H:3 * H]), torch.sigmoid(g[:, 3 * H:])
            c = f_ * c + i_ * g_
            h = o_ * torch.tanh(c)
            out[:, t, d * H:(d + 1) * H] = h
            c_all[:, t, d * H:(d + 1) * H] = c
            gates[:, t, d * 4 * H:(d + 1) * 4 * H] = torch.cat([i_, f_, g_, o_], dim=1)
        h_n[d], c_n[d] = h, c
    return out, h_n, c_n, gates, c_all


def lstm_preactivations(w_hh, xproj, h0, dtype=torch.float64):
    """The gate pre-activations of step 0 of ``lstm_steps`` from h0 (2, B, H): (2, B, 4H), forward direction at frame 0, backward at T - 1."""
    w_hh, xproj, h0 = (torch.as_tensor(v).to(dtype) for v in (w_hh, xproj, h0))
    T, H = xproj.shape[1], w_hh.shape[2]
    return torch.stack([xproj[:, T - 1 if d else 0, d * 4 * H:(d + 1) * 4 * H] + (h0[d] @ w_hh[d].t()) for d in range(2)])


def aligner_forward(sd: dict, mel: torch.Tensor):
    """mel (B, T, n_mels) -> (logits (B, T, V), {"bn3": (B, T, conv_dim), "lstm": (B, T, 2 lstm_dim)}) in mel's dtype, from the fp32
    state_dict the reference holds.  The whole padded batch, no masking (model.py:41-48)."""
    dt = mel.dtype
    P = lambda k: sd[k].to(dt)  # noqa: E731
    x = mel
    for i in range(3):
        p = f"convs.{i}."
        y = F.conv1d(x.transpose(1, 2), P(p + "conv.weight"), None, padding=2)
        y = F.relu(y)
        y = F.batch_norm(y, P(p + "bnorm.running_mean"), P(p + "bnorm.running_var"), P(p + "bnorm.weight"), P(p + "bnorm.bias"), False, 0.1, BN_EPS)
        x = y.transpose(1, 2)
    bn3 = x
    fwd = lstm_direction(x, P("rnn.weight_ih_l0"), P("rnn.weight_hh_l0"), P("rnn.bias_ih_l0"), P("rnn.bias_hh_l0"), False)
    bwd = lstm_direction(x, P("rnn.weight_ih_l0_reverse"), P("rnn.weight_hh_l0_reverse"), P("rnn.bias_ih_l0_reverse"), P("rnn.bias_hh_l0_reverse"), True)
    lstm = torch.cat([fwd, bwd], dim=-1)
    logits = lstm @ P("lin.weight").t() + P("lin.bias")
    return logits, {"bn3": bn3, "lstm": lstm}


def softmax_rows(logits: torch.Tensor, mel_len) -> torch.Tensor:
    """extract_durations.py:91-93 per row; frames at or beyond mel_len[b] are zero."""
    pred = torch.zeros_like(logits)
    for b, n in enumerate(mel_len):
        pred[b, :int(n)] = torch.softmax(logits[b, :int(n)], dim=-1)
    return pred


def path_weights(tokens: np.ndarray, pred: np.ndarray) -> np.ndarray:
    """w[i][j] = fl32(1 - pred[i, tokens[j]]) widened to fp64 (numpy subtracts in float32, scipy widens)."""
    pm = np.asarray(pred, dtype=np.float32)[:, np.asarray(tokens).astype(np.int64)]
    return (np.float32(1.0) - pm).astype(np.float32).astype(np.float64)


def dp_tables(tokens: np.ndarray, pred: np.ndarray):
    """-> (dist (T, N) fp64, move (T, N): 0 diagonal, 1 previous frame, 2 previous token, tie (T, N) bool: the two smallest
    predecessor distances of the cell are equal).  dist[0][0] = 0 (Dijkstra's source), sums in path order."""
    w = path_weights(tokens, pred)
    T, N = w.shape
    dist = np.zeros((T, N), dtype=np.float64)
    move = np.zeros((T, N), dtype=np.int8)
    tie = np.zeros((T, N), dtype=bool)
    inf = float("inf")
    for i in range(T):
        for j in range(N):
            if i == 0 and j == 0:
                continue
            dg = dist[i - 1, j - 1] if (i > 0 and j > 0) else inf
            up = dist[i - 1, j] if i > 0 else inf
            lf = dist[i, j - 1] if j > 0 else inf
            if dg <= up and dg <= lf:
                best, m = dg, 0
            elif up <= lf:
                best, m = up, 1
            else:
                best, m = lf, 2
            s = sorted((dg, up, lf))
            tie[i, j] = s[0] == s[1]
            dist[i, j] = best + w[i, j]
            move[i, j] = m
    return dist, move, tie


def dp_durations(tokens: np.ndarray, pred: np.ndarray, with_info: bool = False):
    """The fp64 DP with the documented tie rule -> durations (N,) int32 [, cost = dist[T-1][N-1], unique: no tie on the path]."""
    dist, move, tie = dp_tables(tokens, pred)
    T, N = dist.shape
    dur = np.zeros(N, dtype=np.int32)
    i, j = T - 1, N - 1
    dur[j] += 1
    unique = True
    while i > 0 or j > 0:
        unique = unique and not tie[i, j]
        m = move[i, j]
        if m == 2:
            j -= 1
        else:
            i -= 1
            if m == 0:
                j -= 1
            dur[j] += 1  # the backward walk enters frame i at the LAST token the path visits in it
    if with_info:
        return dur, float(dist[T - 1, N - 1]), bool(unique)
    return dur


def dp_durations_fast(tokens: np.ndarray, pred: np.ndarray):
    """``dp_durations`` for sizes where ``dp_tables``' Python double loop is too slow (2100 x 2048): the same fp64 programme swept along
    the anti-diagonals i + j = d with numpy -- the same three predecessor reads (+inf outside the grid), the same tie rule (diagonal,
    then previous frame, then previous token), the same best + w and the same backward walk -> (durations (N,) int32, cost)."""
    w = path_weights(tokens, pred)
    T, N = w.shape
    D = np.full((T + 1, N + 1), np.inf, dtype=np.float64)  # D[i + 1][j + 1] = dist[i][j]; row 0 and column 0 stand for "outside"
    move = np.zeros((T, N), dtype=np.int8)
    D[1, 1] = 0.0
    for d in range(1, T + N - 1):
        j = np.arange(max(0, d - (T - 1)), min(N - 1, d) + 1)
        i = d - j
        dg, up, lf = D[i, j], D[i, j + 1], D[i + 1, j]
        m = np.where((dg <= up) & (dg <= lf), 0, np.where(up <= lf, 1, 2))
        best = np.where(m == 0, dg, np.where(m == 1, up, lf))
        D[i + 1, j + 1] = best + w[i, j]
        move[i, j] = m
    dur = np.zeros(N, dtype=np.int32)
    i, j = T - 1, N - 1
    dur[j] += 1
    while i > 0 or j > 0:
        m = move[i, j]
        if m == 2:
            j -= 1
        else:
            i -= 1
            if m == 0:
                j -= 1
            dur[j] += 1
    return dur, float(D[T, N])


def path_cost(durations: np.ndarray, tokens: np.ndarray, pred: np.ndarray) -> float:
    """Cost of the cheapest path consistent with ``durations`` (frame i's last token is fixed by them).  Since w >= 0 the path
    enters each new frame diagonally whenever the token advances, then moves right to the frame's last token."""
    w = path_weights(tokens, pred)
    T, N = w.shape
    last = np.repeat(np.arange(N), np.asarray(durations).astype(np.int64))
    assert last.shape[0] == T, "durations must sum to the number of frames"
    cost = 0.0
    for j in range(1, last[0] + 1):
        cost += w[0, j]
    for i in range(1, T):
        lo = last[i - 1] if last[i] == last[i - 1] else last[i - 1] + 1
        for j in range(lo, last[i] + 1):
            cost += w[i, j]
    assert last[-1] == N - 1, "the path ends at the last token"
    return float(cost)
