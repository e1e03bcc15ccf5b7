#!/usr/bin/env python3
"""Time one training step of the aligner at the shipped shape (B = 16, T = 600, n_mels 80, conv_dim = lstm_dim = 512): forward, CTC
loss and gradient, backward, clip_grad_norm_ at 1.0, Adam.

    python tools/aligner_train_time.py [--case all] [--steps 20] [--warmup 5] [--rounds 2] [--out FILE]

Cases, on the same GPU, the same seeded weights and batch:
  ours         parrot_tts_amd.aligner.TrainableAligner with parrot_tts_amd.aligner.CTCLoss
  restatement  tests/aligner_train_ref.py (torch functional ops, the LSTM as a Python loop over time) with torch's CTC loss
  torch_nn     the same network from torch.nn modules (Conv1d / BatchNorm1d / nn.LSTM / Linear) with torch's CTC loss: what a torch
               user would run
A step time is a host clock around ``steps`` steps that end in a device synchronise, after ``warmup`` steps; the cases alternate
``rounds`` times so the spread shows.  Prints one JSON line.  For the per-kernel share run one case alone under
``rocprofv3 --kernel-trace --stats -d DIR -- python tools/aligner_train_time.py --case ours --steps 3 --warmup 2``."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

B, T, N_MELS, V, H, D, N = 16, 600, 80, 61, 512, 512, 60


class TorchAligner(nn.Module):
    def __init__(self):
        super().__init__()
        self.convs = nn.ModuleList([nn.Conv1d(N_MELS if i == 0 else D, D, 5, padding=2, bias=False) for i in range(3)])
        self.bnorms = nn.ModuleList([nn.BatchNorm1d(D) for _ in range(3)])
        self.rnn = nn.LSTM(D, H, batch_first=True, bidirectional=True)
        self.lin = nn.Linear(2 * H, V)

    def load_reference_state(self, sd):
        own = {}
        for k, v in sd.items():
            k = k.replace(".conv.weight", ".weight")
            for i in range(3):
                k = k.replace(f"convs.{i}.bnorm.", f"bnorms.{i}.")
            own[k] = v
        own.pop("step")
        self.load_state_dict(own)

    def forward(self, x):
        x = x.transpose(1, 2)
        for conv, bn in zip(self.convs, self.bnorms):
            x = bn(torch.relu(conv(x)))
        x, _ = self.rnn(x.transpose(1, 2))
        return self.lin(x)


def make_batch(dev):
    from parrot_tts_amd import synth
    cfg = {"audio": {"n_mels": N_MELS}, "model": {"lstm_dim": H, "conv_dim": D}}
    sd = synth.synth_aligner_state_dict(cfg, V, seed=21, gain=2.0)
    rng = np.random.Generator(np.random.PCG64(22))
    mel_len = [T] + [int(v) for v in rng.integers(T // 2, T, size=B - 1)]
    mel = synth.synth_aligner_mel(B, T, N_MELS, mel_len, seed=23)
    tokens = torch.from_numpy(rng.integers(1, V, size=(B, N)).astype(np.int64))
    tokens_len = torch.from_numpy(rng.integers(N // 2, N + 1, size=B).astype(np.int64))
    return sd, mel.to(dev), tokens.to(dev), torch.tensor(mel_len, device=dev), tokens_len.to(dev)


def make_case(case, sd, dev):
    """-> (step function, parameters)"""
    if case == "ours":
        from parrot_tts_amd import aligner as A
        model = A.TrainableAligner(N_MELS, V, H, D)
        model.load_state_dict(sd)
        model = model.to(dev).train()
        params, loss_fn = list(model.parameters()), A.CTCLoss()
        fwd = model
    elif case == "torch_nn":
        model = TorchAligner()
        model.load_reference_state(sd)
        model = model.to(dev).train()
        params, loss_fn = list(model.parameters()), nn.CTCLoss()
        fwd = model
    elif case == "restatement":
        import aligner_train_ref as TR
        P = {k: v.to(dev) for k, v in TR.leaf_params(sd, torch.float32).items()}
        for k in TR.PARAM_KEYS:
            P[k] = P[k].detach().requires_grad_(True)
        params, loss_fn = [P[k] for k in TR.PARAM_KEYS], nn.CTCLoss()

        def fwd(mel):
            logits, bufs = TR.forward(P, mel, True)
            P.update(bufs)
            return logits
    else:
        raise SystemExit(f"unknown case {case}")
    optim = torch.optim.Adam(params, lr=1e-4)

    def step(mel, tokens, mel_len, tokens_len):
        pred = fwd(mel).transpose(0, 1).log_softmax(2)
        loss = loss_fn(pred, tokens, mel_len, tokens_len)
        optim.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        optim.step()
        return loss

    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="all", choices=["all", "ours", "restatement", "torch_nn"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("aligner_train_time: no GPU; a step time is measured on the device or not at all")
    dev = torch.device("cuda:0")
    sd, mel, tokens, mel_len, tokens_len = make_batch(dev)
    cases = ["ours", "restatement", "torch_nn"] if args.case == "all" else [args.case]
    steps = {c: make_case(c, sd, dev) for c in cases}
    times = {c: [] for c in cases}
    losses = {}
    for c in cases:
        for _ in range(args.warmup):
            steps[c](mel, tokens, mel_len, tokens_len)
        torch.cuda.synchronize()
    for _ in range(args.rounds):
        for c in cases:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                loss = steps[c](mel, tokens, mel_len, tokens_len)
            torch.cuda.synchronize()
            times[c].append((time.perf_counter() - t0) / args.steps * 1e3)
            losses[c] = float(loss.detach())
    out = {"shape": {"B": B, "T": T, "n_mels": N_MELS, "V": V, "lstm_dim": H, "conv_dim": D, "N": N}, "steps": args.steps, "warmup": args.warmup,
           "step_ms": times, "last_loss": losses}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
