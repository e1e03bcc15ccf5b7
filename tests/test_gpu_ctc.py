"""GPU: the aligner's CTC validation loss on the device (parrot_tts_amd.aligner.ctc_loss / Aligner.ctc_loss over parrot_ctc_loss) and
the aligner_eval driver.

The yardstick is the reference's own operator (utils/aligner/trainer.py:60-63) run on the CPU in fp64:
``F.ctc_loss(logits.double().transpose(0, 1).log_softmax(2), ..., reduction='none')``.  The tolerance is relative and per row:
e_ref is the largest relative error of torch's CPU fp32 ``ctc_loss`` against that fp64 run over all finite rows of BOUND_CASES,
measured here, and the device stays within 2 x e_ref on every finite row (2: device expf / logf an ulp off the host's, another
sum order over V).  The cases added for the kernel's own paths (PATH_CASES: more than one state per thread) are held to the same
bound and do not enter e_ref.  Rows without any alignment are +inf on both sides.  Measured (MI355X): DESIGN.md section 3.

The whole file also passes under PARROT_POISON_WS=nan (workspace and outputs filled with NaN at the top of the entry point)."""
import json
import math
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from parrot_tts_amd import _lib, synth  # noqa: E402
from parrot_tts_amd import aligner as A  # noqa: E402

DEV = "cuda:0"


def _tokens(rng, B, N, V, no_repeat_rows=()):
    tokens = rng.integers(1, V, size=(B, N))
    for b in no_repeat_rows:
        for j in range(1, N):
            if tokens[b, j] == tokens[b, j - 1]:
                tokens[b, j] = tokens[b, j] % (V - 1) + 1
    return torch.from_numpy(tokens)


def _case(seed, B, T, V, N, gain, mel_len=None, tokens_len=None, no_repeat_rows=()):
    gen = torch.Generator().manual_seed(seed)
    logits = torch.randn((B, T, V), generator=gen) * gain
    tokens = _tokens(np.random.Generator(np.random.PCG64(seed)), B, N, V, no_repeat_rows)
    return logits, tokens, list(mel_len or [T] * B), list(tokens_len or [N] * B)


def _doubled(mel_len_row1):
    logits, tokens, ml, tl = _case(21, 3, 12, 21, 6, 2.0, mel_len=(12, mel_len_row1, 9), tokens_len=(6, 6, 4))
    tokens[1] = torch.tensor([3, 5, 5, 7, 2, 9])  # one repeat: 7 frames at least
    return logits, tokens, ml, tl


def _with_blank():
    logits, tokens, ml, tl = _case(22, 2, 14, 21, 5, 2.0, mel_len=(14, 11))
    tokens[0] = torch.tensor([4, 0, 0, 7, 0])  # the blank as a label, doubled and last: legal, torch computes it too
    return logits, tokens, ml, tl


BOUND_CASES = {
    "b3t23": lambda: _case(1, 3, 23, 21, 5, 1.0),
    "b3t23_peaky": lambda: _case(1, 3, 23, 21, 5, 6.0),
    "ragged_t_eq_n": lambda: _case(2, 4, 60, 21, 9, 3.0, mel_len=(60, 23, 41, 9), tokens_len=(9, 4, 7, 9), no_repeat_rows=(3,)),
    "ragged_small": lambda: _case(3, 2, 12, 21, 6, 2.0, mel_len=(12, 6), no_repeat_rows=(1,)),
    "smallest": lambda: _case(4, 1, 1, 21, 1, 1.0),
    "s257": lambda: _case(5, 2, 300, 41, 128, 4.0),
    "s601_v100": lambda: _case(6, 2, 700, 100, 300, 4.0),
    "long": lambda: _case(7, 2, 2000, 41, 200, 5.0),
    "doubled_feasible": lambda: _doubled(7),
    "doubled_infeasible": lambda: _doubled(6),
    "blank_token": _with_blank,
}
# beyond 1024 states a thread owns K = ceil(S / 1024) contiguous states: S = 1201 and 1027 (K = 2, the second with idle threads at
# the end), then 2201, 3201 and the module's limit 4097 (K = 3, 4, 5); tokens without repeats, so that every row has a path
PATH_CASES = {
    "k2": lambda: _case(8, 2, 760, 41, 600, 4.0, mel_len=(760, 700), tokens_len=(600, 513), no_repeat_rows=(0, 1)),
    "k345": lambda: _case(9, 3, 2300, 21, 2048, 3.0, mel_len=(2300, 1250, 1800), tokens_len=(2048, 1100, 1600), no_repeat_rows=(0, 1, 2)),
}
ALL_CASES = {**BOUND_CASES, **PATH_CASES}
_cache = {}


def _yardstick(logits, tokens, mel_len, tokens_len, dtype=torch.float64):
    lp = logits.to(dtype).transpose(0, 1).log_softmax(2)
    return F.ctc_loss(lp, tokens, torch.tensor(mel_len), torch.tensor(tokens_len), reduction="none").double()


def _rel(got, want):
    fin = torch.isfinite(want)
    return ((got[fin] - want[fin]).abs() / want[fin].abs()).tolist()


def _results():
    """Every case once: inputs, the fp64 yardstick, torch's fp32 result, the device's nll and mean.  Shared and left unchanged."""
    if not _cache:
        for name, make in ALL_CASES.items():
            logits, tokens, ml, tl = make()
            dl = logits.to(DEV)
            _cache[name] = dict(logits=logits, tokens=tokens, ml=ml, tl=tl, y64=_yardstick(logits, tokens, ml, tl),
                                y32=_yardstick(logits, tokens, ml, tl, torch.float32), nll=A.ctc_loss(dl, tokens, ml, tl, reduction="none").cpu(),
                                mean=A.ctc_loss(dl, tokens, ml, tl).cpu(), total=A.ctc_loss(dl, tokens, ml, tl, reduction="sum").cpu())
        _cache["e_ref"] = max(e for n in BOUND_CASES for e in _rel(_cache[n]["y32"], _cache[n]["y64"]))
    return _cache


@pytest.mark.parametrize("name", list(ALL_CASES))
def test_given_logits_against_the_fp64_yardstick(name):
    res = _results()
    r, e_ref = res[name], res["e_ref"]
    nll, y64 = r["nll"], r["y64"]
    assert nll.dtype == torch.float64 and tuple(nll.shape) == (len(r["ml"]),)
    e_dev, e_t32 = _rel(nll, y64), _rel(r["y32"], y64)
    print(f"CTCPARITY {name}: device max rel err {max(e_dev, default=0.0):.3e}, torch fp32 {max(e_t32, default=0.0):.3e}, "
          f"e_ref (all bound cases) {e_ref:.3e}, nll {y64.tolist()}")
    assert 1e-10 < e_ref < 1e-4  # torch's fp32 run is an fp32 run
    inf = torch.isinf(y64)
    assert torch.equal(torch.isinf(nll), inf) and bool((nll[inf] > 0).all()) and not torch.isnan(nll).any()
    assert all(e <= 2 * e_ref for e in e_dev), (name, e_dev, e_ref)
    # reduction='mean': the fp64 mean of nll / tokens_len in row order, rounded to fp32 once
    s = 0.0
    for v, n in zip(nll.tolist(), r["tl"]):
        s += v / n
    assert r["mean"].dtype == torch.float32 and r["mean"].dim() == 0
    assert np.float32(r["mean"].item()).tobytes() == np.float32(s / len(r["tl"])).tobytes()
    want_mean = float((y64 / torch.tensor(r["tl"], dtype=torch.float64)).mean())
    if math.isfinite(want_mean):
        assert abs(r["mean"].item() - want_mean) <= (2 * e_ref + 2.0 ** -24) * abs(want_mean)
    else:
        assert r["mean"].item() == math.inf
    assert r["total"].dtype == torch.float64 and r["total"].dim() == 0
    assert r["total"].item() == (pytest.approx(float(nll.sum()), rel=1e-14) if math.isfinite(float(nll.sum())) else math.inf)


def test_special_rows():
    res = _results()
    feas, infeas = res["doubled_feasible"], res["doubled_infeasible"]
    assert torch.isfinite(feas["nll"]).all() and torch.isfinite(feas["y64"]).all()  # mel_len = tokens_len + 1 with one repeat: feasible
    assert infeas["nll"][1].item() == math.inf and infeas["y64"][1].item() == math.inf
    for b in (0, 2):  # the other rows of that batch: bit for bit those of the run without the infeasible row
        assert infeas["nll"][b].numpy().tobytes() == feas["nll"][b].numpy().tobytes()
    assert infeas["mean"].item() == math.inf
    assert torch.isfinite(res["ragged_t_eq_n"]["nll"]).all()  # T == N without a repeat: the diagonal path alone
    assert (res["blank_token"]["tokens"][0] == 0).sum() == 3 and torch.isfinite(res["blank_token"]["nll"]).all()
    assert res["smallest"]["nll"].item() == pytest.approx(res["smallest"]["y64"].item(), rel=2 * res["e_ref"])


@pytest.mark.parametrize("name", ["ragged_t_eq_n", "k2"])
def test_nothing_beyond_the_lengths_is_read(name):
    r = _results()[name]
    logits, tokens, ml, tl = r["logits"].clone(), r["tokens"].clone(), r["ml"], r["tl"]
    V = logits.shape[2]
    for b in range(len(ml)):
        logits[b, ml[b]:] = float("nan")
        tokens[b, tl[b]:] = torch.tensor([V + 5, -1] * tokens.shape[1])[:tokens.shape[1] - tl[b]]
    dl = logits.to(DEV)
    got = A.ctc_loss(dl, tokens, ml, tl, reduction="none")
    assert got.cpu().numpy().tobytes() == r["nll"].numpy().tobytes()
    assert A.ctc_loss(dl, tokens, ml, tl).cpu().numpy().tobytes() == r["mean"].numpy().tobytes()
    # two calls are bit-equal
    assert torch.equal(A.ctc_loss(dl, tokens, ml, tl, reduction="none"), got)
    for b in range(len(ml)):
        # a row inside a batch equals that row run alone, given the same logits ...
        alone = A.ctc_loss(dl[b:b + 1], tokens[b:b + 1], ml[b:b + 1], tl[b:b + 1], reduction="none")
        assert alone.cpu().numpy().tobytes() == r["nll"][b:b + 1].numpy().tobytes(), b
        # ... and cut to its own lengths (another block size, another number of states per thread)
        cut = A.ctc_loss(dl[b:b + 1, :ml[b]], tokens[b:b + 1, :tl[b]], ml[b:b + 1], tl[b:b + 1], reduction="none")
        assert cut.cpu().numpy().tobytes() == r["nll"][b:b + 1].numpy().tobytes(), b


def test_errors():
    """No fault is produced on purpose: every case is a status path, refused before a kernel could read through the bad value."""
    logits, tokens, ml, tl = _case(1, 3, 23, 21, 5, 1.0)
    V, T = 21, 23
    dl = logits.to(DEV)
    good = A.ctc_loss(dl, tokens, ml, tl, reduction="none")
    bad = tokens.clone()
    bad[1, 2] = V                                        # a token == V inside the length
    with pytest.raises(ValueError, match="token"):
        A.ctc_loss(dl, bad, ml, tl)
    for bad_len in ([23, 0, 23], [23, T + 1, 23]):       # host-side and device-side lengths alike
        with pytest.raises(ValueError, match="mel_len"):
            A.ctc_loss(dl, tokens, bad_len, tl)
        with pytest.raises(ValueError, match="length"):
            A.ctc_loss(dl, tokens, torch.tensor(bad_len, device=DEV), torch.tensor(tl, device=DEV))
    with pytest.raises(ValueError, match="length"):
        A.ctc_loss(dl, tokens, torch.tensor(ml, device=DEV), torch.tensor([5, 6, 5], device=DEV))
    for val in (float("nan"), float("inf")):
        x = dl.clone()
        x[2, 22, 7] = val                                 # the last real frame of row 2
        with pytest.raises(FloatingPointError, match="logit"):
            A.ctc_loss(x, tokens, ml, tl)
    with pytest.raises(RuntimeError, match="GPU"):       # no CPU path
        A.ctc_loss(logits, tokens, ml, tl)
    with pytest.raises(ValueError, match="reduction"):
        A.ctc_loss(dl, tokens, ml, tl, reduction="batchmean")
    with pytest.raises(_lib.ParrotHipError) as e:        # N over the limit
        A.ctc_loss(dl[:1], torch.ones((1, A.MAX_TOKENS + 1), dtype=torch.int64), [23], [3])
    assert e.value.code == -5
    lib = _lib.lib()
    assert lib.parrot_ctc_workspace_bytes(1, A.MAX_FRAMES + 1, 4) == 0 and lib.parrot_ctc_workspace_bytes(1, 4, A.MAX_TOKENS + 1) == 0
    # the bad row alone is NaN, the call's other rows are computed, and the library is fine afterwards
    nll = torch.empty(3, dtype=torch.float64, device=DEV)
    n_ws = int(lib.parrot_ctc_workspace_bytes(3, T, 5))
    ws = torch.empty(n_ws, dtype=torch.uint8, device=DEV)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)  # noqa: E731
    bd, mld, tld = bad.to(DEV), i32(ml), i32(tl)
    _lib.check(lib.parrot_ctc_loss(A.dptr(dl), A.dptr(bd), A.dptr(mld), A.dptr(tld), 3, T, V, 5, A.dptr(nll), None, A.dptr(ws), n_ws,
                                   A.stream_ptr(torch.device(DEV))))
    assert int(ws[:4].view(torch.int32).item()) == 9
    assert math.isnan(nll[1].item()) and torch.equal(nll[[0, 2]], good[[0, 2]])
    assert torch.equal(A.ctc_loss(dl, tokens, ml, tl, reduction="none"), good)


def _small_model():
    cfg = synth.small_aligner_config()
    sd = synth.synth_aligner_state_dict(cfg, 21, seed=3, gain=14.0)
    model = A.Aligner(16, 21, 32, 32)
    model.load_state_dict(sd)
    return cfg, sd, model.eval().to(DEV)


def test_end_to_end_with_the_model():
    _, _, model = _small_model()
    mel = synth.synth_aligner_mel(3, 60, 16, seed=11).to(DEV)
    ml, tl = [60, 23, 41], [9, 4, 7]
    tokens = _tokens(np.random.Generator(np.random.PCG64(12)), 3, 9, 21)
    logits = model(mel)
    for red in ("none", "mean", "sum"):
        a, b = model.ctc_loss(mel, ml, tokens, tl, reduction=red), A.ctc_loss(logits, tokens, ml, tl, reduction=red)
        assert a.dtype == b.dtype and torch.equal(a, b), red
    nll = A.ctc_loss(logits, tokens, ml, tl, reduction="none").cpu()
    y64 = _yardstick(logits.cpu(), tokens, ml, tl)  # the yardstick on the DEVICE's logits
    e_ref = _results()["e_ref"]
    e_dev = _rel(nll, y64)
    print(f"CTCE2E: device max rel err {max(e_dev):.3e} (bound 2 x {e_ref:.3e}), nll {y64.tolist()}")
    assert torch.isfinite(y64).all() and all(e <= 2 * e_ref for e in e_dev)


LENS = [(37, 9), (52, 14), (20, 25), (45, 6), (31, 8), (28, 5)]  # utt02: fewer frames than tokens, no alignment


def test_driver_in_a_child_process(tmp_path):
    import yaml
    cfg, sd, model = _small_model()
    cfg = synth.small_aligner_config(str(tmp_path / "data"))
    symbols = [chr(ord("a") + i) for i in range(20)]
    data = tmp_path / "data"
    for d in ("mels", "tokens", "checkpoints"):
        (data / d).mkdir(parents=True, exist_ok=True)
    rng = np.random.Generator(np.random.PCG64(5))
    dataset, mels, toks = [], [], []
    for i, (T, N) in enumerate(LENS):
        item = f"utt{i:02d}"
        mels.append(synth.synth_aligner_mel(1, T, 16, seed=20 + i)[0])
        toks.append(torch.from_numpy(rng.integers(1, 21, size=N)))
        np.save(data / "mels" / f"{item}.npy", mels[-1].numpy(), allow_pickle=False)
        np.save(data / "tokens" / f"{item}.npy", toks[-1].numpy(), allow_pickle=False)
        dataset.append({"item_id": item, "mel_len": T, "tokens_len": N})
    with open(data / "dataset.pkl", "wb") as f:
        pickle.dump(dataset, f)
    with open(data / "symbols.pkl", "wb") as f:
        pickle.dump(symbols, f)
    torch.save({"config": cfg, "symbols": symbols, "model": sd}, data / "checkpoints" / "latest_model.pt")
    with open(tmp_path / "config.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    r = subprocess.run([sys.executable, "-m", "parrot_tts_amd.cli.aligner_eval", "--config", str(tmp_path / "config.yaml"), "--batch_size", "3",
                        "--per_item"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert set(line) == {"ctc_loss", "n_items", "n_infeasible", "n_failed", "n_batches", "step", "precision", "items"}
    assert line["n_items"] == 6 and line["n_batches"] == 2 and line["n_failed"] == 0 and line["n_infeasible"] == 1
    assert line["precision"] in ("f16x3", "bf16x6", "f32") and line["step"] == 3  # the checkpoint's 1, and one forward per batch
    want = {}
    for idx in ([0, 1, 2], [3, 4, 5]):  # the same batches, directly
        ml, tl = [LENS[i][0] for i in idx], [LENS[i][1] for i in idx]
        mel = torch.zeros((3, max(ml), 16))
        tokens = torch.zeros((3, max(tl)), dtype=torch.int64)
        for b, i in enumerate(idx):
            mel[b, :ml[b]] = mels[i]
            tokens[b, :tl[b]] = toks[i]
        nll = model.ctc_loss(mel.to(DEV), ml, tokens, tl, reduction="none").cpu().tolist()
        for b, i in enumerate(idx):
            want[f"utt{i:02d}"] = nll[b] / tl[b]
    assert line["items"] == want and want["utt02"] == math.inf
    finite = [v for v in want.values() if math.isfinite(v)]
    assert len(finite) == 5 and line["ctc_loss"] == math.fsum(finite) / 5


def test_whole_file_under_poison():
    """This file once more in a child process under PARROT_POISON_WS=nan: a kernel reading a byte of the workspace or of an
    output that nobody wrote would turn a loss into NaN there."""
    if os.environ.get("PARROT_POISON_WS"):
        return  # (already a poisoned run: the tests above were it)
    env = dict(os.environ, PARROT_POISON_WS="nan")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", os.path.abspath(__file__), "-k", "not whole_file"], cwd=ROOT,
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
