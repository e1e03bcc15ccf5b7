"""GPU: the aligner's inference kernels on their own (csrc/aligner.h: lstm_step_kernel, align_softmax_kernel, align_dp_kernel) and
lstm_train_step_kernel (csrc/aligner_train.h) beside its inference twin, at the sizes where their loops take a second or a partial
trip.  The recurrence runs through parrot_debug_lstm, which is the step loop of parrot_aligner_forward (kernel 0) or of
parrot_aligner_train_forward (kernel 1) on caller-owned buffers; the softmax through ``Aligner.softmax`` of a tiny model with
num_symbols = V; the dynamic programme through ``align_durations``.  References: tests/aligner_ref.py (``lstm_steps``,
``dp_durations_fast``, ``aligner_forward``), pinned on the CPU by tests/test_aligner_cpu.py, and torch.softmax in fp64.

  * Structure, bit for bit: a batch row run alone, the backward direction against the forward one on reversed input, kernel 0
    against kernel 1, two runs, frames no step owns, rows beside a NaN, the softmax in place and a softmax row run alone, a ragged DP
    call against one-at-a-time calls.  Durations equal the fp64 DP's and the cost is bit-equal to it.
  * Real values: err = max |ours - ref64| over the tensor; yard = max |ref32 - ref64|, ref32 the same restatement in fp32 on the CPU on
    the same inputs; bound = max(4 yard, half an fp32 ulp of the tensor's largest magnitude).  4 is the allowance of
    tests/test_gpu_aligner.py for another fp32 summation order, the floor is the one of tests/test_gpu_aligner_train.py.  Every case
    prints err, yard and their ratio; the last test prints the largest ratio per kernel (DESIGN.md section 4 records them).
  * One step with exact pre-activations: w_hh in {0, +-1/4}, h0 multiples of 1/8 in [-1, 1], xproj multiples of 1/16: every product is
    a multiple of 1/32 and every partial sum stays below 4, so the H-term sum is the same number in fp32 and fp64 in whatever order,
    and the whole error is expf / tanhf.  A dropped or doubled term moves a gate by at least sigmoid'(4) / 32 = 5.5e-4.

The whole file also passes under PARROT_POISON_WS=nan (workspaces, h_n / c_n, pred, dur and cost filled with NaN first)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import aligner_ref as R  # noqa: E402
from parrot_tts_amd import _lib, ops, synth  # noqa: E402
from parrot_tts_amd import aligner as A  # noqa: E402

DEV = "cuda:0"
FACTOR = 4.0
SENT = -7777.0
KERNELS = [0, 1]  # parrot_debug_lstm: 0 lstm_step_kernel (8 batch rows per pass), 1 lstm_train_step_kernel (16)
RATIOS = {}  # kernel -> (largest err / yard seen, where)


def _rng(*seed):
    return np.random.Generator(np.random.PCG64(list(seed)))


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _held(kernel, name, ours, ref32, ref64, factor=FACTOR):
    """Print the figures, then hold ``ours`` to the rule of the module docstring.  Returns err / yard."""
    ours, ref32, ref64 = ours.detach().cpu().double(), ref32.double(), ref64.double()
    err, yard = float((ours - ref64).abs().max()), float((ref32 - ref64).abs().max())
    floor = float(np.spacing(np.float32(ref64.abs().max().item()))) / 2
    bound = max(factor * yard, floor)
    ratio = err / yard if yard > 0 else 0.0
    print(f"{kernel} {name}: err {err:.3e}  yard {yard:.3e}  ratio {ratio:.2f}  floor {floor:.3e}")
    if yard > 0 and ratio > RATIOS.get(kernel, (0.0, ""))[0]:
        RATIOS[kernel] = (ratio, name)
    assert np.isfinite(err) and err <= bound, (kernel, name, err, bound, yard, floor)
    return ratio


def _same(a, b):
    """Bit-equal fp32 tensors (a NaN equals the same NaN, -0 differs from +0)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# =========================================================================================================================================
# the LSTM recurrence
# =========================================================================================================================================
# H: 16 one trip of the k-loop with only lanes q < 4; 48 one partial trip; 80 two trips, the second partial; 128 two full trips; 1024
# the limit.  B: 1 a partial pass; 8 one full pass of kernel 0; 9 its second pass of one row; 17 its third pass of one row and the
# second pass of one row of kernel 1.
LSTM_SHAPES = [(16, 1, 1), (16, 8, 2), (16, 9, 5), (16, 17, 2), (48, 1, 2), (48, 8, 5), (48, 9, 1), (48, 17, 5), (80, 1, 5), (80, 8, 1),
               (80, 9, 2), (80, 17, 5), (128, 1, 1), (128, 8, 5), (128, 9, 2), (128, 17, 1), (1024, 9, 2)]
_lstm_cases = {}


def _lstm_inputs(H, B, T, seed=0):
    rng = _rng(41, H, B, T, seed)
    w_hh = _f32(rng.standard_normal((2, 4 * H, H)) / np.sqrt(H))
    xproj = _f32(rng.standard_normal((B, T, 8 * H)))
    h0 = _f32(np.tanh(rng.standard_normal((2, B, H))))
    c0 = _f32(rng.standard_normal((2, B, H)))
    return w_hh, xproj, h0, c0


def _run(kernel, w_hh, xproj, h0=None, c0=None, n_steps=None, out=None):
    d = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    return ops.debug_lstm(d(w_hh), d(xproj), kernel, d(h0), d(c0), n_steps, out)


def _lstm_case(shape):
    """Inputs, the fp64 and fp32 restatements from a zero state, and both kernels' runs of one shape, computed once."""
    if shape not in _lstm_cases:
        w_hh, xproj, h0, c0 = _lstm_inputs(*shape)
        names = ("out", "h_n", "c_n", "gates", "c_all")
        ref = {dt: dict(zip(names, R.lstm_steps(w_hh, xproj, None, None, None, dt))) for dt in (torch.float64, torch.float32)}
        _lstm_cases[shape] = (w_hh, xproj, h0, c0, ref, {k: _run(k, w_hh, xproj) for k in KERNELS})
    return _lstm_cases[shape]


@pytest.mark.parametrize("shape", LSTM_SHAPES, ids=lambda s: "H%d-B%d-T%d" % s)
def test_lstm_full_recurrence_against_fp64(shape):
    """Gaussian W_hh / sqrt(H) and gaussian xproj from a zero state: every element of out, h_n, c_n (and gates, c_all of kernel 1)."""
    *_, ref, ours = _lstm_case(shape)
    for k in KERNELS:
        for name in ("out", "h_n", "c_n") + (("gates", "c_all") if k == 1 else ()):
            _held(f"lstm kernel {k}", "H%d-B%d-T%d %s" % (*shape, name), ours[k][name], ref[torch.float32][name], ref[torch.float64][name])


@pytest.mark.parametrize("shape", LSTM_SHAPES, ids=lambda s: "H%d-B%d-T%d" % s)
def test_lstm_kernels_agree_bit_for_bit_and_so_do_two_runs(shape):
    """lstm_train_step_kernel makes "the same order of every sum" as lstm_step_kernel (csrc/aligner_train.h): out, h_n and c_n are the
    same bits on every shape, from a zero state and from a given one; and out is [h], c_all its cell states."""
    w_hh, xproj, h0, c0, _, zero = _lstm_case(shape)
    H, B, T = shape
    given = {k: _run(k, w_hh, xproj, h0, c0) for k in KERNELS}
    for runs in (zero, given):
        for name in ("out", "h_n", "c_n"):
            assert _same(runs[0][name], runs[1][name]), name
        assert _same(runs[1]["h_n"][0], runs[1]["out"][:, T - 1, :H]) and _same(runs[1]["h_n"][1], runs[1]["out"][:, 0, H:])
        assert _same(runs[1]["c_n"][0], runs[1]["c_all"][:, T - 1, :H]) and _same(runs[1]["c_n"][1], runs[1]["c_all"][:, 0, H:])
    assert not _same(zero[0]["out"], given[0]["out"])  # (the given state is read)
    for k in KERNELS:
        again = _run(k, w_hh, xproj, h0, c0)
        for name in again:
            assert _same(again[name], given[k][name]), (k, name)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("H", [16, 48, 80, 128])
def test_lstm_row_does_not_depend_on_its_batch(H, kernel):
    """Rows 0, 7, 8, 15, 16 of a B = 17 run (first and last row of a pass of either kernel, and the one-row passes) equal the same
    row run alone at B = 1, bit for bit, in every output."""
    T = 2
    w_hh, xproj, h0, c0 = _lstm_inputs(H, 17, T, seed=1)
    full = _run(kernel, w_hh, xproj, h0, c0)
    for b in (0, 7, 8, 15, 16):
        alone = _run(kernel, w_hh, xproj[b:b + 1], h0[:, b:b + 1].contiguous(), c0[:, b:b + 1].contiguous())
        for name in alone:
            want = full[name][:, b:b + 1] if name in ("h_n", "c_n") else full[name][b:b + 1]
            assert _same(alone[name], want), (b, name)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("shape", [(48, 9, 5), (80, 17, 5), (128, 8, 2)], ids=lambda s: "H%d-B%d-T%d" % s)
def test_lstm_backward_direction_is_the_forward_one_on_reversed_input(shape, kernel):
    H, B, T = shape
    w_hh, xproj, h0, c0 = _lstm_inputs(H, B, T, seed=2)
    w_hh[1] = w_hh[0]
    xproj[..., 4 * H:] = xproj[..., :4 * H].flip(1)
    h0[1], c0[1] = h0[0], c0[0]
    got = _run(kernel, w_hh, xproj, h0, c0)
    assert _same(got["out"][..., H:], got["out"][..., :H].flip(1).contiguous())
    assert _same(got["h_n"][1], got["h_n"][0]) and _same(got["c_n"][1], got["c_n"][0])
    if kernel == 1:
        assert _same(got["gates"][..., 4 * H:], got["gates"][..., :4 * H].flip(1).contiguous())
        assert _same(got["c_all"][..., H:], got["c_all"][..., :H].flip(1).contiguous())


@pytest.mark.parametrize("kernel", KERNELS)
def test_lstm_fewer_steps_leave_the_other_frames_alone(kernel):
    """n_steps = 2 of T = 5: the forward direction owns frames 0, 1 and the backward one frames 4, 3; they hold what the full run
    holds there, h_n / c_n are the state after step 1, and every other element of out keeps the caller's sentinel."""
    H, B, T, n = 80, 9, 5, 2
    w_hh, xproj, h0, c0 = _lstm_inputs(H, B, T, seed=3)
    full = _run(kernel, w_hh, xproj, h0, c0)
    out = torch.full((B, T, 2 * H), SENT, dtype=torch.float32, device=DEV)
    part = _run(kernel, w_hh, xproj, h0, c0, n_steps=n, out=out)
    assert part["out"] is out
    assert _same(out[:, :n, :H], full["out"][:, :n, :H]) and _same(out[:, T - n:, H:], full["out"][:, T - n:, H:])
    assert bool((out[:, n:, :H] == SENT).all()) and bool((out[:, :T - n, H:] == SENT).all())
    assert _same(part["h_n"][0], full["out"][:, n - 1, :H]) and _same(part["h_n"][1], full["out"][:, T - n, H:])
    if kernel == 1:
        assert _same(part["c_n"][0], full["c_all"][:, n - 1, :H]) and _same(part["c_n"][1], full["c_all"][:, T - n, H:])
        assert _same(part["gates"][:, :n, :4 * H], full["gates"][:, :n, :4 * H]) and _same(part["gates"][:, T - n:, 4 * H:], full["gates"][:, T - n:, 4 * H:])
    # the state handed on: the remaining three steps from (h_n, c_n) are the full run's
    rest = torch.cat([xproj[:, n:, :4 * H], xproj[:, :T - n, 4 * H:]], dim=-1).contiguous()
    cont = _run(kernel, w_hh, rest, part["h_n"].cpu(), part["c_n"].cpu())
    assert _same(cont["out"][..., :H], full["out"][:, n:, :H]) and _same(cont["out"][..., H:], full["out"][:, :T - n, H:])
    assert _same(cont["h_n"], full["h_n"]) and _same(cont["c_n"], full["c_n"])


def _exact_case(H, B):
    """One step whose H-term sums are exact in any order (module docstring).  Weight row (direction d, gate g, unit u) belongs to
    thread row c = 4 g + u % 4 of its workgroup and is the (u // 4)-th row that thread row sees; its 8 non-zeros sit at
    k = 8 (u // 4) + m + 3 c + 5 d (mod H), m < 8: over u // 4 = 0 .. H / 4 - 1 that is every k exactly twice per (c, d), so every
    (k-lane, trip) slot and every position inside a float4 of every thread row is hit."""
    rng = _rng(43, H, B)
    w = np.zeros((2, 4, H, H), np.float32)
    for d in range(2):
        for g in range(4):
            for u in range(H):
                k = (8 * (u // 4) + np.arange(8) + 3 * (4 * g + u % 4) + 5 * d) % H
                w[d, g, u, k] = rng.choice([-0.25, 0.25], size=8)
    for d in range(2):
        for c in range(16):
            hits = (w[d, c // 4, (c % 4)::4] != 0).sum(axis=0)
            assert hits.shape == (H,) and (hits == 2).all()
    w_hh = _f32(w.reshape(2, 4 * H, H))
    h0 = _f32(rng.choice(np.r_[-8:0, 1:9], size=(2, B, H)) / 8.0)
    c0 = _f32(rng.integers(-16, 17, size=(2, B, H)) / 8.0)
    xproj = _f32(rng.integers(-32, 33, size=(B, 2, 8 * H)) / 16.0)
    return w_hh, xproj, h0, c0


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("H, B", [(16, 17), (48, 17), (80, 17), (128, 17), (1024, 9)])
def test_lstm_one_step_with_exact_preactivations(H, B, kernel):
    """Measured on the MI355X: DESIGN.md section 4."""
    w_hh, xproj, h0, c0 = _exact_case(H, B)
    pre64, pre32 = R.lstm_preactivations(w_hh, xproj, h0, torch.float64), R.lstm_preactivations(w_hh, xproj, h0, torch.float32)
    assert torch.equal(pre32.double(), pre64) and float(pre64.abs().max()) <= 4.0
    assert torch.equal(pre64 * 32, torch.round(pre64 * 32)) and float((h0 @ w_hh.transpose(1, 2)).abs().max()) > 0.5
    names = ("out", "h_n", "c_n", "gates", "c_all")
    ref = {dt: dict(zip(names, R.lstm_steps(w_hh, xproj, h0, c0, 1, dt))) for dt in (torch.float64, torch.float32)}
    got = _run(kernel, w_hh, xproj, h0, c0, n_steps=1)
    own = torch.zeros(B, 2, 8 * H, dtype=torch.bool)  # the gates step 0 owns: forward at frame 0, backward at frame 1
    own[:, 0, :4 * H] = True
    own[:, 1, 4 * H:] = True
    for name in (("gates",) if kernel == 1 else ()) + ("c_n", "h_n"):
        pick = (lambda t: t[own]) if name == "gates" else (lambda t: t)
        _held(f"lstm kernel {kernel}, exact sums", f"H{H}-B{B} {name}", pick(got[name].cpu()), pick(ref[torch.float32][name]), pick(ref[torch.float64][name]))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("b", [8, 16])
def test_lstm_confines_a_nan_to_its_row(b, kernel):
    """A NaN in xproj[b, 0, unit] (forward direction, step 0) spreads through W_hh to every forward unit of row b at step 1 and to
    no other row: rows that share b's batch pass, and the passes after it, keep the bits of the clean run."""
    H, B, T = 80, 17, 2
    w_hh, xproj, h0, c0 = _lstm_inputs(H, B, T, seed=4)
    clean = _run(kernel, w_hh, xproj, h0, c0)
    bad = xproj.clone()
    bad[b, 0, 2 * H + 37] = float("nan")
    got = _run(kernel, w_hh, bad, h0, c0)
    others = [r for r in range(B) if r != b]
    for name in got:
        assert bool(torch.isfinite(clean[name]).all()), name
        rows = (lambda t: t[:, others]) if name in ("h_n", "c_n") else (lambda t: t[others])
        assert _same(rows(got[name]), rows(clean[name])), name
    assert bool(torch.isnan(got["out"][b, 1, :H]).all()) and bool(torch.isnan(got["h_n"][0, b]).all()) and bool(torch.isnan(got["c_n"][0, b]).all())
    assert _same(got["out"][b, :, H:], clean["out"][b, :, H:])  # (the backward direction of row b never sees it)


def test_lstm_refusals():
    """Every refusal of parrot_debug_lstm, on real buffers: nothing is launched, so every output keeps its fill.  An accepted call works
    afterwards."""
    lib = _lib.lib()
    H, B, T = 16, 2, 3
    w_hh, xproj, h0, c0 = (t.to(DEV) for t in _lstm_inputs(H, B, T, seed=5))
    outs = {k: torch.full(n, SENT, dtype=torch.float32, device=DEV)
            for k, n in (("out", (B, T, 2 * H)), ("h_n", (2, B, H)), ("c_n", (2, B, H)), ("gates", (B, T, 8 * H)), ("c_all", (B, T, 2 * H)))}
    need = int(lib.parrot_debug_lstm_workspace_bytes(B, T, H, 0))
    assert need >= 3 * 2 * B * H * 4 and need == int(lib.parrot_debug_lstm_workspace_bytes(B, T, H, 1))
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    p = ops.dptr

    def call(**over):
        a = dict(w_hh=p(w_hh), xproj=p(xproj), h0=p(h0), c0=p(c0), B=B, T=T, H=H, n_steps=T, kernel=1, out=p(outs["out"]), h_n=p(outs["h_n"]),
                 c_n=p(outs["c_n"]), gates=p(outs["gates"]), c_all=p(outs["c_all"]), ws=p(ws), ws_bytes=need)
        a.update(over)
        with torch.cuda.device(DEV):
            return lib.parrot_debug_lstm(a["w_hh"], a["xproj"], a["h0"], a["c0"], a["B"], a["T"], a["H"], a["n_steps"], a["kernel"], a["out"],
                                         a["h_n"], a["c_n"], a["gates"], a["c_all"], a["ws"], a["ws_bytes"], ops.stream_ptr(DEV))

    INVALID, UNSUPPORTED = -1, -5
    cases = [(dict(w_hh=None), INVALID), (dict(xproj=None), INVALID), (dict(out=None), INVALID), (dict(h_n=None), INVALID),
             (dict(c_n=None), INVALID), (dict(ws=None), INVALID), (dict(h0=None), INVALID), (dict(c0=None), INVALID),
             (dict(gates=None), INVALID), (dict(c_all=None), INVALID), (dict(kernel=0), INVALID),  # (kernel 0 keeps no gates / c_all)
             (dict(kernel=2), INVALID), (dict(kernel=-1), INVALID),
             (dict(B=0), INVALID), (dict(B=-3), INVALID), (dict(T=0), INVALID), (dict(H=0), INVALID), (dict(n_steps=0), INVALID),
             (dict(n_steps=-1), INVALID), (dict(n_steps=T + 1), INVALID),
             (dict(H=24), UNSUPPORTED), (dict(H=8), UNSUPPORTED), (dict(H=1040), UNSUPPORTED), (dict(B=65536), UNSUPPORTED),
             (dict(T=32769, n_steps=1), UNSUPPORTED), (dict(ws_bytes=need - 1), UNSUPPORTED), (dict(ws_bytes=0), UNSUPPORTED)]
    for over, code in cases:
        assert call(**over) == code, over
        assert lib.parrot_last_error().startswith(b"debug_lstm"), over
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert bool((t == SENT).all()), k
    for args in ((0, T, H, 0), (B, 0, H, 0), (B, T, 24, 0), (B, T, 1040, 1), (65536, T, H, 0), (B, T, H, 2), (B, 32769, H, 0)):
        assert lib.parrot_debug_lstm_workspace_bytes(*args) == 0, args
    assert call() == 0 and call(kernel=0, gates=None, c_all=None, h0=None, c0=None) == 0
    want = R.lstm_steps(w_hh.cpu(), xproj.cpu(), None, None, None, torch.float64)[0]
    assert float((outs["out"].cpu().double() - want).abs().max()) < 1e-5


# =========================================================================================================================================
# align_softmax_kernel
# =========================================================================================================================================
SOFTMAX_V = [1, 2, 63, 64, 65, 129, 300]  # one lane; two; a wave less one; a full wave; a second trip of one lane; a third; five trips
SM_B, SM_T, SM_LEN = 3, 7, [7, 1, 4]  # B T = 21 rows: the last workgroup holds one; mel_len: T, 1 and a value in between
_sm_models = {}


def _sm_model(V):
    if V not in _sm_models:
        _sm_models[V] = A.Aligner(16, V, 16, 16).eval().to(DEV)
    return _sm_models[V]


def _sm_logits(V, draw):
    rng = _rng(47, V, ["gaussian", "peaky", "shifted", "equal"].index(draw))
    x = rng.standard_normal((SM_B, SM_T, V))
    if draw == "peaky":
        x = x * 30.0
    elif draw == "shifted":
        x = x + 1e4
    elif draw == "equal":
        x = np.repeat(rng.standard_normal((SM_B, SM_T, 1)) * 5.0, V, axis=2)
    x = _f32(x)
    for b, n in enumerate(SM_LEN):
        x[b, n:] = float("nan")  # frames at or beyond mel_len are never examined
    return x


@pytest.mark.parametrize("draw", ["gaussian", "peaky", "shifted", "equal"])
@pytest.mark.parametrize("V", SOFTMAX_V)
def test_softmax_against_fp64_and_its_structure(V, draw):
    model = _sm_model(V)
    x = _sm_logits(V, draw)
    xd = x.to(DEV)
    pred = model.softmax(xd, SM_LEN)  # (check=True: a status other than 0 raises, the NaN of the padding included)
    real = torch.zeros(SM_B, SM_T, dtype=torch.bool)
    for b, n in enumerate(SM_LEN):
        real[b, :n] = True
    assert bool((pred.cpu()[~real].view(torch.int32) == 0).all())  # padding frames: +0.0
    ref64, ref32 = torch.softmax(x[real].double(), -1), torch.softmax(x[real], -1)
    _held("softmax", f"V{V} {draw}", pred.cpu()[real], ref32, ref64)
    assert float((pred.cpu()[real].double().sum(-1) - 1).abs().max()) <= 1e-6
    if V == 1:
        assert bool((pred.cpu()[real] == 1.0).all())
    # in place
    buf, ml = xd.clone(), torch.tensor(SM_LEN, dtype=torch.int32, device=DEV)
    dev = torch.device(DEV)
    with torch.cuda.device(dev):
        h = model._current_handle(dev)
        _lib.check(_lib.lib().parrot_align_softmax(h, A.dptr(buf), A.dptr(ml), SM_B, SM_T, A.dptr(buf), A.stream_ptr(dev)))
        _lib.check(_lib.lib().parrot_aligner_check(h, A.stream_ptr(dev)))
    assert _same(buf, pred)
    # a row alone: another wave of another workgroup
    for b, n in enumerate(SM_LEN):
        assert _same(model.softmax(xd[b:b + 1], [n]), pred[b:b + 1]), b
    assert _same(model.softmax(xd, SM_LEN), pred)


# =========================================================================================================================================
# align_dp_kernel
# =========================================================================================================================================
DP_V = 70
# (T, N): an anti-diagonal of 255, 256 and 257 cells (one trip less a lane, one full trip, a second trip of one lane); three trips;
# the limit N = 2048 with more frames than tokens; more tokens than frames (jlo > 0 in later trips); one frame; one token
DP_SHAPES = [(300, 255), (300, 256), (300, 257), (700, 600), (2100, 2048), (40, 300), (1, 300), (300, 1)]
DP_CASES = [("planted", T, N) for T, N in DP_SHAPES] + [(kind, T, N) for kind in ("uniform", "saturated") for T, N in ((300, 257), (40, 300))]
RAGGED = [("saturated", 300, 257), ("planted", 700, 600), ("planted", 2100, 2048), ("uniform", 40, 300), ("planted", 1, 300), ("planted", 300, 1)]
_dp_cases = {}


def _planted_pred(rng, T, N, V, tokens, boost=5.0):
    """pred (T, V) around a planted monotonic alignment, frame i belonging to token a(i) (tools/make_aligner_goldens.py planted_pred,
    restated)."""
    cuts = np.sort(rng.choice(np.arange(1, T), size=min(N, T) - 1, replace=False)) if min(N, T) > 1 else np.array([], int)
    a = np.searchsorted(cuts, np.arange(T), side="right")
    if N > T:  # more tokens than frames: some tokens are passed by right moves
        a = np.sort(rng.choice(np.arange(N), size=T, replace=False))
        a[-1] = N - 1
    logits = rng.standard_normal(size=(T, V))
    logits[np.arange(T), tokens[a]] += boost
    return torch.softmax(_f32(logits), dim=-1).numpy()


def _dp_case(case):
    """(tokens (N,), pred (T, V), reference durations, reference cost) of one case, computed once."""
    if case not in _dp_cases:
        kind, T, N = case
        rng = _rng(53, ["planted", "uniform", "saturated"].index(kind), T, N)
        tokens = rng.integers(1, DP_V, size=N).astype(np.int64)
        if kind == "planted":
            pred = _planted_pred(rng, T, N, DP_V, tokens)
        elif kind == "uniform":  # every cell tied: the tie rule alone decides, across j = 255 | 256 too
            pred = np.full((T, DP_V), 1.0 / DP_V, np.float32)
        else:  # w exactly 0 or 1
            pred = np.zeros((T, DP_V), np.float32)
            pred[np.arange(T), rng.integers(0, DP_V, size=T)] = 1.0
            assert set(np.unique(R.path_weights(tokens, pred)).tolist()) == {0.0, 1.0}
        dur, cost = R.dp_durations_fast(tokens, pred)
        _dp_cases[case] = (tokens, pred, dur, cost)
    return _dp_cases[case]


def _bits(x):
    return np.float64(x).tobytes()


def _dp_alone(case):
    tokens, pred, _, _ = _dp_case(case)
    dur, cost = A.align_durations(torch.from_numpy(pred).to(DEV)[None], torch.from_numpy(tokens)[None], [pred.shape[0]], [tokens.shape[0]])
    return dur[0].cpu().numpy(), float(cost[0])


@pytest.mark.parametrize("case", DP_CASES, ids=lambda c: "%s-T%d-N%d" % c)
def test_dp_against_the_fp64_programme(case):
    tokens, pred, dur_ref, cost_ref = _dp_case(case)
    dur, cost = _dp_alone(case)
    assert dur.dtype == np.int32 and int(dur.sum()) == pred.shape[0]
    assert _bits(cost) == _bits(cost_ref), (cost, cost_ref)
    bad = np.flatnonzero(dur != dur_ref)
    assert bad.size == 0, (bad[:8], dur[bad[:8]], dur_ref[bad[:8]])


def test_dp_ragged_call_at_a_wide_stride():
    """Six rows in one call at row stride N = 2048 and T = 2100, far above most rows' own lengths.  The padding is hostile: pred
    beyond mel_len[b] is NaN, tokens beyond tokens_len[b] are V (refused if read).  Equal to the one-at-a-time calls, status 0 (no
    exception), dur zero beyond tokens_len."""
    B, T, N = len(RAGGED), 2100, 2048
    pred = np.full((B, T, DP_V), np.nan, np.float32)
    tokens = np.full((B, N), DP_V, np.int64)
    for b, case in enumerate(RAGGED):
        tk, p, _, _ = _dp_case(case)
        pred[b, :p.shape[0]] = p
        tokens[b, :tk.shape[0]] = tk
    ml, tl = [c[1] for c in RAGGED], [c[2] for c in RAGGED]
    dur, cost = A.align_durations(torch.from_numpy(pred).to(DEV), torch.from_numpy(tokens), ml, tl)
    dur, cost = dur.cpu().numpy(), cost.cpu().numpy()
    for b, case in enumerate(RAGGED):
        _, _, dur_ref, cost_ref = _dp_case(case)
        d1, c1 = _dp_alone(case)
        assert np.array_equal(dur[b, :tl[b]], d1) and np.array_equal(d1, dur_ref) and not dur[b, tl[b]:].any(), case
        assert int(dur[b].sum()) == ml[b], case
        assert _bits(cost[b]) == _bits(c1) == _bits(cost_ref), case


# =========================================================================================================================================
# the whole model at edge shapes: the epilogue and the transposes around the kernels above
# =========================================================================================================================================
EDGE = dict(n_mels=24, conv_dim=48, lstm_dim=48, V=65)
_edge = {}


def _edge_sd():
    if "sd" not in _edge:
        cfg = synth.default_aligner_config()
        cfg["audio"]["n_mels"] = EDGE["n_mels"]
        cfg["model"].update(lstm_dim=EDGE["lstm_dim"], conv_dim=EDGE["conv_dim"])
        _edge["sd"] = synth.synth_aligner_state_dict(cfg, EDGE["V"], seed=61, gain=2.0)
    return _edge["sd"]


def _edge_model(precision):
    if precision not in _edge:
        m = A.Aligner(EDGE["n_mels"], EDGE["V"], EDGE["lstm_dim"], EDGE["conv_dim"], precision=precision)
        m.load_state_dict(_edge_sd())
        _edge[precision] = m.eval().to(DEV)
    return _edge[precision]


def _edge_ref(B, T):
    """mel, the fp64 restatement and d_ref = the fp32 restatement's distance from it, per stage, computed once per shape."""
    if (B, T) not in _edge:
        mel = synth.synth_aligner_mel(B, T, EDGE["n_mels"], seed=62 + B + T)
        l64, st64 = R.aligner_forward(_edge_sd(), mel.double())
        l32, st32 = R.aligner_forward(_edge_sd(), mel)
        ref = dict(st64, logits=l64)
        d_ref = {k: float((dict(st32, logits=l32)[k].double() - ref[k]).abs().max()) for k in ref}
        assert all(v > 0 for v in d_ref.values())
        _edge[(B, T)] = (mel, ref, d_ref)
    return _edge[(B, T)]


@pytest.mark.parametrize("precision", ["f16x3", "bf16x6", "f32"])
@pytest.mark.parametrize("B, T", [(9, 1), (9, 33), (17, 5)])
def test_whole_model_at_edge_shapes(B, T, precision):
    """conv_dim = lstm_dim = 48 and V = 65 (partial tiles of every transpose, a partial k trip of the recurrence), B = 9 and 17 (second
    and third batch pass), T = 1, 5 and 33: bn3, lstm and the logits within 4 x d_ref of the fp64 restatement, the rule of
    tests/test_gpu_aligner.py test_stage_and_logit_parity with d_ref computed here."""
    mel, ref, d_ref = _edge_ref(B, T)
    logits, st = _edge_model(precision)(mel.to(DEV), stages=True)
    got = dict(st, logits=logits)
    ratios = {k: float((got[k].cpu().double() - ref[k]).abs().max()) / d_ref[k] for k in ("bn3", "lstm", "logits")}
    print(f"ALIGNEDGE B{B}-T{T} {precision}: " + " ".join(f"{k} {v:.2f} x d_ref ({d_ref[k]:.2e})" for k, v in ratios.items()))
    for k, v in ratios.items():
        if v > RATIOS.get(f"whole model {k}", (0.0, ""))[0]:
            RATIOS[f"whole model {k}"] = (v, f"B{B}-T{T} {precision}")
        assert v <= 4.0, (k, v)


def test_report_ratios():
    for k in sorted(RATIOS):
        print(f"largest over this run, {k}: {RATIOS[k][0]:.2f} ({RATIOS[k][1]})")


def test_whole_file_under_poison():
    """This file once more in a child process under PARROT_POISON_WS=nan: a kernel reading a byte nobody wrote would turn a state, a
    probability, a cost or a duration into NaN / garbage there."""
    if os.environ.get("PARROT_POISON_WS"):
        return  # (already a poisoned run: the tests above were it)
    env = dict(os.environ, PARROT_POISON_WS="nan")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-x", os.path.abspath(__file__), "-k", "not whole_file"], cwd=ROOT,
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
