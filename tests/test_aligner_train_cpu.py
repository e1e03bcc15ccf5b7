"""CPU: the test-side restatement of the aligner in training (tests/aligner_train_ref.py) against the goldens recorded from the
reference (tools/make_aligner_train_goldens.py), its eval mode against tests/aligner_ref.py, its gradients against finite
differences; and what of ``TrainableAligner`` and the training driver needs no device."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import aligner_ref as R0  # noqa: E402
import aligner_train_ref as TR  # noqa: E402
from parrot_tts_amd import aligner as A  # noqa: E402
from parrot_tts_amd.cli import aligner_train as CLI  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.mark.parametrize("name", TR.TRAIN_GOLDENS)
def test_restatement_equals_the_reference_goldens(name):
    z, meta = TR.load_golden(GOLD, name)
    shape = meta["shape"]
    sd = TR.golden_state_dict(z)
    sd_now, mel, tokens, ml, tl = TR.make_case(shape)  # the fixture's inputs are the seeded case, bit for bit
    assert sorted(sd) == sorted(sd_now) and all(torch.equal(sd[k], sd_now[k]) for k in sd)
    assert np.array_equal(z["mel"], mel.numpy()) and np.array_equal(z["tokens"], tokens.numpy())
    assert np.array_equal(z["mel_len"], ml.numpy()) and np.array_equal(z["tokens_len"], tl.numpy())
    logits, loss, grads, bufs = TR.loss_and_grads(sd, mel, tokens, ml, tl, torch.float64)
    assert float((logits - torch.from_numpy(z["logits64"])).abs().max()) <= 1e-12
    assert abs(float(loss) - float(z["loss64"])) <= 1e-12
    for k in TR.PARAM_KEYS:
        g = torch.from_numpy(z["grad." + k])
        assert float((grads[k] - g).abs().max()) <= 1e-11 * max(1.0, float(g.abs().max())), k
    for k in TR.BUFFER_KEYS:
        assert float((bufs[k] - torch.from_numpy(z["after." + k])).abs().max()) <= 1e-12, k
    for i in range(3):  # what the reference's module counted in that one step
        assert int(z[f"after.convs.{i}.bnorm.num_batches_tracked"]) == int(sd[f"convs.{i}.bnorm.num_batches_tracked"]) + 1
    assert int(z["after.step"]) == int(sd["step"]) + 1


@pytest.mark.parametrize("shape", ["S1", "S3"])
def test_eval_mode_is_the_inference_restatement(shape):
    sd, mel, *_ = TR.make_case(shape)
    P = {k: v.double() for k, v in sd.items() if v.dim() > 0}
    logits, bufs = TR.forward(P, mel.double(), False)
    # (the same formula in fp64 with BatchNorm associated differently: rounding at 1e-16 of O(1) values through four layers)
    assert float((logits - R0.aligner_forward(sd, mel.double())[0]).abs().max()) <= 1e-12
    assert all(torch.equal(bufs[k], P[k]) for k in TR.BUFFER_KEYS)


def test_one_value_per_channel_raises_as_torch_does():
    sd, mel, *_ = TR.make_case("S3")
    P = {k: v for k, v in sd.items() if v.dim() > 0}
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        TR.forward(P, mel[:, :1], True)
    TR.forward(P, mel, True)  # B = 1, T = 2 runs


def test_gradcheck_at_a_reduced_shape():
    B, T, n_mels, V, H, D = 2, 6, 3, 4, 3, 4
    gen = torch.Generator().manual_seed(3)
    shapes = A.aligner_param_shapes(n_mels, V, H, D)
    P = {k: torch.randn(s, generator=gen, dtype=torch.float64) * 0.5 for k, s in shapes.items()}
    for i in range(3):
        P[f"convs.{i}.bnorm.running_var"] = P[f"convs.{i}.bnorm.running_var"].abs() + 0.5
    mel = torch.randn((B, T, n_mels), generator=gen, dtype=torch.float64)
    w = torch.randn((B, T, V), generator=gen, dtype=torch.float64)
    leaves = [P[k].clone().requires_grad_(True) for k in TR.PARAM_KEYS]

    def f(*params):
        Q = dict(P)
        Q.update(zip(TR.PARAM_KEYS, params))
        return (TR.forward(Q, mel, True)[0] * w).sum()

    assert torch.autograd.gradcheck(f, leaves, eps=1e-6, atol=1e-6, rtol=1e-4)


def test_state_dict_keys_and_shapes_are_the_references():
    n_mels, V, H, D = 24, 13, 32, 48
    m = A.TrainableAligner(n_mels, V, H, D)
    want = {k: tuple(s) for k, s in A.aligner_param_shapes(n_mels, V, H, D).items()}
    want["step"] = ()
    for i in range(3):
        want[f"convs.{i}.bnorm.num_batches_tracked"] = ()
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == want
    assert sorted(k for k, _ in m.named_parameters()) == sorted(TR.PARAM_KEYS)
    assert all(isinstance(p, torch.nn.Parameter) and p.requires_grad for p in m.parameters())
    assert m.training and m.get_step() == 1
    inf = A.Aligner(n_mels, V, H, D)  # a state dict moves freely between the two
    inf.load_state_dict(m.state_dict())
    m.load_state_dict(inf.state_dict())
    ck = {"config": {"audio": {"n_mels": n_mels}, "model": {"lstm_dim": H, "conv_dim": D}}, "symbols": list("abcdefghijkl"), "model": m.state_dict()}
    m2 = A.TrainableAligner.from_checkpoint(ck)
    assert all(torch.equal(a, b) for a, b in zip(m2.state_dict().values(), m.state_dict().values()))


def test_a_cpu_tensor_raises():
    m = A.TrainableAligner(24, 13, 32, 32)
    with pytest.raises(RuntimeError, match="GPU"):
        m(torch.zeros((2, 5, 24)))
    with pytest.raises(RuntimeError, match="GPU"):
        m.eval()(torch.zeros((2, 5, 24)))


def test_sampler_reproduces_the_references_index_order():
    with open(os.path.join(GOLD, "aligner_sampler_order.json")) as f:
        fx = json.load(f)
    order = CLI.BinnedLengthOrder(fx["mel_lens"], fx["batch_size"], 3 * fx["batch_size"])
    for want in fx["epochs"]:  # one Random for the sampler's life: the epochs differ, and each starts from the one before
        got = order.epoch()
        assert got == want
        assert sorted(got) == list(range(len(fx["mel_lens"])))
    assert fx["epochs"][0] != fx["epochs"][1]


def test_checkpoint_dict_has_the_references_keys():
    m = A.TrainableAligner(24, 13, 32, 32)
    optim = torch.optim.Adam(m.parameters(), lr=1e-4)
    config, symbols = {"audio": {"n_mels": 24}, "model": {"lstm_dim": 32, "conv_dim": 32}}, list("abcdefghijkl")
    ck = CLI.checkpoint_dict(m, optim, config, symbols)
    assert sorted(ck) == ["config", "model", "optim", "symbols"]
    assert sorted(ck["model"]) == sorted(m.state_dict()) and ck["config"] is config and ck["symbols"] is symbols
    assert sorted(ck["optim"]) == ["param_groups", "state"]
    A.Aligner.from_checkpoint(ck)  # the inference module reads it


def test_argument_errors_of_the_four_entry_points():
    """The C calls validate before any HIP call, so their argument errors need no device: null arguments, the dimension limits of
    parrot_aligner_forward, B T == 1 in training, training without a saved buffer, a null weight, a workspace that is too small.  The
    pointers handed over are host buffers; none of these paths reads through them."""
    import ctypes as C
    from parrot_tts_amd import _lib, build
    build.build()
    lib = _lib.lib()
    E_INVALID, E_NOMEM, E_UNSUPPORTED = -1, -4, -5
    buf = (C.c_float * 64)()
    ptr = C.cast(buf, C.c_void_p)

    def weights(skip=None):
        w = _lib.AlignerDevWeights()
        for name, kind in w._fields_:
            if name == skip:
                continue
            if kind is C.c_void_p:
                setattr(w, name, ptr.value)
            else:
                for i in range(len(getattr(w, name))):
                    getattr(w, name)[i] = ptr.value
        return w

    cfg = _lib.AlignerCfg(24, 13, 32, 32, 1e-5)
    w, g = weights(), _lib.AlignerGrads()
    n_ws, n_sv = lib.parrot_aligner_train_workspace_bytes(C.byref(cfg), 3, 37), lib.parrot_aligner_train_saved_bytes(C.byref(cfg), 3, 37)
    assert n_ws > n_sv > 0 and n_ws % 256 == 0 and n_sv % 256 == 0
    assert lib.parrot_aligner_train_workspace_bytes(C.byref(cfg), 4, 37) > n_ws
    for bad in (_lib.AlignerCfg(24, 13, 40, 32, 1e-5), _lib.AlignerCfg(24, 13, 32, 24, 1e-5), _lib.AlignerCfg(24, 13, 1040, 32, 1e-5),
                _lib.AlignerCfg(0, 13, 32, 32, 1e-5)):
        assert lib.parrot_aligner_train_workspace_bytes(C.byref(bad), 3, 37) == 0 and lib.parrot_aligner_train_saved_bytes(C.byref(bad), 3, 37) == 0
    for B, T in ((0, 37), (3, 0), (3, 32769), (65536, 1), (65535, 32768)):
        assert lib.parrot_aligner_train_workspace_bytes(C.byref(cfg), B, T) == 0 and lib.parrot_aligner_train_saved_bytes(C.byref(cfg), B, T) == 0
    assert lib.parrot_aligner_train_saved_bytes(None, 3, 37) == 0

    def fwd(cfg_=cfg, w_=w, mel=ptr, B=3, T=37, training=1, logits=ptr, saved=ptr, ws=ptr, ws_bytes=None):
        return lib.parrot_aligner_train_forward(C.byref(cfg_) if cfg_ is not None else None, C.byref(w_) if w_ is not None else None, mel, B, T,
                                                training, logits, saved, ws, n_ws if ws_bytes is None else ws_bytes, None)

    def bwd(cfg_=cfg, w_=w, mel=ptr, saved=ptr, grad=ptr, B=3, T=37, g_=g, ws=ptr, ws_bytes=None):
        return lib.parrot_aligner_train_backward(C.byref(cfg_) if cfg_ is not None else None, C.byref(w_) if w_ is not None else None, mel, saved,
                                                 grad, B, T, C.byref(g_) if g_ is not None else None, ws, n_ws if ws_bytes is None else ws_bytes, None)

    for kw in ({"cfg_": None}, {"w_": None}, {"mel": None}, {"logits": None}, {"ws": None}):
        assert fwd(**kw) == E_INVALID and b"null" in lib.parrot_last_error(), kw
    for kw in ({"cfg_": None}, {"w_": None}, {"mel": None}, {"saved": None}, {"grad": None}, {"g_": None}, {"ws": None}):
        assert bwd(**kw) == E_INVALID and b"null" in lib.parrot_last_error(), kw
    for call in (fwd, bwd):
        assert call(cfg_=_lib.AlignerCfg(24, 13, 40, 32, 1e-5)) == E_UNSUPPORTED and b"multiples of 16" in lib.parrot_last_error()
        assert call(cfg_=_lib.AlignerCfg(24, 13, 1040, 32, 1e-5)) == E_UNSUPPORTED and b"1024" in lib.parrot_last_error()
        assert call(T=32769) == E_UNSUPPORTED and b"32768" in lib.parrot_last_error()
        assert call(B=0) == E_INVALID
        for field in ("conv_w", "bn_var", "w_hh", "lin_b"):
            assert call(w_=weights(skip=field)) == E_INVALID and b"null weight" in lib.parrot_last_error(), field
        assert call(B=1, T=1) == E_INVALID and b"more than 1 value per channel" in lib.parrot_last_error()
        assert call(ws_bytes=n_ws - 256) == E_NOMEM and b"workspace too small" in lib.parrot_last_error()
    assert fwd(saved=None) == E_INVALID and b"saved" in lib.parrot_last_error()  # training keeps its activations somewhere
    assert fwd(B=1, T=1, training=0, saved=None, ws_bytes=0) == E_NOMEM  # (eval has no B T limit and needs no saved buffer: it gets as far as the workspace)
