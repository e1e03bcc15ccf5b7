"""CPU: what the vocoder's training path rests on and needs no device -- the restatement (tests/voc_train_ref.py) against the oracle
and against central differences, the share of lrelu inputs that the mask test leaves out, the new entry points in the header, the
export list and the ctypes table, and the size of the saved buffer against the formula of DESIGN.md."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import voc_train_ref as VR  # noqa: E402
from oracle import parrot_oracle as O  # noqa: E402

NEW = ("parrot_voc_train_forward", "parrot_voc_train_backward", "parrot_voc_train_saved_bytes", "parrot_voc_train_workspace_bytes",
       "parrot_voc_train_out_len")
NEW_DEBUG = ("parrot_voc_train_lrelu_sites", "parrot_voc_train_lrelu_site_elems", "parrot_voc_train_lrelu_mask", "parrot_debug_voc_conv_fwd",
             "parrot_debug_voc_conv_dx", "parrot_debug_voc_conv_dw_workspace_bytes", "parrot_debug_voc_conv_dw", "parrot_debug_voc_wn_fwd",
             "parrot_debug_voc_wn_bwd")


@pytest.mark.parametrize("name", ["V1", "V3"])
def test_restatement_without_masks_is_the_oracle_bit_for_bit(name):
    h, sd, batch = VR.make_case(name)
    with torch.no_grad():
        wav, inputs = VR.forward(sd, h, batch)
        want = O.code_generator_forward(sd, h, batch["code"], batch["spkr"])
    assert torch.equal(wav, want) and len(inputs) == VR.n_sites(h)


@pytest.mark.parametrize("name", ["V3", "V4"])
def test_fp64_gradients_agree_with_central_differences(name):
    """Along one random direction per parameter, masks fixed at the base point's: h = 1e-6, to 1e-6 relative plus 1e-9."""
    h, sd, batch = VR.make_case(name)
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        wav, inputs = VR.forward(sd64, h, batch)
    masks = [x > 0 for x in inputs]
    g = torch.Generator().manual_seed(3)
    up = torch.randn(wav.shape, generator=g, dtype=torch.float64)
    _, grads, _, _ = VR.loss_and_grads(sd, h, batch, torch.float64, up, masks)
    eps = 1e-6
    for k in sd:
        d = torch.randn(sd[k].shape, generator=g, dtype=torch.float64)
        vals = []
        for sign in (1, -1):
            p = dict(sd64)
            p[k] = sd64[k] + sign * eps * d
            with torch.no_grad():
                vals.append(float((VR.forward(p, h, batch, masks)[0] * up).sum()))
        num, ana = (vals[0] - vals[1]) / (2 * eps), float((grads[k] * d).sum())
        assert abs(num - ana) <= 1e-6 * abs(ana) + 1e-9, (k, num, ana)


@pytest.mark.parametrize("name", VR.CASES)
def test_the_references_own_fp32_masks_stay_within_the_caps(name):
    in64, in32 = VR.own_inputs(name)
    share, worst = VR.check_caps(VR.excluded(in64, in32, None))
    print(f"{name}: excluded share {share:.2e}, worst site {worst:.2e}")


def test_new_entry_points_are_declared_exported_and_bound():
    from parrot_tts_amd import _lib, build
    build.build()
    raw = C.CDLL(_lib.LIB_PATH)
    for header, names in (("parrot_hip.h", NEW), ("parrot_hip_debug.h", NEW_DEBUG)):
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        for n in names:
            assert re.search(r"\b%s\s*\(" % n, src), f"{n} is not declared in {header}"
            assert hasattr(raw, n), f"{n} is not exported"
            assert n in _lib.SIGNATURES, f"{n} has no ctypes signature"
    assert C.sizeof(_lib.VocLayerPtrs) == 3 * 8
    assert C.sizeof(_lib.VocTrainPtrs) == 8 * (2 + 3 * (1 + _lib.MAX_STAGES + _lib.VOC_TRAIN_MAX_RB + 1))


def saved_bytes_formula(h, B, U):
    """DESIGN.md section 3, "Vocoder generator training": every buffer starts at a multiple of 256 bytes; floats."""
    a256 = lambda n: (4 * n + 255) // 256 * 256  # noqa: E731
    c0, nk = h["upsample_initial_channel"], len(h["resblock_kernel_sizes"])
    per = nk * (6 if str(h["resblock"]) == "1" else 2)
    E = h["embedding_dim"]
    cin0 = E * (2 if h.get("multispkr") else 1)
    total, T, layers = a256(B * cin0 * U), U, [(c0, cin0 * 7)]
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        total += a256(B * (c0 >> i) * T)                      # a_up[i]
        layers.append((c0 >> i, (c0 >> (i + 1)) * k))         # ups[i]: rows are the input channels
        T = (T - 1) * u - 2 * ((k - u) // 2) + k
        total += per * a256(B * (c0 >> (i + 1)) * T)          # the activated input of every resblock conv
    c_last = c0 >> len(h["upsample_rates"])
    total += a256(B * c_last * T) + a256(B * T)               # a_post, y
    for i in range(len(h["upsample_rates"])):
        ch = c0 >> (i + 1)
        for k in h["resblock_kernel_sizes"]:
            layers += [(ch, ch * k)] * (6 if str(h["resblock"]) == "1" else 2)
    layers.append((1, c_last * 7))
    return total + sum(a256(rows) + a256(rows * n) for rows, n in layers)


@pytest.mark.parametrize("name", ["V1", "V5"])
def test_saved_bytes_follow_the_formula(name):
    from parrot_tts_amd import _lib, build
    from parrot_tts_amd.vocoder_train import TrainableCodeGenerator
    build.build()
    h, _, batch = VR.make_case(name)
    cfg = TrainableCodeGenerator(h)._cfg()
    for B, U in (tuple(batch["code"].shape), (16, 28)):
        assert _lib.lib().parrot_voc_train_saved_bytes(C.byref(cfg), B, U) == saved_bytes_formula(h, B, U), (B, U)
    assert _lib.lib().parrot_voc_train_saved_bytes(C.byref(cfg), 0, 3) == 0 and _lib.lib().parrot_voc_train_saved_bytes(C.byref(cfg), 1, 0) == 0
    assert _lib.lib().parrot_voc_train_lrelu_sites(C.byref(cfg)) == VR.n_sites(h) == 96
