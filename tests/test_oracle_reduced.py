"""CPU tests of the reduced-precision emulation (oracle/reduced.py) and a static check of the built library's LDS-DMA loads.

The emulation is what tests/test_gpu_reduced_precision.py holds the bf16 / fp16 kernels to element by element, so its pieces are
pinned here: the roundings against torch's casts, the fp16 weight scale against its rule, the layer classification as a literal
table (a change to the library's plan selection must be made here on purpose), and the unrounded emulation against the oracle."""
import os
import shutil
import struct
import subprocess
import sys
import tempfile

import pytest
import torch

from oracle import parrot_oracle as O
from oracle import reduced as R
from parrot_tts_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_baseline_shapes import NON_DEFAULT_VOC  # noqa: E402  (the config list itself; its tests stay GPU-marked)


def _bits(t):
    return t.to(torch.float32).contiguous().view(torch.int32)


def _crafted():
    v = []
    for e in (-149, -140, -133, -127, -126, -125, -25, -24, -15, -14, -13, -1, 0, 1, 10, 13, 15, 16, 100, 127):
        for m in (1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.5, 1.0 + 2.0 ** -9, 2.0 - 2.0 ** -23):
            v.append(m * 2.0 ** e)
    v += [0.0, 8190.0, 8189.0, 8191.0, 8190.5, 9000.0, 65504.0, 65519.0, 65520.0, 65536.0, 2049.0, 2051.0, 3.0e38, 3.4028234e38,
          2.0 ** -24 * 0.5, 2.0 ** -24 * 1.5, 2.0 ** -27, 2.0 ** -28 * 3, 2.0 ** -126 * (1 - 2.0 ** -9), 1e-6, 1e3]
    x = torch.tensor(v, dtype=torch.float32)
    return torch.cat([x, -x, torch.tensor([float("inf"), -float("inf")])])


def test_round_bf16_matches_torch_cast_on_crafted_values():
    x = _crafted()
    assert torch.equal(_bits(R.round_bf16(x)), _bits(x.to(torch.bfloat16).to(torch.float32)))
    assert float(R.round_bf16(torch.tensor([1.0 + 2.0 ** -8]))) == 1.0                      # tie to even (down)
    assert float(R.round_bf16(torch.tensor([1.0 + 3 * 2.0 ** -8]))) == 1.0 + 2.0 ** -6      # tie to even (up)
    assert torch.isinf(R.round_bf16(torch.tensor([3.4028234e38]))).all()                   # RNE overflows past bf16's maximum
    assert _bits(R.round_bf16(torch.tensor([-0.0]))).item() == _bits(torch.tensor([-0.0])).item()
    g = torch.Generator().manual_seed(1)
    r = torch.randn(200000, generator=g) * torch.exp2(torch.randint(-140, 120, (200000,), generator=g).float())
    assert torch.equal(_bits(R.round_bf16(r)), _bits(r.to(torch.bfloat16).to(torch.float32)))


@pytest.mark.parametrize("scale", [1.0, R.F16_XS, 2.0 ** 14, 2.0 ** -3])
def test_round_f16_matches_torch_cast_on_crafted_values(scale):
    x = _crafted()
    want = ((x * scale).to(torch.float16).to(torch.float32) / scale)
    assert torch.equal(_bits(R.round_f16(x, scale)), _bits(want))
    g = torch.Generator().manual_seed(2)
    r = torch.randn(200000, generator=g) * torch.exp2(torch.randint(-30, 18, (200000,), generator=g).float())
    assert torch.equal(_bits(R.round_f16(r, scale)), _bits((r * scale).to(torch.float16).to(torch.float32) / scale))


def test_round_f16_activation_range_edges():
    """Activations are scaled by 8 before the fp16 rounding: 8189 stays finite, 8190 x 8 = 65520 rounds to inf (ties to even
    past fp16's maximum 65504), and so does everything above."""
    x = torch.tensor([8189.0, 8190.0, 9000.0, -8190.0, 2.0 ** -27, 2.0 ** -28, 3 * 2.0 ** -29])
    y = R.round_f16(x, R.F16_XS)
    assert float(y[0]) == 65504.0 / 8 and torch.isinf(y[1:4]).all()
    assert float(y[4]) == 2.0 ** -27 and float(y[5]) == 0.0 and float(y[6]) == 2.0 ** -27  # the subnormal edge: 2^-24 / 8


def test_round_rtz_truncates():
    x = torch.tensor([1.0 + 2.0 ** -7 - 2.0 ** -20, -(1.0 + 2.0 ** -7 - 2.0 ** -20)])
    assert R.round_rtz(x, "bf16").tolist() == [1.0, -1.0]
    assert R.round_bf16(x).tolist() == [1.0 + 2.0 ** -7, -(1.0 + 2.0 ** -7)]


def test_f16_weight_scale_puts_max_into_2p14_2p15():
    g = torch.Generator().manual_seed(3)
    for mag in torch.logspace(-6, 3, 40).tolist():
        w = torch.randn(64, 64, 3, generator=g) * mag
        s = R.f16_weight_scale(w)
        assert s > 0 and float.hex(s).startswith("0x1.0000000000000p")   # a power of two
        m = float(w.abs().max()) * s
        assert 2.0 ** 14 <= m < 2.0 ** 15, (mag, s, m)
        assert torch.isfinite(R.round_f16(w, s)).all()
    assert R.f16_weight_scale(torch.full((4,), 2.0 ** 14)) == 1.0
    assert R.f16_weight_scale(torch.full((4,), -(2.0 ** 15 - 1))) == 1.0
    assert R.f16_weight_scale(torch.zeros(4)) == 1.0
    assert R.f16_weight_scale(torch.tensor([1.0, float("inf")])) == 1.0


# ----------------------------------------------------------------------------------------------------------------------
# classification: the layers of every shipped / tested vocoder config that stay fp32 in the bf16 / f16 modes.  Everything not
# listed is reduced.  fp32: conv_post (1 output row), the 32 -> 16 k4 u2 ConvTranspose1d (conv_valu.h), every conv with < 32
# GEMM rows or C_in % 16 != 0 -- except the 16-channel ResBlock1 convs, which the fused pair kernels run reduced (fused != 0).
# ----------------------------------------------------------------------------------------------------------------------
_RB_LOW = lambda cs, ks: [("rb", c, c, k) for c in cs for k in ks]  # noqa: E731
FP32_LAYERS = {
    ("default", 0): [("conv", 16, 1, 7), ("convt", 32, 16, 4)] + _RB_LOW([16], [3, 7, 11]),
    ("default", 2): [("conv", 16, 1, 7), ("convt", 32, 16, 4)],
    ("small", 0): [("conv", 2, 1, 7), ("convt", 4, 2, 4), ("convt", 8, 4, 4)] + _RB_LOW([2, 4, 8, 16], [3, 7, 11]),
    ("small", 2): [("conv", 2, 1, 7), ("convt", 4, 2, 4), ("convt", 8, 4, 4)] + _RB_LOW([2, 4, 8], [3, 7, 11]),
    ("non_default_0", 0): [("conv", 8, 1, 7), ("convt", 16, 8, 4), ("convt", 32, 16, 4)] + _RB_LOW([8, 16], [3, 7, 11]),
    ("non_default_0", 2): [("conv", 8, 1, 7), ("convt", 16, 8, 4), ("convt", 32, 16, 4)] + _RB_LOW([8], [3, 7, 11]),
    ("non_default_1", 0): [("conv", 16, 1, 7)] + _RB_LOW([16], [3, 5]),
    ("non_default_1", 2): [("conv", 16, 1, 7)] + _RB_LOW([16], [5]),   # (k = 5: no pair kernel; exact fused / layer kernels)
    ("non_default_2", 0): [("conv", 8, 1, 7), ("convt", 16, 8, 4), ("convt", 32, 16, 4)] + _RB_LOW([8, 16], [3, 7, 11]),
    ("non_default_2", 2): [("conv", 8, 1, 7), ("convt", 16, 8, 4), ("convt", 32, 16, 4)] + _RB_LOW([8], [3, 7, 11]),
}
N_LAYERS = {"default": 97, "small": 97, "non_default_0": 78, "non_default_1": 28, "non_default_2": 97}


def _voc_configs():
    cfgs = {"default": synth.default_voc_config(), "small": synth.small_voc_config()}
    for i, nd in enumerate(NON_DEFAULT_VOC):
        h = synth.small_voc_config()
        h.update(nd)
        cfgs[f"non_default_{i}"] = h
    return cfgs


@pytest.mark.parametrize("name", list(N_LAYERS))
def test_reduced_layer_classifies_every_vocoder_conv(name):
    h = _voc_configs()[name]
    for fused in (0, 1, 2):
        layers = R.vocoder_layers(h, fused)
        assert len(layers) == N_LAYERS[name]
        fp32 = sorted({l[:4] for l in layers if not l[4]})
        assert fp32 == sorted(FP32_LAYERS[(name, 0 if fused == 0 else 2)]), (name, fused, fp32)
        # a layer's class depends on its shape and the fused mode only
        assert len({l[:4] for l in layers if l[4]} & set(fp32)) == 0


def test_reduced_layer_plan_rules():
    """conv_build's split rule and the VALU overrides, branch by branch."""
    assert R.reduced_layer("conv", 256, 512, 7)                            # conv_pre
    assert not R.reduced_layer("conv", 256, 16, 7)                         # < 32 rows
    assert R.reduced_layer("conv", 16, 32, 3)                              # 32 rows, C_in = 16
    assert not R.reduced_layer("conv", 20, 64, 3)                          # C_in % 16 != 0
    assert not R.reduced_layer("conv", 64, 64, 3, pre_slope=1.5)          # slope outside [0, 1]
    assert R.reduced_layer("conv", 64, 64, 3, pre_slope=0.01)
    assert not R.reduced_layer("conv", 64, 64, 3, tile_cfg=0)              # a forced tile runs the exact kernel
    assert R.reduced_layer("convt", 64, 32, 4, 2, padding=1)               # M = 32 x 2 rows
    assert not R.reduced_layer("convt", 32, 16, 4, 2, padding=1)           # convt_valu_kernel
    assert R.reduced_layer("convt", 32, 16, 4, 2, padding=1, valu_kernels=False)
    assert R.reduced_layer("convt", 32, 16, 8, 4, padding=2)               # 64 rows, not the VALU shape
    assert not R.reduced_layer("convt", 8, 4, 8, 4, padding=2)             # C_in = 8
    assert R.reduced_layer("rb", 16, 16, 7, fused=1) and not R.reduced_layer("rb", 16, 16, 7, fused=0)
    assert not R.reduced_layer("rb", 16, 16, 7, fused=2, resblock_type=2)
    assert not R.reduced_layer("rb", 16, 16, 5, fused=2)
    assert R.reduced_layer("rb", 64, 64, 11, fused=0) and R.reduced_layer("rb", 64, 64, 5, fused=2)
    with pytest.raises(ValueError):
        R.reduced_layer("linear", 16, 16, 1)


# ----------------------------------------------------------------------------------------------------------------------
# the emulated forward
# ----------------------------------------------------------------------------------------------------------------------
def test_unrounded_emulation_is_the_oracle_bit_for_bit():
    for h, U, B in ((synth.small_voc_config(), 25, 3), (synth.default_voc_config(), 12, 1)):
        sd = synth.synth_voc_state_dict(h, seed=5)
        b = synth.synth_voc_batch(B, U, h, seed=6)
        st0, st1 = {}, {}
        with torch.no_grad():
            y0 = O.code_generator_forward(sd, h, b["code"], b["spkr"], stages=st0)
        y1 = R.code_generator_forward_reduced(sd, h, b["code"], b["spkr"], None, stages=st1)
        assert torch.equal(y0, y1)
        assert st0.keys() == st1.keys() and all(torch.equal(st0[k], st1[k]) for k in st0)
    assert O.F is torch.nn.functional  # restored


def test_emulation_restores_the_oracle_after_an_exception():
    h = synth.small_voc_config()
    with pytest.raises(RuntimeError):
        with R.reduced_functional(h, "bf16"):
            assert O.F is not torch.nn.functional
            raise RuntimeError("boom")
    assert O.F is torch.nn.functional


@pytest.mark.parametrize("mode", R.MODES)
def test_stage_emulation_rounding_dominates_accumulation_order(mode):
    """Anchored at a common input, a single-conv stage of the reduced emulation moves far more than evaluating it in float32
    instead of float64 does: the margin the GPU tests' teeth assertions rely on.  (Over a whole generator it does not: a rounding
    flip caused by accumulation order moves later roundings by an operand ulp, and the flips compound through the chained convs
    until the two evaluations are as far apart as rounded and unrounded -- hence the GPU tests anchor every stage.)  And the
    stage functions compose to the whole emulated forward, bit for bit."""
    h = synth.small_voc_config()
    sd = synth.synth_voc_state_dict(h, seed=9)
    b = synth.synth_voc_batch(2, 30, h, seed=10)
    st = {}
    y = R.code_generator_forward_reduced(sd, h, b["code"], b["spkr"], mode, torch.float64, stages=st)
    prev = "embed"
    for stage in ["conv_pre"] + [f"{p}{i}" for i in range(5) for p in ("ups", "mrf")] + ["post"]:
        got = R.generator_stage_reduced(sd, h, stage, st[prev], mode, torch.float64)
        assert torch.equal(got, y if stage == "post" else st[stage]), stage
        prev = stage
    for stage, x in (("conv_pre", st["embed"]), ("ups0", st["conv_pre"]), ("ups1", st["mrf0"])):
        y64 = R.generator_stage_reduced(sd, h, stage, x, mode, torch.float64)
        y32 = R.generator_stage_reduced(sd, h, stage, x, mode, torch.float32)
        yf = R.generator_stage_reduced(sd, h, stage, x, None)
        d = float((y32 - y64).abs().max())
        assert float((yf - y64).abs().max()) >= 20 * (4 * d + 2.0 ** -20), stage


# ----------------------------------------------------------------------------------------------------------------------
# static check: one wait state between an M0 write and the LDS-DMA load that reads it
# ----------------------------------------------------------------------------------------------------------------------
def _tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"), "/opt/rocm/llvm/bin"):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    return shutil.which(name)


def _gfx950_code_objects(lib_path):
    """The gfx950 device code objects of every offload bundle in a HIP shared library (one bundle per translation unit):
    '__CLANG_OFFLOAD_BUNDLE__', u64 entry count, then per entry u64 offset (from the bundle start), u64 size, u64 triple length,
    triple."""
    data = open(lib_path, "rb").read()
    magic, out, i = b"__CLANG_OFFLOAD_BUNDLE__", [], 0
    while True:
        i = data.find(magic, i)
        if i < 0:
            return out
        (n,) = struct.unpack_from("<Q", data, i + len(magic))
        p = i + len(magic) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if triple.endswith("gfx950") and size:
                out.append(data[i + off:i + off + size])
        i += len(magic)


def _writes_m0(ins):
    parts = ins.split(None, 1)
    return len(parts) == 2 and parts[0].startswith(("s_", "v_readfirstlane", "v_readlane")) and parts[1].split(",")[0].strip() == "m0"


def m0_hazards(disasm):
    """(function, load) pairs whose closest earlier M0 write is not followed by a wait state before an LDS-DMA load."""
    bad, fn, window, n_loads = [], None, [], 0
    for line in disasm.splitlines():
        if line.endswith(">:"):
            fn, window = line.split("<", 1)[1][:-2], []
            continue
        ins = line.split("//")[0].strip()
        if not ins or fn is None:
            continue
        if ins.startswith("buffer_load_") and ins.endswith(" lds"):
            n_loads += 1
            states = 0
            for prev in reversed(window):
                if _writes_m0(prev):
                    break
                states += int(prev.split()[1]) + 1 if prev.startswith("s_nop") else 1
            else:
                states = 1  # no M0 write in this function before the load
            if states < 1:
                bad.append((fn, ins))
        window.append(ins)
    return bad, n_loads


def test_lds_dma_loads_have_a_wait_state_after_the_m0_write():
    """An SALU write of M0 needs one wait state before a buffer_load ... lds reads it (the operand-plane consumers of
    conv_split16.h issue them from inline asm, where the compiler pads nothing)."""
    from parrot_tts_amd import build
    assert os.path.exists(build.LIB), "build the library first (__graft_entry__.build())"
    objdump = _tool("llvm-objdump")
    assert objdump, "llvm-objdump (ROCm's LLVM) not found"
    cos = _gfx950_code_objects(build.LIB)
    assert cos, "no gfx950 code object in the library"
    bad, n_loads = [], 0
    with tempfile.TemporaryDirectory() as tmp:
        for j, co in enumerate(cos):
            path = os.path.join(tmp, f"co{j}.o")
            with open(path, "wb") as f:
                f.write(co)
            dis = subprocess.run([objdump, "-d", path], capture_output=True, text=True, check=True).stdout
            b, n = m0_hazards(dis)
            bad += b
            n_loads += n
    assert n_loads > 0, "no LDS-DMA load found: the operand-plane consumers are missing from the build"
    assert not bad, f"{len(bad)} LDS-DMA loads read M0 in the instruction after its write, e.g. {bad[:3]}"


def test_m0_hazard_scan_on_crafted_listings():
    hdr = "0000 <k>:\n"
    assert m0_hazards(hdr + "s_mov_b32 m0, s3\nbuffer_load_dwordx4 v1, s[4:7], s2 offen lds\n")[0]
    assert not m0_hazards(hdr + "s_mov_b32 m0, s3\ns_nop 0\nbuffer_load_dwordx4 v1, s[4:7], s2 offen lds\n")[0]
    assert not m0_hazards(hdr + "s_mov_b32 m0, s3\nv_mov_b32 v2, v3\nbuffer_load_dwordx4 v1, s[4:7], s2 offen lds\n")[0]
    assert m0_hazards(hdr + "s_add_i32 m0, s3, 16\nbuffer_load_dword v1, s[4:7], s2 offen lds\n")[0]
