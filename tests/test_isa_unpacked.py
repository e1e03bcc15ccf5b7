"""The split-scheme MFMA kernels carry no packed-fp32 arithmetic and no scratch (checked in the gfx950 ISA, not in the source).

A v_pk_{mul,add,fma}_f32 beside MFMAs costs more vector issue than the two scalar ops it replaces (DESIGN.md section 7,
tools/probes/interleave_unpacked.hip), and hipcc's SLP vectoriser forms them from adjacent scalar fp32 ops at -O3: the units of
these kernels are built with -fno-slp-vectorize (build.py TU_FLAGS) and their conversion code is written with scalar multiplies.
The units are compiled here to assembly with build.py's own flags; needs hipcc, no GPU.

Scratch: the fused pair kernels are held to 168 VGPRs (three workgroups per CU) and must fit them without spilling: every operand
address of resblock_split_kernel is one per-lane slot register plus a compile-time offset (three column registers and the address
registers derived from each were what the 32-, 64- and 128-channel kernels used to spill: 8 / 28 / 24 bytes)."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from parrot_tts_amd import build as B

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")

PACKED = ("v_pk_mul_f32", "v_pk_add_f32", "v_pk_fma_f32")
UNITS = ("tu_mrf.hip", "tu_resblock.hip", "tu_split16.hip")
# (unit, fragment of the mangled kernel name): the kernels of the default scheme's fused ResBlock path and the layer kernel's 128 x 128 tile
NAMED = [
    ("tu_mrf.hip", "21resblock_split_kernelINS_8SchF16x3ELi2ELi8ELb1EE"),     # whole-MRF launch, 32 channels
    ("tu_resblock.hip", "21resblock_split_kernelINS_8SchF16x3ELi2ELi0ELb0EE"),
    ("tu_resblock.hip", "21resblock_split_kernelINS_8SchF16x3ELi4ELi0ELb0EE"),
    ("tu_resblock.hip", "21resblock_split_kernelINS_8SchF16x3ELi8ELi0ELb0EE"),
    ("tu_resblock.hip", "21resblock_split_kernelINS_8SchF16x3ELi16ELi0ELb0EE"),
    ("tu_resblock.hip", "23resblock16_split_kernelINS_8SchF16x3EE"),
    ("tu_split16.hip", "19conv_split16_kernelINS_8SchF16x3ELi2ELi2ELi4ELi4E"),   # every tap count of the 128 x 128 tile
]


def _kernels(asm: str) -> dict:
    """{mangled kernel name: (instruction mnemonics, scratch bytes)} of one unit's device assembly."""
    out, name, ops = {}, None, []
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, ops = m.group(1), []
            continue
        if name is None:
            continue
        m = re.match(r"^; ScratchSize: (\d+)", line)
        if m:
            out[name] = (ops, int(m.group(1)))
            name = None
            continue
        m = re.match(r"^\t([a-z]\w+)", line)
        if m:
            ops.append(m.group(1))
    return out


@pytest.fixture(scope="module")
def unit_kernels(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("isa")

    def compile_one(src):
        dst = os.path.join(tmp, src + ".s")
        cmd = [HIPCC] + B.FLAGS + B.TU_FLAGS.get(src, []) + ["--cuda-device-only", "-S", os.path.join(B.CSRC, src), "-o", dst]
        subprocess.run(cmd, check=True, cwd=B.CSRC, capture_output=True)
        with open(dst) as f:
            return _kernels(f.read())

    with ThreadPoolExecutor(max_workers=len(UNITS)) as ex:
        return dict(zip(UNITS, ex.map(compile_one, UNITS)))


def test_every_split_unit_is_built_without_the_slp_vectoriser():
    units = [f for f in B.SOURCES if f.startswith(("tu_split", "tu_mrf", "tu_resblock"))]
    assert units and all("-fno-slp-vectorize" in B.TU_FLAGS.get(f, []) for f in units)
    assert B.TU_FLAGS["tu_split16.hip"][:2] == ["-mllvm", "-disable-machine-sink"]  # (the older per-unit flag is still there)


@pytest.mark.parametrize("unit,frag", NAMED, ids=[f.split("kernelINS_")[1] for _, f in NAMED])
def test_named_kernels_hold_no_packed_fp32_arithmetic(unit_kernels, unit, frag):
    hits = {k: v for k, v in unit_kernels[unit].items() if frag in k}
    assert hits, f"{frag} not found in {unit}"
    for name, (ops, _) in hits.items():
        n_mfma = sum(o.startswith("v_mfma") for o in ops)
        assert n_mfma > 0, name
        packed = {p: ops.count(p) for p in PACKED if p in ops}
        print(name, "mfma", n_mfma, "packed", packed)
        assert not packed, (name, packed)


def test_no_kernel_of_these_units_holds_packed_fp32_arithmetic(unit_kernels):
    """bf16x6 and the other tile shapes get the same treatment as the named kernels."""
    for unit, ks in unit_kernels.items():
        assert ks, unit
        for name, (ops, _) in ks.items():
            packed = {p: ops.count(p) for p in PACKED if p in ops}
            assert not packed, (unit, name, packed)


@pytest.mark.parametrize("unit,frag", NAMED, ids=[f.split("kernelINS_")[1] for _, f in NAMED])
def test_named_kernels_use_no_scratch(unit_kernels, unit, frag):
    hits = {k: v for k, v in unit_kernels[unit].items() if frag in k}
    assert hits
    for name, (_, scratch) in hits.items():
        print(name, "scratch bytes", scratch)
        assert scratch == 0, (name, scratch)
