"""Build libparrot_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU).  Every csrc/*.hip is one translation unit,
compiled in parallel, then linked: host_*.hip hold the C ABI, one unit per subsystem (three for the vocoder, host_voc*.hip, around voc.h;
shared declarations in host_common.h; the five host_*_train.hip fill their matrix products through train_gemm_host.h), tu_*.hip
instantiate the kernel templates (tu_train_gemm.hip: the fp32 tap-GEMM kernels all four training paths run on)."""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libparrot_hip.so")
OBJ = os.path.join(HERE, "build")
SOURCES = sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith(".h")) + [os.path.join("..", "..", "include", h) for h in ("parrot_hip.h", "parrot_hip_debug.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]
# Per-source flags.  tu_split16: LLVM's machine-sink pass moves the weight refills for the next chunk's first k-step -- which feed
# nothing but loop-carried registers -- out of the MFMA block into the loop latch, behind the slab conversion and the barrier, so
# that the first step of every chunk waits a full fetch latency (tools/isa_schedule.py shows it in the ISA).  Without the pass
# they stay where they are written: conv_split16 128 x 128: 6.88 -> 6.78 ms per step (mean of five same-box A/B pairs, the
# sign held in four, one tie: at the edge of the run-to-run noise), no spills, nothing else moves.
TU_FLAGS = {f: ["-mllvm", "-disable-machine-sink"] for f in ("tu_split16.hip", "tu_split16_wide.hip", "tu_split16_xpl.hip")}
# The units of the split-scheme MFMA kernels (and the attention cores): no SLP vectoriser.  At -O3 it pairs adjacent scalar fp32
# multiplies / adds / FMAs of the operand conversion, the bias and rescale loops and the epilogues into v_pk_{mul,add,fma}_f32.
# A wave64 v_mul_f32 already issues at full rate on gfx950, so packing buys no throughput, and a packed fp32 op beside MFMAs
# costs more issue time than the two scalar ops it replaces (tools/probes/interleave_unpacked.hip measures both).
# tests/test_isa_unpacked.py holds these kernels to zero packed fp32 arithmetic and zero scratch.
NO_SLP_UNITS = ("tu_mrf.hip", "tu_mrf_single.hip", "tu_resblock.hip", "tu_split16.hip", "tu_split16_single.hip",
                "tu_split16_single_f16.hip", "tu_split16_wide.hip", "tu_split16_xpl.hip", "tu_split_bf16x6.hip", "tu_split_f16x3.hip",
                "tu_split_single.hip", "tu_attn.hip")
for _f in NO_SLP_UNITS:
    TU_FLAGS[_f] = TU_FLAGS.get(_f, []) + ["-fno-slp-vectorize"]


def _stale() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(os.path.join(CSRC, f)) > t for f in SOURCES + HEADERS)


def build(force: bool = False, verbose: bool = False, extra_flags=(), lib_path: str = None, obj_dir: str = None) -> str:
    """Compile csrc/*.hip -> parrot_tts_amd/libparrot_hip.so.  Returns the library path.
    `lib_path` / `obj_dir` / `extra_flags`: experiment builds of the same sources (tools/build_exp.sh -> build_exp/)."""
    if lib_path is None and not force and not _stale():
        return LIB
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    LIB_OUT, OBJ_OUT = lib_path or LIB, obj_dir or OBJ
    os.makedirs(OBJ_OUT, exist_ok=True)

    def compile_one(src):
        obj = os.path.join(OBJ_OUT, os.path.splitext(src)[0] + ".o")
        tu = [] if os.environ.get("PARROT_NO_TU_FLAGS") else TU_FLAGS.get(src, [])  # (A/B builds: tools/build_exp.sh)
        cmd = [hipcc] + FLAGS + tu + list(extra_flags) + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.run(cmd, check=True, cwd=CSRC)
        return obj

    with ThreadPoolExecutor(max_workers=max(1, min(len(SOURCES), 16, (os.cpu_count() or 2) - 1))) as ex:
        objs = list(ex.map(compile_one, SOURCES))
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_OUT] + objs
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, cwd=CSRC)
    return LIB_OUT


if __name__ == "__main__":
    if "--exp" in sys.argv:  # python -m parrot_tts_amd.build --exp TAG -DFOO -DBAR ...  ->  build_exp/libparrot_TAG.so
        i = sys.argv.index("--exp")
        tag, flags = sys.argv[i + 1], sys.argv[i + 2:]
        root = os.path.dirname(HERE)
        print(build(force=True, verbose=False, extra_flags=flags, lib_path=os.path.join(root, "build_exp", f"libparrot_{tag}.so"),
                    obj_dir=os.path.join(root, "build_exp", "obj_" + tag)))
    else:
        print(build(force="--force" in sys.argv, verbose=True))
