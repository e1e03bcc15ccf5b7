"""CPU: the C-ABI library builds, loads, and exports every symbol include/parrot_hip.h (the product interface) and
include/parrot_hip_debug.h (test / profiling / probe entry points) declare (no compute calls -- there is no GPU here)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from parrot_tts_amd import build, _lib
    build.build()
    return _lib.lib()


def _declared(header="parrot_hip.h"):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(parrot_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported_and_bound(lib):
    from parrot_tts_amd import _lib
    product, debug = _declared(), _declared("parrot_hip_debug.h")
    assert len(product) >= 20
    # the product header carries no debug / profiling / probe entry point
    assert not [n for n in product if "debug" in n or "prof" in n or "selftest" in n]
    assert not set(product) & set(debug)
    names = sorted(product + debug)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(raw, n), f"{n} declared in parrot_hip.h but not exported"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature in _lib.py"
    assert sorted(_lib.SIGNATURES) == names, "ctypes table and header disagree"


def _exported(path, llvm="/opt/rocm/llvm/bin"):
    """Names the library defines in its dynamic symbol table: llvm-nm -D --defined-only, or -- an LLVM tree that ships without
    llvm-nm -- the same table through llvm-readelf --dyn-syms (defined = any section index but UND)."""
    import subprocess
    nm = os.path.join(llvm, "llvm-nm")
    if os.path.exists(nm):
        out = subprocess.run([nm, "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        return {line.split()[-1] for line in out.splitlines() if line.split()}
    out = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--dyn-syms", "-W", path], check=True, capture_output=True, text=True).stdout
    rows = [line.split() for line in out.splitlines()]
    return {r[7].split("@")[0] for r in rows if len(r) == 8 and r[0].rstrip(":").isdigit() and r[6] != "UND"}


def test_exported_c_names_are_exactly_the_declared_ones(lib):
    """The host side is several translation units whose shared helpers live in namespace parrot (mangled); the only unmangled
    parrot_* names the library exports are the entry points of the two headers -- no more and no fewer."""
    from parrot_tts_amd import _lib
    exported = {n for n in _exported(_lib.LIB_PATH) if n.startswith("parrot_")}
    assert len(exported) >= 20
    assert exported == set(_declared() + _declared("parrot_hip_debug.h"))


def test_abi_basics(lib):
    assert lib.parrot_abi_version() == 7
    assert lib.parrot_conv_num_tile_cfgs() >= 3
    assert isinstance(lib.parrot_last_error(), bytes)
    # argument validation happens before any HIP call
    assert lib.parrot_conv_run(None, None, None, None, 1, 1, 0, 1.0, None) == -1
    assert b"null" in lib.parrot_last_error()


def test_length_regulator_workspace_bytes_are_the_recorded_ones(lib):
    """The query sizes with the layout function that parrot_length_regulator carves with (lr_scratch, host_tte.hip), reserving
    max(L, 1) output columns: same bytes as before the two were unified (tests/golden/workspace_bytes.json, recorded by
    tools/make_workspace_goldens.py).  Needs no device."""
    import json
    with open(os.path.join(ROOT, "tests", "golden", "workspace_bytes.json")) as f:
        golden = json.load(f)["length_regulator"]
    for B, S, D, L in [(1, 1, 1, 0), (2, 7, 256, 0), (2, 7, 256, 33), (64, 64, 256, 2048)]:
        assert lib.parrot_length_regulator_workspace_bytes(B, S, D, L) == golden[f"{B},{S},{D},{L}"], (B, S, D, L)
    for B, S, D in [(0, 7, 256), (-1, 7, 256), (2, 0, 256), (2, -3, 256), (2, 7, 0), (2, 7, -1)]:
        assert lib.parrot_length_regulator_workspace_bytes(B, S, D, 33) == 0, (B, S, D)


def test_train_workspace_and_saved_bytes_are_the_recorded_ones(lib):
    """parrot_{aligner,tte,voc}_train_{workspace,saved}_bytes return what they returned before the three training units came to share
    one set of product wrappers and one weight-gradient partial-buffer rule (tests/golden/train_workspace_bytes.json, recorded by
    tools/make_workspace_goldens.py --train, which says why these shapes: either side of the 64 MiB budget, and a single-tap
    group).  Every case carries the config it was recorded with.  Needs no device."""
    import json
    from parrot_tts_amd import _lib
    with open(os.path.join(ROOT, "tests", "golden", "train_workspace_bytes.json")) as f:
        golden = json.load(f)
    tup = lambda v: tuple(tup(x) for x in v) if isinstance(v, list) else v
    make = {"aligner": lambda c: _lib.AlignerCfg(**c),
            "tte": lambda c: _lib.TteTrainCfg(tte=_lib.TteCfg(**c), pad_idx=0, p_enc=0.1, p_dec=0.1, p_dp=0.5),
            "voc": lambda c: _lib.VocCfg(**{k: tup(v) for k, v in c.items()})}
    assert sorted(golden) == sorted(make) and all(len(golden[m]) >= 5 for m in make)
    for model, cases in golden.items():
        for case in cases:
            cfg = make[model](case["cfg"])
            for what in ("workspace", "saved"):
                got = getattr(lib, f"parrot_{model}_train_{what}_bytes")(ctypes.byref(cfg), *case["shape"])
                assert got == case[what], (model, what, case["shape"])
    assert [c["workspace"] for c in golden["aligner"]].count(0) == 1  # (the one refused shape; every other query answers)
    assert all(c["workspace"] > 0 and c["saved"] > 0 for m in ("tte", "voc") for c in golden[m])


def test_struct_sizes_match_header():
    from parrot_tts_amd import _lib
    assert ctypes.sizeof(_lib.ConvDesc) == 12 * 4
    assert ctypes.sizeof(_lib.TteCfg) == 14 * 4
    n_int = 7 + 8 + 8 + 1 + 4 + 1 + 16 + 1
    assert ctypes.sizeof(_lib.VocCfg) == n_int * 4


def test_header_is_plain_c_and_links_from_c(lib, tmp_path):
    """The boundary is a C ABI: include/parrot_hip.h compiles as C (gcc -std=c99 -pedantic) and a C program binds the
    entry points by name with dlopen -- no C++ or torch types involved."""
    import shutil
    import subprocess
    from parrot_tts_amd import _lib
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "abi.c"
    src.write_text('''
#include <dlfcn.h>
#include <stdio.h>
#include <string.h>
#include "parrot_hip.h"
int main(int argc, char** argv) {
    void* h = dlopen(argv[1], RTLD_NOW);
    if (!h) { fprintf(stderr, "%s\\n", dlerror()); return 2; }
    int (*ver)(void) = (int (*)(void))dlsym(h, "parrot_abi_version");
    const char* (*err)(void) = (const char* (*)(void))dlsym(h, "parrot_last_error");
    int (*run)(parrot_conv_t*, const float*, const float*, float*, int32_t, int32_t, int32_t, float, void*) =
        (int (*)(parrot_conv_t*, const float*, const float*, float*, int32_t, int32_t, int32_t, float, void*))dlsym(h, "parrot_conv_run");
    if (!ver || !err || !run) return 3;
    if (ver() != PARROT_ABI_VERSION) return 4;
    if (run(NULL, NULL, NULL, NULL, 1, 1, 0, 1.0f, NULL) != PARROT_E_INVALID) return 5;
    if (!strstr(err(), "null")) return 6;
    printf("ok\\n");
    return 0;
}
''')
    hdr = tmp_path / "hdr.c"
    hdr.write_text('#include "parrot_hip.h"\n#include "parrot_hip_debug.h"\nint parrot_header_only_tu;\n')
    subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(hdr)], check=True)
    exe = tmp_path / "abi"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-ldl"], check=True)
    env = dict(os.environ)
    import torch
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    out = subprocess.run([str(exe), _lib.LIB_PATH], check=True, capture_output=True, text=True, env=env)
    assert out.stdout.strip() == "ok"
