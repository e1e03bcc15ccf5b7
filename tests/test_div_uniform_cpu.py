"""csrc/div_uniform.h: the branch mean's division by a launch-uniform divisor without the IEEE division sequence.

The EPI_ADD_DIV epilogues replace x / 3 by q = x r; e = fma(-q, 3, x); q' = fma(e, r, q), r = RN(1 / 3), keeping q where e is zero or
NaN (x = -0 and x = +-inf).  That is only legal if q' has the quotient's bits for EVERY fp32 x: tools/probes/div3_exhaustive.cpp
runs the very header text with the host compiler over all 2^32 bit patterns (subnormals, infinities, NaN-ness).  Powers of two
take the exact multiply by the reciprocal, any other divisor the division itself.  No GPU; ~10-30 s of host CPU."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
pytestmark = pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = os.path.join(tmp_path_factory.mktemp("div"), "div3_exhaustive")
    # -ffp-contract=off: nothing but the header's own fmaf calls may fuse; no -ffast-math, no flush-to-zero
    subprocess.run([CXX, "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", os.path.join(ROOT, "tools", "probes", "div3_exhaustive.cpp"),
                    "-o", exe], check=True)
    return exe


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True)
    rows = [json.loads(line) for line in r.stdout.splitlines()]
    return r.returncode, rows


def test_division_by_three_is_bit_exact_for_every_fp32_input(checker):
    rc, rows = _run(checker, "3")
    print(rows)
    assert len(rows) == 1 and rows[0]["d"] == 3 and rows[0]["mode"] == "fma3"
    assert rows[0]["r_bits"] == "0x3eaaaaab"  # RN(1 / 3)
    assert rows[0]["inputs"] == 2 ** 32
    assert rows[0]["mismatches"] == 0 and rows[0]["first_mismatch_bits"] is None and rc == 0


def test_powers_of_two_take_the_exact_multiply_and_other_divisors_the_division(checker):
    rc, rows = _run(checker, "--stride", "4099", "1", "2", "4", "0.5", "5", "7", "6")
    print(rows)
    modes = {r["d"]: r["mode"] for r in rows}
    assert modes == {1: "mul", 2: "mul", 4: "mul", 0.5: "mul", 5: "true", 7: "true", 6: "true"}
    assert all(r["mismatches"] == 0 and r["inputs"] > 10 ** 6 for r in rows) and rc == 0
