#!/bin/bash
# Build the library of a given commit (default HEAD) into build_exp/lib_base.so for same-box A/B runs
# (PARROT_HIP_LIB=build_exp/lib_base.so python bench.py ...): GPU boxes differ by a few percent.
# The commit's own build.py compiles the commit's own sources, so the source list and the per-unit flags are that commit's;
# the object files stay in build_exp/obj_base (tools/kernel_isa_diff.py compares them with parrot_tts_amd/build).
set -e
REV=${1:-HEAD}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
mkdir -p "$ROOT/build_exp"
git -C "$ROOT" archive "$REV" parrot_tts_amd/csrc parrot_tts_amd/build.py include | tar -x -C "$TMP"
python3 - "$TMP/parrot_tts_amd" "$ROOT/build_exp" <<'EOF'
import sys
sys.path.insert(0, sys.argv[1])
import build
print(build.build(force=True, lib_path=sys.argv[2] + "/lib_base.so", obj_dir=sys.argv[2] + "/obj_base"))
EOF
