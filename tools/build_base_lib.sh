#!/bin/bash
# Build the library of a git revision (default HEAD) with that revision's own build.py into ab/base/, for same-box A/B runs against the in-tree build
# (PM_LIB=ab/base/pinthememory_amd/libpinmem_hip.so).
set -e
REV=${1:-HEAD}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$ROOT/ab/base
rm -rf "$OUT"
mkdir -p "$OUT"
git -C "$ROOT" archive "$REV" pinthememory_amd/csrc pinthememory_amd/build.py include | tar -x -C "$OUT"
(cd "$OUT" && python pinthememory_amd/build.py --force)
echo "built ab/base/pinthememory_amd/libpinmem_hip.so from $REV"
