#!/bin/bash
# Build a kernel variant of libdash into tools/variants/libdash_NAME.so (experiments only).
# Usage: [SRC=file.hip] [PATCHES="tools/experiments/x.patch ..."] tools/build_variant.sh NAME [extra hipcc flags...]
# PATCHES are applied to a temporary copy of the kernel source (e.g. issue_probes.patch: the
# DASH_PAD_VALU / DASH_PAD_SALU / DASH_PAD_VHALF issue-cost probes and DASH_HEADLINE_ONLY).
# The variant's kernels are linked with the product's other objects, as the Makefile lists and builds them.
set -euo pipefail
NAME=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
PKG=$ROOT/ue22cs343bb1-openmp-assignment_amd
OUT=${OUT:-$ROOT/tools/variants}; mkdir -p "$OUT"
HIPCC=/opt/rocm/bin/hipcc
SRC=${SRC:-$PKG/csrc/dash_kernels.hip}
if [ -n "${PATCHES:-}" ]; then
    TMP=$(mktemp -d); cp "$SRC" "$TMP/dash_kernels.hip"
    for p in $PATCHES; do patch -s "$TMP/dash_kernels.hip" "$ROOT/$p"; done
    SRC=$TMP/dash_kernels.hip
fi
HOST_OBJ=$(make -s -C "$PKG" print-host-obj)
make -s -C "$PKG" $HOST_OBJ
$HIPCC --offload-arch=gfx950 -O3 -std=c++17 -fPIC -I"$ROOT/include" -I"$PKG/csrc" -Wno-bitwise-instead-of-logical -Wno-pass-failed \
    -DDASH_WAVES_PER_EU=5 "$@" -c -o "$OUT/k_$NAME.o" "$SRC"
(cd "$PKG" && $HIPCC --offload-arch=gfx950 -shared -fPIC -o "$OUT/libdash_$NAME.so" "$OUT/k_$NAME.o" $HOST_OBJ)
rm -f "$OUT/k_$NAME.o"
echo "built $OUT/libdash_$NAME.so"
