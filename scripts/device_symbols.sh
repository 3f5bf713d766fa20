#!/bin/bash
# Device code of libfdm_engine.so as a list: for each of the five translation units, compile device-only with the
# Makefile's HIPFLAGS, unbundle the gfx950 code object and write the sorted "name size" list of its defined FUNC symbols.
# A host-side refactor leaves the five lists identical (same kernels, same byte sizes); needs no GPU.
# usage: scripts/device_symbols.sh OUTDIR [TREE]     (TREE: another checkout to list, default this one)
#   scripts/device_symbols.sh build/devsyms/parent ../parent && scripts/device_symbols.sh build/devsyms/branch &&
#   diff -r build/devsyms/parent build/devsyms/branch
set -euo pipefail
[ $# -ge 1 ] || { echo "usage: $0 OUTDIR [TREE]" >&2; exit 2; }
mkdir -p "$1"
OUT=$(cd "$1" && pwd)
TREE=$(cd "${2:-$(dirname "$0")/..}" && pwd)
CSRC=$TREE/fastdem_amd/csrc
ROCM=${ROCM_PATH:-/opt/rocm}
HIPCC=${HIPCC:-$ROCM/bin/hipcc}
LLVM=$ROCM/lib/llvm/bin
HIPFLAGS=$(make -s -C "$CSRC" --eval='print-hipflags: ; @echo $(HIPFLAGS)' print-hipflags)
UNITS=$(make -s -C "$CSRC" --eval='print-units: ; @echo $(UNITS)' print-units)
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT

one() {
  local u=$1
  $HIPCC $HIPFLAGS -w --cuda-device-only -c -o "$TMP/$u.dev.o" "$CSRC/$u.hip"
  "$LLVM/clang-offload-bundler" --unbundle --type=o --targets=hip-amdgcn-amd-amdhsa--gfx950 \
      --input="$TMP/$u.dev.o" --output="$TMP/$u.co"
  "$LLVM/llvm-readelf" --symbols --wide "$TMP/$u.co" |
      awk '$4 == "FUNC" && $7 != "UND" { print $8, $3 }' | LC_ALL=C sort > "$OUT/$u.syms"
}
pids=()
for u in $UNITS; do one "$u" & pids+=($!); done
for p in "${pids[@]}"; do wait "$p"; done
for u in $UNITS; do printf '%-20s %4d symbols\n' "$u" "$(wc -l < "$OUT/$u.syms")"; done
