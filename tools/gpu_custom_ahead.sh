#!/bin/bash
# The measurement behind profiles/r20_custom_ahead.txt on one MI355X.  $1 (optional): a checkout of the PARENT commit, built, whose
# tools/gpu_custom_chain.py gives the baseline in the same session.  Every step that uses the GPU runs under a time limit of its
# own, and the script ends at the first step that fails.
set -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-$ROOT/profiles}
mkdir -p "$OUT"
PARENT_ARGS=()
if [ -n "${1:-}" ]; then
  (cd "$1" && timeout -k 10 420 python tools/gpu_custom_chain.py --windows 32 --out "$OUT/r20_parent_custom_chain.txt") || exit $?
  PARENT_ARGS=(--parent "$OUT/r20_parent_custom_chain.txt")
fi
timeout -k 10 540 python "$ROOT/tools/gpu_custom_ahead.py" "${PARENT_ARGS[@]}" --out "$OUT/r20_custom_ahead.txt" || exit $?
for L in 1 4 8; do
  timeout -k 10 300 python "$ROOT/tools/gpu_custom_ahead.py" --skip-single --lanes $L --out "$OUT/r20_custom_ahead.txt" || exit $?
done
