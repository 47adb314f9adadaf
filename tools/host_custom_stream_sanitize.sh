#!/bin/bash
# AddressSanitizer + UBSan (leak check included), then ThreadSanitizer, over the host code of custom chains that grow
# (vdf_nova_custom_chain_begin / _push_checkpoints / _push_advice) and of the evaluator of vdf_nova_eval_and_prove_custom
# (csrc/host/custom_stream.hpp), CPU only: tools/host_forward_rebuild_sanitize.sh's recipe with tools/host_custom_stream_check.cpp as
# the program.  The host translation units of libvdf_nova.so are compiled with the sanitizers into ONE stand-alone program with its
# own main, which is then run.  Nothing is loaded into an interpreter and no device is touched; libvdf_hip.so is linked as it is for
# the symbols the host objects name.  The second build (-fsanitize=thread) runs the evaluator part alone.
set -euo pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
W=${1:-/tmp/vdf_custom_stream_san}
rm -rf "$W" && mkdir -p "$W/asan" "$W/tsan"
cd "$ROOT/vdf_amd/csrc"
build() {   # $1: directory, the rest: the sanitizer's flags
  local D=$1; shift
  local pids=()
  for f in host_math minroot_host r1cs nova_host trace_walks circuits_host compress_host wire_host rounds_host custom_chain_host custom_stream_host; do
    g++ -O1 -g -std=c++17 "$@" -fno-omit-frame-pointer -pthread -c host/$f.cpp -o "$D/$f.o" &
    pids+=($!)
  done
  for p in "${pids[@]}"; do wait "$p"; done
  g++ -O1 -g -std=c++17 "$@" -fno-omit-frame-pointer -pthread -I "$ROOT/include" \
    "$ROOT/tools/host_custom_stream_check.cpp" "$D"/*.o -L"$ROOT/vdf_amd" -lvdf_hip -Wl,-rpath,"$ROOT/vdf_amd" -o "$D/check"
}
build "$W/asan" -fsanitize=address,undefined -fno-sanitize-recover=undefined
ASAN_OPTIONS=detect_leaks=1 "$W/asan/check"
build "$W/tsan" -fsanitize=thread
TSAN_OPTIONS=halt_on_error=1 "$W/tsan/check" evaluator
