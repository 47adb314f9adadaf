#!/bin/bash
# AddressSanitizer + UBSan (leak check included) over the host side of the family-1 device random oracle,
# vdf_nova_ro_block_constants and vdf_nova_ro_hash_batch_eval_ro (csrc/host/nova_host.cpp over host/r1cs.cpp), CPU only:
# tools/host_aggregate_sanitize.sh's recipe with tools/host_ro_block_check.cpp as the program.  The host translation units of
# libvdf_nova.so are compiled with the sanitizers into ONE stand-alone program with its own main, which is then run.  Nothing is
# loaded into an interpreter and no device is touched; libvdf_hip.so is linked as it is for the symbols the host objects name.
set -euo pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
W=${1:-/tmp/vdf_ro_block_san}
rm -rf "$W" && mkdir -p "$W/asan"
cd "$ROOT/vdf_amd/csrc"
D="$W/asan"
FLAGS="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
pids=()
for f in host_math minroot_host r1cs nova_host trace_walks circuits_host compress_host aggregate_host wire_host rounds_host custom_chain_host custom_stream_host; do
  g++ -O1 -g -std=c++17 $FLAGS -fno-omit-frame-pointer -pthread -c host/$f.cpp -o "$D/$f.o" &
  pids+=($!)
done
for p in "${pids[@]}"; do wait "$p"; done
g++ -O1 -g -std=c++17 $FLAGS -fno-omit-frame-pointer -pthread -I "$ROOT/include" \
  "$ROOT/tools/host_ro_block_check.cpp" "$D"/*.o -L"$ROOT/vdf_amd" -lvdf_hip -Wl,-rpath,"$ROOT/vdf_amd" -o "$D/check"
ASAN_OPTIONS=detect_leaks=1 "$D/check"
