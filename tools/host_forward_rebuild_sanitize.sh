#!/bin/bash
# AddressSanitizer + UBSan (leak check included) over the host code of traces rebuilt by forward tapes
# (vdf_nova_forward_tape_rebuild_eval_lanes, the ascending vdf_custom_chain constructors, csrc/tape_launch.h), CPU only:
# tools/host_tape_table_sanitize.sh's recipe with tools/host_forward_rebuild_check.cpp as the program.  The host translation units of
# libvdf_nova.so are compiled with the sanitizers into ONE stand-alone program with its own main, which is then run.  Nothing is
# loaded into an interpreter and no device is touched; libvdf_hip.so is linked as it is for the symbols the host objects name.
set -euo pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
W=${1:-/tmp/vdf_forward_rebuild_asan}
rm -rf "$W" && mkdir -p "$W"
cd "$ROOT/vdf_amd/csrc"
for f in host_math minroot_host r1cs nova_host trace_walks circuits_host compress_host wire_host rounds_host custom_chain_host; do
  g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -pthread -c host/$f.cpp -o "$W/$f.o" &
done
wait
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -pthread -I "$ROOT/include" \
  "$ROOT/tools/host_forward_rebuild_check.cpp" "$W"/*.o -L"$ROOT/vdf_amd" -lvdf_hip -Wl,-rpath,"$ROOT/vdf_amd" -o "$W/check"
ASAN_OPTIONS=detect_leaks=1 "$W/check"
