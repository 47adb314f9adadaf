#!/bin/bash
# AddressSanitizer + UBSan (leak check included) over the host code of tape tables (VDF_TAPE_TAB, vdf_cs_tab), CPU only:
# tools/host_pow_chain_sanitize.sh's recipe with tools/host_tape_table_check.cpp as the program.  The host translation units of
# libvdf_nova.so are compiled with the sanitizers into ONE stand-alone program with its own main, which is then run.  Nothing is
# loaded into an interpreter and no device is touched; libvdf_hip.so is linked as it is for the symbols the host objects name.
set -euo pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
W=${1:-/tmp/vdf_tape_table_asan}
rm -rf "$W" && mkdir -p "$W"
cd "$ROOT/vdf_amd/csrc"
for f in host_math minroot_host r1cs nova_host trace_walks circuits_host compress_host wire_host rounds_host custom_chain_host; do
  g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -pthread -c host/$f.cpp -o "$W/$f.o" &
done
wait
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -pthread -I "$ROOT/include" \
  "$ROOT/tools/host_tape_table_check.cpp" "$W"/*.o -L"$ROOT/vdf_amd" -lvdf_hip -Wl,-rpath,"$ROOT/vdf_amd" -o "$W/check"
ASAN_OPTIONS=detect_leaks=1 "$W/check"
