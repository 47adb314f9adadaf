#!/bin/bash
# AddressSanitizer + UBSan over the custom chain's host code, CPU only: the host translation units of libvdf_nova.so compiled with
# the sanitizers into ONE stand-alone program with its own main (tools/host_custom_chain_check.cpp), which is then run.  Nothing is
# loaded into an interpreter and no device is touched; libvdf_hip.so is linked as it is for the symbols the host objects name.
set -euo pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
W=${1:-/tmp/vdf_chain_asan}
rm -rf "$W" && mkdir -p "$W"
cd "$ROOT/vdf_amd/csrc"
for f in host_math minroot_host r1cs nova_host trace_walks circuits_host compress_host wire_host rounds_host custom_chain_host; do
  g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -pthread -c host/$f.cpp -o "$W/$f.o" &
done
wait
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -pthread -I "$ROOT/include" \
  "$ROOT/tools/host_custom_chain_check.cpp" "$W"/*.o -L"$ROOT/vdf_amd" -lvdf_hip -Wl,-rpath,"$ROOT/vdf_amd" -o "$W/check"
"$W/check"
