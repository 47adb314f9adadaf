#!/bin/bash
# AddressSanitizer + UBSan (leak check included) over the host-only part of proof aggregation, vdf_nova_aggregate_fold_instances
# (csrc/host/aggregate_host.cpp: the verifier's transcript and folds), CPU only: tools/host_custom_stream_sanitize.sh's recipe with
# tools/host_aggregate_check.cpp as the program and the inputs of tests/golden/aggregate.json.  The host translation units of
# libvdf_nova.so are compiled with the sanitizers into ONE stand-alone program with its own main, which is then run.  Nothing is
# loaded into an interpreter and no device is touched; libvdf_hip.so is linked as it is for the symbols the host objects name.
# vdf_nova_aggregate_deserialize is not covered: it takes a parameter set, and a parameter set needs a device.
set -euo pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
W=${1:-/tmp/vdf_aggregate_san}
rm -rf "$W" && mkdir -p "$W/asan"
# the golden file's per-side inputs as lines of hex (wire encoding: tests/aggregate_spec.py over oracle/wire.py)
PYTHONPATH="$ROOT:$ROOT/tests" python3 - "$ROOT/tests/golden/aggregate.json" > "$W/cases.txt" <<'EOF'
import json, sys
from oracle import nova as nv, wire
g = json.load(open(sys.argv[1]))
hx = lambda v: int(v, 16)
inst = lambda j: wire.encode_instance(nv.Relaxed(tuple(map(hx, j["comm_W"])), tuple(map(hx, j["comm_E"])), hx(j["u"]), list(map(hx, j["X"])), [], []), True)
pt = lambda p: wire.compress_point(None if tuple(map(hx, p)) == (0, 0) else tuple(map(hx, p)))
for K, a in sorted(g["aggregates"].items()):
    for side, s in enumerate(a["sides"]):
        tt = b"".join(pt(p) for p in s["comm_TT"]).hex() or "-"
        print(side, hx(g["params"]).to_bytes(32, "little").hex(), K, b"".join(inst(j) for j in s["instances"]).hex(), tt, inst(s["acc"]).hex())
EOF
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
  "$ROOT/tools/host_aggregate_check.cpp" "$D"/*.o -L"$ROOT/vdf_amd" -lvdf_hip -Wl,-rpath,"$ROOT/vdf_amd" -o "$D/check"
ASAN_OPTIONS=detect_leaks=1 "$D/check" "$W/cases.txt"
