#!/bin/bash
# A/B of the fused quotient step and the bounded-top product bodies on ONE box, interleaved: a second build of the library with
# `make -C vdf_amd/csrc ab AB_FLAGS=-DVDF_FE_R10` (the quotient digit and its carry flag computed apart, the generic bodies in the
# lazy group law: the device code before both changes, by tools/compare_device_code.py) against the shipped one.  The second
# build is SELECTED with VDF_HIP_LIB (vdf_amd/_lib.py); the shipped vdf_amd/libvdf_hip.so is never touched.  The headline run
# of bench.py as it stands, then the short one; a run that fails ends the script.
# usage (GPU box, repo root): bash tools/ab_fe_fused.sh [rounds]
set -eu
R=$(pwd)
AB=$R/vdf_amd/csrc/build/ab/libvdf_hip.so
[ -f "$AB" ] || { echo "build the A/B library first: make -C vdf_amd/csrc ab AB_FLAGS=-DVDF_FE_R10"; exit 1; }
for args in "" "--steps 20 --warmup 3"; do
  for round in $(seq 1 ${1:-5}); do
    for which in r10 shipped; do
      if [ $which = r10 ]; then export VDF_HIP_LIB=$AB; else unset VDF_HIP_LIB; fi
      line=$(timeout -k 10 150 python3 $R/bench.py --gpus 1 $args 2>/dev/null)
      echo "$line" | python3 -c "import json,sys; d=json.loads(sys.stdin.read()); print('== bench.py --gpus 1 $args round $round [$which] msm %.4f GPoints/s  %.4f ms/step' % (d['value'], d['ms_per_step']))"
    done
  done
done
