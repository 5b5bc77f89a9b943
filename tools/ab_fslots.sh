#!/bin/bash
# float M&M -> Costas slots (round 6) against double slots, every shape
set -e -o pipefail
O=${AB_OUT:-$PWD/ab_out}/fslots2
mkdir -p "$O"
for c in c2 c4 c3; do
  timeout -k 10 900 bash tools/ab_bench.sh 2 --config $c --steps 10 --warmup 3 2>&1 | tee -a "$O/ab_$c.txt"
done
for L in base fsall; do
  QPSK_DEMOD_LIB=$PWD/qpsk-modulator-demodulator_amd/_build/ab/lib$L.so timeout -k 10 600 python bench.py --full --config c3 --sub-configs none --no-drop-in --no-host-ring --no-framer --no-cpu-baseline --no-parity --steps 10 --warmup 3 --detail "$O/detail_$L.json" > "$O/line_$L.json" 2>/dev/null
done
