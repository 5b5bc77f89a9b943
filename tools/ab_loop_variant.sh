#!/bin/bash
# tools/ab_loop_variant.sh ROUNDS CONFIG V1 V2 ... [-- bench args]: alternate
# bench.py --timed-only runs of loop shapes on one box.  A shape is a
# loop_variant number (qpsk_demod_params.loop_variant) on the in-tree build, or
# LIB:VARIANT for an A/B library built by tools/ab_build.sh
# (qpsk-modulator-demodulator_amd/_build/ab/libLIB.so).  Per run: value
# (MSa/s), kernel ms, the loop's cycles per symbol.  Stops at the first
# failing run; every run has its own time limit.
set -e -o pipefail
rounds=$1; cfg=$2; shift 2
shapes=()
while [ $# -gt 0 ] && [ "$1" != "--" ]; do shapes+=("$1"); shift; done
[ "$1" == "--" ] && shift
[ $# -gt 0 ] || set -- --steps 10 --warmup 3
root=$(cd "$(dirname "$0")/.." && pwd)
for i in $(seq 1 "$rounds"); do
  for sh in "${shapes[@]}"; do
    v=${sh##*:}
    lib=
    [ "$sh" != "$v" ] && lib=$root/qpsk-modulator-demodulator_amd/_build/ab/lib${sh%%:*}.so
    out=$(QPSK_DEMOD_LIB=$lib timeout -k 10 300 python "$root/bench.py" --timed-only --config "$cfg" --loop-variant "$v" "$@" 2>/dev/null | tail -1)
    echo "[$cfg $sh] $(echo "$out" | python3 -c '
import json, sys
d = json.loads(sys.stdin.read())
k = d.get("kernels", {})
ms = {a: round(b["ms"], 2) for a, b in k.items() if isinstance(b, dict) and "ms" in b}
print("value", d["value"], "ms", json.dumps(ms), "loop_cps", k.get("loop", {}).get("cycles_per_symbol"))')"
  done
done
