#!/usr/bin/env python3
"""tools/ab_bar.py FILE [BASE]: the merge bar over an A/B record of
tools/ab_loop_variant.sh.

Per config and shape: n, median / min / max of the value (MSa/s) and the median
kernel times.  A shape wins a config against BASE (default: the first shape
of the file) if its median lies above BASE's maximum and beats BASE's median
by at least three times BASE's own (max - min) / median.
"""
import json
import re
import statistics
import sys

LINE = re.compile(r"^\[(\S+) (\S+)\] value (\S+) ms (\{.*\}) loop_cps (\S+)")


def main():
    rows = {}
    for ln in open(sys.argv[1]):
        m = LINE.match(ln)
        if m:
            cfg, shape, value, ms, cps = m.groups()
            rows.setdefault(cfg, {}).setdefault(shape, []).append((float(value), json.loads(ms), cps))
    for cfg, shapes in rows.items():
        base = sys.argv[2] if len(sys.argv) > 2 else next(iter(shapes))
        bv = [r[0] for r in shapes[base]]
        bmed, spread = statistics.median(bv), (max(bv) - min(bv)) / statistics.median(bv)
        for shape, rs in shapes.items():
            v = [r[0] for r in rs]
            med = statistics.median(v)
            kern = {k: round(statistics.median([r[1][k] for r in rs if k in r[1]]), 2) for k in rs[0][1]}
            cps = [float(r[2]) for r in rs if r[2] not in ("None", "null")]
            line = (f"{cfg} {shape}: n {len(v)} median {med:.1f} min {min(v):.1f} max {max(v):.1f} "
                    f"kernels_ms {json.dumps(kern)} loop_cps {statistics.median(cps) if cps else None}")
            if shape != base:
                gain = med / bmed - 1.0
                wins = med > max(bv) and gain >= 3.0 * spread
                line += (f" | vs {base}: {100 * gain:+.2f} % (bar: above max {max(bv):.1f} and >= "
                         f"{300 * spread:.2f} %) -> {'WINS' if wins else 'does not clear the bar'}")
            else:
                line += f" | spread (max - min) / median {100 * spread:.2f} %"
            print(line)


if __name__ == "__main__":
    main()
