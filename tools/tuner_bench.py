#!/usr/bin/env python3
"""What the tuner (qpsk_tuner_apply_fmt) costs on one MI355X, the legs
alternated in one run.

Writes one JSON file (--out, default profiles/tuner_bench.json).  The C3 shape
(4096 streams x 2^20 samples, sps 4) is synthesised clean in device memory
(qpsk_synth_generate with no carrier and no noise: the modulator's baseband);
the tuner reads those rows and writes rows of its own, T = 16.  Every handle
has taken one call before it is timed, so a timed call emits about as many
samples as its rate gives.  Legs, --repeats rounds of each in turn, every one
timed with device events around calls queued on one stream:

  cf32_r1, cf32_r1.25, cf32_r4   CF32 in, CF32 out, freq = 0.03, r = 1, 1.25, 4
  cs8_r1.25                      CS8 in, CF32 out, r = 1.25
  copy_cf32                      yardstick: a device-to-device copy of the same rows
  path_cf32                      yardstick: qpsk_path_apply_fmt (one tap, r = 1) on them
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "qpsk-modulator-demodulator_amd"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FS = 10_000_000
ALPHA = 0.4000000059604645
C3 = dict(streams=4096, sps=4, span=32)
RATES = {"cf32_r1": 1.0, "cf32_r1.25": 1.25, "cf32_r4": 4.0, "cs8_r1.25": 1.25}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tuner_bench.json"))
    ap.add_argument("--streams", type=int, default=C3["streams"])
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--calls", type=int, default=2, help="timed calls a leg and round")
    ap.add_argument("--freq", type=float, default=0.03)
    ap.add_argument("--taps-per-phase", type=int, default=16)
    ap.add_argument("--legs", default="", help="comma-separated subset of the legs (default: all)")
    args = ap.parse_args()

    import torch
    import qpsk_amd as Q
    torch.cuda.init()
    dev = torch.device("cuda", 0)
    S, n, sps, span = args.streams, args.samples, C3["sps"], C3["span"]
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    iq, _ = Q.synth_generate(S, n, FS, FS // sps, rrc_alpha=ALPHA, rrc_span=span, seed=0x5159534B, lo_ppm=0.0,
                             device=dev.index, stream=stream.cuda_stream)
    cap = max(Q.tuner_out_bound(Q.tuner_params(), n), Q.path_out_bound(Q.path_params(), n))
    pitch = (cap + 7) // 8 * 8                       # rows the 16-byte accesses take
    y32 = torch.empty((S, 2 * pitch), dtype=torch.float32, device=dev)
    x8 = torch.empty((S, 2 * n), dtype=torch.int8, device=dev)
    for s0 in range(0, S, 256):                      # half of full scale at the signal's peak
        blk = iq[s0: s0 + 256]
        x8[s0: s0 + 256] = (blk * (64.0 / float(blk.abs().max()))).round().clamp(-127, 127).to(torch.int8)

    def tuner(r):
        tu = Q.Tuner(S, freq=args.freq, rate=r, tau0=0.3, taps_per_phase=args.taps_per_phase, device=dev.index)
        tu.set_stream(stream.cuda_stream)
        return tu

    want = [k for k in args.legs.split(",") if k] or list(RATES) + ["copy_cf32", "path_cf32"]
    tuners = {name: tuner(r) for name, r in RATES.items() if name in want}
    pa = Q.Path(S, device=dev.index)
    pa.set_stream(stream.cuda_stream)
    emitted = {}

    def timed(fn):
        out = []
        for _ in range(args.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            out.append(round(e0.elapsed_time(e1), 3))
        return out

    def leg(name):
        tu = tuners[name]
        if name.startswith("cf32"):
            def fn():
                emitted[name] = tu.apply_device(iq, n, y32, out_cap=cap)
        else:
            def fn():
                emitted[name] = tu.apply_device(x8, n, y32, fmt="cs8", out_fmt="cf32", out_cap=cap)
        return lambda: timed(fn)

    legs = {name: leg(name) for name in tuners}
    if "copy_cf32" in want:
        legs["copy_cf32"] = lambda: timed(lambda: y32[:, : 2 * n].copy_(iq))
    if "path_cf32" in want:
        legs["path_cf32"] = lambda: timed(lambda: pa.apply_device(iq, n, y32, out_cap=cap))
    rec = {"device": torch.cuda.get_device_name(dev), "streams": S, "samples": n, "freq": args.freq,
           "taps_per_phase": args.taps_per_phase, "tile_outputs": Q.TUNER_TILE_OUTPUTS, "out_cap": cap,
           "library": os.path.relpath(Q.LIB_PATH, ROOT), "runs": []}
    for name in legs:                                # warm-up: code objects, first touches, the streams' first call
        legs[name]()
    for rep in range(args.repeats):
        for name in legs:
            run = {"leg": name, "repeat": rep, "ms": legs[name]()}
            rec["runs"].append(run)
            print(json.dumps(run), flush=True)
    for name in legs:
        ms = [m for r in rec["runs"] if r["leg"] == name for m in r["ms"]]
        rec[name + "_ms"] = ms
        rec[name + "_ms_median"] = round(statistics.median(ms), 3)
    rec["emitted_min_max"] = {k: [int(v.min()), int(v.max())] for k, v in emitted.items()}
    rec["ginputs_per_s"] = {k: round(S * n / 1e9 / (rec[k + "_ms_median"] / 1e3), 3) for k in tuners}
    # bytes a call moves: the input rows once, the output rows once
    moved = {k: S * n * (8 if k.startswith("cf32") else 2) + S * int(emitted[k].max()) * 8 for k in tuners}
    rec["gbytes_per_s"] = {k: round(moved[k] / 1e9 / (rec[k + "_ms_median"] / 1e3), 1) for k in tuners}
    if "copy_cf32" in legs:
        rec["gbytes_per_s"]["copy_cf32"] = round(S * n * 16 / 1e9 / (rec["copy_cf32_ms_median"] / 1e3), 1)
        rec["over_copy"] = {k: round(rec[k + "_ms_median"] / rec["copy_cf32_ms_median"], 3) for k in tuners}
    if "path_cf32" in legs:
        rec["over_path"] = {k: round(rec[k + "_ms_median"] / rec["path_cf32_ms_median"], 3) for k in tuners}
    print(json.dumps({k: v for k, v in rec.items() if k != "runs"}), flush=True)
    for h in list(tuners.values()) + [pa]:
        h.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
