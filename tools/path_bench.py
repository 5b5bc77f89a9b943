#!/usr/bin/env python3
"""What the propagation path (qpsk_path_apply_fmt) costs on one MI355X, the
legs alternated in one run.

Writes one JSON file (--out, default profiles/path_bench.json).  The C3 shape
(4096 streams x 2^20 samples, sps 4, 129 taps) is synthesised clean in device
memory (qpsk_synth_generate with no carrier and no noise: the modulator's
baseband); the path reads those rows and writes rows of its own.  Every handle
has taken one call before it is timed, so a timed call emits about as many
samples as it takes.  Legs, --repeats rounds of each in turn, every one timed
with device events around calls queued on one stream:

  cf32_L1        CF32 in, CF32 out, one unit tap, r = 1
  cf32_L4        the project's four taps
  cf32_L1_ppm    one tap, a 100 ppm spread of clock offsets with random tau
  cf32_L4_ppm    four taps and the spread
  cs8_L1, cs8_L4_ppm   CS8 in, CS8 out (a quarter of the bytes)
  copy_cf32, copy_cs8  yardstick: a device-to-device copy of the same rows
                 (bytes in plus bytes out)
  channel_cf32   yardstick: qpsk_channel_apply_fmt on the same rows
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_bench.json"))
    ap.add_argument("--streams", type=int, default=C3["streams"])
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--calls", type=int, default=2, help="timed calls a leg and round")
    ap.add_argument("--spread-ppm", type=float, default=100.0)
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
    spread = dict(clock_spread=args.spread_ppm, tau_random=1)
    cap = Q.path_out_bound(Q.path_params(**spread), n)
    pitch = (cap + 7) // 8 * 8                       # rows the 16-byte accesses take
    y32 = torch.empty((S, 2 * pitch), dtype=torch.float32, device=dev)
    x8 = torch.empty((S, 2 * n), dtype=torch.int8, device=dev)
    for s0 in range(0, S, 256):                      # half of full scale at the signal's peak
        blk = iq[s0: s0 + 256]
        x8[s0: s0 + 256] = (blk * (64.0 / float(blk.abs().max()))).round().clamp(-127, 127).to(torch.int8)
    y8 = torch.empty((S, 2 * pitch), dtype=torch.int8, device=dev)

    def path(**kw):
        pa = Q.Path(S, device=dev.index, **kw)
        pa.set_stream(stream.cuda_stream)
        return pa

    paths = {"cf32_L1": path(), "cf32_L4": path(multipath=1), "cf32_L1_ppm": path(**spread),
             "cf32_L4_ppm": path(multipath=1, **spread), "cs8_L1": path(), "cs8_L4_ppm": path(multipath=1, **spread)}
    ch = Q.Channel(S, sample_rate=float(FS), device=dev.index)
    ch.set_stream(stream.cuda_stream)
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
        pa = paths[name]
        if name.startswith("cf32"):
            def fn():
                emitted[name] = pa.apply_device(iq, n, y32, out_cap=cap)
        else:
            def fn():
                emitted[name] = pa.apply_device(x8, n, y8, fmt="cs8", out_cap=cap)
        return lambda: timed(fn)

    legs = {name: leg(name) for name in paths}
    legs["copy_cf32"] = lambda: timed(lambda: y32[:, : 2 * n].copy_(iq))
    legs["copy_cs8"] = lambda: timed(lambda: y8[:, : 2 * n].copy_(x8))
    legs["channel_cf32"] = lambda: timed(lambda: ch.apply_device(iq, n, out_dev=y32[:, : 2 * n]))
    rec = {"device": torch.cuda.get_device_name(dev), "streams": S, "samples": n, "spread_ppm": args.spread_ppm,
           "tile_outputs": Q.PATH_TILE_OUTPUTS, "out_cap": cap, "runs": []}
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
    gs = S * n / 1e9
    rec["gsamples_per_s"] = {k: round(gs / (rec[k + "_ms_median"] / 1e3), 3) for k in paths}
    rec["gbytes_moved"] = {"cf32": round(S * n * 16 / 1e9, 1), "cs8": round(S * n * 4 / 1e9, 1)}
    rec["gbytes_per_s"] = {k: round(S * n * (16 if "cf32" in k else 4) / 1e9 / (rec[k + "_ms_median"] / 1e3), 1)
                           for k in list(paths) + ["copy_cf32", "copy_cs8"]}
    rec["over_copy"] = {k: round(rec[k + "_ms_median"] / rec["copy_" + k.split("_")[0] + "_ms_median"], 3) for k in paths}
    rec["over_channel"] = {k: round(rec[k + "_ms_median"] / rec["channel_cf32_ms_median"], 3)
                           for k in paths if k.startswith("cf32")}
    print(json.dumps({k: v for k, v in rec.items() if k != "runs"}), flush=True)
    for h in list(paths.values()) + [ch]:
        h.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
