#!/usr/bin/env python3
"""What the test bench's channel costs on one MI355X, the legs alternated in
one run.

Writes one JSON file (--out, default profiles/channel_bench.json).  The C3
shape (4096 streams x 2^20 samples, sps 4, 129 taps) is synthesised clean in
device memory (qpsk_synth_generate with no carrier and no noise: the
modulator's baseband); the channel reads those rows and writes rows of its
own.  Legs, --repeats rounds of each in turn, every one timed with device
events around calls queued on one stream:

  cf32          qpsk_channel_apply_fmt, CF32 in, CF32 out, no noise
  cs8           the same into CS8 rows (a quarter of the bytes written)
  cf32_noise    CF32 out with noise_rms = 0.05 (a third sincos, a log and a
  cs8_noise     sqrt a sample), and the same into CS8
  demod         qpsk_demod_process on the channel's CF32 rows from a fresh
                state: the step the channel feeds, for scale
  tile          the channel on the first 16 streams alone, one workgroup: its
                scan wave and its three trig waves have a compute unit to
                themselves
  one           the channel on one stream: one serial chain of phase steps,
                with one row of trig a block beside it

The last two split the kernel's time without stamps: a workgroup's blocks take
max(scan, trig) each, the scan is the same chain for 1 and for 16 streams, and
only the trig grows with the streams; so `one` is the scan (plus a sixteenth of
the trig work, on another wave) and `tile` - `one` is what the trig adds.

The CPU yardstick: oracle.apply_lo_pair over one stream of the same length on
one core, timed with the host clock and scaled by the number of streams.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "qpsk-modulator-demodulator_amd"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FS = 10_000_000
ALPHA = 0.4000000059604645
C3 = dict(streams=4096, sps=4, span=32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "channel_bench.json"))
    ap.add_argument("--streams", type=int, default=C3["streams"])
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--calls", type=int, default=2, help="timed calls a leg and round")
    ap.add_argument("--noise-rms", type=float, default=0.05)
    args = ap.parse_args()

    import numpy as np
    import torch
    import oracle as O
    import qpsk_amd as Q
    torch.cuda.init()
    dev = torch.device("cuda", 0)
    S, n, sps, span = args.streams, args.samples, C3["sps"], C3["span"]
    rs = FS // sps
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    iq, _ = Q.synth_generate(S, n, FS, rs, rrc_alpha=ALPHA, rrc_span=span, seed=0x5159534B, lo_ppm=0.0,
                             device=dev.index, stream=stream.cuda_stream)
    y32 = torch.empty_like(iq)
    y8 = torch.empty((S, 2 * n), dtype=torch.int8, device=dev)
    d = Q.BatchDemodulator(S, Q.params(FS, rs, ALPHA, span, device=dev.index, max_samples_per_call=n))
    d.set_stream(stream.cuda_stream)
    fresh = d.get_state()
    ms_sym = d.max_symbols(n)
    bits = torch.zeros((S, ((2 * ms_sym + 7) // 8 + 127) // 64 * 64), dtype=torch.uint8, device=dev)
    nbits = torch.zeros(S, dtype=torch.int64, device=dev)

    def channel(k, rms):
        ch = Q.Channel(k, sample_rate=float(FS), noise_rms=rms, noise_seed=7, device=dev.index)
        ch.set_stream(stream.cuda_stream)
        return ch

    chans = {"cf32": channel(S, 0.0), "cs8": channel(S, 0.0), "cf32_noise": channel(S, args.noise_rms),
             "cs8_noise": channel(S, args.noise_rms), "tile": channel(Q.CHANNEL_TILE_STREAMS, 0.0), "one": channel(1, 0.0)}

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

    def demod():
        d.set_state(fresh)
        return timed(lambda: d.process_device(y32, n, bits, nbits))

    legs = {
        "cf32": lambda: timed(lambda: chans["cf32"].apply_device(iq, n, out_dev=y32)),
        "cs8": lambda: timed(lambda: chans["cs8"].apply_device(iq, n, out_dev=y8, out_fmt="cs8")),
        "cf32_noise": lambda: timed(lambda: chans["cf32_noise"].apply_device(iq, n, out_dev=y32)),
        "cs8_noise": lambda: timed(lambda: chans["cs8_noise"].apply_device(iq, n, out_dev=y8, out_fmt="cs8")),
        "tile": lambda: timed(lambda: chans["tile"].apply_device(iq[: Q.CHANNEL_TILE_STREAMS], n,
                                                                 out_dev=y32[: Q.CHANNEL_TILE_STREAMS])),
        "one": lambda: timed(lambda: chans["one"].apply_device(iq[:1], n, out_dev=y32[:1])),
        "demod": demod,
    }
    rec = {"device": torch.cuda.get_device_name(dev), "streams": S, "samples": n, "sps": sps, "taps": sps * span + 1,
           "noise_rms": args.noise_rms, "tile_streams": Q.CHANNEL_TILE_STREAMS, "block_samples": Q.CHANNEL_BLOCK_SAMPLES,
           "runs": []}
    for name in ("cf32", "cs8", "cf32_noise", "tile", "one"):   # warm-up: code objects, first touches of the rows
        legs[name]()
    chans["cf32"].apply_device(iq, n, out_dev=y32)              # the demodulator's input, whichever leg ran last
    legs["demod"]()
    for rep in range(args.repeats):
        for name in ("cf32", "demod", "cs8", "cf32_noise", "cs8_noise", "tile", "one"):
            if name == "demod":
                chans["cf32"].apply_device(iq, n, out_dev=y32)
            run = {"leg": name, "repeat": rep, "ms": legs[name]()}
            rec["runs"].append(run)
            print(json.dumps(run), flush=True)
    for name in legs:
        ms = [m for r in rec["runs"] if r["leg"] == name for m in r["ms"]]
        rec[name + "_ms"] = ms
        rec[name + "_ms_median"] = round(statistics.median(ms), 3)
    rec["demod_bits_min_max"] = [int(nbits.min()), int(nbits.max())]
    gs = S * n / 1e9
    rec["gsamples_per_s"] = {k: round(gs / (rec[k + "_ms_median"] / 1e3), 3) for k in ("cf32", "cs8", "cf32_noise", "cs8_noise")}
    rec["channel_over_demod"] = round(rec["cf32_ms_median"] / rec["demod_ms_median"], 3)
    # the split: one stream is the scan chain, a full tile adds the trig of 15 more streams on three waves
    per = 1e6 / n   # ms a call -> ns a sample and stream chain
    rec["split"] = {"scan_ns_per_sample": round(rec["one_ms_median"] * per, 2),
                    "tile_ns_per_sample": round(rec["tile_ms_median"] * per, 2),
                    "full_batch_ns_per_sample_and_tile": round(rec["cf32_ms_median"] * per, 2),
                    "bound": "scan" if rec["tile_ms_median"] < 1.15 * rec["one_ms_median"] else "trig"}

    # the CPU yardstick, one core, one stream
    x = iq[0].cpu().numpy()
    tx, rx = O.OracleNCO(100e6, FS, 1, 0, seed=1000), O.OracleNCO(100e6, FS, 1, 0, seed=2000)
    t0 = time.perf_counter()
    want = O.apply_lo_pair(tx, rx, x)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    ref = Q.Channel(1, sample_rate=float(FS), device=dev.index)
    got = ref.apply_device(iq[:1].clone(), n).cpu().numpy()[0]
    ref.close()
    rec["cpu_one_stream_ms"] = round(cpu_ms, 2)
    rec["cpu_scaled_to_batch_ms"] = round(cpu_ms * S, 1)
    rec["cpu_scaled_over_device"] = round(cpu_ms * S / rec["cf32_ms_median"], 1)
    rec["one_stream_equals_oracle"] = bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))
    print(json.dumps({k: v for k, v in rec.items() if k != "runs"}), flush=True)
    for c in chans.values():
        c.close()
    d.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
