#!/usr/bin/env python3
"""What counting bit errors costs on one MI355X, on the device and as bench.py
does it, the legs alternated in one run.

Writes one JSON file (--out, default profiles/ber_count_bench.json).  The C3
shape (4096 streams x 2^20 samples, sps 4, 129 taps) is synthesised in device
memory (qpsk_synth_generate, which also leaves the transmitted bits there) and
demodulated once from a fresh handle; the bit rows stay where they are.  Legs,
--repeats rounds of each in turn:

  device     qpsk_ber_count_device over all 4096 streams, timed with device
             events around the launch (--launches of them, each reported)
  device256  the same over the first 256 streams alone: a launch takes as long
             as its slowest stream, and one stream of 4096 that never locates
             (the worst case below) sets the time of the whole batch
  host32     bench.ber_after_lock over the first 32 streams (what the headline
  host256    benchmark counts), and over 256: a host clock around the call and
             a synchronise, the downloads of both packed rows included

The device rows of the first 32 and 256 streams are summed and compared with
what ber_after_lock returned.  Then, once, the known worst case: received rows
of random bits (no stretch of them occurs in the reference), so no window is
ever located and every window scans min(N, w + 4 W) positions.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "qpsk-modulator-demodulator_amd"), os.path.join(ROOT, "oracle"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FS = 10_000_000
ALPHA = 0.4000000059604645
C3 = dict(streams=4096, sps=4, span=32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ber_count_bench.json"))
    ap.add_argument("--streams", type=int, default=C3["streams"])
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--esn0-db", type=float, default=None, help="AWGN Es/N0 of the batch (default: none, as C3)")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--launches", type=int, default=3)
    args = ap.parse_args()

    import torch
    import bench
    import qpsk_amd as Q
    torch.cuda.init()
    dev = torch.device("cuda", 0)
    S, n, sps, span = args.streams, args.samples, C3["sps"], C3["span"]
    rs = FS // sps
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    iq, tx = Q.synth_generate(S, n, FS, rs, rrc_alpha=ALPHA, rrc_span=span, seed=0x5159534B, lo_ppm=1.0,
                              esn0_db=args.esn0_db, device=dev.index, stream=stream.cuda_stream)
    d = Q.BatchDemodulator(S, Q.params(FS, rs, ALPHA, span, device=dev.index, max_samples_per_call=n))
    d.set_stream(stream.cuda_stream)
    ms = d.max_symbols(n)
    bits = torch.zeros((S, ((2 * ms + 7) // 8 + 127) // 64 * 64), dtype=torch.uint8, device=dev)
    nbits = torch.zeros(S, dtype=torch.int64, device=dev)
    d.process_device(iq, n, bits, nbits)
    stream.synchronize()
    d.close()
    del iq
    torch.cuda.empty_cache()
    n_ref = torch.full((S,), 8 * tx.shape[1], dtype=torch.int64, device=dev)
    out_dev = torch.zeros((S, 64), dtype=torch.uint8, device=dev)
    rec = {"device": torch.cuda.get_device_name(dev), "streams": S, "samples": n, "sps": sps, "taps": sps * span + 1,
           "esn0_db": args.esn0_db, "bits_per_stream_min_max": [int(nbits.min()), int(nbits.max())],
           "params": dict(skip_bits=8000, window=2048, key_bits=64, search=512), "runs": []}

    def device_leg(k):
        ms_each = []
        for _ in range(args.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            Q.ber_count_device(bits[:k], nbits[:k], tx[:k], n_ref[:k], out_dev=out_dev[:k], hip_stream=stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            ms_each.append(round(e0.elapsed_time(e1), 4))
        return {"leg": "device" if k == S else f"device{k}", "streams": k, "ms": ms_each}

    def host_leg(k):
        stream.synchronize()
        t0 = time.perf_counter()
        got = bench.ber_after_lock(bits, nbits, tx, k)
        stream.synchronize()
        return {"leg": f"host{k}", "streams": k, "ms": [round((time.perf_counter() - t0) * 1e3, 2)],
                "counts": [int(v) for v in got]}

    Q.ber_count_device(bits, nbits, tx, n_ref, out_dev=out_dev, hip_stream=stream.cuda_stream)   # warm-up
    stream.synchronize()
    hosts = sorted({min(S, 32), min(S, 256)})
    for rep in range(args.repeats):
        for leg in [lambda: device_leg(hosts[-1]), lambda: device_leg(S)] + [lambda k=k: host_leg(k) for k in hosts]:
            run = dict(leg(), repeat=rep)
            rec["runs"].append(run)
            print(json.dumps(run), flush=True)
    rows = out_dev.cpu().numpy().view(Q.BER_ROW_DTYPE).reshape(-1)
    rec["all_streams"] = Q.ber_summary(rows)
    rec["streams_located"] = int(rows["located"].sum())
    for k in hosts:
        s = Q.ber_summary(rows[:k])
        want = next(r["counts"] for r in rec["runs"] if r["leg"] == f"host{k}")
        rec[f"first_{k}"] = s
        rec[f"first_{k}_equal_ber_after_lock"] = [s["bit_errors"], s["bits"], s["lost_windows"], s["symbol_slips"]] == want
    rec["device_ms"] = [m for r in rec["runs"] if r["leg"] == "device" for m in r["ms"]]
    rec[f"device{hosts[-1]}_ms"] = [m for r in rec["runs"] if r["leg"] == f"device{hosts[-1]}" for m in r["ms"]]
    rec[f"first_{hosts[-1]}_located"] = int(rows["located"][:hosts[-1]].sum())
    # the windows of the streams that never located: each scanned min(N, w + 4 W) positions
    rec["windows_of_streams_never_located"] = int(rows["windows"][rows["located"] == 0].sum())
    for k in hosts:
        rec[f"host{k}_ms"] = [m for r in rec["runs"] if r["leg"] == f"host{k}" for m in r["ms"]]

    # the worst case, once: nothing in the received rows occurs in the reference
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    noise = torch.randint(0, 256, tuple(bits.shape), dtype=torch.uint8, device=dev, generator=g)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream.synchronize()
    e0.record(stream)
    Q.ber_count_device(noise, nbits, tx, n_ref, out_dev=out_dev, hip_stream=stream.cuda_stream)
    e1.record(stream)
    e1.synchronize()
    worst = out_dev.cpu().numpy().view(Q.BER_ROW_DTYPE).reshape(-1)
    rec["never_located"] = {"ms": round(e0.elapsed_time(e1), 2), "streams": S, "summary": Q.ber_summary(worst),
                            "windows": int(worst["windows"].sum()), "streams_located": int(worst["located"].sum())}
    print(json.dumps({k: v for k, v in rec.items() if k != "runs"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
