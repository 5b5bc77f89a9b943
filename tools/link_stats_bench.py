#!/usr/bin/env python3
"""What link statistics cost on one MI355X: statistics off against on, the
legs alternated in one run.

Writes one JSON file (--out, default profiles/link_stats_bench.json).  Per
shape (C3: 4096 streams, sps 4, 129 taps; C2: 256 streams, sps 8, 65 taps),
2^20 samples per stream resident in device memory, pipelined calls
(qpsk_demod_process_async) without symbol rows: GSa/s over the timed calls and
the kernels' own milliseconds per call (matched filter, symbol loop, from
qpsk_demod_stage_times), statistics off and on in turn, --repeats rounds.  With
statistics on the symbol loop runs its symbol-carrying form (more LDS: at C3
one matched-filter workgroup less fits beside it); a
third leg, statistics off and symbol rows asked for, runs that form without
the sums, which tells the form's cost from the sums' own.  The bits of the
legs are compared, and the statistics of the last on leg are summarised (mean
dist2 / mean power over the batch).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "qpsk-modulator-demodulator_amd"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FS = 10_000_000
ALPHA = 0.4000000059604645
SHAPES = {"c3": dict(streams=4096, sps=4, span=32), "c2": dict(streams=256, sps=8, span=8)}


def mean(v):
    return sum(v) / len(v)


def legs(Q, torch, dev, key, n, steps, repeats):
    import numpy as np
    cfg = SHAPES[key]
    S = cfg["streams"]
    x, _ = Q.synth_generate(S, n, FS, FS // cfg["sps"], rrc_alpha=ALPHA, rrc_span=cfg["span"], seed=0x5159534B,
                            lo_ppm=1.0, device=dev.index)
    d = Q.BatchDemodulator(S, Q.params(FS, FS // cfg["sps"], ALPHA, cfg["span"], device=dev.index,
                                       max_samples_per_call=n))
    ms = d.max_symbols(n)
    bits = torch.zeros((S, ((2 * ms + 7) // 8 + 63) // 64 * 64), dtype=torch.uint8, device=dev)
    nb = torch.zeros(S, dtype=torch.int64, device=dev)
    syms = torch.zeros((S, 2 * ms), dtype=torch.float32, device=dev)
    ns = torch.zeros(S, dtype=torch.int64, device=dev)
    stream = torch.cuda.Stream(dev)
    d.set_stream(stream.cuda_stream)
    state0 = d.get_state()
    rec = {"streams": S, "samples": n, "taps": cfg["sps"] * cfg["span"] + 1, "steps": steps, "runs": []}
    first_bits, stats = {}, None
    for rep in range(repeats):
        for leg in ("off", "on", "rows"):
            on = leg == "on"
            out = dict(syms_dev=syms, n_syms_dev=ns) if leg == "rows" else {}
            d.set_state(state0)
            d.enable_link_stats(on)
            with torch.cuda.stream(stream):
                d.process_device_async(x, n, bits, nb, **out)   # warm-up, from the initial state
                d.pipeline_wait()
                stream.synchronize()
                if rep == 0:
                    first_bits[leg] = (bits.cpu().numpy().copy(), nb.cpu().numpy().copy())
                d.enable_timing(True)
                t0 = time.perf_counter()
                for _ in range(steps):
                    d.process_device_async(x, n, bits, nb, **out)
                d.pipeline_wait()
                stream.synchronize()
                dt = time.perf_counter() - t0
            st = d.stage_times()
            d.enable_timing(False)
            if on:
                stats = d.link_stats()
            run = {"leg": leg, "link_stats": on, "symbol_rows": leg == "rows", "repeat": rep,
                   "fir_ms": round(st["fir"], 3), "loop_ms": round(st["loop"], 3), "ms_per_call": round(dt / steps * 1e3, 3),
                   "GSa_s": round(S * n * steps / dt / 1e9, 2)}
            rec["runs"].append(run)
            print(json.dumps({key: run}), flush=True)
    a = first_bits["off"]
    rec["bits_equal_in_every_leg"] = all(bool(np.array_equal(a[1], b[1]) and all(
        np.array_equal(a[0][s, : (int(a[1][s]) + 7) // 8], b[0][s, : (int(b[1][s]) + 7) // 8]) for s in range(S)))
        for b in (first_bits["on"], first_bits["rows"]))
    for name in ("off", "on", "rows"):
        for k in ("GSa_s", "fir_ms", "loop_ms"):
            rec[f"{k}_{name}"] = [r[k] for r in rec["runs"] if r["leg"] == name]
    for k in ("GSa_s", "fir_ms", "loop_ms"):
        rec[f"{k}_ratio_on_over_off"] = round(mean(rec[f"{k}_on"]) / mean(rec[f"{k}_off"]), 4)
        rec[f"{k}_ratio_rows_over_off"] = round(mean(rec[f"{k}_rows"]) / mean(rec[f"{k}_off"]), 4)
    nsym = stats["n_symbols"].astype(np.float64)
    rec["statistics_of_the_last_on_leg"] = {
        "calls_counted": steps + 1,
        "symbols_per_stream_min_max": [int(stats["n_symbols"].min()), int(stats["n_symbols"].max())],
        "mean_dist2_over_mean_power_median": round(float(np.median(stats["sum_dist2"] / stats["sum_power"])), 6),
        "mean_power_median": round(float(np.median(stats["sum_power"] / nsym)), 6),
        "streams_with_abs_costas_freq_above_1": int((np.abs(stats["costas_freq"]) > 1.0).sum()),
    }
    d.close()
    del x
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_stats_bench.json"))
    ap.add_argument("--legs", default="c3,c2", help="comma list of c3, c2")
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=2)
    args = ap.parse_args()

    import torch
    import qpsk_amd as Q
    torch.cuda.init()
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(dev), "repeats": args.repeats}
    for key in [l for l in args.legs.split(",") if l]:
        out[key] = legs(Q, torch, dev, key, args.samples, args.steps, args.repeats)
        print(json.dumps({key: {k: v for k, v in out[key].items() if k != "runs"}}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
