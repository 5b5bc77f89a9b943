#!/usr/bin/env python3
"""What resetting, reading and writing selected streams costs on one MI355X.

Writes one JSON file (--out, default profiles/stream_state_bench.json):

  idle      at the C3 shape (4096 streams, sps 4, 129 taps) on a handle with
            nothing queued: qpsk_demod_reset_streams, _get_streams_state and
            _set_streams_state of n = 1, 64 and 4096 rows (evenly spread over
            the batch) against the whole-blob qpsk_demod_get_state and
            _set_state of the same handle, alternated, --repeats times each;
            every time in ms, and the medians.  The C calls are timed on
            buffers made beforehand, so no Python copy of a blob is in them.
  pipeline  --calls pipelined C3 calls (2^20 samples a stream, device rows),
            plain, and with one reset_streams of 64 rows behind the middle
            call, alternated: wall time of the run, and of the reset call
            itself (the wait for the queued calls is in it).

The whole-blob calls are the yardstick: before these entry points they were
the only way to restart or move one stream.
"""
from __future__ import annotations

import argparse
import ctypes as C
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


def ms(fn):
    t0 = time.perf_counter()
    rc = fn()
    dt = (time.perf_counter() - t0) * 1e3
    if rc != 0:
        raise RuntimeError(f"status {rc}")
    return round(dt, 4)


def spread(S, n):
    return [k * (S // n) for k in range(n)]


def idle_legs(Q, d, repeats):
    L, h, S = Q.lib(), d._h, d.S
    whole = L.qpsk_demod_state_bytes(h)
    blob = C.create_string_buffer(whole)
    rec = {"streams": S, "taps": int(d.rrc_taps().size), "whole_blob_bytes": int(whole), "repeats": repeats, "rows": {}}
    times = {"get_state": [], "set_state": []}
    for n in (1, 64, S):
        ids = (C.c_int32 * n)(*spread(S, n))
        size = L.qpsk_demod_streams_state_bytes(h, n)
        sub = C.create_string_buffer(size)
        t = {"reset_streams": [], "get_streams_state": [], "set_streams_state": []}
        L.qpsk_demod_get_streams_state(h, ids, n, sub, size)   # warm-up: the staging buffer grows here
        for _ in range(repeats):
            t["get_streams_state"].append(ms(lambda: L.qpsk_demod_get_streams_state(h, ids, n, sub, size)))
            times["get_state"].append(ms(lambda: L.qpsk_demod_get_state(h, blob, whole)))
            t["set_streams_state"].append(ms(lambda: L.qpsk_demod_set_streams_state(h, ids, n, sub, size)))
            times["set_state"].append(ms(lambda: L.qpsk_demod_set_state(h, blob, whole)))
            t["reset_streams"].append(ms(lambda: L.qpsk_demod_reset_streams(h, ids, n)))
            L.qpsk_demod_set_state(h, blob, whole)   # the rows as they were
        rec["rows"][str(n)] = {"sub_blob_bytes": int(size), "ms": t,
                               "median_ms": {k: statistics.median(v) for k, v in t.items()}}
    rec["whole_blob"] = {"ms": times, "median_ms": {k: statistics.median(v) for k, v in times.items()}}
    return rec


def pipeline_leg(Q, torch, dev, d, x, n, calls, repeats):
    S = d.S
    msym = d.max_symbols(n)
    bits = torch.zeros((S, ((2 * msym + 7) // 8 + 63) // 64 * 64), dtype=torch.uint8, device=dev)
    nb = torch.zeros(S, dtype=torch.int64, device=dev)
    stream = torch.cuda.Stream(dev)
    d.set_stream(stream.cuda_stream)
    ids = spread(S, 64)
    runs = []

    def run(reset_at):
        reset_ms = None
        with torch.cuda.stream(stream):
            d.process_device_async(x, n, bits, nb)   # warm-up
            d.pipeline_wait()
            stream.synchronize()
            t0 = time.perf_counter()
            for k in range(calls):
                d.process_device_async(x, n, bits, nb)
                if k == reset_at:
                    t1 = time.perf_counter()
                    d.reset_streams(ids)
                    reset_ms = (time.perf_counter() - t1) * 1e3
            d.pipeline_wait()
            stream.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
        return round(dt, 3), None if reset_ms is None else round(reset_ms, 3)

    for rep in range(repeats):
        for kind, at in (("plain", None), ("reset", calls // 2 - 1)):
            wall, reset_ms = run(at)
            runs.append({"leg": kind, "repeat": rep, "wall_ms": wall, "ms_per_call": round(wall / calls, 3),
                         "reset_call_ms": reset_ms})
    med = {k: statistics.median(r["wall_ms"] for r in runs if r["leg"] == k) for k in ("plain", "reset")}
    return {"calls": calls, "samples": n, "reset_rows": 64, "reset_behind_call": calls // 2, "runs": runs,
            "median_wall_ms": med, "median_flush_cost_ms": round(med["reset"] - med["plain"], 3),
            "median_reset_call_ms": statistics.median(r["reset_call_ms"] for r in runs if r["leg"] == "reset"),
            "gate_timeouts": d.gate_timeouts()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_state_bench.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--pipeline-repeats", type=int, default=3)
    a = ap.parse_args()
    import torch
    torch.cuda.init()   # torch's HIP runtime first, then the library's
    import qpsk_amd as Q
    dev = torch.device("cuda", 0)
    S, n, rs = C3["streams"], a.samples, FS // C3["sps"]
    x, _ = Q.synth_generate(S, n, FS, rs, rrc_alpha=ALPHA, rrc_span=C3["span"], seed=0x5159534B, lo_ppm=1.0,
                            device=dev.index)
    d = Q.BatchDemodulator(S, Q.params(FS, rs, ALPHA, C3["span"], device=dev.index, max_samples_per_call=n))
    msym = d.max_symbols(n)
    bits = torch.zeros((S, ((2 * msym + 7) // 8 + 63) // 64 * 64), dtype=torch.uint8, device=dev)
    nb = torch.zeros(S, dtype=torch.int64, device=dev)
    d.process_device(x, n, bits, nb)   # every row holds a running receiver
    torch.cuda.synchronize(dev)
    del bits, nb
    out = {"device": torch.cuda.get_device_name(dev), "shape": dict(C3, taps=C3["sps"] * C3["span"] + 1),
           "idle": idle_legs(Q, d, a.repeats)}
    out["pipeline"] = pipeline_leg(Q, torch, dev, d, x, n, a.calls, a.pipeline_repeats)
    d.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"idle_median_ms": {k: v["median_ms"] for k, v in out["idle"]["rows"].items()},
                      "whole_blob_median_ms": out["idle"]["whole_blob"]["median_ms"],
                      "pipeline": {k: out["pipeline"][k] for k in ("median_wall_ms", "median_flush_cost_ms",
                                                                   "median_reset_call_ms", "gate_timeouts")}}))


if __name__ == "__main__":
    main()
