#!/usr/bin/env python3
"""CS16 against CF32 input on one MI355X, A/B x2 per leg on the same handle.

Writes one JSON file (--out, default profiles/cs16_bench.json):

  host_ring   the host_ring_c3 shape of bench.py (4096 streams, 2^18-sample
              chunks, sps 4, 129 taps, one pinned slot per chunk): GSa/s and
              H2D GB/s of a CF32 ring and of a CS16 ring, the ratio, and the
              stage times of the CS16 run (which stage bounds it);
  fir         the matched filter's kernel time (qpsk_demod_stage_times) at C3
              and at the C4 shard, 2^20 samples per stream in device memory,
              CS16 against CF32 rows, in synchronous calls ("alone") and in
              pipelined calls (beside the previous call's symbol loop).

Both formats carry the same samples: the synthesised batch quantised to int16
at half of full scale, and those int16 widened on the GPU (x * 2^-15) for the
CF32 legs, so the two formats must return the same bits, which is checked.
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
SHAPES = {"c3": dict(streams=4096, sps=4, span=32), "c4": dict(streams=4096, sps=8, span=8)}


def make_inputs(Q, torch, dev, cfg, n):
    """(x16 [S, 2n] int16, x32 [S, 2n] float32 = x16 * 2^-15), both on the device."""
    S = cfg["streams"]
    x32, _ = Q.synth_generate(S, n, FS, FS // cfg["sps"], rrc_alpha=ALPHA, rrc_span=cfg["span"], seed=0x5159534B,
                              lo_ppm=1.0, device=dev.index)
    peak = float(x32[:64].abs().max())
    x16 = torch.empty((S, 2 * n), dtype=torch.int16, device=dev)
    for r in range(0, S, 256):             # row blocks: no second float copy of the batch
        blk = x32[r: r + 256]
        q = (blk * (16384.0 / peak)).round_().clamp_(-32768, 32767).to(torch.int16)
        x16[r: r + 256] = q
        blk.copy_(q.to(torch.float32).mul_(2.0 ** -15))
    torch.cuda.synchronize(dev)
    return x16, x32


def fir_legs(Q, torch, dev, key, n, steps, repeats):
    cfg = SHAPES[key]
    S = cfg["streams"]
    x16, x32 = make_inputs(Q, torch, dev, cfg, n)
    d = Q.BatchDemodulator(S, Q.params(FS, FS // cfg["sps"], ALPHA, cfg["span"], device=dev.index,
                                       max_samples_per_call=n))
    ms = d.max_symbols(n)
    bits = torch.zeros((S, ((2 * ms + 7) // 8 + 63) // 64 * 64), dtype=torch.uint8, device=dev)
    nb = torch.zeros(S, dtype=torch.int64, device=dev)
    stream = torch.cuda.Stream(dev)
    d.set_stream(stream.cuda_stream)
    state0 = d.get_state()
    rec = {"streams": S, "samples": n, "taps": cfg["sps"] * cfg["span"] + 1, "steps": steps, "runs": []}
    first_bits = {}
    for rep in range(repeats):
        for fmt in ("cf32", "cs16"):
            for how in ("alone", "pipelined"):
                x = x16 if fmt == "cs16" else x32
                call = {("cf32", "alone"): d.process_device, ("cf32", "pipelined"): d.process_device_async,
                        ("cs16", "alone"): d.process_device_cs16,
                        ("cs16", "pipelined"): d.process_device_async_cs16}[(fmt, how)]
                d.set_state(state0)
                with torch.cuda.stream(stream):
                    call(x, n, bits, nb)            # warm-up, from the initial state
                    d.pipeline_wait()
                    stream.synchronize()
                    if rep == 0 and how == "alone":
                        first_bits[fmt] = (bits.cpu().numpy().copy(), nb.cpu().numpy().copy())
                    d.enable_timing(True)
                    t0 = time.perf_counter()
                    for _ in range(steps):
                        call(x, n, bits, nb)
                    d.pipeline_wait()
                    stream.synchronize()
                    dt = time.perf_counter() - t0
                st = d.stage_times()
                d.enable_timing(False)
                rec["runs"].append({"format": fmt, "calls": how, "repeat": rep, "fir_ms": round(st["fir"], 3),
                                    "loop_ms": round(st["loop"], 3), "ms_per_call": round(dt / steps * 1e3, 3),
                                    "GSa_s": round(S * n * steps / dt / 1e9, 2)})
    import numpy as np
    a, b = first_bits["cf32"], first_bits["cs16"]
    rec["bits_equal_between_formats"] = bool(np.array_equal(a[1], b[1]) and all(
        np.array_equal(a[0][s, : (int(a[1][s]) + 7) // 8], b[0][s, : (int(b[1][s]) + 7) // 8]) for s in range(S)))
    for how in ("alone", "pipelined"):
        for fmt in ("cf32", "cs16"):
            v = [r["fir_ms"] for r in rec["runs"] if r["format"] == fmt and r["calls"] == how]
            rec[f"fir_ms_{how}_{fmt}"] = v
    d.close()
    del x16, x32
    torch.cuda.empty_cache()
    return rec


def ring_run(Q, torch, dev, d, x, fmt, chunk, k, steps, warmup):
    S = d.S
    ring = Q.HostRing(d, k, fmt=fmt)
    for j in range(k):                     # slot j <- chunk j of every stream (D2H into pinned memory)
        slot = torch.from_numpy(ring.next_slot())
        slot[:, : 2 * chunk].copy_(x[:, 2 * chunk * j: 2 * chunk * (j + 1)])
        ring.submit(None, chunk)
    torch.cuda.synchronize(dev)
    bits0, nb0, _ = ring.collect()
    first = (bits0.copy(), nb0.copy())
    pending = k - 1

    def run(calls):
        nonlocal pending
        for _ in range(calls):
            if pending == k:
                ring.collect()
                pending -= 1
            ring.submit(None, chunk)
            pending += 1
        while pending:
            ring.collect()
            pending -= 1

    run(warmup * k)
    d.enable_timing(True)
    t0 = time.perf_counter()
    run(steps * k)
    dt = time.perf_counter() - t0
    st = d.stage_times()
    d.enable_timing(False)
    ring.close()
    bytes_per_sample = 4 if fmt == "cs16" else 8
    total = S * chunk * k * steps
    return {"format": fmt, "GSa_s": round(total / dt / 1e9, 3), "h2d_GBps": round(bytes_per_sample * total / dt / 1e9, 2),
            "ms_per_chunk": round(dt / (steps * k) * 1e3, 3),
            "stage_ms_per_chunk": {"fir": round(st["fir"], 3), "loop": round(st["loop"], 3)}}, first


def ring_legs(Q, torch, dev, n, chunk, steps, warmup, repeats):
    import numpy as np
    cfg = SHAPES["c3"]
    S, k = cfg["streams"], n // chunk
    x16, x32 = make_inputs(Q, torch, dev, cfg, n)
    rec = {"streams": S, "chunk": chunk, "chunks_per_step": k, "depth": k, "steps": steps, "runs": []}
    firsts = {}
    for rep in range(repeats):
        for fmt, x in (("cf32", x32), ("cs16", x16)):
            d = Q.BatchDemodulator(S, Q.params(FS, FS // cfg["sps"], ALPHA, cfg["span"], device=dev.index,
                                               max_samples_per_call=chunk))
            r, first = ring_run(Q, torch, dev, d, x, fmt, chunk, k, steps, warmup)
            d.close()
            torch.cuda.empty_cache()
            r["repeat"] = rep
            rec["runs"].append(r)
            firsts.setdefault(fmt, first)
    a, b = firsts["cf32"], firsts["cs16"]
    rec["bits_equal_between_formats"] = bool(np.array_equal(a[1], b[1]) and all(
        np.array_equal(a[0][s, : (int(a[1][s]) + 7) // 8], b[0][s, : (int(b[1][s]) + 7) // 8]) for s in range(S)))
    for fmt in ("cf32", "cs16"):
        rec[f"GSa_s_{fmt}"] = [r["GSa_s"] for r in rec["runs"] if r["format"] == fmt]
    rec["ratio_cs16_over_cf32"] = round(sum(rec["GSa_s_cs16"]) / sum(rec["GSa_s_cf32"]), 3)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cs16_bench.json"))
    ap.add_argument("--legs", default="ring,c3,c4", help="comma list of ring, c3, c4")
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--chunk", type=int, default=1 << 18)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=2)
    args = ap.parse_args()

    import torch
    import qpsk_amd as Q
    torch.cuda.init()
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(dev), "repeats": args.repeats}
    legs = [l for l in args.legs.split(",") if l]
    if "ring" in legs:
        out["host_ring"] = ring_legs(Q, torch, dev, args.samples, args.chunk, max(args.steps - 1, 1), 1, args.repeats)
        print(json.dumps({"host_ring": {k: v for k, v in out["host_ring"].items() if k != "runs"}}), flush=True)
    for key in ("c3", "c4"):
        if key in legs:
            out.setdefault("fir", {})[key] = fir_legs(Q, torch, dev, key, args.samples, args.steps, args.repeats)
            print(json.dumps({key: {k: v for k, v in out["fir"][key].items() if k != "runs"}}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
