#!/usr/bin/env python3
"""CS8 against CS16 and CF32 input on one MI355X, the legs alternated on one box.

Writes one JSON file (--out, default profiles/int8_bench.json):

  host_ring   the host_ring_c3 shape of bench.py (4096 streams, 2^18-sample
              chunks, sps 4, 129 taps, one pinned slot per chunk): GSa/s, H2D
              GB/s and ms per chunk of a CF32, a CS16 and a CS8 ring, the
              kernels' own ms per chunk (matched filter, symbol loop), and the
              ratios to the CS16 leg;
  fir         the matched filter's kernel time (qpsk_demod_stage_times) at C3
              and at the C4 shard, 2^20 samples per stream in device memory,
              CS8 against CS16 rows, in synchronous calls ("alone") and in
              pipelined calls (beside the previous call's symbol loop).

Every format carries the same samples: the synthesised batch quantised to int8
at half of full scale (+-64), those values times 256 as int16 (x * 256 * 2^-15 =
x * 2^-7 exactly) and widened on the GPU for the CF32 leg, so the formats must
return the same bits, which is checked.
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
SAMPLE_BYTES = {"cf32": 8, "cs16": 4, "cs8": 2}


def make_inputs(Q, torch, dev, cfg, n, fmts):
    """{fmt: [S, 2n] device rows} of the same samples in every format asked for."""
    S = cfg["streams"]
    x32, _ = Q.synth_generate(S, n, FS, FS // cfg["sps"], rrc_alpha=ALPHA, rrc_span=cfg["span"], seed=0x5159534B,
                              lo_ppm=1.0, device=dev.index)
    peak = float(x32[:64].abs().max())
    x8 = torch.empty((S, 2 * n), dtype=torch.int8, device=dev)
    for r in range(0, S, 256):             # row blocks: no second float copy of the batch
        blk = x32[r: r + 256]
        q = (blk * (64.0 / peak)).round_().clamp_(-128, 127).to(torch.int8)
        x8[r: r + 256] = q
        if "cf32" in fmts:
            blk.copy_(q.to(torch.float32).mul_(2.0 ** -7))
    out = {"cs8": x8}
    if "cf32" in fmts:
        out["cf32"] = x32
    else:
        del x32
    if "cs16" in fmts:
        x16 = torch.empty((S, 2 * n), dtype=torch.int16, device=dev)
        for r in range(0, S, 256):
            x16[r: r + 256] = x8[r: r + 256].to(torch.int16) * 256
        out["cs16"] = x16
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    return out


def rows_equal(np, a, b, S):
    return bool(np.array_equal(a[1], b[1]) and all(
        np.array_equal(a[0][s, : (int(a[1][s]) + 7) // 8], b[0][s, : (int(b[1][s]) + 7) // 8]) for s in range(S)))


def mean(v):
    return sum(v) / len(v)


def fir_legs(Q, torch, dev, key, n, steps, repeats):
    import numpy as np
    cfg = SHAPES[key]
    S = cfg["streams"]
    fmts = ("cs16", "cs8")
    x = make_inputs(Q, torch, dev, cfg, n, fmts)
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
        for fmt in fmts:
            for how in ("alone", "pipelined"):
                call = d.process_device_fmt if how == "alone" else d.process_device_async_fmt
                d.set_state(state0)
                with torch.cuda.stream(stream):
                    call(x[fmt], n, bits, nb, fmt)            # warm-up, from the initial state
                    d.pipeline_wait()
                    stream.synchronize()
                    if rep == 0 and how == "alone":
                        first_bits[fmt] = (bits.cpu().numpy().copy(), nb.cpu().numpy().copy())
                    d.enable_timing(True)
                    t0 = time.perf_counter()
                    for _ in range(steps):
                        call(x[fmt], n, bits, nb, fmt)
                    d.pipeline_wait()
                    stream.synchronize()
                    dt = time.perf_counter() - t0
                st = d.stage_times()
                d.enable_timing(False)
                rec["runs"].append({"format": fmt, "calls": how, "repeat": rep, "fir_ms": round(st["fir"], 3),
                                    "loop_ms": round(st["loop"], 3), "ms_per_call": round(dt / steps * 1e3, 3),
                                    "GSa_s": round(S * n * steps / dt / 1e9, 2)})
    rec["bits_equal_between_formats"] = rows_equal(np, first_bits["cs16"], first_bits["cs8"], S)
    for how in ("alone", "pipelined"):
        for fmt in fmts:
            rec[f"fir_ms_{how}_{fmt}"] = [r["fir_ms"] for r in rec["runs"] if r["format"] == fmt and r["calls"] == how]
            rec[f"GSa_s_{how}_{fmt}"] = [r["GSa_s"] for r in rec["runs"] if r["format"] == fmt and r["calls"] == how]
        rec[f"fir_ms_ratio_cs8_over_cs16_{how}"] = round(mean(rec[f"fir_ms_{how}_cs8"]) /
                                                         mean(rec[f"fir_ms_{how}_cs16"]), 4)
        rec[f"GSa_s_ratio_cs8_over_cs16_{how}"] = round(mean(rec[f"GSa_s_{how}_cs8"]) /
                                                        mean(rec[f"GSa_s_{how}_cs16"]), 4)
    d.close()
    del x
    torch.cuda.empty_cache()
    return rec


def ring_run(Q, torch, dev, d, x, fmt, chunk, k, steps, warmup):
    S = d.S
    ring = Q.HostRing.create_fmt(d, k, fmt)
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
    total = S * chunk * k * steps
    return {"format": fmt, "GSa_s": round(total / dt / 1e9, 3),
            "h2d_GBps": round(SAMPLE_BYTES[fmt] * total / dt / 1e9, 2),
            "ms_per_chunk": round(dt / (steps * k) * 1e3, 3),
            "kernel_ms_per_chunk": {"fir": round(st["fir"], 3), "loop": round(st["loop"], 3),
                                    "span": round(st["total"], 3)}}, first


def ring_legs(Q, torch, dev, n, chunk, steps, warmup, repeats):
    import numpy as np
    cfg = SHAPES["c3"]
    S, k = cfg["streams"], n // chunk
    fmts = ("cf32", "cs16", "cs8")
    x = make_inputs(Q, torch, dev, cfg, n, fmts)
    rec = {"streams": S, "chunk": chunk, "chunks_per_step": k, "depth": k, "steps": steps, "runs": []}
    firsts = {}
    for rep in range(repeats):
        for fmt in fmts:
            d = Q.BatchDemodulator(S, Q.params(FS, FS // cfg["sps"], ALPHA, cfg["span"], device=dev.index,
                                               max_samples_per_call=chunk))
            r, first = ring_run(Q, torch, dev, d, x[fmt], fmt, chunk, k, steps, warmup)
            d.close()
            torch.cuda.empty_cache()
            r["repeat"] = rep
            rec["runs"].append(r)
            firsts.setdefault(fmt, first)
            print(json.dumps(r), flush=True)
    rec["bits_equal_between_formats"] = all(rows_equal(np, firsts["cs16"], firsts[f], S) for f in ("cf32", "cs8"))
    for fmt in fmts:
        rec[f"GSa_s_{fmt}"] = [r["GSa_s"] for r in rec["runs"] if r["format"] == fmt]
        rec[f"h2d_GBps_{fmt}"] = [r["h2d_GBps"] for r in rec["runs"] if r["format"] == fmt]
    for fmt in ("cf32", "cs8"):
        rec[f"ratio_{fmt}_over_cs16"] = round(mean(rec[f"GSa_s_{fmt}"]) / mean(rec["GSa_s_cs16"]), 3)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "int8_bench.json"))
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
    if os.path.exists(args.out):           # legs measured by an earlier run of this tool stay
        with open(args.out) as f:
            out.update({k: v for k, v in json.load(f).items() if k in ("host_ring", "fir")})
    legs = [l for l in args.legs.split(",") if l]

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    if "ring" in legs:
        out["host_ring"] = ring_legs(Q, torch, dev, args.samples, args.chunk, max(args.steps - 1, 1), 1, args.repeats)
        print(json.dumps({"host_ring": {k: v for k, v in out["host_ring"].items() if k != "runs"}}), flush=True)
        save()
    for key in ("c3", "c4"):
        if key in legs:
            out.setdefault("fir", {})[key] = fir_legs(Q, torch, dev, key, args.samples, args.steps, args.repeats)
            print(json.dumps({key: {k: v for k, v in out["fir"][key].items() if k != "runs"}}), flush=True)
            save()


if __name__ == "__main__":
    main()
