#!/usr/bin/env python3
"""What a framed ring costs or saves against framing on the host, on one MI355X.

Two legs over the same CS8 slots, alternated in one run:

  A  a bits ring (qpsk_rx_collect), then qpsk_tsc_find per stream and one
     qpsk_framer_push over the batch on the collecting thread: what
     INTEGRATION's ring example did before the ring could own a framer;
  B  a framed ring with keep_bits = 0 (qpsk_rx_collect_frames).

Shapes: host_ring_c3 of bench.py (4096 streams, sps 4, 129 taps) and C2's
streams (256, sps 8, 65 taps), chunks of --chunk samples, --depth slots.

Traffics:
  frames  every row is one qpsk_mod_modulate_bytes frame (TSC, MESSAGE_START,
          the testAtDataLevel text, MESSAGE_STOP) repeated, started at another
          sample per stream, quantised to int8 at half of full scale; the legs
          search for the TSC and the markers;
  noise   uniform int8 noise and no TSC, so that every bit of every chunk
          reaches the start hunt and no search exits early (its worst case).

Per run: GSa/s, ms per chunk, host ms per chunk spent after collect returned,
D2H bytes per chunk, frames per chunk, and the kernels' own ms per chunk
(matched filter, symbol loop: qpsk_demod_stage_times).  Per shape and traffic
also the device framer chain alone (TSC search, framer step, packing) on one
chunk's bit rows, timed by events on an idle device.  The legs must return
the same frames, which is checked on the first chunks.

Writes one JSON file (--out, default profiles/rx_frames_bench.json).
"""
from __future__ import annotations

import argparse
import ctypes as C
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
TSC = "11001010011101100100100110101100" + "01110100111001011010001101101001"
START, END = b"MESSAGE_START", b"MESSAGE_STOP"
TEXT = b"The Quick Brown fox jump yes yes man good!"
SHAPES = {"host_ring_c3": dict(streams=4096, sps=4, span=32), "c2": dict(streams=256, sps=8, span=8)}
MAX_FRAME = 128
RING = 1 << 16      # framer ring bytes a stream: entering a frame appends the rest of the chunk's bits (16 KiB at C3)


def make_slots(Q, torch, dev, cfg, traffic, chunk, depth):
    """depth device tensors [S, 2 chunk] int8."""
    S = cfg["streams"]
    if traffic == "noise":
        g = torch.Generator(device=dev).manual_seed(5)
        return [torch.randint(-64, 65, (S, 2 * chunk), dtype=torch.int8, device=dev, generator=g)
                for _ in range(depth)]
    import numpy as np
    m = Q.QPSKModulator(FS, FS // cfg["sps"], ALPHA, cfg["span"], tsc=TSC, device=dev.index)
    frame = m.ModulateBytes(TEXT, START, END)
    m.close()
    n_frame = frame.size // 2
    reps = (chunk * depth + n_frame) // n_frame + 2
    q = np.round(np.tile(frame, reps) * (64.0 / np.abs(frame).max())).astype(np.int8)
    row = torch.from_numpy(q).to(dev)
    slots = [torch.empty((S, 2 * chunk), dtype=torch.int8, device=dev) for _ in range(depth)]
    for s in range(S):
        a = 2 * ((37 * s) % n_frame)
        for j in range(depth):
            slots[j][s].copy_(row[a + 2 * chunk * j: a + 2 * chunk * (j + 1)])
    torch.cuda.synchronize(dev)
    return slots


def open_ring(Q, torch, dev, cfg, slots, chunk, depth, framed, tsc):
    S = cfg["streams"]
    d = Q.BatchDemodulator(S, Q.params(FS, FS // cfg["sps"], ALPHA, cfg["span"], device=dev.index,
                                       max_samples_per_call=chunk))
    ring = Q.HostRing.create_fmt(d, depth, "cs8")
    if framed:
        ring.attach_framer(START, END, tsc=tsc, ring_capacity=RING, max_frame_bytes=MAX_FRAME, keep_bits=False)
    for j in range(depth):                 # slot j <- chunk j, once: the slots are resubmitted in place
        torch.from_numpy(ring.next_slot())[:, : 2 * chunk].copy_(slots[j])
        ring.submit(None, chunk)
    torch.cuda.synchronize(dev)
    return d, ring


def leg(Q, torch, dev, cfg, slots, chunk, depth, steps, warmup, framed, tsc):
    import numpy as np
    L = Q.lib()
    S = cfg["streams"]
    d, ring = open_ring(Q, torch, dev, cfg, slots, chunk, depth, framed, tsc)
    stride = ring.bits_stride
    u8p, i64p = C.POINTER(C.c_uint8), C.POINTER(C.c_int64)
    lens = np.zeros(S, np.int64)
    off = np.zeros(S, np.int64)
    ticket = C.c_int64()
    host_s = [0.0]
    seen = []                              # per collected chunk: {stream: frame}
    d2h = []
    if framed:
        buf = np.zeros(ring.frames_bytes(), np.uint8)

        def collect():
            rc = L.qpsk_rx_collect_frames(ring._r, buf.ctypes.data_as(u8p), buf.size, off.ctypes.data_as(i64p),
                                          lens.ctypes.data_as(i64p), None, 0, None, C.byref(ticket))
            assert rc in (0, Q.QPSK_ERR_CAPACITY), L.qpsk_last_error()   # a truncated frame is flagged
            t0 = time.perf_counter()
            held = np.minimum(lens, MAX_FRAME)
            got = {int(s): bytes(buf[off[s]: off[s] + held[s]]) for s in np.flatnonzero(off >= 0)}
            host_s[0] += time.perf_counter() - t0
            seen.append(got)
            last = int(off.argmax())
            d2h.append((2 * S + 2) * 8 + (int(off[last]) + (int(held[last]) + 15) // 16 * 16 if got else 0))
    else:
        bits = np.zeros((S, stride), np.uint8)
        nb = np.zeros(S, np.int64)
        pay = np.zeros((S, MAX_FRAME), np.uint8)
        fr = Q.Framer(S, START, END, ring_capacity=RING)
        rows = [C.cast(bits.ctypes.data + s * stride, u8p) for s in range(S)]
        tsc_b = tsc.encode() if tsc else None

        def collect():
            rc = L.qpsk_rx_collect(ring._r, bits.ctypes.data_as(u8p), stride, nb.ctypes.data_as(i64p), C.byref(ticket))
            assert rc == 0, L.qpsk_last_error()
            t0 = time.perf_counter()
            for s in range(S):             # HandleBits: qpsk_tsc_find + qpsk_framer_push
                off[s] = L.qpsk_tsc_find(rows[s], int(nb[s]), tsc_b)
            rc = L.qpsk_framer_push(fr._h, bits.ctypes.data_as(u8p), stride, off.ctypes.data_as(i64p),
                                    nb.ctypes.data_as(i64p), pay.ctypes.data_as(u8p), MAX_FRAME,
                                    lens.ctypes.data_as(i64p))
            assert rc == 0, L.qpsk_last_error()
            got = {int(s): bytes(pay[s, : lens[s]]) for s in np.flatnonzero(lens > 0)}
            host_s[0] += time.perf_counter() - t0
            seen.append(got)
            d2h.append(S * 8 + S * ((int(nb.max()) + 7) // 8))

    pending = depth

    def run(calls):
        nonlocal pending
        for _ in range(calls):
            if pending == depth:
                collect()
                pending -= 1
            ring.submit(None, chunk)
            pending += 1
        while pending:
            collect()
            pending -= 1

    run(warmup * depth)
    first = seen[: 2 * depth]
    host_s[0], n0 = 0.0, len(seen)
    d.enable_timing(True)
    t0 = time.perf_counter()
    run(steps * depth)
    dt = time.perf_counter() - t0
    st = d.stage_times()
    d.enable_timing(False)
    chunks = len(seen) - n0
    last_bits = None if framed else (bits.copy(), nb.copy())
    ring.close()
    d.close()
    torch.cuda.empty_cache()
    rec = {"leg": "B framed ring" if framed else "A bits ring + host framer",
           "GSa_s": round(S * chunk * chunks / dt / 1e9, 3), "ms_per_chunk": round(dt / chunks * 1e3, 3),
           "host_ms_per_chunk_after_collect": round(host_s[0] / chunks * 1e3, 3),
           "d2h_bytes_per_chunk": int(sum(d2h[n0:]) / chunks),
           "frames_per_chunk": round(sum(len(g) for g in seen[n0:]) / chunks, 1),
           "kernel_ms_per_chunk": {"fir": round(st["fir"], 3), "loop": round(st["loop"], 3),
                                   "span": round(st["total"], 3)}}
    return rec, first, last_bits


def chain_alone(Q, torch, dev, S, bits, nb, tsc, repeats=5):
    """The device framer chain on one chunk's bit rows, idle device: ms per step, median."""
    st = torch.cuda.Stream(dev)
    fr = Q.DeviceFramer(S, START, END, ring_capacity=RING, device=dev.index)
    fr.set_stream(st.cuda_stream)
    with torch.cuda.stream(st):
        bd, nbd = torch.from_numpy(bits).to(dev), torch.from_numpy(nb).to(dev)
        offs = torch.zeros(S, dtype=torch.int64, device=dev)
        pay = torch.zeros((S, MAX_FRAME), dtype=torch.uint8, device=dev)
        npay = torch.zeros(S, dtype=torch.int64, device=dev)
        packed = torch.zeros(S * MAX_FRAME, dtype=torch.uint8, device=dev)
        poff = torch.zeros(S, dtype=torch.int64, device=dev)
        head = torch.zeros(2, dtype=torch.int64, device=dev)
        ms = {"tsc": [], "framer": [], "pack": []}
        for _ in range(repeats + 1):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record(st)
            Q.tsc_find_device(bd, nbd, tsc, offs, st.cuda_stream)
            ev[1].record(st)
            fr.push(bd, nbd, pay, npay, offs)
            ev[2].record(st)
            Q.frames_pack_device(pay, npay, packed, poff, head, st.cuda_stream)
            ev[3].record(st)
            st.synchronize()
            for k, name in enumerate(ms):
                ms[name].append(ev[k].elapsed_time(ev[k + 1]))
    med = lambda v: sorted(v[1:])[len(v[1:]) // 2]   # noqa: E731  (the first step grows the scratch)
    out = {k: round(med(v), 4) for k, v in ms.items()}
    out["total"] = round(sum(out.values()), 4)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rx_frames_bench.json"))
    ap.add_argument("--shapes", default="host_ring_c3,c2")
    ap.add_argument("--chunk", type=int, default=1 << 18)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=2)
    args = ap.parse_args()

    import torch
    import qpsk_amd as Q
    torch.cuda.init()
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(dev), "chunk": args.chunk, "depth": args.depth, "steps": args.steps,
           "repeats": args.repeats, "format": "cs8", "max_frame_bytes": MAX_FRAME, "shapes": {}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    for key in [k for k in args.shapes.split(",") if k]:
        cfg = SHAPES[key]
        rec = out["shapes"].setdefault(key, {"streams": cfg["streams"], "taps": cfg["sps"] * cfg["span"] + 1})
        for traffic in ("frames", "noise"):
            tsc = TSC if traffic == "frames" else None
            slots = make_slots(Q, torch, dev, cfg, traffic, args.chunk, args.depth)
            t = rec.setdefault(traffic, {"tsc": bool(tsc), "runs": []})
            firsts, last_bits = {}, None
            for rep in range(args.repeats):
                for framed in (False, True):
                    r, first, lb = leg(Q, torch, dev, cfg, slots, args.chunk, args.depth, args.steps, args.warmup,
                                       framed, tsc)
                    r["repeat"] = rep
                    t["runs"].append(r)
                    firsts.setdefault(framed, first)
                    last_bits = lb or last_bits
                    print(json.dumps({key: {traffic: r}}), flush=True)
            t["frames_equal_between_legs"] = firsts[False] == firsts[True]
            t["frames_in_first_chunks"] = sum(len(g) for g in firsts[True])
            t["device_framer_chain_alone_ms"] = chain_alone(Q, torch, dev, cfg["streams"], *last_bits, tsc)
            for name, framed in (("A", False), ("B", True)):
                runs = [r for r in t["runs"] if r["leg"].startswith(name)]
                for k in ("GSa_s", "ms_per_chunk", "host_ms_per_chunk_after_collect", "d2h_bytes_per_chunk"):
                    t[f"{k}_{name}"] = [r[k] for r in runs]
                t[f"fir_ms_{name}"] = [r["kernel_ms_per_chunk"]["fir"] for r in runs]
            t["GSa_s_ratio_B_over_A"] = round(sum(t["GSa_s_B"]) / sum(t["GSa_s_A"]), 3)
            del slots
            torch.cuda.empty_cache()
            save()
    print(json.dumps({k: {tr: {n: v for n, v in t.items() if n != "runs"} for tr, t in s.items() if isinstance(t, dict)}
                      for k, s in out["shapes"].items()}), flush=True)


if __name__ == "__main__":
    main()
