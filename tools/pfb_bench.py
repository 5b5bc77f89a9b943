#!/usr/bin/env python3
"""What the polyphase channeliser (qpsk_pfb_apply_fmt) costs on one MI355X, the
legs alternated in one run.

Writes one JSON file (--out, default profiles/pfb_bench.json).  The shape is 4
bands x M = 1024 channels, K = 8 taps a branch, 2^18 frames a call: 4096 output
rows, 8.6 GB out and 4.3 GB in at CF32.  The wideband rows are seeded noise in
device memory; every handle has taken one call before it is timed, so a timed
call reads its history and emits exactly 2^18 frames.  Legs, --repeats rounds
of each in turn, every one timed with device events around calls queued on one
stream:

  cf32, cs16, cs8    the shape above from rows of that format
  m64                64 bands x M = 64, K = 8: the same rows out, 64 frames a tile
  m4096              1 band x M = 4096, K = 8: one frame a tile, 8-byte stores
  copy_out           yardstick: a device-to-device copy of the output bytes
  torch_1band        yardstick: a torch restatement on band 0 (strided view,
                     tap multiply-sum, torch.fft.ifft * M, sign), in chunks of
                     2^14 frames; its rows are held to the kernel's within 1e-4
  demod              yardstick: BatchDemodulator.process_device_fmt (sps 4,
                     span 8) on the 4096 rows the cf32 leg produced
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pfb_bench.json"))
    ap.add_argument("--frames", type=int, default=1 << 18)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--calls", type=int, default=2, help="timed calls a leg and round")
    args = ap.parse_args()

    import numpy as np
    import torch
    import qpsk_amd as Q
    torch.cuda.init()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    frames, K = args.frames, 8
    rows_out = 4096
    shapes = {"cf32": (4, 1024), "cs16": (4, 1024), "cs8": (4, 1024), "m64": (64, 64), "m4096": (1, 4096)}
    n_in = {name: frames * (M // 2) for name, (B, M) in shapes.items()}
    total_in = 4 * n_in["cf32"]                       # the same for every shape: bands * frames * M / 2
    assert all(B * n_in[name] == total_in and B * M == rows_out for name, (B, M) in shapes.items())

    g = torch.Generator(device=dev).manual_seed(0x5159534B)
    x32 = torch.empty(2 * total_in, dtype=torch.float32, device=dev).normal_(generator=g).mul_(0.25)
    x16 = (x32 * 8192.0).round().clamp(-32767, 32767).to(torch.int16)
    x8 = (x32 * 32.0).round().clamp(-127, 127).to(torch.int8)
    y = torch.empty((rows_out, 2 * frames), dtype=torch.float32, device=dev)
    y2 = torch.empty_like(y)
    src = {"cf32": (x32, "cf32"), "cs16": (x16, "cs16"), "cs8": (x8, "cs8"), "m64": (x32, "cf32"), "m4096": (x32, "cf32")}

    handles = {}
    for name, (B, M) in shapes.items():
        pf = Q.Channeliser(B, channels=M, taps_per_branch=K, device=dev.index)
        pf.set_stream(stream.cuda_stream)
        handles[name] = pf
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
        B, M = shapes[name]
        x, fmt = src[name]
        rows = x.view(B, -1)
        pf = handles[name]

        def fn():
            emitted[name] = pf.apply_device(rows, n_in[name], y, fmt=fmt, out_cap=frames)
        return lambda: timed(fn)

    # the torch restatement, band 0 of the cf32 shape
    M, D, L = 1024, 512, 1024 * K
    p = handles["cf32"].p
    h = torch.from_numpy(Q.pfb_design(p)).to(dev)
    hrev = h.view(K, M).flip(0).flip(1).contiguous()           # hrev[k', q] = h[(M - 1 - q) + (K - 1 - k') M]
    sign = 1.0 - 2.0 * ((torch.arange(M, device=dev)[None, :] & torch.arange(2, device=dev)[:, None]) & 1).float()
    chunk = 1 << 14
    t_out = torch.empty((frames, M), dtype=torch.complex64, device=dev)

    def torch_band(first_call=False):
        # band 0's second call: its history is the first call's tail (the rows are the same every call)
        xb = torch.view_as_complex(x32.view(4, -1, 2)[0])
        hist = torch.zeros(L, dtype=torch.complex64, device=dev) if first_call else xb[-L:]
        xp = torch.cat([hist, xb])
        m0 = 0 if first_call else frames                      # parity of the absolute frame: frames is even
        for f0 in range(0, frames, chunk):
            # U[m, k', q] = x[m D - L + 1 + k' M + q] (index into the call), + L into xp
            U = torch.as_strided(xp, (chunk, K, M), (D, M, 1), storage_offset=f0 * D + 1)
            v = (U * hrev[None]).sum(1).flip(1)
            a = torch.fft.ifft(v, dim=1) * M
            par = (torch.arange(f0, f0 + chunk, device=dev) + m0) & 1
            t_out[f0: f0 + chunk] = a * sign[par]

    dm = Q.BatchDemodulator(rows_out, Q.params(FS // 8, FS // 32, ALPHA, 8, max_samples_per_call=frames))
    dm.set_stream(stream.cuda_stream)
    ms_bits = dm.max_symbols(frames)
    bits = torch.zeros((rows_out, (2 * ms_bits + 7) // 8 + 8), dtype=torch.uint8, device=dev)
    nbits = torch.zeros(rows_out, dtype=torch.int64, device=dev)

    legs = {name: leg(name) for name in shapes}
    legs["copy_out"] = lambda: timed(lambda: y2.copy_(y))
    legs["torch_1band"] = lambda: timed(torch_band)
    legs["demod"] = lambda: timed(lambda: dm.process_device_fmt(y, frames, bits, nbits, "cf32"))
    legs["cf32"]()                                   # the demodulator's rows: the channels of the noise
    rec = {"device": torch.cuda.get_device_name(dev), "frames": frames, "taps_per_branch": K, "rows_out": rows_out,
           "shapes": {k: {"bands": b, "channels": m, "tile_frames": Q.pfb_tile_frames(m)} for k, (b, m) in shapes.items()},
           "runs": []}
    for name in legs:                                # warm-up: code objects, first touches, the bands' first call
        legs[name]()
    # the restatement against the kernel: band 0, the second call onwards
    legs["cf32"]()
    torch_band()
    stream.synchronize()
    got = torch.view_as_complex(y[:M].view(M, frames, 2)).t()
    rec["torch_vs_kernel_max_abs"] = float((got - t_out).abs().max())
    assert rec["torch_vs_kernel_max_abs"] < 1e-4, rec["torch_vs_kernel_max_abs"]
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
    out_bytes = rows_out * frames * 8
    in_bytes = {"cf32": 8, "cs16": 4, "cs8": 2, "m64": 8, "m4096": 8}
    rec["gbytes_out"] = round(out_bytes / 1e9, 2)
    rec["gbytes_in"] = {k: round(total_in * b / 1e9, 2) for k, b in in_bytes.items()}
    rec["wideband_gsamples_per_s"] = {k: round(total_in / 1e9 / (rec[k + "_ms_median"] / 1e3), 3) for k in shapes}
    rec["channel_gsamples_per_s"] = {k: round(rows_out * frames / 1e9 / (rec[k + "_ms_median"] / 1e3), 3) for k in shapes}
    rec["gbytes_per_s"] = {k: round((out_bytes + total_in * in_bytes[k]) / 1e9 / (rec[k + "_ms_median"] / 1e3), 1) for k in shapes}
    rec["copy_out_gbytes_per_s"] = round(2 * out_bytes / 1e9 / (rec["copy_out_ms_median"] / 1e3), 1)
    rec["over_copy_out"] = {k: round(rec[k + "_ms_median"] / rec["copy_out_ms_median"], 3) for k in shapes}
    rec["torch_4bands_ms_estimate"] = round(4 * rec["torch_1band_ms_median"], 3)
    rec["over_torch"] = round(rec["cf32_ms_median"] / rec["torch_4bands_ms_estimate"], 4)
    rec["over_demod"] = round(rec["cf32_ms_median"] / rec["demod_ms_median"], 3)
    flops = rows_out * frames * (4 * K + 10 * 10 / 2) + 0.0     # 2 mul + 2 add a tap and part; 10 flop a butterfly, log2 M / 2 an element
    rec["cf32_tflops_unfused"] = round(flops / 1e12 / (rec["cf32_ms_median"] / 1e3), 2)
    print(json.dumps({k: v for k, v in rec.items() if k != "runs"}), flush=True)
    for hnd in list(handles.values()) + [dm]:
        hnd.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
