#!/usr/bin/env python3
"""What the polyphase synthesis bank (qpsk_sfb_apply_fmt) costs on one MI355X,
the legs alternated in one run.

Writes one JSON file (--out, default profiles/sfb_bench.json).  Every shape
takes 4096 input rows of 2^18 frames, K = 8 taps a branch: 8.6 GB in at CF32,
and 2^29 wideband samples out (4.3 GB at CF32, 2.1 GB at CS16, 1.1 GB at CS8).
The input rows are seeded noise in device memory; every handle has taken one
call before it is timed, so a timed call reads its history.  Legs, --repeats
rounds of each in turn, every one timed with device events around calls queued
on one stream:

  m1024_cf32, _cs16, _cs8    4 bands x M = 1024 into rows of that format
  m64_cf32, _cs16, _cs8      64 bands x M = 64
  m4096_cf32, _cs16, _cs8    1 band x M = 4096: one frame a transform tile
  copy_in            yardstick: a device-to-device copy of the input rows
  pfb                yardstick: the channeliser at 4 x M = 1024, K = 8 on the CF32
                     wideband rows the bank made (2^18 frames out, 4096 rows)
  torch_1band        yardstick: a torch restatement on band 0 of 4 x M = 1024
                     (sign, torch.fft.ifft * M, the 2K tap products summed over
                     shifted views), in chunks of 2^14 frames; its row is held
                     to the kernel's within 1e-4 of the row's largest sample
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sfb_bench.json"))
    ap.add_argument("--frames", type=int, default=1 << 18)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--calls", type=int, default=2, help="timed calls a leg and round")
    args = ap.parse_args()

    import torch
    import qpsk_amd as Q
    torch.cuda.init()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    frames, K = args.frames, 8
    H = 2 * K - 1
    rows_in = 4096
    shapes = {"m1024": (4, 1024), "m64": (64, 64), "m4096": (1, 4096)}
    fmts = {"cf32": (torch.float32, 1.0), "cs16": (torch.int16, 2000.0), "cs8": (torch.int8, 8.0)}
    total_out = rows_in // 2 * frames                  # bands * frames * M / 2, the same for every shape
    assert all(B * M == rows_in for B, M in shapes.values()) and frames % 2 == 0

    g = torch.Generator(device=dev).manual_seed(0x5159534B)
    x = torch.empty((rows_in, 2 * frames), dtype=torch.float32, device=dev).normal_(generator=g).mul_(0.25)
    x2 = torch.empty_like(x)
    wide = {f: torch.empty(2 * total_out, dtype=dt, device=dev) for f, (dt, _) in fmts.items()}

    handles = {}
    for name, (B, M) in shapes.items():
        sf = Q.SynthesisBank(B, channels=M, taps_per_branch=K, device=dev.index)
        sf.set_stream(stream.cuda_stream)
        handles[name] = sf
    pf = Q.Channeliser(4, channels=1024, taps_per_branch=K, device=dev.index)
    pf.set_stream(stream.cuda_stream)

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

    def leg(name, fmt):
        B, M = shapes[name]
        sf, (_, scale) = handles[name], fmts[fmt]
        rows = wide[fmt].view(B, -1)
        return lambda: timed(lambda: sf.apply_device(x, frames, rows, out_fmt=fmt, scale_out=scale))

    # the torch restatement, band 0 of 4 x M = 1024
    M, D = 1024, 512
    taps = torch.from_numpy(Q.pfb_design(Q.pfb_params(channels=M, taps_per_branch=K))).to(dev)
    gj = taps.view(2 * K, D)                                   # gj[j, r] = g[j D + r]
    c = torch.arange(M, device=dev)
    chunk = 1 << 14
    t_out = torch.empty((frames, D), dtype=torch.complex64, device=dev)

    def torch_band():
        # band 0's second call onwards: its history is the call's own tail (the rows are the same every call), and the
        # absolute frame has the call's parity (frames is even)
        s = torch.view_as_complex(x[:M].view(M, frames, 2))
        s = torch.cat([s[:, -H:], s], dim=1)
        for f0 in range(0, frames, chunk):
            z = s[:, f0: f0 + chunk + H].t()                   # [chunk + H, M], frame f0 - H + row
            par = (torch.arange(f0 - H, f0 + chunk, device=dev) & 1)[:, None]
            z = torch.where((par & c[None, :] & 1).bool(), -z, z)
            u = torch.fft.ifft(z, dim=1) * M
            acc = torch.zeros((chunk, D), dtype=torch.complex64, device=dev)
            for j in range(2 * K):
                col = (j & 1) * D
                acc += gj[j][None, :] * u[H - j: H - j + chunk, col: col + D]
            t_out[f0: f0 + chunk] = acc

    y = torch.empty((rows_in, 2 * frames), dtype=torch.float32, device=dev)
    legs = {f"{name}_{fmt}": leg(name, fmt) for name in shapes for fmt in fmts}
    legs["copy_in"] = lambda: timed(lambda: x2.copy_(x))
    legs["pfb"] = lambda: timed(lambda: pf.apply_device(wide["cf32"].view(4, -1), total_out // 4, y, out_cap=frames))
    legs["torch_1band"] = lambda: timed(torch_band)
    rec = {"device": torch.cuda.get_device_name(dev), "frames": frames, "taps_per_branch": K, "rows_in": rows_in,
           "shapes": {k: {"bands": b, "channels": m, "transform_tile_frames": Q.pfb_tile_frames(m),
                          "slab_frames": max(64, (1 << 22) // m // b)} for k, (b, m) in shapes.items()},
           "runs": []}
    for name in legs:                                # warm-up: code objects, first touches, the bands' first call
        legs[name]()
    # the restatement against the kernel: band 0, the second call onwards
    legs["m1024_cf32"]()
    torch_band()
    stream.synchronize()
    got = torch.view_as_complex(wide["cf32"].view(4, -1)[0].view(frames, D, 2))
    rec["torch_vs_kernel_max_abs"] = float((got - t_out).abs().max())
    rec["kernel_max_abs"] = float(got.abs().max())
    assert rec["torch_vs_kernel_max_abs"] < 1e-4 * rec["kernel_max_abs"], rec
    legs["m1024_cf32"]()                             # the channeliser's input again
    for rep in range(args.repeats):
        for name in legs:
            run = {"leg": name, "repeat": rep, "ms": legs[name]()}
            rec["runs"].append(run)
            print(json.dumps(run), flush=True)
    for name in legs:
        ms = [m for r in rec["runs"] if r["leg"] == name for m in r["ms"]]
        rec[name + "_ms"] = ms
        rec[name + "_ms_median"] = round(statistics.median(ms), 3)
    in_bytes = rows_in * frames * 8
    out_bytes = {"cf32": 8, "cs16": 4, "cs8": 2}
    sfb_legs = [f"{name}_{fmt}" for name in shapes for fmt in fmts]
    rec["gbytes_in"] = round(in_bytes / 1e9, 2)
    rec["gbytes_out"] = {f: round(total_out * b / 1e9, 2) for f, b in out_bytes.items()}
    rec["wideband_gsamples_per_s"] = {k: round(total_out / 1e9 / (rec[k + "_ms_median"] / 1e3), 3) for k in sfb_legs}
    rec["gbytes_per_s"] = {k: round((in_bytes + total_out * out_bytes[k.split("_")[1]]) / 1e9 / (rec[k + "_ms_median"] / 1e3), 1)
                           for k in sfb_legs}
    rec["copy_in_gbytes_per_s"] = round(2 * in_bytes / 1e9 / (rec["copy_in_ms_median"] / 1e3), 1)
    rec["over_copy_in"] = {k: round(rec[k + "_ms_median"] / rec["copy_in_ms_median"], 3) for k in sfb_legs}
    rec["over_pfb"] = round(rec["m1024_cf32_ms_median"] / rec["pfb_ms_median"], 3)
    rec["torch_4bands_ms_estimate"] = round(4 * rec["torch_1band_ms_median"], 3)
    rec["over_torch"] = round(rec["m1024_cf32_ms_median"] / rec["torch_4bands_ms_estimate"], 4)
    flops = rows_in * frames * (10 * 10 / 2) + total_out * 8 * K + 0.0   # 10 flop a butterfly, log2 M / 2 an element; 2 mul + 2 add a term
    rec["m1024_cf32_tflops_unfused"] = round(flops / 1e12 / (rec["m1024_cf32_ms_median"] / 1e3), 2)
    print(json.dumps({k: v for k, v in rec.items() if k != "runs"}), flush=True)
    for hnd in list(handles.values()) + [pf]:
        hnd.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
