#!/usr/bin/env python
"""tools/framer_bench.py -- the device TSC search + DeModulateBytes framer on
the bit rows of one DeModulate call of a BASELINE config (C2 or C3), timed
with HIP events over `reps` pushes, with a checksum of every payload so two
library builds (QPSK_DEMOD_LIB) can be compared for identical output.

  python tools/framer_bench.py [--config c2|c3] [--reps 10] [--markers present|absent]

--markers absent runs the same rows with a 13-byte start marker that does not
occur in them: the start hunt scans every chunk of every row and the
keep-carry path runs, where the default's 1-byte markers end both searches in
their first chunk.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qpsk-modulator-demodulator_amd"))
sys.path.insert(0, ROOT)
sys.argv, _argv = sys.argv[:1], sys.argv
import bench  # noqa: E402
sys.argv = _argv


# the synthetic rows are random bits: 104 given bits sit at one position with
# probability 2^-104, and "frames_per_call": 0.0 in the result line confirms it
ABSENT_START = b"MESSAGE_START"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=["c2", "c3", "c4"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--markers", default="present", choices=["present", "absent"])
    args = ap.parse_args()
    import numpy as np
    import torch
    import qpsk_amd as Q
    cfg = bench.CONFIGS[args.config]
    S, n = cfg["streams"], 1 << 20
    rs = bench.FS // cfg["sps"]
    dev = torch.device("cuda", 0)
    iq, _ = Q.synth_generate(S, n, bench.FS, rs, rrc_alpha=bench.ALPHA, rrc_span=cfg["span"], seed=0x5159534B,
                             lo_ppm=1.0)
    d = Q.BatchDemodulator(S, Q.params(bench.FS, rs, bench.ALPHA, cfg["span"], max_samples_per_call=n))
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    d.set_stream(stream.cuda_stream)
    ms = d.max_symbols(n)
    bits = torch.zeros((S, ((2 * ms + 7) // 8 + 127) // 64 * 64), dtype=torch.uint8, device=dev)
    nbits = torch.zeros(S, dtype=torch.int64, device=dev)
    d.process_device(iq, n, bits, nbits)
    stream.synchronize()
    del iq
    start = b"\x02" if args.markers == "present" else ABSENT_START
    fr = Q.DeviceFramer(S, start, b"\x03", ring_capacity=1 << 16)
    fr.set_stream(stream.cuda_stream)
    offs = torch.zeros(S, dtype=torch.int64, device=dev)
    pay = torch.zeros((S, 256), dtype=torch.uint8, device=dev)
    npay = torch.zeros(S, dtype=torch.int64, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    t_tsc, t_push, frames, digest = [], [], 0, 0
    for r in range(args.reps + 1):
        ev[0].record(stream)
        Q.tsc_find_device(bits, nbits, bench.TSC_BITS, offs, stream.cuda_stream)
        ev[1].record(stream)
        fr.push(bits, nbits, pay, npay, None)
        ev[2].record(stream)
        stream.synchronize()
        np_ = npay.cpu().numpy()
        pb = pay.cpu().numpy()
        h = 0
        for s in range(S):
            k = int(min(np_[s], 256))
            h = (h * 1000003 + int(np_[s]) * 7919 + int(pb[s, :k].astype(np.int64).sum())) % (1 << 61)
        digest = (digest * 31 + h) % (1 << 61)
        if r:
            t_tsc.append(ev[0].elapsed_time(ev[1]))
            t_push.append(ev[1].elapsed_time(ev[2]))
            frames += int((npay > 0).sum().item())
    inf, cnt, car = fr.status()
    state = int(np.asarray(inf).sum()) * 1000003 + int(np.asarray(cnt).sum()) * 31 + int(np.asarray(car).sum())
    print(json.dumps({"lib": os.path.basename(os.environ.get("QPSK_DEMOD_LIB", "in-tree")), "config": args.config,
                      "markers": args.markers, "streams": S, "tsc_ms": round(float(np.median(t_tsc)), 4),
                      "framer_ms": round(float(np.median(t_push)), 4),
                      "framer_ms_all": [round(x, 4) for x in t_push],
                      "frames_per_call": frames / args.reps,
                      "frames_per_s": round(frames / (sum(t_push) * 1e-3), 1),
                      "offsets": int((offs >= 0).sum().item()), "digest": digest, "state": state}))
    torch.cuda.set_stream(torch.cuda.default_stream(dev))


if __name__ == "__main__":
    main()
