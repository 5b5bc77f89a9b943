#!/usr/bin/env python3
"""A BER-versus-Es/N0 curve from thousands of independent streams on one
MI355X, with no bit leaving the device: per Es/N0 point the C3 batch (4096
streams x 2^20 samples, sps 4, 129 taps) is synthesised with that much AWGN
(qpsk_synth_generate), demodulated from a fresh state, and its bit errors are
counted against the transmitted bits where both lie (qpsk_ber_count_device).
Only the 64-byte rows come back.

Writes one JSON file (--out, default profiles/ber_curve.json): per point the
ber_summary over all streams (bench.py's "BER after lock" figures), the
streams that located and the milliseconds of each stage by device events.  The
values are recorded as measured; nothing here asserts them.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "qpsk-modulator-demodulator_amd"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FS = 10_000_000
ALPHA = 0.4000000059604645
C3 = dict(streams=4096, sps=4, span=32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ber_curve.json"))
    ap.add_argument("--streams", type=int, default=C3["streams"])
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--esn0-db", default="0:12:1", help="first:last:step in dB (inclusive)")
    args = ap.parse_args()
    first, last, step = (float(v) for v in args.esn0_db.split(":"))
    points = [first + k * step for k in range(int(round((last - first) / step)) + 1)]

    import torch
    import qpsk_amd as Q
    torch.cuda.init()
    dev = torch.device("cuda", 0)
    S, n, sps, span = args.streams, args.samples, C3["sps"], C3["span"]
    rs = FS // sps
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    d = Q.BatchDemodulator(S, Q.params(FS, rs, ALPHA, span, device=dev.index, max_samples_per_call=n))
    d.set_stream(stream.cuda_stream)
    fresh = d.get_state()
    ms = d.max_symbols(n)
    bits = torch.zeros((S, ((2 * ms + 7) // 8 + 127) // 64 * 64), dtype=torch.uint8, device=dev)
    nbits = torch.zeros(S, dtype=torch.int64, device=dev)
    out_dev = torch.zeros((S, 64), dtype=torch.uint8, device=dev)
    iq = tx = n_ref = None
    rec = {"device": torch.cuda.get_device_name(dev), "streams": S, "samples": n, "sps": sps, "taps": sps * span + 1,
           "params": dict(skip_bits=8000, window=2048, key_bits=64, search=512), "points": []}
    for esn0 in points:
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        d.set_state(fresh)
        ev[0].record(stream)
        iq, tx = Q.synth_generate(S, n, FS, rs, rrc_alpha=ALPHA, rrc_span=span, seed=0x5159534B, lo_ppm=1.0,
                                  esn0_db=esn0, device=dev.index, stream=stream.cuda_stream, out=iq, tx_bits=tx)
        if n_ref is None:
            n_ref = torch.full((S,), 8 * tx.shape[1], dtype=torch.int64, device=dev)
        ev[1].record(stream)
        d.process_device(iq, n, bits, nbits)
        ev[2].record(stream)
        Q.ber_count_device(bits, nbits, tx, n_ref, out_dev=out_dev, hip_stream=stream.cuda_stream)
        ev[3].record(stream)
        ev[3].synchronize()
        rows = out_dev.cpu().numpy().view(Q.BER_ROW_DTYPE).reshape(-1)
        point = dict(esn0_db=esn0, **Q.ber_summary(rows), streams_located=int(rows["located"].sum()),
                     streams_counted=int((rows["bits"] > 0).sum()), windows=int(rows["windows"].sum()),
                     synth_ms=round(ev[0].elapsed_time(ev[1]), 2), demod_ms=round(ev[1].elapsed_time(ev[2]), 2),
                     ber_count_ms=round(ev[2].elapsed_time(ev[3]), 3))
        rec["points"].append(point)
        print(json.dumps(point), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    d.close()


if __name__ == "__main__":
    main()
