#!/usr/bin/env python3
"""Host time of one call on one MI355X, where the host is all there is to time.

--calls (default 1000) back-to-back device-memory calls of 64 samples x 8
streams, straight through the C ABI (no Python wrapper in the loop), timed on
the host around one final wait (and up to the last call's return: the time the
host spent issuing them), --repeats times:

  sync       qpsk_demod_process, QPSK_MEM_DEVICE, on the handle's own stream
  pipelined  qpsk_demod_process_async, then qpsk_demod_pipeline_wait

Prints one JSON line: the library, microseconds per call of every repeat
([issued, waited for]) and the medians of each leg.  A library of another revision goes in through
QPSK_DEMOD_LIB, as in tools/ab_bench.sh; alternate the runs.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qpsk-modulator-demodulator_amd"))

FS = 10_000_000
ALPHA = 0.4000000059604645


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--samples", type=int, default=64)
    a = ap.parse_args()
    import torch
    torch.cuda.init()   # torch's HIP runtime first, then the library's
    import qpsk_amd as Q
    dev = torch.device("cuda", 0)
    S, n, sps, span = a.streams, a.samples, 8, 8
    x, _ = Q.synth_generate(S, n, FS, FS // sps, rrc_alpha=ALPHA, rrc_span=span, seed=0x5159534B, lo_ppm=1.0,
                            device=dev.index)
    d = Q.BatchDemodulator(S, Q.params(FS, FS // sps, ALPHA, span, device=dev.index, max_samples_per_call=n))
    bits = torch.zeros((S, 64), dtype=torch.uint8, device=dev)
    nb = torch.zeros(S, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    L, h = Q.lib(), d._h
    xp, stride, bp, bstride, nbp = x.data_ptr(), x.shape[1], bits.data_ptr(), bits.shape[1], nb.data_ptr()

    def sync_call():
        return L.qpsk_demod_process(h, Q.MODE_DEMODULATE, xp, stride, n, None, Q.MEM_DEVICE, bp, bstride, nbp,
                                    None, 0, None)

    def async_call():
        return L.qpsk_demod_process_async(h, Q.MODE_DEMODULATE, xp, stride, n, None, bp, bstride, nbp, None, 0, None)

    def leg(call):
        for _ in range(200):   # the lazily made buffers, streams and events exist after these
            call()
        L.qpsk_demod_pipeline_wait(h, None)
        torch.cuda.synchronize(dev)
        us = []
        for _ in range(a.repeats):
            bad = 0
            t0 = time.perf_counter()
            for _ in range(a.calls):
                bad |= call()
            t1 = time.perf_counter()
            L.qpsk_demod_pipeline_wait(h, None)
            torch.cuda.synchronize(dev)
            t2 = time.perf_counter()
            us.append([round((t - t0) * 1e6 / a.calls, 3) for t in (t1, t2)])
            if bad:
                raise RuntimeError(f"a call failed (statuses or-ed: {bad})")
        return us

    out = {"lib": os.path.basename(os.environ.get("QPSK_DEMOD_LIB", "in-tree")), "calls": a.calls, "streams": S,
           "samples": n}
    for name, call in (("sync", sync_call), ("pipelined", async_call)):
        us = leg(call)
        out[name + "_us_per_call"] = us
        out[name + "_issue_median_us"] = statistics.median(u[0] for u in us)
        out[name + "_median_us"] = statistics.median(u[1] for u in us)
    out["gate_timeouts"] = d.gate_timeouts()
    d.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
