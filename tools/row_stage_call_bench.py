#!/usr/bin/env python3
"""What a small device call costs the host on the three test-bench stages
(channel, path, channeliser): the handle bound to a torch stream, 10 warm-up
calls, then 7 repeats of 200 device calls of 64 rows x 4096 CF32 samples (the
channeliser: 64 bands, M = 64, K = 8) under a host clock that ends in a
synchronise.  Prints one JSON line: per stage the [issue, total] microseconds a
call of every repeat (issue: until the last call returned; total: until the
stream was idle) and their medians.  The library is QPSK_DEMOD_LIB's (an A/B
build of another revision) or the tree's; profiles/row_stage_ab.txt alternates
the two run by run."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qpsk-modulator-demodulator_amd"))

import numpy as np
import torch

torch.cuda.init()
import qpsk_amd as Q  # noqa: E402

S, N, CALLS, REPEATS = 64, 4096, 200, 7


def timed(call, st):
    for _ in range(10):
        call()
    st.synchronize()
    runs = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        for _ in range(CALLS):
            call()
        t1 = time.perf_counter()
        st.synchronize()
        t2 = time.perf_counter()
        runs.append([round((t1 - t0) / CALLS * 1e6, 3), round((t2 - t0) / CALLS * 1e6, 3)])
    return runs


def main():
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.standard_normal((S, 2 * N)).astype(np.float32)).cuda()
    st = torch.cuda.Stream()
    rec = {"lib": os.path.basename(os.environ.get("QPSK_DEMOD_LIB", "in-tree")), "rows": S, "samples": N, "calls": CALLS}
    with torch.cuda.stream(st):
        ch = Q.Channel(S, sample_rate=1e6)
        ch.set_stream(st.cuda_stream)
        rows = x.clone()
        rec["channel"] = timed(lambda: ch.apply_device(rows, N), st)
        ch.close()

        pa = Q.Path(S, clock_ppm=20.0, multipath=1)
        pa.set_stream(st.cuda_stream)
        cap = pa.out_bound(N)
        o = torch.zeros((S, 2 * cap), dtype=torch.float32, device="cuda")
        rec["path"] = timed(lambda: pa.apply_device(x, N, o), st)
        pa.close()

        pf = Q.Channeliser(S)
        pf.set_stream(st.cuda_stream)
        cap = pf.out_bound(N)
        o = torch.zeros((pf.n_rows, 2 * cap), dtype=torch.float32, device="cuda")
        rec["pfb"] = timed(lambda: pf.apply_device(x, N, o), st)
        pf.close()
    for k in ("channel", "path", "pfb"):
        rec[k + "_issue_median_us"] = statistics.median(r[0] for r in rec[k])
        rec[k + "_median_us"] = statistics.median(r[1] for r in rec[k])
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
