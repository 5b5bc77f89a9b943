"""GPU parity at the BASELINE.json workloads, at full size.

C3 (4096 x 2^20, sps 4, 129 taps), the C4 shard (4096 x 2^20, sps 8, 65 taps)
and C5 (8192 x 2^20, +-5 kHz CFO + multipath + AWGN, FLL on) run on the HIP
path exactly as bench.py synthesises them (same generator, seeds and LO
pair), through QPSKDeModulator.DeModulate semantics (QPSKDeModulator.cs:345-425):
seven consecutive calls on the same buffer, as the bench's timed region
feeds it.  Each call's bit rows of the first 8 and the last 8 streams (the
last rows start 32 GiB into the input at C3 and the C4 shard and 64 GiB into
it at C5; the assert below checks > 16 GiB for all three), plus the 4 streams whose Costas phase
grew the most (QPSK false lock: |freq| near a multiple of pi/2, theta growing
every symbol past the single +-2pi wrap of CostasLoopQpsk.cs:90-91, so the
large-|theta| reduction paths run), are compared with the CPU oracle calling
the real glibc trig (what .NET's Math.Sin/Cos and MathF.Sin/Cos reach on
Linux), one oracle demodulator per stream fed the same seven calls.

Bar: bits identical on every call; rotated symbols of the first (fresh
state) and the seventh (steady state) call bit-identical with the Costas NCO
on glibc's own sin/cos (costas_trig = 1), within SYM_TOL with the default
portable table sincos (costas_trig = 0, within 1 ulp of glibc).
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import common as K
import oracle as O
import qpsk_amd as Q
from gpu_harness import SYM_TOL, dev

pytestmark = pytest.mark.gpu

N = 1 << 20
CALLS = 7
SEED = 0x5159534B            # bench.py synth_kw

CASES = {
    # key: streams, sps, rrc span, impaired channel + FLL, pipelined calls
    "c3": dict(S=4096, sps=4, span=32, impaired=False, pipelined=True),
    "c4_shard": dict(S=4096, sps=8, span=8, impaired=False, pipelined=False),
    "c5": dict(S=8192, sps=8, span=8, impaired=True, pipelined=False),
}


@pytest.fixture(scope="module", autouse=True)
def _gpu(dev):
    yield
    dev.cuda.empty_cache()


def _rows(t, idx):
    return np.concatenate([t[i: i + 1].cpu().numpy() for i in idx])


def _oracle_stream(row, sps, span, fll):
    """CALLS DeModulate calls of one oracle instance on the same row."""
    d = K.oracle_for(sps, span, trig=O.TRIG_LIBM, enable_fll=fll)
    return [d.demodulate_ex(row) for _ in range(CALLS)]


@pytest.mark.parametrize("key,trig", [(k, 0) for k in CASES] + [("c3", 1), ("c5", 1)])
def test_baseline_workload_seven_calls_vs_libm_oracle(key, trig):
    import torch
    c = CASES[key]
    S, sps, span, imp = c["S"], c["sps"], c["span"], c["impaired"]
    dev = torch.device("cuda", 0)
    iq, _tx = Q.synth_generate(S, N, K.FS, K.FS // sps, rrc_alpha=K.ALPHA, rrc_span=span, seed=SEED,
                               lo_ppm=1.0, cfo_hz=5000.0 if imp else 0.0, multipath=imp,
                               esn0_db=20.0 if imp else None)
    del _tx
    assert iq.stride(0) * 4 * (S - 1) > (16 << 30)   # last rows ~32 GiB (C3, C4) / ~64 GiB (C5) in
    b = Q.BatchDemodulator(S, Q.params(K.FS, K.FS // sps, K.ALPHA, span, enable_fll=imp,
                                       max_samples_per_call=N, costas_trig=trig))
    ms = b.max_symbols(N)
    stream = torch.cuda.Stream(dev)
    b.set_stream(stream.cuda_stream)
    outs = []
    for k in range(CALLS):
        bits = torch.zeros((S, (2 * ms + 7) // 8 + 8), dtype=torch.uint8, device=dev)
        nb = torch.zeros(S, dtype=torch.int64, device=dev)
        sy = ns = None
        if k in (0, CALLS - 1):
            sy = torch.zeros((S, 2 * ms), dtype=torch.float32, device=dev)
            ns = torch.zeros(S, dtype=torch.int64, device=dev)
        outs.append((bits, nb, sy, ns))
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(stream):
        for bits, nb, sy, ns in outs:
            if c["pipelined"]:
                b.process_device_async(iq, N, bits, nb, syms_dev=sy, n_syms_dev=ns)
            else:
                b.process_device(iq, N, bits, nb, syms_dev=sy, n_syms_dev=ns)
        if c["pipelined"]:
            b.pipeline_wait()
    stream.synchronize()
    assert b.status() == 0
    theta = b.stream_states()["theta"]
    idx = list(range(8)) + list(range(S - 8, S))
    idx += [int(i) for i in np.argsort(-np.abs(theta)) if int(i) not in idx][:4]
    host = _rows(iq, idx)
    got = []
    for bits, nb, sy, ns in outs:
        got.append((_rows(bits, idx), _rows(nb, idx), None if sy is None else _rows(sy, idx),
                    None if ns is None else _rows(ns, idx)))
    b.close()
    del outs, iq
    torch.cuda.empty_cache()

    with ThreadPoolExecutor(max_workers=len(idx)) as ex:
        ref = list(ex.map(lambda r: _oracle_stream(r, sps, span, imp), list(host)))
    exact = trig == 1
    for j, s in enumerate(idx):
        for k in range(CALLS):
            gb, gnb, gsy, gns = (x[j] if x is not None else None for x in got[k])
            rb, rsy, _ = ref[j][k]
            assert Q.unpack_bits(gb, int(gnb)) == rb, f"{key} stream {s} (|theta| {abs(theta[s]):.3g}) call {k}: bits"
            if gsy is not None:
                g = gsy[: 2 * int(gns)]
                assert g.shape == rsy.shape, f"{key} stream {s} call {k}: symbol count"
                if exact:
                    assert K.bitwise_equal(g, rsy), f"{key} stream {s} call {k}: symbols (bitwise)"
                else:
                    assert np.max(np.abs(g - rsy), initial=0) <= SYM_TOL, f"{key} stream {s} call {k}"


def _pipelined_rows(S, n, calls, sps, span, seed, idx, stats=None, **kw):
    """`calls` consecutive pipelined calls of n samples on a GPU-synthesised
    batch; returns the host input rows idx and per call (bits, n_bits) of idx
    (stats: a dict that receives the handle's gate timeouts)."""
    import torch
    dev = torch.device("cuda", 0)
    iq, _ = Q.synth_generate(S, n * calls, K.FS, K.FS // sps, rrc_alpha=K.ALPHA, rrc_span=span, seed=seed,
                             lo_ppm=1.0)
    b = Q.BatchDemodulator(S, Q.params(K.FS, K.FS // sps, K.ALPHA, span, max_samples_per_call=n, **kw))
    ms = b.max_symbols(n)
    stream = torch.cuda.Stream(dev)
    b.set_stream(stream.cuda_stream)
    outs = []
    torch.cuda.synchronize(dev)
    # the input copies and the zeroed output rows on the handle's stream: made
    # on torch's default stream they would race the handle's kernels (a
    # test-harness race, seen once as a gate-test mismatch between two runs)
    with torch.cuda.stream(stream):
        for k in range(calls):
            x = iq[:, 2 * n * k: 2 * n * (k + 1)].contiguous()
            bits = torch.zeros((S, (2 * ms + 7) // 8 + 8), dtype=torch.uint8, device=dev)
            nb = torch.zeros(S, dtype=torch.int64, device=dev)
            b.process_device_async(x, n, bits, nb)
            outs.append((x, bits, nb))
    b.pipeline_wait()
    torch.cuda.synchronize(dev)
    host = _rows(iq, idx)
    got = [(_rows(bits, idx), _rows(nb, idx)) for _, bits, nb in outs]
    if stats is not None:
        stats["gate_timeouts"] = b.gate_timeouts()
    b.close()
    return host, got


def _oracle_calls(row, n, calls, sps, span):
    d = K.oracle_for(sps, span)
    return [d.demodulate_ex(row[2 * n * k: 2 * n * (k + 1)])[0] for k in range(calls)]


def test_pipelined_loop_grid_larger_than_the_chip():
    """12000 streams at sps 4: 375 loop workgroups, more than the 256 CUs hold
    at once (one 125 KB workgroup each), so the residency gate the next FIR
    waits on is the first dispatch wave, min(grid, CUs), not the whole grid;
    the pipelined calls finish and match the oracle."""
    S, n, calls = 12000, 4096, 3
    idx = [0, 1, 5999, S - 2, S - 1]
    host, got = _pipelined_rows(S, n, calls, 4, 32, 0x47415445, idx)
    for j, s in enumerate(idx):
        ref = _oracle_calls(host[j], n, calls, 4, 32)
        for k in range(calls):
            gb, gnb = got[k][0][j], got[k][1][j]
            assert Q.unpack_bits(gb, int(gnb)) == ref[k], f"stream {s} call {k}"


def test_pipelined_results_do_not_depend_on_the_gate(monkeypatch):
    """QPSK_PIPELINE_GATE=0 (what a counter-collecting profiler gets) changes
    only the dispatch order, not one bit."""
    S, n, calls = 300, 8192, 4
    idx = list(range(S))
    _, with_gate = _pipelined_rows(S, n, calls, 8, 8, 0x51, idx)
    monkeypatch.setenv("QPSK_PIPELINE_GATE", "0")
    _, without = _pipelined_rows(S, n, calls, 8, 8, 0x51, idx)
    for k in range(calls):
        assert np.array_equal(with_gate[k][1], without[k][1])
        for s in range(S):
            nb = int(with_gate[k][1][s])
            assert np.array_equal(with_gate[k][0][s][: (nb + 7) // 8], without[k][0][s][: (nb + 7) // 8])


def test_gate_that_never_opens_times_out_bit_exact(monkeypatch):
    """The residency gate's wait is bounded: with the loop kernel's residency
    count suppressed (QPSK_GATE_NO_PUBLISH=1) every wait runs to its cap
    (QPSK_GATE_TIMEOUT_MS) and the matched filter goes ahead; the calls still
    finish, each wait is counted, and the bits are the gated run's."""
    import time
    S, n, calls = 300, 8192, 4
    idx = list(range(S))
    st = {}
    _, with_gate = _pipelined_rows(S, n, calls, 8, 8, 0x52, idx, stats=st)
    assert st["gate_timeouts"] == 0
    monkeypatch.setenv("QPSK_PIPELINE_GATE", "1")
    monkeypatch.setenv("QPSK_GATE_NO_PUBLISH", "1")
    monkeypatch.setenv("QPSK_GATE_TIMEOUT_MS", "200")
    t0 = time.perf_counter()
    _, stuck = _pipelined_rows(S, n, calls, 8, 8, 0x52, idx, stats=st)
    dt = time.perf_counter() - t0
    assert st["gate_timeouts"] == calls - 1      # every call after the first waited
    assert dt < 30.0
    for k in range(calls):
        assert np.array_equal(with_gate[k][1], stuck[k][1])
        for s in range(S):
            nb = int(with_gate[k][1][s])
            assert np.array_equal(with_gate[k][0][s][: (nb + 7) // 8], stuck[k][0][s][: (nb + 7) // 8])


def test_two_pipelined_handles_interleaved():
    """Two handles on one GPU, their pipelined calls interleaved: each has its
    own residency counter and gate, and each matches the oracle."""
    import torch
    dev = torch.device("cuda", 0)
    S, n, calls = 64, 8192, 3
    iq, _ = Q.synth_generate(S, n * calls, K.FS, K.FS // 8, rrc_alpha=K.ALPHA, rrc_span=8, seed=77, lo_ppm=1.0)
    hs = [Q.BatchDemodulator(S, Q.params(K.FS, K.FS // 8, K.ALPHA, 8, max_samples_per_call=n)) for _ in range(2)]
    ms = hs[0].max_symbols(n)
    outs = [[], []]
    for k in range(calls):
        x = iq[:, 2 * n * k: 2 * n * (k + 1)].contiguous()
        for h, o in zip(hs, outs):
            bits = torch.zeros((S, (2 * ms + 7) // 8 + 8), dtype=torch.uint8, device=dev)
            nb = torch.zeros(S, dtype=torch.int64, device=dev)
            h.process_device_async(x, n, bits, nb)
            o.append((x, bits, nb))
    for h in hs:
        h.pipeline_wait()
    torch.cuda.synchronize(dev)
    host = iq[:4].cpu().numpy()
    for s in range(4):
        ref = _oracle_calls(host[s], n, calls, 8, 8)
        for o in outs:
            for k in range(calls):
                _, bits, nb = o[k]
                assert Q.unpack_bits(bits[s].cpu().numpy(), int(nb[s])) == ref[k], (s, k)
    for h in hs:
        h.close()
