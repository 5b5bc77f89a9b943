"""Integer input, bit for bit: CS16 (interleaved int16 I,Q), CS8 (int8 I,Q)
and CU8 (uint8 I,Q, zero at 128).  The cases the formats share, each written
once with the format as an argument; tests/test_gpu_cs16.py and
tests/test_gpu_int8.py name the cases each format runs and keep the tests
that only one of them has.  No test file: nothing here is collected.

A sample's value is SoapySDR's: float32(x) * scale, for CU8 float32(x - 128) *
scale.  The integer is exact in float and the multiply is one IEEE rounding,
which numpy reproduces (gpu_harness.widened).  So the reference of every check
here is the CPU oracle fed those widened floats, at tolerance 0: matched-filter
rows (qpsk_demod_last_mf against O.oracle_fir), bits and rotated symbols
(against OracleDemod).

Inputs: K.batch_signals rows quantised at half of full scale, and rows of
uniform random integers over the format's whole range with its extremes, 0
and +-1 placed at their head (gpu_harness.FORMATS holds the figures).

Stagings of the tile kernel.  One 16-byte load holds 4 CS16 samples or 8 CS8 /
CU8 samples.  Rows that are 16-byte aligned with a stride of a multiple of
that many samples take it.  Host-memory calls stage rows pitched to a whole
load, so they take it whatever max_samples_per_call is.  Device rows aligned
to one sample only (4 bytes for CS16, 2 bytes for 8-bit), or with another
stride, take one load per sample; 8-bit rows that are 8-byte aligned take
8-byte loads of 4 samples for T = 13 and 21, where T - 1 = 4 mod 8.
test_matched_filter_rows_bitwise (stage_case) therefore runs its call sequence four ways
per tap count: host calls at max_samples_per_call 4098 and 4097, and device
calls in the "vector" and the "scalar" layout.

Call sequences.  Every residue of a row's length modulo the load must end a
row.  ragged_calls (1, T-2, T-1, T, 2047, 2048, 2049, 4097 samples) covers the
four residues of CS16; for the eight of the 8-bit formats it gives 0, 1 and 7
and calls_for adds calls of 2050 ... 2054 samples for 2 ... 6
(tests/test_int8_call_sequence.py).

Entry points.  CS16 goes through process_cs16, process_device_cs16,
process_device_async_cs16, set_cs16_scale, cs16_scale and HostRing(fmt="cs16");
CS8 and CU8 through the format-tagged ones (process_fmt ..., set_input_scale,
HostRing.create_fmt).  The runners take that family from FORMATS.
"""
import contextlib
import functools

import numpy as np

import common as K
import oracle as O
import qpsk_amd as Q
from gpu_harness import (FORMATS, TILE, as_fmt, assert_rows, assert_same, call_rows, calls_for, decoded, device_calls,
                         entry, fir_ref, host_call, host_calls, lengths_of, make, oracle_run, ragged_calls, random_rows,
                         rrc, set_scale, signal_q, split_calls, widened)

def oracle_chain(w, calls, sps, span, **okw):
    return oracle_run(w, calls, K.FS // sps, span, **okw)


# ---------------------------------------------------------------------------
# matched-filter rows
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stage_inputs(sps, span, fmt, lanes=8, seed=0, scale=None):
    """(rows, calls, per-stream reference rows): 6 rows, 4 of random integers
    and 2 of quantised signal, over the format's call sequence (module docstring)."""
    T = sps * span + 1
    calls = calls_for(T) if FORMATS[fmt].per_load == 8 else ragged_calls(T)
    total = sum(c[0] for c in calls)
    assert all(sum(c[s] for c in calls) == total for s in range(6))
    x = random_rows(6, total, seed + T, fmt)
    sig = signal_q(sps, span, 2, fmt, n_bits=2 * (total // sps + 2 * span + 8), seed0=40)
    assert sig.shape[1] >= 2 * total
    x[4:] = sig[:, : 2 * total]
    w = widened(x, fmt, scale)
    refs = [fir_ref(rrc(sps, span), w[s], lanes) for s in range(6)]
    x.setflags(write=False)
    return x, calls, refs


def stage_case(sps, span, fmt, how, lanes=8, seed=0, scale=None):
    x, calls, refs = stage_inputs(sps, span, fmt, lanes, seed, scale)
    b = make(6, sps, span, 4097 if how == "host-4097" else 4098, vector_lanes=lanes)
    if scale is not None:
        set_scale(b, fmt, scale)
    if how.startswith("host"):
        _, mfs = host_calls(b, x, calls, fmt)
    else:
        _, mfs = device_calls(b, x, calls, fmt, layout=how.split("-")[1])
    assert b.status() == 0
    b.close()
    assert_rows(mfs, calls, refs)


# ---------------------------------------------------------------------------
# whole chain
# ---------------------------------------------------------------------------


def chain_host_device_pipelined_chunked(fmt, sps, span, S):
    """Bits and symbols of ragged host calls, device calls (both layouts),
    pipelined calls and one chunked call (max_samples_per_call below the call
    length: 3 chunks, host and device memory)."""
    x = signal_q(sps, span, S, fmt)
    n = x.shape[1] // 2
    w = widened(x, fmt)
    calls = split_calls(S, n, 3, seed=sps + S)
    nmax = max(max(c) for c in calls)
    want = oracle_chain(w, calls, sps, span)
    runs = [("host", host_calls), ("device vector", functools.partial(device_calls, layout="vector")),
            ("device scalar", functools.partial(device_calls, layout="scalar")),
            ("pipelined", functools.partial(device_calls, pipelined=True))]
    for what, run in runs:
        b = make(S, sps, span, nmax + 5)
        got, _ = run(b, x, calls, fmt)
        assert b.status() == 0
        if what == "pipelined":
            assert b.pipeline_depth() == 2
        b.close()
        assert_same(got, want, what=what)

    one = [[n] * S]
    want1 = oracle_chain(w, one, sps, span)
    for run in (host_calls, device_calls, functools.partial(device_calls, layout="scalar", pipelined=True)):
        b = make(S, sps, span, n // 3 + 1)   # 3 chunks
        got = run(b, x, one, fmt)[0]
        assert b.status() == 0
        b.close()
        assert_same(got, want1, what="chunked")


def chain_costas_trig_and_constellation_mode(fmt, trig):
    """costas_trig 0 and 1 (the oracle's portable / libm trig), with
    deModulateConstellation calls between the DeModulate ones."""
    sps, span, S = 8, 8, 5
    x = signal_q(sps, span, S, fmt, seed0=20 + trig)
    n = x.shape[1] // 2
    calls = split_calls(S, n, 3, seed=90 + trig)
    mode = [0, 1, 0, 1]
    want = oracle_chain(widened(x, fmt), calls, sps, span, mode=mode, trig=O.TRIG_LIBM if trig else O.TRIG_PORTABLE)
    nmax = max(max(c) for c in calls)
    for run in (host_calls, device_calls, functools.partial(device_calls, pipelined=True)):
        b = make(S, sps, span, nmax, costas_trig=trig)
        got = run(b, x, calls, fmt, mode=mode)[0]
        assert b.status() == 0
        b.close()
        assert_same(got, want)


# ---------------------------------------------------------------------------
# equivalence to the float path (no oracle)
# ---------------------------------------------------------------------------
def equals_the_float_path_fed_the_widened_floats(fmt, sps, span):
    S = 5
    x = np.concatenate([signal_q(sps, span, S, fmt, seed0=60), random_rows(S, 1500, 61, fmt)], axis=1)
    n = x.shape[1] // 2
    calls = split_calls(S, n, 4, seed=62)
    nmax = max(max(c) for c in calls)
    a, f = make(S, sps, span, nmax + 2), make(S, sps, span, nmax + 2)
    got_int, mf_int = host_calls(a, x, calls, fmt)
    got32, mf32 = host_calls(f, widened(x, fmt), calls, "cf32")
    assert a.status() == 0 and f.status() == 0
    assert a.get_state() == f.get_state(), "state blobs (float either way)"
    a.close()
    f.close()
    assert_same(got_int, got32)
    for ci, (mi, m32) in enumerate(zip(mf_int, mf32)):
        assert K.bitwise_equal(mi, m32), f"call {ci}: matched-filter rows"


# ---------------------------------------------------------------------------
# several formats on one handle
# ---------------------------------------------------------------------------
# rows' format -> (per-call formats, per-call lengths of n samples, max_samples_per_call from n and
# the longest call, entry-point family)
MIXED = {
    "cs16": (["cf32", "cs16", "cf32"], lambda n: [n // 3, n // 4 + 1, n - n // 3 - n // 4 - 1],
             lambda n, longest: n, "cs16"),
    "cs8": (["cf32", "cs8", "cs16", "cu8", "cs8"],
            lambda n: [n // 5, n // 5 + 1, n // 5 + 3, n // 5, n - 4 * (n // 5) - 4],
            lambda n, longest: longest, "fmt"),
}


def mixed_format_calls_on_one_handle(base):
    """The same samples call by call in several formats (the CS8 rows as
    floats, int8, int16 x 256 at the CS16 default scale and uint8; the CS16
    rows as floats and int16), against one oracle run over the widened floats."""
    sps, span, S = 4, 32, 5
    fmts, lens_of, capacity, family = MIXED[base]
    v = signal_q(sps, span, S, base, seed0=70)
    n = v.shape[1] // 2
    w = widened(v, base)
    calls = [[k] * S for k in lens_of(n)]
    b = make(S, sps, span, capacity(n, max(max(c) for c in calls)))
    pos = np.zeros(S, np.int64)
    got, mfs = [], []
    for lens, fmt in zip(calls, fmts):
        rows = call_rows(v, lens, pos)
        rows = rows if fmt == base else widened(rows, base) if fmt == "cf32" else as_fmt(rows, fmt)
        assert rows.dtype == FORMATS[fmt].np_dtype
        got.append(host_call(b, rows, lengths_of(lens), fmt=fmt, family=family))
        mfs.append(b.last_mf(lens[0]).copy())
        pos += np.array(lens)
    assert b.status() == 0
    b.close()
    assert_same(got, oracle_chain(w, calls, sps, span))
    assert_rows(mfs, calls, [fir_ref(rrc(sps, span), w[s]) for s in range(S)])


# ---------------------------------------------------------------------------
# non-finite history
# ---------------------------------------------------------------------------
def nan_and_inf_in_the_history_of_an_integer_call(sps, span, fmt):
    """A float call whose last T-1 samples hold a NaN and an Inf, then an integer
    call: its first outputs have them in their windows, so the tile kernel's
    recompute path reads the float history and the integer row."""
    S, T = 3, sps * span + 1
    n1, n2 = 700, TILE + 300
    f = np.random.default_rng(80).standard_normal((S, 2 * n1)).astype(np.float32)
    f[0, 2 * (n1 - 5)] = np.nan                  # I of stream 0, 5 samples from the end
    f[1, 2 * (n1 - (T - 1)) + 1] = np.inf        # Q of stream 1, the oldest history sample
    f[2, 2 * (n1 - 1)] = -np.inf                 # stream 2: the newest
    f[2, 2 * (n1 - 2) + 1] = np.nan
    x = random_rows(S, n2, 81, fmt)
    b = make(S, sps, span, n2)
    with contextlib.suppress(Q.QPSKError):       # non-finite timing: reported, rows still written
        b.process(f)
    with contextlib.suppress(Q.QPSKError):
        entry(b, "process", fmt)(x)
    mf = b.last_mf(n2)
    assert b.status() & Q.STATUS_NONFINITE_TIMING
    b.close()
    h = rrc(sps, span)
    for s in range(S):
        ref = fir_ref(h, np.concatenate([f[s], widened(x[s], fmt)]))[2 * n1:]
        assert np.isnan(ref[: 2 * (T - 1)]).any() and np.isfinite(ref[2 * (T - 1):]).all()
        assert K.bitwise_equal(mf[s], ref, nan_any_payload=True), f"stream {s}"


# ---------------------------------------------------------------------------
# scales
# ---------------------------------------------------------------------------
def scale_change_between_pipelined_calls_applies_to_the_later_one(fmt):
    """The scale is captured when a call is issued: the queued call keeps its own."""
    sps, span, S = 8, 8, 5
    default, odd = FORMATS[fmt].scale, FORMATS[fmt].odd_scale
    x = signal_q(sps, span, S, fmt, seed0=77)
    n = x.shape[1] // 2
    k = n // 4
    calls = [[k] * S, [k] * S, [k] * S, [n - 3 * k] * S]
    scales = [None, odd, None, default]           # set before calls 1 and 3
    per_call = [default, odd, odd, default]
    w = np.concatenate([widened(x[:, 2 * k * c: (2 * k * (c + 1) if c < 3 else 2 * n)], fmt, per_call[c])
                        for c in range(4)], axis=1)
    b = make(S, sps, span, n - 3 * k)
    got, _ = device_calls(b, x, calls, fmt, pipelined=True, scales=scales)
    assert b.status() == 0
    b.close()
    assert_same(got, oracle_chain(w, calls, sps, span))


# ---------------------------------------------------------------------------
# FLL and IQ balancer in front (one widening pass ahead of them)
# ---------------------------------------------------------------------------
FLL = dict(enable_fll=True, cfo_loop_bandwidth=1e-3)
OFLL = dict(enable_fll=True, cfo_loop_bw=1e-3)
FRONT = {"fll-systolic": (FLL, OFLL), "fll-one-lane": (dict(vector_lanes=4, **FLL), dict(lanes=4, **OFLL)),
         "iq-balance": (dict(iq_balance=True), dict(iq_balance=True)),
         "iq-balance-fll": (dict(iq_balance=True, **FLL), dict(iq_balance=True, **OFLL))}


def fll_and_iq_balance_ragged_chunks(fmt, front):
    """Ragged chunks (shorter than one 16-byte load and than the 40-tap window,
    empty ones): host calls (the 16-byte widening pass) and device calls in the
    one-load-per-sample layout; CS16 through pipelined calls too."""
    kw, okw = FRONT[front]
    sps, span, S = 8, 8, 7
    x = signal_q(sps, span, S, fmt, n_bits=1200, seed0=85, cfo_hz=-3000.0)
    n = x.shape[1] // 2
    rng = np.random.default_rng(86)
    calls, used = [], np.zeros(S, np.int64)
    for c in range(7):
        lens = rng.integers(0, 50, S) if c < 5 else np.full(S, 37 + 1000 * (c - 5))
        if c < 2 and FORMATS[fmt].per_load == 8:
            lens = np.minimum(lens, 7)          # rows that end inside their first 8-sample load
        lens[c % S] = 0
        calls.append([int(v) for v in lens])
        used += lens
    calls.append([int(n - u) for u in used])
    want = oracle_chain(widened(x, fmt), calls, sps, span, **okw)
    nmax = max(max(c) for c in calls)
    runs = [host_calls, functools.partial(device_calls, layout="scalar")]
    if fmt == "cs16":
        runs.append(functools.partial(device_calls, pipelined=True))
    for run in runs:
        b = make(S, sps, span, nmax, **kw)
        got = run(b, x, calls, fmt)[0]
        assert b.status() == 0
        b.close()
        assert_same(got, want)


# ---------------------------------------------------------------------------
# the host ring
# ---------------------------------------------------------------------------
# streams, samples a slot holds beyond the longest chunk (8-bit: no multiple of
# 8, so the device slots are pitched), an empty chunk among the others
RING = {"cs16": (4, 8, True), "cs8": (5, 3, False), "cu8": (5, 3, False)}


def host_ring_equals_consecutive_calls(fmt, depth, fill):
    """6 ragged chunks through a ring of the format, filled in place through
    next_slot ("zero-copy"), passed from caller memory ("copy") or in turn."""
    sps, span = 8, 8
    S, pad, empty = RING[fmt]
    x = signal_q(sps, span, S, fmt, seed0=95)
    n = x.shape[1] // 2
    calls = split_calls(S, n, 5, seed=96 + depth)
    assert len(calls) == 6
    if empty:
        calls.insert(3, [0] * S)
    nmax = max(max(c) for c in calls)
    ref_b = make(S, sps, span, nmax + pad)
    want, _ = host_calls(ref_b, x, calls, fmt)
    ref_b.close()

    b = make(S, sps, span, nmax + pad)
    ring = Q.HostRing(b, depth, fmt="cs16") if FORMATS[fmt].family == "cs16" else Q.HostRing.create_fmt(b, depth, fmt)
    slot = ring.next_slot()
    assert slot.dtype == FORMATS[fmt].np_dtype and slot.shape == (S, 2 * (nmax + pad))
    pos = np.zeros(S, np.int64)
    got, pending = [], 0

    def collect():
        bits, nb, _ = ring.collect()
        got.append(decoded(Q.MODE_DEMODULATE, bits, nb, None, None))

    for ci, lens in enumerate(calls):
        if pending == depth:
            collect()
            pending -= 1
        rows = call_rows(x, lens, pos)
        m = rows.shape[1] // 2
        if fill == "zero-copy" or (fill == "alternate" and ci % 2 == 0):
            slot = ring.next_slot()
            slot[:, : 2 * m] = rows
            ring.submit(None, m, lengths_of(lens))
        else:
            ring.submit(rows if m else np.zeros((S, 2), x.dtype), m, lengths_of(lens))
        pending += 1
        pos += np.array(lens)
    while pending:
        collect()
        pending -= 1
    ring.close()
    assert b.status() == 0
    b.close()
    assert_same(got, want)
    assert_same(got, oracle_chain(widened(x, fmt), calls, sps, span))
