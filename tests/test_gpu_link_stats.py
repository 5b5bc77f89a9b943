"""Per-stream link statistics (qpsk_demod_link_stats) against the oracle.

Expected values come from the oracle's symbols, never from the library: per
stream one OracleDemod is fed the same calls, its rotated symbols are
concatenated, and dist2 and the power are formed in numpy float32 with one
rounding per operation,

    dec = rot >= 0 ? 1 : -1      e = rot - dec
    dist2 = eI*eI + eQ*eQ        pw = rotI*rotI + rotQ*rotQ

then summed sequentially as float64 (np.add.accumulate; np.sum is pairwise).
The tolerance on n_symbols, sum_dist2 and sum_power is 0 (bit patterns; a NaN
meets a NaN).  A twin handle with statistics off and symbol rows on returns
the oracle's symbols bit for bit in the same test, so a mismatch in the sums
is the sums' own.

The loop-state fields equal the same handle's stream_states() taken right
after, bit for bit, and the oracle's private fields (read_state) at the shapes
and knobs where tests/test_gpu_state.py compares the blob with them: sps 8 /
65 taps and sps 4 / 129 taps.

Shapes: 5 streams and 70 (two workgroups of 64 x 64, three of 32 x 64, twelve
of 6 x 512, the last partly filled), six ragged calls of at most 2049 samples
with an empty call, per-stream lengths with zeros, and a one-sample call.
"""
import contextlib
import functools

import numpy as np
import pytest

import common as K
import oracle as O
import qpsk_amd as Q
from gpu_harness import call_rows, dev, oracle_run, quantised, widened

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("dev")]

SMAX = 70
SHAPES = [(8, 8), (4, 32), (2, 10)]
VARIANTS = {8: [0, 1, 2, 3, 5, 6, 7], 4: [0, 1, 2, 3, 5], 2: [0, 1, 2, 3]}
STATE_SHAPES = {(8, 8), (4, 32)}          # where test_gpu_state.py pins the blob to the oracle
ALT = "alternate"                         # constellation mode on odd calls
# name -> (handle knobs, oracle knobs, call modes)
CFGS = {
    "plain": ({}, {}, None),
    "glibc-trig": (dict(costas_trig=1), dict(trig=O.TRIG_LIBM), None),
    "non-differential": (dict(differential=False), dict(differential=False), None),
    "constellation-alternated": ({}, {}, ALT),
    "fll": (dict(enable_fll=True, cfo_loop_bandwidth=1e-3), dict(enable_fll=True, cfo_loop_bw=1e-3), None),
}
f4, f8 = np.float32, np.float64


# ---------------------------------------------------------------------------
# signals, calls, the oracle
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def signal_i8(sps, span):
    base = K.batch_signals(SMAX, seed0=5200 + sps, sps=sps, span=span, n_bits=2 * 6800 // sps, snr_db=14,
                           cfo_hz=1500.0)
    q = quantised(base, "cs8")
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def signal(sps, span, kind="base"):
    """[70, 2n] float32 rows of at least 6500 samples, noisy and 1.5 kHz off
    tune; "q8": the same rows on the int8 grid, as a CS8 call widens them."""
    if kind == "q8":
        x = widened(signal_i8(sps, span), "cs8")
    else:
        x = K.batch_signals(SMAX, seed0=5200 + sps, sps=sps, span=span, n_bits=2 * 6800 // sps, snr_db=14,
                            cfo_hz=1500.0)
    x = np.ascontiguousarray(x, dtype=f4)
    assert x.shape[1] // 2 >= 6500
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def sequence(S=SMAX):
    """Six calls as tuples of per-stream lengths: ragged with zeros, empty for
    every stream, one sample (shorter than a symbol at every sps), 2049, ragged
    with other zeros, 1111."""
    calls = [tuple(0 if s % 5 == 3 else 1500 + 37 * (s % 7) for s in range(S)),
             (0,) * S,
             (1,) * S,
             (2049,) * S,
             tuple(0 if s % 4 == 1 else 700 + 13 * s for s in range(S)),
             (1111,) * S]
    assert max(sum(c[s] for c in calls) for s in range(S)) <= 6500
    return tuple(calls)


def uniform(*ns, S=SMAX):
    return tuple((int(n),) * S for n in ns)


def call_modes(cfg, n_calls):
    if CFGS[cfg][2] != ALT:
        return [Q.MODE_DEMODULATE] * n_calls
    return [Q.MODE_CONSTELLATION if ci % 2 else Q.MODE_DEMODULATE for ci in range(n_calls)]


def sums_of(syms):
    """(n, sum_dist2, sum_power) of interleaved float32 symbols, as the header defines them."""
    r = np.asarray(syms, f4).reshape(-1, 2)
    if r.shape[0] == 0:
        return 0, f8(0.0), f8(0.0)
    one = f4(1.0)
    dec = np.where(r >= 0, one, -one).astype(f4)       # GetSign: a NaN gives -1
    e = r - dec
    d2 = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]
    pw = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
    assert e.dtype == f4 and d2.dtype == f4 and pw.dtype == f4
    with np.errstate(invalid="ignore"):
        return (r.shape[0], np.add.accumulate(d2.astype(f8))[-1], np.add.accumulate(pw.astype(f8))[-1])


@functools.lru_cache(maxsize=None)
def trace(sps, span, cfg, calls, kind="base"):
    """The oracle over calls on all the streams the calls name: outs[ci][s] =
    (bits, symbols) of call ci, states[s] = read_state() after the last call."""
    iq = signal(sps, span, kind)[: len(calls[0])]
    states = []

    def after_call(ci, dms):
        if ci == len(calls) - 1:
            states.extend(dm.read_state() for dm in dms)

    outs = oracle_run(iq, calls, K.FS // sps, span, mode=call_modes(cfg, len(calls)), after_call=after_call,
                      **CFGS[cfg][1])
    return outs, states


def expected_sums(outs, S, first=0):
    """Per stream the sums over the symbols of calls first.. of a trace."""
    return [sums_of(np.concatenate([outs[ci][s][1] for ci in range(first, len(outs))])) for s in range(S)]


# ---------------------------------------------------------------------------
# handles, calls, comparisons
# ---------------------------------------------------------------------------
def make(sps, span, S, cfg="plain", msc=2560, **knobs):
    kw = dict(CFGS[cfg][0])
    kw.update(knobs)
    return Q.BatchDemodulator(S, Q.params(K.FS, K.FS // sps, K.ALPHA, span, max_samples_per_call=msc, **kw))


def host_call(b, iq, calls, ci, mode=Q.MODE_DEMODULATE, want_syms=False, fmt=None):
    """Call ci of calls on b (which has run calls 0 .. ci - 1): uniform calls
    pass n_samples, ragged ones per-stream lengths."""
    S = len(calls[ci])
    lens = np.array(calls[ci], np.int64)
    pos = np.sum(np.array(calls[:ci], np.int64).reshape(-1, S), axis=0)
    x = call_rows(iq[:S], lens, pos)
    lengths = None if len(set(calls[ci])) == 1 and lens[0] > 0 else lens
    if fmt is None:
        bits, nb, syms, ns = b.process(x, mode=mode, lengths=lengths, want_syms=want_syms)
    else:
        bits, nb, syms, ns = b.process_fmt(x, fmt, mode=mode, lengths=lengths, want_syms=want_syms)
    dec = [Q.unpack_bits(bits[s], int(nb[s])) if mode == Q.MODE_DEMODULATE else "" for s in range(S)]
    sy = [syms[s, : 2 * int(ns[s])].copy() for s in range(S)] if syms is not None else None
    return dec, sy, ns.copy()


def same(a, b, dtype):
    return K.bitwise_equal(np.asarray(a, dtype).reshape(-1), np.asarray(b, dtype).reshape(-1), nan_any_payload=True)


def assert_sums(rows, want, what):
    assert rows.dtype == Q.LINK_STATS_DTYPE and rows.shape == (len(want),)
    for s, (n, sd, sp) in enumerate(want):
        r = rows[s]
        assert int(r["n_symbols"]) == n, f"{what} stream {s}: n_symbols {int(r['n_symbols'])} vs {n}"
        assert same(r["sum_dist2"], sd, f8), f"{what} stream {s}: sum_dist2 {r['sum_dist2']!r} vs {sd!r}"
        assert same(r["sum_power"], sp, f8), f"{what} stream {s}: sum_power {r['sum_power']!r} vs {sp!r}"


def assert_loop_state(rows, b, fll, what, ostates=None):
    """The loop-state fields against the handle's own records taken right
    after, and against the oracle's fields where given."""
    st = b.stream_states()
    for s in range(b.S):
        r = rows[s]
        pairs = [("costas_freq", st[s]["freq"], f8), ("costas_theta", st[s]["theta"], f8), ("mm_mu", st[s]["mu"], f8),
                 ("mm_rate", st[s]["integ"], f8), ("fll_freq", st[s]["fll_freq"] if fll else f4(0.0), f4)]
        for name, want, dt in pairs:
            assert same(r[name], want, dt), f"{what} stream {s}: {name} {r[name]!r} vs the record's {want!r}"
        assert int(r["error"]) == int(st[s]["error"]), f"{what} stream {s}: error"
        if ostates is not None:
            o = ostates[s]
            opairs = [("costas_freq", o["costas_freq"], f8), ("costas_theta", o["costas_theta"], f8),
                      ("mm_mu", o["mm_mu"], f8), ("mm_rate", o["mm_nco_integral"], f8)]
            if fll:
                opairs.append(("fll_freq", o["fll_freq"], f4))
            for name, want, dt in opairs:
                assert same(r[name], want, dt), f"{what} stream {s}: {name} {r[name]!r} vs the oracle's {want!r}"
            assert int(r["error"]) == 0


def run_case(sps, span, S, cfg, want_rows, calls=None, **knobs):
    """The sequence on a handle with statistics on (symbol rows as asked) and on
    a twin with statistics off and symbol rows on: the twin's symbols are the
    oracle's, the statistics are the oracle's sums, and without symbol rows the
    handle's bits, counts, status and state blob are the twin's after every call."""
    calls = calls or sequence()
    outs, ostates = trace(sps, span, cfg, calls)
    sub = tuple(c[:S] for c in calls)
    modes = call_modes(cfg, len(calls))
    iq = signal(sps, span)
    fll = bool(CFGS[cfg][0].get("enable_fll"))
    b, twin = make(sps, span, S, cfg, **knobs), make(sps, span, S, cfg, **knobs)
    b.enable_link_stats()
    for ci in range(len(sub)):
        rows_now = want_rows or modes[ci] == Q.MODE_CONSTELLATION     # that mode takes symbol rows
        bits, sy, ns = host_call(b, iq, sub, ci, modes[ci], want_syms=rows_now)
        tbits, tsy, tns = host_call(twin, iq, sub, ci, modes[ci], want_syms=True)
        for s in range(S):
            assert tbits[s] == outs[ci][s][0], f"call {ci} stream {s}: the twin's bits differ from the oracle's"
            assert K.bitwise_equal(tsy[s], outs[ci][s][1]), f"call {ci} stream {s}: the twin's symbols differ"
            if sy is not None:
                assert K.bitwise_equal(sy[s], tsy[s]), f"call {ci} stream {s}: symbol rows differ with statistics on"
        assert bits == tbits and np.array_equal(ns, tns), f"call {ci}: bits or counts differ with statistics on"
        assert b.status() == 0 == twin.status(), f"call {ci}: a status flag (OUTPUT_TRUNCATED = 2?)"
        assert b.get_state() == twin.get_state(), f"call {ci}: state blobs differ with statistics on"
    rows = b.link_stats()
    what = f"sps {sps} S {S} {cfg} {knobs}"
    assert_sums(rows, expected_sums(outs, S), what)
    assert_loop_state(rows, b, fll, what, ostates[:S] if (sps, span) in STATE_SHAPES else None)
    b.close()
    twin.close()


# ---------------------------------------------------------------------------
# 1. every loop shape, with and without symbol rows
# ---------------------------------------------------------------------------
SHAPE_CASES = [(sps, span, v) for sps, span in SHAPES for v in VARIANTS[sps]]


@pytest.mark.parametrize("want_rows", [False, True], ids=["no-rows", "rows"])
@pytest.mark.parametrize("S", [5, SMAX])
@pytest.mark.parametrize("sps,span,variant", SHAPE_CASES, ids=[f"sps{a}-T{a * b + 1}-v{v}" for a, b, v in SHAPE_CASES])
def test_sums_and_loop_state_every_shape(sps, span, variant, S, want_rows):
    run_case(sps, span, S, "plain", want_rows, loop_variant=variant)


# ---------------------------------------------------------------------------
# 2. the knobs: glibc trig, no differential decode, constellation mode, FLL
# ---------------------------------------------------------------------------
KNOB_CASES = [(cfg, sps, span, 0) for cfg in CFGS if cfg != "plain" for sps, span in [(8, 8), (4, 32)]]
KNOB_CASES += [("glibc-trig", 8, 8, 6), ("glibc-trig", 8, 8, 7), ("glibc-trig", 4, 32, 2), ("fll", 8, 8, 2)]


@pytest.mark.parametrize("cfg,sps,span,variant", KNOB_CASES,
                         ids=[f"{c}-sps{a}-T{a * b + 1}-v{v}" for c, a, b, v in KNOB_CASES])
def test_sums_and_loop_state_every_knob(cfg, sps, span, variant):
    run_case(sps, span, SMAX, cfg, False, loop_variant=variant)


# ---------------------------------------------------------------------------
# 3. chunked, pipelined, device rows, formats, ring, group
# ---------------------------------------------------------------------------
def test_chunked_call_equals_one_call():
    """max_samples_per_call = 1000 against one 4097-sample call: five internal
    chunks continue the sums exactly as one kernel does."""
    sps, span = 8, 8
    calls = uniform(4097)
    outs, ostates = trace(sps, span, "plain", calls)
    iq = signal(sps, span)
    got = []
    for msc in (1000, 4097):
        b = make(sps, span, SMAX, msc=msc)
        b.enable_link_stats()
        host_call(b, iq, calls, 0)
        rows = b.link_stats()
        assert_sums(rows, expected_sums(outs, SMAX), f"msc {msc}")
        assert_loop_state(rows, b, False, f"msc {msc}", ostates)
        assert b.status() == 0
        got.append(rows.tobytes())
        b.close()
    assert got[0] == got[1]


def test_pipelined_calls_device_rows_and_alignment(dev):
    """Three process_async calls queued, then one read (no wait in between);
    host and device rows hold the same bytes; a misaligned device row is refused."""
    torch = dev
    sps, span = 4, 32
    calls = uniform(2000, 1500, 2500)
    outs, ostates = trace(sps, span, "plain", calls)
    iq = signal(sps, span)
    b = make(sps, span, SMAX)
    b.enable_link_stats()
    ms = b.max_symbols(2500)
    xd = torch.from_numpy(np.ascontiguousarray(iq[:, : 2 * 6000])).cuda()
    keep, pos = [], 0
    for n in (2000, 1500, 2500):
        bits = torch.zeros((SMAX, ((2 * ms + 7) // 8 + 63) // 64 * 64), dtype=torch.uint8, device="cuda")
        nb = torch.zeros(SMAX, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        b.process_device_async(xd[:, 2 * pos: 2 * (pos + n)], n, bits, nb)
        keep.append((bits, nb))
        pos += n
    rows = b.link_stats()                                   # waits for the three calls
    assert_sums(rows, expected_sums(outs, SMAX), "pipelined")
    assert_loop_state(rows, b, False, "pipelined", ostates)
    for ci, (bits, nb) in enumerate(keep):
        hb, hn = bits.cpu().numpy(), nb.cpu().numpy()
        for s in range(SMAX):
            assert Q.unpack_bits(hb[s], int(hn[s])) == outs[ci][s][0], f"call {ci} stream {s}: bits"
    buf = torch.zeros(64 * SMAX + 8, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="8-byte aligned"):
        b.link_stats_device(buf[4: 4 + 64 * SMAX])
    b.link_stats_device(buf[: 64 * SMAX])
    assert b.status() == 0                                  # waits for the handle's stream
    assert buf[: 64 * SMAX].cpu().numpy().tobytes() == rows.tobytes()
    b.link_stats_device(buf[8:], reset=True)                # then zeroes the sums
    b.status()
    assert buf[8:].cpu().numpy().tobytes() == rows.tobytes()
    after = b.link_stats()
    assert_sums(after, [(0, f8(0.0), f8(0.0))] * SMAX, "after a device read with reset")
    assert_loop_state(after, b, False, "after a device read with reset", ostates)
    b.close()


def test_one_cs8_call_in_a_cf32_sequence():
    sps, span = 8, 8
    calls = sequence()
    outs, ostates = trace(sps, span, "plain", calls, "q8")
    b = make(sps, span, SMAX)
    b.enable_link_stats()
    for ci in range(len(calls)):
        if ci == 3:
            host_call(b, signal_i8(sps, span), calls, ci, fmt="cs8")
        else:
            host_call(b, signal(sps, span, "q8"), calls, ci)
    rows = b.link_stats()
    assert_sums(rows, expected_sums(outs, SMAX), "CS8 call 3")
    assert_loop_state(rows, b, False, "CS8 call 3", ostates)
    b.close()


def test_cs8_ring_three_chunks():
    """Three chunks submitted and collected through a CS8 ring, then one read
    on the handle while the ring lives (as qpsk_demod_status may be)."""
    sps, span = 8, 8
    calls = uniform(2000, 2000, 2000)
    outs, ostates = trace(sps, span, "plain", calls, "q8")
    x = signal_i8(sps, span)
    b = make(sps, span, SMAX, msc=2000)
    b.enable_link_stats()
    ring = Q.HostRing.create_fmt(b, 2, "cs8")
    got = []
    ring.submit(np.ascontiguousarray(x[:, 0:4000]), 2000)
    ring.submit(np.ascontiguousarray(x[:, 4000:8000]), 2000)
    got.append(ring.collect())
    ring.submit(np.ascontiguousarray(x[:, 8000:12000]), 2000)
    got.append(ring.collect())
    got.append(ring.collect())
    rows = b.link_stats()
    ring.close()
    for ci, (bits, nb, _) in enumerate(got):
        for s in range(SMAX):
            assert Q.unpack_bits(bits[s], int(nb[s])) == outs[ci][s][0], f"chunk {ci} stream {s}: bits"
    assert_sums(rows, expected_sums(outs, SMAX), "ring")
    assert_loop_state(rows, b, False, "ring", ostates)
    b.close()


def test_two_shard_group_equals_one_handle():
    sps, span = 8, 8
    calls = sequence()
    outs, ostates = trace(sps, span, "plain", calls)
    iq = signal(sps, span)
    p = Q.params(K.FS, K.FS // sps, K.ALPHA, span, max_samples_per_call=2560)
    g = Q.DemodGroup(SMAX, p, [0, 0])
    one = make(sps, span, SMAX)
    with pytest.raises(Q.QPSKError, match="-6"):
        g.link_stats()
    g.enable_link_stats()
    one.enable_link_stats()
    for ci in range(len(calls)):
        host_call(g, iq, calls, ci)
        host_call(one, iq, calls, ci)
    rows = g.link_stats(reset=True)
    assert_sums(rows, expected_sums(outs, SMAX), "group")
    assert rows.tobytes() == one.link_stats().tobytes()
    assert_sums(g.link_stats(), [(0, f8(0.0), f8(0.0))] * SMAX, "group after reset")
    g.close()
    one.close()


# ---------------------------------------------------------------------------
# 4. enable, reset, set_state
# ---------------------------------------------------------------------------
def test_enable_reset_and_set_state_semantics():
    sps, span = 4, 32
    calls = sequence()
    outs, ostates = trace(sps, span, "plain", calls)
    iq = signal(sps, span)
    zeros = [(0, f8(0.0), f8(0.0))] * SMAX
    b = make(sps, span, SMAX)
    L = Q.lib()
    out = np.zeros(SMAX, Q.LINK_STATS_DTYPE)
    # before enabling: a state error (and the null-argument code for a null out)
    assert L.qpsk_demod_link_stats(b._h, out.ctypes.data, Q.MEM_HOST, 0) == Q.QPSK_ERR_STATE
    assert L.qpsk_demod_link_stats(b._h, None, Q.MEM_HOST, 0) == Q.QPSK_ERR_ARGUMENT_NULL
    assert L.qpsk_demod_link_stats(b._h, out.ctypes.data, 2, 0) == Q.QPSK_ERR_ARGUMENT
    with pytest.raises(Q.QPSKError, match="-6"):
        b.link_stats()
    host_call(b, iq, calls, 0)                              # not counted: statistics are off
    b.enable_link_stats()
    assert_sums(b.link_stats(), zeros, "fresh")
    for ci in (1, 2, 3):
        host_call(b, iq, calls, ci)
    r1, r2 = b.link_stats(), b.link_stats()
    assert r1.tobytes() == r2.tobytes(), "two reads without reset differ"
    want13 = [sums_of(np.concatenate([outs[ci][s][1] for ci in (1, 2, 3)])) for s in range(SMAX)]
    assert_sums(r1, want13, "calls 1-3")
    blob = b.get_state()
    r3 = b.link_stats(reset=True)
    assert r3.tobytes() == r1.tobytes(), "a read with reset returns the sums it then zeroes"
    r4 = b.link_stats()
    assert_sums(r4, zeros, "after reset")
    for name in ("costas_freq", "costas_theta", "mm_mu", "mm_rate", "fll_freq", "error"):
        assert r4[name].tobytes() == r1[name].tobytes(), f"reset changed {name}"
    for ci in (4, 5):
        host_call(b, iq, calls, ci)
    r5 = b.link_stats()
    assert_sums(r5, expected_sums(outs, SMAX, first=4), "calls 4-5 after the reset")
    assert_loop_state(r5, b, False, "calls 4-5", ostates)
    # set_state: the loop-state fields follow the blob, the sums stay
    b.set_state(blob)
    r6 = b.link_stats()
    for name in ("n_symbols", "sum_dist2", "sum_power"):
        assert r6[name].tobytes() == r5[name].tobytes(), f"set_state changed {name}"
    for name in ("costas_freq", "costas_theta", "mm_mu", "mm_rate"):
        assert r6[name].tobytes() == r1[name].tobytes(), f"{name} is not the restored state's"
    # enabling again zeroes the sums; off again: reads are refused, calls are not counted
    b.enable_link_stats()
    assert_sums(b.link_stats(), zeros, "enabled again")
    host_call(b, iq, calls, 4)
    b.enable_link_stats(False)
    with pytest.raises(Q.QPSKError, match="-6"):
        b.link_stats()
    host_call(b, iq, calls, 5)
    b.enable_link_stats()
    assert_sums(b.link_stats(), zeros, "off and on again")
    b.close()


# ---------------------------------------------------------------------------
# 5. a NaN sample
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant,bad", [(2, 33), (5, 1), (7, 64)])
def test_nan_sample_stays_in_its_stream(variant, bad):
    """A NaN sample in one stream of the 2049-sample call: that stream's sums
    are NaN from there on (its count is still its symbols'), every other
    stream of its workgroup and of the batch is the oracle's bit for bit."""
    sps, span = 8, 8
    calls = sequence()
    outs, _ = trace(sps, span, "plain", calls)
    pos3 = sum(c[bad] for c in calls[:3])
    iq = signal(sps, span).copy()
    iq[bad, 2 * (pos3 + 100)] = np.nan
    b, twin = make(sps, span, SMAX, loop_variant=variant), make(sps, span, SMAX, loop_variant=variant)
    b.enable_link_stats()
    n_bad = 0
    for ci in range(len(calls)):
        with contextlib.suppress(Q.QPSKError):              # non-finite timing: reported, rows still written
            host_call(b, iq, calls, ci)
        lens = np.array(calls[ci], np.int64)
        x = call_rows(iq, lens, np.sum(np.array(calls[:ci], np.int64).reshape(-1, SMAX), axis=0))
        n_syms = np.zeros(SMAX, np.int64)
        nb = np.zeros(SMAX, np.int64)
        ms = max(twin.max_symbols(int(lens.max())), 1)
        bits = np.zeros((SMAX, (2 * ms + 7) // 8 + 8), np.uint8)
        sy = np.zeros((SMAX, 2 * ms), f4)
        Q.lib().qpsk_demod_process(twin._h, Q.MODE_DEMODULATE, x.ctypes.data if x.size else None, x.shape[1],
                                   x.shape[1] // 2, lens.ctypes.data_as(Q._i64p), Q.MEM_HOST, bits.ctypes.data,
                                   bits.shape[1], nb.ctypes.data, sy.ctypes.data, sy.shape[1], n_syms.ctypes.data)
        n_bad += int(n_syms[bad])
    rows = b.link_stats()
    assert b.status() & Q.STATUS_NONFINITE_TIMING
    want = expected_sums(outs, SMAX)
    good = [s for s in range(SMAX) if s != bad]
    assert_sums(rows[good], [want[s] for s in good], f"variant {variant}, beside the NaN stream")
    r = rows[bad]
    assert np.isnan(r["sum_dist2"]) and np.isnan(r["sum_power"]), "the NaN stream's sums"
    assert int(r["n_symbols"]) == n_bad > 0
    b.close()
    twin.close()
