"""State blobs (qpsk_demod_get_state / set_state) at every call edge.

Ten streams (two FLL waves, the second partly filled) at sps 8 / T = 65 and
sps 4 / T = 129 run one ragged call sequence per shape in which, in the same
call, different streams sit on different edges: an empty call for that stream
only, calls shorter than a symbol (1, 3, sps - 1), the FLL delay line (39, 40,
41), the filter history (T - 2, T - 1, T) and the loop's round sizes (63, 64,
65, 255, 256, 257); then a call that is empty for every stream, more ragged
calls, and the remainder: twelve calls, twelve boundaries.

Reference: per stream one OracleDemod fed the same calls, its private fields
read after every call (OracleDemod.read_state, tests only).  The blob is
compared with them field by field as bit patterns:

  record      every StreamState field against the reference's field of the
              same meaning; error and tofs are 0
  carry       the first carry_n samples against the retained M&M queue
  history     T - 1 samples, oldest first, against the matched filter's delay
              line read backwards from its write position
  delay line  all 80 entries as they lie (the reference's doubled line), and
              fll_pos against the filter's _pos

Then the blob is restored at every boundary (fresh and reused takers), moved
to handles with other knobs, taken while pipelined calls are queued, and bad
blobs are refused by a live handle before any kernel could see them.  Whole
blobs are compared byte for byte wherever two handles ran the same calls.

test_sequence_reaches_its_edges asserts from the oracle alone, without a GPU,
that the sequence does what it is for.
"""
import functools

import numpy as np
import pytest

import common as K
import oracle as O
import qpsk_amd as Q
import gpu_harness as H
from gpu_harness import as_fmt, assert_state, call_rows, decoded, dev, oracle_run, quantised, widened
from state_blobs import bad_blob

gpu = pytest.mark.gpu

S = 10
SHAPES = [(8, 8), (4, 32)]
FLL = dict(enable_fll=True, cfo_loop_bandwidth=1e-3)
OFLL = dict(enable_fll=True, cfo_loop_bw=1e-3)
ALT = "alternate"   # constellation mode on odd calls
# name -> (handle knobs, oracle knobs, signal, call modes)
CFGS = {
    "plain": ({}, {}, "base", None),
    "fll": (FLL, OFLL, "base", None),
    "iqb": (dict(iq_balance=True), dict(iq_balance=True), "dc", None),
    "iqb+fll": (dict(iq_balance=True, **FLL), dict(iq_balance=True, **OFLL), "dc", None),
    "glibc-trig": (dict(costas_trig=1), dict(trig=O.TRIG_LIBM), "base", None),
    "non-differential": (dict(differential=False), dict(differential=False), "base", None),
    "constellation-alternated": ({}, {}, "base", ALT),
    # the base signal quantised to int8 steps: what CS16 / CS8 / CU8 rows widen to
    "fll-q8": (FLL, OFLL, "q8", None),
}
ALL_EMPTY = 5       # index of the call that is empty for every stream
# retained M&M queue lengths the oracle reaches at a boundary of this sequence:
# 0 (nothing fed yet), 1 and 3 (one short call), then 3 for good; 2 would take
# two 1-sample calls in a row, which the edge list does not hold
QUEUE_LENGTHS = {0, 1, 3}


def taps_of(sps, span):
    return sps * span + 1


# ---------------------------------------------------------------------------
# signals, the call sequence, the oracle
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def signal_i8(sps, span):
    base = K.batch_signals(S, seed0=3100 + sps, sps=sps, span=span, n_bits=16000 // sps, snr_db=16,
                           cfo_hz=2000.0)
    q = quantised(base, "cs8")
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def signal(sps, span, kind):
    """[S, 2n] float32 rows, about 8 000 samples each, 2 kHz off tune."""
    if kind == "q8":
        x = widened(signal_i8(sps, span), "cs8")
    else:
        x = K.batch_signals(S, seed0=3100 + sps, sps=sps, span=span, n_bits=16000 // sps, snr_db=16,
                            cfo_hz=2000.0)
        if kind == "dc":   # as test_iq_balance_prestage_bit_exact
            x[:, 0::2] += 0.3
            x[:, 1::2] -= 0.2
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    return x


def edges(sps, span):
    T = taps_of(sps, span)
    return sorted({0, 1, 3, sps - 1, 39, 40, 41, T - 2, T - 1, T, 63, 64, 65, 255, 256, 257})


@functools.lru_cache(maxsize=None)
def sequence(sps, span):
    """Twelve calls as tuples of per-stream lengths: ten ragged ones in which
    stream s of ragged call c takes edge (s + c) mod len(edges), the all-empty
    call after the fifth, and the remainder."""
    E = edges(sps, span)
    n = signal(sps, span, "base").shape[1] // 2
    calls = []
    for c in range(10):
        if len(calls) == ALL_EMPTY:
            calls.append((0,) * S)
        calls.append(tuple(E[(s + c) % len(E)] for s in range(S)))
    used = np.sum(np.array(calls), axis=0)
    calls.append(tuple(int(n - u) for u in used))
    assert len(calls) == 12 and min(calls[-1]) > 4000
    return tuple(calls)


def call_modes(cfg, n_calls):
    if CFGS[cfg][3] != ALT:
        return [Q.MODE_DEMODULATE] * n_calls
    return [Q.MODE_CONSTELLATION if ci % 2 else Q.MODE_DEMODULATE for ci in range(n_calls)]


def positions(calls, k):
    """Samples each stream has consumed at boundary k (after call k); k = -1: none."""
    return np.sum(np.array(calls[: k + 1], dtype=np.int64).reshape(-1, S), axis=0)


def shortest_call(calls):
    return min((c for c in range(len(calls)) if c != ALL_EMPTY), key=lambda c: sum(calls[c]))


@functools.lru_cache(maxsize=None)
def oracle_trace(cfg, sps, span, lanes=8, lanes_after=None):
    """(outs, states): outs[ci][s] = (bits, symbols) as oracle_run gives them,
    states[ci][s] = read_state() after call ci.  lanes_after = (k, w): every
    instance moves to Vector width w after call k."""
    _, okw, kind, _ = CFGS[cfg]
    iq, calls = signal(sps, span, kind), sequence(sps, span)
    states = []

    def after_call(ci, dms):
        states.append([d.read_state() for d in dms])
        if lanes_after and lanes_after[0] == ci:
            for d in dms:
                d.set_lanes(lanes_after[1])

    outs = oracle_run(iq, calls, K.FS // sps, span, mode=call_modes(cfg, len(calls)), after_call=after_call,
                      lanes=lanes, **okw)
    return outs, states


# ---------------------------------------------------------------------------
# handles and calls
# ---------------------------------------------------------------------------
def make_handle(cfg, sps, span, n_streams=S, msc=None, **knobs):
    gkw = dict(CFGS[cfg][0])
    gkw.update(knobs)
    n = signal(sps, span, "base").shape[1] // 2
    return Q.BatchDemodulator(n_streams, Q.params(K.FS, K.FS // sps, K.ALPHA, span,
                                                  max_samples_per_call=msc or n, **gkw))


def assert_out(got, want, what):
    for s, ((gb, gs), (wb, ws)) in enumerate(zip(got, want)):
        assert gb == wb, f"{what} stream {s}: bits differ ({len(gb)} vs {len(wb)})"
        assert K.bitwise_equal(gs, ws), f"{what} stream {s}: symbols differ ({gs.size} vs {ws.size} floats)"


def host_call(b, cfg, sps, span, ci, rows=None, fmt=None):
    """Call ci of the sequence on handle b (which stands at boundary ci - 1)."""
    calls = sequence(sps, span)
    rows = signal(sps, span, CFGS[cfg][2]) if rows is None else rows
    lens = np.array(calls[ci], np.int64)
    mode = call_modes(cfg, len(calls))[ci]
    pos = positions(calls, ci - 1)
    return H.host_call(b, call_rows(rows, lens, pos), lens, mode, fmt or "cf32", family="fmt")


def run_rest(b, cfg, sps, span, first, want, what, **kw):
    """Calls first.. of the sequence on b, each against the oracle's rows."""
    for ci in range(first, len(sequence(sps, span))):
        assert_out(host_call(b, cfg, sps, span, ci, **kw), want[ci], f"{what}, call {ci}")


@functools.lru_cache(maxsize=None)
def run_a(cfg, sps, span, upto=None, knobs=()):
    """Handle A: the sequence straight through (or its calls 0..upto) in host
    calls; (outs per call, blob after every call)."""
    b = make_handle(cfg, sps, span, **dict(knobs))
    outs, blobs = [], []
    last = len(sequence(sps, span)) - 1 if upto is None else upto
    for ci in range(last + 1):
        outs.append(host_call(b, cfg, sps, span, ci))
        blobs.append(b.get_state())
    b.close()
    return outs, blobs


# ---------------------------------------------------------------------------
# without a GPU: the sequence does what it is for
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sps,span", SHAPES)
def test_sequence_reaches_its_edges(sps, span):
    T, E, calls = taps_of(sps, span), edges(sps, span), sequence(sps, span)
    ragged = [c for ci, c in enumerate(calls[:-1]) if ci != ALL_EMPTY]
    assert {v for c in ragged for v in c} == set(E), "every edge is some stream's call length"
    assert all(len(set(c)) == S for c in ragged), "in one call every stream sits on another edge"
    assert sum(calls[ALL_EMPTY]) == 0 and len(calls) == 12
    assert sum(0 in c for c in ragged) >= 5, "an empty call for one stream only"
    outs, states = oracle_trace("fll", sps, span)
    ref = oracle_run(signal(sps, span, "base"), [list(c) for c in calls], K.FS // sps, span, **OFLL)
    for ci in range(len(calls)):   # the trace is oracle_run with the fields read in between
        assert_out(outs[ci], ref[ci], f"call {ci}")
    assert sum(len(b) for b, _ in outs[-1]) > 2 * 4000 // sps * S
    # the FLL's write position in mid-ring
    assert any(st["fll_pos"] not in (0,) for sts in states[:-1] for st in sts)
    assert len({st["fll_pos"] for sts in states for st in sts}) >= 20
    # retained queue lengths
    reached = {st["mm_buf_count"] for sts in states for st in sts}
    assert reached & {0, 1, 2, 3} == QUEUE_LENGTHS and max(reached) == 3, reached
    # a history only partly overwritten: fewer than T - 1 samples since the last
    # boundary, seen in the oracle as a write position that moved by that many
    partial = 0
    for ci in range(1, len(calls)):
        for s in range(S):
            moved = (states[ci][s]["rrc_pos"] - states[ci - 1][s]["rrc_pos"]) % T
            assert moved == calls[ci][s] % T
            partial += 0 < calls[ci][s] < T - 1
    assert partial >= 4 * S
    # IQ-balancer averages that have moved from zero
    _, st_iqb = oracle_trace("iqb+fll", sps, span)
    assert all(st["iqb_avg_real"] != 0 and st["iqb_avg_img"] != 0 for st in st_iqb[0] if st["rrc_pos"])
    # every stream's first symbol lies behind some boundary, and ahead of one
    assert {st["mm_has_prev"] for sts in states for st in sts} == {0, 1}
    assert {st["diff_have_prev"] for sts in states for st in sts} == {0, 1}


# ---------------------------------------------------------------------------
# 1. the state after every call against the oracle
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("sps,span", SHAPES)
@pytest.mark.parametrize("cfg", ["plain", "fll", "iqb", "iqb+fll", "glibc-trig", "non-differential",
                                 "constellation-alternated"])
def test_state_after_every_call_equals_the_oracle(dev, cfg, sps, span):
    want, states = oracle_trace(cfg, sps, span)
    outs, blobs = run_a(cfg, sps, span)
    for ci in range(len(blobs)):
        assert_out(outs[ci], want[ci], f"call {ci}")
        assert_state(blobs[ci], states[ci], sps, span, f"after call {ci}")


# ---------------------------------------------------------------------------
# 2. restore at every boundary
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("sps,span", SHAPES)
@pytest.mark.parametrize("cfg", ["plain", "iqb+fll"])
def test_restore_at_every_boundary(dev, cfg, sps, span):
    """blob k goes into a fresh handle (even k) or into one reused handle (odd
    k), so both history-buffer parities are met on both sides.  The next call's
    rows are the oracle's, and the taker's blob after it is A's, byte for byte:
    no byte of the blob is excluded.  From the all-empty call, the shortest
    call and the middle one the rest of the sequence runs too."""
    calls = sequence(sps, span)
    want, _ = oracle_trace(cfg, sps, span)
    _, blobs = run_a(cfg, sps, span)
    long_from = {ALL_EMPTY, shortest_call(calls), len(calls) // 2}
    reused = make_handle(cfg, sps, span)
    for k in range(len(calls) - 1):
        b = reused if k % 2 else make_handle(cfg, sps, span)
        b.set_state(blobs[k])
        assert b.get_state() == blobs[k], f"boundary {k}: the blob read back"
        last = len(calls) - 1 if k in long_from else k + 1
        for ci in range(k + 1, last + 1):
            assert_out(host_call(b, cfg, sps, span, ci), want[ci], f"restored at {k}, call {ci}")
            got = b.get_state()
            if got != blobs[ci]:
                ga, wa = np.frombuffer(got, np.uint8), np.frombuffer(blobs[ci], np.uint8)
                pytest.fail(f"restored at {k}, after call {ci}: {np.count_nonzero(ga != wa)} blob bytes differ, "
                            f"first at {int(np.flatnonzero(ga != wa)[0])}")
        if b is not reused:
            b.close()
    reused.close()


# ---------------------------------------------------------------------------
# 3. portability: the same S and T, other knobs
# ---------------------------------------------------------------------------
def geometry(variant, sps, span):
    g = Q.loop_shape(variant, S, float(sps), 256, 0, True, rrc_taps=taps_of(sps, span))
    return tuple(g[k] for k in ("streams", "lanes", "round", "slots", "prefix", "cap"))


def other_loop_variants(sps, span):
    """One loop_variant per distinct shape qpsk_demod_loop_shape grants here,
    the automatic one (A's) aside."""
    seen = {geometry(0, sps, span): 0}
    for v in range(1, 8):
        seen.setdefault(geometry(v, sps, span), v)
    return sorted(v for v in seen.values() if v)


def test_loop_shapes_to_move_between():
    assert len(other_loop_variants(8, 8)) >= 4 and len(other_loop_variants(4, 32)) >= 2


@gpu
@pytest.mark.parametrize("sps,span", SHAPES)
def test_blob_moves_to_every_loop_shape(dev, sps, span):
    calls = sequence(sps, span)
    want, _ = oracle_trace("plain", sps, span)
    _, blobs = run_a("plain", sps, span)
    for v in other_loop_variants(sps, span):
        for k in (1, ALL_EMPTY):   # inside the short calls, and after the all-empty one
            b = make_handle("plain", sps, span, loop_variant=v)
            b.set_state(blobs[k])
            run_rest(b, "plain", sps, span, k + 1, want, f"loop_variant {v} from boundary {k}")
            assert b.get_state() == blobs[-1], f"loop_variant {v}: the final blob"
            b.close()
    assert len(calls) == len(blobs)


@gpu
@pytest.mark.parametrize("sps,span", SHAPES)
@pytest.mark.parametrize("lanes", [(8, 4), (4, 8)], ids=["8-to-4", "4-to-8"])
def test_blob_moves_between_vector_widths_and_fll_kernels(dev, sps, span, lanes):
    """vector_lanes 8 runs the systolic FLL kernel, 4 the one-lane kernel (and
    another summation order in both filters).  The reference has one width per
    machine; the oracle instances are moved to the other width at the same
    boundary (OracleDemod.set_lanes, tests only)."""
    frm, to = lanes
    k = 3
    want, states = oracle_trace("fll", sps, span, lanes=frm, lanes_after=(k, to))
    _, blobs = run_a("fll", sps, span, upto=k, knobs=(("vector_lanes", frm),))
    assert_state(blobs[k], states[k], sps, span, f"{frm} lanes, after call {k}")
    b = make_handle("fll", sps, span, vector_lanes=to)
    b.set_state(blobs[k])
    for ci in range(k + 1, len(want)):
        assert_out(host_call(b, "fll", sps, span, ci), want[ci], f"{frm} -> {to} lanes, call {ci}")
        assert_state(b.get_state(), states[ci], sps, span, f"{frm} -> {to} lanes, after call {ci}")
    b.close()


@gpu
@pytest.mark.parametrize("sps,span", SHAPES)
def test_blob_moves_to_a_handle_that_chunks_the_next_call(dev, sps, span):
    """max_samples_per_call = 60: the 255 .. 257-sample calls run as five
    internal chunks, the remainder as over a hundred (the tofs path straight
    after a restore)."""
    calls = sequence(sps, span)
    want, states = oracle_trace("iqb+fll", sps, span)
    _, blobs = run_a("iqb+fll", sps, span)
    first = next(k for k in range(len(calls)) if max(calls[k + 1]) >= 3 * 60)
    for k in (first, ALL_EMPTY, len(calls) - 2):
        assert max(calls[k + 1]) >= 3 * 60
        b = make_handle("iqb+fll", sps, span, msc=60)
        b.set_state(blobs[k])
        for ci in range(k + 1, len(calls)):
            assert_out(host_call(b, "iqb+fll", sps, span, ci), want[ci], f"chunked from {k}, call {ci}")
            assert_state(b.get_state(), states[ci], sps, span, f"chunked from {k}, after call {ci}")
        b.close()


def async_calls(torch, b, cfg, sps, span, first, last, peek=()):
    """Calls first..last on b through process_device_async on a stream of its
    own.  peek: after these calls get_state is taken with nothing waited for.
    Returns (device rows per call, blobs by call index)."""
    calls = sequence(sps, span)
    rows = signal(sps, span, CFGS[cfg][2])
    stream = torch.cuda.Stream()
    b.set_stream(stream.cuda_stream)
    ms = max(b.max_symbols(max(max(c) for c in calls[first: last + 1])), 1)
    outs, blobs = [], {}
    with torch.cuda.stream(stream):
        for ci in range(first, last + 1):
            lens = np.array(calls[ci], np.int64)
            n = int(lens.max())
            x = np.zeros((S, 2 * max(n, 1)), np.float32)
            x[:, : 2 * n] = call_rows(rows, lens, positions(calls, ci - 1))
            xd = torch.from_numpy(x).to("cuda")
            bits = torch.zeros((S, (2 * ms + 7) // 8 + 8), dtype=torch.uint8, device="cuda")
            sy = torch.zeros((S, 2 * ms), dtype=torch.float32, device="cuda")
            nb = torch.zeros(S, dtype=torch.int64, device="cuda")
            ns = torch.zeros(S, dtype=torch.int64, device="cuda")
            b.process_device_async(xd, n, bits, nb, syms_dev=sy, n_syms_dev=ns, lengths=lens)
            outs.append((xd, bits, nb, sy, ns))
            if ci in peek:
                blobs[ci] = b.get_state()
    return outs, blobs


def collect(torch, b, outs):
    b.pipeline_wait()
    torch.cuda.synchronize()
    return [decoded(Q.MODE_DEMODULATE, bits.cpu().numpy(), nb.cpu().numpy(), sy.cpu().numpy(), ns.cpu().numpy())
            for _, bits, nb, sy, ns in outs]


@gpu
@pytest.mark.parametrize("sps,span", SHAPES)
@pytest.mark.parametrize("cfg", ["plain", "fll"])
def test_blob_moves_to_a_pipelined_taker(dev, cfg, sps, span):
    calls = sequence(sps, span)
    want, _ = oracle_trace(cfg, sps, span)
    _, blobs = run_a(cfg, sps, span)
    for k in (2, ALL_EMPTY):
        b = make_handle(cfg, sps, span)
        b.set_state(blobs[k])
        outs, _ = async_calls(dev, b, cfg, sps, span, k + 1, len(calls) - 1)
        for i, got in enumerate(collect(dev, b, outs)):
            assert_out(got, want[k + 1 + i], f"pipelined from {k}, call {k + 1 + i}")
        assert b.get_state() == blobs[-1]
        b.close()


@gpu
@pytest.mark.parametrize("sps,span", SHAPES)
@pytest.mark.parametrize("fmt", ["cs16", "cs8", "cu8"])
def test_blob_moves_to_a_taker_fed_integer_rows(dev, fmt, sps, span):
    """A runs on the floats the integer rows widen to (the signal quantised to
    int8 steps first, as the format tests do); the taker gets the rows."""
    v = signal_i8(sps, span)
    rows = as_fmt(v, fmt)
    assert K.bitwise_equal(widened(rows, fmt), signal(sps, span, "q8"))
    want, _ = oracle_trace("fll-q8", sps, span)
    _, blobs = run_a("fll-q8", sps, span)
    k = 4
    b = make_handle("fll-q8", sps, span)
    b.set_state(blobs[k])
    run_rest(b, "fll-q8", sps, span, k + 1, want, f"{fmt} rows from boundary {k}", rows=rows, fmt=fmt)
    assert b.get_state() == blobs[-1]
    b.close()


@gpu
@pytest.mark.parametrize("sps,span", SHAPES)
def test_blob_moves_into_a_group_shard_and_back(dev, sps, span):
    """A group of 2 S streams on two shards of one device: a shard's S is the
    handle's.  A's blob goes into shard 1 (shard 0 gets empty calls), the next
    call runs through the group, shard 1's blob goes into a fresh handle."""
    cfg, k = "iqb+fll", 6
    calls = sequence(sps, span)
    want, _ = oracle_trace(cfg, sps, span)
    _, blobs = run_a(cfg, sps, span)
    rows = signal(sps, span, CFGS[cfg][2])
    n = rows.shape[1] // 2
    p = Q.params(K.FS, K.FS // sps, K.ALPHA, span, max_samples_per_call=n, **CFGS[cfg][0])
    grp = Q.DemodGroup(2 * S, p, [0, 0])
    assert grp.shard(1)[:2] == (S, S)
    fresh = grp.get_state(0)
    grp.set_state(1, blobs[k])
    assert grp.get_state(1) == blobs[k] and grp.get_state(0) == fresh
    lens = np.concatenate([np.zeros(S, np.int64), np.array(calls[k + 1], np.int64)])
    pos = np.concatenate([np.zeros(S, np.int64), positions(calls, k)])
    res = grp.process(call_rows(np.concatenate([rows, rows]), lens, pos), lengths=lens, want_syms=True)
    assert_out(decoded(Q.MODE_DEMODULATE, *res, rows=range(S, 2 * S)), want[k + 1], f"group shard 1, call {k + 1}")
    assert int(res[1][:S].sum()) == 0 and grp.get_state(0) == fresh
    back = grp.get_state(1)
    assert back == blobs[k + 1]
    grp.close()
    b = make_handle(cfg, sps, span)
    b.set_state(back)
    run_rest(b, cfg, sps, span, k + 2, want, "back in a single handle")
    assert b.get_state() == blobs[-1]
    b.close()


# ---------------------------------------------------------------------------
# 4. a blob taken under load
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("sps,span", SHAPES)
@pytest.mark.parametrize("cfg", ["plain", "iqb+fll"])
def test_blob_taken_while_calls_are_queued(dev, cfg, sps, span):
    """Every call pipelined, get_state after calls 1, 4, 5, 8 and the last with
    no pipeline_wait before it (with the FLL the newest loop kernel is not even
    issued yet): each blob is the synchronous handle's at that boundary, and
    the queued calls' rows, collected at the end, are the oracle's."""
    calls = sequence(sps, span)
    want, _ = oracle_trace(cfg, sps, span)
    _, blobs = run_a(cfg, sps, span)
    b = make_handle(cfg, sps, span)
    peek = (1, 4, ALL_EMPTY, 8, len(calls) - 1)
    outs, got = async_calls(dev, b, cfg, sps, span, 0, len(calls) - 1, peek=peek)
    for ci in peek:
        assert got[ci] == blobs[ci], f"blob taken with calls queued, after call {ci}"
    for ci, rows in enumerate(collect(dev, b, outs)):
        assert_out(rows, want[ci], f"queued call {ci}")
    b.close()


# ---------------------------------------------------------------------------
# 5. a live handle refuses a bad blob and stays as it was
# ---------------------------------------------------------------------------
BAD = [("carry_n", Q.STATE_CARRY_MAX + 1), ("fll_pos", Q.STATE_FLL_TAPS), ("tofs", 1)]


def spoiled(blob, n_streams, stream, field, value):
    """A live blob with one field of one record overwritten."""
    raw = bytearray(blob)
    rec = np.frombuffer(raw, dtype=Q.STREAM_STATE_DTYPE, count=n_streams, offset=Q.STATE_HEADER_BYTES)
    rec[field][stream] = value
    return bytes(raw)


@gpu
@pytest.mark.parametrize("sps,span", SHAPES)
def test_live_handle_refuses_bad_blobs_untouched(dev, sps, span):
    """Every assertion on a bad blob comes before the next process call: a blob
    wrongly accepted fails here, and no kernel ever runs on it."""
    cfg = "iqb+fll"
    calls = sequence(sps, span)
    want, _ = oracle_trace(cfg, sps, span)
    half = len(calls) // 2
    b = make_handle(cfg, sps, span)
    for ci in range(half):
        assert_out(host_call(b, cfg, sps, span, ci), want[ci], f"call {ci}")
    before = b.get_state()
    for field, value in BAD:
        for bad in (bad_blob(sps, span, S, S - 1, field, value), spoiled(before, S, S - 1, field, value)):
            with pytest.raises(ValueError, match=f"stream {S - 1}: {field}"):
                b.set_state(bad)
            assert b.get_state() == before, f"{field}: the handle changed"
    # the same through a two-shard group (5 + 5 streams)
    grp = Q.DemodGroup(S, b.p, [0, 0])
    n1 = grp.shard(1)[1]
    g0, g1 = grp.get_state(0), grp.get_state(1)
    for field, value in BAD:
        for bad in (bad_blob(sps, span, n1, n1 - 1, field, value), spoiled(g1, n1, n1 - 1, field, value)):
            with pytest.raises(ValueError, match=f"stream {n1 - 1}: {field}"):
                grp.set_state(1, bad)
            assert grp.get_state(0) == g0 and grp.get_state(1) == g1, f"{field}: the group changed"
    grp.close()
    run_rest(b, cfg, sps, span, half, want, "after the refusals")
    b.close()
