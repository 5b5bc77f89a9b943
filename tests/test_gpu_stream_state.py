"""Reset, read and write the state of selected streams of a batch
(qpsk_demod_reset_streams, qpsk_demod_get_streams_state,
qpsk_demod_set_streams_state, and the group's forms) on the GPU.

Every comparison is tolerance 0, on bytes or bit patterns.  Two references:

  rows    the host-only qpsk_state_blob_select / qpsk_state_blob_merge
          (tests/test_stream_state_abi.py holds those to numpy indexing): a
          read is select of the whole blob, a write leaves merge of it
  reset   per stream one OracleDemod fed the same calls; at the boundary where
          the handle calls reset_streams(ids) the instances of ids are dropped
          and constructed anew, as a C# host would (QPSKDeModulator.cs:11-56)

Ten streams at sps 8 / T = 65 and sps 4 / T = 129 (and sps 3 / T = 16 for the
copies: an even tap count leaves history rows of 8 * 15 bytes) run five ragged
host calls: long, all short (0, 1, T - 1 samples among them), long, all short,
the remainder; about 8 000 samples a stream.  IQ balancer and FLL are on where
rows are copied, so that every section of a row is non-zero.
"""
import functools

import numpy as np
import pytest

import common as K
import oracle as O
import qpsk_amd as Q
import gpu_harness as H
from gpu_harness import dev
from state_blobs import bad_blob, fresh_records, make_blob

pytestmark = pytest.mark.gpu

f4, f8 = np.float32, np.float64
S = 10
SHAPES = [(8, 8), (4, 32)]
COPY_SHAPES = SHAPES + [(3, 5)]
IDS = (0, S - 1, 4, 3)
ID_LISTS = [[0], [S - 1], [4, 3], list(range(S - 1, -1, -1))]
FLL = dict(enable_fll=True, cfo_loop_bandwidth=1e-3)
OFLL = dict(enable_fll=True, cfo_loop_bw=1e-3)
# name -> (handle knobs, oracle knobs, a DC offset on the signal)
CFGS = {
    "plain": ({}, {}, False),
    "iqb+fll": (dict(iq_balance=True, **FLL), dict(iq_balance=True, **OFLL), True),
    "non-differential": (dict(differential=False), dict(differential=False), False),
    "glibc-trig": (dict(costas_trig=1), dict(trig=O.TRIG_LIBM), False),
}
LONG, SHORT = (0, 2), (1, 3)   # the calls of the sequence by kind (call 4: the remainder)


def taps_of(sps, span):
    return 16 if (sps, span) == (3, 5) else sps * span + 1


# ---------------------------------------------------------------------------
# signals, the call sequence, the oracle
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def signal(sps, span, dc=False, n_streams=S):
    """[n_streams, 2n] float32 rows, about 8 000 samples each, noisy and 2 kHz
    off tune.  sps 3 takes the sps 4 rows (its cases copy rows; nothing decodes
    them); past ten streams the rows are the first ten rotated in time."""
    if sps == 3:
        sps, span = 4, 32
    x = K.batch_signals(S, seed0=7300 + sps, sps=sps, span=span, n_bits=16000 // sps, snr_db=16, cfo_hz=2000.0)
    if dc:
        x[:, 0::2] += 0.3
        x[:, 1::2] -= 0.2
    x = np.stack([x[s] if s < S else np.roll(x[s % S], 2 * 37 * s) for s in range(n_streams)])
    x = np.ascontiguousarray(x, dtype=f4)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def sequence(sps, span, n_streams=S):
    T = taps_of(sps, span)
    n = signal(sps, span).shape[1] // 2
    short = [0, 1, T - 1, 3, sps - 1, 40, T, 2, 64, 5]
    calls = [tuple(900 + 13 * (s % 10) for s in range(n_streams)),
             tuple(short[s % 10] for s in range(n_streams)),
             tuple(2300 + 7 * (s % 10) for s in range(n_streams)),
             tuple(short[(s + 3) % 10] for s in range(n_streams))]
    calls.append(tuple(n - sum(c[s] for c in calls) for s in range(n_streams)))
    assert {0, 1, T - 1} <= set(calls[1]) and min(calls[4]) > 3500
    return tuple(calls)


@functools.lru_cache(maxsize=None)
def oracle(cfg, sps, span, k=None, ids=(), n_streams=S):
    """outs[ci][s] = (bits, symbols): the oracle over the sequence; after call k
    the instances of ids are replaced by new ones."""
    _, okw, dc = CFGS[cfg]
    rs = K.FS // sps

    def after_call(ci, dms):
        if ci == k:
            for s in ids:
                dms[s] = O.OracleDemod(K.FS, rs, K.ALPHA, span, **okw)

    return H.oracle_run(signal(sps, span, dc, n_streams), [list(c) for c in sequence(sps, span, n_streams)], rs,
                        span, after_call=after_call, **okw)


# ---------------------------------------------------------------------------
# handles and calls
# ---------------------------------------------------------------------------
def params(cfg, sps, span, msc=None, **knobs):
    kw = dict(CFGS[cfg][0])
    kw.update(knobs)
    n = signal(sps, span).shape[1] // 2
    return Q.params(K.FS, K.FS // sps, K.ALPHA, span, max_samples_per_call=msc or n, **kw)


def make(cfg, sps, span, n_streams=S, **kw):
    b = Q.BatchDemodulator(n_streams, params(cfg, sps, span, **kw))
    assert b.rrc_taps().size == taps_of(sps, span)
    return b


def call(b, x, calls, ci, feed=None):
    """Call ci of the sequence on b, whose row r takes stream feed[r] of x
    (default: its own) from where that stream stands."""
    feed = list(range(len(calls[ci]))) if feed is None else list(feed)
    lens = np.array([calls[ci][f] for f in feed], np.int64)
    pos = np.array([sum(c[f] for c in calls[:ci]) for f in feed], np.int64)
    return H.host_call(b, H.call_rows(x[feed], lens, pos), lens)


def check_calls(b, x, calls, cis, want, what, feed=None):
    feed = list(range(len(calls[0]))) if feed is None else list(feed)
    for ci in cis:
        H.assert_same([call(b, x, calls, ci, feed)], [[want[ci][f] for f in feed]], what=f"{what},")


def fresh_rows(n, taps):
    """The rows of n streams of a new handle, as a blob."""
    return make_blob(fresh_records(n), taps)


def assert_blob(got, want, what):
    if got != want:
        ga, wa = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        assert ga.size == wa.size, f"{what}: {ga.size} vs {wa.size} bytes"
        pytest.fail(f"{what}: {np.count_nonzero(ga != wa)} bytes differ, first at {int(np.flatnonzero(ga != wa)[0])}")


def pipelined(b, x, calls, hook):
    """The sequence through process_device_async on a torch stream bound to b;
    hook(ci) runs once call ci is queued.  The decoded rows per call."""
    torch = H.need_gpu(torch=True)
    n_rows = x.shape[0]
    stream = torch.cuda.Stream()
    b.set_stream(stream.cuda_stream)
    ms = max(b.max_symbols(max(max(c) for c in calls)), 1)
    pos = np.zeros(n_rows, np.int64)
    outs = []
    with torch.cuda.stream(stream):
        for ci, lens in enumerate(calls):
            n = int(max(lens))
            rows = np.zeros((n_rows, 2 * max(n, 1)), f4)
            rows[:, : 2 * n] = H.call_rows(x, lens, pos)
            xd = torch.from_numpy(rows).to("cuda")
            bits, sy = H.out_rows(n_rows, ms, "direct")
            nb = torch.zeros(n_rows, dtype=torch.int64, device="cuda")
            ns = torch.zeros(n_rows, dtype=torch.int64, device="cuda")
            b.process_device_async(xd, n, bits, nb, syms_dev=sy, n_syms_dev=ns, lengths=np.array(lens, np.int64))
            outs.append((xd, bits, nb, sy, ns))
            pos += np.array(lens)
            hook(ci)
    b.pipeline_wait()
    torch.cuda.synchronize()
    return [H.decoded(H.DEMODULATE, bits.cpu().numpy(), nb.cpu().numpy(), sy.cpu().numpy(), ns.cpu().numpy())
            for _, bits, nb, sy, ns in outs]


# ---------------------------------------------------------------------------
# 1. read
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sps,span", COPY_SHAPES)
def test_read_is_select_of_the_whole_blob(dev, sps, span):
    x, calls, T = signal(sps, span, True), sequence(sps, span), taps_of(sps, span)
    b = make("iqb+fll", sps, span)
    for ci in range(3):
        call(b, x, calls, ci)
    whole = b.get_state()
    rec, carry, hist, dl = Q.state_blob_parts(whole, S, T)
    for name, sec in (("carry", carry[:, :3]), ("history", hist), ("delay line", dl)):
        assert all(np.any(sec[s]) for s in range(S)), f"every stream's {name} holds something"
    assert np.all(rec["iqb_re"] != 0) and np.all(rec["fll_phase"] != 0)
    for ids in ID_LISTS:
        sub = b.get_streams_state(ids)
        assert len(sub) == Q.state_blob_bytes(len(ids), T)
        assert_blob(sub, Q.state_blob_select(b.p, S, whole, ids), f"rows {ids}")
    assert_blob(b.get_state(), whole, "a read changes nothing")
    b.close()


@pytest.mark.parametrize("sps,span", COPY_SHAPES)
def test_read_waits_for_queued_calls(dev, sps, span):
    """Three pipelined calls queued, none waited for: the rows read are those
    of a twin that ran the same calls synchronously."""
    x, calls = signal(sps, span, True), sequence(sps, span)
    twin = make("iqb+fll", sps, span)
    for ci in range(3):
        call(twin, x, calls, ci)
    whole = twin.get_state()
    twin.close()
    b = make("iqb+fll", sps, span)
    got = {}

    def hook(ci):
        if ci == 2:
            got["rows"] = b.get_streams_state(list(IDS))

    pipelined(b, x, calls[:3], hook)
    assert_blob(got["rows"], Q.state_blob_select(b.p, S, whole, list(IDS)), "rows read behind queued calls")
    assert_blob(b.get_state(), whole, "the handle after them")
    assert b.gate_timeouts() == 0
    b.close()


@pytest.mark.parametrize("sps,span", SHAPES)
def test_rows_restore_into_a_handle_of_their_own(dev, sps, span):
    """A sub-blob is a blob: plain set_state of a fresh n-stream handle takes
    it, and that handle goes on as the oracle's instances of those streams."""
    x, calls = signal(sps, span, True), sequence(sps, span)
    want = oracle("iqb+fll", sps, span)
    a = make("iqb+fll", sps, span)
    for ci in range(3):
        call(a, x, calls, ci)
    ids = [4, 3, S - 1]
    sub = a.get_streams_state(ids)
    a.close()
    Q.state_blob_check(params("iqb+fll", sps, span), len(ids), sub)
    b = make("iqb+fll", sps, span, n_streams=len(ids))
    b.set_state(sub)
    assert_blob(b.get_state(), sub, "the blob read back")
    check_calls(b, x, calls, (3, 4), want, f"rows {ids} in a handle of their own", feed=ids)
    b.close()


# ---------------------------------------------------------------------------
# 2. write
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sps,span", COPY_SHAPES)
def test_write_moves_streams_between_handles(dev, sps, span):
    x, calls, T = signal(sps, span, True), sequence(sps, span), taps_of(sps, span)
    ids_a, ids_b = [2, 7, S - 1], [5, 0, 8]
    a, b = make("iqb+fll", sps, span), make("iqb+fll", sps, span)
    b.enable_link_stats()
    for ci in range(3):
        call(a, x, calls, ci)
        call(b, x, calls, ci)
    sub = a.get_streams_state(ids_a)
    a.close()
    before, sums = b.get_state(), b.link_stats()
    b.set_streams_state(ids_b, sub)
    after = b.get_state()
    assert_blob(after, Q.state_blob_merge(b.p, S, before, ids_b, sub), "B after the write")
    keep = [s for s in range(S) if s not in ids_b]
    for name, got, old in zip(("records", "carries", "histories", "delay lines"), Q.state_blob_parts(after, S, T),
                              Q.state_blob_parts(before, S, T)):
        assert got[keep].tobytes() == old[keep].tobytes(), f"untouched rows: {name}"
        assert got[ids_b].tobytes() != old[ids_b].tobytes(), f"written rows: {name}"
    now = b.link_stats()
    for field in ("n_symbols", "sum_dist2", "sum_power"):
        assert now[field].tobytes() == sums[field].tobytes(), f"the write moved {field}"
    assert np.all(sums["n_symbols"] > 0)
    if (sps, span) in SHAPES:   # B's written rows go on as A's streams, the others as their own
        feed = list(range(S))
        for r, s in zip(ids_b, ids_a):
            feed[r] = s
        check_calls(b, x, calls, (3, 4), oracle("iqb+fll", sps, span), "B after the write", feed=feed)
    b.close()


# ---------------------------------------------------------------------------
# 3. reset against the reference
# ---------------------------------------------------------------------------
def reset_case(cfg, sps, span, k, ids=IDS, n_streams=S, **kw):
    """The sequence in host calls with reset_streams(ids) behind call k."""
    x, calls, T = signal(sps, span, CFGS[cfg][2], n_streams), sequence(sps, span, n_streams), taps_of(sps, span)
    want = oracle(cfg, sps, span, k, tuple(ids), n_streams)
    b = make(cfg, sps, span, n_streams, **kw)
    check_calls(b, x, calls, range(k + 1), want, f"{cfg} before the reset")
    before = b.get_state()
    b.reset_streams(list(ids))
    new = fresh_rows(len(ids), T)
    assert_blob(b.get_streams_state(list(ids)), new, f"{cfg} reset behind call {k}: the rows against a new handle's")
    assert_blob(b.get_state(), Q.state_blob_merge(b.p, n_streams, before, list(ids), new),
                f"{cfg} reset behind call {k}: the other rows")
    check_calls(b, x, calls, range(k + 1, len(calls)), want, f"{cfg} reset behind call {k}")
    b.close()


@pytest.mark.parametrize("sps,span", SHAPES)
@pytest.mark.parametrize("cfg", list(CFGS))
def test_reset_is_a_new_receiver(dev, cfg, sps, span):
    for k in (LONG[0], SHORT[0], LONG[1], SHORT[1]):
        reset_case(cfg, sps, span, k)


def test_reset_without_a_list_does_nothing(dev):
    sps, span = 8, 8
    x, calls = signal(sps, span), sequence(sps, span)
    b = make("plain", sps, span)
    call(b, x, calls, 0)
    before = b.get_state()
    b.reset_streams([])
    assert_blob(b.get_state(), before, "n = 0")
    b.close()


def test_reset_across_two_loop_workgroups(dev):
    """70 streams in 64-stream loop workgroups: the list straddles both."""
    reset_case("plain", 4, 32, SHORT[0], ids=(0, 63, 64, 69), n_streams=70, loop_variant=5)


@pytest.mark.parametrize("sps,span", SHAPES)
def test_reset_before_a_chunked_call(dev, sps, span):
    """max_samples_per_call below the long calls: the call behind the reset
    runs in internal chunks."""
    assert sequence(sps, span)[2][0] > 1024
    reset_case("iqb+fll", sps, span, SHORT[0], msc=1024)


# ---------------------------------------------------------------------------
# 4. pipelined
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sps,span", SHAPES)
@pytest.mark.parametrize("cfg", ["plain", "iqb+fll"])
@pytest.mark.parametrize("k", [SHORT[0], LONG[1]])
def test_reset_between_pipelined_calls(dev, cfg, sps, span, k):
    x, calls = signal(sps, span, CFGS[cfg][2]), sequence(sps, span)
    b = make(cfg, sps, span)
    got = pipelined(b, x, calls, lambda ci: b.reset_streams(list(IDS)) if ci == k else None)
    H.assert_same(got, oracle(cfg, sps, span, k, IDS), what=f"{cfg} pipelined, reset behind call {k},")
    assert b.gate_timeouts() == 0
    b.close()


# ---------------------------------------------------------------------------
# 5. link statistics on
# ---------------------------------------------------------------------------
def sums_of(syms):
    """(n, sum_dist2, sum_power) of interleaved float32 symbols as the header
    defines them: float products and adds, summed in order as float64."""
    r = np.asarray(syms, f4).reshape(-1, 2)
    if r.shape[0] == 0:
        return 0, f8(0.0), f8(0.0)
    one = f4(1.0)
    e = r - np.where(r >= 0, one, -one).astype(f4)
    d2 = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]
    pw = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
    assert d2.dtype == f4 and pw.dtype == f4
    return r.shape[0], np.add.accumulate(d2.astype(f8))[-1], np.add.accumulate(pw.astype(f8))[-1]


@pytest.mark.parametrize("sps,span", SHAPES)
def test_reset_zeroes_the_rows_link_sums(dev, sps, span):
    cfg, k = "iqb+fll", SHORT[0]
    x, calls = signal(sps, span, True), sequence(sps, span)
    want = oracle(cfg, sps, span, k, IDS)
    b = make(cfg, sps, span)
    b.enable_link_stats()
    for ci in range(k + 1):
        call(b, x, calls, ci)
    before = b.link_stats()
    assert np.all(before["n_symbols"] > 0) and np.all(before["costas_freq"] != 0) and np.all(before["fll_freq"] != 0)
    b.reset_streams(list(IDS))
    after = b.link_stats()
    keep = [s for s in range(S) if s not in IDS]
    assert after[keep].tobytes() == before[keep].tobytes(), "the other rows"
    assert after[list(IDS)].tobytes() == np.zeros(len(IDS), Q.LINK_STATS_DTYPE).tobytes(), \
        "reset rows: no symbols, both sums +0, the loop state of a new receiver"
    call(b, x, calls, k + 1)
    rows = b.link_stats()
    for s in range(S):
        first = k + 1 if s in IDS else 0
        n, sd, sp = sums_of(np.concatenate([want[ci][s][1] for ci in range(first, k + 2)]))
        assert int(rows[s]["n_symbols"]) == n, f"stream {s}: n_symbols"
        assert K.bitwise_equal(rows[s]["sum_dist2"].reshape(1), np.array([sd], f8)), f"stream {s}: sum_dist2"
        assert K.bitwise_equal(rows[s]["sum_power"].reshape(1), np.array([sp], f8)), f"stream {s}: sum_power"
    b.close()


# ---------------------------------------------------------------------------
# 6. a ring, a group
# ---------------------------------------------------------------------------
def test_reset_between_two_submits_of_a_cs8_ring(dev):
    sps, span, n = 8, 8, 2000
    x8 = H.quantised(signal(sps, span), "cs8")
    rs = K.FS // sps

    def after_call(ci, dms):
        if ci == 1:
            for s in IDS:
                dms[s] = O.OracleDemod(K.FS, rs, K.ALPHA, span)

    want = H.oracle_run(H.widened(x8, "cs8"), [[n] * S] * 3, rs, span, after_call=after_call)
    b = make("plain", sps, span, msc=n)
    ring = Q.HostRing.create_fmt(b, 2, "cs8")
    got = []
    ring.submit(np.ascontiguousarray(x8[:, 0: 2 * n]), n)
    ring.submit(np.ascontiguousarray(x8[:, 2 * n: 4 * n]), n)
    got.append(ring.collect())
    b.reset_streams(list(IDS))   # chunk 1 is still outstanding: the reset waits for it
    ring.submit(np.ascontiguousarray(x8[:, 4 * n: 6 * n]), n)
    got.append(ring.collect())
    got.append(ring.collect())
    ring.close()
    for ci, (bits, nb, _) in enumerate(got):
        for s in range(S):
            assert Q.unpack_bits(bits[s], int(nb[s])) == want[ci][s][0], f"chunk {ci} stream {s}: bits"
    assert b.gate_timeouts() == 0
    b.close()


def test_group_takes_global_ids(dev):
    sps, span, cfg, k = 8, 8, "iqb+fll", SHORT[0]
    x, calls, T = signal(sps, span, True), sequence(sps, span), taps_of(sps, span)
    g = Q.DemodGroup(S, params(cfg, sps, span), [0, 0])
    first1 = g.shard(1)[0]
    ids = [first1, 0, first1 - 1, S - 1]   # both sides of the shard boundary, out of order
    want = oracle(cfg, sps, span, k, tuple(ids))
    check_calls(g, x, calls, range(k + 1), want, "group before the reset")
    # a bad list moves no shard's state: the bad index follows good ones of both shards
    states = [g.get_state(0), g.get_state(1)]
    sub = fresh_rows(3, T)
    for bad in ([0, first1, S], [0, first1, -1], [first1, 0, first1]):
        with pytest.raises(ValueError, match="qpsk error -1: stream list position 2"):
            g.reset_streams(bad)
        with pytest.raises(ValueError, match="qpsk error -1: stream list position 2"):
            g.set_streams_state(bad, sub)
        with pytest.raises(ValueError, match="qpsk error -1: stream list position 2"):
            g.get_streams_state(bad)
    with pytest.raises(ValueError, match="stream 2: carry_n"):
        g.set_streams_state([0, first1, 1], bad_blob(sps, span, 3, 2, "carry_n", 257))
    assert [g.get_state(0), g.get_state(1)] == states
    g.reset_streams(ids)
    assert_blob(g.get_streams_state(ids), fresh_rows(len(ids), T), "group reset: the rows against a new handle's")
    check_calls(g, x, calls, (k + 1, k + 2), want, "group reset")
    # stream 2 (shard 0) moves onto stream S - 1 (shard 1); a read across both shards comes in list order
    whole = [g.get_state(0), g.get_state(1)]
    both = g.get_streams_state([S - 1, 2])
    assert_blob(both[32: 32 + 2 * 112], Q.state_blob_select(g.p, S - first1, whole[1], [S - 1 - first1])[32: 32 + 112] +
                Q.state_blob_select(g.p, first1, whole[0], [2])[32: 32 + 112], "records across two shards")
    sub = g.get_streams_state([2])
    assert_blob(sub, Q.state_blob_select(g.p, first1, whole[0], [2]), "stream 2 of shard 0")
    g.set_streams_state([S - 1], sub)
    assert_blob(g.get_state(1), Q.state_blob_merge(g.p, S - first1, whole[1], [S - 1 - first1], sub), "shard 1")
    assert_blob(g.get_state(0), whole[0], "shard 0")
    feed = list(range(S - 1)) + [2]
    check_calls(g, x, calls, (k + 3,), want, "stream 2 moved onto the last row", feed=feed)
    g.close()


# ---------------------------------------------------------------------------
# 7. refusals on a live handle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sps,span", SHAPES)
def test_a_live_handle_refuses_bad_calls(dev, sps, span):
    import ctypes as C
    cfg = "iqb+fll"
    x, calls, T = signal(sps, span, True), sequence(sps, span), taps_of(sps, span)
    want = oracle(cfg, sps, span)
    b = make(cfg, sps, span)
    check_calls(b, x, calls, range(3), want, "before")
    before = b.get_state()
    good = Q.state_blob_select(b.p, S, before, [1, 2])
    L = Q.lib()
    for bad, text in (([1, S], "position 1: index %d outside" % S), ([1, -1], "position 1: index -1 outside"),
                      ([3, 1, 3], "position 2: index 3 repeated"), ([], "n = 0"), (list(range(S)) + [0], "n = 11")):
        for op in ((lambda: b.get_streams_state(bad)), (lambda: b.set_streams_state(bad, good))) + \
                  (((lambda: b.reset_streams(bad)),) if bad else ()):
            with pytest.raises(ValueError, match="qpsk error -1: stream list.*" + text):
                op()
    ids = (C.c_int32 * 2)(1, 2)
    for d in (-1, 1):   # a wrong length, either way
        buf = C.create_string_buffer(len(good) + 1)
        assert L.qpsk_demod_get_streams_state(b._h, ids, 2, buf, len(good) + d) == Q.QPSK_ERR_ARGUMENT
        assert buf.raw == b"\0" * (len(good) + 1)
        buf = C.create_string_buffer(good + b"\0", len(good) + 1)
        assert L.qpsk_demod_set_streams_state(b._h, ids, 2, buf, len(good) + d) == Q.QPSK_ERR_ARGUMENT
    assert b.get_streams_state([1, 2]) == good
    assert L.qpsk_demod_streams_state_bytes(b._h, 0) == 0 == L.qpsk_demod_streams_state_bytes(b._h, S + 1)
    assert L.qpsk_demod_streams_state_bytes(b._h, S) == len(before)
    for field, v in (("carry_n", 257), ("mu", 1.0), ("fll_pos", 40), ("base", -1)):
        with pytest.raises(ValueError, match="qpsk error -1: state blob stream 1: %s = " % field):
            b.set_streams_state([1, 2], bad_blob(sps, span, 2, 1, field, v))
    with pytest.raises(ValueError, match="qpsk error -1"):   # rows of another tap count
        b.set_streams_state([1, 2], fresh_rows(2, T + 2))
    with pytest.raises(ValueError, match="qpsk error -1"):   # one row too many for the list
        b.set_streams_state([1, 2], fresh_rows(3, T))
    assert_blob(b.get_state(), before, "after the refused calls")
    check_calls(b, x, calls, (3, 4), want, "after the refused calls")
    b.close()
