"""A framed ring (qpsk_rx_attach_framer / qpsk_rx_collect_frames) against the
oracle's DeModulateBytes per stream and chunk, fed the same chunk (for CS8 the
widened floats): lengths and bytes equal, tolerance 0.

Signals are frame_cases.signals: stream s is tad_frames(30 + 2 s, n_frames),
sps 8, span 8, K.TSC, MESSAGE_START / MESSAGE_STOP.  The frame counts asserted
below are the oracle's own (frame_cases computes each reference once).
"""
import numpy as np
import pytest

import common as K
import frame_cases as F
import qpsk_amd as Q
from gpu_harness import dev  # noqa: F401

RING = 1 << 12      # framer ring bytes a stream: the frames here hold 43 and 97 bytes


def open_ring(S, chunk, depth, fmt="cf32", tsc=K.TSC, attach=True, **kw):
    b = Q.BatchDemodulator(S, Q.params(K.FS, F.RS, K.ALPHA, F.SPAN, max_samples_per_call=chunk))
    ring = Q.HostRing.create_fmt(b, depth, fmt)
    if attach:
        kw.setdefault("max_frame_bytes", 128)
        ring.attach_framer(F.START, F.END, tsc=tsc, ring_capacity=RING, **kw)
    return b, ring


def run_ring(ring, x, chunk, lead, collect, before_submit=None):
    """Submit the whole chunks of x, keeping `lead` chunks outstanding before
    each collect (1: every chunk collected at once); collect() per chunk."""
    starts = F.chunk_starts(x.shape[1] // 2, chunk)
    out, pending = [], 0
    for ci, a in enumerate(starts):
        if before_submit:
            before_submit(ci)
        assert ring.submit(np.ascontiguousarray(x[:, 2 * a: 2 * (a + chunk)]), chunk) == ci
        pending += 1
        if pending == lead:
            out.append(collect())
            pending -= 1
    while pending:
        out.append(collect())
        pending -= 1
    return out


def assert_frames(got, want, P=128):
    """got: collect_frames() results per chunk; want: the oracle's frames."""
    assert len(got) == len(want)
    n = 0
    for ci, (res, exp) in enumerate(zip(got, want)):
        frames, lens, flags, ticket = res[:4]
        assert ticket == ci
        for s, e in enumerate(exp):
            assert int(lens[s]) == len(e), (ci, s)
            assert frames[s] == (e[:P] if e else None), (ci, s)
            n += bool(e)
        assert flags == (Q.FRAMES_TRUNCATED if any(len(e) > P for e in exp) else 0), ci
    return n


_plain_bits = {}


def plain_ring_bits(S, n_frames, chunk, fmt):
    """The bits of a ring without a framer over the same chunks, once per case."""
    key = (S, n_frames, chunk, fmt)
    if key not in _plain_bits:
        x = F.signals(S, n_frames, fmt)
        b, ring = open_ring(S, chunk, 2, fmt, attach=False)
        res = run_ring(ring, x, chunk, 1, ring.collect)
        ring.close()
        b.close()
        _plain_bits[key] = [(bits.copy(), nb.copy()) for bits, nb, _ in res]
    return _plain_bits[key]


def with_tsc(S, n_frames, chunk, fmt, depth, lead, keep_bits):
    x, want = F.tsc_case(S, n_frames, chunk, fmt)
    b, ring = open_ring(S, chunk, depth, fmt, keep_bits=keep_bits)
    assert ring.frames_bytes() == S * 128
    got = run_ring(ring, x, chunk, depth if lead else 1, lambda: ring.collect_frames(want_bits=keep_bits))
    ring.close()
    b.close()
    n = assert_frames(got, want)
    assert n >= 2 * S
    if keep_bits:
        for ci, ((bits, nb), res) in enumerate(zip(plain_ring_bits(S, n_frames, chunk, fmt), got)):
            assert np.array_equal(res[5], nb), ci
            for s in range(S):
                k = (int(nb[s]) + 7) // 8
                assert np.array_equal(res[4][s, :k], bits[s, :k]), (ci, s)
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("keep_bits", [False, True])
@pytest.mark.parametrize("lead", [False, True], ids=["eager", "outstanding"])
@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("fmt", ["cf32", "cs8"])
def test_framed_ring_with_tsc_4_streams(dev, fmt, depth, lead, keep_bits):
    """S = 4, 10 frames, chunks of 4000: 20 frames, 5 a stream, of 43 and 97 bytes."""
    assert with_tsc(4, 10, 4000, fmt, depth, lead, keep_bits) == 20
    want = F.tsc_case(4, 10, 4000, fmt)[1]
    assert sorted({len(e) for row in want for e in row if e}) == [43, 97]


@pytest.mark.gpu
@pytest.mark.parametrize("keep_bits", [False, True])
@pytest.mark.parametrize("lead", [False, True], ids=["eager", "outstanding"])
@pytest.mark.parametrize("depth", [2, 3])
@pytest.mark.parametrize("fmt", ["cf32", "cs8"])
@pytest.mark.parametrize("chunk", [4000, 4097])
def test_framed_ring_with_tsc_70_streams(dev, chunk, fmt, depth, lead, keep_bits):
    """S = 70 (more than a wave of streams), 6 frames: 140 frames, 2 a stream."""
    assert with_tsc(70, 6, chunk, fmt, depth, lead, keep_bits) == 140


@pytest.mark.gpu
@pytest.mark.parametrize("chunk,frames", [(999, 25), (1920, 30)])
def test_framed_ring_without_tsc_frames_straddle_chunks(dev, chunk, frames):
    """No TSC: every bit reaches the framer and the frames straddle the chunks.
    A twin DeviceFramer fed the ring's kept bits returns the same frames and
    ends in the string model's state (in-frame flag, ring count, carry bits)."""
    torch = dev
    x, want, states = F.plain_case(chunk)
    S = x.shape[0]
    b, ring = open_ring(S, chunk, 3, tsc=None, keep_bits=True)
    got = run_ring(ring, x, chunk, 3, lambda: ring.collect_frames(want_bits=True))
    ring.close()
    b.close()
    assert assert_frames(got, want) == frames
    twin = Q.DeviceFramer(S, F.START, F.END, ring_capacity=RING)
    st = torch.cuda.Stream()
    twin.set_stream(st.cuda_stream)
    with torch.cuda.stream(st):
        pay = torch.zeros((S, 128), dtype=torch.uint8, device="cuda")
        npay = torch.zeros(S, dtype=torch.int64, device="cuda")
        for ci, res in enumerate(got):
            twin.push(torch.from_numpy(res[4]).cuda(), torch.from_numpy(res[5]).cuda(), pay, npay)
            n, p = npay.cpu().numpy(), pay.cpu().numpy()
            for s in range(S):
                assert bytes(p[s, : int(n[s])]) == want[ci][s], (ci, s)
    inf, cnt, car = twin.status()
    assert [(bool(inf[s]), int(cnt[s]), int(car[s])) for s in range(S)] == states[-1]


@pytest.mark.gpu
def test_truncated_frames_keep_their_length(dev):
    """max_frame_bytes = 32 < 43: the lengths stay 43 and 97, 32 bytes are
    present, bit 0 is set and QPSK_ERR_CAPACITY comes back (collect_frames
    asserts that the status and the flags agree)."""
    x, want = F.tsc_case(4, 10, 4000, "cf32")
    b, ring = open_ring(4, 4000, 2, max_frame_bytes=32)
    assert ring.frames_bytes() == 4 * 32
    got = run_ring(ring, x, 4000, 2, ring.collect_frames)
    ring.close()
    b.close()
    assert assert_frames(got, want, P=32) == 20
    assert sum(res[2] == Q.FRAMES_TRUNCATED for res in got) >= 5


@pytest.mark.gpu
def test_chunk_capacity_and_a_short_buffer(dev):
    """chunk_frame_bytes = 64 with 32-byte rows: the first two streams' frames
    are stored, the rest get -1 and bit 1 is set.  A frames_cap one short of
    head[0] is refused and the same chunk is then collected."""
    x, want = F.tsc_case(4, 10, 4000, "cf32")
    b, ring = open_ring(4, 4000, 2, max_frame_bytes=30, chunk_frame_bytes=50)   # rounded up to 32 and 64
    assert (ring.max_frame_bytes, ring.frames_bytes()) == (32, 64)
    refused = []

    def collect():
        ci = len(refused)
        total = F.pack_rule([len(e) for e in want[ci]], 32, 64)[3]
        refused.append(total)
        if total:
            with pytest.raises(ValueError, match="frames_cap smaller"):
                ring.collect_frames(frames_cap=total - 1)
        return ring.collect_frames(frames_cap=total)

    got = run_ring(ring, x, 4000, 1, collect)
    ring.close()
    b.close()
    dropped = 0
    for ci, ((frames, lens, flags, ticket), exp) in enumerate(zip(got, want)):
        L = [len(e) for e in exp]
        _, _, off, _, want_flags = F.pack_rule(L, 32, 64)
        assert ticket == ci and list(lens) == L and flags == want_flags
        assert frames == [e[:32] if o >= 0 else None for e, o in zip(exp, off)], ci
        if sum(bool(e) for e in exp) == 4:
            assert [f is not None for f in frames] == [True, True, False, False] and flags & Q.FRAMES_DROPPED
            dropped += 1
    assert dropped >= 1 and sum(t > 0 for t in refused) >= 5


@pytest.mark.gpu
def test_set_markers_between_submits(dev):
    """The TSC-less case driven from IQ: chunks 6..9 run with a marker pair that
    never occurs, then the first pair again; the oracle is given the same
    markers per call.  set_markers is called with chunks outstanding."""
    chunk = 999
    x = F.signals(5, 10)
    n_chunks = len(F.chunk_starts(x.shape[1] // 2, chunk))
    sched = [F.NEVER if 6 <= ci < 10 else (F.START, F.END) for ci in range(n_chunks)]
    want = F.oracle_frames(x, "cf32", chunk, None, schedule=sched)
    assert sum(bool(e) for row in want for e in row) >= 10
    assert not any(e for row in want[6:10] for e in row)
    b, ring = open_ring(5, chunk, 3, tsc=None)

    def before(ci):
        if ci and sched[ci] != sched[ci - 1]:
            ring.set_markers(*sched[ci])

    got = run_ring(ring, x, chunk, 3, ring.collect_frames, before_submit=before)
    ring.close()
    b.close()
    assert_frames(got, want)
    # the switch changed what the oracle returns: the unswitched run differs
    assert want != F.plain_case(chunk)[1]


@pytest.mark.gpu
@pytest.mark.parametrize("lead", [1, 3])
def test_reset_streams_between_submits(dev, lead):
    """Streams 0 and 3 are reset after a chunk that leaves them inside a frame
    (picked from the string model's state): from there on they are compared
    with oracle instances constructed anew, demodulator and framer fresh, and
    the other rows go on undisturbed.  A bad list changes nothing."""
    chunk = 999
    x, _, states = F.plain_case(chunk)
    at = next(ci for ci in range(4, len(states)) if states[ci][0][0] and states[ci][3][0])
    want = F.oracle_frames(x, "cf32", chunk, None, resets={at: (0, 3)})
    assert want != F.plain_case(chunk)[1], "the reset changes what streams 0 and 3 return"
    b, ring = open_ring(5, chunk, 3, tsc=None)

    def before(ci):
        if ci == at - 1:
            for bad in ([0, 0], [5], [1, -1]):
                with pytest.raises(ValueError):
                    ring.reset_streams(bad)
            ring.reset_streams([])
        if ci == at + 1:                              # chunk `at` is the last one submitted
            ring.reset_streams([0, 3])

    got = run_ring(ring, x, chunk, lead, ring.collect_frames, before_submit=before)
    ring.close()
    b.close()
    assert assert_frames(got, want) >= 10


@pytest.mark.gpu
def test_misuse_returns_the_documented_status_and_the_ring_goes_on(dev):
    x, want = F.tsc_case(4, 10, 4000, "cf32")
    chunk = 4000
    rows = lambda ci: np.ascontiguousarray(x[:, 2 * chunk * ci: 2 * chunk * (ci + 1)])   # noqa: E731
    b, ring = open_ring(4, chunk, 2, attach=False)
    with pytest.raises(Q.QPSKError, match="no framer"):
        ring.collect_frames()
    with pytest.raises(Q.QPSKError, match="no framer"):
        ring.set_markers(F.START, F.END)
    assert ring.frames_bytes() == 0
    ring.close()
    b.close()

    # attach is refused while a chunk is outstanding, and the plain ring goes on
    b, ring = open_ring(4, chunk, 2, attach=False)
    ring.submit(rows(0), chunk)
    with pytest.raises(Q.QPSKError, match="outstanding"):
        ring.attach_framer(F.START, F.END, tsc=K.TSC, ring_capacity=RING, max_frame_bytes=128)
    bits, nb, _ = ring.collect()
    want_bits, want_nb = plain_ring_bits(4, 10, chunk, "cf32")[0]
    assert np.array_equal(nb, want_nb) and np.array_equal(bits, want_bits)
    ring.close()
    b.close()

    b, ring = open_ring(4, chunk, 2, attach=False)
    with pytest.raises(ValueError):
        ring.attach_framer(F.START, F.END, tsc=K.TSC, ring_capacity=RING, max_frame_bytes=0)
    with pytest.raises(ValueError):
        ring.attach_framer(F.START, b"", tsc=K.TSC, ring_capacity=RING, max_frame_bytes=128)
    ring.attach_framer(F.START, F.END, tsc=K.TSC, ring_capacity=RING, max_frame_bytes=128)
    with pytest.raises(Q.QPSKError, match="already"):
        ring.attach_framer(F.START, F.END, tsc=K.TSC, ring_capacity=RING, max_frame_bytes=128)
    with pytest.raises(Q.QPSKError, match="no chunk outstanding"):
        ring.collect_frames()
    got = []
    for ci in range(len(want)):
        ring.submit(rows(ci), chunk)
        with pytest.raises(Q.QPSKError, match="keeps no bits"):
            ring.collect()
        with pytest.raises(Q.QPSKError, match="keeps no bits"):
            ring.collect_frames(want_bits=True)
        got.append(ring.collect_frames())
    ring.close()
    b.close()
    assert assert_frames(got, want) == 20


@pytest.mark.gpu
def test_device_resident_chain_packs_the_oracle_frames(dev):
    """process_device -> tsc_find_device -> DeviceFramer.push ->
    frames_pack_device on one torch stream, S = 4."""
    torch = dev
    S, chunk, P = 4, 4000, 128
    x, want = F.tsc_case(S, 10, chunk, "cf32")
    dm = Q.BatchDemodulator(S, Q.params(K.FS, F.RS, K.ALPHA, F.SPAN, max_samples_per_call=chunk))
    st = torch.cuda.Stream()
    dm.set_stream(st.cuda_stream)
    fr = Q.DeviceFramer(S, F.START, F.END, ring_capacity=RING)
    fr.set_stream(st.cuda_stream)
    ms = dm.max_symbols(chunk)
    n = 0
    with torch.cuda.stream(st):
        bits = torch.zeros((S, (2 * ms + 7) // 8 + 8), dtype=torch.uint8, device="cuda")
        nbits = torch.zeros(S, dtype=torch.int64, device="cuda")
        offs = torch.zeros(S, dtype=torch.int64, device="cuda")
        pay = torch.zeros((S, P), dtype=torch.uint8, device="cuda")
        npay = torch.zeros(S, dtype=torch.int64, device="cuda")
        packed = torch.zeros(S * P, dtype=torch.uint8, device="cuda")
        poff = torch.zeros(S, dtype=torch.int64, device="cuda")
        head = torch.zeros(2, dtype=torch.int64, device="cuda")
        for ci, a in enumerate(F.chunk_starts(x.shape[1] // 2, chunk)):
            xd = torch.from_numpy(np.ascontiguousarray(x[:, 2 * a: 2 * (a + chunk)])).cuda()
            dm.process_device(xd, chunk, bits, nbits)
            Q.tsc_find_device(bits, nbits, K.TSC, offs, st.cuda_stream)
            fr.push(bits, nbits, pay, npay, offs)
            Q.frames_pack_device(pay, npay, packed, poff, head, st.cuda_stream)
            total, flags = head.cpu().tolist()
            L = [len(e) for e in want[ci]]
            _, _, want_off, want_total, want_flags = F.pack_rule(L, P, S * P)
            assert (total, flags) == (want_total, want_flags) and npay.cpu().tolist() == L
            assert poff.cpu().tolist() == list(want_off)
            got = packed.cpu().numpy()
            for s, e in enumerate(want[ci]):
                if e:
                    assert bytes(got[want_off[s]: want_off[s] + len(e)]) == e, (ci, s)
                    n += 1
    dm.close()
    assert n == 20
