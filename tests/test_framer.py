"""Framer and TSC search: the host framer and the device-resident framer
(include/qpsk_demod.h, qpsk_framer_dev.hip) against the string-level
restatement of DeModulateBytes (refmodel.RefFramer, QPSKDeModulator.cs:169-259)
and str.find (the TSC strip, :413-422).

The call sequences are built to hit every branch of the reference state
machine: markers straddling call boundaries (the carry tail, :233-235), all 8
lock offsets, frames that open and close in one call, frames spanning many
calls, end markers straddling calls, calls whose TSC search failed (rxBits
empty, :179-180), empty calls, ring overflow with resync (:215-220, :241-245),
and a marker change between calls (markers are per-call arguments).
"""
import numpy as np
import pytest

import common as K
import oracle as O
import qpsk_amd as Q
from gpu_harness import dev
from refmodel import RefFramer


def rand_bytes(rng, n):
    return bytes(rng.integers(0, 256, n, dtype=np.uint8))


def to_bits(b: bytes) -> str:
    return "".join(format(v, "08b") for v in b)


def make_stream(rng, start, end, n_frames, noise_bits=(0, 300), payload=(0, 40)):
    """Noise, then frames (start, payload bytes, end) at arbitrary bit offsets."""
    out = []
    for _ in range(n_frames):
        out.append(K.random_bits(rng, int(rng.integers(*noise_bits))))
        out.append(to_bits(start) + to_bits(rand_bytes(rng, int(rng.integers(*payload)))) + to_bits(end))
    out.append(K.random_bits(rng, int(rng.integers(*noise_bits))))
    return "".join(out)


def make_calls(rng, streams, n_calls, tsc_fail=0.1, max_prefix=24):
    """Split every stream into n_calls rx strings; each call row is a random
    prefix (the bits a TSC strip would drop) + rx, or a failed TSC (-1)."""
    S = len(streams)
    cuts = [np.sort(rng.integers(0, len(s) + 1, n_calls - 1)) for s in streams]
    calls = []
    for c in range(n_calls):
        rows = []
        for s in range(S):
            a = 0 if c == 0 else int(cuts[s][c - 1])
            b = len(streams[s]) if c == n_calls - 1 else int(cuts[s][c])
            rx = streams[s][a:b]
            if rng.random() < tsc_fail:
                rows.append((K.random_bits(rng, int(rng.integers(0, 64))), -1, ""))
            else:
                pre = K.random_bits(rng, int(rng.integers(0, max_prefix)))
                rows.append((pre + rx, len(pre), rx))
        calls.append(rows)
    return calls


def pack_rows(rows):
    nmax = max(len(r[0]) for r in rows)
    stride = (nmax + 7) // 8 + 3          # deliberately not a multiple of 4
    bits = np.zeros((len(rows), stride), np.uint8)
    for s, (row, _, _) in enumerate(rows):
        if row:
            p = Q.pack_bits(row)
            bits[s, : p.size] = p
    nb = np.array([len(r[0]) for r in rows], np.int64)
    off = np.array([r[1] for r in rows], np.int64)
    return bits, nb, off


MARKERS = [(b"\x02", b"\x03"), (b"MESSAGE_START", b"MESSAGE_STOP"), (b"\xA5\x5A", b"\xFF")]


@pytest.mark.parametrize("start,end", MARKERS)
def test_host_framer_matches_string_model(start, end):
    rng = np.random.default_rng(11)
    S = 6
    streams = [make_stream(rng, start, end, 5) for _ in range(S)]
    calls = make_calls(rng, streams, 17)
    fr = Q.Framer(S, start, end)
    refs = [RefFramer() for _ in range(S)]
    n_frames = 0
    for rows in calls:
        bits, nb, off = pack_rows(rows)
        got = fr.push(bits, nb, off, payload_cap=4096)
        for s in range(S):
            exp = refs[s].push(rows[s][2], start, end)
            assert got[s] == exp
            n_frames += bool(exp)
    assert n_frames >= 10


def tad_frames(seed, n_frames, tsc=K.TSC, sps=8, span=8):
    """testAtDataLevel frames (TSC + MESSAGE_START/STOP around the payload text)
    through a seeded ±1 ppm LO pair (testAtDataLevel.cs:27-46)."""
    fs = K.FS
    rs = fs // sps
    tx = O.OracleNCO(100e6, fs, 1, 0, seed=seed)
    rx = O.OracleNCO(100e6, fs, 1, 0, seed=seed + 1)
    return np.concatenate([
        O.apply_lo_pair(tx, rx, O.modulate_text_utf8(fs, rs, K.PAYLOAD + str(i), "MESSAGE_START",
                                                     "MESSAGE_STOP", rrc_alpha=K.ALPHA,
                                                     rrc_span=span, tsc=tsc))
        for i in range(n_frames)])


@pytest.mark.parametrize("tsc,chunks", [(None, 13), (K.TSC, 4000)])
def test_string_model_matches_oracle_framer(tsc, chunks):
    """Pin the string model on the oracle's own DeModulateBytes (C
    restatement, end to end from IQ).  Without a TSC the frames straddle 13
    odd calls; with one, each 4000-sample call keeps what follows its first
    TSC (:413-422)."""
    fs, rs, span = K.FS, K.FS // 8, 8
    sig = tad_frames(15, 10, tsc=tsc or K.TSC)
    a = O.OracleDemod(fs, rs, K.ALPHA, span, tsc=tsc)
    b = O.OracleDemod(fs, rs, K.ALPHA, span, tsc=tsc)
    ref = RefFramer()
    n = sig.size // 2
    if tsc is None:
        spans = [(c[0], c[-1] + 1) for c in np.array_split(np.arange(n), chunks)]
    else:
        spans = [(a0, a0 + chunks) for a0 in range(0, n - chunks + 1, chunks)]
    got = 0
    for lo, hi in spans:
        x = sig[2 * lo: 2 * hi]
        rxb = a.DeModulate(x)
        exp = b.DeModulateBytes(x, b"MESSAGE_START", b"MESSAGE_STOP")
        assert ref.push(rxb, b"MESSAGE_START", b"MESSAGE_STOP") == exp
        got += bool(exp)
    assert got >= 4


# ---------------------------------------------------------------------------
# device framer / TSC (HIP)

RING = 1 << 20   # per-stream ring for the synthetic cases (no frame comes near it)


def run_device(torch, calls, start, end, ring_capacity=RING, payload_cap=4096,
               marker_schedule=None):
    S = len(calls[0])
    fr = Q.DeviceFramer(S, start, end, ring_capacity=ring_capacity)
    # a real stream: handle 0 (torch's legacy default) would mean "library-owned"
    stream = torch.cuda.Stream()
    fr.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        return _run_device(torch, fr, calls, payload_cap, marker_schedule), fr


def _run_device(torch, fr, calls, payload_cap, marker_schedule):
    S = len(calls[0])
    pay = torch.zeros((S, payload_cap), dtype=torch.uint8, device="cuda")
    npay = torch.zeros(S, dtype=torch.int64, device="cuda")
    outs = []
    for ci, rows in enumerate(calls):
        if marker_schedule:
            fr.set_markers(*marker_schedule[ci])
        bits, nb, off = pack_rows(rows)
        bd = torch.from_numpy(bits).cuda()
        nbd = torch.from_numpy(nb).cuda()
        offd = torch.from_numpy(off).cuda()
        fr.push(bd, nbd, pay, npay, offd)
        n = npay.cpu().numpy()
        p = pay.cpu().numpy()
        outs.append([(int(n[s]), bytes(p[s, : min(int(n[s]), payload_cap)])) for s in range(S)])
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("start,end", MARKERS)
def test_device_framer_matches_string_model(dev, start, end):
    rng = np.random.default_rng(21)
    S = 40
    streams = [make_stream(rng, start, end, 6, payload=(0, 300)) for _ in range(S)]
    calls = make_calls(rng, streams, 19)
    outs, _ = run_device(dev, calls, start, end)
    refs = [RefFramer(RING) for _ in range(S)]
    n_frames = 0
    for ci, rows in enumerate(calls):
        for s in range(S):
            exp = refs[s].push(rows[s][2], start, end)
            n, got = outs[ci][s]
            assert (n, got) == (len(exp), exp), (ci, s)
            n_frames += bool(exp)
    assert n_frames >= 2 * S


@pytest.mark.gpu
def test_device_framer_long_rows_and_offsets(dev):
    """Rows of ~260k bits (one C2 call's worth) with frames of every lock
    offset and a payload longer than the caller's payload buffer."""
    rng = np.random.default_rng(22)
    start, end = b"MESSAGE_START", b"MESSAGE_STOP"
    S = 8
    streams = [make_stream(rng, start, end, 8, noise_bits=(0, 60000), payload=(0, 3000))
               for _ in range(S)]
    calls = make_calls(rng, streams, 4, tsc_fail=0.0, max_prefix=64)
    outs, _ = run_device(dev, calls, start, end, payload_cap=1024)
    refs = [RefFramer(RING) for _ in range(S)]
    for ci, rows in enumerate(calls):
        for s in range(S):
            exp = refs[s].push(rows[s][2], start, end)
            n, got = outs[ci][s]
            assert n == len(exp) and got == exp[:1024], (ci, s)


@pytest.mark.gpu
def test_device_framer_overflow_and_marker_change(dev):
    rng = np.random.default_rng(23)
    S = 16
    m1, m2 = (b"\x02", b"\x03"), (b"\xA5\x5A", b"\xFF")
    streams = [make_stream(rng, m1[0], m1[1], 4, payload=(0, 60)) +
               make_stream(rng, m2[0], m2[1], 4, payload=(0, 60)) for _ in range(S)]
    calls = make_calls(rng, streams, 12)
    sched = [m1] * 6 + [m2] * 6
    outs, fr = run_device(dev, calls, *m1, ring_capacity=24, marker_schedule=sched)
    refs = [RefFramer(ring_capacity=24) for _ in range(S)]
    for ci, rows in enumerate(calls):
        for s in range(S):
            exp = refs[s].push(rows[s][2], *sched[ci])
            assert outs[ci][s] == (len(exp), exp), (ci, s)
    inf, cnt, car = fr.status()
    for s in range(S):
        assert bool(inf[s]) == refs[s].in_frame
        assert cnt[s] == len(refs[s].ring)
        assert car[s] == len(refs[s].carry)


@pytest.mark.gpu
@pytest.mark.parametrize("tsc", [K.TSC, "1011001", "1" * 33, K.TSC * 3, "01" * 2100, "   ", "10x1"])
def test_tsc_find_device_matches_str_find(dev, tsc):
    torch = dev
    rng = np.random.default_rng(24)
    S = 33
    rows = []
    for s in range(S):
        r = K.random_bits(rng, int(rng.integers(0, 5000)))
        if s % 3 and tsc.strip() and set(tsc) <= {"0", "1"}:   # bit rows hold only 0/1
            i = int(rng.integers(0, len(r) + 1))
            r = r[:i] + tsc + r[i:] + K.random_bits(rng, int(rng.integers(0, 100)))
        rows.append(r)
    bits, nb, _ = pack_rows([(r, 0, r) for r in rows])
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        offs = torch.full((S,), -7, dtype=torch.int64, device="cuda")
        bd = torch.from_numpy(bits).cuda()
        Q.tsc_find_device(bd, torch.from_numpy(nb).cuda(), tsc, offs, st.cuda_stream)
        got = offs.cpu().numpy()
    for s, r in enumerate(rows):
        if not tsc.strip():
            exp = 0
        else:
            i = r.find(tsc)
            exp = -1 if i < 0 else i + len(tsc)
        assert got[s] == exp, (s, len(r))
        assert Q.tsc_find(bits[s], len(r), tsc) == exp


@pytest.mark.gpu
def test_device_bytes_chain_matches_oracle(dev):
    """DeModulateBytes end to end on the device: process_device -> TSC search
    -> device framer, per stream against the oracle's DeModulateBytes on the
    testAtDataLevel frames (TSC + MESSAGE_START/STOP) with per-stream LOs."""
    torch = dev
    fs, sps, span = K.FS, 8, 8
    rs = fs // sps
    S = 4
    sigs = [tad_frames(30 + 2 * s, 10) for s in range(S)]
    n_all = min(x.size // 2 for x in sigs)
    chunk = 4000
    p = Q.params(fs, rs, K.ALPHA, span, max_samples_per_call=chunk)
    dm = Q.BatchDemodulator(S, p)
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    dm.set_stream(st.cuda_stream)
    fr = Q.DeviceFramer(S, b"MESSAGE_START", b"MESSAGE_STOP")
    fr.set_stream(st.cuda_stream)
    ms = dm.max_symbols(chunk)
    bits = torch.zeros((S, (2 * ms + 7) // 8 + 8), dtype=torch.uint8, device="cuda")
    nbits = torch.zeros(S, dtype=torch.int64, device="cuda")
    offs = torch.zeros(S, dtype=torch.int64, device="cuda")
    pay = torch.zeros((S, 256), dtype=torch.uint8, device="cuda")
    npay = torch.zeros(S, dtype=torch.int64, device="cuda")
    orc = [O.OracleDemod(fs, rs, K.ALPHA, span, tsc=K.TSC) for _ in range(S)]
    frames = 0
    for a in range(0, n_all - chunk + 1, chunk):
        x = np.stack([sig[2 * a: 2 * (a + chunk)] for sig in sigs]).astype(np.float32)
        xd = torch.from_numpy(x).cuda()
        dm.process_device(xd, chunk, bits, nbits)
        Q.tsc_find_device(bits, nbits, K.TSC, offs, st.cuda_stream)
        fr.push(bits, nbits, pay, npay, offs)
        n = npay.cpu().numpy()
        pb = pay.cpu().numpy()
        for s in range(S):
            exp = orc[s].DeModulateBytes(x[s], b"MESSAGE_START", b"MESSAGE_STOP")
            assert (int(n[s]), bytes(pb[s, : int(n[s])])) == (len(exp), exp), (a, s)
            frames += bool(exp)
    torch.cuda.set_stream(torch.cuda.default_stream())
    assert frames >= 2 * S


# ---------------------------------------------------------------------------
# Chunk edges of the early-exit searches (qpsk_framer_dev.hip).  The sizes are
# the kernels' constants: tsc_find_kernel and the framer's start hunt scan
# kFrThreads (256) windows of 32 bit positions per chunk, the end search
# kFrThreads * kEndPerThread (256 * 8) ring bytes, and each stops after the
# chunk that holds a match.
TSC_CHUNK = 256 * 32      # kFrThreads windows x 32 positions (tsc_find_kernel, start hunt)
END_CHUNK = 256 * 8       # kFrThreads * kEndPerThread ring bytes (end search)


def test_chunk_sizes_are_the_kernels_constants():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "qpsk-modulator-demodulator_amd", "csrc", "qpsk_framer_dev.hip")) as f:
        src = f.read()
    thr = int(re.search(r"constexpr int kFrThreads = (\d+);", src).group(1))
    per = int(re.search(r"constexpr int kEndPerThread = (\d+);", src).group(1))
    assert re.search(r"constexpr int kHuntWindows = kFrThreads;", src)
    assert (thr * 32, thr * per) == (TSC_CHUNK, END_CHUNK)


def rand01(rng, n):
    """n random bits as a bytearray of b'0' / b'1'."""
    return bytearray((rng.integers(0, 2, n, dtype=np.uint8) + 48).tobytes())


def place_first(rng, pat: str, n, first, others=(), protect=()):
    """An n-bit '0'/'1' string whose first occurrence of pat is at `first`
    (None: no occurrence at all), with further copies at `others` (> first).
    Random filler; an occurrence in front of `first` loses one filler bit until
    str.find says the first one is where the case means it to be.  protect:
    (position, bits) pieces written into the filler that the repair leaves alone."""
    m = len(pat)
    pb = pat.encode()
    row = rand01(rng, n)
    fixed = np.zeros(n, bool)
    for q, piece in protect:
        row[q: q + len(piece)] = piece.encode()
        fixed[q: q + len(piece)] = True
    for q in ([] if first is None else [first, *others]):
        assert q + m <= n
        row[q: q + m] = pb
        fixed[q: q + m] = True
    stop = n if first is None else first
    at = 0
    for _ in range(4 * n + 16):
        i = row.find(pb, at)
        if i < 0 or i >= stop:
            break
        free = [k for k in range(i, i + m) if not fixed[k]]
        assert free, "an occurrence made of fixed bits only"
        row[free[-1]] ^= 1                    # '0' <-> '1'
        at = max(0, i - m + 1)
    s = row.decode()
    assert s.find(pat) == (-1 if first is None else first)
    for q, piece in protect:
        assert s[q: q + len(piece)] == piece
    return s


TSC_LENGTHS = [1, 7, 15, 16, 17, 31, 32, 33, 64, 4200]
_tsc_cases = {}


def tsc_edge_rows(m):
    """(pattern, rows) of B2 for one pattern length; every row's expectation is str.find's."""
    if m in _tsc_cases:
        return _tsc_cases[m]
    rng = np.random.default_rng(7000 + m)
    pat = "1" if m == 1 else K.random_bits(rng, m)
    C = TSC_CHUNK
    near = sorted(range(C - m - 2, C + 3), key=lambda p: (abs(p - C), p))[:40]
    rows = []
    for p in sorted(near) + [2 * C - 1, 2 * C, 2 * C + 1, 3 * C, 30000]:
        # a second copy 40 bits later (behind the first one's end if the pattern
        # is longer than that: two copies of a random pattern cannot overlap)
        # or one chunk later
        for others in ((), (p + 40 if m <= 40 else p + m + 40,), (p + C,)):
            n = max([p, *others]) + m + int(rng.integers(0, 100))
            rows.append(place_first(rng, pat, n, p, others))
    for last in (C - 1, C, C + 1):            # the only occurrence at the last legal position n - m
        rows.append(place_first(rng, pat, last + m, last))
    # three chunks without an occurrence, seeded with near-misses: the first 16
    # and the first 32 pattern bits followed by a differing bit
    for _ in range(2):
        protect = []
        spots = rng.choice(np.arange(40, 3 * C - 40, 80), 48, replace=False)
        for k, qs in ((16, spots[:24]), (32, spots[24:])):
            if m > k:
                miss = pat[:k] + ("1" if pat[k] == "0" else "0")
                protect += [(int(q), miss) for q in qs]
        protect.sort()
        rows.append(place_first(rng, pat, 3 * C + 5, None, protect=protect))
        if m > 16:
            assert rows[-1].count(pat[:16]) >= 24
    _tsc_cases[m] = (pat, rows)
    return pat, rows


def tsc_expect(row, tsc):
    i = row.find(tsc)
    return -1 if i < 0 else i + len(tsc)


PERIODIC = [("1" * 33, ["1" * n for n in (32, 33, 3 * TSC_CHUNK + 7)] + ["01" * 12300]),
            ("1" * 32 + "0", ["1" * (3 * TSC_CHUNK + 7), "1" * TSC_CHUNK + "0" + "1" * 40, "1" * (TSC_CHUNK - 32) + "0"]),
            ("01" * 20, ["01" * 12300, "1" + "01" * 12300, "1" * (3 * TSC_CHUNK + 7), "10" * 19 + "1"]),
            ("01" * 19 + "00", ["01" * 12300, "01" * 4090 + "00" + "01" * 30, "1" + "01" * 8200 + "001"])]


@pytest.mark.parametrize("m", TSC_LENGTHS)
def test_tsc_find_host_at_chunk_edges(m):
    pat, rows = tsc_edge_rows(m)
    bits, _, _ = pack_rows([(r, 0, r) for r in rows])
    for s, r in enumerate(rows):
        assert Q.tsc_find(bits[s], len(r), pat) == tsc_expect(r, pat), (m, s, len(r))


def test_tsc_edge_case_count():
    """966 rows with a first occurrence at or near a chunk edge, alone or with a second copy."""
    total = 0
    for m in TSC_LENGTHS:
        pat, rows = tsc_edge_rows(m)
        hits = [r.find(pat) for r in rows]
        total += sum(h >= 0 for h in hits) - 3
        for p in (TSC_CHUNK - 1, TSC_CHUNK, TSC_CHUNK + 1, 2 * TSC_CHUNK - 1, 2 * TSC_CHUNK, 3 * TSC_CHUNK):
            assert hits.count(p) >= 3, (m, p)
        assert hits.count(-1) == 2
    assert total == 966


def tsc_device(torch, rows, tsc):
    bits, nb, _ = pack_rows([(r, 0, r) for r in rows])
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        offs = torch.full((len(rows),), -7, dtype=torch.int64, device="cuda")
        bd = torch.from_numpy(bits).cuda()
        Q.tsc_find_device(bd, torch.from_numpy(nb).cuda(), tsc, offs, st.cuda_stream)
        got = offs.cpu().numpy()
    return bits, got


@pytest.mark.gpu
@pytest.mark.parametrize("m", TSC_LENGTHS)
def test_tsc_find_device_at_chunk_edges(dev, m):
    """One launch, one row per case: the first occurrence on either side of
    every chunk edge and across it, a later copy in the same or the next
    chunk (which a search that leaves early, or late, would report)."""
    pat, rows = tsc_edge_rows(m)
    want = [tsc_expect(r, pat) for r in rows]
    bits, got = tsc_device(dev, rows, pat)
    for s, r in enumerate(rows):
        assert got[s] == want[s], (m, s, len(r), r.find(pat))
        assert Q.tsc_find(bits[s], len(r), pat) == want[s]


@pytest.mark.gpu
@pytest.mark.parametrize("tsc,rows", PERIODIC, ids=["ones", "ones-broken", "01", "01-broken"])
def test_tsc_find_device_periodic_rows(dev, tsc, rows):
    bits, got = tsc_device(dev, rows, tsc)
    for s, r in enumerate(rows):
        assert got[s] == tsc_expect(r, tsc), (s, len(r))
        assert Q.tsc_find(bits[s], len(r), tsc) == tsc_expect(r, tsc)


# ---------------------------------------------------------------------------
# framer: reference first, then the device with status() after every call

def ref_calls(calls, sched, ring_capacity):
    """RefFramer per stream; per call and stream (payload, in_frame, ring bytes,
    carry bits), and the framers (for their lock offsets)."""
    S = len(calls[0])
    refs = [RefFramer(ring_capacity) for _ in range(S)]
    want = []
    for ci, rows in enumerate(calls):
        res = []
        for s in range(S):
            pay = refs[s].push(rows[s][2], *sched[ci])
            res.append((pay, refs[s].in_frame, len(refs[s].ring), len(refs[s].carry)))
        want.append(res)
    return want, refs


def device_matches(torch, calls, sched, ring_capacity, want, payload_cap=4096):
    S = len(calls[0])
    fr = Q.DeviceFramer(S, *sched[0], ring_capacity=ring_capacity)
    stream = torch.cuda.Stream()
    fr.set_stream(stream.cuda_stream)
    with torch.cuda.stream(stream):
        pay = torch.zeros((S, payload_cap), dtype=torch.uint8, device="cuda")
        npay = torch.zeros(S, dtype=torch.int64, device="cuda")
        for ci, rows in enumerate(calls):
            if ci and sched[ci] != sched[ci - 1]:
                fr.set_markers(*sched[ci])
            bits, nb, off = pack_rows(rows)
            fr.push(torch.from_numpy(bits).cuda(), torch.from_numpy(nb).cuda(), pay, npay,
                    torch.from_numpy(off).cuda())
            n = npay.cpu().numpy()
            p = pay.cpu().numpy()
            inf, cnt, car = fr.status()
            for s in range(S):
                exp, in_frame, count, carry = want[ci][s]
                assert int(n[s]) == len(exp), (ci, s, int(n[s]), len(exp))
                assert bytes(p[s, : len(exp)]) == exp, (ci, s)
                assert (bool(inf[s]), int(cnt[s]), int(car[s])) == (in_frame, count, carry), (ci, s)


def rows_of(pieces, rng, max_prefix=24):
    """One call: per stream its rx string behind a random prefix (the bits a TSC strip drops)."""
    rows = []
    for rx in pieces:
        pre = K.random_bits(rng, int(rng.integers(0, max_prefix)))
        rows.append((pre + rx, len(pre), rx))
    return rows


def bytes_without(rng, n, marker: bytes):
    """n random bytes in which marker does not occur."""
    b = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    while True:
        i = b.find(marker)
        if i < 0:
            return bytes(b)
        b[i] ^= 0x55


EDGE_MARKERS = [(b"MESSAGE_START", b"MESSAGE_STOP"), (b"\xA5\x5A\xC3", b"\x3C\xFF")]
_end_cases = {}


def end_edge_case(start, end):
    """B3, end search.  Streams 0..11: a frame that opens and closes in one call,
    the end marker's first occurrence at ring positions 2047, 2048, 2049,
    2048 - ne + 1 (across the chunk edge) and 4096 -+ 1, alone and with a second
    end marker one chunk later.  Then frames already open with bytes in the ring
    and a partial packer byte: stream 12 appends more than two chunks of bytes
    with no end marker, then closes; streams 13.. split the end marker k | ne - k
    bytes over the old ring and the call's new bytes (k = 1 .. ne - 1, the search
    starts ne bytes in front of the new ones)."""
    key = (start, end)
    if key in _end_cases:
        return _end_cases[key]
    rng = np.random.default_rng(7100 + len(end))
    ne = len(end)
    sb, eb = to_bits(start), to_bits(end)
    noise = lambda k: place_first(rng, sb, k, None) if k else ""   # noqa: E731  no start marker at any offset
    streams = []                                                   # per stream: rx strings of calls 0..2
    where = []
    for pos in (END_CHUNK - 1, END_CHUNK, END_CHUNK + 1, END_CHUNK - ne + 1, 2 * END_CHUNK - 1, 2 * END_CHUNK + 1):
        for second in (False, True):
            body = bytes_without(rng, pos, end) + end
            if second:
                body += bytes_without(rng, END_CHUNK - ne, end) + end
            assert body.find(end) == pos
            body += rand_bytes(rng, 3)
            rx = noise(int(rng.integers(0, 60))) + sb + to_bits(body) + K.random_bits(rng, int(rng.integers(0, 8)))
            streams.append([rx, noise(50), ""])
            where.append(pos)
    # open frames: call 0 opens and leaves a partial byte, call 1 appends, call 2 closes
    long_body = bytes_without(rng, 2 * END_CHUNK + 300, end)
    lb = to_bits(long_body)
    streams.append([noise(13) + sb + to_bits(bytes_without(rng, 40, end)) + "101",
                    lb, "01101" + eb + "0110"])
    for k in range(1, ne):
        head = to_bits(bytes_without(rng, 30 + k, end))
        bits = head + eb + K.random_bits(rng, 11)
        cut = len(head) + 8 * k + 3                                # k marker bytes and 3 more bits in call 0
        streams.append([noise(5) + sb + bits[:cut], bits[cut:], noise(40)])
    calls = [rows_of([st[c] for st in streams], rng) for c in range(3)]
    sched = [(start, end)] * 3
    want, _ = ref_calls(calls, sched, RING)
    for s, pos in enumerate(where):                                # the scenario, from the string model
        assert len(want[0][s][0]) == pos and not want[0][s][1], (s, pos)
    s = len(where)
    assert want[0][s][1] and want[0][s][2] == 40 and want[1][s][1] and want[1][s][2] > 2 * END_CHUNK + 40
    assert len(want[2][s][0]) == want[1][s][2] + 1                 # 3 + 5 bits complete the partial byte
    for k in range(1, ne):
        s = len(where) + k
        assert want[0][s][1] and want[0][s][2] == 30 + k + k, (k, want[0][s])
        assert len(want[1][s][0]) == 30 + k, (k, want[1][s])
    _end_cases[key] = (calls, sched, want)
    return _end_cases[key]


@pytest.mark.parametrize("start,end", EDGE_MARKERS)
def test_host_framer_end_search_at_chunk_edges(start, end):
    calls, sched, want = end_edge_case(start, end)
    fr = Q.Framer(len(calls[0]), start, end, ring_capacity=RING)
    for ci, rows in enumerate(calls):
        bits, nb, off = pack_rows(rows)
        got = fr.push(bits, nb, off, payload_cap=8192)
        assert got == [w[0] for w in want[ci]], ci


@pytest.mark.gpu
@pytest.mark.parametrize("start,end", EDGE_MARKERS)
def test_device_framer_end_search_at_chunk_edges(dev, start, end):
    calls, sched, want = end_edge_case(start, end)
    device_matches(dev, calls, sched, RING, want, payload_cap=8192)


def test_end_marker_in_front_of_the_search_start_is_not_found():
    marker_change_case()


_marker_change = []


def marker_change_case():
    """An end marker that lies in the ring in front of the search start: the
    markers change between calls (they are per-call arguments) and the new end
    marker already sits in the bytes an earlier call appended.  RingIndexOf
    starts at count - (appended + ne) (QPSKDeModulator.cs:246), so the frame
    closes at the later copy; in stream 1 the old copy begins one byte in
    front of that start, reaches into the searched bytes and still must not
    match."""
    if _marker_change:
        return _marker_change[0]
    rng = np.random.default_rng(7200)
    start, end_a, end_b = b"\xA5\x5A\xC3", b"\x3C\xFF", b"\x77\x10\x99"
    sb = to_bits(start)
    body = bytes_without(rng, 50, end_a)
    body0 = body[:20] + end_b + body[23:]                          # end_b early in the ring
    body1 = body[:46] + end_b + b"\x00"                            # end_b one byte in front of call 1's search start
    tail = to_bits(bytes_without(rng, 9, end_b) + end_b) + "11"
    streams = [[sb + to_bits(body0) + "1", "0110", "011" + tail],  # 1 + 4 + 3 bits: one more ring byte
               [sb + to_bits(body1), to_bits(b"\x99"), tail]]
    calls = [rows_of([st[c] for st in streams], rng) for c in range(3)]
    sched = [(start, end_a), (start, end_b), (start, end_b)]
    want, _ = ref_calls(calls, sched, RING)
    assert want[1][0][1] and want[1][1][1], "both frames stay open over the marker change"
    assert len(want[2][0][0]) == 50 + 1 + 9 and len(want[2][1][0]) == 50 + 1 + 9
    _marker_change.append((calls, sched, want))
    return _marker_change[0]


@pytest.mark.gpu
def test_device_framer_end_marker_in_front_of_the_search_start(dev):
    calls, sched, want = marker_change_case()
    device_matches(dev, calls, sched, RING, want)


_hunt_cases = {}


def hunt_edge_case(start, end, ks):
    """B3, start hunt: the start marker's first bit at every position from
    8192 k - 8 ns to 8192 k + 8 of the candidate string (all eight lock
    offsets), one stream each; then two markers of which the later one has
    the smaller offset, and a marker that begins in the carry and ends in a
    long row.  Call 0 opens the frames (no end marker in it), call 1 closes
    them."""
    key = (start, end, ks)
    if key in _hunt_cases:
        return _hunt_cases[key]
    rng = np.random.default_rng(7300 + len(start))
    ns = len(start)
    sb, eb = to_bits(start), to_bits(end)
    C = TSC_CHUNK
    after = to_bits(bytes_without(rng, 6, end)) + "101"            # a partial byte of 3 bits stays in the packer
    close = "01101" + eb                                           # 5 bits complete it, then the end marker
    streams, lock = [], []
    for k in ks:
        for q in range(C * k - 8 * ns, C * k + 9):
            streams.append([place_first(rng, sb, q + 8 * ns, q) + after, close])
            lock.append(q % 8)
    # offset 3 in chunk 0 and offset 0 in chunk 2: offset 0 wins (the offset loop runs first)
    q1, q2 = 8 * 300 + 3, 2 * C + 8 * 77
    streams.append([place_first(rng, sb, q2 + 8 * ns, q1, (q2,)) + after, close])
    lock.append(0)
    # offset 5 in chunk 0, offset 2 in chunk 1, none at offset 0: offset 2 wins
    q1, q2 = 8 * 500 + 5, C + 8 * 40 + 2
    streams.append([place_first(rng, sb, q2 + 8 * ns, q1, (q2,)) + after, close])
    lock.append(2)
    n_open = len(streams)
    # the marker begins in the carry (call 0 ends inside it) and ends in a long row
    split = 8 * ns - 5
    streams.append([place_first(rng, sb, 90, None) + sb[:split],
                    sb[split:] + to_bits(bytes_without(rng, 2 * C // 8, end)) + "1"])
    calls = [rows_of([st[c] for st in streams], rng, max_prefix=9) for c in range(2)]
    sched = [(start, end)] * 2
    S = len(streams)
    refs = [RefFramer(RING) for _ in range(S)]
    want = []
    for ci, rows in enumerate(calls):
        res = []
        for s in range(S):
            pay = refs[s].push(rows[s][2], start, end)
            res.append((pay, refs[s].in_frame, len(refs[s].ring), len(refs[s].carry)))
        if ci == 0:                                                # the scenario, from the string model
            assert [r.locked for r in refs[:n_open]] == lock
            assert not refs[-1].in_frame and len(refs[-1].carry) == 8 * ns + 7
        want.append(res)
    assert all(len(want[1][s][0]) == 7 for s in range(n_open))
    assert refs[-1].in_frame and len(refs[-1].ring) == 2 * C // 8
    _hunt_cases[key] = (calls, sched, want)
    return _hunt_cases[key]


HUNT = [(b"\xA5\x5A", b"\x3C\xFF", (1, 2)), (b"MESSAGE_START", b"MESSAGE_STOP", (1,))]


@pytest.mark.parametrize("start,end,ks", HUNT)
def test_host_framer_start_hunt_at_chunk_edges(start, end, ks):
    calls, sched, want = hunt_edge_case(start, end, ks)
    fr = Q.Framer(len(calls[0]), start, end, ring_capacity=RING)
    for ci, rows in enumerate(calls):
        bits, nb, off = pack_rows(rows)
        assert fr.push(bits, nb, off, payload_cap=4096) == [w[0] for w in want[ci]], ci


@pytest.mark.gpu
@pytest.mark.parametrize("start,end,ks", HUNT)
def test_device_framer_start_hunt_at_chunk_edges(dev, start, end, ks):
    calls, sched, want = hunt_edge_case(start, end, ks)
    device_matches(dev, calls, sched, RING, want)


DRIP_MARKERS = [(b"\x02", b"\x03"), (b"\xA5\x5A\xC3", b"\x3C\xFF")]
_drip_cases = {}


def drip_case(start, end):
    """Start hunt, short calls: 5 noise bits, the start marker, a 3-byte
    payload, the end marker and 9 tail bits arrive k bits per call, one stream
    per k (a stream that has run out gets an empty rx).  While carry + rx is
    shorter than the start marker the hunt has no position to test."""
    key = (start, end)
    if key in _drip_cases:
        return _drip_cases[key]
    rng = np.random.default_rng(7500 + len(start))
    ns = len(start)
    ks = (1, 2, 3, 5, 7, 8 * ns - 1)
    streams, payloads = [], []
    for _ in ks:
        payloads.append(bytes_without(rng, 3, end))
        streams.append(place_first(rng, to_bits(start), 5 + 8 * ns, 5) + to_bits(payloads[-1]) + to_bits(end) +
                       K.random_bits(rng, 9))
    n_calls = max(-(-len(st) // k) for st, k in zip(streams, ks))
    calls = [rows_of([st[c * k: (c + 1) * k] for st, k in zip(streams, ks)], rng) for c in range(n_calls)]
    sched = [(start, end)] * n_calls
    want, _ = ref_calls(calls, sched, RING)
    for s in range(len(ks)):                                       # the scenario, from the string model
        assert [w[s][0] for w in want if w[s][0]] == [payloads[s]], s
        hunting = [(False, 0, 0)] + [w[s][1:] for w in want[:-1]]  # the state each call starts from
        assert any(not in_frame and rows[s][2] and carry + len(rows[s][2]) < 8 * ns
                   for rows, (in_frame, _, carry) in zip(calls, hunting)), s
    _drip_cases[key] = (calls, sched, want)
    return _drip_cases[key]


@pytest.mark.parametrize("start,end", DRIP_MARKERS)
def test_host_framer_start_hunt_on_dripping_bits(start, end):
    calls, sched, want = drip_case(start, end)
    fr = Q.Framer(len(calls[0]), start, end, ring_capacity=RING)
    for ci, rows in enumerate(calls):
        bits, nb, off = pack_rows(rows)
        assert fr.push(bits, nb, off, payload_cap=4096) == [w[0] for w in want[ci]], ci


@pytest.mark.gpu
@pytest.mark.parametrize("start,end", DRIP_MARKERS)
def test_device_framer_start_hunt_on_dripping_bits(dev, start, end):
    calls, sched, want = drip_case(start, end)
    device_matches(dev, calls, sched, RING, want)


# ---------------------------------------------------------------------------
# B4.  Low-entropy streams: markers that overlap themselves, start == end, an
# end marker inside the start marker's tail -- where a data-parallel
# restatement of a string state machine tends to diverge from it.
LOW_ENTROPY = [(b"\xAA", b"\xAA"), (b"\xAA\xAA", b"\x55"), (b"\x00", b"\x00\x00"), (b"\xFF\xFF", b"\xFF"),
               (b"ABA", b"BAB"), (b"\x02", b"\x02\x02\x03"), (b"\xF0\x0F", b"\x0F\xF0")]
LOW_RINGS = [8, 24, 4096]
_low = {}


def low_entropy_case(pair, cap):
    """64 streams of 200..1500 bits drawn from marker pieces, over 40 calls cut
    at random positions; 5 % of the rows have a failed TSC, the others a
    random prefix of 0..23 bits.  Returns (calls, sched, want, frames)."""
    key = (pair, cap)
    if key in _low:
        return _low[key]
    start, end = LOW_ENTROPY[pair]
    rng = np.random.default_rng(7400 + 10 * pair + LOW_RINGS.index(cap))
    sb, eb = to_bits(start), to_bits(end)
    pieces = [sb, eb, sb[:-1], eb[1:], "0", "1", "01", sb[:8], eb[-8:]]
    streams = []
    for _ in range(64):
        n = int(rng.integers(200, 1501))
        out, total = [], 0
        while total < n:
            out.append(pieces[int(rng.integers(len(pieces)))])
            total += len(out[-1])
        streams.append("".join(out)[:n])
    calls = make_calls(rng, streams, 40, tsc_fail=0.05, max_prefix=24)
    sched = [(start, end)] * 40
    want, _ = ref_calls(calls, sched, cap)
    frames = sum(bool(w[0]) for res in want for w in res)
    _low[key] = (calls, sched, want, frames)
    return _low[key]


def test_host_framer_low_entropy_streams():
    total = pushes = 0
    for pair in range(len(LOW_ENTROPY)):
        for cap in LOW_RINGS:
            calls, sched, want, frames = low_entropy_case(pair, cap)
            assert frames >= 20, (LOW_ENTROPY[pair], cap, frames)
            total += frames
            fr = Q.Framer(64, *LOW_ENTROPY[pair], ring_capacity=cap)
            for ci, rows in enumerate(calls):
                bits, nb, off = pack_rows(rows)
                got = fr.push(bits, nb, off, payload_cap=4096)
                assert got == [w[0] for w in want[ci]], (LOW_ENTROPY[pair], cap, ci)
                pushes += len(rows)
    assert pushes == 53760 and total >= 4000, (pushes, total)


@pytest.mark.gpu
@pytest.mark.parametrize("cap", LOW_RINGS)
@pytest.mark.parametrize("pair", range(len(LOW_ENTROPY)), ids=[f"{s.hex()}-{e.hex()}" for s, e in LOW_ENTROPY])
def test_device_framer_low_entropy_streams(dev, pair, cap):
    """status() after every call: a frame that closes with an empty payload
    returns the same as "no frame", so only the state shows such a close."""
    calls, sched, want, frames = low_entropy_case(pair, cap)
    assert frames >= 20
    device_matches(dev, calls, sched, cap, want)
