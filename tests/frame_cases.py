"""What the frame tests share (tests/test_gpu_frames_pack.py,
tests/test_gpu_rx_frames.py): the testAtDataLevel signals, the oracle's
DeModulateBytes per stream and chunk, computed once per case and left
unchanged, and the packing rule of qpsk_frames_pack_device in numpy.

Importing this module needs no GPU.
"""
import functools

import numpy as np

import common as K
import oracle as O
from gpu_harness import quantised, widened
from refmodel import RefFramer

START, END = b"MESSAGE_START", b"MESSAGE_STOP"
NEVER = (b"\xF0\x0F\xAA\x55NEVER", b"\x01\x02NOPE")   # a marker pair that occurs in no signal here
SPS, SPAN = 8, 8
RS = K.FS // SPS


def tad_frames(seed, n_frames, tsc=K.TSC, sps=SPS, span=SPAN):
    """testAtDataLevel frames (TSC + MESSAGE_START/STOP around the payload text)
    through a seeded +-1 ppm LO pair (testAtDataLevel.cs:27-46)."""
    fs = K.FS
    rs = fs // sps
    tx = O.OracleNCO(100e6, fs, 1, 0, seed=seed)
    rx = O.OracleNCO(100e6, fs, 1, 0, seed=seed + 1)
    return np.concatenate([
        O.apply_lo_pair(tx, rx, O.modulate_text_utf8(fs, rs, K.PAYLOAD + str(i), "MESSAGE_START",
                                                     "MESSAGE_STOP", rrc_alpha=K.ALPHA,
                                                     rrc_span=span, tsc=tsc))
        for i in range(n_frames)])


@functools.lru_cache(maxsize=None)
def signals(S, n_frames, fmt="cf32"):
    """[S, 2n] rows: stream s is tad_frames(30 + 2s, n_frames), cut to the
    shortest; "cs8": quantised as gpu_harness.quantised does."""
    sigs = [tad_frames(30 + 2 * s, n_frames) for s in range(S)]
    n = min(x.size for x in sigs)
    x = np.stack([v[:n] for v in sigs]).astype(np.float32)
    if fmt != "cf32":
        x = quantised(x, fmt)
    x.setflags(write=False)
    return x


def chunk_starts(n, chunk):
    """The whole chunks of n samples."""
    return list(range(0, n - chunk + 1, chunk))


def oracle_input(rows, fmt):
    """What the oracle is fed for rows of fmt: the floats, or the widened integers."""
    return rows if fmt == "cf32" else widened(rows, fmt)


def oracle_frames(x, fmt, chunk, tsc, schedule=None, resets=None, track=False):
    """The oracle's DeModulateBytes per chunk and stream over the whole chunks
    of x: a list over chunks of lists over streams of bytes.  schedule[ci]: the
    marker pair of chunk ci (default START, END).  resets: {ci: streams}, the
    streams whose instance is constructed anew after chunk ci.  track: also
    the string model's framer (in_frame, ring bytes, carry bits) per chunk and
    stream, from a second instance's DeModulate bits."""
    S = x.shape[0]
    new = lambda: O.OracleDemod(K.FS, RS, K.ALPHA, SPAN, tsc=tsc)   # noqa: E731
    orc = [new() for _ in range(S)]
    bits = [new() for _ in range(S)] if track else None
    refs = [RefFramer() for _ in range(S)] if track else None
    out, states = [], []
    for ci, a in enumerate(chunk_starts(x.shape[1] // 2, chunk)):
        st, en = schedule[ci] if schedule else (START, END)
        xs = oracle_input(x[:, 2 * a: 2 * (a + chunk)], fmt)
        out.append([orc[s].DeModulateBytes(xs[s], st, en) for s in range(S)])
        if track:
            row = []
            for s in range(S):
                got = refs[s].push(bits[s].DeModulate(xs[s]), st, en)
                assert got == out[-1][s], "the string model left the oracle"
                row.append((refs[s].in_frame, len(refs[s].ring), len(refs[s].carry)))
            states.append(row)
        for s in (resets or {}).get(ci, ()):
            orc[s] = new()
            if track:
                bits[s], refs[s] = new(), RefFramer()
    return (out, states) if track else out


@functools.lru_cache(maxsize=None)
def tsc_case(S, n_frames, chunk, fmt):
    """(rows, oracle frames) of the cases with a TSC."""
    x = signals(S, n_frames, fmt)
    return x, oracle_frames(x, fmt, chunk, K.TSC)


@functools.lru_cache(maxsize=None)
def plain_case(chunk):
    """(rows, oracle frames, string-model states) of the TSC-less case: S = 5,
    10 frames, CF32; the frames straddle the chunks."""
    x = signals(5, 10)
    return (x,) + oracle_frames(x, "cf32", chunk, None, track=True)


def pack_rule(lengths, P, C):
    """The packing rule of qpsk_frames_pack_device in numpy: (k, a, offsets,
    total, flags) of n_payload = lengths for rows of P bytes and a capacity C."""
    L = np.asarray(lengths, dtype=np.int64)
    k = np.minimum(np.maximum(L, 0), P)
    a = (k + 15) // 16 * 16
    E = np.cumsum(a) - a
    stored = (k > 0) & (E + a <= C)
    offsets = np.where(stored, E, -1).astype(np.int64)
    total = int((E + a)[stored].max()) if stored.any() else 0
    flags = (1 if (L > P).any() else 0) | (2 if ((k > 0) & ~stored).any() else 0)
    return k, a, offsets, total, flags


def packed_bytes(rows, lengths, P, C):
    """packed[0:total] as the rule defines it: the stored frames' k bytes and
    the zeros behind them."""
    k, a, offsets, total, _ = pack_rule(lengths, P, C)
    out = np.zeros(total, dtype=np.uint8)
    for s in np.flatnonzero(offsets >= 0):
        out[offsets[s]: offsets[s] + k[s]] = rows[s, : k[s]]
    return out
