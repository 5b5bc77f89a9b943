"""What the GPU tests share: the GPU requirement, the per-format facts, call
builders, one oracle runner, one host and one device runner over a handle,
the matched-filter reference and the comparisons.

Results have one shape everywhere: per call a list over streams of
(bits as a '0'/'1' string, rotated symbols as interleaved float32); bits are
"" for deModulateConstellation calls, symbols None where no rows were asked for.

Importing this module needs no GPU (the non-GPU tests of the call sequences
use it too); only need_gpu and its fixtures ask for one.
"""
import collections
import functools

import numpy as np
import pytest

import common as K
import oracle as O
import qpsk_amd

SYM_TOL = 1e-5   # constellation tolerance vs the libm-trig oracle
DEMODULATE = qpsk_amd.MODE_DEMODULATE


# ---------------------------------------------------------------------------
# the GPU requirement
# ---------------------------------------------------------------------------
def need_gpu(torch=False):
    """Fail the test without an MI355X; the binding, or torch where asked."""
    import torch as T
    if not T.cuda.is_available():
        pytest.fail("gpu tests need an MI355X")
    return T if torch else qpsk_amd


@pytest.fixture(scope="module")
def Q():
    """The binding and a device."""
    return need_gpu()


@pytest.fixture(scope="module")
def dev():
    """torch and a device."""
    torch = need_gpu(torch=True)
    torch.cuda.init()
    return torch


# ---------------------------------------------------------------------------
# per-format facts
# ---------------------------------------------------------------------------
# zero:      the stored value of sample 0 (a sample's value is float32(x - zero) * scale)
# scale:     the default; odd_scale: no power of two, so the multiply rounds
# amplitude: what quantised() scales a signal's peak to (half of full scale)
# extremes:  smallest and largest sample, placed at the head of random rows
# draw:      the type random rows are drawn in (CS8 rows are CU8's bytes)
# per_load:  samples in one 16-byte load
# layouts:   device rows as (lead, residue) in samples: a row starts `lead`
#            samples into its allocation and the pitch is `residue` mod per_load,
#            so device_rows asserts data_ptr % 16 == lead * bytes per sample and
#            stride % (2 per_load) == 2 residue.  "vector" rows take the 16-byte
#            loads, "half" rows (8-bit only) the 8-byte loads where T - 1 = 4 mod
#            8, "scalar" rows one load per sample.
# family:    the entry points the format suite reaches the format through: "cs16"
#            (process_cs16, set_cs16_scale, HostRing(fmt="cs16")) or "fmt"
#            (process_fmt, set_input_scale, HostRing.create_fmt)
Format = collections.namedtuple("Format", "np_dtype torch_dtype zero scale odd_scale amplitude extremes draw "
                                          "per_load layouts family")
_f32 = np.float32
_BYTE = dict(scale=_f32(1.0) / _f32(128), odd_scale=_f32(1 / 100), amplitude=64, extremes=(-128, 127), draw=np.uint8,
             per_load=8, layouts={"vector": (0, 0), "half": (4, 4), "scalar": (1, 1)}, family="fmt")
FORMATS = {
    "cf32": Format(np.float32, "float32", 0, None, None, None, None, None, 2, {}, None),
    "cs16": Format(np.int16, "int16", 0, _f32(1.0) / _f32(32768), _f32(1 / 20000), 16384, (-32768, 32767), np.int16,
                   4, {"vector": (0, 0), "scalar": (1, 1)}, "cs16"),
    "cs8": Format(np.int8, "int8", 0, **_BYTE),
    "cu8": Format(np.uint8, "uint8", 128, **_BYTE),
}


def widened(x, fmt, scale=None):
    """The value the library gives integer samples: an exact integer, one multiply."""
    F = FORMATS[fmt]
    assert x.dtype == F.np_dtype
    w = (x.astype(np.int32) - F.zero).astype(np.float32) * np.float32(F.scale if scale is None else scale)
    assert w.dtype == np.float32
    return w


def as_fmt(v, fmt):
    """int8 sample values as rows of fmt with the same value at its default
    scale (CS16: v * 256 / 32768 = v / 128 exactly)."""
    assert v.dtype == np.int8
    if fmt == "cf32":
        return widened(v, "cs8")
    if fmt == "cs16":
        return v.astype(np.int16) * np.int16(256)
    return v if fmt == "cs8" else (v.astype(np.int16) + 128).astype(np.uint8)


def quantised(base, fmt):
    """Float rows scaled to the format's amplitude (half of full scale) and rounded."""
    if fmt == "cu8":
        return as_fmt(quantised(base, "cs8"), "cu8")
    F = FORMATS[fmt]
    q = np.round(base * (float(F.amplitude) / np.abs(base).max())).astype(F.np_dtype)
    assert np.abs(q.astype(np.int32)).max() == F.amplitude
    return q


@functools.lru_cache(maxsize=None)
def signal_q(sps, span, S, fmt, n_bits=1600, seed0=0, cfo_hz=0.0):
    """K.batch_signals rows quantised to fmt.  Past 5 streams the rows are the
    first 5 rotated in time (still QPSK, all different)."""
    base = K.batch_signals(min(S, 5), seed0=seed0, sps=sps, span=span, n_bits=n_bits, snr_db=18, cfo_hz=cfo_hz)
    q = quantised(base, fmt)
    out = np.stack([q[s] if s < 5 else np.roll(q[s % 5], 2 * 37 * s) for s in range(S)])
    out.setflags(write=False)
    return out


def random_rows(S, n, seed, fmt):
    """Uniform over the format's whole range; the extremes, 0 and +-1 lead each row."""
    F = FORMATS[fmt]
    info = np.iinfo(F.draw)
    x = np.random.default_rng(seed).integers(info.min, info.max + 1, (S, 2 * n), dtype=F.draw).view(F.np_dtype)
    lo, hi = F.extremes
    head = (np.array([lo, hi, 0, 0, 1, -1, -1, 1, lo, lo], np.int32) + F.zero).astype(F.np_dtype)
    k = min(head.size, x.shape[1])
    x[:, :k] = head[:k]
    return x


def device_rows(S, n_cap, layout, fmt):
    """A device view of S rows of fmt holding n_cap samples each, in one of
    the format's layouts (FORMATS)."""
    import torch
    F = FORMATS[fmt]
    lead, res = F.layouts[layout]
    pitch = n_cap + lead
    pitch += (res - pitch) % F.per_load   # samples per row = res mod per_load
    v = torch.zeros((S, 2 * pitch), dtype=getattr(torch, F.torch_dtype), device="cuda")[:, 2 * lead: 2 * (lead + n_cap)]
    assert v.data_ptr() % 16 == lead * (16 // F.per_load) and v.stride(0) % (2 * F.per_load) == 2 * res
    return v


def entry(b, kind, fmt, family=None):
    """b's process, process_device or process_device_async for rows of fmt: the
    float entry point, the _cs16 one or the format-tagged one."""
    if fmt == "cf32":
        return getattr(b, kind)
    if (family or FORMATS[fmt].family) == "cs16":
        assert fmt == "cs16"
        return getattr(b, kind + "_cs16")
    return functools.partial(getattr(b, kind + "_fmt"), fmt=fmt)


def set_scale(b, fmt, scale, family=None):
    if (family or FORMATS[fmt].family) == "cs16":
        b.set_cs16_scale(scale)
    else:
        b.set_input_scale(fmt, scale)


# ---------------------------------------------------------------------------
# call builders
# ---------------------------------------------------------------------------
def call_rows(x, lens, pos):
    """The [S, 2 max(lens)] rows of one call whose stream s takes lens[s]
    samples of x[s] from pos[s] on, zero behind each stream's length."""
    S, n = x.shape[0], int(max(lens))
    rows = np.zeros((S, 2 * max(n, 1)), x.dtype)
    for s in range(S):
        rows[s, : 2 * lens[s]] = x[s, 2 * pos[s]: 2 * (pos[s] + lens[s])]
    return rows[:, : 2 * n]


def lengths_of(lens):
    """None for a uniform call, else the per-stream lengths."""
    return None if all(l == lens[0] for l in lens) else np.array(lens, np.int64)


def decoded(mode, bits, nb, syms, ns, rows=None):
    """One call's outputs as [(bits, symbols)] over rows (default: all)."""
    return [(qpsk_amd.unpack_bits(bits[s], int(nb[s])) if mode == DEMODULATE else "",
             None if syms is None else syms[s, : 2 * int(ns[s])].copy())
            for s in (range(len(nb)) if rows is None else rows)]


def make(S, sps, span, n_max, **knobs):
    return qpsk_amd.BatchDemodulator(S, qpsk_amd.params(K.FS, K.FS // sps, K.ALPHA, span, max_samples_per_call=n_max,
                                                        **knobs))


def split_calls(S, n, k, seed, ragged=True):
    """k + 1 calls that use up n samples of every stream; ragged ones carry
    per-stream lengths and leave one stream empty."""
    rng = np.random.default_rng(seed)
    calls, used = [], np.zeros(S, np.int64)
    for c in range(k):
        lens = rng.integers(0, n // (k + 1), S) if (ragged and c % 2) else np.full(S, n // (k + 2))
        if ragged and c % 2:
            lens[c % S] = 0
        calls.append([int(v) for v in lens])
        used += lens
    calls.append([int(n - u) for u in used])
    return calls


# (sps, span) -> T = sps * span + 1: one pair per tile-kernel instantiation of
# launch_fir (qpsk_kernels.hip); tests/test_gpu_fir.py keeps the two lists equal
SPECIALISED = [(2, 6), (2, 8), (2, 10), (4, 8), (4, 10), (4, 12), (8, 8), (8, 12), (4, 32)]
TILE = 2048   # outputs per workgroup of fir_tile_kernel (256 threads x 8)


def _ids(pairs):
    return [f"T{s * p + 1}" for s, p in pairs]


def ragged_calls(T, S=6):
    """Per-call [S] lengths: stream s takes 1, T-2, T-1, T, 2047, 2048, 2049, 0,
    4097 samples in that order, started s places in (so stream 0 builds its
    history from calls shorter than T-1, and every stream reaches and crosses
    the 2048-output tile edge with both parities of n).  A call in which the
    rotation leaves no stream empty gets one: stream (call % S) sits that call
    out and takes its length in the next one."""
    base = [1, T - 2, T - 1, T, TILE - 1, TILE, TILE + 1, 0, 2 * TILE + 1]
    todo = [base[s:] + base[:s] for s in range(S)]
    calls = []
    while any(todo):
        lens = [q[0] if q else 0 for q in todo]
        if 0 not in lens:
            lens[len(calls) % S] = 0
        for s in range(S):
            if todo[s] and lens[s] == todo[s][0]:
                todo[s].pop(0)
        calls.append(lens)
    return calls


def ragged_loop_calls(S, n, seed, big=4096):
    """Per-stream call sizes for the symbol loop: 0, 1, 2 and 3 samples, calls
    longer than a round, and a different size per stream in every call, so
    streams end in different rounds (the loader's slow path) with odd and even
    carries; n samples a stream in all.  big: the longest of the first nine
    sizes (rows much shorter than it would end in that call)."""
    rng = np.random.default_rng(seed)
    sizes = [1, 2, 3, 0, 777, 5, big, 130, 63]
    calls, left, k = [], np.full(S, n), 0
    while left.max() > 0:
        c = [int(min(left[s], sizes[(k + s) % len(sizes)] if k < 9 else rng.integers(100, 3000)))
             for s in range(S)]
        calls.append(c)
        left -= np.array(c)
        k += 1
    return calls


def calls_for(T, S=6):
    """ragged_calls(T), then five calls in which every stream takes 2050 ... 2054
    samples once (row ends at 2 ... 6 mod 8)."""
    calls = [list(c) for c in ragged_calls(T, S)]
    for k in range(5):
        calls.append([TILE + 2 + (k + s) % 5 for s in range(S)])
    return calls


# ---------------------------------------------------------------------------
# the oracle over a call sequence
# ---------------------------------------------------------------------------
def oracle_run(iq, calls, rs, span, mode=None, after_call=None, state0=None, **okw):
    """Per-stream OracleDemod instances (symbol rate rs in Hz, keywords okw) fed
    the same call sequence.  calls: per-call [S] lengths in complex samples;
    mode per call; after_call(ci, instances) runs behind every call.  state0:
    per stream a dict of loop fields (OracleDemod.write_state) set before the
    first call."""
    S = iq.shape[0]
    dms = [O.OracleDemod(K.FS, rs, K.ALPHA, span, **okw) for _ in range(S)]
    for dm, st in zip(dms, state0 or ()):
        if st:
            dm.write_state(**st)
    pos = np.zeros(S, dtype=np.int64)
    out = []
    for ci, lens in enumerate(calls):
        res = []
        for s, dm in enumerate(dms):
            x = iq[s, 2 * pos[s]: 2 * (pos[s] + lens[s])]
            if mode is None or mode[ci] == DEMODULATE:
                bits, syms, _ = dm.demodulate_ex(x)
                res.append((bits, syms))
            else:
                res.append(("", dm.deModulateConstellation(x)))
            pos[s] += lens[s]
        out.append(res)
        if after_call:
            after_call(ci, dms)
    return out


# ---------------------------------------------------------------------------
# calls on a handle
# ---------------------------------------------------------------------------
def host_call(b, rows, lengths, mode=DEMODULATE, fmt="cf32", family=None, want_syms=True):
    """One host-memory call of rows in fmt on b; lengths goes to the call as it
    is (None: every stream takes the whole row).  Returns decoded()'s rows."""
    bits, nb, syms, ns = entry(b, "process", fmt, family)(rows, mode=mode, lengths=lengths, want_syms=want_syms)
    return decoded(mode, bits, nb, syms if want_syms else None, ns)


def host_calls(b, x, calls, fmt="cf32", family=None, mode=None, always_lengths=False):
    """The call sequence in host-memory calls on b, with symbol rows.  A uniform
    call passes lengths=None unless always_lengths.  Returns per call the
    decoded rows and last_mf (None after a chunked call)."""
    pos = np.zeros(x.shape[0], np.int64)
    out, mfs = [], []
    for ci, lens in enumerate(calls):
        rows = call_rows(x, lens, pos)
        n = rows.shape[1] // 2
        out.append(host_call(b, rows, np.array(lens, np.int64) if always_lengths else lengths_of(lens),
                             mode[ci] if mode else DEMODULATE, fmt, family))
        mfs.append(b.last_mf(n).copy() if n <= b.p.max_samples_per_call else None)
        pos += np.array(lens)
    return out, mfs


def gpu_run(iq, calls, rs, span, mode=None, want_syms=True, max_samples=None, **knobs):
    """A fresh handle (symbol rate rs in Hz; max_samples: the internal chunk
    size, default the longest call + 8) over the float call sequence; the
    decoded rows per call.  want_syms=False runs the bits-only kernel; its
    rows carry None for symbols."""
    chunk = max_samples or max(max(c) for c in calls) + 8
    b = qpsk_amd.BatchDemodulator(iq.shape[0], qpsk_amd.params(K.FS, rs, K.ALPHA, span, max_samples_per_call=chunk,
                                                                 **knobs))
    pos = np.zeros(iq.shape[0], np.int64)
    out = []
    try:
        for ci, lens in enumerate(calls):
            out.append(host_call(b, call_rows(iq, lens, pos), lengths_of(lens), mode[ci] if mode else DEMODULATE,
                                 want_syms=want_syms))
            pos += np.array(lens)
    finally:
        b.close()
    return out


def device_calls(b, x, calls, fmt, family=None, layout="vector", pipelined=False, mode=None, scales=None):
    """The call sequence in device-memory calls on b (synchronous, or pipelined
    with one wait at the end), rows of fmt in one of its layouts, each call's
    outputs in rows of its own.  scales[ci]: set before call ci.  Returns per
    call the decoded rows and, for synchronous unchunked calls, last_mf."""
    import torch
    S = x.shape[0]
    nmax = max(max(c) for c in calls)
    ms = max(b.max_symbols(nmax), 1)
    pos = np.zeros(S, np.int64)
    outs, mfs = [], []
    for ci, lens in enumerate(calls):
        m = mode[ci] if mode else DEMODULATE
        rows = call_rows(x, lens, pos)
        n = rows.shape[1] // 2
        xd = device_rows(S, max(n, 1), layout, fmt)
        if n:
            xd[:, : 2 * n].copy_(torch.from_numpy(np.ascontiguousarray(rows)))
        bits = torch.zeros((S, ((2 * ms + 7) // 8 + 63) // 64 * 64), dtype=torch.uint8, device="cuda")
        sy = torch.zeros((S, 2 * ms), dtype=torch.float32, device="cuda")
        nb = torch.zeros(S, dtype=torch.int64, device="cuda")
        ns = torch.zeros(S, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        if scales and scales[ci] is not None:
            set_scale(b, fmt, scales[ci], family)
        call = entry(b, "process_device_async" if pipelined else "process_device", fmt, family)
        call(xd, n, bits if m == DEMODULATE else None, nb if m == DEMODULATE else None, mode=m,
             syms_dev=sy, n_syms_dev=ns, lengths=lengths_of(lens))
        if not pipelined and n <= b.p.max_samples_per_call:   # not after a chunked call
            mfs.append(b.last_mf(n).copy())
        outs.append((m, xd, bits, nb, sy, ns))
        pos += np.array(lens)
    if pipelined:
        b.pipeline_wait()
    torch.cuda.synchronize()
    return [decoded(m, bits.cpu().numpy(), nb.cpu().numpy(), sy.cpu().numpy(), ns.cpu().numpy())
            for m, _, bits, nb, sy, ns in outs], mfs


def out_rows(S, ms, layout):
    """Device output rows.  "direct": word-aligned rows the loop kernel writes
    in place; "staged": a 1-byte-offset bit row of odd stride and an odd
    symbol stride, which take the staging buffers and the 2-D copies."""
    import torch
    if layout == "staged":
        bw = (2 * ms + 7) // 8 + 9
        bw += 1 - bw % 2
        bits = torch.zeros((S, bw + 1), dtype=torch.uint8, device="cuda")[:, 1:]
        sy = torch.zeros((S, 2 * ms + 1), dtype=torch.float32, device="cuda")
    else:
        bits = torch.zeros((S, ((2 * ms + 7) // 8 + 63) // 64 * 64), dtype=torch.uint8, device="cuda")
        sy = torch.zeros((S, 2 * ms), dtype=torch.float32, device="cuda")
    return bits, sy


def async_run(iq, calls, sps, span, sync_every=0, layout=None, prepare=None, finish=None, want_syms=True,
              max_samples=None, close_unwaited=False, **knobs):
    """The float call sequence through process_device_async on a torch stream of
    its own (front stage of call k+1 overlapping the back stage of call k),
    every call's outputs in their own device rows, one pipeline_wait at the
    end.  sync_every > 0 makes every sync_every-th call a synchronous
    process_device (mixed ordering).  layout: None (rows as a caller would size
    them), or out_rows' layouts.  prepare(b) runs on the new handle before the
    first call (a state to restore), finish(b) after the wait, before the
    handle is closed.  want_syms=False passes no symbol rows (the bits-only
    kernel); the rows then carry None for symbols.  max_samples: the internal
    chunk size (default the longest call + 8).  close_unwaited: the handle is
    closed with the calls still queued, no pipeline_wait, and the rows are read
    after that (finish does not run).  Returns the decoded rows and pipeline_depth."""
    import torch
    S = iq.shape[0]
    nmax = max(max(c) for c in calls)
    b = make(S, sps, span, max_samples or nmax + 8, **knobs)
    if prepare:
        prepare(b)
    stream = torch.cuda.Stream()
    b.set_stream(stream.cuda_stream)
    ms = max(b.max_symbols(nmax), 1)
    pos = np.zeros(S, dtype=np.int64)
    outs = []
    with torch.cuda.stream(stream):
        for ci, lens in enumerate(calls):
            n = int(max(lens))
            x = np.zeros((S, 2 * max(n, 1)), np.float32)
            x[:, : 2 * n] = call_rows(iq, lens, pos)
            xd = torch.from_numpy(x).to("cuda", non_blocking=False)
            if layout:
                bits, sy = out_rows(S, ms, layout)
            else:
                bits = torch.zeros((S, (2 * ms + 7) // 8 + 8), dtype=torch.uint8, device="cuda")
                sy = torch.zeros((S, 2 * ms), dtype=torch.float32, device="cuda")
            nb = torch.zeros(S, dtype=torch.int64, device="cuda")
            ns = torch.zeros(S, dtype=torch.int64, device="cuda")
            out = dict(syms_dev=sy, n_syms_dev=ns) if want_syms else {}
            if sync_every and ci % sync_every == sync_every - 1:
                assert lengths_of(lens) is None
                b.process_device(xd, n, bits, nb, **out)
            else:
                b.process_device_async(xd, n, bits, nb, lengths=lengths_of(lens), **out)
            outs.append((xd, bits, nb, sy, ns))
            pos += np.array(lens)
    depth = b.pipeline_depth()
    if close_unwaited:
        b.close()
    else:
        b.pipeline_wait()
    torch.cuda.synchronize()
    res = [decoded(DEMODULATE, bits.cpu().numpy(), nb.cpu().numpy(), sy.cpu().numpy() if want_syms else None,
                   ns.cpu().numpy())
           for _, bits, nb, sy, ns in outs]
    if finish and not close_unwaited:
        finish(b)
    b.close()
    return res, depth


# ---------------------------------------------------------------------------
# the matched-filter reference
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rrc(sps, span):
    """The reference's float32 RRC taps for (K.FS, K.FS // sps, K.ALPHA, span)."""
    h = K.oracle_for(sps, span).rrc_f32()
    h.setflags(write=False)
    return h


def fir_ref(h, row, lanes=8):
    """One streaming reference filter over a whole interleaved row."""
    tiq = np.zeros(2 * h.size, np.float32)
    tiq[0::2] = h
    return O.oracle_fir(tiq, row, lanes=lanes)


def is_neg_zero(v):
    return np.signbit(v) & (v == 0)


def assert_rows(mfs, calls, refs):
    """Each call's last_mf rows against refs[s], the reference filter's output
    over stream s's whole input: bit for bit, and no -0."""
    pos = np.zeros(len(refs), np.int64)
    for ci, (mf, lens) in enumerate(zip(mfs, calls)):
        for s, n in enumerate(lens):
            got, want = mf[s, : 2 * n], refs[s][2 * pos[s]: 2 * (pos[s] + n)]
            if not K.bitwise_equal(got, want):
                bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
                pytest.fail(f"call {ci} stream {s} (n = {n}): {bad.size} floats differ, first at output "
                            f"{bad[0] // 2}: {got[bad[0]]!r} vs {want[bad[0]]!r}")
            assert not is_neg_zero(got).any(), f"call {ci} stream {s}: -0 in the matched filter"
            pos[s] += n


# ---------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------
def same_bits(a, b, dtype, nan_any_payload=False):
    return K.bitwise_equal(np.asarray(a, dtype=dtype).reshape(-1), np.asarray(b, dtype=dtype).reshape(-1),
                           nan_any_payload=nan_any_payload)


def assert_state(blob, ostates, sps, span, what, rows=None, nan_rows=(), taps=None):
    """A state blob (qpsk_demod_get_state) against ostates[s] = the oracle's
    read_state() of stream s, field by field as bit patterns: the record, the
    carry, the filter history and the FLL delay line.  rows: the streams to
    compare (default: all); nan_rows: streams whose floats compare under the
    NaN rule (NaN where the reference has NaN, payloads aside); taps: the
    filter's length where it is not sps * span + 1 (a non-integer sps)."""
    S, T = len(ostates), taps or sps * span + 1
    rec, carry, hist, dl = qpsk_amd.state_blob_parts(blob, S, T)
    f4, f8 = np.float32, np.float64
    for s in (range(S) if rows is None else rows):
        o, r, nan_ok = ostates[s], rec[s], s in nan_rows
        ints = [("base", o["mm_base_index"]), ("has_prev", o["mm_has_prev"]), ("carry_n", o["mm_buf_count"]),
                ("diff_have", o["diff_have_prev"]), ("fll_pos", o["fll_pos"]), ("error", 0), ("tofs", 0)]
        for name, want in ints:
            assert int(r[name]) == int(want), f"{what} stream {s}: {name} {int(r[name])} vs {int(want)}"
        floats = [("mu", o["mm_mu"], f8), ("integ", o["mm_nco_integral"], f8),
                  ("theta", o["costas_theta"], f8), ("freq", o["costas_freq"], f8),
                  ("psi", o["mm_prev_sample"][0], f4), ("psq", o["mm_prev_sample"][1], f4),
                  ("pdi", o["mm_prev_decision"][0], f4), ("pdq", o["mm_prev_decision"][1], f4),
                  ("diff_pi", o["diff_prev"][0], f4), ("diff_pq", o["diff_prev"][1], f4),
                  ("fll_phase", o["fll_phase"], f4), ("fll_freq", o["fll_freq"], f4),
                  ("iqb_re", o["iqb_avg_real"], f4), ("iqb_im", o["iqb_avg_img"], f4)]
        for name, want, dt in floats:
            assert same_bits(r[name], want, dt, nan_ok), f"{what} stream {s}: {name} {r[name]!r} vs {want!r}"
        k = int(r["carry_n"])
        assert same_bits(carry[s, :k], o["mm_queue"], f4), f"{what} stream {s}: carry ({k} samples)"
        # the history, oldest first = the reference's delay line read from T - 1
        # writes back up to the newest one, at _pos - 1
        idx = (o["rrc_pos"] - (T - 1) + np.arange(T - 1)) % T
        if not same_bits(hist[s], o["rrc_delay"][idx], f4):
            bad = np.flatnonzero((hist[s].view(np.uint32) != o["rrc_delay"][idx].view(np.uint32)).any(axis=1))
            pytest.fail(f"{what} stream {s}: {bad.size} history samples differ, first at {bad[0]} of {T - 1}")
        assert same_bits(dl[s], o["fll_delay"], f4), f"{what} stream {s}: FLL delay line (pos {o['fll_pos']})"
        # and as the FLL reads it: the 39 samples before the write position
        pos = int(r["fll_pos"])
        back = (pos - 1 - np.arange(qpsk_amd.STATE_FLL_TAPS - 1)) % qpsk_amd.STATE_FLL_TAPS
        assert same_bits(dl[s][back], o["fll_delay"][(o["fll_pos"] - 1 - np.arange(39)) % 40], f4)


def assert_same(got, want, exact=True, what="", nan_rows=()):
    """Two results call by call and stream by stream: equal bits, the same
    symbol count, symbols bit for bit (exact) or within SYM_TOL; rows without
    symbols (None) compare their bits alone.  nan_rows: streams whose symbols
    compare under the NaN rule (NaN where want has NaN, payloads aside)."""
    assert len(got) == len(want)
    for ci, (ra, rb) in enumerate(zip(got, want)):
        for s, ((ba, sa), (bb, sb)) in enumerate(zip(ra, rb)):
            assert ba == bb, f"{what} call {ci} stream {s}: bits differ ({len(ba)} vs {len(bb)})"
            if sa is None or sb is None:
                continue
            assert sa.shape == sb.shape, f"{what} call {ci} stream {s}: symbol count"
            if exact:
                assert K.bitwise_equal(sa, sb, nan_any_payload=s in nan_rows), \
                    f"{what} call {ci} stream {s}: symbols differ (bitwise)"
            else:
                assert np.max(np.abs(sa - sb), initial=0) <= SYM_TOL
