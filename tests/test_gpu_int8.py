"""CS8 (int8 I,Q) and CU8 (uint8 I,Q, zero at 128) input, bit for bit.

A sample's value is SoapySDR's: CS8 float32(x) * scale, CU8 float32(x - 128) *
scale; the integer is exact in float and the multiply is one IEEE rounding,
which numpy reproduces (`widened`).  So the reference of every check here is
the CPU oracle fed those floats, at tolerance 0: matched-filter rows
(qpsk_demod_last_mf against O.oracle_fir), bits and rotated symbols (against
OracleDemod).

Stagings of the tile kernel.  One 16-byte load holds 8 samples; rows that are
16-byte aligned with a stride of a multiple of 8 samples take it (for T = 13
and 21, where T - 1 = 4 mod 8, 8-byte loads of 4 samples from 8-byte alignment
on).  Host-memory calls stage rows pitched to 8 samples, so they take it
whatever max_samples_per_call is; device rows that are 2-byte aligned only take
one 2-byte load per sample.  With 8-sample loads every residue of a row's
length mod 8 must end a row: ragged_calls gives 0, 1 and 7, `calls_for` adds
calls of 2050 ... 2054 samples for 2 ... 6.
"""
import contextlib
import functools

import numpy as np
import pytest

import common as K
import oracle as O
from test_gpu_cs16 import assert_same, call_rows, lengths_of, make, oracle_chain, split_calls
from test_gpu_fir import SPECIALISED, TILE, _ids, assert_rows, fir_ref, ragged_calls, rrc

pytestmark = pytest.mark.gpu

DEFAULT_SCALE = np.float32(1.0) / np.float32(128)
ODD_SCALE = np.float32(1 / 100)   # no power of two: the multiply rounds
DTYPE = {"cs8": np.int8, "cu8": np.uint8, "cs16": np.int16, "cf32": np.float32}
FMTS = ["cs8", "cu8"]


@pytest.fixture(scope="module")
def Q():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need an MI355X")
    import qpsk_amd
    return qpsk_amd


# ---------------------------------------------------------------------------
# inputs and references
# ---------------------------------------------------------------------------
def widened(x, fmt, scale=DEFAULT_SCALE):
    """The value the library gives 8-bit samples: an exact integer, one multiply."""
    assert x.dtype == DTYPE[fmt]
    if fmt == "cs8":
        w = x.astype(np.float32) * np.float32(scale)
    else:
        w = (x.astype(np.int16) - 128).astype(np.float32) * np.float32(scale)
    assert w.dtype == np.float32
    return w


def as_fmt(v, fmt):
    """int8 sample values as rows of fmt carrying the same samples."""
    assert v.dtype == np.int8
    return v if fmt == "cs8" else (v.astype(np.int16) + 128).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def signal_i8(sps, span, S, n_bits=1600, seed0=0, cfo_hz=0.0):
    """K.batch_signals rows quantised to +-64 (half of full scale), as int8
    values.  Past 5 streams the rows are the first 5 rotated in time."""
    base = K.batch_signals(min(S, 5), seed0=seed0, sps=sps, span=span, n_bits=n_bits, snr_db=18, cfo_hz=cfo_hz)
    q = np.round(base * (64.0 / np.abs(base).max())).astype(np.int8)
    rows = [q[s] if s < 5 else np.roll(q[s % 5], 2 * 37 * s) for s in range(S)]
    out = np.stack(rows)
    assert np.abs(out.astype(np.int16)).max() == 64
    out.setflags(write=False)
    return out


def random_bytes(S, n, seed, fmt):
    """Uniform over all 256 values; the extremes, zero and +-1 lead each row."""
    x = np.random.default_rng(seed).integers(0, 256, (S, 2 * n), dtype=np.uint8)
    head = np.array([-128, 127, 0, 0, 1, -1, -1, 1, -128, -128], np.int8)
    k = min(head.size, x.shape[1])
    if fmt == "cs8":
        x = x.view(np.int8)
        x[:, :k] = head[:k]
    else:
        x[:, :k] = as_fmt(head, "cu8")[:k]    # 0, 255, 128, 128, 129, 127, 127, 129, 0, 0
    return x


def calls_for(T, S=6):
    """ragged_calls(T), then five calls in which every stream takes 2050 ... 2054
    samples once (row ends at 2 ... 6 mod 8)."""
    calls = [list(c) for c in ragged_calls(T, S)]
    for k in range(5):
        calls.append([TILE + 2 + (k + s) % 5 for s in range(S)])
    return calls


def run_call(Q, b, fmt, rows, m, lens):
    """One host call of rows in fmt on handle b."""
    if fmt == "cf32":
        return b.process(rows, mode=m, lengths=lengths_of(lens), want_syms=True)
    return b.process_fmt(rows, fmt, mode=m, lengths=lengths_of(lens), want_syms=True)


def decoded(Q, m, bits, nb, syms, ns, S):
    return [(Q.unpack_bits(bits[s], int(nb[s])) if m == Q.MODE_DEMODULATE else "",
             syms[s, : 2 * int(ns[s])].copy()) for s in range(S)]


def host_calls(Q, b, x, calls, fmt, mode=None):
    """Host-memory calls on handle b; per call the decoded rows and last_mf."""
    S = x.shape[0]
    pos = np.zeros(S, np.int64)
    out, mfs = [], []
    for ci, lens in enumerate(calls):
        m = mode[ci] if mode else Q.MODE_DEMODULATE
        rows, n = call_rows(x, calls, ci, pos, x.dtype)
        bits, nb, syms, ns = run_call(Q, b, fmt, rows, m, lens)
        out.append(decoded(Q, m, bits, nb, syms, ns, S))
        mfs.append(b.last_mf(n).copy() if n <= b.p.max_samples_per_call else None)   # not after a chunked call
        pos += np.array(lens)
    return out, mfs


def device_rows(S, n_cap, layout, dtype):
    """A byte device view of S rows holding n_cap samples each.
    'vector': 16-byte aligned rows, stride_elems % 16 == 0.
    'half':   rows 4 samples in (8-byte, not 16-byte aligned), stride_elems = 8 mod 16.
    'scalar': rows one sample in (2-byte aligned only), stride_elems = 2 mod 16."""
    import torch
    td = torch.int8 if dtype == np.int8 else torch.uint8
    lead, res = {"vector": (0, 0), "half": (4, 4), "scalar": (1, 1)}[layout]
    pitch = n_cap + lead
    pitch += (res - pitch) % 8            # samples per row = res mod 8
    v = torch.zeros((S, 2 * pitch), dtype=td, device="cuda")[:, 2 * lead: 2 * (lead + n_cap)]
    assert v.data_ptr() % 16 == 2 * lead and v.stride(0) % 16 == 2 * res
    return v


def device_calls(Q, b, x, calls, fmt, layout="vector", pipelined=False, mode=None, scales=None):
    """Device-memory calls (synchronous, or pipelined with one wait at the
    end), each call's outputs in rows of its own.  scales[ci]: set before call ci."""
    import torch
    S = x.shape[0]
    nmax = max(max(c) for c in calls)
    ms = max(b.max_symbols(nmax), 1)
    pos = np.zeros(S, np.int64)
    outs, mfs = [], []
    for ci, lens in enumerate(calls):
        m = mode[ci] if mode else Q.MODE_DEMODULATE
        rows, n = call_rows(x, calls, ci, pos, x.dtype)
        xd = device_rows(S, max(n, 1), layout, x.dtype)
        if n:
            xd[:, : 2 * n].copy_(torch.from_numpy(np.ascontiguousarray(rows)))
        bits = torch.zeros((S, ((2 * ms + 7) // 8 + 63) // 64 * 64), dtype=torch.uint8, device="cuda")
        sy = torch.zeros((S, 2 * ms), dtype=torch.float32, device="cuda")
        nb = torch.zeros(S, dtype=torch.int64, device="cuda")
        ns = torch.zeros(S, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        if scales and scales[ci] is not None:
            b.set_input_scale(fmt, scales[ci])
        call = b.process_device_async_fmt if pipelined else b.process_device_fmt
        call(xd, n, bits if m == Q.MODE_DEMODULATE else None, nb if m == Q.MODE_DEMODULATE else None, fmt, mode=m,
             syms_dev=sy, n_syms_dev=ns, lengths=lengths_of(lens))
        if not pipelined and n <= b.p.max_samples_per_call:   # not after a chunked call
            mfs.append(b.last_mf(n).copy())
        outs.append((m, xd, bits, nb, sy, ns))
        pos += np.array(lens)
    if pipelined:
        b.pipeline_wait()
    torch.cuda.synchronize()
    res = []
    for m, _, bits, nb, sy, ns in outs:
        res.append(decoded(Q, m, bits.cpu().numpy(), nb.cpu().numpy(), sy.cpu().numpy(), ns.cpu().numpy(), S))
    return res, mfs


# ---------------------------------------------------------------------------
# 1. every value
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def every_pair():
    """One row of 65 536 samples: every (I, Q) byte pair once, shuffled."""
    k = np.random.default_rng(8000).permutation(65536).astype(np.uint32)
    row = np.stack([(k >> 8).astype(np.uint8), (k & 255).astype(np.uint8)], 1).reshape(1, -1)
    assert len({(int(a), int(c)) for a, c in row.reshape(-1, 2)}) == 65536
    row.setflags(write=False)
    return row


@pytest.mark.parametrize("scale", [None, ODD_SCALE], ids=["default-scale", "scale-1/100"])
@pytest.mark.parametrize("fmt", FMTS)
def test_every_byte_pair_bitwise(Q, fmt, scale):
    """The input domain is finite: all 65 536 (I, Q) pairs through the T = 65
    tile kernel, against fir_ref of the numpy-widened row."""
    sps, span, n = 8, 8, 65536
    x = every_pair().view(DTYPE[fmt])
    b = make(Q, 1, sps, span, n)
    if scale is not None:
        b.set_input_scale(fmt, scale)
    b.process_fmt(x, fmt)
    mf = b.last_mf(n)
    assert b.status() == 0
    b.close()
    ref = fir_ref(rrc(sps, span), widened(x, fmt, DEFAULT_SCALE if scale is None else scale)[0])
    assert K.bitwise_equal(mf[0], ref)


# ---------------------------------------------------------------------------
# 2. matched-filter rows
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stage_inputs(sps, span, fmt, lanes=8, seed=0, scale=None):
    """(rows, calls, per-stream reference rows): 6 rows, 4 of random bytes and
    2 of quantised signal, over calls_for(T)."""
    T = sps * span + 1
    calls = calls_for(T)
    total = sum(c[0] for c in calls)
    assert all(sum(c[s] for c in calls) == total for s in range(6))
    x = random_bytes(6, total, seed + T, fmt)
    sig = signal_i8(sps, span, 2, n_bits=2 * (total // sps + 2 * span + 8), seed0=40)
    assert sig.shape[1] >= 2 * total
    x[4:] = as_fmt(sig[:, : 2 * total], fmt)
    w = widened(x, fmt, DEFAULT_SCALE if scale is None else scale)
    refs = [fir_ref(rrc(sps, span), w[s], lanes) for s in range(6)]
    x.setflags(write=False)
    return x, calls, refs


def stage_case(Q, sps, span, fmt, how, lanes=8, seed=0, scale=None):
    x, calls, refs = stage_inputs(sps, span, fmt, lanes, seed, scale)
    b = make(Q, 6, sps, span, 4097 if how == "host-4097" else 4098, vector_lanes=lanes)
    if scale is not None:
        b.set_input_scale(fmt, scale)
    if how.startswith("host"):
        _, mfs = host_calls(Q, b, x, calls, fmt)
    else:
        _, mfs = device_calls(Q, b, x, calls, fmt, layout=how.split("-")[1])
    assert b.status() == 0
    b.close()
    assert_rows(mfs, calls, refs)


@pytest.mark.parametrize("how", ["host-4098", "host-4097", "device-vector", "device-scalar"])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("sps,span", SPECIALISED, ids=_ids(SPECIALISED))
def test_matched_filter_rows_bitwise(Q, sps, span, fmt, how):
    """Every specialised tap count over the call sequence, through both
    stagings (module docstring)."""
    stage_case(Q, sps, span, fmt, how, seed=9000)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("sps,span", [(2, 6), (2, 10)], ids=["T13", "T21"])
def test_matched_filter_rows_8_byte_aligned(Q, sps, span, fmt):
    """T - 1 = 4 mod 8: rows that are 8-byte but not 16-byte aligned take the
    8-byte (4-sample) loads."""
    stage_case(Q, sps, span, fmt, "device-half", seed=9000)


@pytest.mark.parametrize("sps,span,lanes,fmt", [(3, 5, 8, "cu8"), (8, 8, 4, "cs8")], ids=["T16-generic", "T65-W4"])
def test_matched_filter_generic_kernel_and_lanes_4(Q, sps, span, lanes, fmt):
    """fir_generic_kernel with an even tap count, and vector_lanes 4."""
    stage_case(Q, sps, span, fmt, "host-4098", lanes=lanes, seed=9100)
    stage_case(Q, sps, span, fmt, "device-scalar", lanes=lanes, seed=9100)


# ---------------------------------------------------------------------------
# 4. whole chain
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sps,span,S", [(2, 10, 5), (4, 32, 70)], ids=["T21-S5", "T129-S70"])
def test_chain_host_device_pipelined_chunked(Q, sps, span, S):
    """Bits and symbols of ragged host calls, device calls (both layouts),
    pipelined calls and one chunked call of 3 chunks, cs8."""
    fmt = "cs8"
    x = signal_i8(sps, span, S)
    n = x.shape[1] // 2
    w = widened(x, fmt)
    calls = split_calls(S, n, 3, seed=sps + S)
    nmax = max(max(c) for c in calls)
    want = oracle_chain(w, calls, sps, span)
    runs = [("host", host_calls), ("device vector", functools.partial(device_calls, layout="vector")),
            ("device scalar", functools.partial(device_calls, layout="scalar")),
            ("pipelined", functools.partial(device_calls, pipelined=True))]
    for what, run in runs:
        b = make(Q, S, sps, span, nmax + 5)
        got, _ = run(Q, b, x, calls, fmt)
        assert b.status() == 0
        if what == "pipelined":
            assert b.pipeline_depth() == 2
        b.close()
        assert_same(got, want, what)

    one = [[n] * S]
    want1 = oracle_chain(w, one, sps, span)
    for run in (host_calls, device_calls, functools.partial(device_calls, layout="scalar", pipelined=True)):
        b = make(Q, S, sps, span, n // 3 + 1)   # 3 chunks
        got = run(Q, b, x, one, fmt)[0]
        assert b.status() == 0
        b.close()
        assert_same(got, want1, "chunked")


def test_chain_glibc_trig_and_constellation_mode(Q):
    """costas_trig 1 (the oracle's libm trig), with deModulateConstellation
    calls between the DeModulate ones."""
    sps, span, S, fmt = 8, 8, 5, "cs8"
    x = signal_i8(sps, span, S, seed0=21)
    n = x.shape[1] // 2
    calls = split_calls(S, n, 3, seed=91)
    mode = [0, 1, 0, 1]
    want = oracle_chain(widened(x, fmt), calls, sps, span, mode=mode, trig=O.TRIG_LIBM)
    nmax = max(max(c) for c in calls)
    for run in (host_calls, device_calls, functools.partial(device_calls, pipelined=True)):
        b = make(Q, S, sps, span, nmax, costas_trig=1)
        got = run(Q, b, x, calls, fmt, mode=mode)[0]
        assert b.status() == 0
        b.close()
        assert_same(got, want)


# ---------------------------------------------------------------------------
# 5. equivalence to the float path (no oracle)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_equals_the_float_path_fed_the_widened_floats(Q, fmt):
    sps, span, S = 8, 8, 5
    x = np.concatenate([as_fmt(signal_i8(sps, span, S, seed0=60), fmt), random_bytes(S, 1500, 61, fmt)], axis=1)
    n = x.shape[1] // 2
    calls = split_calls(S, n, 4, seed=62)
    nmax = max(max(c) for c in calls)
    a, f = make(Q, S, sps, span, nmax + 2), make(Q, S, sps, span, nmax + 2)
    got8, mf8 = host_calls(Q, a, x, calls, fmt)
    got32, mf32 = host_calls(Q, f, widened(x, fmt), calls, "cf32")
    assert a.status() == 0 and f.status() == 0
    assert a.get_state() == f.get_state(), "state blobs (float either way)"
    a.close()
    f.close()
    assert_same(got8, got32)
    for ci, (m8, m32) in enumerate(zip(mf8, mf32)):
        assert K.bitwise_equal(m8, m32), f"call {ci}: matched-filter rows"


# ---------------------------------------------------------------------------
# 6. all four formats on one handle
# ---------------------------------------------------------------------------
def test_cf32_cs8_cs16_cu8_calls_on_one_handle(Q):
    """The same samples call by call as floats, int8, int16 (x 256 at the CS16
    default scale: v * 256 / 32768 = v / 128 exactly) and uint8, against one
    oracle run over the concatenated floats."""
    sps, span, S = 4, 32, 5
    v = signal_i8(sps, span, S, seed0=70)
    n = v.shape[1] // 2
    w = widened(v, "cs8")
    k = n // 5
    calls = [[k] * S, [k + 1] * S, [k + 3] * S, [k] * S, [n - 4 * k - 4] * S]
    fmts = ["cf32", "cs8", "cs16", "cu8", "cs8"]
    b = make(Q, S, sps, span, max(max(c) for c in calls))
    pos = np.zeros(S, np.int64)
    got, mfs = [], []
    for ci, (lens, fmt) in enumerate(zip(calls, fmts)):
        rows, m = call_rows(v, calls, ci, pos, np.int8)
        rows = {"cf32": lambda r: widened(r, "cs8"), "cs8": lambda r: r, "cu8": lambda r: as_fmt(r, "cu8"),
                "cs16": lambda r: r.astype(np.int16) * np.int16(256)}[fmt](rows)
        assert rows.dtype == DTYPE[fmt]
        bits, nb, syms, ns = run_call(Q, b, fmt, rows, Q.MODE_DEMODULATE, lens)
        got.append(decoded(Q, Q.MODE_DEMODULATE, bits, nb, syms, ns, S))
        mfs.append(b.last_mf(m).copy())
        pos += np.array(lens)
    assert b.status() == 0
    b.close()
    assert_same(got, oracle_chain(w, calls, sps, span))
    assert_rows(mfs, calls, [fir_ref(rrc(sps, span), w[s]) for s in range(S)])


# ---------------------------------------------------------------------------
# 7. non-finite history
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sps,span", [(8, 8), (4, 32)], ids=_ids([(8, 8), (4, 32)]))
def test_nan_and_inf_in_the_history_of_a_cs8_call(Q, sps, span):
    """A float call whose last T-1 samples hold a NaN and an Inf, then a CS8
    call: its first outputs have them in their windows, so the tile kernel's
    recompute path reads the float history and the byte row."""
    S, T = 3, sps * span + 1
    n1, n2 = 700, TILE + 300
    f = np.random.default_rng(80).standard_normal((S, 2 * n1)).astype(np.float32)
    f[0, 2 * (n1 - 5)] = np.nan                  # I of stream 0, 5 samples from the end
    f[1, 2 * (n1 - (T - 1)) + 1] = np.inf        # Q of stream 1, the oldest history sample
    f[2, 2 * (n1 - 1)] = -np.inf                 # stream 2: the newest
    f[2, 2 * (n1 - 2) + 1] = np.nan
    x = random_bytes(S, n2, 81, "cs8")
    b = make(Q, S, sps, span, n2)
    with contextlib.suppress(Q.QPSKError):       # non-finite timing: reported, rows still written
        b.process(f)
    with contextlib.suppress(Q.QPSKError):
        b.process_fmt(x, "cs8")
    mf = b.last_mf(n2)
    assert b.status() & Q.STATUS_NONFINITE_TIMING
    b.close()
    h = rrc(sps, span)
    for s in range(S):
        ref = fir_ref(h, np.concatenate([f[s], widened(x[s], "cs8")]))[2 * n1:]
        assert np.isnan(ref[: 2 * (T - 1)]).any() and np.isfinite(ref[2 * (T - 1):]).all()
        assert K.bitwise_equal(mf[s], ref, nan_any_payload=True), f"stream {s}"


# ---------------------------------------------------------------------------
# 8. scales
# ---------------------------------------------------------------------------
def test_scale_defaults_setters_and_rejections(Q):
    b = make(Q, 2, 8, 8, 256)
    for fmt in FMTS:
        assert np.float32(b.input_scale(fmt)) == DEFAULT_SCALE == np.float32(2.0 ** -7)
        for bad in (0.0, -1.0, -0.0, float("nan"), float("inf"), float("-inf")):
            with pytest.raises(ValueError, match="qpsk error -3"):   # QPSK_ERR_OUT_OF_RANGE
                b.set_input_scale(fmt, bad)
            assert np.float32(b.input_scale(fmt)) == DEFAULT_SCALE
    b.set_input_scale("cs8", ODD_SCALE)                              # per format
    assert np.float32(b.input_scale("cs8")) == ODD_SCALE and np.float32(b.input_scale("cu8")) == DEFAULT_SCALE
    # CS16: one variable behind both pairs of entry points
    assert np.float32(b.input_scale("cs16")) == np.float32(b.cs16_scale()) == np.float32(2.0 ** -15)
    b.set_input_scale("cs16", 1 / 20000)
    assert np.float32(b.cs16_scale()) == np.float32(1 / 20000)
    b.set_cs16_scale(0.25)
    assert b.input_scale("cs16") == 0.25
    # CF32 has none; an unknown format
    L, v = Q.lib(), Q.C.c_float()
    with pytest.raises(ValueError, match="qpsk error -1"):
        b.set_input_scale("cf32", 1.0)
    assert L.qpsk_demod_get_input_scale(b._h, Q.FMT_CF32, Q.C.byref(v)) == Q.QPSK_ERR_ARGUMENT
    for unknown in (-1, 4):
        assert L.qpsk_demod_set_input_scale(b._h, unknown, Q.C.c_float(1.0)) == Q.QPSK_ERR_ARGUMENT
        assert L.qpsk_demod_get_input_scale(b._h, unknown, Q.C.byref(v)) == Q.QPSK_ERR_ARGUMENT
    b.close()


@pytest.mark.parametrize("fmt", FMTS)
def test_scale_change_between_pipelined_calls_applies_to_the_later_one(Q, fmt):
    """The scale is captured when a call is issued: the queued call keeps its own."""
    sps, span, S = 8, 8, 5
    x = as_fmt(signal_i8(sps, span, S, seed0=77), fmt)
    n = x.shape[1] // 2
    k = n // 4
    calls = [[k] * S, [k] * S, [k] * S, [n - 3 * k] * S]
    scales = [None, ODD_SCALE, None, DEFAULT_SCALE]           # set before calls 1 and 3
    per_call = [DEFAULT_SCALE, ODD_SCALE, ODD_SCALE, DEFAULT_SCALE]
    w = np.concatenate([widened(x[:, 2 * k * c: (2 * k * (c + 1) if c < 3 else 2 * n)], fmt, per_call[c])
                        for c in range(4)], axis=1)
    b = make(Q, S, sps, span, n - 3 * k)
    got, _ = device_calls(Q, b, x, calls, fmt, pipelined=True, scales=scales)
    assert b.status() == 0
    b.close()
    assert_same(got, oracle_chain(w, calls, sps, span))


# ---------------------------------------------------------------------------
# 9. FLL and IQ balancer in front (one widening pass ahead of them)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,kw,okw", [
    ("cs8", dict(enable_fll=True, cfo_loop_bandwidth=1e-3), dict(enable_fll=True, cfo_loop_bw=1e-3)),
    ("cu8", dict(enable_fll=True, cfo_loop_bandwidth=1e-3, vector_lanes=4),
     dict(enable_fll=True, cfo_loop_bw=1e-3, lanes=4)),
    ("cu8", dict(iq_balance=True), dict(iq_balance=True)),
    ("cs8", dict(iq_balance=True, enable_fll=True, cfo_loop_bandwidth=1e-3),
     dict(iq_balance=True, enable_fll=True, cfo_loop_bw=1e-3)),
], ids=["fll-systolic", "fll-one-lane", "iq-balance", "iq-balance-fll"])
def test_fll_and_iq_balance_ragged_chunks(Q, fmt, kw, okw):
    """Ragged chunks (shorter than 8 samples and than the 40-tap window, empty
    ones): host calls (the 16-byte widening pass) and device calls in the
    2-byte layout."""
    sps, span, S = 8, 8, 7
    x = as_fmt(signal_i8(sps, span, S, n_bits=1200, seed0=85, cfo_hz=-3000.0), fmt)
    n = x.shape[1] // 2
    rng = np.random.default_rng(86)
    calls, used = [], np.zeros(S, np.int64)
    for c in range(7):
        lens = rng.integers(0, 50, S) if c < 5 else np.full(S, 37 + 1000 * (c - 5))
        if c < 2:
            lens = np.minimum(lens, 7)
        lens[c % S] = 0
        calls.append([int(v) for v in lens])
        used += lens
    calls.append([int(n - u) for u in used])
    want = oracle_chain(widened(x, fmt), calls, sps, span, **okw)
    nmax = max(max(c) for c in calls)
    for run in (host_calls, functools.partial(device_calls, layout="scalar")):
        b = make(Q, S, sps, span, nmax, **kw)
        got = run(Q, b, x, calls, fmt)[0]
        assert b.status() == 0
        b.close()
        assert_same(got, want)


# ---------------------------------------------------------------------------
# 10. the ring
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
def test_host_ring_equals_consecutive_calls(Q, fmt):
    """Depth 3, 6 ragged chunks, filled in place through next_slot and passed
    from caller memory in turn."""
    sps, span, S, depth = 8, 8, 5, 3
    x = as_fmt(signal_i8(sps, span, S, seed0=95), fmt)
    n = x.shape[1] // 2
    calls = split_calls(S, n, 5, seed=99)
    assert len(calls) == 6
    nmax = max(max(c) for c in calls)
    ref_b = make(Q, S, sps, span, nmax + 3)
    want, _ = host_calls(Q, ref_b, x, calls, fmt)
    ref_b.close()

    b = make(Q, S, sps, span, nmax + 3)              # no multiple of 8: the device slots are pitched
    ring = Q.HostRing.create_fmt(b, depth, fmt)
    slot = ring.next_slot()
    assert slot.dtype == DTYPE[fmt] and slot.shape == (S, 2 * (nmax + 3))
    pos = np.zeros(S, np.int64)
    got, pending = [], 0

    def collect():
        bits, nb, _ = ring.collect()
        got.append([(Q.unpack_bits(bits[s], int(nb[s])), None) for s in range(S)])

    for ci, lens in enumerate(calls):
        if pending == depth:
            collect()
            pending -= 1
        rows, m = call_rows(x, calls, ci, pos, x.dtype)
        if ci % 2 == 0:
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


def test_ring_format_misuse_is_a_state_error(Q):
    C, L = Q.C, Q.lib()
    b = make(Q, 2, 8, 8, 512)
    f32 = np.zeros((2, 200), np.float32)
    i8 = np.zeros((2, 200), np.int8)
    u8 = np.full((2, 200), 128, np.uint8)
    ptr, stride, t = C.c_void_p(), C.c_int64(), C.c_int64()
    ring = Q.HostRing.create_fmt(b, 2, "cs8")
    assert L.qpsk_rx_next_slot(ring._r, C.byref(ptr), C.byref(stride)) == Q.QPSK_ERR_STATE
    assert L.qpsk_rx_submit(ring._r, f32.ctypes.data, 200, 100, None, C.byref(t)) == Q.QPSK_ERR_STATE
    assert L.qpsk_rx_submit_fmt(ring._r, Q.FMT_CU8, u8.ctypes.data, 200, 100, None, C.byref(t)) == Q.QPSK_ERR_STATE
    assert L.qpsk_rx_next_slot_fmt(ring._r, Q.FMT_CS16, C.byref(ptr), C.byref(stride)) == Q.QPSK_ERR_STATE
    assert L.qpsk_rx_submit_fmt(ring._r, 4, i8.ctypes.data, 200, 100, None, C.byref(t)) == Q.QPSK_ERR_ARGUMENT
    with pytest.raises(ValueError):
        ring.submit(u8, 100)                     # the binding converts nothing either
    ring.submit(i8, 100)
    ring.collect()
    ring.close()
    ring = Q.HostRing(b, 2)
    assert L.qpsk_rx_next_slot_fmt(ring._r, Q.FMT_CS8, C.byref(ptr), C.byref(stride)) == Q.QPSK_ERR_STATE
    assert L.qpsk_rx_submit_fmt(ring._r, Q.FMT_CU8, u8.ctypes.data, 200, 100, None, C.byref(t)) == Q.QPSK_ERR_STATE
    assert L.qpsk_rx_next_slot_fmt(ring._r, Q.FMT_CF32, C.byref(ptr), C.byref(stride)) == Q.QPSK_OK
    ring.submit(f32, 100)
    ring.collect()
    ring.close()
    r = C.c_void_p()
    assert L.qpsk_rx_create_fmt(b._h, 2, 7, C.byref(r)) == Q.QPSK_ERR_ARGUMENT
    assert b.status() == 0
    b.close()


# ---------------------------------------------------------------------------
# 11. argument errors, returned before any launch
# ---------------------------------------------------------------------------
def test_argument_errors(Q):
    import torch
    S, n = 2, 100
    b = make(Q, S, 8, 8, 256)
    before = b.get_state()
    ms = b.max_symbols(n)
    bits = torch.zeros((S, (2 * ms + 7) // 8 + 8), dtype=torch.uint8, device="cuda")
    nb = torch.zeros(S, dtype=torch.int64, device="cuda")
    buf = torch.zeros((S, 2 * n + 8), dtype=torch.int8, device="cuda")
    odd_addr = buf[:, 1: 2 * n + 1]
    assert odd_addr.data_ptr() % 2 == 1 and odd_addr.stride(0) % 2 == 0
    odd_stride = torch.zeros((S, 2 * n + 1), dtype=torch.int8, device="cuda")[:, : 2 * n]
    assert odd_stride.data_ptr() % 2 == 0 and odd_stride.stride(0) % 2 == 1
    for bad in (odd_addr, odd_stride):
        for call in (b.process_device_fmt, b.process_device_async_fmt):
            with pytest.raises(ValueError, match="qpsk error -1"):   # QPSK_ERR_ARGUMENT
                call(bad, n, bits, nb, "cs8")
    L = Q.lib()
    args = (bits.data_ptr(), bits.stride(0), nb.data_ptr(), None, 0, None)
    for fmt in (Q.FMT_CS8, Q.FMT_CU8):
        assert L.qpsk_demod_process_fmt(b._h, fmt, 0, buf.data_ptr(), 2 * n - 2, n, None, Q.MEM_DEVICE, *args) == \
            Q.QPSK_ERR_ARGUMENT                                      # stride < 2 n
        assert L.qpsk_demod_process_fmt(b._h, fmt, 0, None, 2 * n, n, None, Q.MEM_DEVICE, *args) == \
            Q.QPSK_ERR_ARGUMENT_NULL
        assert L.qpsk_demod_process_fmt(b._h, fmt, 0, buf.data_ptr(), 1 << 33, (1 << 31) - 128, None,
                                        Q.MEM_DEVICE, *args) == Q.QPSK_ERR_OUT_OF_RANGE   # the 2^31 - 129 limit
    for unknown in (-1, 4):
        assert L.qpsk_demod_process_fmt(b._h, unknown, 0, buf.data_ptr(), 2 * n + 8, n, None, Q.MEM_DEVICE,
                                        *args) == Q.QPSK_ERR_ARGUMENT
        assert L.qpsk_demod_process_async_fmt(b._h, unknown, 0, buf.data_ptr(), 2 * n + 8, n, None,
                                              *args) == Q.QPSK_ERR_ARGUMENT
    x = np.zeros((S, 2 * n), np.int8)
    with pytest.raises(ValueError):
        b.process_fmt(np.zeros((S, 2 * n + 1), np.int8), "cs8")   # odd count
    with pytest.raises(ValueError):
        b.process_fmt(x.astype(np.int16), "cs8")                  # nothing is converted on the way
    with pytest.raises(ValueError):
        b.process_fmt(x, "cu8")                                   # int8 rows are no CU8 rows
    with pytest.raises(ValueError):
        b.process_fmt(x, "cs12")
    with pytest.raises(ValueError):
        b.process_device_fmt(buf.to(torch.int16), n, bits, nb, "cs8")
    assert b.get_state() == before, "nothing ran"
    b.process_fmt(x, "cs8")
    assert b.status() == 0
    b.close()


# ---------------------------------------------------------------------------
# 12. group
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["cs16", "cs8"])
def test_group_process_fmt_equals_one_handle(Q, fmt):
    """Two shards on device 0, host and device rows: bitwise one handle's."""
    import torch
    sps, span, S = 8, 8, 7
    v = signal_i8(sps, span, S, seed0=110)
    x = v if fmt == "cs8" else v.astype(np.int16) * np.int16(256)
    n = x.shape[1] // 2
    k = n // 2 + 3
    p = Q.params(K.FS, K.FS // sps, K.ALPHA, span, max_samples_per_call=k)
    one, grp = Q.BatchDemodulator(S, p), Q.DemodGroup(S, p, [0, 0])
    # host rows, ragged
    lens = np.array([k - 5 * s for s in range(S)], np.int64)
    x0 = np.ascontiguousarray(x[:, : 2 * k])
    a = one.process_fmt(x0, fmt, lengths=lens, want_syms=True)
    g = grp.process_fmt(x0, fmt, lengths=lens, want_syms=True)
    assert np.array_equal(a[1], g[1]) and np.array_equal(a[3], g[3]) and a[1].min() > 0
    for s in range(S):
        nb, ns = int(a[1][s]), int(a[3][s])
        assert np.array_equal(a[0][s, : (nb + 7) // 8], g[0][s, : (nb + 7) // 8]), s
        assert K.bitwise_equal(a[2][s, : 2 * ns], g[2][s, : 2 * ns]), s
    # device rows (second shard's rows start at row 3: an odd multiple of the stride)
    m = n - k
    ms = one.max_symbols(m)
    xd = torch.from_numpy(np.ascontiguousarray(x[:, 2 * k:])).cuda()

    def out():
        return (torch.zeros((S, (2 * ms + 7) // 8 + 8), dtype=torch.uint8, device="cuda"),
                torch.zeros(S, dtype=torch.int64, device="cuda"),
                torch.zeros((S, 2 * ms), dtype=torch.float32, device="cuda"),
                torch.zeros(S, dtype=torch.int64, device="cuda"))
    r, c = out(), out()
    torch.cuda.synchronize()
    one.process_device_fmt(xd, m, r[0], r[1], fmt, syms_dev=r[2], n_syms_dev=r[3])
    grp.process_device_fmt(xd, m, c[0], c[1], fmt, syms_dev=c[2], n_syms_dev=c[3])   # joined on return
    torch.cuda.synchronize()
    assert torch.equal(r[1], c[1]) and torch.equal(r[3], c[3]) and int(r[1].min()) > 0
    for s in range(S):
        nb, ns = int(r[1][s]), int(r[3][s])
        assert torch.equal(r[0][s, : (nb + 7) // 8], c[0][s, : (nb + 7) // 8]), s
        assert torch.equal(r[2][s, : 2 * ns].view(torch.int32), c[2][s, : 2 * ns].view(torch.int32)), s
    assert one.status() == 0
    one.close()
    grp.close()


def test_group_bad_length_in_the_last_shard_moves_no_state(Q):
    sps, span, S = 8, 8, 4
    p = Q.params(K.FS, K.FS // sps, K.ALPHA, span, max_samples_per_call=4096)
    grp = Q.DemodGroup(S, p, [0, 0])
    x = as_fmt(signal_i8(sps, span, S, seed0=120), "cu8")[:, : 2 * 1000].copy()
    grp.process_fmt(x, "cu8")                                   # some state to keep
    before = [grp.get_state(k) for k in range(2)]
    L = Q.lib()
    nb = np.zeros(S, np.int64)
    bits = np.zeros((S, 4096), np.uint8)
    lens = np.array([1000, 1000, 1000, -1], np.int64)           # the last shard's last row
    rc = L.qpsk_demod_group_process_fmt(grp._g, Q.FMT_CU8, 0, x.ctypes.data, x.shape[1], 0,
                                        lens.ctypes.data_as(Q.C.POINTER(Q.C.c_int64)), Q.MEM_HOST, bits.ctypes.data,
                                        4096, nb.ctypes.data, None, 0, None)
    assert rc == Q.QPSK_ERR_ARGUMENT
    lens[3] = 1001                                              # longer than the rows' stride allows
    rc = L.qpsk_demod_group_process_fmt(grp._g, Q.FMT_CU8, 0, x.ctypes.data, x.shape[1], 0,
                                        lens.ctypes.data_as(Q.C.POINTER(Q.C.c_int64)), Q.MEM_HOST, bits.ctypes.data,
                                        4096, nb.ctypes.data, None, 0, None)
    assert rc == Q.QPSK_ERR_ARGUMENT
    assert L.qpsk_demod_group_process_fmt(grp._g, 5, 0, x.ctypes.data, x.shape[1], 1000, None, Q.MEM_HOST,
                                          bits.ctypes.data, 4096, nb.ctypes.data, None, 0, None) == Q.QPSK_ERR_ARGUMENT
    assert [grp.get_state(k) for k in range(2)] == before
    grp.close()
