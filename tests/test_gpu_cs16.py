"""CS16 (interleaved int16 I,Q) input, bit for bit.

A CS16 sample's value is float32(x) * scale: an exact conversion and one IEEE
multiply, which numpy reproduces (`x.astype(np.float32) * np.float32(scale)`).
So the reference of every check here is the CPU oracle fed those widened
floats, at tolerance 0: matched-filter rows (qpsk_demod_last_mf against
O.oracle_fir), bits and rotated symbols (against OracleDemod).

Inputs: K.batch_signals rows quantised to int16 at half of full scale, and
rows of uniform random int16 over the whole range with -32768, 32767, 0 and
+-1 placed at their head.

Stagings of the tile kernel.  Host-memory calls stage int16 rows whose pitch
is max_samples_per_call rounded up to 4 samples, so they take the 16-byte
staging whatever max_samples_per_call is; the 4-byte staging runs for device
rows that are 4-byte aligned only or whose stride is no multiple of 4
samples.  test_matched_filter_rows_bitwise therefore runs the ragged call
sequence four ways per tap count: host calls at max_samples_per_call 4098 and
4097, and device calls in a 16-byte layout and in a 4-byte layout.
"""
import contextlib
import functools

import numpy as np
import pytest

import common as K
import oracle as O
from test_gpu_fir import SPECIALISED, TILE, _ids, assert_rows, fir_ref, ragged_calls, rrc

pytestmark = pytest.mark.gpu

DEFAULT_SCALE = np.float32(1.0) / np.float32(32768)
ODD_SCALE = np.float32(1 / 20000)   # no power of two: the multiply rounds


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
def widened(x16, scale=DEFAULT_SCALE):
    """The value the library gives int16 samples: one conversion, one multiply."""
    assert x16.dtype == np.int16
    w = x16.astype(np.float32) * np.float32(scale)
    assert w.dtype == np.float32
    return w


@functools.lru_cache(maxsize=None)
def signal_i16(sps, span, S, n_bits=1600, seed0=0, cfo_hz=0.0):
    """K.batch_signals rows quantised at half of full scale.  Past 5 streams the
    rows are the first 5 rotated in time (still QPSK, all different)."""
    base = K.batch_signals(min(S, 5), seed0=seed0, sps=sps, span=span, n_bits=n_bits, snr_db=18, cfo_hz=cfo_hz)
    q = np.round(base * (16384.0 / np.abs(base).max())).astype(np.int16)
    rows = [q[s] if s < 5 else np.roll(q[s % 5], 2 * 37 * s) for s in range(S)]
    out = np.stack(rows)
    assert np.abs(out).max() == 16384
    out.setflags(write=False)
    return out


def random_i16(S, n, seed):
    """Uniform over the whole int16 range; the extremes, 0 and +-1 lead each row."""
    x = np.random.default_rng(seed).integers(-32768, 32768, (S, 2 * n), dtype=np.int16)
    head = np.array([-32768, 32767, 0, 0, 1, -1, -1, 1, -32768, -32768], np.int16)
    k = min(head.size, x.shape[1])
    x[:, :k] = head[:k]
    return x


def oracle_chain(iq_f32, calls, sps, span, mode=None, **okw):
    """Per call and stream (bits, symbols) of per-stream oracles fed float rows."""
    S = iq_f32.shape[0]
    dms = [K.oracle_for(sps, span, **okw) for _ in range(S)]
    pos = np.zeros(S, np.int64)
    out = []
    for ci, lens in enumerate(calls):
        res = []
        for s in range(S):
            x = iq_f32[s, 2 * pos[s]: 2 * (pos[s] + lens[s])]
            if mode and mode[ci] == 1:
                res.append(("", dms[s].deModulateConstellation(x)))
            else:
                bits, syms, _ = dms[s].demodulate_ex(x)
                res.append((bits, syms))
            pos[s] += lens[s]
        out.append(res)
    return out


def assert_same(got, want, what=""):
    assert len(got) == len(want)
    for ci, (ra, rb) in enumerate(zip(got, want)):
        for s, ((ba, sa), (bb, sb)) in enumerate(zip(ra, rb)):
            assert ba == bb, f"{what} call {ci} stream {s}: bits differ ({len(ba)} vs {len(bb)})"
            if sa is None or sb is None:
                continue
            assert K.bitwise_equal(sa, sb), f"{what} call {ci} stream {s}: symbols differ (bitwise)"


def call_rows(x, calls, ci, pos, dtype):
    """The [S, 2 max(lens)] rows of call ci, zero behind each stream's length."""
    lens = calls[ci]
    S, n = x.shape[0], int(max(lens))
    rows = np.zeros((S, 2 * max(n, 1)), dtype)
    for s in range(S):
        rows[s, : 2 * lens[s]] = x[s, 2 * pos[s]: 2 * (pos[s] + lens[s])]
    return rows[:, : 2 * n] if n else rows[:, :0], n


def lengths_of(lens):
    return None if all(l == lens[0] for l in lens) else np.array(lens, np.int64)


def host_calls(Q, b, x16, calls, mode=None, fmt=None):
    """Host-memory calls on handle b.  fmt[ci] 'cs16' (default) or 'cf32' (then
    x16's rows for that call are widened on the CPU and go through process()).
    Returns per call the decoded rows and last_mf."""
    S = x16.shape[0]
    pos = np.zeros(S, np.int64)
    out, mfs = [], []
    for ci, lens in enumerate(calls):
        m = mode[ci] if mode else Q.MODE_DEMODULATE
        rows, n = call_rows(x16, calls, ci, pos, np.int16)
        if fmt and fmt[ci] == "cf32":
            bits, nb, syms, ns = b.process(widened(rows, b.cs16_scale()), mode=m, lengths=lengths_of(lens),
                                           want_syms=True)
        else:
            bits, nb, syms, ns = b.process_cs16(rows, mode=m, lengths=lengths_of(lens), want_syms=True)
        out.append([(Q.unpack_bits(bits[s], int(nb[s])) if m == Q.MODE_DEMODULATE else "",
                     syms[s, : 2 * int(ns[s])].copy()) for s in range(S)])
        mfs.append(b.last_mf(n).copy() if n <= b.p.max_samples_per_call else None)   # not after a chunked call
        pos += np.array(lens)
    return out, mfs


def device_rows(S, n_cap, layout):
    """An int16 device view of S rows holding n_cap samples each.
    'vector': 16-byte aligned rows, stride_i16 % 8 == 0.
    'scalar': rows one sample in (4-byte aligned only), stride_i16 = 2 mod 8."""
    import torch
    if layout == "vector":
        pitch = (n_cap + 3) // 4 * 4
        v = torch.zeros((S, 2 * pitch), dtype=torch.int16, device="cuda")[:, : 2 * n_cap]
        assert v.data_ptr() % 16 == 0 and v.stride(0) % 8 == 0
    else:
        pitch = n_cap + 1
        pitch += (1 - pitch) % 4   # samples per row = 1 mod 4
        v = torch.zeros((S, 2 * pitch), dtype=torch.int16, device="cuda")[:, 2: 2 * n_cap + 2]
        assert v.data_ptr() % 16 == 4 and v.stride(0) % 8 == 2
    return v


def device_calls(Q, b, x16, calls, layout="vector", pipelined=False, mode=None, scales=None):
    """Device-memory calls (synchronous, or pipelined with one wait at the
    end), each call's outputs in rows of its own.  scales[ci]: set before call ci."""
    import torch
    S = x16.shape[0]
    nmax = max(max(c) for c in calls)
    ms = max(b.max_symbols(nmax), 1)
    pos = np.zeros(S, np.int64)
    outs, mfs = [], []
    for ci, lens in enumerate(calls):
        m = mode[ci] if mode else Q.MODE_DEMODULATE
        rows, n = call_rows(x16, calls, ci, pos, np.int16)
        xd = device_rows(S, max(n, 1), layout)
        if n:
            xd[:, : 2 * n].copy_(torch.from_numpy(np.ascontiguousarray(rows)))
        bits = torch.zeros((S, ((2 * ms + 7) // 8 + 63) // 64 * 64), dtype=torch.uint8, device="cuda")
        sy = torch.zeros((S, 2 * ms), dtype=torch.float32, device="cuda")
        nb = torch.zeros(S, dtype=torch.int64, device="cuda")
        ns = torch.zeros(S, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        if scales and scales[ci] is not None:
            b.set_cs16_scale(scales[ci])
        call = b.process_device_async_cs16 if pipelined else b.process_device_cs16
        call(xd, n, bits if m == Q.MODE_DEMODULATE else None, nb if m == Q.MODE_DEMODULATE else None, mode=m,
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
        bits, nb, sy, ns = bits.cpu().numpy(), nb.cpu().numpy(), sy.cpu().numpy(), ns.cpu().numpy()
        res.append([(Q.unpack_bits(bits[s], int(nb[s])) if m == Q.MODE_DEMODULATE else "",
                     sy[s, : 2 * int(ns[s])].copy()) for s in range(S)])
    return res, mfs


def make(Q, S, sps, span, n_max, **kw):
    return Q.BatchDemodulator(S, Q.params(K.FS, K.FS // sps, K.ALPHA, span, max_samples_per_call=n_max, **kw))


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


# ---------------------------------------------------------------------------
# 1. matched-filter rows
# ---------------------------------------------------------------------------
def stage_inputs(sps, span, total, seed):
    """6 rows of `total` samples: 4 of random int16, 2 of quantised signal."""
    x = random_i16(6, total, seed)
    sig = signal_i16(sps, span, 2, n_bits=2 * (total // sps + 2 * span + 8), seed0=40)
    assert sig.shape[1] >= 2 * total
    x[4:] = sig[:, : 2 * total]
    return x


def stage_case(Q, sps, span, how, lanes=8, seed=0, scale=None):
    T = sps * span + 1
    calls = ragged_calls(T)
    total = sum(c[0] for c in calls)
    x = stage_inputs(sps, span, total, seed + T)
    b = make(Q, 6, sps, span, 4097 if how == "host-4097" else 4098, vector_lanes=lanes)
    if scale is not None:
        b.set_cs16_scale(scale)
    if how.startswith("host"):
        _, mfs = host_calls(Q, b, x, calls)
    else:
        _, mfs = device_calls(Q, b, x, calls, layout=how.split("-")[1])
    assert b.status() == 0
    b.close()
    h = rrc(sps, span)
    w = widened(x, DEFAULT_SCALE if scale is None else scale)
    assert_rows(mfs, calls, [fir_ref(h, w[s], lanes) for s in range(6)])


@pytest.mark.parametrize("how", ["host-4098", "host-4097", "device-vector", "device-scalar"])
@pytest.mark.parametrize("sps,span", SPECIALISED, ids=_ids(SPECIALISED))
def test_matched_filter_rows_bitwise(Q, sps, span, how):
    """Every specialised tap count over the ragged call sequence (calls shorter
    than T-1, 2047 / 2048 / 2049 / 4097 samples, both parities), through both
    stagings (module docstring)."""
    stage_case(Q, sps, span, how, seed=7000)


@pytest.mark.parametrize("sps,span,lanes", [(3, 5, 8), (8, 8, 4)], ids=["T16-generic", "T65-W4"])
def test_matched_filter_generic_kernel_and_lanes_4(Q, sps, span, lanes):
    """fir_generic_kernel with an even tap count, and vector_lanes 4."""
    stage_case(Q, sps, span, "host-4098", lanes=lanes, seed=7100)
    stage_case(Q, sps, span, "device-scalar", lanes=lanes, seed=7200)


# ---------------------------------------------------------------------------
# 2. device layouts
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sps,span", [(8, 8), (4, 32)], ids=_ids([(8, 8), (4, 32)]))
def test_device_input_layouts(Q, sps, span):
    """16-byte rows and 4-byte rows, two calls of 2049 samples: the same rows."""
    S, n = 3, TILE + 1
    h = rrc(sps, span)
    x = random_i16(S, 2 * n, seed=7300 + h.size)
    refs = [fir_ref(h, widened(x[s])) for s in range(S)]
    calls = [[n] * S] * 2
    for layout in ("vector", "scalar"):
        b = make(Q, S, sps, span, n + 3)
        _, mfs = device_calls(Q, b, x, calls, layout=layout)
        b.close()
        try:
            assert_rows(mfs, calls, refs)
        except BaseException as e:
            raise AssertionError(f"layout '{layout}': {e}") from e


def test_device_rows_misaligned_or_odd_stride_are_argument_errors(Q):
    import torch
    S, n = 2, 100
    b = make(Q, S, 8, 8, 256)
    ms = b.max_symbols(n)
    bits = torch.zeros((S, (2 * ms + 7) // 8 + 8), dtype=torch.uint8, device="cuda")
    nb = torch.zeros(S, dtype=torch.int64, device="cuda")
    buf = torch.zeros((S, 2 * n + 8), dtype=torch.int16, device="cuda")
    two_byte = buf[:, 1: 2 * n + 1]
    assert two_byte.data_ptr() % 4 == 2 and two_byte.stride(0) % 2 == 0
    odd = torch.zeros((S, 2 * n + 1), dtype=torch.int16, device="cuda")[:, : 2 * n]
    assert odd.data_ptr() % 4 == 0 and odd.stride(0) % 2 == 1
    for bad in (two_byte, odd):
        for call in (b.process_device_cs16, b.process_device_async_cs16):
            with pytest.raises(ValueError, match="qpsk error -1"):   # QPSK_ERR_ARGUMENT
                call(bad, n, bits, nb)
    # the checks shared with the float entry points
    x = np.zeros((S, 2 * n), np.int16)
    L = Q.lib()
    args = (bits.data_ptr(), bits.stride(0), nb.data_ptr(), None, 0, None)
    assert L.qpsk_demod_process_cs16(b._h, 0, buf.data_ptr(), 2 * n - 2, n, None, Q.MEM_DEVICE, *args) == \
        Q.QPSK_ERR_ARGUMENT                                      # stride < 2 n
    assert L.qpsk_demod_process_cs16(b._h, 0, None, 2 * n, n, None, Q.MEM_DEVICE, *args) == Q.QPSK_ERR_ARGUMENT_NULL
    assert L.qpsk_demod_process_cs16(b._h, 0, buf.data_ptr(), 1 << 33, (1 << 31) - 128, None, Q.MEM_DEVICE,
                                     *args) == Q.QPSK_ERR_OUT_OF_RANGE   # the 2^31 - 129 limit
    with pytest.raises(ValueError):
        b.process_cs16(np.zeros((S, 2 * n + 1), np.int16))       # odd count
    with pytest.raises(ValueError):
        b.process_cs16(x.astype(np.float32))                     # nothing is converted on the way
    b.process_cs16(x)
    assert b.status() == 0
    b.close()


# ---------------------------------------------------------------------------
# 3. whole chain
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("S", [5, 70])
@pytest.mark.parametrize("sps,span", K.CONFIGS)
def test_chain_host_device_pipelined_chunked(Q, sps, span, S):
    """Bits and symbols of ragged host calls, device calls (both layouts),
    pipelined calls and one chunked call (max_samples_per_call below the call
    length, host and device memory)."""
    x = signal_i16(sps, span, S)
    n = x.shape[1] // 2
    w = widened(x)
    calls = split_calls(S, n, 3, seed=sps + S)
    nmax = max(max(c) for c in calls)
    want = oracle_chain(w, calls, sps, span)

    b = make(Q, S, sps, span, nmax + 5)
    got, _ = host_calls(Q, b, x, calls)
    assert b.status() == 0
    b.close()
    assert_same(got, want, "host")

    for layout in ("vector", "scalar"):
        b = make(Q, S, sps, span, nmax + 5)
        got, _ = device_calls(Q, b, x, calls, layout=layout)
        assert b.status() == 0
        b.close()
        assert_same(got, want, f"device {layout}")

    b = make(Q, S, sps, span, nmax + 5)
    got, _ = device_calls(Q, b, x, calls, pipelined=True)
    assert b.pipeline_depth() == 2 and b.status() == 0
    b.close()
    assert_same(got, want, "pipelined")

    one = [[n] * S]
    want1 = oracle_chain(w, one, sps, span)
    for run in (host_calls, device_calls, functools.partial(device_calls, layout="scalar", pipelined=True)):
        b = make(Q, S, sps, span, n // 3 + 1)   # 3 chunks
        got = run(Q, b, x, one)[0]
        assert b.status() == 0
        b.close()
        assert_same(got, want1, "chunked")


@pytest.mark.parametrize("trig", [0, 1], ids=["portable", "glibc"])
def test_chain_costas_trig_and_constellation_mode(Q, trig):
    """costas_trig 0 and 1 once each (the oracle's portable / libm trig), with
    deModulateConstellation calls between the DeModulate ones."""
    sps, span, S = 8, 8, 5
    x = signal_i16(sps, span, S, seed0=20 + trig)
    n = x.shape[1] // 2
    calls = split_calls(S, n, 3, seed=90 + trig)
    mode = [0, 1, 0, 1]
    want = oracle_chain(widened(x), calls, sps, span, mode=mode, trig=O.TRIG_LIBM if trig else O.TRIG_PORTABLE)
    nmax = max(max(c) for c in calls)
    for run in (host_calls, device_calls, functools.partial(device_calls, pipelined=True)):
        b = make(Q, S, sps, span, nmax, costas_trig=trig)
        got = run(Q, b, x, calls, mode=mode)[0]
        assert b.status() == 0
        b.close()
        assert_same(got, want)


# ---------------------------------------------------------------------------
# 4. equivalence to the float path (no oracle)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sps,span", K.CONFIGS)
def test_equals_the_float_path_fed_the_widened_floats(Q, sps, span):
    S = 5
    x = np.concatenate([signal_i16(sps, span, S, seed0=60), random_i16(S, 1500, seed=61)], axis=1)
    n = x.shape[1] // 2
    calls = split_calls(S, n, 4, seed=62)
    nmax = max(max(c) for c in calls)
    a, f = make(Q, S, sps, span, nmax + 2), make(Q, S, sps, span, nmax + 2)
    got16, mf16 = host_calls(Q, a, x, calls)
    got32, mf32 = host_calls(Q, f, x, calls, fmt=["cf32"] * len(calls))
    assert a.status() == 0 and f.status() == 0
    assert a.get_state() == f.get_state(), "state blobs (float either way)"
    a.close()
    f.close()
    assert_same(got16, got32)
    for ci, (m16, m32) in enumerate(zip(mf16, mf32)):
        assert K.bitwise_equal(m16, m32), f"call {ci}: matched-filter rows"


# ---------------------------------------------------------------------------
# 5. mixed formats on one handle
# ---------------------------------------------------------------------------
def test_float_cs16_float_calls_on_one_handle(Q):
    sps, span, S = 4, 32, 5
    x = signal_i16(sps, span, S, seed0=70)
    n = x.shape[1] // 2
    calls = [[n // 3] * S, [n // 4 + 1] * S, [n - n // 3 - n // 4 - 1] * S]
    b = make(Q, S, sps, span, n)
    got, mfs = host_calls(Q, b, x, calls, fmt=["cf32", "cs16", "cf32"])
    assert b.status() == 0
    b.close()
    w = widened(x)
    assert_same(got, oracle_chain(w, calls, sps, span))
    assert_rows(mfs, calls, [fir_ref(rrc(sps, span), w[s]) for s in range(S)])


@pytest.mark.parametrize("sps,span", [(8, 8), (4, 32)], ids=_ids([(8, 8), (4, 32)]))
def test_nan_and_inf_in_the_history_of_a_cs16_call(Q, sps, span):
    """A float call whose last T-1 samples hold a NaN and an Inf, then a CS16
    call: its first outputs have them in their windows, so the tile kernel's
    recompute path reads the float history and the int16 row."""
    S, T = 3, sps * span + 1
    n1, n2 = 700, TILE + 300
    f = np.random.default_rng(80).standard_normal((S, 2 * n1)).astype(np.float32)
    f[0, 2 * (n1 - 5)] = np.nan                  # I of stream 0, 5 samples from the end
    f[1, 2 * (n1 - (T - 1)) + 1] = np.inf        # Q of stream 1, the oldest history sample
    f[2, 2 * (n1 - 1)] = -np.inf                 # stream 2: the newest
    f[2, 2 * (n1 - 2) + 1] = np.nan
    x = random_i16(S, n2, seed=81)
    b = make(Q, S, sps, span, n2)
    with contextlib.suppress(Q.QPSKError):       # non-finite timing: reported, rows still written
        b.process(f)
    with contextlib.suppress(Q.QPSKError):
        b.process_cs16(x)
    mf = b.last_mf(n2)
    assert b.status() & Q.STATUS_NONFINITE_TIMING
    b.close()
    h = rrc(sps, span)
    for s in range(S):
        ref = fir_ref(h, np.concatenate([f[s], widened(x[s])]))[2 * n1:]
        assert np.isnan(ref[: 2 * (T - 1)]).any() and np.isfinite(ref[2 * (T - 1):]).all()
        assert K.bitwise_equal(mf[s], ref, nan_any_payload=True), f"stream {s}"


# ---------------------------------------------------------------------------
# 6. scale
# ---------------------------------------------------------------------------
def test_scale_default_setter_and_rejections(Q):
    b = make(Q, 2, 8, 8, 256)
    assert np.float32(b.cs16_scale()) == DEFAULT_SCALE == np.float32(2.0 ** -15)
    for bad in (0.0, -1.0, -0.0, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="qpsk error -3"):   # QPSK_ERR_OUT_OF_RANGE
            b.set_cs16_scale(bad)
        assert np.float32(b.cs16_scale()) == DEFAULT_SCALE
    b.set_cs16_scale(ODD_SCALE)
    assert np.float32(b.cs16_scale()) == ODD_SCALE
    b.close()


def test_non_power_of_two_scale_bitwise(Q):
    sps, span, S = 8, 8, 5
    stage_case(Q, sps, span, "host-4098", seed=7400, scale=ODD_SCALE)
    stage_case(Q, sps, span, "device-scalar", seed=7500, scale=ODD_SCALE)
    x = signal_i16(sps, span, S, seed0=75)
    n = x.shape[1] // 2
    calls = split_calls(S, n, 2, seed=76)
    b = make(Q, S, sps, span, max(max(c) for c in calls))
    b.set_cs16_scale(ODD_SCALE)
    got, _ = host_calls(Q, b, x, calls)
    b.close()
    w = widened(x, ODD_SCALE)
    assert_same(got, oracle_chain(w, calls, sps, span))


def test_scale_change_between_pipelined_calls_applies_to_the_later_one(Q):
    """The scale is captured when a call is issued: the queued call keeps its own."""
    sps, span, S = 8, 8, 5
    x = signal_i16(sps, span, S, seed0=77)
    n = x.shape[1] // 2
    k = n // 4
    calls = [[k] * S, [k] * S, [k] * S, [n - 3 * k] * S]
    scales = [None, ODD_SCALE, None, DEFAULT_SCALE]           # set before calls 1 and 3
    per_call = [DEFAULT_SCALE, ODD_SCALE, ODD_SCALE, DEFAULT_SCALE]
    w = np.concatenate([widened(x[:, 2 * k * c: (2 * k * (c + 1) if c < 3 else 2 * n)], per_call[c])
                        for c in range(4)], axis=1)
    b = make(Q, S, sps, span, n - 3 * k)
    got, _ = device_calls(Q, b, x, calls, pipelined=True, scales=scales)
    assert b.status() == 0
    b.close()
    assert_same(got, oracle_chain(w, calls, sps, span))


# ---------------------------------------------------------------------------
# 7. FLL and IQ balancer in front (one widening pass ahead of them)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kw,okw", [
    (dict(enable_fll=True, cfo_loop_bandwidth=1e-3), dict(enable_fll=True, cfo_loop_bw=1e-3)),
    (dict(enable_fll=True, cfo_loop_bandwidth=1e-3, vector_lanes=4), dict(enable_fll=True, cfo_loop_bw=1e-3, lanes=4)),
    (dict(iq_balance=True), dict(iq_balance=True)),
    (dict(iq_balance=True, enable_fll=True, cfo_loop_bandwidth=1e-3),
     dict(iq_balance=True, enable_fll=True, cfo_loop_bw=1e-3)),
], ids=["fll-systolic", "fll-one-lane", "iq-balance", "iq-balance-fll"])
def test_fll_and_iq_balance_ragged_chunks(Q, kw, okw):
    """Ragged chunks (shorter than an 8-sample block and than the 40-tap window,
    empty ones), host calls, device calls in the 4-byte layout and pipelined calls."""
    sps, span, S = 8, 8, 7
    x = signal_i16(sps, span, S, n_bits=1200, seed0=85, cfo_hz=-3000.0)
    n = x.shape[1] // 2
    rng = np.random.default_rng(86)
    calls, used = [], np.zeros(S, np.int64)
    for c in range(7):
        lens = rng.integers(0, 50, S) if c < 5 else np.full(S, 37 + 1000 * (c - 5))
        lens[c % S] = 0
        calls.append([int(v) for v in lens])
        used += lens
    calls.append([int(n - u) for u in used])
    want = oracle_chain(widened(x), calls, sps, span, **okw)
    nmax = max(max(c) for c in calls)
    for run in (host_calls, functools.partial(device_calls, layout="scalar"),
                functools.partial(device_calls, pipelined=True)):
        b = make(Q, S, sps, span, nmax, **kw)
        got = run(Q, b, x, calls)[0]
        assert b.status() == 0
        b.close()
        assert_same(got, want)


# ---------------------------------------------------------------------------
# 8. CS16 host ring
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("depth,zero_copy", [(2, False), (3, True)], ids=["depth2-copy", "depth3-zero-copy"])
def test_cs16_host_ring_equals_consecutive_calls(Q, depth, zero_copy):
    sps, span, S = 8, 8, 4
    x = signal_i16(sps, span, S, seed0=95)
    n = x.shape[1] // 2
    calls = split_calls(S, n, 5, seed=96 + depth)
    calls.insert(3, [0] * S)
    nmax = max(max(c) for c in calls)
    ref_b = make(Q, S, sps, span, nmax + 8)
    want, _ = host_calls(Q, ref_b, x, calls)
    ref_b.close()

    b = make(Q, S, sps, span, nmax + 8)
    ring = Q.HostRing(b, depth, fmt="cs16")
    slot = ring.next_slot()
    assert slot.dtype == np.int16 and slot.shape == (S, 2 * (nmax + 8))
    pos = np.zeros(S, np.int64)
    got, pending = [], 0

    def collect():
        bits, nb, _ = ring.collect()
        got.append([(Q.unpack_bits(bits[s], int(nb[s])), None) for s in range(S)])

    for ci, lens in enumerate(calls):
        if pending == depth:
            collect()
            pending -= 1
        rows, m = call_rows(x, calls, ci, pos, np.int16)
        if zero_copy:
            slot = ring.next_slot()
            slot[:, : 2 * m] = rows
            ring.submit(None, m, lengths_of(lens))
        else:
            ring.submit(rows if m else np.zeros((S, 2), np.int16), m, lengths_of(lens))
        pending += 1
        pos += np.array(lens)
    while pending:
        collect()
        pending -= 1
    ring.close()
    b.close()
    assert_same(got, want)
    assert_same(got, oracle_chain(widened(x), calls, sps, span))


def test_ring_format_misuse_is_a_state_error(Q):
    C = Q.C
    L = Q.lib()
    b = make(Q, 2, 8, 8, 512)
    f32 = np.zeros((2, 200), np.float32)
    i16 = np.zeros((2, 200), np.int16)
    ptr, stride, t = C.c_void_p(), C.c_int64(), C.c_int64()
    ring = Q.HostRing(b, 2, fmt="cs16")
    assert L.qpsk_rx_next_slot(ring._r, C.byref(ptr), C.byref(stride)) == Q.QPSK_ERR_STATE
    assert L.qpsk_rx_submit(ring._r, f32.ctypes.data, 200, 100, None, C.byref(t)) == Q.QPSK_ERR_STATE
    with pytest.raises(ValueError):
        ring.submit(f32, 100)                    # the binding converts nothing either
    ring.submit(i16, 100)
    ring.collect()
    ring.close()
    ring = Q.HostRing(b, 2)
    assert L.qpsk_rx_next_slot_cs16(ring._r, C.byref(ptr), C.byref(stride)) == Q.QPSK_ERR_STATE
    assert L.qpsk_rx_submit_cs16(ring._r, i16.ctypes.data, 200, 100, None, C.byref(t)) == Q.QPSK_ERR_STATE
    ring.submit(f32, 100)
    ring.collect()
    ring.close()
    with pytest.raises(ValueError):
        Q.HostRing(b, 2, fmt="cu8")
    b.close()
