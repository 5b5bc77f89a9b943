"""The modulator in a radio's sample format, on the GPU: CF32 / CS16 / CS8 / CU8
rows from host and device memory, ModulateBytes from device payloads, PEAK
normalisation, and modulator rows fed to the demodulator without leaving the
device.

The reference for values is always oracle.modulate / modulate_bytes followed by
the numpy restatement of the quantiser (test_quantise_abi.quantise_ref); every
comparison has tolerance 0.  References are computed once a configuration and
shared by the formats.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import common as K
import oracle as O
import qpsk_amd
import test_quantise_abi as QA
from gpu_harness import FORMATS, Q, assert_same, decoded, dev, oracle_run, widened   # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

FULL = {"cf32": 1.0, "cs16": 32767.0, "cs8": 127.0, "cu8": 127.0}
ALL_FORMATS = ("cf32", "cs16", "cs8", "cu8")
TSC_ODD = K.TSC[:33]          # a dibit straddles the TSC / payload boundary
SENTINEL = 0x5B


def expected(rows, n_out, fmt, norm="fixed", scale=None):
    """The oracle's float rows [S, W] (zero past n_out) in fmt, row by row for
    PEAK; returns (rows of fmt, peaks or None)."""
    scale = FULL[fmt] if scale is None else scale
    if norm == "fixed":
        return QA.quantise_ref(rows.reshape(-1), fmt, "fixed", scale)[0].reshape(rows.shape), None
    out = np.zeros(rows.shape, qpsk_amd._format(fmt)[1])
    peaks = np.zeros(rows.shape[0], np.float32)
    for s, n in enumerate(n_out):
        out[s, :n], peaks[s] = QA.quantise_ref(rows[s, :n], fmt, "peak")
    return out, peaks


def assert_rows_equal(got, n_got, want, n_want, what):
    """Rows [S, W] equal up to each row's length, lengths equal, bit for bit."""
    assert np.array_equal(n_got, n_want), f"{what}: lengths differ"
    assert got.dtype == want.dtype
    w = min(got.shape[1], want.shape[1])
    assert int(n_want.max(initial=0)) <= w
    live = np.arange(w)[None, :] < np.asarray(n_want)[:, None]
    a, b = got[:, :w][live], want[:, :w][live]
    same = a.view(np.uint32) == b.view(np.uint32) if a.dtype == np.float32 else a == b
    if not same.all():
        s, i = np.argwhere((got[:, :w] != want[:, :w]) & live)[0]
        pytest.fail(f"{what}: {np.count_nonzero(~same)} elements differ, first in row {s} (length {n_want[s]}) at "
                    f"{i}: {got[s, i]!r} vs {want[s, i]!r}")


def packed_rows(strings):
    width = max((max(len(b) for b in strings) + 7) // 8, 1)
    rows = np.zeros((len(strings), width), np.uint8)
    for s, b in enumerate(strings):
        if b:
            p = qpsk_amd.pack_bits(b)
            rows[s, : p.size] = p
    return rows, np.array([len(b) for b in strings], np.int64)


def oracle_rows(strings, sps, span, alpha, diff, pulse, tsc, modulate=None):
    """The oracle's rows of the bit strings as [S, W] float32 and their lengths."""
    outs = [(modulate or O.modulate)(K.FS, K.FS // sps, b, rrc_alpha=alpha, rrc_span=span, differential=diff, tsc=tsc,
                                     pulse_shaping=pulse) for b in strings]
    n = np.array([o.size for o in outs], np.int64)
    rows = np.zeros((len(outs), max(int(n.max()), 2)), np.float32)
    for s, o in enumerate(outs):
        rows[s, : o.size] = o
    return rows, n


# ---------------------------------------------------------------------------
# 1. every row length across the kernels' block edges
# ---------------------------------------------------------------------------
# (sps, span, alpha); the second has an even T (delay rounds down), the last sps = 1
EDGE_CONFIGS = [(2, 10, 0.9), (3, 5, 0.5), (8, 8, 0.4), (1, 7, 0.5)]


@functools.lru_cache(maxsize=None)
def edge_strings(sps):
    """Stream s carries s payload bits, s = 0 ... 2 L + 3, L the larger of the
    sample kernel's tile in symbols and the symbol kernel's scan pass."""
    L = max(-(-qpsk_amd.MOD_TILE_SAMPLES // sps), qpsk_amd.MOD_SCAN_DIBITS)
    rng = np.random.default_rng(1000 + sps)
    bits = rng.integers(0, 2, (2 * L + 4, 2 * L + 3), dtype=np.uint8)
    return ["".join(map(str, bits[s, :s])) for s in range(2 * L + 4)]


@pytest.mark.parametrize("sps,span,alpha", EDGE_CONFIGS, ids=[f"sps{c[0]}" for c in EDGE_CONFIGS])
def test_every_row_length_in_every_format(Q, sps, span, alpha):
    strings = edge_strings(sps)
    rows, nb = packed_rows(strings)
    for diff in (True, False):
        m = Q.QPSKModulator(K.FS, K.FS // sps, alpha, span, differentialEncoding=diff, tsc=TSC_ODD)
        for pulse in (True, False):
            ref, n_ref = oracle_rows(strings, sps, span, alpha, diff, pulse, TSC_ODD)
            assert n_ref[0] == m.output_floats(0, pulse) > 0 and (n_ref % 2 == 0).all()
            for fmt in ALL_FORMATS:
                got, n_got = m.modulate_batch(rows, nb, pulse, fmt=fmt, scale=FULL[fmt], raw=True)
                assert_rows_equal(got, n_got, expected(ref, n_ref, fmt)[0], n_ref, f"{fmt} diff={diff} pulse={pulse}")
        m.close()


def test_fewer_than_two_bits_in_all_give_no_output(Q):
    m = Q.QPSKModulator(K.FS, K.FS // 8, K.ALPHA, 8)   # no TSC
    rows, nb = packed_rows(["", "1", "10", "101"])
    for fmt in ALL_FORMATS:
        got, n = m.modulate_batch(rows, nb, fmt=fmt, scale=FULL[fmt], raw=True)
        ref, n_ref = oracle_rows(["", "1", "10", "101"], 8, 8, K.ALPHA, True, True, None)
        assert list(n[:2]) == [0, 0] and n[2] == n[3] > 0
        assert_rows_equal(got, n, expected(ref, n_ref, fmt)[0], n_ref, fmt)
    m.close()


def test_a_filter_too_long_for_lds_reads_global_memory(Q):
    """T = 4096 (sps 585, span 7), the longest filter the oracle designs, is the
    first whose taps (8 bytes each) and quadrants exceed what a workgroup stages."""
    sps, span, alpha = 585, 7, 0.5
    assert K.FS // (K.FS // sps) == sps
    rng = np.random.default_rng(585)
    strings = [K.random_bits(rng, n) for n in (17, 2, 0, 9)]
    rows, nb = packed_rows(strings)
    m = Q.QPSKModulator(K.FS, K.FS // sps, alpha, span, tsc="011")
    ref, n_ref = oracle_rows(strings, sps, span, alpha, True, True, "011")
    assert n_ref.max() == 2 * (4095 // 2 * 2 + 10 * sps)
    for fmt in ("cf32", "cs8"):
        got, n = m.modulate_batch(rows, nb, fmt=fmt, scale=FULL[fmt], raw=True)
        assert_rows_equal(got, n, expected(ref, n_ref, fmt)[0], n_ref, fmt)
    m.close()


# ---------------------------------------------------------------------------
# 2. device rows
# ---------------------------------------------------------------------------
RAGGED_BITS = (0, 1, 2, 7, 333, 1001, 127, 128, 129, 2000)


@functools.lru_cache(maxsize=None)
def ragged(pulse=True, tsc=TSC_ODD):
    """(strings, packed rows, counts, oracle rows, oracle lengths) at sps 8, span 8."""
    rng = np.random.default_rng(22)
    strings = [K.random_bits(rng, n) for n in RAGGED_BITS]
    rows, nb = packed_rows(strings)
    ref, n_ref = oracle_rows(strings, 8, 8, K.ALPHA, True, pulse, tsc)
    return strings, rows, nb, ref, n_ref


class SentinelRows:
    """S device rows of fmt holding n_cap samples each inside one allocation
    filled with SENTINEL bytes, with a pad in front and behind: "vector" rows are
    16-byte aligned with a pitch of a multiple of 16 bytes; "scalar" rows (the
    layout of gpu_harness.device_rows) start one sample in and have a pitch of
    one sample more than a multiple of the 16-byte vector."""
    PAD = 256

    def __init__(self, torch, S, n_cap, fmt, layout):
        F = FORMATS[fmt]
        lead = res = 0 if layout == "vector" else 1
        pitch = n_cap + lead
        pitch += (res - pitch) % F.per_load
        self.dtype = np.dtype(F.np_dtype)
        self.shape = (S, 2 * pitch)
        self.lead, self.n_cap = lead, n_cap
        self.raw = torch.full((2 * self.PAD + S * 2 * pitch * self.dtype.itemsize,), SENTINEL, dtype=torch.uint8,
                              device="cuda")
        self.flat = self.raw[self.PAD: self.raw.numel() - self.PAD].view(getattr(torch, F.torch_dtype))
        self.rows = self.flat.view(S, 2 * pitch)[:, 2 * lead: 2 * (lead + n_cap)]
        assert self.rows.data_ptr() % 16 == lead * (16 // F.per_load)
        assert self.rows.stride(0) % (2 * F.per_load) == 2 * res

    def host(self):
        return self.raw.cpu().numpy()

    def expected_bytes(self, want, n_out):
        """The allocation if exactly want[s, :n_out[s]] was written."""
        body = np.full(self.shape[0] * self.shape[1] * self.dtype.itemsize, SENTINEL, np.uint8).view(self.dtype)
        body = body.reshape(self.shape)
        for s, n in enumerate(n_out):
            body[s, 2 * self.lead: 2 * self.lead + n] = want[s, :n]
        pad = np.full(self.PAD, SENTINEL, np.uint8)
        return np.concatenate([pad, body.reshape(-1).view(np.uint8), pad])


@pytest.mark.parametrize("fmt", ALL_FORMATS)
def test_device_rows_both_layouts_and_nothing_past_a_row(Q, dev, fmt):
    torch = dev
    _, rows, nb, ref, n_ref = ragged()
    want = expected(ref, n_ref, fmt)[0]
    S, n_cap = len(nb), int(n_ref.max()) // 2 + 5
    m = Q.QPSKModulator(K.FS, K.FS // 8, K.ALPHA, 8, tsc=TSC_ODD)
    bits_dev, nb_dev = torch.from_numpy(rows).cuda(), torch.from_numpy(nb).cuda()
    for layout in ("vector", "scalar"):
        out = SentinelRows(torch, S, n_cap, fmt, layout)
        n_out = torch.full((S,), -1, dtype=torch.int64, device="cuda")
        m.modulate_device(bits_dev, nb_dev, out.rows, n_out, fmt=fmt, scale=FULL[fmt])
        assert np.array_equal(n_out.cpu().numpy(), n_ref), layout
        got = out.host()
        if not np.array_equal(got, out.expected_bytes(want, n_ref)):
            bad = np.flatnonzero(got != out.expected_bytes(want, n_ref))
            pytest.fail(f"{fmt} {layout}: {bad.size} bytes of the allocation differ, first at {bad[0] - out.PAD}")
    m.close()


@pytest.mark.parametrize("fmt", ALL_FORMATS)
def test_device_rows_the_library_refuses_are_not_written(Q, dev, fmt):
    torch = dev
    _, rows, nb, ref, n_ref = ragged()
    S, n_need = len(nb), int(n_ref.max()) // 2
    m = Q.QPSKModulator(K.FS, K.FS // 8, K.ALPHA, 8, tsc=TSC_ODD)
    bits_dev, nb_dev = torch.from_numpy(rows).cuda(), torch.from_numpy(nb).cuda()
    out = SentinelRows(torch, S, n_need + 8, fmt, "vector")
    clean = out.host()
    n_out = torch.full((S,), -1, dtype=torch.int64, device="cuda")
    cases = {"misaligned": out.rows[:, 1: 1 + 2 * n_need],                    # half a sample in
             "odd stride": out.flat[: S * (2 * n_need + 1)].view(S, 2 * n_need + 1),
             "short stride": out.flat[: S * (2 * n_need - 2)].view(S, 2 * n_need - 2)}
    for what, view in cases.items():
        with pytest.raises(ValueError, match="qpsk error -1"):
            m.modulate_device(bits_dev, nb_dev, view, n_out, fmt=fmt, scale=FULL[fmt])
        torch.cuda.synchronize()
        assert np.array_equal(out.host(), clean), what
        assert (n_out.cpu().numpy() == -1).all(), what
    m.close()


def test_more_streams_than_the_grid_dimension_are_refused(Q):
    m = Q.QPSKModulator(K.FS, K.FS // 8, K.ALPHA, 8)
    with pytest.raises(ValueError, match="65535"):
        m.modulate_batch(np.zeros((65536, 1), np.uint8), np.zeros(65536, np.int64))
    assert len(m.modulate_batch(np.zeros((4, 1), np.uint8), np.full(4, 8, np.int64))) == 4   # the handle still works
    m.close()


# ---------------------------------------------------------------------------
# 3. PEAK
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["cs16", "cs8"])
def test_peak_rows_host_and_device(Q, dev, fmt):
    torch = dev
    _, rows, nb, ref, n_ref = ragged(tsc=None)
    assert n_ref[0] == 0 and n_ref[1] == 0, "an empty row is part of the batch"
    want, peaks = expected(ref, n_ref, fmt, "peak")
    assert peaks[0] == 0 and peaks[1] == 0 and (peaks[2:] > 0).all()
    m = Q.QPSKModulator(K.FS, K.FS // 8, K.ALPHA, 8)
    # host memory
    got, n = m.modulate_batch(rows, nb, fmt=fmt, norm="peak", raw=True)
    assert_rows_equal(got, n, want, n_ref, "host")
    host_peaks = m.last_peaks
    assert K.bitwise_equal(host_peaks, peaks)
    # the host quantiser on the CF32 output of the same call
    f32, n32 = m.modulate_batch(rows, nb, fmt="cf32", raw=True)
    for s in range(len(nb)):
        q, pk = Q.quantise_iq(f32[s, : n32[s]], fmt, "peak")
        assert np.array_equal(q, got[s, : n[s]]) and pk == host_peaks[s], s
        at = int(np.argmax(np.abs(f32[s, : n32[s]]))) if n32[s] else None
        assert at is None or abs(int(got[s, at])) == QA.RANGE[fmt][1]
    # device memory, both layouts
    S, n_cap = len(nb), int(n_ref.max()) // 2 + 3
    bits_dev, nb_dev = torch.from_numpy(rows).cuda(), torch.from_numpy(nb).cuda()
    for layout in ("vector", "scalar"):
        out = SentinelRows(torch, S, n_cap, fmt, layout)
        n_out = torch.zeros(S, dtype=torch.int64, device="cuda")
        peak_dev = torch.full((S,), -1.0, dtype=torch.float32, device="cuda")
        m.modulate_device(bits_dev, nb_dev, out.rows, n_out, fmt=fmt, norm="peak", peak_dev=peak_dev)
        assert np.array_equal(n_out.cpu().numpy(), n_ref)
        assert np.array_equal(out.host(), out.expected_bytes(want, n_ref)), layout
        assert K.bitwise_equal(peak_dev.cpu().numpy(), peaks), layout
    with pytest.raises(ValueError):
        m.modulate_batch(rows, nb, fmt="cf32", norm="peak")
    m.close()


# ---------------------------------------------------------------------------
# 4. ModulateBytes from device memory
# ---------------------------------------------------------------------------
START, STOP = b"MESSAGE_START", b"MESSAGE_STOP"


@functools.lru_cache(maxsize=None)
def payload_batch():
    rng = np.random.default_rng(44)
    lens = np.array([0, 1, 255, 1500], np.int64)
    pay = np.zeros((4, 1500), np.uint8)
    for s, n in enumerate(lens):
        pay[s, :n] = rng.integers(0, 256, n, dtype=np.uint8)
    outs = [O.modulate_bytes(K.FS, K.FS // 8, pay[s, :n].tobytes(), START, STOP, rrc_alpha=K.ALPHA, rrc_span=8,
                             tsc=TSC_ODD) for s, n in enumerate(lens)]
    n_ref = np.array([o.size for o in outs], np.int64)
    ref = np.zeros((4, int(n_ref.max())), np.float32)
    for s, o in enumerate(outs):
        ref[s, : o.size] = o
    return pay, lens, ref, n_ref


@pytest.mark.parametrize("fmt", ["cf32", "cs8"])
def test_modulate_bytes_from_device_payloads(Q, dev, fmt):
    torch = dev
    pay, lens, ref, n_ref = payload_batch()
    want = expected(ref, n_ref, fmt)[0]
    m = Q.QPSKModulator(K.FS, K.FS // 8, K.ALPHA, 8, tsc=TSC_ODD)
    host, n_host = m.modulate_bytes_batch(pay, lens, START, STOP, fmt=fmt, scale=FULL[fmt], raw=True)
    assert_rows_equal(host, n_host, want, n_ref, "host memory")
    out = SentinelRows(torch, 4, int(n_ref.max()) // 2 + 1, fmt, "vector")
    n_out = torch.zeros(4, dtype=torch.int64, device="cuda")
    pay_dev = torch.from_numpy(pay).cuda()
    keep = pay_dev.clone()
    m.modulate_bytes_device(pay_dev, torch.from_numpy(lens).cuda(), START, STOP, out.rows, n_out, fmt=fmt,
                            scale=FULL[fmt])
    assert np.array_equal(n_out.cpu().numpy(), n_ref)
    assert np.array_equal(out.host(), out.expected_bytes(want, n_ref)), "device memory"
    assert torch.equal(pay_dev, keep)
    one = m.ModulateBytes(pay[2, :255].tobytes(), START, STOP, fmt=fmt, scale=FULL[fmt])
    assert np.array_equal(one, want[2, : n_ref[2]])
    with pytest.raises(ValueError):
        m.modulate_bytes_batch(pay, lens, b"", STOP, fmt=fmt)
    m.close()


# ---------------------------------------------------------------------------
# 5. transmit into receive without leaving the device
# ---------------------------------------------------------------------------
def frames_found(Q, bits):
    """Of the streams' bit strings, how many give back their own text through
    the TSC search and the framer (QPSKDeModulator.DeModulateTextUtf8)."""
    found = 0
    for k, b in enumerate(bits):
        row = Q.pack_bits(b) if b else np.zeros(1, np.uint8)
        at = Q.tsc_find(row, len(b), K.TSC)
        if at < 0:
            continue
        fr = Q.Framer(1, b"\x02", b"\x03")
        got = fr.push(row[None, :], np.array([len(b)], np.int64), np.array([at], np.int64))[0]
        found += got.decode("utf-8", errors="replace").endswith(f"frame {k}: " + K.PAYLOAD)
    return found


def test_modulator_rows_go_straight_into_the_demodulator(Q, dev):
    torch = dev
    sps, span, S = 8, 8, 6
    texts = [(f"frame {k}: " + K.PAYLOAD).encode("utf-8") for k in range(S)]
    pay = np.stack([np.frombuffer(t, np.uint8) for t in texts])
    lens = np.full(S, pay.shape[1], np.int64)
    m = Q.QPSKModulator(K.FS, K.FS // sps, K.ALPHA, span, tsc=K.TSC)
    n = m.output_floats(8 * (pay.shape[1] + 2)) // 2
    pay_dev, lens_dev = torch.from_numpy(pay).cuda(), torch.from_numpy(lens).cuda()
    found = {}
    for fmt in ("cf32", "cs16", "cs8"):
        F = FORMATS[fmt]
        pitch = -(-n // F.per_load) * F.per_load
        rows = torch.zeros((S, 2 * pitch), dtype=getattr(torch, F.torch_dtype), device="cuda")
        n_out = torch.zeros(S, dtype=torch.int64, device="cuda")
        m.modulate_bytes_device(pay_dev, lens_dev, b"\x02", b"\x03", rows, n_out, fmt=fmt, scale=FULL[fmt])
        assert (n_out.cpu().numpy() == 2 * n).all()
        assert rows.data_ptr() % 16 == 0 and (rows.stride(0) * rows.element_size()) % 16 == 0   # the wide loads
        b = Q.BatchDemodulator(S, Q.params(K.FS, K.FS // sps, K.ALPHA, span, max_samples_per_call=n))
        ms = b.max_symbols(n)
        bits = torch.zeros((S, ((2 * ms + 7) // 8 + 63) // 64 * 64), dtype=torch.uint8, device="cuda")
        sy = torch.zeros((S, 2 * ms), dtype=torch.float32, device="cuda")
        nb = torch.zeros(S, dtype=torch.int64, device="cuda")
        ns = torch.zeros(S, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        b.process_device_fmt(rows, n, bits, nb, fmt, syms_dev=sy, n_syms_dev=ns)
        torch.cuda.synchronize()
        assert b.status() == 0
        b.close()
        got = decoded(Q.MODE_DEMODULATE, bits.cpu().numpy(), nb.cpu().numpy(), sy.cpu().numpy(), ns.cpu().numpy())
        x = rows[:, : 2 * n].cpu().numpy()
        w = x if fmt == "cf32" else widened(x, fmt)
        assert_same([got], oracle_run(w, [[n] * S], K.FS // sps, span), what=fmt)
        found[fmt] = frames_found(Q, [g[0] for g in got])
    m.close()
    assert found["cf32"] >= 3, found
    assert found["cs16"] >= found["cf32"] and found["cs8"] >= found["cf32"], found


# ---------------------------------------------------------------------------
# 6. the old entry points
# ---------------------------------------------------------------------------
def test_old_entry_point_equals_fmt_with_cf32_fixed_one(Q):
    _, rows, nb, ref, n_ref = ragged()
    L = Q.lib()
    m = Q.QPSKModulator(K.FS, K.FS // 8, K.ALPHA, 8, tsc=TSC_ODD)
    S, width = len(nb), int(n_ref.max())
    outs = []
    for new in (False, True):
        out = np.zeros((S, width), np.float32)
        n = np.zeros(S, np.int64)
        head = (S, rows.ctypes.data, rows.shape[1], nb.ctypes.data, 1, Q.MEM_HOST, out.ctypes.data, width, n.ctypes.data)
        rc = (L.qpsk_mod_modulate_fmt(m._h, Q.FMT_CF32, Q.NORM_FIXED, C.c_float(1.0), *head, None) if new
              else L.qpsk_mod_modulate(m._h, *head))
        assert rc == Q.QPSK_OK
        outs.append((out, n))
    (old, n_old), (new, n_new) = outs
    assert_rows_equal(new, n_new, old, n_old, "fmt vs old")
    assert_rows_equal(old, n_old, ref[:, :width], n_ref, "old vs oracle")
    m.close()


def test_old_bytes_entry_point_equals_bytes_fmt_with_cf32_fixed_one(Q):
    pay, lens, ref, n_ref = payload_batch()
    L = Q.lib()
    m = Q.QPSKModulator(K.FS, K.FS // 8, K.ALPHA, 8, tsc=TSC_ODD)
    st, en = np.frombuffer(START, np.uint8).copy(), np.frombuffer(STOP, np.uint8).copy()
    S, width = len(lens), int(n_ref.max())
    outs = []
    for new in (False, True):
        out = np.zeros((S, width), np.float32)
        n = np.zeros(S, np.int64)
        head = (S, pay.ctypes.data, pay.shape[1], lens.ctypes.data, st.ctypes.data, st.size, en.ctypes.data, en.size, 1)
        tail = (out.ctypes.data, width, n.ctypes.data)
        rc = (L.qpsk_mod_modulate_bytes_fmt(m._h, Q.FMT_CF32, Q.NORM_FIXED, C.c_float(1.0), *head, Q.MEM_HOST, *tail, None)
              if new else L.qpsk_mod_modulate_bytes(m._h, *head, *tail))
        assert rc == Q.QPSK_OK
        outs.append((out, n))
    (old, n_old), (new, n_new) = outs
    assert_rows_equal(new, n_new, old, n_old, "bytes_fmt vs old")
    assert_rows_equal(old, n_old, ref, n_ref, "old vs oracle")
    m.close()
