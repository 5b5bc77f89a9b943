"""CS8 (int8 I,Q) and CU8 (uint8 I,Q, zero at 128) input, bit for bit, through
the format-tagged entry points.  What is checked, against what, and the
staging rules per format stand in tests/gpu_format_cases.py, which holds the
cases that the 8-bit formats share with CS16 (tests/test_gpu_cs16.py); this
file names the 8-bit cases and keeps the tests that only they have.
"""
import functools

import numpy as np
import pytest

import common as K
import gpu_format_cases as cases
from gpu_format_cases import stage_case
from gpu_harness import FORMATS, SPECIALISED, Q, _ids, as_fmt, fir_ref, make, rrc, signal_q, widened

pytestmark = pytest.mark.gpu

FMTS = ["cs8", "cu8"]


@functools.lru_cache(maxsize=None)
def every_pair():
    """One row of 65 536 samples: every (I, Q) byte pair once, shuffled."""
    k = np.random.default_rng(8000).permutation(65536).astype(np.uint32)
    row = np.stack([(k >> 8).astype(np.uint8), (k & 255).astype(np.uint8)], 1).reshape(1, -1)
    assert len({(int(a), int(c)) for a, c in row.reshape(-1, 2)}) == 65536
    row.setflags(write=False)
    return row


@pytest.mark.parametrize("scale", [None, FORMATS["cs8"].odd_scale], ids=["default-scale", "scale-1/100"])
@pytest.mark.parametrize("fmt", FMTS)
def test_every_byte_pair_bitwise(Q, fmt, scale):
    """The input domain is finite: all 65 536 (I, Q) pairs through the T = 65
    tile kernel, against fir_ref of the numpy-widened row."""
    sps, span, n = 8, 8, 65536
    x = every_pair().view(FORMATS[fmt].np_dtype)
    b = make(1, sps, span, n)
    if scale is not None:
        b.set_input_scale(fmt, scale)
    b.process_fmt(x, fmt)
    mf = b.last_mf(n)
    assert b.status() == 0
    b.close()
    ref = fir_ref(rrc(sps, span), widened(x, fmt, scale)[0])
    assert K.bitwise_equal(mf[0], ref)


@pytest.mark.parametrize("how", ["host-4098", "host-4097", "device-vector", "device-scalar"])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("sps,span", SPECIALISED, ids=_ids(SPECIALISED))
def test_matched_filter_rows_bitwise(Q, sps, span, fmt, how):
    """Every specialised tap count over the call sequence, through both stagings."""
    stage_case(sps, span, fmt, how, seed=9000)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("sps,span", [(2, 6), (2, 10)], ids=["T13", "T21"])
def test_matched_filter_rows_8_byte_aligned(Q, sps, span, fmt):
    """T - 1 = 4 mod 8: rows that are 8-byte but not 16-byte aligned take the
    8-byte (4-sample) loads."""
    stage_case(sps, span, fmt, "device-half", seed=9000)


@pytest.mark.parametrize("sps,span,lanes,fmt", [(3, 5, 8, "cu8"), (8, 8, 4, "cs8")], ids=["T16-generic", "T65-W4"])
def test_matched_filter_generic_kernel_and_lanes_4(Q, sps, span, lanes, fmt):
    """fir_generic_kernel with an even tap count, and vector_lanes 4."""
    stage_case(sps, span, fmt, "host-4098", lanes=lanes, seed=9100)
    stage_case(sps, span, fmt, "device-scalar", lanes=lanes, seed=9100)


@pytest.mark.parametrize("sps,span,S", [(2, 10, 5), (4, 32, 70)], ids=["T21-S5", "T129-S70"])
def test_chain_host_device_pipelined_chunked(Q, sps, span, S):
    cases.chain_host_device_pipelined_chunked("cs8", sps, span, S)


def test_chain_glibc_trig_and_constellation_mode(Q):
    cases.chain_costas_trig_and_constellation_mode("cs8", 1)


@pytest.mark.parametrize("fmt", FMTS)
def test_equals_the_float_path_fed_the_widened_floats(Q, fmt):
    cases.equals_the_float_path_fed_the_widened_floats(fmt, 8, 8)


def test_cf32_cs8_cs16_cu8_calls_on_one_handle(Q):
    cases.mixed_format_calls_on_one_handle("cs8")


@pytest.mark.parametrize("sps,span", [(8, 8), (4, 32)], ids=_ids([(8, 8), (4, 32)]))
def test_nan_and_inf_in_the_history_of_a_cs8_call(Q, sps, span):
    cases.nan_and_inf_in_the_history_of_an_integer_call(sps, span, "cs8")


def test_scale_defaults_setters_and_rejections(Q):
    default, odd = FORMATS["cs8"].scale, FORMATS["cs8"].odd_scale
    b = make(2, 8, 8, 256)
    for fmt in FMTS:
        assert np.float32(b.input_scale(fmt)) == default == np.float32(2.0 ** -7)
        for bad in (0.0, -1.0, -0.0, float("nan"), float("inf"), float("-inf")):
            with pytest.raises(ValueError, match="qpsk error -3"):   # QPSK_ERR_OUT_OF_RANGE
                b.set_input_scale(fmt, bad)
            assert np.float32(b.input_scale(fmt)) == default
    b.set_input_scale("cs8", odd)                                    # per format
    assert np.float32(b.input_scale("cs8")) == odd and np.float32(b.input_scale("cu8")) == default
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
    cases.scale_change_between_pipelined_calls_applies_to_the_later_one(fmt)


@pytest.mark.parametrize("fmt,front", list(zip(["cs8", "cu8", "cu8", "cs8"], cases.FRONT)), ids=list(cases.FRONT))
def test_fll_and_iq_balance_ragged_chunks(Q, fmt, front):
    cases.fll_and_iq_balance_ragged_chunks(fmt, front)


@pytest.mark.parametrize("fmt", FMTS)
def test_host_ring_equals_consecutive_calls(Q, fmt):
    cases.host_ring_equals_consecutive_calls(fmt, 3, "alternate")


def test_ring_format_misuse_is_a_state_error(Q):
    C, L = Q.C, Q.lib()
    b = make(2, 8, 8, 512)
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


def test_argument_errors(Q):
    import torch
    S, n = 2, 100
    b = make(S, 8, 8, 256)
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


@pytest.mark.parametrize("fmt", ["cs16", "cs8"])
def test_group_process_fmt_equals_one_handle(Q, fmt):
    """Two shards on device 0, host and device rows: bitwise one handle's."""
    import torch
    sps, span, S = 8, 8, 7
    x = as_fmt(signal_q(sps, span, S, "cs8", seed0=110), fmt)
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
    x = signal_q(sps, span, S, "cu8", seed0=120)[:, : 2 * 1000].copy()
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
