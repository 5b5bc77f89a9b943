"""CS16 (interleaved int16 I,Q) input, bit for bit, through the _cs16 entry
points.  What is checked, against what, and the staging rules per format
stand in tests/gpu_format_cases.py, which holds the cases that CS16 shares
with CS8 and CU8 (tests/test_gpu_int8.py); this file names the CS16 cases and
keeps the tests that only CS16 has.
"""
import numpy as np
import pytest

import common as K
import gpu_format_cases as cases
from gpu_format_cases import oracle_chain, stage_case
from gpu_harness import (FORMATS, SPECIALISED, TILE, Q, _ids, assert_rows, assert_same, device_calls, fir_ref,
                         host_calls, make, random_rows, rrc, signal_q, split_calls, widened)

pytestmark = pytest.mark.gpu

FMT = "cs16"


@pytest.mark.parametrize("how", ["host-4098", "host-4097", "device-vector", "device-scalar"])
@pytest.mark.parametrize("sps,span", SPECIALISED, ids=_ids(SPECIALISED))
def test_matched_filter_rows_bitwise(Q, sps, span, how):
    """Every specialised tap count over the ragged call sequence, through both stagings."""
    stage_case(sps, span, FMT, how, seed=7000)


@pytest.mark.parametrize("sps,span,lanes", [(3, 5, 8), (8, 8, 4)], ids=["T16-generic", "T65-W4"])
def test_matched_filter_generic_kernel_and_lanes_4(Q, sps, span, lanes):
    """fir_generic_kernel with an even tap count, and vector_lanes 4."""
    stage_case(sps, span, FMT, "host-4098", lanes=lanes, seed=7100)
    stage_case(sps, span, FMT, "device-scalar", lanes=lanes, seed=7200)


@pytest.mark.parametrize("sps,span", [(8, 8), (4, 32)], ids=_ids([(8, 8), (4, 32)]))
def test_device_input_layouts(Q, sps, span):
    """16-byte rows and 4-byte rows, two calls of 2049 samples: the same rows."""
    S, n = 3, TILE + 1
    h = rrc(sps, span)
    x = random_rows(S, 2 * n, 7300 + h.size, "cs16")
    refs = [fir_ref(h, widened(x[s], "cs16")) for s in range(S)]
    calls = [[n] * S] * 2
    for layout in ("vector", "scalar"):
        b = make(S, sps, span, n + 3)
        _, mfs = device_calls(b, x, calls, "cs16", layout=layout)
        b.close()
        try:
            assert_rows(mfs, calls, refs)
        except BaseException as e:
            raise AssertionError(f"layout '{layout}': {e}") from e


def test_device_rows_misaligned_or_odd_stride_are_argument_errors(Q):
    import torch
    S, n = 2, 100
    b = make(S, 8, 8, 256)
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


@pytest.mark.parametrize("S", [5, 70])
@pytest.mark.parametrize("sps,span", K.CONFIGS)
def test_chain_host_device_pipelined_chunked(Q, sps, span, S):
    cases.chain_host_device_pipelined_chunked(FMT, sps, span, S)


@pytest.mark.parametrize("trig", [0, 1], ids=["portable", "glibc"])
def test_chain_costas_trig_and_constellation_mode(Q, trig):
    cases.chain_costas_trig_and_constellation_mode(FMT, trig)


@pytest.mark.parametrize("sps,span", K.CONFIGS)
def test_equals_the_float_path_fed_the_widened_floats(Q, sps, span):
    cases.equals_the_float_path_fed_the_widened_floats(FMT, sps, span)


def test_float_cs16_float_calls_on_one_handle(Q):
    cases.mixed_format_calls_on_one_handle(FMT)


@pytest.mark.parametrize("sps,span", [(8, 8), (4, 32)], ids=_ids([(8, 8), (4, 32)]))
def test_nan_and_inf_in_the_history_of_a_cs16_call(Q, sps, span):
    cases.nan_and_inf_in_the_history_of_an_integer_call(sps, span, FMT)


def test_scale_default_setter_and_rejections(Q):
    default, odd = FORMATS[FMT].scale, FORMATS[FMT].odd_scale
    b = make(2, 8, 8, 256)
    assert np.float32(b.cs16_scale()) == default == np.float32(2.0 ** -15)
    for bad in (0.0, -1.0, -0.0, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="qpsk error -3"):   # QPSK_ERR_OUT_OF_RANGE
            b.set_cs16_scale(bad)
        assert np.float32(b.cs16_scale()) == default
    b.set_cs16_scale(odd)
    assert np.float32(b.cs16_scale()) == odd
    b.close()


def test_non_power_of_two_scale_bitwise(Q):
    sps, span, S, fmt = 8, 8, 5, "cs16"
    odd = FORMATS[fmt].odd_scale
    stage_case(sps, span, fmt, "host-4098", seed=7400, scale=odd)
    stage_case(sps, span, fmt, "device-scalar", seed=7500, scale=odd)
    x = signal_q(sps, span, S, fmt, seed0=75)
    n = x.shape[1] // 2
    calls = split_calls(S, n, 2, seed=76)
    b = make(S, sps, span, max(max(c) for c in calls))
    b.set_cs16_scale(odd)
    got, _ = host_calls(b, x, calls, fmt)
    b.close()
    assert_same(got, oracle_chain(widened(x, fmt, odd), calls, sps, span))


def test_scale_change_between_pipelined_calls_applies_to_the_later_one(Q):
    cases.scale_change_between_pipelined_calls_applies_to_the_later_one(FMT)


@pytest.mark.parametrize("front", list(cases.FRONT))
def test_fll_and_iq_balance_ragged_chunks(Q, front):
    cases.fll_and_iq_balance_ragged_chunks(FMT, front)


@pytest.mark.parametrize("depth,fill", [(2, "copy"), (3, "zero-copy")], ids=["depth2-copy", "depth3-zero-copy"])
def test_cs16_host_ring_equals_consecutive_calls(Q, depth, fill):
    cases.host_ring_equals_consecutive_calls(FMT, depth, fill)


def test_ring_format_misuse_is_a_state_error(Q):
    C = Q.C
    L = Q.lib()
    b = make(2, 8, 8, 512)
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
