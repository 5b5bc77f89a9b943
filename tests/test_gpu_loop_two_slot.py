"""GPU parity of the two-slot sample ring (loop_variant 5, csrc/qpsk_loop.hip).

A row of the ring is [prefix | round][prefix | round]: the loader fills a slot
one round ahead together with the 16 samples before it, so the backlog a
stream carries into a round is read from its own slot.  Every case compares
bits and rotated symbols bitwise with the CPU oracle, through loop_variant=5
and through the automatic shape.

70 streams: more than one workgroup at 64 or 32 streams per workgroup, and the
even spread leaves every workgroup with shadow lanes.  n_bits = 2400 is 40-150
rounds of 64 or 128 samples, so both slots are refilled many times.
"""
import functools

import numpy as np
import pytest

import common as K
import oracle as O
import qpsk_amd as Q
from gpu_harness import assert_same, dev, gpu_run, oracle_run, ragged_loop_calls

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("dev")]

S = 70
VARIANTS = [5, 0]


@functools.lru_cache(maxsize=None)
def signals(sps, span, differential=True, seed0=3000):
    iq = K.batch_signals(S, seed0=seed0, sps=sps, span=span, n_bits=2400, snr_db=14, differential=differential)
    iq.setflags(write=False)
    return iq


def ragged_calls(n, seed):
    """gpu_harness.ragged_loop_calls for this module's S streams."""
    return ragged_loop_calls(S, n, seed)


@functools.lru_cache(maxsize=None)
def ragged_case(sps, span):
    iq = signals(sps, span)
    calls = ragged_calls(iq.shape[1] // 2, sps)
    return iq, calls, oracle_run(iq, calls, K.FS // sps, span)


@pytest.mark.parametrize("want_syms", [True, False])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("sps,span", [(4, 32), (8, 8)])
def test_ragged_calls_bit_exact(sps, span, variant, want_syms):
    iq, calls, ref = ragged_case(sps, span)
    assert_same(gpu_run(iq, calls, K.FS // sps, span, loop_variant=variant, want_syms=want_syms), ref)


@functools.lru_cache(maxsize=None)
def single_call_ref(sps, span, rs):
    iq = signals(sps, span)
    calls = [[iq.shape[1] // 2] * S]
    return iq, calls, oracle_run(iq, calls, rs, span)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("sps,span", [(4, 32), (8, 8)])
def test_internal_chunks_bit_exact(sps, span, variant):
    """One call run as internal chunks of about 1000 samples: the timing runs on
    in the call's coordinates (StreamState.tofs != 0)."""
    iq, calls, ref = single_call_ref(sps, span, K.FS // sps)
    assert_same(gpu_run(iq, calls, K.FS // sps, span, loop_variant=variant, max_samples=1000), ref)
    assert_same(gpu_run(iq, calls, K.FS // sps, span, loop_variant=variant, max_samples=1000,
                        want_syms=False), ref)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("sps,span,off", [(5, 8, 1.02), (5, 8, 0.98), (8, 8, 0.98)])
def test_backlog_at_its_bound_bit_exact(sps, span, off, variant):
    """The demodulator's symbol rate 2 % above / below the signal's (4.90, 5.10
    and 8.16 samples a symbol, none an integer): the loop cannot lock, so the
    symbols are noise to the TED and the streams run through the rounds out of
    step with the round size, read the prefix at its far end and run the
    per-lane catch-up loop.  The correction does not reach its +-0.1 clamp
    here: the loop filter is too narrow to get there within a row (no symbol
    at the clamp, the largest correction 0.006, measured with tests/refmodel.py
    and asserted by test_loop_cases.py::test_backlog_rows_stay_far_from_the_
    clamp).  The clamp as a steady state is tests/test_gpu_loop_edges.py's."""
    rs = int(round(K.FS / sps * off))
    iq, calls, ref = single_call_ref(sps, span, rs)
    assert_same(gpu_run(iq, calls, rs, span, loop_variant=variant), ref)
    assert_same(gpu_run(iq, calls, rs, span, loop_variant=variant, want_syms=False), ref)


@pytest.mark.parametrize("variant", VARIANTS)
def test_non_integer_sps_bit_exact(variant):
    """Symbol rate 2.3 MHz at 10 MHz: sps = 4.3478..."""
    rs, span = 2_300_000, 8
    iq, _, _ = single_call_ref(4, 32, K.FS // 4)
    n = iq.shape[1] // 2
    calls = [[n // 3] * S, [n - n // 3] * S]
    ref = _non_integer_ref(rs, span)
    assert_same(gpu_run(iq, calls, rs, span, loop_variant=variant), ref)


@functools.lru_cache(maxsize=None)
def _non_integer_ref(rs, span):
    iq = signals(4, 32)
    n = iq.shape[1] // 2
    return oracle_run(iq, [[n // 3] * S, [n - n // 3] * S], rs, span)


@pytest.mark.parametrize("variant", VARIANTS)
def test_constellation_and_non_differential_bit_exact(variant):
    iq = signals(4, 32)
    n = iq.shape[1] // 2
    calls = [[n // 2] * S, [n - n // 2] * S]
    mode = [Q.MODE_CONSTELLATION, Q.MODE_DEMODULATE]
    assert_same(gpu_run(iq, calls, K.FS // 4, 32, mode=mode, loop_variant=variant), _modes_ref()[0])
    nd = signals(4, 32, differential=False)
    assert_same(gpu_run(nd, [[nd.shape[1] // 2] * S], K.FS // 4, 32, differential=False, loop_variant=variant),
                _modes_ref()[1])


@functools.lru_cache(maxsize=None)
def _modes_ref():
    iq = signals(4, 32)
    n = iq.shape[1] // 2
    calls = [[n // 2] * S, [n - n // 2] * S]
    a = oracle_run(iq, calls, K.FS // 4, 32, mode=[Q.MODE_CONSTELLATION, Q.MODE_DEMODULATE])
    nd = signals(4, 32, differential=False)
    b = oracle_run(nd, [[nd.shape[1] // 2] * S], K.FS // 4, 32, differential=False)
    return a, b


@pytest.mark.parametrize("variant", VARIANTS)
def test_glibc_trig_bit_exact(variant):
    """costas_trig = 1 pairs lanes l and l + 32 on one stream, so it keeps a
    32-stream shape whatever loop_variant asks for; bit-exact with the libm
    oracle either way."""
    iq, calls, _ = ragged_case(4, 32)
    assert_same(gpu_run(iq, calls, K.FS // 4, 32, loop_variant=variant, costas_trig=1), _glibc_ref())


@functools.lru_cache(maxsize=None)
def _glibc_ref():
    iq, calls, _ = ragged_case(4, 32)
    return oracle_run(iq, calls, K.FS // 4, 32, trig=O.TRIG_LIBM)


def test_small_sps_falls_back_to_auto():
    """sps 2 is below the two-slot shapes' range: loop_variant 5 runs the
    automatic shape and stays bit-exact."""
    iq = signals(2, 10)
    calls = ragged_calls(iq.shape[1] // 2, 2)
    ref = oracle_run(iq, calls, K.FS // 2, 10)
    assert_same(gpu_run(iq, calls, K.FS // 2, 10, loop_variant=5), ref)
    assert_same(gpu_run(iq, calls, K.FS // 2, 10, loop_variant=5, want_syms=False), ref)
