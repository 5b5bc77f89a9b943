"""GPU parity of the loop kernel's loader when a workgroup's matched-filter
rows lie more than 2^32 bytes apart (csrc/qpsk_loop.hip, the loader wave).

The loader's fast path addresses a round of every stream with a 32-bit byte
offset from the workgroup's first MF row.  A row is max_samples_per_call (+
prefix and slack) samples of 8 bytes, so with 32 rows of 18 M samples, or 64
rows of 9 M, the last rows are out of that reach and the loader has to serve
every round on its slow path (64-bit addresses).  Each case is one full
workgroup without shadow rows: three uniform calls of 47 rounds, in which
every round but the last would qualify for the fast path, then a ragged call.
Bits and rotated symbols are compared bitwise with the CPU oracle.

The handle allocates 4.6 GB for the MF rows and 1.2 GB more for symbol rows.
"""
import functools

import pytest

import common as K
import qpsk_amd as Q
from gpu_harness import assert_same, dev, gpu_run, oracle_run

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("dev")]

SPS, SPAN = 4, 32
SMAX = 64
# (streams, loop_variant, max_samples_per_call): streams x row bytes > 2^32
FOUR_SLOT = (32, 2, 18_000_000)
TWO_SLOT = (64, 5, 9_000_000)


def calls_for(S):
    return [[3000] * S] * 3 + [[1000 + 37 * s for s in range(S)]]


@functools.lru_cache(maxsize=None)
def case():
    """64 streams, their calls and the oracle's results; a 32-stream batch
    takes the first 32 of each (streams are independent)."""
    iq = K.batch_signals(SMAX, seed0=7100, sps=SPS, span=SPAN, n_bits=6400, snr_db=14)
    iq.setflags(write=False)
    calls = calls_for(SMAX)
    assert iq.shape[1] // 2 >= sum(max(c) for c in calls)
    return iq, oracle_run(iq, calls, K.FS // SPS, SPAN)


@pytest.mark.parametrize("want_syms", [True, False])
@pytest.mark.parametrize("S,variant,n_max", [FOUR_SLOT, TWO_SLOT], ids=["four_slot_32x64", "two_slot_64x64"])
def test_far_rows_bit_exact(S, variant, n_max, want_syms):
    # one full workgroup on the ring meant, its last row out of the 32-bit reach
    g = Q.loop_shape(variant, S, float(SPS), 256, 0, want_syms)
    assert (g["streams"], g["slots"]) == (S, 2 if variant == 5 else 4)
    assert (S - 1) * n_max * 8 >= 1 << 32
    iq, ref = case()
    got = gpu_run(iq[:S], calls_for(S), K.FS // SPS, SPAN, want_syms=want_syms, max_samples=n_max,
                  loop_variant=variant)
    assert_same(got, [res[:S] for res in ref])
