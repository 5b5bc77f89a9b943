"""The symbol loop (csrc/qpsk_loop.hip) on the paths where its optimistic code
is wrong: the M&M at its +-0.1 timing clamp as a steady state, the output
capacity stop and the carry overflow below sps 2, the Costas fast pass at,
just under and just over its range beside quiet streams of the same wave, and
loop records the loop did not write itself.

One device reaches all of them: the loop state is seeded (tests/loop_cases.py:
the seed ladder, the placement of its rows over the workgroups of every loop
shape, and the preconditions, which are asserted from the reference model
alone before the device is touched).  After every call the bits, n_bits, the
rotated symbols, n_syms and the whole state blob are compared with the seeded
oracle as bit patterns; NaN payloads are let go only on the rows the oracle
makes NaN, and status() is 0 wherever the oracle's timing stays a number.
"""
import functools

import numpy as np
import pytest

import common as K
import oracle as O
import qpsk_amd as Q
import gpu_harness as H
import loop_cases as LC
from gpu_harness import dev

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("dev")]

S = LC.S


taps_of = LC.taps_of
TIMING = [(sps, v) for sps in (2, 4, 5, 8) for v in LC.VARIANTS[sps, 0]]
GLIBC = [(sps, v) for sps in (4, 8) for v in LC.VARIANTS[sps, 1]]
PLANS = ["one", "ragged", "chunks", "pipelined"]


@pytest.fixture(scope="module", autouse=True)
def inputs_reach_their_edges():
    """Before the device is touched: the conditions on the inputs."""
    for sps in LC.SHAPES:
        LC.preconditions(sps, 0)
    for sps in (4, 8):
        LC.preconditions(sps, 1)
    for key in LC.LOW_SPS:
        LC.low_sps_preconditions(key)


def seed_handle(b, taps, rows):
    """Overwrite the fresh handle's records with the rows' seeds."""
    blob = LC.seeded_blob(b.get_state(), taps, rows)
    b.set_state(blob)
    assert b.get_state() == blob


def run_plan(plan, sps, trig, variant, want_syms, differential=True, rows=None):
    """The layout's rows (or rows) through plan on a seeded handle, every call
    against the seeded oracle: outputs, state blob (after every synchronous
    call, at the end of a pipelined run) and status."""
    span, taps, rs = LC.SHAPES[sps][0], taps_of(sps), K.FS // sps
    name = "one" if plan == "chunks" else "ragged" if plan == "pipelined" else plan
    rows = rows or LC.layout(trig)
    x, calls = LC.signals(sps), [list(c) for c in LC.plan(name, sps, trig)]
    want, states = LC.reference(name, sps, trig, differential) if rows is LC.layout(trig) else quiet_reference(sps, trig)
    nan = LC.nan_streams(want, states)
    knobs = dict(loop_variant=variant, costas_trig=trig, differential=differential)
    what = f"sps {sps} variant {variant} {plan}"
    if plan == "pipelined":
        def finish(b):
            H.assert_state(b.get_state(), states[-1], sps, span, f"{what}, at the end", nan_rows=nan)
            assert b.status() == 0
        got, _ = H.async_run(x, calls, sps, span, prepare=lambda b: seed_handle(b, taps, rows), finish=finish,
                             want_syms=want_syms, **knobs)
        H.assert_same(got, want, what=what, nan_rows=nan)
        return got
    n_max = max(max(c) for c in calls)
    b = H.make(S, sps, span, 1000 if plan == "chunks" else n_max + 8, **knobs)
    got = []
    try:
        seed_handle(b, taps, rows)
        pos = np.zeros(S, np.int64)
        for ci, lens in enumerate(calls):
            got.append(H.host_call(b, H.call_rows(x, lens, pos), H.lengths_of(lens), want_syms=want_syms))
            pos += np.array(lens)
            H.assert_same(got[-1:], want[ci: ci + 1], what=f"{what}, call {ci}:", nan_rows=nan)
            H.assert_state(b.get_state(), states[ci], sps, span, f"{what}, after call {ci}", nan_rows=nan)
        assert b.status() == (Q.STATUS_NONFINITE_TIMING if LC.nonfinite_timing(states) else 0)
    finally:
        b.close()
    return got


# ---------------------------------------------------------------------------
# 1. pinned and straddling timing (the phase and decode seeds ride along)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("want_syms", [True, False], ids=["syms", "bits-only"])
@pytest.mark.parametrize("sps,variant", TIMING)
def test_timing_at_the_clamp_bit_exact(sps, variant, want_syms, plan):
    """sps exactly 2, 4 and 8 are the low edge of a capacity class each: a
    pinned-low row advances sps - 0.1 a symbol for the whole row, and one
    workgroup holds such rows only, so the wave's uniform count is the largest
    the class's CAP has to take.  The portable-trig phase ladder is part of
    the same batch: the Costas redo runs on every one of these shapes."""
    run_plan(plan, sps, 0, variant, want_syms)


def test_non_differential_decode_of_the_ladder():
    run_plan("ragged", 4, 0, 0, True, differential=False)
    run_plan("one", 8, 0, 0, False, differential=False)


# ---------------------------------------------------------------------------
# 2. the Costas range with glibc's sincos; the control workgroup
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("plan", ["one", "ragged"])
@pytest.mark.parametrize("want_syms", [True, False], ids=["syms", "bits-only"])
@pytest.mark.parametrize("sps,variant", GLIBC)
def test_costas_range_glibc_trig_bit_exact(sps, variant, want_syms, plan):
    """costas_trig = 1: the ladder around 0x1.921fbp+26, where the fast pass
    ends, and around 105414350, where glibc itself changes its reduction."""
    run_plan(plan, sps, 1, variant, want_syms)


def quiet_rows(trig):
    """The layout with every row that leaves the fast pass's range made fresh."""
    return tuple(LC.FRESH if r.kind in LC.HUGE_KINDS else r for r in LC.layout(trig))


@functools.lru_cache(maxsize=None)
def quiet_reference(sps, trig):
    rows, states = quiet_rows(trig), []
    outs = H.oracle_run(LC.signals(sps), [list(c) for c in LC.plan("one", sps, trig)], K.FS // sps,
                        LC.SHAPES[sps][0], state0=LC.state0(rows), trig=O.TRIG_LIBM if trig else O.TRIG_PORTABLE,
                        after_call=lambda ci, dms: states.append([d.read_state() for d in dms]))
    return outs, states


@pytest.mark.parametrize("sps,trig,variant", [(4, 0, 0), (4, 0, 5), (8, 0, 0), (4, 1, 0)])
def test_quiet_rows_redone_equal_quiet_rows_not_redone(sps, trig, variant):
    """The same batch with and without its huge rows: every quiet row (the
    control workgroup's, and the quiet neighbours of a huge row, which the redo
    recomputes on the full-range path) comes out the same, bit for bit."""
    rows = LC.layout(trig)
    with_huge = run_plan("one", sps, trig, variant, True)
    without = run_plan("one", sps, trig, variant, True, rows=quiet_rows(trig))
    quiet = [s for s, r in enumerate(rows) if r.kind not in LC.HUGE_KINDS]
    assert len(quiet) >= S - 14 and set(LC.CONTROL) <= set(quiet)
    for s in quiet:
        assert with_huge[0][s][0] == without[0][s][0], f"stream {s} ({rows[s].name}): bits"
        assert K.bitwise_equal(with_huge[0][s][1], without[0][s][1]), f"stream {s} ({rows[s].name}): symbols"


# ---------------------------------------------------------------------------
# 3. sps in [1, 2): the capacity stop and the carry overflow
# ---------------------------------------------------------------------------
def low_handle(key, n_max):
    rs, span = LC.LOW_SPS[key]
    b = Q.BatchDemodulator(LC.LS, Q.params(K.FS, rs, K.ALPHA, span, max_samples_per_call=n_max + 8))
    taps = b.rrc_taps().size
    seed_handle(b, taps, LC.low_sps_layout())
    return b, taps


def assert_low_state(blob, ostates, taps, rows, what):
    """The tap count is the handle's (sps 1.5 designs its filter at 2 samples a symbol)."""
    H.assert_state(blob, ostates, None, None, what, rows=rows, taps=taps)


@pytest.mark.parametrize("plan", ["uniform", "ragged"])
@pytest.mark.parametrize("key", list(LC.LOW_SPS))
def test_below_sps_2_device_calls(dev, key, plan):
    """Device-memory calls report through status(): 0 until the call at which
    the oracle's queue passes 256 samples, CARRY_OVERFLOW at that call.  The
    streams that have not overflowed stay bit-exact to the end (at least two
    calls further), state and carry included; an overflowed stream carries
    error bit 0 in its record from its call on and is compared no further."""
    torch = dev
    rows, x = LC.low_sps_layout(), LC.low_sps_signals(key)
    calls = [list(c) for c in LC.low_sps_plan(plan)]
    want, states, over = LC.low_sps_reference(key, plan)
    first = min((o for o in over if o is not None), default=None)
    assert first is None or first + 2 < len(calls)
    n_max = max(max(c) for c in calls)
    b, taps = low_handle(key, n_max)
    ms = max(b.max_symbols(n_max), 1)
    pos = np.zeros(LC.LS, np.int64)
    try:
        for ci, lens in enumerate(calls):
            n = int(max(lens))
            xd = torch.from_numpy(np.ascontiguousarray(H.call_rows(x, lens, pos))).to("cuda") if n else \
                torch.zeros((LC.LS, 2), dtype=torch.float32, device="cuda")
            bits = torch.zeros((LC.LS, ((2 * ms + 7) // 8 + 63) // 64 * 64), dtype=torch.uint8, device="cuda")
            sy = torch.zeros((LC.LS, 2 * ms), dtype=torch.float32, device="cuda")
            nb = torch.zeros(LC.LS, dtype=torch.int64, device="cuda")
            ns = torch.zeros(LC.LS, dtype=torch.int64, device="cuda")
            # (the device-memory entry point that takes per-stream lengths)
            b.process_device_async(xd, n, bits, nb, syms_dev=sy, n_syms_dev=ns, lengths=H.lengths_of(lens))
            b.pipeline_wait()
            torch.cuda.synchronize()
            pos += np.array(lens)
            got = H.decoded(Q.MODE_DEMODULATE, bits.cpu().numpy(), nb.cpu().numpy(), sy.cpu().numpy(),
                            ns.cpu().numpy())
            good = [s for s in range(LC.LS) if over[s] is None or ci < over[s]]
            for s in good:
                assert got[s][0] == want[ci][s][0], f"{key} call {ci} stream {s} ({rows[s].name}): bits"
                assert K.bitwise_equal(got[s][1], want[ci][s][1]), f"{key} call {ci} stream {s}: symbols"
            blob = b.get_state()
            assert_low_state(blob, states[ci], taps, good, f"{key} after call {ci}")
            err = Q.state_blob_parts(blob, LC.LS, taps)[0]["error"]
            assert [s for s in range(LC.LS) if err[s] & 1] == [s for s in range(LC.LS) if s not in good], \
                f"{key} after call {ci}: error bits {np.flatnonzero(err).tolist()}"
            status = b.status()
            if first is None or ci < first:
                assert status == 0, f"{key} call {ci}: status {status} before any overflow is due"
            elif any(o == ci for o in over):
                assert status == Q.STATUS_CARRY_OVERFLOW, f"{key} call {ci}: status {status}"
            else:
                assert status & ~Q.STATUS_CARRY_OVERFLOW == 0
    finally:
        b.close()


def test_carry_overflow_fails_the_host_call_it_happens_in(dev):
    """sps 1, 300-sample host calls: eight calls return and match the oracle,
    the ninth returns QPSK_ERR_STATE; status() has CARRY_OVERFLOW, and the
    record's error bit 0 and the link-statistics row's sticky error are set
    for the overflowed streams only."""
    key = "sps 1"
    rows, x = LC.low_sps_layout(), LC.low_sps_signals(key)
    calls = [list(c) for c in LC.low_sps_plan("uniform")]
    want, states, over = LC.low_sps_reference(key, "uniform")
    first = min(o for o in over if o is not None)
    assert first == 8
    b, taps = low_handle(key, LC.LOW_CALL)
    b.enable_link_stats()
    pos = np.zeros(LC.LS, np.int64)
    try:
        for ci in range(first):
            got = H.host_call(b, H.call_rows(x, calls[ci], pos), H.lengths_of(calls[ci]))
            pos += np.array(calls[ci])
            H.assert_same([got], want[ci: ci + 1], what=f"host call {ci}:")
            assert_low_state(b.get_state(), states[ci], taps, None, f"after host call {ci}")
            assert not b.link_stats()["error"].any()
        assert b.status() == 0
        with pytest.raises(Q.QPSKError, match=f"qpsk error {Q.QPSK_ERR_STATE}:.*256"):
            H.host_call(b, H.call_rows(x, calls[first], pos), H.lengths_of(calls[first]))
        assert b.status() == Q.STATUS_CARRY_OVERFLOW
        hit = [s for s in range(LC.LS) if over[s] == first]
        assert len(hit) >= 15 and all(rows[s].kind in ("low", "straddle") for s in hit)
        err = b.stream_states()["error"]
        assert [s for s in range(LC.LS) if err[s] & 1] == hit
        assert [s for s in range(LC.LS) if b.link_stats()["error"][s]] == hit
        assert_low_state(b.get_state(), states[first], taps, [s for s in range(LC.LS) if s not in hit],
                         "after the failed call")
    finally:
        b.close()
