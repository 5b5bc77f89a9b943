"""The Band-Edge FLL where its optimistic block is wrong: the IEEERemainder
phase wrap, the frequency clamp, stored states the first step of a call must
take as they are, a -0 phase, overflowing band powers.

qpsk_fll.hip runs each 8-sample block branch-free and redoes it exactly when a
stream of the wave needed the wrap (Band-Edge Filter.cs:185-189), the clamp
(:191-195) or started from a -0 phase; the one-lane kernel (qpsk_kernels.hip)
has its own wrap and clamp.  Unit-amplitude signals never clamp and wrap a few
times per million samples, so these cases scale the input until most samples
do both.

Reference: per stream one standalone O.OracleFLL, built as OracleDemod builds
its own (QPSKDeModulator.cs:35), stepped ONE SAMPLE AT A TIME with its state
read after each, then the reference matched filter (fir_ref) over its output,
and the oracle chain (oracle_run) for bits and symbols.  After EVERY call:
last_mf rows, bits, symbols, and the handle's fll_phase / fll_freq
(stream_states()) against the oracle's state at that sample, all as bit
patterns.  The FLL's output is not readable through the ABI and the matched
filter never emits -0, so the state compare is what shows a wrong wrap or
clamp at once.

Every precondition (how often each row wraps and clamps, the -0 the
remainder returns) is computed from the oracle alone and asserted before the
GPU is touched; the unmarked tests assert them without a GPU.

Two things the oracle showed while the cases were built.  A clamped stream
turns by max_freq per sample, so a block that clamps nearly always wraps as
well, and the redo is decided per wave: with the ten ladder rows in one wave
and a half the kernel without the frequency term of its redo ballot still
passed.  The ladder therefore also places its two 1e3 rows among quiet rows
only, and freq_only_blocks() counts, from the oracle, the blocks in which the
clamp alone decides.  And at amplitude 1e20 these rows do not overflow the
band powers yet; the overflow case adds rows at 1e21 (error +-Inf) and 1e22
(error NaN).

Stored states (set_state): no phase or frequency is rejected --
qpsk_demod_set_state checks the blob's header and length and the fields the
kernels use as addresses (qpsk_state_blob_check: carry_n, fll_pos, tofs, the
flags, base, mu), never a float that is data -- so every listed phase and
frequency, NaN and Inf included, is run.
"""
import copy
import functools

import numpy as np
import pytest

import common as K
import oracle as O
from gpu_harness import Q, call_rows, fir_ref, is_neg_zero, oracle_run, rrc

gpu = pytest.mark.gpu

TWO_PI = np.float32(2.0) * np.float32(3.14159274101257324219)   # Band-Edge Filter.cs: 2f * MathF.PI
BW = 1e-3                                                       # cfo_loop_bandwidth of the ladder
CONFIGS = [(8, 8), (4, 32)]
# amplitude of ladder row r; odd rows swap I and Q
AMPS = [1, 8, 64, 64, 1e3, 1e3, 3e4, 3e4, 1e18, 1e-3]
# stream position -> ladder row.  A wave of the systolic kernel holds 8
# streams, two per 16-lane DPP row (even / odd), and decides the redo per wave.
#   wave 0: every kind of row.  Quiet rows 0, 1 and 9 each share a DPP row with
#           a loud one (4, 2, 8) and are recomputed with it; row 8 wraps at
#           every sample, so every block of this wave is redone.
#   wave 1, wave 2: row 4 (even DPP lane), row 5 (odd) among quiet rows only.
#           A clamped stream turns by max_freq per sample, so nearly every
#           block that clamps also wraps; here the rare blocks in which the
#           clamp alone asks for the redo are not hidden by a neighbour's wrap
#           (freq_only_blocks counts them).
#   wave 3: rows 5 and 7 in a partly filled wave (the masked path).
ORDER = [0, 4, 2, 1, 9, 8, 6, 3,
         4, 0, 1, 9, 0, 1, 9, 0,
         1, 5, 9, 0, 1, 9, 0, 1,
         5, 7]


def u32(v):
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)


def max_freq(sps):
    return TWO_PI * (np.float32(2.0) / np.float32(sps))         # Band-Edge Filter.cs:58


def oracle_fll(sps, bw, lanes=8):
    """The FLL as OracleDemod builds it: integer fs / rs, 40 taps, portable trig."""
    return O.OracleFLL(float(K.FS // (K.FS // sps)), K.ALPHA, 40, float(np.float32(bw)), lanes=lanes,
                       trig=O.TRIG_PORTABLE)


def trace(fll, row, state0=(0.0, 0.0), shadow=None):
    """Step fll over row one sample at a time: (output [2n], states [n + 1, 2],
    steps [n]); states[t] is (phase, freq) before sample t, states[n] the final
    one.  shadow: a second FLL of the same design, put at (phase before, 0)
    ahead of every sample, so that it mixes and filters the same samples and
    its frequency afterwards is this sample's beta * error (clamped):
    steps[t]."""
    n = row.size // 2
    out = np.zeros(2 * n, np.float32)
    st = np.zeros((n + 1, 2), np.float32)
    steps = np.zeros(n, np.float32)
    st[0] = state0
    for t in range(n):
        if shadow is not None:
            shadow.set_state(st[t, 0], 0.0)
            shadow.process(row[2 * t: 2 * t + 2])
            steps[t] = shadow.state()[1]
        out[2 * t: 2 * t + 2] = fll.process(row[2 * t: 2 * t + 2])
        st[t + 1] = fll.state()
    return out, st, steps


def events(st, sps):
    """(wraps, samples clamped at +max, at -max) of a state trace: a wrap is
    |phase before + freq after| > 2 pi, in float32."""
    with np.errstate(invalid="ignore", over="ignore"):
        wraps = int(np.count_nonzero(np.abs(st[:-1, 0] + st[1:, 1]) > TWO_PI))
    return wraps, int(np.count_nonzero(st[1:, 1] == max_freq(sps))), int(np.count_nonzero(st[1:, 1] == -max_freq(sps)))


class Case:
    """Inputs in stream order and the oracle's answers for them."""

    def __init__(self, rows, sps, span, bw, lanes, feed=None, state0=None, shadow=False):
        self.rows = rows                       # what the handle is fed (any format)
        feed = rows if feed is None else feed  # the float samples the FLL sees
        self.feed = feed
        self.sps, self.span, self.bw, self.lanes = sps, span, bw, lanes
        S = rows.shape[0]
        self.fll_out, self.states = [], []
        self.true_wrap, self.true_clamp = [], []
        done = {}
        for s in range(S):
            key = (feed[s].tobytes(), None if state0 is None else u32(state0[s]).tobytes())
            if key in done:                    # the same row again (a neighbour in another wave)
                for v in (self.fll_out, self.states, self.true_wrap, self.true_clamp):
                    v.append(v[done[key]])
                continue
            done[key] = s
            f = oracle_fll(sps, bw, lanes)
            s0 = (0.0, 0.0)
            if state0 is not None:
                s0 = state0[s]
                f.set_state(*s0)
            y, st, steps = trace(f, feed[s], s0, oracle_fll(sps, bw, lanes) if shadow else None)
            self.fll_out.append(y)
            self.states.append(st)
            # what the kernel's optimistic block sees: the frequency before the
            # clamp, f + beta * error, and the phase before the wrap, both exact
            # where the step itself is not at the clamp (there: counted as a wrap)
            sat = np.abs(steps) == max_freq(sps)
            with np.errstate(invalid="ignore", over="ignore"):
                fu = st[:-1, 1] + steps
                self.true_wrap.append((np.abs(st[:-1, 0] + fu) > TWO_PI) | sat)
                self.true_clamp.append((np.abs(fu) > max_freq(sps)) & ~sat)
        self.mf = [fir_ref(rrc(sps, span), y, lanes) for y in self.fll_out]
        self.events = [events(st, sps) for st in self.states]


def swap_iq(row):
    return np.ascontiguousarray(row.reshape(-1, 2)[:, ::-1]).reshape(-1)


@functools.lru_cache(maxsize=None)
def ladder_base(sps, span):
    """The ten ladder rows before scaling (odd rows with I and Q swapped), in ladder order."""
    iq = K.batch_signals(10, seed0=1200, sps=sps, span=span, n_bits=700, cfo_hz=-3000.0, snr_db=22)
    rows = np.stack([swap_iq(iq[r]) if r & 1 else iq[r] for r in range(10)])
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def ladder_case(sps, span, lanes):
    """A1's case, with its preconditions asserted from the oracle alone."""
    base = ladder_base(sps, span)
    rows = np.stack([base[r] * np.float32(AMPS[r]) for r in ORDER])
    assert rows.dtype == np.float32
    c = Case(rows, sps, span, BW, lanes, shadow=True)
    ev = {r: c.events[p] for p, r in enumerate(ORDER)}          # by ladder row
    assert all(np.isfinite(y).all() for y in c.fll_out), "an FLL output is not finite"
    assert sum(e[0] >= 100 for e in ev.values()) >= 3, ev
    assert sum(e[1] >= 400 for e in ev.values()) >= 3, ev
    assert sum(e[2] >= 400 for e in ev.values()) >= 3, ev
    assert sum(e == (0, 0, 0) for e in ev.values()) >= 2, ev
    # the rows the stream order is built around
    n = rows.shape[1] // 2
    for quiet in (0, 1, 9):
        assert ev[quiet] == (0, 0, 0), (quiet, ev[quiet])
    assert ev[8][1] + ev[8][2] >= n - 1, ("row 8 clamps at every sample but at most one", ev[8])
    assert ev[2][0] >= 100, ev[2]
    for loud in (4, 5):
        assert ev[loud][0] >= 100 and ev[loud][1] >= 400 and ev[loud][2] >= 400, (loud, ev[loud])
    return c


def ragged(S, n, seed):
    """Per-call [S] lengths: calls shorter than an 8-sample block, shorter than
    the 40-tap window, streams sitting calls out, then one long call of the rest."""
    rng = np.random.default_rng(seed)
    plan = [(1, 8), (0, 50), (8, 40), (0, 50), (1, 8), (0, 50), (37, 38), (37, 38)]
    calls, used = [], np.zeros(S, np.int64)
    for c, (lo, hi) in enumerate(plan):
        lens = rng.integers(lo, hi, S)
        lens[c % S] = 0
        if c == 3:
            lens[::2] = 0
        if not lens.any():
            lens[(c + 1) % S] = 5
        calls.append([int(v) for v in lens])
        used += lens
    assert (used < n - 200).all()
    calls.append([int(n - u) for u in used])
    return calls


def freq_only_blocks(c, calls):
    """Blocks of the last (long) call, in full waves, in which no stream of the
    wave wraps and one exceeds max_freq at the block's last sample only: the
    optimistic block equals the exact one up to there, so the frequency term
    of the redo ballot alone decides, and without it the next block would
    start from the unclamped frequency."""
    S = c.rows.shape[0]
    start = [sum(call[s] for call in calls[:-1]) for s in range(S)]
    last = calls[-1]
    total = 0
    for w0 in range(0, S - S % 8, 8):
        for t0 in range(0, min(last[w0: w0 + 8]) - 7, 8):
            hit = False
            for s in range(w0, w0 + 8):
                a = start[s] + t0
                tc = c.true_clamp[s][a: a + 8]
                if c.true_wrap[s][a: a + 8].any() or tc[:7].any():
                    break
                hit |= bool(tc[7])
            else:
                total += hit
    return total


def ladder_calls(sps, span, lanes):
    c = ladder_case(sps, span, lanes)
    calls = ragged(c.rows.shape[0], c.rows.shape[1] // 2, seed=19 + sps + lanes)
    # the systolic kernel's blocks (lanes 8).  At sps 4 max_freq is pi: a
    # clamped stream wraps within two samples, and the frequency term never
    # decides alone
    if sps == 8 and lanes == 8:
        assert freq_only_blocks(c, calls) >= 4, freq_only_blocks(c, calls)
    return c, calls


def same_floats(got, want, nan_ok):
    return K.bitwise_equal(np.asarray(got, np.float32), np.asarray(want, np.float32), nan_any_payload=nan_ok)


def drive(Q, b, case, calls, process, chain=None, nan_rows=(), may_raise=False):
    """Run calls on handle b; after every call compare each stream's last_mf
    row, FLL state and (chain: oracle_run's rows) bits and symbols.  nan_rows:
    streams compared under the NaN rule (NaN where the reference has NaN,
    payloads aside).  may_raise: a host call that met a non-finite value in the
    timing loop raises after the kernels ran; its bits are then not compared.
    Returns the number of calls that raised."""
    S = case.rows.shape[0]
    pos = np.zeros(S, np.int64)
    raised = 0
    for ci, lens in enumerate(calls):
        x = call_rows(case.rows, lens, pos)
        n = x.shape[1] // 2
        res = None
        try:
            res = process(x, np.array(lens, np.int64))
        except Q.QPSKError as e:
            assert may_raise and "non-finite" in str(e), f"call {ci}: {e}"
            raised += 1
        mf = b.last_mf(n)
        st = b.stream_states()
        pos += np.array(lens)
        for s in range(S):
            nan_ok = s in nan_rows
            k = lens[s]
            ph, fr = case.states[s][pos[s]]
            for name, g, w in (("fll_freq", st["fll_freq"][s], fr), ("fll_phase", st["fll_phase"][s], ph)):
                assert same_floats([g], [w], nan_ok), (
                    f"call {ci} stream {s} after {pos[s]} samples: {name} {g!r} (0x{int(u32([g])[0]):08x}) vs "
                    f"{w!r} (0x{int(u32([w])[0]):08x})")
            got, want = mf[s, : 2 * k], case.mf[s][2 * (pos[s] - k): 2 * pos[s]]
            if not same_floats(got, want, nan_ok):
                bad = np.flatnonzero((u32(got) != u32(want)) & ~(np.isnan(got) & np.isnan(want) & nan_ok))
                pytest.fail(f"call {ci} stream {s} (n = {k}): {bad.size} matched-filter floats differ, first at "
                            f"output {bad[0] // 2}: {got[bad[0]]!r} vs {want[bad[0]]!r}")
            if not nan_ok:
                assert not is_neg_zero(got).any(), f"call {ci} stream {s}: -0 in the matched filter"
            if chain is not None and res is not None and not nan_ok:
                bits, nb, syms, ns = res
                wb, ws = chain[ci][s]
                assert Q.unpack_bits(bits[s], int(nb[s])) == wb, f"call {ci} stream {s}: bits"
                assert K.bitwise_equal(syms[s, : 2 * int(ns[s])], ws), f"call {ci} stream {s}: symbols"
    return raised


# ---------------------------------------------------------------------------
# preconditions, without a GPU
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [8, 4])
@pytest.mark.parametrize("sps,span", CONFIGS)
def test_ladder_rows_wrap_and_clamp_in_the_oracle(sps, span, lanes):
    ladder_calls(sps, span, lanes)


def test_cs8_rows_at_scale_one_wrap_and_clamp_in_the_oracle():
    cs8_case(8, 8)


def test_overflowing_row_is_nan_in_the_oracle():
    overflow_case()


def test_stored_state_cases_in_the_oracle():
    for order in STORED_CALLS.values():
        stored_case(tuple(order))


# ---------------------------------------------------------------------------
# A1. amplitude ladder
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("lanes", [8, 4], ids=["systolic", "one-lane"])
@pytest.mark.parametrize("sps,span", CONFIGS)
def test_amplitude_ladder_through_wrap_and_clamp(Q, sps, span, lanes):
    c, calls = ladder_calls(sps, span, lanes)
    S, n = c.rows.shape[0], c.rows.shape[1] // 2
    chain = oracle_run(c.rows, calls, K.FS // sps, span, enable_fll=True, cfo_loop_bw=BW, lanes=lanes)
    b = Q.BatchDemodulator(S, Q.params(K.FS, K.FS // sps, K.ALPHA, span, max_samples_per_call=n, enable_fll=True,
                                       cfo_loop_bandwidth=BW, vector_lanes=lanes))
    drive(Q, b, c, calls, lambda x, lens: b.process(x, lengths=lens, want_syms=True), chain=chain)
    assert b.status() == 0
    b.close()


# ---------------------------------------------------------------------------
# A1b. uniform calls across the block paths
# ---------------------------------------------------------------------------
# The systolic kernel runs one register-window block wherever all 8 streams of
# a wave have 8 samples: as a call's first block, in its main loop (nmin >= 56,
# 32 samples an iteration while t0 + 48 <= nmin) and behind it.  The ladder's
# ragged lengths reach the blocks outside the main loop only in waves where
# nearly every block is redone, so here every call has one length for all
# streams, and a quiet and a mixed wave stand next to the loud one.
#   wave 0: ORDER's first wave, every block redone
#   wave 1: quiet rows, never redone
#   wave 2: mixed, the amplitude-64 rows 2 and 3 wrap now and then
#   wave 3: partly filled, the ring step throughout
EDGE_ORDER = ORDER[:8] + [0, 1, 9, 0, 1, 9, 0, 1] + [1, 2, 9, 0, 1, 9, 0, 3] + [5, 7]
# the smallest lengths that cross each edge: 56 is the first that enters the
# main loop, 88 and 120 its second and third iteration, and the +-1 neighbours
# put 0 or 1 ragged samples and 2 or 5 uniform blocks behind it
EDGE_LENS = [8, 16, 55, 56, 57, 87, 88, 89, 120, 121, 7]
MIXED_WAVE = 2


def block_position(n, t0):
    """Where the kernel runs the full block at t0 of a uniform call of n samples."""
    if t0 == 0:
        return "first"
    end = 8
    if n >= 56:
        while True:
            end += 32
            if end + 48 > n:
                break
    return "loop" if t0 < end else "tail"


@functools.lru_cache(maxsize=None)
def edge_case(sps, span):
    """(case, calls, counts, mixed): the ladder's oracle rows in EDGE_ORDER, the
    uniform calls, and the full blocks of the short calls in the three full
    waves counted as counts[position] = [fast, redone] (redone: a stream of the
    wave wraps or clamps in the block); mixed = that of wave 2's "loop" blocks.
    The preconditions are asserted here, from the oracle alone."""
    c0 = ladder_case(sps, span, 8)
    at = [ORDER.index(r) for r in EDGE_ORDER]
    c = copy.copy(c0)
    c.rows = c.feed = c0.rows[at]
    for name in ("fll_out", "states", "true_wrap", "true_clamp", "mf", "events"):
        setattr(c, name, [getattr(c0, name)[p] for p in at])
    S, n = c.rows.shape[0], c.rows.shape[1] // 2
    assert n - sum(EDGE_LENS) >= 200
    calls = [[k] * S for k in EDGE_LENS + [n - sum(EDGE_LENS)]]
    counts = {pos: [0, 0] for pos in ("first", "loop", "tail")}
    mixed = [0, 0]
    start = 0
    for k in EDGE_LENS:
        for w in range(3):
            for t0 in range(0, k - 7, 8):
                a = start + t0
                redone = any(c.true_wrap[s][a: a + 8].any() or c.true_clamp[s][a: a + 8].any()
                             for s in range(8 * w, 8 * w + 8))
                pos = block_position(k, t0)
                counts[pos][redone] += 1
                if w == MIXED_WAVE and pos == "loop":
                    mixed[redone] += 1
        start += k
    for pos, (fast, redone) in counts.items():
        assert fast >= 10 and redone >= 10, (pos, counts)
    assert mixed[0] >= 1 and mixed[1] >= 1, mixed
    return c, calls, counts, mixed


@pytest.mark.parametrize("sps,span", CONFIGS)
def test_uniform_calls_reach_every_block_path_in_the_oracle(sps, span):
    """The oracle's [fast, redone] counts: sps 8 first [19, 11], loop [98, 58],
    tail [46, 23], mixed wave's loop [46, 6]; sps 4 first [15, 15], loop
    [60, 96], tail [33, 36], mixed wave's loop [8, 44]."""
    edge_case(sps, span)


@gpu
@pytest.mark.parametrize("sps,span", CONFIGS)
def test_uniform_calls_across_the_block_paths(Q, sps, span):
    c, calls, _, _ = edge_case(sps, span)
    S, n = c.rows.shape[0], c.rows.shape[1] // 2
    chain = oracle_run(c.rows, calls, K.FS // sps, span, enable_fll=True, cfo_loop_bw=BW, lanes=8)
    b = Q.BatchDemodulator(S, Q.params(K.FS, K.FS // sps, K.ALPHA, span, max_samples_per_call=n, enable_fll=True,
                                       cfo_loop_bandwidth=BW, vector_lanes=8))
    drive(Q, b, c, calls, lambda x, lens: b.process(x, lengths=lens, want_syms=True), chain=chain)
    assert b.status() == 0
    b.close()


# ---------------------------------------------------------------------------
# A2. integer input at scale 1
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cs8_case(sps, span):
    base = ladder_base(sps, span)
    q = np.round(base * (64.0 / np.abs(base).max(axis=1, keepdims=True))).astype(np.int8)
    assert np.abs(q.astype(np.int16)).max() == 64
    c = Case(q, sps, span, BW, 8, feed=q.astype(np.float32) * np.float32(1.0))   # widened: exact integers
    assert any(e[0] >= 100 for e in c.events), c.events
    assert any(e[1] + e[2] >= 1 for e in c.events), c.events
    return c


@gpu
def test_cs8_at_scale_one_lives_in_the_redo_path(Q):
    sps, span = 8, 8
    c = cs8_case(sps, span)
    S, n = c.rows.shape[0], c.rows.shape[1] // 2
    calls = ragged(S, n, seed=21)
    chain = oracle_run(c.feed, calls, K.FS // sps, span, enable_fll=True, cfo_loop_bw=BW)
    b = Q.BatchDemodulator(S, Q.params(K.FS, K.FS // sps, K.ALPHA, span, max_samples_per_call=n, enable_fll=True,
                                       cfo_loop_bandwidth=BW))
    b.set_input_scale("cs8", 1.0)
    assert b.input_scale("cs8") == 1.0
    drive(Q, b, c, calls, lambda x, lens: b.process_fmt(x, "cs8", lengths=lens, want_syms=True), chain=chain)
    assert b.status() == 0
    b.close()


# ---------------------------------------------------------------------------
# A3. overflowing power
# ---------------------------------------------------------------------------
# stream -> amplitude, in one full wave next to normal rows (4 and 5 share a DPP
# row, 6 shares one with 7).  At 1e20 these rows (peak 0.54) do
# not overflow the band powers yet (the band-edge filters pass a fraction of
# the signal): the row stays finite and clamps at every sample.  At 1e21 a
# power is Inf while the other is finite, so the error is +-Inf: the reference's
# phase += freq + 0 * error is NaN, the kernel's phase += freq is +-Inf and the
# wrap of the same step makes it NaN (file comment of qpsk_fll.hip).  At 1e22
# both powers are Inf and the error NaN at once.
HUGE = {5: 1e20, 4: 1e21, 6: 1e22}
BAD = (4, 6)


@functools.lru_cache(maxsize=None)
def overflow_case():
    rows = ladder_base(8, 8).copy()
    for s, amp in HUGE.items():
        rows[s] = rows[s] * np.float32(amp)
    assert np.isfinite(rows).all()
    c = Case(rows, 8, 8, BW, 8)
    n = rows.shape[1] // 2
    assert np.isfinite(c.fll_out[5]).all() and c.events[5][1] + c.events[5][2] >= n - 1, c.events[5]
    for s in BAD:
        first = int(np.flatnonzero(np.isnan(c.states[s][:, 0]))[0])
        assert first < 16, (s, first)
        assert np.isnan(c.states[s][first:, 0]).all() and np.isnan(c.fll_out[s][2 * first:]).all(), s
        assert np.isnan(c.mf[s]).any()
        # +-Inf error: the frequency is clamped (finite) in the step that makes the phase NaN
        assert (abs(c.states[s][first, 1]) == max_freq(8)) == (s == 4), (s, c.states[s][first])
    assert all(np.isfinite(c.fll_out[s]).all() for s in range(rows.shape[0]) if s not in BAD)
    return c


@gpu
def test_overflowing_band_powers_next_to_normal_rows(Q):
    c = overflow_case()
    sps, span = 8, 8
    S, n = c.rows.shape[0], c.rows.shape[1] // 2
    calls = ragged(S, n, seed=31)
    # the chain of the finite rows; the oracle's timing loop throws on a NaN
    # row (tests/test_gpu_scale.py::test_oracle_follows_dotnet_nan_timing)
    dms = {s: K.oracle_for(sps, span, enable_fll=True, cfo_loop_bw=BW) for s in range(S) if s not in BAD}
    pos, chain = np.zeros(S, np.int64), []
    for lens in calls:
        res = []
        for s in range(S):
            res.append(dms[s].demodulate_ex(c.rows[s, 2 * pos[s]: 2 * (pos[s] + lens[s])])[:2] if s not in BAD else None)
        pos += np.array(lens)
        chain.append(res)
    b = Q.BatchDemodulator(S, Q.params(K.FS, K.FS // sps, K.ALPHA, span, max_samples_per_call=n, enable_fll=True,
                                       cfo_loop_bandwidth=BW))
    raised = drive(Q, b, c, calls, lambda x, lens: b.process(x, lengths=lens, want_syms=True), chain=chain,
                   nan_rows=BAD, may_raise=True)
    assert raised >= 1
    # as the non-FLL tests (test_gpu_scale.py::test_nonfinite_samples_in_the_matched_filter)
    assert b.status() & Q.STATUS_NONFINITE_TIMING
    assert b.status() == 0          # cleared by the read
    b.close()


# ---------------------------------------------------------------------------
# A4. stored states
# ---------------------------------------------------------------------------
F32 = np.float32
STORED_PHASES = [F32(-0.0),
                 TWO_PI, np.nextafter(TWO_PI, F32(np.inf)), np.nextafter(TWO_PI, F32(0)),
                 -TWO_PI, -np.nextafter(TWO_PI, F32(np.inf)), -np.nextafter(TWO_PI, F32(0)),
                 F32(100), F32(119.9), F32(121), F32(1e6), F32(3e38), F32(np.inf), F32(np.nan)]
STORED_CALLS = {"short-calls": [1, 7, 8, 9, 50], "long-call-first": [120, 1, 7]}


def stored_freqs(sps):
    return [max_freq(sps), -max_freq(sps), F32(10), F32(-10), F32(-0.0), F32(np.nan)]


@functools.lru_cache(maxsize=None)
def stored_case(order):
    """Every stored phase with every stored frequency over ordinary signal
    rows, then the stream whose first sample wraps to -0: phase -2 * (2 pi),
    freq -0, a row of zeros (equal band powers)."""
    sps, span = 8, 8
    total = sum(order)
    sig = K.batch_signals(5, seed0=1300, sps=sps, span=span, n_bits=200, cfo_hz=-3000.0, snr_db=22)
    state0 = [(p, f) for p in STORED_PHASES for f in stored_freqs(sps)]
    rows = [np.roll(sig[k % 5], -2 * 11 * k)[: 2 * total] for k in range(len(state0))]
    state0.append((F32(-2.0) * TWO_PI, F32(-0.0)))
    rows.append(np.zeros(2 * total, np.float32))
    rows = np.stack(rows).astype(np.float32)
    c = Case(rows, sps, span, 1e-4, 8, state0=state0)
    z = c.states[-1]
    assert u32(z[1, 0]) == 0x80000000, "remainderf(-2 * 2pi, 2pi) is -0 after the first sample"
    nan = [s for s in range(len(state0)) if not np.isfinite(c.fll_out[s]).all()]
    assert len(nan) >= len(STORED_PHASES) + 2 * (len(stored_freqs(sps)) - 1)   # every NaN freq, Inf and NaN phase
    assert len(state0) - len(nan) >= 50
    return c


@gpu
@pytest.mark.parametrize("order", list(STORED_CALLS), ids=list(STORED_CALLS))
def test_first_step_takes_stored_states_as_they_are(Q, order):
    """No chain bits: the oracle's chain has no setter.  With "short-calls" the
    -0 stream's first call ends on the sample that wrapped to -0, so the stored
    0x80000000 is compared and the next call starts from it."""
    lens = STORED_CALLS[order]
    c = stored_case(tuple(lens))
    sps, span = 8, 8
    S = c.rows.shape[0]
    b = Q.BatchDemodulator(S, Q.params(K.FS, K.FS // sps, K.ALPHA, span, max_samples_per_call=max(lens),
                                       enable_fll=True))
    blob = bytearray(b.get_state())
    st = np.frombuffer(blob, dtype=Q.STREAM_STATE_DTYPE, count=S, offset=Q.STATE_HEADER_BYTES)
    for s in range(S):
        st["fll_phase"][s], st["fll_freq"][s] = c.states[s][0]
    b.set_state(bytes(blob))
    back = b.stream_states()
    for s in range(S):   # nothing rejected, nothing canonicalised
        assert same_floats([back["fll_phase"][s], back["fll_freq"][s]], c.states[s][0], True), s
    drive(Q, b, c, [[k] * S for k in lens], lambda x, ln: b.process(x, lengths=ln, want_syms=True),
          nan_rows=tuple(range(S)), may_raise=True)
    assert b.status() & Q.STATUS_NONFINITE_TIMING   # the NaN and Inf states reach the timing loop
    b.close()
