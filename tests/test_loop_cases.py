"""The symbol-loop edge suite's inputs, without a GPU (tests/loop_cases.py).

  * every seed is a state set_state accepts (qpsk_state_blob_check on the host)
  * the seeded oracle (OracleDemod.write_state) equals tests/refmodel.py seeded
    through its Python attributes: bits, rotated symbols and end state over a
    ragged call sequence, tolerance 0, with the portable and the libm sincos.
    The two restatements were compared from fresh state only before
  * the layouts reach what they are for (the preconditions the GPU suite
    asserts again before it touches the device)
"""
import numpy as np
import pytest

import common as K
import oracle as O
import qpsk_amd as Q
import gpu_harness as H
import loop_cases as LC


def distinct(rows):
    seen = {}
    for s, r in enumerate(rows):
        seen.setdefault(r.name, s)
    return sorted(seen.values())


@pytest.mark.parametrize("trig", [0, 1])
def test_seeds_are_states_set_state_accepts(trig):
    sps, (span, _) = 4, LC.SHAPES[4]
    taps = sps * span + 1
    rows = LC.layout(trig)
    blob = LC.seeded_blob(LC.fresh_blob(LC.S, taps), taps, rows)
    Q.state_blob_check(Q.params(K.FS, K.FS // sps, K.ALPHA, span), LC.S, blob)
    rec = Q.state_blob_parts(blob, LC.S, taps)[0]
    for s, r in enumerate(rows):
        # values the reference can hold
        assert (rec["pdi"][s], rec["pdq"][s]) == (0, 0) and not rec["has_prev"][s] or \
            {abs(rec["pdi"][s]), abs(rec["pdq"][s])} == {1.0}, r.name
        assert not rec["diff_have"][s] or {abs(rec["diff_pi"][s]), abs(rec["diff_pq"][s])} == {1.0}, r.name
        assert 0.0 <= rec["mu"][s] < 1.0 and rec["base"][s] == 1 and rec["carry_n"][s] == 0
    kinds = {r.kind for r in rows}
    assert {"low", "high", "straddle", "fresh", "cross", "at", "next", "above", "pi", "nonfinite", "empty",
            "control"} == kinds
    assert np.float32(LC.MU_TOP) == np.float32(1.0) and LC.MU_TOP < 1.0
    rows = LC.low_sps_layout()
    for key, (rs, span) in LC.LOW_SPS.items():
        taps = Q.design(Q.params(K.FS, rs, K.ALPHA, span))[0].size
        Q.state_blob_check(Q.params(K.FS, rs, K.ALPHA, span), LC.LS,
                           LC.seeded_blob(LC.fresh_blob(LC.LS, taps), taps, rows))


def assert_model_equals_oracle(rs, span, x, y, calls, seed, trig, nan_ok, what):
    dm = O.OracleDemod(K.FS, rs, K.ALPHA, span, trig=O.TRIG_LIBM if trig else O.TRIG_PORTABLE)
    dm.write_state(**LC.oracle_fields(seed))
    outs, mm, co, diff = LC.model_run(rs, span, y, calls, seed, portable=not trig)
    pos = 0
    for ci, n in enumerate(calls):
        bits, syms, _ = dm.demodulate_ex(x[2 * pos: 2 * (pos + n)])
        pos += n
        assert bits == outs[ci][0], f"{what}, call {ci}: bits"
        assert K.bitwise_equal(syms, outs[ci][1], nan_any_payload=nan_ok), f"{what}, call {ci}: symbols"
    st = dm.read_state()
    f4, f8 = np.float32, np.float64
    want = [("mm_base_index", mm.base, None), ("mm_has_prev", int(mm.has_prev), None),
            ("mm_buf_count", mm.buf.shape[0], None), ("diff_have_prev", int(diff["have"]), None),
            ("mm_mu", mm.mu, f8), ("mm_nco_integral", mm.integ, f8), ("costas_theta", co.theta, f8),
            ("costas_freq", co.freq, f8), ("mm_prev_sample", mm.ps, f4), ("mm_prev_decision", mm.pd, f4),
            ("diff_prev", diff["p"], f4), ("mm_queue", mm.buf, f4)]
    for name, v, dt in want:
        if dt is None:
            assert int(st[name]) == int(v), f"{what}: {name} {st[name]} vs {v}"
        else:
            assert H.same_bits(st[name], v, dt, nan_ok), f"{what}: {name} {st[name]!r} vs {v!r}"


@pytest.mark.parametrize("trig", [0, 1], ids=["portable", "libm"])
def test_seeded_oracle_equals_the_seeded_model(trig):
    sps, (span, _) = 4, LC.SHAPES[4]
    rows, x = LC.layout(trig), LC.signals(sps)
    plan = LC.plan("ragged", sps, trig)
    for s in distinct(rows):
        calls = [c[s] for c in plan]
        assert rows[s].kind == "empty" or len([c for c in calls if c]) >= 4
        assert_model_equals_oracle(K.FS // sps, span, x[s], LC.matched(K.FS // sps, span, sps, s), calls,
                                   rows[s].seed, trig, rows[s].kind == "nonfinite", f"stream {s} ({rows[s].name})")


@pytest.mark.parametrize("key", list(LC.LOW_SPS))
@pytest.mark.parametrize("trig", [0, 1], ids=["portable", "libm"])
def test_seeded_oracle_equals_the_seeded_model_below_sps_2(key, trig):
    """The capacity stop's extra TED update and a queue of hundreds of samples
    are in this compare (sps 1); the 16-call ragged plan holds 0 .. 3-sample calls."""
    rs, span = LC.LOW_SPS[key]
    rows, x = LC.low_sps_layout(), LC.low_sps_signals(key)
    for s in distinct(rows):
        calls = [c[s] for c in LC.low_sps_plan("ragged")]
        assert_model_equals_oracle(rs, span, x[s], LC.matched(rs, span, key, s), calls, rows[s].seed, trig, False,
                                   f"{key} stream {s} ({rows[s].name})")


@pytest.mark.parametrize("trig", [0, 1], ids=["portable", "glibc"])
@pytest.mark.parametrize("sps", list(LC.SHAPES))
def test_layout_reaches_the_clamp_the_windows_and_the_ranges(sps, trig):
    print(LC.preconditions(sps, trig))


@pytest.mark.parametrize("key", list(LC.LOW_SPS))
def test_low_sps_rows_stop_at_capacity_and_overflow_where_computed(key):
    print(LC.low_sps_preconditions(key))


def test_ragged_plan_has_its_short_calls():
    for sps in LC.SHAPES:
        calls = LC.plan("ragged", sps, 0)
        n = LC.signals(sps).shape[1] // 2
        for s, row in enumerate(LC.layout(0)):
            mine = [c[s] for c in calls]
            assert sum(mine) == (0 if row.kind == "empty" else n)
        assert {0, 1, 2, 3} <= {v for c in calls for v in c}
        assert len({tuple(c) for c in calls}) == len(calls) >= 9


def test_variant_lists_are_the_shapes_granted():
    sizes = set()
    for (sps, trig), vs in LC.VARIANTS.items():
        assert LC.loop_variants(sps, trig) == vs, (sps, trig)
        for v in vs:
            g = Q.loop_shape(v, LC.S, float(sps), 256, trig, True, rrc_taps=LC.taps_of(sps))
            sizes.add(g["streams"])
    assert sizes == set(LC.WG_STREAMS)
    for rs, span in LC.LOW_SPS.values():   # below sps 2 every variant runs the 16 x 64 shape of 80 slots
        for v in range(8):
            g = Q.loop_shape(v, LC.LS, K.FS / rs, 256, 0, True, rrc_taps=17)
            assert (g["streams"], g["round"], g["cap"]) == (16, 64, 80)


@pytest.mark.parametrize("sps,span,off", [(5, 8, 1.02), (5, 8, 0.98), (8, 8, 0.98)])
def test_backlog_rows_stay_far_from_the_clamp(sps, span, off):
    """What test_gpu_loop_two_slot.test_backlog_at_its_bound_bit_exact's
    docstring says of its streams, from the model: with the symbol rate 2 % off
    no symbol's correction comes near +-0.1 (measured: at most 0.006)."""
    import test_gpu_loop_two_slot as T
    rs = int(round(K.FS / sps * off))
    iq = T.signals(sps, span)
    h = O.OracleDemod(K.FS, rs, K.ALPHA, span).rrc_f32()
    for s in (0, T.S // 2, T.S - 1):
        _, mm, _, _ = LC.model_run(rs, span, H.fir_ref(h, iq[s]), [iq.shape[1] // 2], {}, True)
        raw = [abs(c) for _, c, _ in mm.trace if c is not None]
        assert len(raw) > 1100 and LC.clamp_shares(mm.trace)[0] == 0 and max(raw) < 0.01, (s, max(raw))
