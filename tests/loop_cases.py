"""Seeds, layouts and preconditions of the symbol-loop edge suite
(tests/test_gpu_loop_edges.py); no GPU is needed here.

The symbol loop (csrc/qpsk_loop.hip) is optimistic in three places, and all
three are decided per wave (one wave = one workgroup's streams):

  M&M      a round's uniform symbol count is voted by the wave; the capacity
           constants (CAP of every shape, lag_max, kguar, the vote thresholds)
           rest on an advance of sps -+ 0.1 per symbol held for good
  M&M      below sps 2 the output capacity (n symbols for n samples) stops a
           call; the queue then keeps more than 3 samples, and past 256 the
           stream is flagged (QPSK_STATUS_CARRY_OVERFLOW)
  Costas   the round runs a fast pass whose sincos reduction holds for
           |theta| <= 2^40 (costas_trig 1: < 0x1.921fbp+26) and is redone for
           the whole wave when one stream left that range

A well-behaved signal from a fresh state reaches none of them, so the loop
state is seeded: the records of a fresh handle's blob are overwritten
(seeded_blob) and restored with set_state, and the oracle instances get the
same fields through OracleDemod.write_state.  Every seed is a state the
reference can hold and set_state accepts (test_seeds_are_states_set_state_
accepts): pd in {+-1} or (0, 0) without has_prev, diff_p in {+-1}, mu in
[0, 1), any integ, theta, freq and ps.

Layout (S = 134 streams, as the FLL suite's ORDER): workgroup b of G =
ceil(S / streams) owns streams [b S / G, (b + 1) S / G), with 6 .. 64 streams
per workgroup depending on loop_variant.  Streams 0 .. 43 interleave the
ladder rows (pinned high / low, straddling, huge theta, decode seeds, empty
and fresh rows), 44 .. 88 are all pinned low (the largest uniform count), 89
.. 133 are plain fresh rows (the control: a wave that never redoes a round).
For every shape some workgroup is mixed, one holds only pinned-low rows, one
only control rows, and some are partly filled: the kernel spreads the batch evenly, so these lie
where the spread puts them (preconditions()).

The preconditions are conditions on the inputs.  They are computed from
tests/refmodel.py stepped one symbol at a time (and from the oracle's rows
where a NaN is asked for) and never from the code under test.
"""
import collections
import functools
import math

import numpy as np

import common as K
import oracle as O
import qpsk_amd as Q
import refmodel as M
import gpu_harness as H
from state_blobs import fresh_records, make_blob

Row = collections.namedtuple("Row", "name kind seed")

S = 134
MIXED, LOW, CONTROL = range(0, 44), range(44, 89), range(89, 134)
# sps -> (rrc span, payload bits): about 600 symbols a row
SHAPES = {2: (10, 1280), 4: (32, 1200), 5: (8, 1200), 8: (8, 1200)}
WG_STREAMS = (6, 12, 16, 24, 32, 64)   # streams per workgroup over the loop shapes

PORTABLE_LIMIT = 2.0 ** 40                       # the table reduction's range: |theta| <= 2^40
GLIBC_LIMIT = float.fromhex("0x1.921fbp+26")     # QPSK_GLIBC_SMALL_LIMIT: the fast pass holds below it
GLIBC_BRANRED = 105414350.0                      # glibc: |x| < this takes reduce_sincos, else __branred
TWO_PI = 2.0 * math.pi

# a previous symbol and decision for the rows that start with has_prev = 1
PREV = dict(has_prev=1, psi=np.float32(0.3), psq=np.float32(-0.2), pdi=np.float32(1), pdq=np.float32(-1))
MU_TOP = math.nextafter(1.0, 0.0)                # the largest mu; its float cast is 1.0f


def taps_of(sps):
    return sps * SHAPES[sps][0] + 1


def loop_variants(sps, trig):
    """One loop_variant per distinct shape qpsk_demod_loop_shape grants S
    streams at this sps (as tests/test_gpu_state.py lists its shapes), the
    automatic one first."""
    seen = {}
    for v in range(8):
        g = Q.loop_shape(v, S, float(sps), 256, trig, True, rrc_taps=taps_of(sps))
        seen.setdefault(tuple(g[k] for k in ("streams", "lanes", "round", "slots", "prefix", "cap")), v)
    return sorted(seen.values())


# (sps, costas_trig) -> loop_variants() when the layout was made: a new shape
# must be looked at (its workgroup size belongs in WG_STREAMS)
VARIANTS = {(2, 0): [0, 1, 3], (4, 0): [0, 1, 3, 5], (5, 0): [0, 1, 3, 5], (8, 0): [0, 1, 2, 3, 4, 5, 6],
            (4, 1): [0, 1, 3], (8, 1): [0, 1, 2, 3, 4, 6]}


def out_of_range(theta, trig):
    """theta is outside the Costas fast pass's range (the round is redone)."""
    a = abs(theta)
    return a >= GLIBC_LIMIT if trig else a > PORTABLE_LIMIT


# ---------------------------------------------------------------------------
# the seed ladder
# ---------------------------------------------------------------------------
def timing_rows():
    rows = [Row("integ -0.5", "low", dict(integ=-0.5, **PREV)),
            Row("integ +0.5", "high", dict(integ=0.5, **PREV)),
            Row("integ -Inf", "low", dict(integ=-math.inf, **PREV)),
            Row("integ +Inf", "high", dict(integ=math.inf, **PREV)),
            Row("integ +0.1", "straddle", dict(integ=0.1, **PREV)),
            Row("integ -0.1", "straddle", dict(integ=-0.1, **PREV)),
            Row("integ 0, has_prev 1", "fresh", dict(integ=0.0, **PREV))]
    for mu, mname in ((0.0, "0"), (MU_TOP, "1-")):
        for hp in (0, 1):
            for integ, kind in ((-0.5, "low"), (0.5, "high")):
                seed = dict(integ=integ, mu=mu, **(PREV if hp else {}))
                rows.append(Row(f"mu {mname}, has_prev {hp}, integ {integ:+}", kind, seed))
    return rows


def phase_rows(trig):
    lim = GLIBC_LIMIT if trig else PORTABLE_LIMIT
    inside = math.nextafter(lim, 0.0) if trig else lim      # the largest theta in range
    outside = lim if trig else math.nextafter(lim, math.inf)   # the smallest out of range
    rows = [Row("limit - 20, freq 2pi + 1", "cross", dict(theta=lim - 20, freq=TWO_PI + 1)),
            Row("-(limit - 20), freq -(2pi + 1)", "cross", dict(theta=-(lim - 20), freq=-(TWO_PI + 1))),
            Row("largest in range", "at", dict(theta=inside, freq=0.0)),
            Row("smallest out of range", "next", dict(theta=outside, freq=0.0)),
            Row("-(smallest out of range)", "next", dict(theta=-outside, freq=0.0)),
            Row("limit + 4096", "above", dict(theta=lim + 4096, freq=0.0)),
            Row("theta 0, freq limit / 110", "cross", dict(theta=0.0, freq=lim / 110.0))]
    if trig:
        rows += [Row("limit + 1 ulp", "next", dict(theta=math.nextafter(lim, math.inf), freq=0.0)),
                 Row("branred - 20, freq 2pi + 1", "above", dict(theta=GLIBC_BRANRED - 20, freq=TWO_PI + 1)),
                 Row("branred", "above", dict(theta=GLIBC_BRANRED, freq=TWO_PI)),
                 Row("branred - 1 ulp", "above", dict(theta=math.nextafter(GLIBC_BRANRED, 0.0), freq=TWO_PI))]
    for sign in (1.0, -1.0):
        p = math.pi
        ladder = [math.nextafter(math.nextafter(p, 0.0), 0.0), math.nextafter(p, 0.0), p,
                  math.nextafter(p, 4.0), math.nextafter(math.nextafter(p, 4.0), 4.0)]
        for i, v in enumerate(ladder):
            rows.append(Row(f"{'+' if sign > 0 else '-'}pi {i - 2:+d} ulp", "pi", dict(theta=sign * v, freq=0.0)))
    rows += [Row("theta +Inf", "nonfinite", dict(theta=math.inf, freq=0.0)),
             Row("theta -Inf", "nonfinite", dict(theta=-math.inf, freq=0.0)),
             Row("theta NaN", "nonfinite", dict(theta=math.nan, freq=0.0))]
    return rows


def decode_rows():
    rows = [Row("diff_have 0", "fresh", dict(diff_have=0))]
    for pi in (1, -1):
        for pq in (1, -1):
            rows.append(Row(f"diff_prev ({pi:+d}, {pq:+d})", "fresh",
                            dict(diff_have=1, diff_pi=np.float32(pi), diff_pq=np.float32(pq))))
    return rows


HUGE_KINDS = ("cross", "next", "above", "nonfinite")   # rows that leave the fast pass's range
EMPTY = Row("empty", "empty", {})
FRESH = Row("fresh", "fresh", {})
CONTROL_ROW = Row("control", "control", {})


@functools.lru_cache(maxsize=None)
def layout(trig):
    """The S rows.  The mixed region interleaves the timing and phase ladders
    (so a workgroup of 6 already holds pinned and huge rows), with two empty
    rows near its head; what is left of it is fresh."""
    t, p, d = timing_rows(), phase_rows(trig), decode_rows()
    # the decode seeds ride on the first +-pi rows (every case compares bits)
    at = [i for i, r in enumerate(p) if r.kind == "pi"]
    for i, dr in zip(at, d):
        p[i] = Row(f"{p[i].name}, {dr.name}", "pi", dict(p[i].seed, **dr.seed))
    mixed = []
    for i in range(max(len(t), len(p))):
        mixed += t[i: i + 1] + p[i: i + 1]
        if i in (1, 6):
            mixed.append(EMPTY)
    assert len(mixed) <= len(MIXED), len(mixed)
    mixed += [FRESH] * (len(MIXED) - len(mixed))
    low = [Row(r.name, r.kind, r.seed) for r in t if r.kind == "low"]
    rows = mixed + [low[i % len(low)] for i in range(len(LOW))] + [CONTROL_ROW] * len(CONTROL)
    assert len(rows) == S
    return tuple(rows)


def workgroups(n_streams, per_wg):
    """The kernel's even spread: [(first, end)] per workgroup."""
    g = -(-n_streams // per_wg)
    return [(b * n_streams // g, (b + 1) * n_streams // g) for b in range(g)]


# ---------------------------------------------------------------------------
# seeds into the oracle, the model and a blob
# ---------------------------------------------------------------------------
_ORACLE = dict(base="mm_base_index", mu="mm_mu", integ="mm_nco_integral", has_prev="mm_has_prev",
               theta="costas_theta", freq="costas_freq", diff_have="diff_have_prev")


def oracle_fields(seed):
    """A seed (StreamState field names) as OracleDemod.write_state's keywords."""
    out = {_ORACLE[k]: v for k, v in seed.items() if k in _ORACLE}
    if "psi" in seed:
        out["mm_prev_sample"] = (seed["psi"], seed["psq"])
    if "pdi" in seed:
        out["mm_prev_decision"] = (seed["pdi"], seed["pdq"])
    if "diff_pi" in seed:
        out["diff_prev"] = (seed["diff_pi"], seed["diff_pq"])
    assert set(seed) <= set(_ORACLE) | {"psi", "psq", "pdi", "pdq", "diff_pi", "diff_pq"}
    return out


def seed_model(mm, costas, diff, seed):
    """The same seed into refmodel's MM, Costas and decode_bits state, through
    their Python attributes."""
    f = np.float32
    mm.base = int(seed.get("base", mm.base))
    mm.mu = float(seed.get("mu", mm.mu))
    mm.integ = float(seed.get("integ", mm.integ))
    mm.has_prev = bool(seed.get("has_prev", mm.has_prev))
    if "psi" in seed:
        mm.ps = (f(seed["psi"]), f(seed["psq"]))
    if "pdi" in seed:
        mm.pd = (f(seed["pdi"]), f(seed["pdq"]))
    costas.theta = float(seed.get("theta", costas.theta))
    costas.freq = float(seed.get("freq", costas.freq))
    diff["have"] = bool(seed.get("diff_have", diff["have"]))
    if "diff_pi" in seed:
        diff["p"] = (f(seed["diff_pi"]), f(seed["diff_pq"]))


def seeded_blob(blob, taps, rows):
    """A handle's blob with rows[s].seed written over stream s's record; the
    carries, histories and delay lines stay as they are."""
    rec, carry, hist, dl = Q.state_blob_parts(blob, len(rows), taps)
    for s, row in enumerate(rows):
        for name, v in row.seed.items():
            rec[name][s] = v
    out = make_blob(rec, taps, carry, hist, dl)
    assert out[: Q.STATE_HEADER_BYTES] == blob[: Q.STATE_HEADER_BYTES] and len(out) == len(blob)
    return out


def fresh_blob(n_streams, taps):
    """What get_state returns on a new handle, built without one."""
    return make_blob(fresh_records(n_streams), taps)


# ---------------------------------------------------------------------------
# signals and call plans
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def signals(sps):
    span, n_bits = SHAPES[sps]
    iq = K.batch_signals(S, seed0=5200 + 10 * sps, sps=sps, span=span, n_bits=n_bits, snr_db=14)
    iq.setflags(write=False)
    return iq


def lengths_for(rows, n):
    """One call's lengths: n samples, none for the empty rows."""
    return [0 if r.kind == "empty" else int(n) for r in rows]


@functools.lru_cache(maxsize=None)
def plan(name, sps, trig):
    """Per-call [S] lengths.  "one": one call (also run as internal chunks);
    "ragged": 0-, 1-, 2- and 3-sample calls, streams ending in different
    rounds (gpu_harness.ragged_loop_calls); the empty rows take nothing."""
    rows, n = layout(trig), signals(sps).shape[1] // 2
    if name == "one":
        return (tuple(lengths_for(rows, n)),)
    assert name == "ragged"
    calls = H.ragged_loop_calls(S, n, seed=sps, big=n // 3)
    return tuple(tuple(0 if r.kind == "empty" else c for r, c in zip(rows, call)) for call in calls)


def state0(rows):
    return [oracle_fields(r.seed) for r in rows]


@functools.lru_cache(maxsize=None)
def reference(name, sps, trig, differential=True):
    """(outs, states) of the seeded oracle over plan(name): oracle_run's rows
    and read_state() after every call."""
    rows, states = layout(trig), []
    outs = H.oracle_run(signals(sps), [list(c) for c in plan(name, sps, trig)], K.FS // sps, SHAPES[sps][0],
                        after_call=lambda ci, dms: states.append([d.read_state() for d in dms]),
                        state0=state0(rows), trig=O.TRIG_LIBM if trig else O.TRIG_PORTABLE,
                        differential=differential)
    return outs, states


def nan_streams(outs, states):
    """The streams the oracle makes NaN: a NaN among its symbols or loop fields."""
    bad = set()
    for res, sts in zip(outs, states):
        for s, ((_, sy), st) in enumerate(zip(res, sts)):
            if np.isnan(sy).any() or any(np.isnan(st[k]) for k in ("costas_theta", "costas_freq", "mm_mu",
                                                                    "mm_nco_integral")):
                bad.add(s)
    return bad


def nonfinite_timing(states):
    """The oracle's M&M integrator went NaN in some stream: the status flag
    QPSK_STATUS_NONFINITE_TIMING is due."""
    return any(np.isnan(st["mm_nco_integral"]) for sts in states for st in sts)


# ---------------------------------------------------------------------------
# the model, stepped one symbol at a time
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gains(rs, span):
    g = O.OracleDemod(K.FS, rs, K.ALPHA, span).gains()
    return g["mm_sps"], g["kp"], g["ki"]


@functools.lru_cache(maxsize=None)
def matched(rs, span, key, s):
    """Stream s's matched-filter output over its whole row (the oracle's FIR:
    the model restates the loops, the filter has a suite of its own)."""
    x = signals(key)[s] if isinstance(key, int) else low_sps_signals(key)[s]
    h = O.OracleDemod(K.FS, rs, K.ALPHA, span).rrc_f32()
    y = H.fir_ref(h, x)
    y.setflags(write=False)
    return y


class TracedCostas(M.Costas):
    """refmodel's Costas loop that records every sincos argument."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.args = []

    def process(self, i, q):
        self.args.append(self.theta)
        return super().process(i, q)


def model_run(rs, span, y, calls, seed, portable, differential=True):
    """refmodel's MM, Costas and decode_bits over the matched-filter row y cut
    into calls, from seed.  Returns per call (bits, rotated symbols), and the
    models (the M&M's trace and the Costas arguments filled in)."""
    sps, kp, ki = gains(rs, span)
    mm = M.MM(sps, kp, ki)
    co = TracedCostas(float(rs), rs / 120.0, 0.707, portable)
    diff = {"have": False, "p": (np.float32(0), np.float32(0))}
    seed_model(mm, co, diff, seed)
    mm.trace = []
    out, pos = [], 0
    for n in calls:
        if n == 0:          # DeModulate with an empty span returns at once
            out.append(("", np.zeros(0, np.float32)))
            continue
        sy = mm.process(y[2 * pos: 2 * (pos + n)], 2 * n).reshape(-1, 2)
        rot = [co.process(a, b) for a, b in sy]
        bits, diff = M.decode_bits(rot, differential, diff)
        out.append((bits, np.array(rot, dtype=np.float32).reshape(-1)))
        pos += n
    return out, mm, co, diff


def clamp_shares(trace):
    """(clamped, unclamped) counts over the symbols that ran the TED."""
    raw = [c for _, c, _ in trace if c is not None]
    clamped = sum(1 for c in raw if abs(c) >= 0.1)
    return clamped, len(raw) - clamped


def densest_window(trace, width=64):
    """The most symbol starts any window of `width` samples holds."""
    starts = sorted(b for b, _, put in trace if put)
    best = lo = 0
    for hi, b in enumerate(starts):
        while starts[lo] <= b - width:
            lo += 1
        best = max(best, hi - lo + 1)
    return best


def window_bound(sps):
    """Symbol starts a 64-sample window must hold on a pinned-low row: more than
    the nominal rate can give, ceil(64 / (sps - 0.1))."""
    return math.ceil(64.0 / (sps - 0.1))


@functools.lru_cache(maxsize=None)
def timing_trace(sps, s, trig=0):
    rs, span = K.FS // sps, SHAPES[sps][0]
    row = layout(trig)[s]
    n = signals(sps).shape[1] // 2
    _, mm, _, _ = model_run(rs, span, matched(rs, span, sps, s), [n], {k: v for k, v in row.seed.items()
                                                                      if k not in ("theta", "freq")}, True)
    return tuple(mm.trace)


@functools.lru_cache(maxsize=None)
def phase_args(sps, s, trig):
    rs, span = K.FS // sps, SHAPES[sps][0]
    n = signals(sps).shape[1] // 2
    _, _, co, _ = model_run(rs, span, matched(rs, span, sps, s), [n], layout(trig)[s].seed, not trig)
    return tuple(co.args)


@functools.lru_cache(maxsize=None)
def preconditions(sps, trig):
    """Assert that the layout reaches what it is for at this sps; returns the
    figures (for the tests to print)."""
    rows = layout(trig)
    fig = {}
    # --- placement, for every workgroup size
    for per in WG_STREAMS:
        wgs = workgroups(S, per)
        kinds = [{rows[s].kind for s in range(a, b)} for a, b in wgs]
        assert any({"low", "high"} <= k and k & set(HUGE_KINDS) for k in kinds), f"{per}: no mixed workgroup"
        assert any("empty" in k and k & set(HUGE_KINDS) for k in kinds), f"{per}: no empty row beside a huge one"
        assert any(k == {"low"} for k in kinds), f"{per}: no workgroup of pinned-low rows only"
        assert any(k == {"control"} for k in kinds), f"{per}: no control workgroup"
        # the kernel spreads the batch evenly: the partly filled workgroups
        # (shadow lanes) lie where the spread puts them, not at the end
        assert min(b - a for a, b in wgs) < per, f"{per}: every workgroup is full"
    # --- timing
    starts = 0
    for s, row in enumerate(rows):
        if row.kind in ("low", "high"):
            tr = timing_trace(sps, s)
            clamped, free = clamp_shares(tr)
            assert free == 0 and clamped > 400, f"stream {s} ({row.name}): {free} unclamped steps of {clamped + free}"
            sign = {(c > 0) for _, c, _ in tr if c is not None}
            assert sign == {row.kind == "high"}, f"stream {s}: both clamps"
            if row.kind == "low" and s in LOW:
                starts = max(starts, densest_window(tr))
        elif row.kind == "straddle":
            clamped, free = clamp_shares(timing_trace(sps, s))
            fig[f"straddle {row.name}"] = (clamped, free)
            assert min(clamped, free) >= 0.2 * (clamped + free), f"stream {s} ({row.name}): {clamped} / {free}"
    fig["starts in 64 samples"] = starts
    assert starts >= window_bound(sps), f"{starts} symbol starts in a 64-sample window, want {window_bound(sps)}"
    # --- phase
    for s, row in enumerate(rows):
        if row.kind not in ("cross", "at", "next", "above"):
            continue
        out = [out_of_range(t, trig) for t in phase_args(sps, s, trig)]
        fig[f"{row.name}"] = (sum(out), len(out))
        if row.kind == "cross":
            assert 20 <= sum(out) <= len(out) - 20, f"stream {s} ({row.name}): {sum(out)} of {len(out)} out of range"
            assert not out[0] and out[-1]
        elif row.kind == "at":
            assert not any(out), f"stream {s} ({row.name}): out of range"
        elif row.kind == "next":
            assert out[0] and not all(out), f"stream {s} ({row.name})"
        elif row.name.startswith("limit +"):
            assert all(out), f"stream {s} ({row.name}): back in range"
        else:
            assert any(out)
    outs, states = reference("one", sps, trig)
    nan = nan_streams(outs, states)
    want = {s for s, r in enumerate(rows) if r.kind == "nonfinite"}
    assert nan == want, f"NaN streams {sorted(nan)} vs the non-finite seeds {sorted(want)}"
    assert all(np.isnan(outs[0][s][1]).all() for s in want)
    assert not nonfinite_timing(states)
    return fig


# ---------------------------------------------------------------------------
# below sps 2: the 16 x 64 "any" shape, the capacity stop, the carry overflow
# ---------------------------------------------------------------------------
LS = 40                                 # three workgroups of 16: 13, 13 and 14 streams
LOW_SPS = {"sps 1": (K.FS, 8), "sps 1.5": (6_666_667, 8)}    # symbol rate in Hz, rrc span
LOW_CALL = 300
LOW_CALLS = 12


@functools.lru_cache(maxsize=None)
def low_sps_layout():
    head = [Row("integ -0.5", "low", dict(integ=-0.5, **PREV)), FRESH,
            Row("integ +0.5", "high", dict(integ=0.5, **PREV)), EMPTY,
            Row("integ -0.1", "straddle", dict(integ=-0.1, **PREV)),
            Row("integ -0.5, has_prev 0", "low", dict(integ=-0.5)),
            Row("integ -Inf, mu 1-", "low", dict(integ=-math.inf, mu=MU_TOP, **PREV)),
            Row("diff_prev (-1, +1)", "fresh", dict(diff_have=1, diff_pi=np.float32(-1), diff_pq=np.float32(1))),
            Row("limit - 20, freq 2pi + 1", "cross", dict(theta=PORTABLE_LIMIT - 20, freq=TWO_PI + 1))]
    rows = head + [FRESH] * (13 - len(head))
    rows += [Row("integ -0.5", "low", dict(integ=-0.5, **PREV))] * 13 + [CONTROL_ROW] * 14
    assert len(rows) == LS
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def low_sps_signals(key):
    """Plain noise (below two samples a symbol there is no pulse to shape)."""
    rng = np.random.default_rng(77 + len(key))
    x = (0.5 * rng.standard_normal((LS, 2 * LOW_CALL * LOW_CALLS))).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def low_sps_plan(name):
    """"uniform": LOW_CALLS calls of LOW_CALL samples; "ragged": the same total
    in calls of other lengths per stream (0 .. 3 samples among them)."""
    rows = low_sps_layout()
    if name == "uniform":
        return tuple(tuple(lengths_for(rows, LOW_CALL)) for _ in range(LOW_CALLS))
    assert name == "ragged"
    sizes = [1, 300, 2, 299, 3, 0, 301, 64, 257, 150, 63, 320]
    total = LOW_CALL * LOW_CALLS
    calls, left, k = [], np.full(LS, total), 0
    while left.max() > 0 and len(calls) < 16:
        c = [int(min(left[s], sizes[(k + s) % len(sizes)])) for s in range(LS)]
        calls.append(tuple(0 if r.kind == "empty" else v for r, v in zip(rows, c)))
        left -= np.array(c)
        k += 1
    return tuple(calls)


@functools.lru_cache(maxsize=None)
def low_sps_reference(key, name):
    """(outs, states, overflow): the seeded oracle over the plan, and per stream
    the first call after which its queue holds more than 256 samples (None:
    never).  From that call on the kernel's record is no state of the reference
    (include/qpsk_demod.h), so the stream is compared no further."""
    rs, span = LOW_SPS[key]
    rows, states = low_sps_layout(), []
    outs = H.oracle_run(low_sps_signals(key), [list(c) for c in low_sps_plan(name)], rs, span,
                        after_call=lambda ci, dms: states.append([d.read_state() for d in dms]),
                        state0=state0(rows))
    over = [next((ci for ci, sts in enumerate(states) if sts[s]["mm_buf_count"] > Q.STATE_CARRY_MAX), None)
            for s in range(LS)]
    return outs, states, over


@functools.lru_cache(maxsize=None)
def low_sps_trace(key, s):
    rs, span = LOW_SPS[key]
    calls = [c[s] for c in low_sps_plan("uniform")]
    _, mm, _, _ = model_run(rs, span, matched(rs, span, key, s), calls, low_sps_layout()[s].seed, True)
    return tuple(mm.trace)


@functools.lru_cache(maxsize=None)
def low_sps_preconditions(key):
    rs, _ = LOW_SPS[key]
    sps = K.FS / rs
    rows = low_sps_layout()
    kinds = [{rows[s].kind for s in range(a, b)} for a, b in workgroups(LS, 16)]
    assert {"low", "high", "empty", "cross"} <= kinds[0] and kinds[1] == {"low"} and kinds[2] == {"control"}
    outs, states, over = low_sps_reference(key, "uniform")
    calls = low_sps_plan("uniform")
    fig = {"overflow": over}
    stopped = 0
    for s, row in enumerate(rows):
        n_syms = [res[s][1].size // 2 for res in outs]
        if row.kind == "low":
            tr = low_sps_trace(key, s)
            clamped, free = clamp_shares(tr)
            assert free == 0, f"stream {s}: {free} unclamped steps"
            fig["starts in 64 samples"] = max(fig.get("starts in 64 samples", 0), densest_window(tr))
        if sps == 1.0 and row.kind == "low":
            # the capacity stop's extra TED update: one traced symbol a call is not put out
            assert sum(1 for _, _, put in tr if not put) == LOW_CALLS, f"stream {s}: calls stopped at capacity"
            assert n_syms == [c[s] for c in calls], f"stream {s}: not every call stops at capacity"
            # 0.9 samples a symbol: 30 more of every 300 stay queued
            assert over[s] == math.ceil(Q.STATE_CARRY_MAX / (0.1 * LOW_CALL)) - 1 == 8, f"stream {s}: {over[s]}"
        stopped += any(k == c[s] and k for k, c in zip(n_syms, calls))
    assert fig["starts in 64 samples"] >= window_bound(sps), fig
    fig["streams stopped at capacity"] = stopped
    if sps == 1.0:
        assert stopped >= 30, f"{stopped} streams stop at capacity"
        assert all(o is None for s, o in enumerate(over) if rows[s].kind in ("control", "fresh", "empty", "high"))
        # a fresh stream stops at capacity too, and its queue keeps more than 3 samples
        assert max(st["mm_buf_count"] for sts in states for st in sts[26:]) > 3
    else:
        assert all(o is None for o in over), "no overflow at sps 1.5"
    assert over.count(None) >= 14
    return fig
