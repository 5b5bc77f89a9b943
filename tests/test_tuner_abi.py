"""The tuner's host half (qpsk_tuner_*, csrc/qpsk_tuner.cpp) without a GPU: the
exports, the design and the oscillator's tables against their formulas bit for
bit, the oscillator's error, the emit count against a bisection on its
predicate, qpsk_tuner_apply_host against the numpy yardstick
(tuner_cases.tuner_reference) at tolerance 0, the yardstick against a float64
ideal, the retune's phase continuity, and every rejection."""
import ctypes as C
import math

import numpy as np
import pytest

import qpsk_amd as Q
import tuner_cases as TC

DT = Q.TUNER_STATE_DTYPE
f32 = np.float32


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def rows_of(S, n, seed):
    x = np.random.default_rng(seed).standard_normal((S, 2 * n)).astype(f32)
    head = np.array([0.0, -0.0, 1e-45, -1e-40, 1.0, -1.0, -0.0, 3e-39], f32)
    x[:, : head.size] = head
    return x


def host_calls(p, state, x, lens, taps=None):
    """Calls of lens[i] samples on every stream through the host form; the
    joined output rows of each stream and the state behind them."""
    S = x.shape[0]
    out, pos = [[] for _ in range(S)], 0
    for n in lens:
        rows = np.ascontiguousarray(x[:, 2 * pos: 2 * (pos + n)]) if n else np.zeros((S, 2), f32)
        state, o, n_out = Q.tuner_apply_host(p, state, rows, n=n, taps=taps)
        for s in range(S):
            out[s].append(o[s, : 2 * n_out[s]].copy())
        pos += n
    return [np.concatenate(o) for o in out], state


def test_the_exports_exist():
    real = C.CDLL(Q.LIB_PATH)
    names = [n for n in Q.EXPORTED_SYMBOLS if n.startswith("qpsk_tuner_")]
    assert len(names) == 19
    for n in names:
        assert hasattr(real, n), n
    assert Q.tuner_state_size() == 320 == DT.itemsize
    p = Q.tuner_params()
    assert (p.freq, p.rate, p.tau0, p.cutoff, p.taps_per_phase, p.first_stream, p.device) == (0.0, 1.0, 0.0, 0.0, 16, 0, 0)
    assert C.sizeof(Q.TunerParams) == 72


@pytest.mark.parametrize("T", [4, 8, 12, 16, 32])
@pytest.mark.parametrize("fc", [0.4, 0.1, 0.5, 0.4 / 3.7])
def test_the_design_equals_its_formula_bit_for_bit(T, fc):
    h = Q.tuner_design(T, fc)
    assert bits_equal(h, np.array(TC.design(T, fc)))
    assert bits_equal(h, h[::-1].copy())                     # symmetric about 32 T
    assert abs(float(h.astype(np.float64).sum()) - 64.0) < 1e-4


def test_both_tables_equal_their_formulas_bit_for_bit():
    c, f = Q.tuner_tables()
    C0, F0 = TC.tables()
    assert bits_equal(c, C0) and bits_equal(f, F0)
    assert c[0].tobytes() == f[0].tobytes() == np.array([1.0, 0.0], f32).tobytes()


def test_the_oscillator_is_within_its_bound_of_the_exact_exponential():
    rng = np.random.default_rng(1)
    ph = rng.integers(0, 2 ** 64, 200000, dtype=np.uint64)
    edge = [0, 1, (1 << 44) - 1, 1 << 44, (1 << 54) - 1, 1 << 54, (1 << 63) - 1, 1 << 63, (1 << 64) - 1,
            (1 << 62), (1 << 62) - 1, 3 << 62, (3 << 62) - 1]
    ph = np.concatenate([ph, np.array(edge, np.uint64)])
    w = Q.tuner_osc(ph)
    wr, wi = TC.osc(ph)
    assert bits_equal(w[:, 0], wr) and bits_equal(w[:, 1], wi)
    ang = 2.0 * np.pi * (ph.astype(np.float64) / 2.0 ** 64)   # the double's own rounding is 2^-53 of a turn
    err = np.abs((w[:, 0].astype(np.float64) + 1j * w[:, 1].astype(np.float64)) - np.exp(1j * ang))
    bound = 2.0 * np.pi * 2.0 ** -20 + 2.0 ** -21
    print(f"oscillator: worst error {err.max():.3e}, bound {bound:.3e}")
    assert err.max() <= bound


@pytest.mark.parametrize("T", [4, 16, 32])
@pytest.mark.parametrize("r", [0.25, 0.3, 0.8, 1.0, 1.0 + 1e-4, 1.25, 3.7, 4.0])
def test_the_count_equals_a_bisection_on_its_predicate(T, r):
    rng = np.random.default_rng(int(r * 1000) + T)
    ends = list(range(0, 70)) + [2 ** 20 + 3, 2 ** 31 + 1, 2 ** 40 + 7, 2 ** 49 + 12345, 2 ** 50 - 1, 2 ** 50]
    ends += [int(v) for v in rng.integers(0, 2 ** 50, 40)]
    for tau in (0.0, 0.3, 1.0 - 2.0 ** -53):
        for e in ends:
            want = TC.py_emitted(r, tau, T, e)
            assert Q.tuner_count(r, tau, T, 0, e) == want, (r, tau, T, e)
            assert Q.tuner_count(r, tau, T, max(want - 5, 0), e) == min(5, want)
            assert Q.tuner_count(r, tau, T, want + 3, e) == 0
    for bad in ((0.2, 0.0, 16, 0, 5), (4.5, 0.0, 16, 0, 5), (1.0, 1.0, 16, 0, 5), (1.0, -0.1, 16, 0, 5),
                (1.0, 0.0, 15, 0, 5), (1.0, 0.0, 34, 0, 5), (1.0, 0.0, 2, 0, 5), (1.0, 0.0, 16, -1, 5),
                (1.0, 0.0, 16, 0, -1), (1.0, 0.0, 16, 0, 2 ** 50 + 1), (float("nan"), 0.0, 16, 0, 5)):
        with pytest.raises(ValueError):
            Q.tuner_count(*bad)


def test_out_bound_suffices_at_every_rate():
    for r in TC.RATES + [0.3]:
        p = Q.tuner_params(rate=r)
        for n in (0, 1, 7, 1000, 4097):
            assert Q.tuner_out_bound(p, n) == TC.py_out_bound(n, r)
            for tau in (0.0, 0.999):
                for start in (0, 5, 2 ** 40 + 3, 2 ** 50 - n):
                    got = TC.py_emitted(r, tau, 16, start + n) - TC.py_emitted(r, tau, 16, start)
                    assert got <= Q.tuner_out_bound(p, n)
    assert Q.tuner_out_bound(Q.tuner_params(), 100, rates=[1.0, 0.5, 2.0]) == 204
    with pytest.raises(ValueError):
        Q.tuner_out_bound(Q.tuner_params(), 100, rates=[1.0, 0.2])
    with pytest.raises(ValueError):
        Q.tuner_out_bound(Q.tuner_params(), -1)


CUTS = [0, 1, 2, 3, 5, 31, 32, 33, 0, 64, 7, 300, 1, 221]


@pytest.mark.parametrize("T", TC.TAPS)
@pytest.mark.parametrize("r", TC.RATES)
def test_the_host_form_equals_the_yardstick_over_ragged_cuts(T, r):
    """Every freq of the list as one stream of a batch; calls shorter than the
    history and zero-length ones; per-stream lengths in the last call."""
    S, n = len(TC.FREQS), sum(CUTS)
    x = rows_of(S, n + 40, 7)
    p = Q.tuner_params(rate=r, tau0=0.3, taps_per_phase=T)
    h = TC.design(T, TC.default_cutoff(r))
    state = Q.tuner_state_init(p, S, freq=TC.FREQS)
    got, state = host_calls(p, state, x, CUTS)
    lens = [40 - s for s in range(S)]
    state, o, n_out = Q.tuner_apply_host(p, state, np.ascontiguousarray(x[:, 2 * n:]), lengths=lens)
    models = [TC.PyTuner(r, 0.3, T, f) for f in TC.FREQS]
    for s in range(S):
        whole = np.concatenate([got[s], o[s, : 2 * n_out[s]]])
        want = TC.tuner_reference(x[s, : 2 * (n + lens[s])], r, 0.3, T, h, TC.freq_word(TC.FREQS[s]))
        assert bits_equal(whole, want), (T, r, TC.FREQS[s])
        for c in CUTS + [lens[s]]:
            models[s].call(x[s, 2 * models[s].in_pos: 2 * (models[s].in_pos + c)])
    assert state == b"".join(m.record(DT).tobytes() for m in models)


@pytest.mark.parametrize("T", [4, 16, 32])
def test_the_host_form_at_positions_past_2_40_through_the_state(T):
    rs, fr = [0.25, 1.0 + 1e-4, 3.7], [0.4999, -0.5, 0.03]
    S, n, base = len(rs), 700, 2 ** 40 + 12345
    x = rows_of(S, n + 32, 9)                                  # the first 32 samples are the history
    p = Q.tuner_params(tau0=0.7, taps_per_phase=T, cutoff=0.2)
    models = [TC.PyTuner(rs[s], 0.7, T, fr[s]).at(base, x[s, :64]) for s in range(S)]
    for m in models:
        m.ph0 = 0x123456789ABCDEF0
    state = b"".join(m.record(DT).tobytes() for m in models)
    Q.tuner_state_check(p, S, state)
    k0 = [m.out_pos for m in models]
    got, state = host_calls(p, state, x[:, 64:], [5, 300, 0, 395])
    for s in range(S):
        want = TC.tuner_reference(x[s], rs[s], 0.7, T, TC.design(T, 0.2), TC.freq_word(fr[s]), 0x123456789ABCDEF0,
                                  k0=k0[s], in0=base - 32)
        assert bits_equal(got[s], want), (T, s)
        assert want.size > 0
    st = np.frombuffer(state, DT)
    assert (st["in_pos"] == base + n).all()


def test_replaced_taps_and_the_q_and_f_edges():
    """tau = 0 and an integer r: q = 0 and f = 0 at every output; tau just under
    1 at r = 1: q = 63 and f just under 1."""
    x = rows_of(1, 500, 11)
    taps = np.random.default_rng(3).standard_normal(64 * 8 + 1).astype(f32)
    for r, tau in ((1.0, 0.0), (2.0, 0.0), (1.0, 1.0 - 2.0 ** -30)):
        p = Q.tuner_params(rate=r, tau0=tau, taps_per_phase=8, freq=0.11)
        got, _ = host_calls(p, Q.tuner_state_init(p, 1), x, [123, 377], taps=taps)
        assert bits_equal(got[0], TC.tuner_reference(x[0], r, tau, 8, taps, TC.freq_word(0.11)))
    u = (1.0 - 2.0 ** -30) * 64.0
    assert math.floor(u) == 63 and 0.999 < f32(u - 63.0) < 1.0


def test_the_yardstick_against_the_float64_ideal():
    """A unit tone inside the passband: the residual after removing the tone it
    should become, e^{j 2 pi (tone - freq) p_k}, is what the Hamming window's
    stopband leaves of the images, and lies within the bound measured with the
    yardstick (tuner_cases.IDEAL_RESIDUAL_DB) plus 3 dB; against the ideal that
    mixes by the exact exponential and takes the continuous windowed sinc at
    the exact position, the float arithmetic, the dropped phase bits and the
    interpolation between prototype points leave far less."""
    got = []
    for (T, r, freq, tone) in TC.IDEAL_CASES:
        n = 6000
        i = np.arange(n)
        xc = np.exp(2j * np.pi * tone * i)
        x = np.zeros(2 * n, f32)
        x[0::2], x[1::2] = xc.real, xc.imag
        fc = TC.default_cutoff(r)
        y = TC.tuner_reference(x, r, 0.3, T, TC.design(T, fc), TC.freq_word(freq))
        ideal, tone_out, k = TC.ideal_output(tone, r, 0.3, T, fc, freq, n)
        yc = (y[0::2].astype(np.float64) + 1j * y[1::2].astype(np.float64))[k]
        res = 10.0 * np.log10(np.mean(np.abs(yc - tone_out) ** 2))
        dev = 10.0 * np.log10(np.mean(np.abs(yc - ideal) ** 2))
        print(f"T {T} r {r} freq {freq} tone {tone}: residual {res:.1f} dB, against the ideal {dev:.1f} dB")
        got.append((res, dev))
    for (res, dev), listed in zip(got, TC.IDEAL_RESIDUAL_DB):
        assert res <= TC.IDEAL_BOUND_DB
        assert abs(res - listed) <= 0.5            # the listed figures are the measured ones
        # float32 inputs and sums (2^-24 each), 2 pi 2^-20 of phase, taps read between points 1/64 apart
        assert dev <= -90.0


def test_set_freq_keeps_the_phase_of_in_pos():
    rng = np.random.default_rng(5)
    for _ in range(200):
        m = TC.PyTuner(1.0, 0.0, 16, float(rng.uniform(-0.5, 0.5)))
        m.ph0 = int(rng.integers(0, 2 ** 64, dtype=np.uint64))
        m.in_pos = int(rng.integers(0, 2 ** 50))
        before = m.phase(m.in_pos)
        m.set_freq(float(rng.uniform(-0.5, 0.5)))
        assert m.phase(m.in_pos) == before
    # and in the yardstick: a retune at sample 300 equals two references joined there
    x = rows_of(1, 800, 13)[0]
    T, h = 8, TC.design(8, 0.4)
    m = TC.PyTuner(1.25, 0.3, T, 0.03)
    n1 = m.call(x[:600])
    a = TC.tuner_reference(x[:600], 1.25, 0.3, T, h, m.fw, m.ph0)
    m.set_freq(-0.2)
    b = TC.tuner_reference(x, 1.25, 0.3, T, h, m.fw, m.ph0, k0=n1)
    # the host form with the same switch through its state
    p = Q.tuner_params(rate=1.25, tau0=0.3, taps_per_phase=T, freq=0.03, cutoff=0.4)
    state, o1, c1 = Q.tuner_apply_host(p, Q.tuner_state_init(p, 1), x[None, :600].copy())
    st = np.frombuffer(state, DT).copy()
    st["fw"], st["ph0"] = m.fw, m.ph0
    state, o2, c2 = Q.tuner_apply_host(p, st.tobytes(), x[None, 600:].copy())
    assert c1[0] == n1 and bits_equal(o1[0, : 2 * n1], a) and bits_equal(o2[0, : 2 * c2[0]], b)
    # outputs whose taps lie wholly behind the switch are those of a stream tuned to -0.2 from a shifted phase
    assert b.size > 100


def test_create_and_state_init_reject_what_is_out_of_range():
    bad = [dict(freq=0.5), dict(freq=-0.51), dict(freq=float("nan")), dict(rate=0.2), dict(rate=4.1),
           dict(rate=float("nan")), dict(tau0=1.0), dict(tau0=-0.1), dict(taps_per_phase=2), dict(taps_per_phase=34),
           dict(taps_per_phase=7), dict(cutoff=0.51), dict(cutoff=-0.1), dict(cutoff=float("nan")),
           dict(first_stream=-1)]
    for kw in bad:
        p = Q.tuner_params(**kw)
        with pytest.raises(ValueError, match="qpsk error -3"):
            Q.tuner_state_init(p, 2)
        h = C.c_void_p()
        assert Q.lib().qpsk_tuner_create(C.byref(p), 2, None, None, C.byref(h)) == Q.QPSK_ERR_OUT_OF_RANGE and not h
    p = Q.tuner_params()
    for kw in (dict(freq=[0.0, 0.5]), dict(rate=[1.0, 5.0]), dict(freq=[float("nan"), 0.0])):
        with pytest.raises(ValueError, match="qpsk error -3"):
            Q.tuner_state_init(p, 2, **kw)
    with pytest.raises(ValueError):
        Q.tuner_state_init(p, 0)
    h = C.c_void_p()
    assert Q.lib().qpsk_tuner_create(C.byref(p), 0, None, None, C.byref(h)) == Q.QPSK_ERR_ARGUMENT
    for T, fc in ((16, 0.0), (16, 0.6), (3, 0.4), (34, 0.4)):
        with pytest.raises(ValueError):
            Q.tuner_design(T, fc)
    hbuf = np.zeros(64 * 16 + 1, f32)
    assert Q.lib().qpsk_tuner_design(16, 0.4, hbuf.ctypes.data, 64 * 16) == Q.QPSK_ERR_ARGUMENT


def test_every_state_check_failure_names_stream_and_field():
    p = Q.tuner_params(rate=1.25, tau0=0.3)
    x = rows_of(2, 100, 15)
    state, _, _ = Q.tuner_apply_host(p, Q.tuner_state_init(p, 2), x)
    Q.tuner_state_check(p, 2, state)

    def broken(field, s, value, idx=None):
        st = np.frombuffer(state, DT).copy()
        if idx is None:
            st[field][s] = value
        else:
            st[field][s][idx] = value
        return st.tobytes()

    cases = [("r", 1, 0.2, None, "stream 1: r"), ("r", 0, float("nan"), None, "stream 0: r"),
             ("tau", 1, 1.0, None, "stream 1: tau"), ("in_pos", 0, -1, None, "stream 0: in_pos"),
             ("in_pos", 1, 2 ** 50 + 1, None, "stream 1: in_pos"), ("out_pos", 1, 5, None, "stream 1: out_pos"),
             ("reserved", 0, 1, 3, "stream 0: reserved")]
    for field, s, v, idx, text in cases:
        with pytest.raises(ValueError, match=text):
            Q.tuner_state_check(p, 2, broken(field, s, v, idx))
    fresh = np.frombuffer(Q.tuner_state_init(p, 2), DT).copy()
    fresh["hist"][1, 31, 1] = -0.0
    with pytest.raises(ValueError, match=r"stream 1: hist\[31\]"):
        Q.tuner_state_check(p, 2, fresh.tobytes())
    with pytest.raises(ValueError, match="state length"):
        Q.tuner_state_check(p, 2, state[:-1])
    with pytest.raises(ValueError):
        Q.tuner_state_check(p, 3, state)
    # fw and ph0 may hold anything
    Q.tuner_state_check(p, 2, broken("ph0", 0, 2 ** 64 - 1))
    Q.tuner_state_check(p, 2, broken("fw", 1, -2 ** 63))
    # T is part of the predicate: the same blob is no state of a handle with other taps
    with pytest.raises(ValueError, match="out_pos"):
        Q.tuner_state_check(Q.tuner_params(rate=1.25, tau0=0.3, taps_per_phase=8), 2, state)


def test_what_the_host_form_refuses_changes_nothing():
    p = Q.tuner_params(rate=0.8)
    S, n = 2, 50
    x = rows_of(S, n, 17)
    state0, _, _ = Q.tuner_apply_host(p, Q.tuner_state_init(p, S), x)
    need = max(TC.py_count(0.8, 0.0, 16, int(r["out_pos"]), int(r["in_pos"]) + n) for r in np.frombuffer(state0, DT))
    L = Q.lib()

    def call(state=None, rows=x, stride_in=None, out=None, stride_out=None, cap=None, n_samples=n, lengths=None,
             n_out=True, taps=None, bytes_=None):
        st = C.create_string_buffer(state0 if state is None else state, len(state0 if state is None else state))
        o = np.full((S, 2 * (need + 2)), 7.0, f32) if out is None else out
        cnt = np.full(S, -9, np.int64)
        ln = None if lengths is None else np.asarray(lengths, np.int64)
        rc = L.qpsk_tuner_apply_host(C.byref(p), None if taps is None else taps.ctypes.data, st,
                                     len(st) if bytes_ is None else bytes_, S,
                                     None if rows is None else rows.ctypes.data,
                                     rows.shape[1] if stride_in is None and rows is not None else (stride_in or 0),
                                     o.ctypes.data if o is not False else None,
                                     o.shape[1] if stride_out is None and o is not False else (stride_out or 0),
                                     need + 2 if cap is None else cap, n_samples,
                                     None if ln is None else ln.ctypes.data_as(C.POINTER(C.c_int64)),
                                     cnt.ctypes.data_as(C.POINTER(C.c_int64)) if n_out else None)
        unchanged = st.raw == (state0 if state is None else state) and (o is False or (o == 7.0).all()) and (cnt == -9).all()
        return rc, unchanged

    assert call() == (0, False)
    big = np.full((S, 8 * n), 7.0, f32)
    bad_taps = np.array(TC.design(16, 0.4))
    bad_taps[5] = np.inf
    refused = [
        dict(cap=need - 1), dict(cap=-1), dict(n_samples=-1), dict(stride_in=2 * n - 1), dict(stride_out=2 * need),
        dict(lengths=[1, n + 1]), dict(lengths=[-1, 2]), dict(n_out=False), dict(rows=None), dict(out=False),
        dict(bytes_=len(state0) - 1), dict(state=state0[:320] + bytes(8) + state0[328:]),        # stream 1: r = 0
        dict(taps=bad_taps),
    ]
    for k, kw in enumerate(refused):
        rc, unchanged = call(**kw)
        assert rc < 0 and unchanged, (k, kw, rc)
    # rows that overlap: the output begins inside the input
    st = C.create_string_buffer(state0, len(state0))
    cnt = np.full(S, -9, np.int64)
    before = big.copy()
    rc = L.qpsk_tuner_apply_host(C.byref(p), None, st, len(st), S, big.ctypes.data, big.shape[1],
                                 big[:, 2 * n - 2:].ctypes.data, big.shape[1], need + 2, n, None,
                                 cnt.ctypes.data_as(C.POINTER(C.c_int64)))
    assert rc == Q.QPSK_ERR_ARGUMENT and st.raw == state0 and (big == before).all() and (cnt == -9).all()
    # a stream that would pass 2^50
    m = TC.PyTuner(0.8, 0.0, 16).at(2 ** 50 - 10)
    far = m.record(DT).tobytes() * 2
    rc, unchanged = call(state=far)
    assert rc == Q.QPSK_ERR_ARGUMENT and unchanged
