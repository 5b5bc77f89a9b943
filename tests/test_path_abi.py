"""The propagation path's C ABI without a GPU: the declarations and exports, the
parameter defaults, the create checks that come before a device is touched,
qpsk_path_count and qpsk_path_out_bound against their Python restatement,
qpsk_path_apply_host against the numpy yardstick (tests/path_cases.py) with
outputs, counts and the state after every call compared, and
qpsk_path_state_check on records built in numpy at and just past every edge.
Every comparison is at tolerance 0."""
import ctypes as C
import functools
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import common as K
import path_cases as PC
import qpsk_amd as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["qpsk_path_params_init", "qpsk_path_create", "qpsk_path_destroy", "qpsk_path_set_stream",
           "qpsk_path_set_taps", "qpsk_path_apply_fmt", "qpsk_path_out_bound", "qpsk_path_count",
           "qpsk_path_state_size", "qpsk_path_state_init", "qpsk_path_get_state", "qpsk_path_set_state",
           "qpsk_path_reset_streams", "qpsk_path_state_check", "qpsk_path_apply_host"]
RS = [1 - 1e-3, 1 - 1e-9, 1.0, 1 + 1e-9, 1 + 1e-3]
TAUS = [0.0, 0.5, 1 - 2.0 ** -53]
CUTS = [0, 1, 2, 3, 5, 16, 17, 63, 64, 65, 1023, 1024, 1025]
N = 4000          # the listed cuts alone take 3308 samples; the rest follows them
CUTS.append(N - sum(CUTS))
assert CUTS[-1] > 0


def last_error():
    return Q.lib().qpsk_last_error().decode()


def test_header_declares_and_library_exports_the_entries():
    src = open(os.path.join(ROOT, "include", "qpsk_demod.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", Q.LIB_PATH]).decode()
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert re.search(r"\bT " + name + r"\b", nm), name
        assert name in Q.EXPORTED_SYMBOLS
    assert re.search(r"#define\s+QPSK_ABI_VERSION\s+3\b", src)
    assert re.search(r"#define\s+QPSK_PATH_TILE_OUTPUTS\s+%d\b" % Q.PATH_TILE_OUTPUTS, src)
    assert Q.PATH_TILE_OUTPUTS == PC.TILE
    assert Q.lib().qpsk_abi_version() == 3


def test_params_init_defaults_state_size_and_the_created_state():
    p = Q.PathParams()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    Q.lib().qpsk_path_params_init(C.byref(p))
    assert (p.clock_ppm, p.clock_spread, p.clock_seed, p.tau0) == (0.0, 0.0, 3000, 0.0)
    assert (p.tau_random, p.multipath, p.first_stream, p.device) == (0, 0, 0, 0)
    assert list(p.reserved) == [0] * 7
    assert C.sizeof(p) == 80
    assert Q.path_state_size() == 256 == Q.PATH_STATE_DTYPE.itemsize
    st = np.frombuffer(Q.path_state_init(p, 3), Q.PATH_STATE_DTYPE)
    for s in range(3):
        assert st[s].tobytes() == PC.PyPath(1.0, 0.0).record(Q.PATH_STATE_DTYPE).tobytes()
    # multipath = 1: the project's taps; a spread and a random tau: the draws of clock_seed + g
    p = Q.path_params(clock_ppm=-40.0, clock_spread=100.0, clock_seed=77, tau_random=1, multipath=1, first_stream=5)
    st = np.frombuffer(Q.path_state_init(p, 4), Q.PATH_STATE_DTYPE)
    rs = set()
    for s in range(4):
        r, tau = PC.clock(5 + s, -40.0, 100.0, 77, 0.0, True)
        assert st[s].tobytes() == PC.PyPath(r, tau, PC.project_taps()).record(Q.PATH_STATE_DTYPE).tobytes()
        assert abs((r - 1) * 1e6 + 40.0) <= 100.0 and 0 <= tau < 1
        rs.add(r)
    assert len(rs) == 4
    assert st["taps"][0, 1, 0] == np.float32(0.25 * math.cos(0.7)) and st["taps"][0, 2, 1] == np.float32(0.1 * math.sin(-1.9))


@pytest.mark.parametrize("fields", [
    dict(clock_ppm=1000.5), dict(clock_ppm=-1000.5), dict(clock_ppm=600.0, clock_spread=400.5),
    dict(clock_spread=-1.0), dict(clock_ppm=float("nan")), dict(clock_ppm=float("inf")),
    dict(clock_spread=float("nan")), dict(clock_spread=float("inf")), dict(tau0=1.0), dict(tau0=-2.0 ** -60),
    dict(tau0=float("nan")), dict(tau0=float("inf")), dict(first_stream=-1)], ids=str)
def test_create_rejects_bad_params_before_touching_a_device(fields):
    p = Q.path_params(device=12345, **fields)          # no such device: reaching it would be QPSK_ERR_DEVICE
    h = C.c_void_p()
    assert Q.lib().qpsk_path_create(C.byref(p), 4, C.byref(h)) == Q.QPSK_ERR_OUT_OF_RANGE
    assert next(iter(fields)).split("_")[0] in last_error() and not h.value
    assert Q.lib().qpsk_path_state_init(C.byref(p), 1, C.create_string_buffer(256), 256) == Q.QPSK_ERR_OUT_OF_RANGE
    assert Q.lib().qpsk_path_out_bound(C.byref(p), 10) == Q.QPSK_ERR_OUT_OF_RANGE


def test_create_accepts_the_edges_of_the_ranges_and_rejects_no_streams():
    h = C.c_void_p()
    assert Q.lib().qpsk_path_create(C.byref(Q.path_params(device=12345)), 0, C.byref(h)) == Q.QPSK_ERR_ARGUMENT
    for fields in (dict(clock_ppm=1000.0), dict(clock_ppm=-1000.0), dict(clock_ppm=-600.0, clock_spread=400.0),
                   dict(tau0=1 - 2.0 ** -53)):
        p = Q.path_params(**fields)
        st = Q.path_state_init(p, 64)                  # the same checks, no device
        Q.path_state_check(64, st)
        r = np.frombuffer(st, Q.PATH_STATE_DTYPE)["r"]
        assert (r >= PC.R_MIN).all() and (r <= PC.R_MAX).all()


# ---------------------------------------------------------------------------
# the count and the bound
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("r", RS)
def test_count_equals_the_python_restatement(r, tau):
    for in_end in [0, 1, 2, 3, 4, 1000]:
        assert Q.path_count(r, tau, 0, in_end) == PC.py_count(r, tau, 0, in_end), in_end
    assert Q.path_count(1.0, 0.0, 0, 1000) == 998
    for base in (2 ** 40, 2 ** 40 - 7, 2 ** 50 - 2000):
        for d in (0, 1, 2, 3, 999, 1000, 1001):
            want = PC.py_emitted(r, tau, base + d)
            assert Q.path_count(r, tau, 0, base + d) == want, (base, d)
            out_pos = PC.py_emitted(r, tau, base)
            assert Q.path_count(r, tau, out_pos, base + d) == want - out_pos
            assert Q.path_count(r, tau, want + 5, base + d) == 0
    # by the predicate itself at the count's edge
    k = Q.path_count(r, tau, 0, 2 ** 40)
    assert math.floor(PC.p_of(r, tau, k - 1)) <= 2 ** 40 - 3 < math.floor(PC.p_of(r, tau, k))


def test_count_refuses_what_is_no_clock_or_position():
    for args in [(0.9, 0.0, 0, 10), (PC.R_MAX + 1e-9, 0.0, 0, 10), (float("nan"), 0.0, 0, 10), (1.0, 1.0, 0, 10),
                 (1.0, -0.1, 0, 10), (1.0, float("nan"), 0, 10), (1.0, 0.0, -1, 10), (1.0, 0.0, 0, -1),
                 (1.0, 0.0, 0, 2 ** 50 + 1)]:
        assert Q.lib().qpsk_path_count(*args) == Q.QPSK_ERR_ARGUMENT, args
    assert Q.path_count(PC.R_MIN, 0.0, 0, 2 ** 50) > 0 and Q.path_count(PC.R_MAX, 0.0, 0, 2 ** 50) > 0


@pytest.mark.parametrize("r,tau", list(itertools.product(RS, TAUS)))
def test_count_over_any_cut_sums_to_one_call(r, tau):
    rng = np.random.default_rng(5)
    for cuts in (CUTS, list(rng.integers(0, 40, 200)), [1] * 50, [2 ** 40, 1, 2, 3, 1000]):
        in_pos = out_pos = 0
        for c in cuts:
            got = Q.path_count(r, tau, out_pos, in_pos + int(c))
            assert got == PC.py_count(r, tau, out_pos, in_pos + int(c))
            in_pos, out_pos = in_pos + int(c), out_pos + got
        assert out_pos == Q.path_count(r, tau, 0, in_pos)


@pytest.mark.parametrize("ppm,spread", [(0.0, 0.0), (1000.0, 0.0), (-1000.0, 0.0), (-300.0, 700.0), (1e-3, 0.0)])
def test_out_bound_is_the_formula_and_never_below_the_count(ppm, spread):
    p = Q.path_params(clock_ppm=ppm, clock_spread=spread)
    r_lo = 1.0 + -(abs(ppm) + spread) * 1e-6
    for n in [0, 1, 2, 3, 4, 5, 999, 1000, 1001, 2 ** 20, 2 ** 40]:
        b = Q.path_out_bound(p, n)
        assert b == PC.py_out_bound(n, ppm, spread)
        for tau in TAUS:
            for in_pos in (0, 1, 2, 3, 17, 2 ** 40 + 1):
                out_pos = PC.py_emitted(r_lo, tau, in_pos)
                assert PC.py_count(r_lo, tau, out_pos, in_pos + n) <= b, (n, tau, in_pos)
    assert Q.lib().qpsk_path_out_bound(C.byref(p), -1) == Q.QPSK_ERR_ARGUMENT


# ---------------------------------------------------------------------------
# the host form of the call against the yardstick
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stream(seed, special=False):
    x = np.random.default_rng(seed).standard_normal(2 * N).astype(np.float32)
    if special:
        x[:6] = [0.0, -0.0, 1e-45, -1e-40, -0.0, 3e-39]
        x[200:204] = [-0.0, -0.0, np.inf, 1.0]           # the Inf makes NaNs of its neighbours' products
    x.setflags(write=False)
    return x


def taps_of(L, seed=3):
    rng = np.random.default_rng(seed + L)
    t = (rng.standard_normal((L, 2)) * 0.3).astype(np.float32)
    t[0] = [1.0, 0.0] if L == 1 else [0.9, -0.1]
    return t


def run_host_calls(x, r, tau, taps, cuts):
    """The stream through qpsk_path_apply_host over cuts, every call's outputs,
    count and the state behind it compared with the Python model; returns all outputs."""
    py = PC.PyPath(r, tau, taps)
    state = py.record(Q.PATH_STATE_DTYPE).tobytes()
    Q.path_state_check(1, state)
    pos, outs = 0, []
    for ci, c in enumerate(cuts):
        rows = np.array(x[2 * pos: 2 * (pos + c)]).reshape(1, -1)
        cap = PC.py_out_bound(c, 1000.0)
        out = np.full((1, 2 * cap + 2), np.float32(777.0))
        state, out, n_out = Q.path_apply_host(state, rows, out=out, out_cap=cap, n=c)
        want_n = py.call(rows)
        assert int(n_out[0]) == want_n, (ci, c)
        assert (out[0, 2 * want_n:] == 777.0).all(), f"call {ci}: written past its count"
        assert state == py.record(Q.PATH_STATE_DTYPE).tobytes(), f"state after call {ci} ({c} samples)"
        Q.path_state_check(1, state)
        outs.append(out[0, : 2 * want_n].copy())
        pos += c
    return np.concatenate(outs)


def assert_bits(got, want, what):
    """Bit for bit, NaNs included (host and yardstick both run on the CPU)."""
    assert got.shape == want.shape, f"{what}: {got.size // 2} outputs vs {want.size // 2}"
    if not K.bitwise_equal(got, want):
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        pytest.fail(f"{what}: {bad.size} floats differ, first at output {bad[0] // 2}: {got[bad[0]]!r} vs {want[bad[0]]!r}")


def test_identity_returns_the_row_two_samples_short():
    x = stream(1, special=True)
    got = run_host_calls(x, 1.0, 0.0, PC.IDENTITY, [N])
    want = PC.path_reference(x, 1.0, 0.0, PC.IDENTITY)
    assert got.size == 2 * (N - 2)
    assert_bits(got, want, "identity")
    assert np.isnan(got).any(), "the Inf reached the interpolator"
    # finite samples come back bit for bit, except that -0 becomes +0
    fin = np.ones(N - 2, bool)
    fin[99:103] = False                                # outputs whose four samples hold the Inf (sample 101)
    back = np.array(x[: 2 * (N - 2)])
    back[K_negzero(back)] = 0.0
    assert K.bitwise_equal(got.reshape(-1, 2)[fin], back.reshape(-1, 2)[fin])
    assert not K_negzero(got).any() and K_negzero(np.array(x)).any()


def K_negzero(v):
    return np.signbit(v) & (v == 0)


@pytest.mark.parametrize("L", [1, 4, 8])
@pytest.mark.parametrize("r,tau", [(1.0, 0.0), (1 - 1e-3, 0.0), (1 + 1e-3, 0.37), (1 + 1e-3, 1 - 2.0 ** -53),
                                   (1 - 1e-3, 0.9991), (1.0 + 37e-6, 0.5)])
def test_host_call_equals_the_yardstick_over_the_ragged_cut(r, tau, L):
    x, taps = stream(2 + L), (PC.project_taps() if L == 4 else taps_of(L))
    want = PC.path_reference(x, r, tau, taps)
    assert want.size // 2 == PC.py_emitted(r, tau, N)
    if abs(r - 1.0) > 0.9e-3:
        n = np.floor(tau + np.arange(want.size // 2) * r).astype(np.int64)
        slips = np.count_nonzero(np.diff(n) != 1)
        assert slips >= 2, "an index slip about every 1000 outputs"
    assert_bits(run_host_calls(x, r, tau, taps, CUTS), want, f"cut, L = {L}")
    assert_bits(run_host_calls(x, r, tau, taps, [N]), want, f"one call, L = {L}")
    assert_bits(run_host_calls(x, r, tau, taps, CUTS[::-1]), want, f"cut reversed, L = {L}")


def test_host_call_with_streams_lengths_and_positions_near_2_40():
    S, n = 3, 700
    clocks = [(1 - 1e-3, 0.25), (1.0, 0.0), (1 + 1e-3, 0.75)]
    base = 2 ** 40 - 300
    x = np.stack([stream(20 + s)[: 2 * n] for s in range(S)])
    pys = [PC.PyPath(r, tau, taps_of(2 + 3 * s)).at(base) for s, (r, tau) in enumerate(clocks)]
    state = b"".join(p.record(Q.PATH_STATE_DTYPE).tobytes() for p in pys)
    Q.path_state_check(S, state)
    lens = [n, 0, 333]
    k0 = [p.out_pos for p in pys]
    state, out, n_out = Q.path_apply_host(state, x, lengths=lens)
    for s in range(S):
        # the history is zeros, which is what the yardstick reads before its row
        want = PC.path_reference(x[s, : 2 * lens[s]], *clocks[s], pys[s].taps, k0=k0[s], in0=base) if lens[s] else None
        cnt = pys[s].call(x[s, : 2 * lens[s]])
        assert n_out[s] == cnt
        if lens[s]:
            assert want.size == 2 * cnt
            assert_bits(out[s, : 2 * cnt], want, f"stream {s} near 2^40")
    assert state == b"".join(p.record(Q.PATH_STATE_DTYPE).tobytes() for p in pys)


# ---------------------------------------------------------------------------
# the state check
# ---------------------------------------------------------------------------
def good_state(S=3):
    pys = [PC.PyPath(1 + 1e-4 * s, 0.25 * s, taps_of(1 + 2 * s)) for s in range(S)]
    for s, p in enumerate(pys):
        p.call(stream(30 + s)[: 2 * (5 + 9 * s)])      # 5, 14 and 23 samples: stream 0 has negative-index history
    return np.concatenate([p.record(Q.PATH_STATE_DTYPE) for p in pys])


def check(st):
    return Q.lib().qpsk_path_state_check(st.size, st.tobytes(), st.nbytes)


def consistent(st, s):
    st["out_pos"][s] = PC.py_emitted(float(st["r"][s]), float(st["tau"][s]), int(st["in_pos"][s]))


def test_state_check_accepts_the_edges():
    assert check(good_state()) == Q.QPSK_OK
    for field, v in (("r", PC.R_MIN), ("r", PC.R_MAX), ("tau", 0.0), ("tau", 1 - 2.0 ** -53)):
        st = good_state()
        st[field][1] = v
        consistent(st, 1)
        assert check(st) == Q.QPSK_OK, (field, v, last_error())
    st = good_state()
    st["in_pos"][2] = 2 ** 50
    consistent(st, 2)
    st["hist"][2] = np.nan                             # any bits at non-negative indices
    assert check(st) == Q.QPSK_OK, last_error()
    st = good_state()
    st["in_pos"][0] = st["out_pos"][0] = 0
    st["hist"][0] = 0.0
    st["n_taps"][0] = 8
    st["taps"][0] = 0.5
    assert check(st) == Q.QPSK_OK, last_error()


@pytest.mark.parametrize("field,value,s", [
    ("r", np.nextafter(PC.R_MIN, 0.0), 0), ("r", np.nextafter(PC.R_MAX, 2.0), 1), ("r", float("nan"), 2),
    ("r", float("inf"), 0), ("tau", 1.0, 1), ("tau", -2.0 ** -1074, 2), ("tau", float("nan"), 0),
    ("in_pos", -1, 1), ("in_pos", 2 ** 50 + 1, 1), ("out_pos", -1, 2), ("n_taps", 0, 0), ("n_taps", 9, 1)], ids=str)
def test_state_check_refuses_just_past_every_edge(field, value, s):
    st = good_state()
    st[field][s] = value
    assert check(st) == Q.QPSK_ERR_ARGUMENT
    assert f"stream {s}: {field}" in last_error(), last_error()


def test_state_check_refuses_inconsistent_positions_taps_history_and_reserved():
    st = good_state()
    st["out_pos"][1] += 1
    assert check(st) == Q.QPSK_ERR_ARGUMENT and "stream 1: out_pos" in last_error()
    st = good_state()
    st["out_pos"][2] -= 1
    assert check(st) == Q.QPSK_ERR_ARGUMENT and "stream 2: out_pos" in last_error()
    st = good_state()
    st["taps"][0, 1, 0] = 1e-30                        # n_taps = 1: tap 1 is unused
    assert check(st) == Q.QPSK_ERR_ARGUMENT and "stream 0: taps[1].re" in last_error()
    st = good_state()
    st["taps"][0, 7, 1] = -0.0                         # not +0
    assert check(st) == Q.QPSK_ERR_ARGUMENT and "stream 0: taps[7].im" in last_error()
    st = good_state()
    st["taps"][1, 2, 1] = np.inf                       # n_taps = 3: tap 2 is used
    assert check(st) == Q.QPSK_ERR_ARGUMENT and "stream 1: taps[2].im" in last_error()
    st = good_state()
    st["hist"][0, 10, 1] = -0.0                        # in_pos = 5: hist[10] is index -1
    assert check(st) == Q.QPSK_ERR_ARGUMENT and "stream 0: hist[10]" in last_error()
    st = good_state()
    st["hist"][0, 11, 0] = np.nan                      # index 0: any bits
    assert check(st) == Q.QPSK_OK
    for b in (0, 27):
        st = good_state()
        st["reserved"][2, b] = 1
        assert check(st) == Q.QPSK_ERR_ARGUMENT and "stream 2: reserved" in last_error()
    st = good_state()
    assert Q.lib().qpsk_path_state_check(3, st.tobytes(), st.nbytes - 1) == Q.QPSK_ERR_ARGUMENT
    assert Q.lib().qpsk_path_state_check(0, st.tobytes(), 0) == Q.QPSK_ERR_ARGUMENT
    assert Q.lib().qpsk_path_state_check(3, None, st.nbytes) == Q.QPSK_ERR_ARGUMENT_NULL


def test_a_rejected_host_call_leaves_state_and_output_as_they_were():
    st = good_state()
    x = np.stack([stream(40 + s)[:400] for s in range(3)])
    out = np.full((3, 220), np.float32(-5.0))
    n_out = np.full(3, -9, np.int64)

    def call(state, rows=x, out=out, cap=110, n=100, lengths=None, stride_in=None):
        buf = C.create_string_buffer(state, len(state))
        ln = None if lengths is None else np.array(lengths, np.int64).ctypes.data_as(C.POINTER(C.c_int64))
        rc = Q.lib().qpsk_path_apply_host(buf, len(buf), 3, rows.ctypes.data, stride_in or rows.strides[0] // 4,
                                          out.ctypes.data, out.strides[0] // 4, cap, n, ln,
                                          n_out.ctypes.data_as(C.POINTER(C.c_int64)))
        return rc, buf.raw

    good = st.tobytes()
    bad = st.copy()
    bad["tau"][1] = 1.5
    short = Q.path_count(float(st["r"][0]), float(st["tau"][0]), int(st["out_pos"][0]), int(st["in_pos"][0]) + 100) - 1
    for kw, code in ((dict(state=bad.tobytes()), Q.QPSK_ERR_ARGUMENT), (dict(state=good, cap=short), Q.QPSK_ERR_ARGUMENT),
                     (dict(state=good, n=-1), Q.QPSK_ERR_ARGUMENT), (dict(state=good, lengths=[1, 101, 2]), Q.QPSK_ERR_ARGUMENT),
                     (dict(state=good, lengths=[1, -1, 2]), Q.QPSK_ERR_ARGUMENT), (dict(state=good, stride_in=198), Q.QPSK_ERR_ARGUMENT),
                     (dict(state=good, out=x[:, 150:], cap=110), Q.QPSK_ERR_ARGUMENT),           # overlap, capacity enough
                     (dict(state=good, cap=111), Q.QPSK_ERR_ARGUMENT),            # stride_out < 2 out_cap
                     (dict(state=good, out=x[:, 20:], cap=90), Q.QPSK_ERR_ARGUMENT)):   # overlap
        rc, after = call(**kw)
        assert rc == code, (kw.keys(), rc, last_error())
        assert after == kw["state"], kw.keys()
        assert (out == -5.0).all() and (n_out == -9).all(), kw.keys()
    assert "would emit" in (call(good, cap=short), last_error())[1]
    rc, after = call(good)
    assert rc == Q.QPSK_OK and after != good and (n_out > 90).all() and (out[:, :180] != -5.0).all()
