"""The polyphase channeliser's host half (qpsk_pfb_*, csrc/qpsk_pfb.cpp): the
exports, the parameter edges, the prototype and the twiddles against their
formulas, the host form of the call (qpsk_pfb_apply_host) against the numpy
yardstick at tolerance 0, the count, the state and its check, and the yardstick
itself against the filter-bank sum in float64.  Needs no GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pfb_cases as PC
import qpsk_amd as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["qpsk_pfb_params_init", "qpsk_pfb_create", "qpsk_pfb_destroy", "qpsk_pfb_set_stream", "qpsk_pfb_design",
           "qpsk_pfb_twiddles", "qpsk_pfb_set_taps", "qpsk_pfb_count", "qpsk_pfb_out_bound", "qpsk_pfb_tile_frames",
           "qpsk_pfb_apply_fmt", "qpsk_pfb_state_size", "qpsk_pfb_state_init", "qpsk_pfb_get_state",
           "qpsk_pfb_set_state", "qpsk_pfb_reset_bands", "qpsk_pfb_state_check", "qpsk_pfb_apply_host"]
f32 = np.float32


def ulps(a, b):
    """The distance of two float32 arrays in representable steps."""
    def key(v):
        i = np.asarray(v, f32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def test_header_library_and_binding_agree_on_the_entry_points():
    src = open(os.path.join(ROOT, "include", "qpsk_demod.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", Q.LIB_PATH]).decode()
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert re.search(r"\bT " + name + r"\b", nm), name
        assert name in Q.EXPORTED_SYMBOLS
    assert re.search(r"#define\s+QPSK_ABI_VERSION\s+3\b", src) and Q.lib().qpsk_abi_version() == 3
    for name, value in (("QPSK_PFB_MIN_CHANNELS", Q.PFB_MIN_CHANNELS), ("QPSK_PFB_MAX_CHANNELS", Q.PFB_MAX_CHANNELS),
                        ("QPSK_PFB_MAX_BRANCH_TAPS", Q.PFB_MAX_BRANCH_TAPS), ("QPSK_PFB_MAX_TAPS", Q.PFB_MAX_TAPS),
                        ("QPSK_PFB_STATE_HEAD", Q.PFB_STATE_HEAD)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", src), name
    for m in ("apply", "apply_device", "lengths_for_demod", "set_taps", "get_state", "set_state", "reset_bands",
              "set_stream", "out_bound"):
        assert callable(getattr(Q.Channeliser, m)), m
    for M in PC.CHANNELS:
        assert Q.pfb_tile_frames(M) == PC.tile_frames(M)
    assert C.sizeof(Q.PfbParams) == 64


def test_params_init_defaults():
    p = Q.pfb_params()
    assert (p.channels, p.taps_per_branch, p.gain, p.device) == (64, 8, 1.0, 0) and not any(p.reserved)
    assert Q.pfb_state_size(p) == 64 + 8 * 512
    assert Q.pfb_state_init(p, 3) == bytes(3 * (64 + 8 * 512))


@pytest.mark.parametrize("kw", [dict(channels=4), dict(channels=8192), dict(channels=24), dict(channels=0),
                                dict(channels=-16), dict(taps_per_branch=0), dict(taps_per_branch=17),
                                dict(channels=4096, taps_per_branch=16), dict(channels=4096, taps_per_branch=9),
                                dict(gain=float("nan")), dict(gain=float("inf")), dict(gain=-float("inf"))],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_bad_parameters_are_refused_before_a_device_is_touched(kw):
    p = Q.pfb_params(**kw)
    h = C.c_void_p()
    assert Q.lib().qpsk_pfb_create(C.byref(p), 1, C.byref(h)) == Q.QPSK_ERR_OUT_OF_RANGE and not h.value
    assert Q.lib().qpsk_pfb_state_size(C.byref(p)) == Q.QPSK_ERR_OUT_OF_RANGE
    assert Q.lib().qpsk_pfb_design(C.byref(p), None, 0) == Q.QPSK_ERR_OUT_OF_RANGE
    with pytest.raises(ValueError):
        Q.pfb_state_init(p, 1)


def test_the_largest_prototype_is_accepted_and_band_counts_are_checked():
    for M, K in ((4096, 8), (2048, 16), (8, 1), (8, 16)):
        p = Q.pfb_params(channels=M, taps_per_branch=K)
        assert Q.pfb_state_size(p) == 64 + 8 * M * K and Q.pfb_design(p).size == M * K
    assert 4096 * 8 == 32768
    p, h = Q.pfb_params(), C.c_void_p()
    for n_bands in (0, -1, 65536):
        assert Q.lib().qpsk_pfb_create(C.byref(p), n_bands, C.byref(h)) == Q.QPSK_ERR_ARGUMENT
    assert Q.lib().qpsk_pfb_create(None, 1, C.byref(h)) == Q.QPSK_ERR_ARGUMENT_NULL
    assert Q.lib().qpsk_pfb_create(C.byref(p), 1, None) == Q.QPSK_ERR_ARGUMENT_NULL
    for call in (lambda: Q.lib().qpsk_pfb_design(C.byref(p), np.zeros(8, f32).ctypes.data, 8),
                 lambda: Q.lib().qpsk_pfb_twiddles(64, np.zeros(8, f32).ctypes.data, 32)):
        assert call() == Q.QPSK_ERR_ARGUMENT
    assert Q.lib().qpsk_pfb_twiddles(48, None, 48) == Q.QPSK_ERR_OUT_OF_RANGE
    assert Q.lib().qpsk_pfb_tile_frames(4) == Q.QPSK_ERR_OUT_OF_RANGE


@pytest.mark.parametrize("M,K", [(M, 2) for M in PC.CHANNELS] + [(16, K) for K in PC.BRANCH_TAPS] +
                         [(1024, 8), (4096, 8), (64, 16)])
def test_design_follows_its_formula(M, K):
    """Each tap within one float step of the numpy evaluation (two double
    evaluations differ by about 1e-16 relative, which moves a float rounding by
    one step at most), h[0] = 0, the symmetry bit for bit, the DC gain."""
    L = M * K
    h = Q.pfb_design(Q.pfb_params(channels=M, taps_per_branch=K))
    want = PC.design_formula(M, K)
    assert h.dtype == f32 and h.shape == (L,)
    assert ulps(h, want).max() <= 1
    assert h[0] == 0 and not np.signbit(h[0])
    assert h[1:].tobytes() == h[:0:-1].tobytes()               # h[n] == h[L - n]
    assert abs(float(h.astype(np.float64).sum()) - 1.0) <= L * 2.0 ** -24
    assert np.isfinite(h).all() and h[L // 2] == h.max()


@pytest.mark.parametrize("M", PC.CHANNELS)
def test_twiddles_follow_their_formula(M):
    w = Q.pfb_twiddles(M)
    assert w.shape == (M // 2, 2) and ulps(w, PC.twiddle_formula(M)).max() <= 1
    assert w[0].tobytes() == np.array([1.0, 0.0], f32).tobytes()
    assert w[M // 4].tobytes() == np.array([0.0, 1.0], f32).tobytes()


@pytest.mark.parametrize("M", PC.CHANNELS + [64])
def test_count_equals_a_loop_over_frames(M):
    D = M // 2
    ends = sorted({0, 1, 2, D - 1, D, D + 1, 2 * D - 1, 2 * D, 2 * D + 1, 7 * D + 3, 1000})
    for e in ends:
        total = PC.py_emitted(M, e)
        assert Q.pfb_count(M, 0, e) == total == -(-e // D)
        for out_pos in (0, 1, total - 1, total, total + 1, total + 5):
            if out_pos >= 0:
                assert Q.pfb_count(M, out_pos, e) == PC.py_count(M, out_pos, e)
        assert Q.pfb_out_bound(M, e) == PC.py_out_bound(M, e) >= total
    for e in (2 ** 50, 2 ** 50 - 1, 2 ** 40 + 1):
        assert Q.pfb_count(M, 0, e) == -(-e // D) and Q.pfb_out_bound(M, e) == e // D + 1
    in_pos = out_pos = 0
    for c in PC.ragged_cuts(M, 2) * 2:           # a cut's counts sum to one call's
        got = Q.pfb_count(M, out_pos, in_pos + c)
        assert got <= Q.pfb_out_bound(M, c)
        in_pos, out_pos = in_pos + c, out_pos + got
    assert out_pos == Q.pfb_count(M, 0, in_pos)
    for bad in (lambda: Q.pfb_count(M, -1, 10), lambda: Q.pfb_count(M, 0, -1), lambda: Q.pfb_count(M, 0, 2 ** 50 + 1),
                lambda: Q.pfb_count(M + 1, 0, 10), lambda: Q.pfb_out_bound(M, -1), lambda: Q.pfb_out_bound(M, 2 ** 50 + 1)):
        with pytest.raises(ValueError):
            bad()


def host_sequence(p, x, calls, taps=None):
    """The call sequence through qpsk_pfb_apply_host (calls: per call the [B]
    lengths), the state against the model after every call.  Returns per band
    the [M, 2 frames] rows of everything emitted, and the final state."""
    B, M, K = x.shape[0], p.channels, p.taps_per_branch
    dt = Q.pfb_state_dtype(M, K)
    state = Q.pfb_state_init(p, B)
    models = [PC.PyPfb(M, K) for _ in range(B)]
    pos = np.zeros(B, np.int64)
    got = [[] for _ in range(B)]
    for ci, lens in enumerate(calls):
        n = max(lens)
        rows = np.zeros((B, 2 * max(n, 1)), f32)
        for b in range(B):
            rows[b, : 2 * lens[b]] = x[b, 2 * pos[b]: 2 * (pos[b] + lens[b])]
        cap = Q.pfb_out_bound(M, n)
        out = np.full((B * M, 2 * cap), f32(-77.0))
        uniform = all(l == lens[0] for l in lens)
        state, o, n_out = Q.pfb_apply_host(p, state, rows, lengths=None if uniform else lens, out=out, n=n, taps=taps)
        assert o is out
        st = np.frombuffer(state, dt)
        for b in range(B):
            assert models[b].call(rows[b, : 2 * lens[b]]) == n_out[b], (ci, b)
            assert st[b].tobytes() == models[b].record(dt).tobytes(), f"state after call {ci}, band {b}"
            blk = out[b * M: (b + 1) * M]
            assert (blk[:, 2 * n_out[b]:] == f32(-77.0)).all(), f"call {ci} band {b}: written past its count"
            got[b].append(blk[:, : 2 * n_out[b]].copy())
        Q.pfb_state_check(p, B, state)
        pos += np.array(lens)
    return [np.concatenate(g, axis=1) for g in got], state


def assert_rows_equal(got, want, what):
    assert got.shape == want.shape, f"{what}: {got.shape} vs {want.shape}"
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        c, k = bad[0]
        pytest.fail(f"{what}: {len(bad)} floats differ, first at channel {c} frame {k // 2}: "
                    f"{got[c, k]!r} vs {want[c, k]!r}")


@pytest.mark.parametrize("M,K", [(M, 2) for M in PC.CHANNELS] + [(16, K) for K in PC.BRANCH_TAPS if K != 2])
def test_host_form_equals_the_yardstick_over_ragged_cuts(M, K):
    """Tolerance 0, signed zeros included, on finite rows; the cuts cross frame
    parity and the history mid-call; the second band takes them in another order."""
    cuts = PC.ragged_cuts(M, K)
    B, n = 2, sum(cuts)
    x = PC.random_rows(B, n, seed=M + K)
    p = Q.pfb_params(channels=M, taps_per_branch=K)
    calls = [[cuts[i], cuts[(i + 3) % len(cuts)]] for i in range(len(cuts))]
    got, _ = host_sequence(p, x, calls)
    h, W = Q.pfb_design(p), Q.pfb_twiddles(M)
    for b in range(B):
        want = PC.pfb_reference(x[b], M, K, h, W)
        assert want.shape[1] // 2 == -(-n // (M // 2)) >= 3
        assert_rows_equal(got[b], want, f"M = {M}, K = {K}, band {b}")


def test_silence_comes_out_as_zeros_whose_sign_the_definition_fixes():
    """+0 in: a[c] = +0 through every butterfly, so odd channels of odd frames are -0."""
    M, K = 16, 2
    p = Q.pfb_params(channels=M, taps_per_branch=K)
    x = np.zeros((1, 2 * 5 * (M // 2)), f32)
    got, _ = host_sequence(p, x, [[3], [M // 2 * 5 - 3]])
    assert_rows_equal(got[0], PC.pfb_reference(x[0], M, K, Q.pfb_design(p), Q.pfb_twiddles(M)), "silence")
    y = got[0].reshape(M, 5, 2)
    odd = (np.arange(M)[:, None] & np.arange(5)[None, :] & 1).astype(bool)
    assert (y == 0).all() and (np.signbit(y[..., 0]) == odd).all() and (np.signbit(y[..., 1]) == odd).all()


def test_host_form_with_a_gain_and_taps_of_the_callers():
    M, K = 32, 3
    x = PC.random_rows(1, 400, seed=5)
    taps = (np.random.default_rng(6).standard_normal(M * K) * 0.2).astype(f32)
    gain = f32(np.sqrt(8.0))
    p = Q.pfb_params(channels=M, taps_per_branch=K, gain=gain)
    got, _ = host_sequence(p, x, [[150], [250]], taps=taps)
    assert_rows_equal(got[0], PC.pfb_reference(x[0], M, K, taps, Q.pfb_twiddles(M), gain=gain), "own taps and a gain")
    bad = taps.copy()
    bad[7] = np.inf
    with pytest.raises(ValueError, match="tap 7"):
        Q.pfb_apply_host(p, Q.pfb_state_init(p, 1), np.zeros((1, 8), f32), taps=bad)
    assert Q.lib().qpsk_pfb_design(C.byref(p), taps.ctypes.data, M * K - 1) == Q.QPSK_ERR_ARGUMENT


def test_a_constant_input_comes_out_of_channel_0_alone():
    """DC gain 1: after K frames channel 0 carries the constant, the others
    only the prototype's stop band."""
    M, K = 16, 8
    x = np.tile(np.array([0.75, -0.5], f32), 40 * M)
    p = Q.pfb_params(channels=M, taps_per_branch=K)
    _, out, n_out = Q.pfb_apply_host(p, Q.pfb_state_init(p, 1), x.reshape(1, -1).copy())
    y = out[:, : 2 * n_out[0]].reshape(M, -1, 2)[:, 2 * K + 1:]
    assert np.abs(y[0] - [0.75, -0.5]).max() < 1e-6
    assert np.abs(y[1:]).max() < 2e-3


def test_state_check_at_and_past_every_edge():
    M, K, B = 16, 2, 2
    D, L = M // 2, M * K
    p = Q.pfb_params(channels=M, taps_per_branch=K)
    dt = Q.pfb_state_dtype(M, K)
    x = PC.random_rows(B, 100, seed=9)
    _, blob = host_sequence(p, x, [[5, 100]])            # band 0: hist[0 .. L - 6] lie before its start
    good = np.frombuffer(blob, dt).copy()

    def refused(rec, match):
        with pytest.raises(ValueError, match=match):
            Q.pfb_state_check(p, B, rec.tobytes())

    Q.pfb_state_check(p, B, good.tobytes())
    s = good.copy(); s["in_pos"][1] = 2 ** 50; s["out_pos"][1] = 2 ** 50 // D
    Q.pfb_state_check(p, B, s.tobytes())
    s = good.copy(); s["in_pos"][1] = 2 ** 50 + 1; s["out_pos"][1] = 2 ** 50 // D + 1
    refused(s, "band 1: in_pos")
    s = good.copy(); s["in_pos"][0] = -1
    refused(s, "band 0: in_pos")
    for d in (-1, 1):
        s = good.copy(); s["out_pos"][1] += d
        refused(s, "band 1: out_pos")
    s = good.copy(); s["in_pos"][0] = D + 1            # ceil((D + 1) / D) = 2, the record says 1
    refused(s, "band 0: out_pos")
    s = good.copy(); s["hist"][0, L - 6, 1] = 1.0
    refused(s, r"band 0: hist\[%d\]" % (L - 6))
    s = good.copy(); s["hist"][0, 0, 0] = -0.0
    refused(s, r"band 0: hist\[0\]")
    s = good.copy(); s["hist"][0, L - 5, 0] = np.nan; s["hist"][1, 0, 1] = np.inf   # the history proper: any bits
    Q.pfb_state_check(p, B, s.tobytes())
    for k in (0, 47):
        s = good.copy(); s["reserved"][1, k] = 1
        refused(s, "band 1: reserved")
    for blob_ in (blob[:-1], blob + b"\0", blob[: len(blob) // 2], b""):
        with pytest.raises(ValueError):
            Q.pfb_state_check(p, B, blob_)
    with pytest.raises(ValueError):
        Q.pfb_state_check(Q.pfb_params(channels=M, taps_per_branch=K + 1), B, blob)
    assert Q.lib().qpsk_pfb_state_check(C.byref(p), B, None, len(blob)) == Q.QPSK_ERR_ARGUMENT_NULL
    assert Q.lib().qpsk_pfb_state_check(C.byref(p), 0, blob, 0) == Q.QPSK_ERR_ARGUMENT


def test_what_the_host_form_refuses_changes_nothing():
    M, K, B, n = 16, 2, 2, 40
    p = Q.pfb_params(channels=M, taps_per_branch=K)
    x = PC.random_rows(B, 100, seed=10)
    _, blob = host_sequence(p, x, [[30, 30]])
    need = Q.pfb_count(M, 4, 30 + n)
    L_ = Q.lib()

    def call(state, rows, stride_in, out, stride_out, cap, n_s, lengths, n_out):
        lp = None if lengths is None else np.array(lengths, np.int64).ctypes.data_as(C.POINTER(C.c_int64))
        return L_.qpsk_pfb_apply_host(C.byref(p), None, state, len(state), B, rows.ctypes.data, stride_in, out.ctypes.data,
                                      stride_out, cap, n_s, lp, n_out.ctypes.data_as(C.POINTER(C.c_int64)))

    rows = np.array(x[:, : 2 * n])
    big = np.full(B * M * 2 * need + 4 * n * B, f32(-5.0))
    out = np.full((B * M, 2 * need), f32(-5.0))
    n_out = np.full(B, -9, np.int64)
    st = C.create_string_buffer(blob, len(blob))
    bad = np.frombuffer(blob, Q.pfb_state_dtype(M, K)).copy()
    bad["out_pos"][1] += 1
    bad_st = C.create_string_buffer(bad.tobytes(), len(blob))
    A = Q.QPSK_ERR_ARGUMENT
    assert call(st, rows, 2 * n, out, 2 * need, need - 1, n, None, n_out) == A            # one short of capacity
    assert "would emit" in Q.lib().qpsk_last_error().decode()
    assert call(st, rows, 2 * n, out, 2 * need, need, n, [1, n + 1], n_out) == A          # a length past n_samples
    assert call(st, rows, 2 * n, out, 2 * need, need, n, [-1, 1], n_out) == A
    assert call(st, rows, 2 * n - 2, out, 2 * need, need, n, None, n_out) == A            # strides too small
    assert call(st, rows, 2 * n, out, 2 * need - 2, need, n, None, n_out) == A
    assert call(st, big[: 4 * n], 2 * n, big[2 * n:], 2 * need, need, n, None, n_out) == A    # overlapping rows
    assert call(bad_st, rows, 2 * n, out, 2 * need, need, n, None, n_out) == A            # a bad state
    assert "band 1: out_pos" in Q.lib().qpsk_last_error().decode()
    assert call(st, rows, 2 * n, out, 2 * need, need, -1, None, n_out) == A
    assert st.raw == blob and (out == f32(-5.0)).all() and (big == f32(-5.0)).all() and (n_out == -9).all()
    assert call(st, rows, 2 * n, out, 2 * need, need, n, None, n_out) == 0 and (n_out == need).all()
    assert st.raw != blob


# The yardstick's largest error against the filter-bank sum in complex128, as a
# multiple of eps * sum_n |h[n]| |x[m D - n]| (eps = 2^-24), measured per M on
# the rows of the test below (K = 2, frames 1 .. 7, every channel up to M = 256
# and 256 drawn ones above; DESIGN.md 3.18 has the table).  The test
# asserts 4 x these, so that another summation order within the rule's freedom
# still passes.
MEASURED_EPS = {8: 1.04, 16: 1.42, 32: 1.28, 64: 1.02, 128: 0.80, 256: 0.78, 512: 0.46, 1024: 0.36, 2048: 0.34,
                4096: 0.23}


@pytest.mark.parametrize("M", PC.CHANNELS)
def test_the_definition_equals_the_filter_bank_sum_in_float64(M):
    K, frames = 2, 8
    D = M // 2
    x = PC.random_rows(1, frames * D, seed=100 + M)[0]
    h, W = Q.pfb_design(Q.pfb_params(channels=M, taps_per_branch=K)), Q.pfb_twiddles(M)
    y = PC.pfb_reference(x, M, K, h, W)
    m = np.arange(1, frames)                             # frame 0 reads x[0] = +0 alone: no scale
    c = np.arange(M) if M <= 256 else np.random.default_rng(M).choice(M, 256, replace=False)
    exact, scale = PC.pfb_exact(x, M, K, h, m, c)
    got = (y[:, 0::2].astype(np.float64) + 1j * y[:, 1::2].astype(np.float64))[c, 1:]
    err = float((np.abs(got - exact) / scale[None, :]).max() / 2.0 ** -24)
    print(f"M = {M}: yardstick error {err:.3f} eps of sum |h||x|")
    assert err <= 4 * MEASURED_EPS[M]
