"""The polyphase synthesis bank's host half (qpsk_sfb_*, csrc/qpsk_sfb.cpp): the
exports, the parameter edges, the host form of the call (qpsk_sfb_apply_host)
against the numpy yardstick at tolerance 0, the state and its check, what a
refused call leaves behind, and the yardstick itself against the filter-bank
sum in float64.  Needs no GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pfb_cases as PC
import qpsk_amd as Q
import sfb_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["qpsk_sfb_params_init", "qpsk_sfb_create", "qpsk_sfb_destroy", "qpsk_sfb_set_stream", "qpsk_sfb_set_taps",
           "qpsk_sfb_tile_frames", "qpsk_sfb_apply_fmt", "qpsk_sfb_state_size", "qpsk_sfb_state_init",
           "qpsk_sfb_get_state", "qpsk_sfb_set_state", "qpsk_sfb_reset_bands", "qpsk_sfb_state_check",
           "qpsk_sfb_apply_host"]
f32 = np.float32


def design(M, K):
    return Q.pfb_design(Q.pfb_params(channels=M, taps_per_branch=K))


def test_header_library_and_binding_agree_on_the_entry_points():
    src = open(os.path.join(ROOT, "include", "qpsk_demod.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", Q.LIB_PATH]).decode()
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert re.search(r"\bT " + name + r"\b", nm), name
        assert name in Q.EXPORTED_SYMBOLS
    assert re.search(r"#define\s+QPSK_ABI_VERSION\s+3\b", src) and Q.lib().qpsk_abi_version() == 3
    for name, value in (("QPSK_SFB_STATE_HEAD", Q.SFB_STATE_HEAD), ("QPSK_SFB_TILE_TRANSFORM", Q.SFB_TILE_TRANSFORM),
                        ("QPSK_SFB_TILE_SUM", Q.SFB_TILE_SUM), ("QPSK_SFB_TILE_SLAB", Q.SFB_TILE_SLAB)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", src), name
    for m in ("apply_host", "apply_device", "out_len", "set_taps", "get_state", "set_state", "reset_bands", "set_stream"):
        assert callable(getattr(Q.SynthesisBank, m)), m
    assert issubclass(Q.SynthesisBank, Q._RowStage)
    assert C.sizeof(Q.SfbParams) == 60
    assert not re.search(r"form,\s+(\*\s+)?the synthesis bank\.", src), "the channeliser's list of what is not built"


def test_params_init_defaults_and_tile_frames():
    p = Q.sfb_params()
    assert (p.channels, p.taps_per_branch, p.device) == (64, 8, 0) and not any(p.reserved)
    assert Q.sfb_state_size(p) == 64 + 8 * 64 * 15
    assert Q.sfb_state_init(p, 3) == bytes(3 * (64 + 8 * 64 * 15))
    for M in PC.CHANNELS:
        for K in (1, 2, 8):
            T = Q.sfb_tile_frames(M, K, Q.SFB_TILE_TRANSFORM)
            assert T == SC.transform_tile(M, K) and 1 <= T <= PC.tile_frames(M) and (T + 2 * K - 1) % PC.tile_frames(M) == 0
            assert Q.sfb_tile_frames(M, K, Q.SFB_TILE_SUM) == SC.SUM_RUN
            assert Q.sfb_tile_frames(M, K, Q.SFB_TILE_SLAB) == SC.slab_frames(M)
    assert Q.lib().qpsk_sfb_tile_frames(64, 8, 3) == Q.QPSK_ERR_ARGUMENT
    assert Q.lib().qpsk_sfb_tile_frames(64, 8, -1) == Q.QPSK_ERR_ARGUMENT
    assert Q.lib().qpsk_sfb_tile_frames(4, 8, 0) == Q.QPSK_ERR_OUT_OF_RANGE
    assert Q.lib().qpsk_sfb_tile_frames(64, 17, 0) == Q.QPSK_ERR_OUT_OF_RANGE


@pytest.mark.parametrize("kw", [dict(channels=4), dict(channels=8192), dict(channels=24), dict(channels=0),
                                dict(channels=-16), dict(taps_per_branch=0), dict(taps_per_branch=17),
                                dict(channels=4096, taps_per_branch=16), dict(channels=4096, taps_per_branch=9)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_bad_parameters_are_refused_before_a_device_is_touched(kw):
    p = Q.sfb_params(**kw)
    h = C.c_void_p()
    assert Q.lib().qpsk_sfb_create(C.byref(p), 1, C.byref(h)) == Q.QPSK_ERR_OUT_OF_RANGE and not h.value
    assert Q.lib().qpsk_sfb_state_size(C.byref(p)) == Q.QPSK_ERR_OUT_OF_RANGE
    with pytest.raises(ValueError):
        Q.sfb_state_init(p, 1)


def test_the_largest_shapes_are_accepted_and_band_counts_are_checked():
    for M, K in ((4096, 8), (2048, 16), (8, 1), (8, 16)):
        assert Q.sfb_state_size(Q.sfb_params(channels=M, taps_per_branch=K)) == 64 + 8 * M * (2 * K - 1)
    p, h = Q.sfb_params(), C.c_void_p()
    for n_bands in (0, -1, 65536):
        assert Q.lib().qpsk_sfb_create(C.byref(p), n_bands, C.byref(h)) == Q.QPSK_ERR_ARGUMENT
    assert Q.lib().qpsk_sfb_create(None, 1, C.byref(h)) == Q.QPSK_ERR_ARGUMENT_NULL
    assert Q.lib().qpsk_sfb_create(C.byref(p), 1, None) == Q.QPSK_ERR_ARGUMENT_NULL
    assert Q.lib().qpsk_sfb_state_size(None) == Q.QPSK_ERR_ARGUMENT_NULL


def host_sequence(p, x, calls, taps=None, scale_out=1.0):
    """The call sequence through qpsk_sfb_apply_host (x [B M, 2 n]; calls: per
    call the [B] lengths in frames), the state against the model after every
    call.  Returns per band the [2 samples] row of everything emitted, and the
    final state."""
    M, K = p.channels, p.taps_per_branch
    B, D = x.shape[0] // M, M // 2
    dt = Q.sfb_state_dtype(M, K)
    state = Q.sfb_state_init(p, B)
    models = [SC.PySfb(M, K) for _ in range(B)]
    pos = np.zeros(B, np.int64)
    got = [[] for _ in range(B)]
    for ci, lens in enumerate(calls):
        n = max(lens)
        rows = np.zeros((B * M, 2 * max(n, 1)), f32)
        for b in range(B):
            rows[b * M: (b + 1) * M, : 2 * lens[b]] = x[b * M: (b + 1) * M, 2 * pos[b]: 2 * (pos[b] + lens[b])]
        out = np.full((B, 2 * max(n, 1) * D), f32(-77.0))
        uniform = all(l == lens[0] for l in lens)
        state, o = Q.sfb_apply_host(p, state, rows, lengths=None if uniform else lens, out=out, n=n, taps=taps,
                                    scale_out=scale_out)
        assert o is out
        st = np.frombuffer(state, dt)
        for b in range(B):
            assert models[b].call(rows[b * M: (b + 1) * M, : 2 * lens[b]]) == lens[b] * D
            assert st[b].tobytes() == models[b].record(dt).tobytes(), f"state after call {ci}, band {b}"
            assert (out[b, 2 * lens[b] * D:] == f32(-77.0)).all(), f"call {ci} band {b}: written past its samples"
            got[b].append(out[b, : 2 * lens[b] * D].copy())
        Q.sfb_state_check(p, B, state)
        pos += np.array(lens)
    return [np.concatenate(g) for g in got], state


def assert_row_equal(got, want, what):
    assert got.shape == want.shape, f"{what}: {got.shape} vs {want.shape}"
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        pytest.fail(f"{what}: {bad.size} floats differ, first at sample {bad[0] // 2}: {got[bad[0]]!r} vs {want[bad[0]]!r}")


@pytest.mark.parametrize("M,K", [(M, 2) for M in PC.CHANNELS] + [(16, K) for K in PC.BRANCH_TAPS if K != 2])
def test_host_form_equals_the_yardstick_over_call_cuts(M, K):
    """Tolerance 0, signed zeros included, on finite rows; calls of 0, 1, 2,
    2K - 2, 2K - 1, 2K and 6K + 1 frames; the second band takes them in another
    order, so most calls carry different lengths."""
    cuts = SC.call_cuts(K)
    B, n = 2, sum(cuts)
    x = SC.random_rows(B, M, n, seed=M + K)
    p = Q.sfb_params(channels=M, taps_per_branch=K)
    calls = [[cuts[i], cuts[(i + 3) % len(cuts)]] for i in range(len(cuts))]
    scale = f32(M // 2)
    got, _ = host_sequence(p, x, calls, scale_out=scale)
    g, W = design(M, K), Q.pfb_twiddles(M)
    for b in range(B):
        want = SC.sfb_reference(x[b * M: (b + 1) * M], M, K, g, W, scale_out=scale)
        assert want.size == 2 * n * (M // 2)
        assert_row_equal(got[b], want, f"M = {M}, K = {K}, band {b}")


def test_silence_comes_out_as_plus_zero():
    """+0 and -0 in: every product is a zero of some sign, acc starts at +0 and
    +0 + -0 = +0, so every output is +0 whatever the frame's sign step did."""
    M, K = 16, 2
    p = Q.sfb_params(channels=M, taps_per_branch=K)
    x = np.zeros((M, 2 * 9), f32)
    x[1::2] = f32(-0.0)
    got, _ = host_sequence(p, x, [[3], [6]])
    assert_row_equal(got[0], SC.sfb_reference(x, M, K, design(M, K), Q.pfb_twiddles(M)), "silence")
    assert (got[0].view(np.uint32) == 0).all()


def test_host_form_with_taps_of_the_callers_and_a_scale():
    M, K = 32, 3
    x = SC.random_rows(1, M, 40, seed=5)
    taps = (np.random.default_rng(6).standard_normal(M * K) * 0.2).astype(f32)
    scale = f32(np.sqrt(8.0))
    p = Q.sfb_params(channels=M, taps_per_branch=K)
    got, _ = host_sequence(p, x, [[15], [25]], taps=taps, scale_out=scale)
    assert_row_equal(got[0], SC.sfb_reference(x, M, K, taps, Q.pfb_twiddles(M), scale_out=scale), "own taps and a scale")
    bad = taps.copy()
    bad[7] = np.inf
    with pytest.raises(ValueError, match="tap 7"):
        Q.sfb_apply_host(p, Q.sfb_state_init(p, 1), np.zeros((M, 8), f32), taps=bad)
    for s in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="scale_out"):
            Q.sfb_apply_host(p, Q.sfb_state_init(p, 1), np.zeros((M, 8), f32), scale_out=s)


def test_one_row_comes_out_as_its_carrier():
    """A constant on row c alone, scale_out = D: behind the prototype's length
    the wideband row is that constant times e^{+j 2 pi c i / M} (DC gain 1 of a
    prototype applied at rate fs after an upsampling by D), up to the
    prototype's images at the other multiples of fs / D, which its stop band
    holds below 2e-3."""
    M, K, n, c = 16, 8, 80, 3
    D = M // 2
    x = np.zeros((M, 2 * n), f32)
    x[c, 0::2], x[c, 1::2] = 0.75, -0.5
    p = Q.sfb_params(channels=M, taps_per_branch=K)
    _, out = Q.sfb_apply_host(p, Q.sfb_state_init(p, 1), x, scale_out=D)
    y = out[0, 0::2].astype(np.float64) + 1j * out[0, 1::2]
    i = np.arange(n * D)
    want = (0.75 - 0.5j) * np.exp(2j * np.pi * c * i / M)
    assert np.abs(y - want)[M * K:].max() < 2e-3


def test_state_check_at_and_past_every_edge():
    M, K, B = 16, 2, 2
    D, H = M // 2, 2 * K - 1
    p = Q.sfb_params(channels=M, taps_per_branch=K)
    dt = Q.sfb_state_dtype(M, K)
    x = SC.random_rows(B, M, 10, seed=9)
    _, blob = host_sequence(p, x, [[1, 10]])             # band 0: hist frames 0 and 1 lie before its start
    good = np.frombuffer(blob, dt).copy()
    top = 2 ** 50 // D

    def refused(rec, match):
        with pytest.raises(ValueError, match=match):
            Q.sfb_state_check(p, B, rec.tobytes())

    Q.sfb_state_check(p, B, good.tobytes())
    s = good.copy(); s["in_pos"][1] = top; s["out_pos"][1] = top * D
    Q.sfb_state_check(p, B, s.tobytes())
    s = good.copy(); s["in_pos"][1] = top + 1; s["out_pos"][1] = (top + 1) * D
    refused(s, "band 1: in_pos")
    s = good.copy(); s["in_pos"][0] = -1; s["out_pos"][0] = -D
    refused(s, "band 0: in_pos")
    for d in (-1, 1):
        s = good.copy(); s["out_pos"][1] += d
        refused(s, "band 1: out_pos")
    s = good.copy(); s["in_pos"][0] = 2                  # the record says 1 * D
    refused(s, "band 0: out_pos")
    s = good.copy(); s["hist"][0, H - 2, M - 1, 1] = 1.0
    refused(s, r"band 0: hist\[%d\]\[%d\]" % (H - 2, M - 1))
    s = good.copy(); s["hist"][0, 0, 0, 0] = -0.0
    refused(s, r"band 0: hist\[0\]\[0\]")
    s = good.copy(); s["hist"][0, H - 1, 0, 0] = np.nan; s["hist"][1, 0, 0, 1] = np.inf   # the history proper: any bits
    Q.sfb_state_check(p, B, s.tobytes())
    for k in (0, 47):
        s = good.copy(); s["reserved"][1, k] = 1
        refused(s, "band 1: reserved")
    for blob_ in (blob[:-1], blob + b"\0", blob[: len(blob) // 2], b""):
        with pytest.raises(ValueError):
            Q.sfb_state_check(p, B, blob_)
    with pytest.raises(ValueError):
        Q.sfb_state_check(Q.sfb_params(channels=M, taps_per_branch=K + 1), B, blob)
    assert Q.lib().qpsk_sfb_state_check(C.byref(p), B, None, len(blob)) == Q.QPSK_ERR_ARGUMENT_NULL
    assert Q.lib().qpsk_sfb_state_check(C.byref(p), 0, blob, 0) == Q.QPSK_ERR_ARGUMENT


def test_what_the_host_form_refuses_changes_nothing():
    M, K, B, n = 16, 2, 2, 5
    D = M // 2
    p = Q.sfb_params(channels=M, taps_per_branch=K)
    x = SC.random_rows(B, M, 20, seed=10)
    _, blob = host_sequence(p, x, [[4, 4]])
    L_ = Q.lib()

    def call(state, rows, stride_in, out, stride_out, n_f, lengths, scale=1.0):
        lp = None if lengths is None else np.array(lengths, np.int64).ctypes.data_as(C.POINTER(C.c_int64))
        return L_.qpsk_sfb_apply_host(C.byref(p), None, state, len(state), B, rows.ctypes.data, stride_in, out.ctypes.data,
                                      stride_out, C.c_float(scale), n_f, lp)

    rows = np.array(x[:, : 2 * n])
    big = np.full(B * M * 2 * n + B * 2 * n * D, f32(-5.0))
    out = np.full((B, 2 * n * D), f32(-5.0))
    st = C.create_string_buffer(blob, len(blob))
    bad = np.frombuffer(blob, Q.sfb_state_dtype(M, K)).copy()
    bad["out_pos"][1] += 1
    bad_st = C.create_string_buffer(bad.tobytes(), len(blob))
    top = np.frombuffer(blob, Q.sfb_state_dtype(M, K)).copy()
    top["in_pos"][0] = 2 ** 50 // D - n + 1
    top["out_pos"][0] = top["in_pos"][0] * D
    top_st = C.create_string_buffer(top.tobytes(), len(blob))
    A = Q.QPSK_ERR_ARGUMENT
    assert call(st, rows, 2 * n, out, 2 * n * D, n, [1, n + 1]) == A                      # a length past n_frames
    assert call(st, rows, 2 * n, out, 2 * n * D, n, [-1, 1]) == A
    assert call(st, rows, 2 * n - 2, out, 2 * n * D, n, None) == A                        # strides too small
    assert call(st, rows, 2 * n, out, 2 * n * D - 2, n, None) == A
    assert call(st, big, 2 * n, big[B * M * 2 * n - 2:], 2 * n * D, n, None) == A         # overlapping rows
    assert call(bad_st, rows, 2 * n, out, 2 * n * D, n, None) == A                        # a bad state
    assert "band 1: out_pos" in Q.lib().qpsk_last_error().decode()
    assert call(top_st, rows, 2 * n, out, 2 * n * D, n, None) == A                        # past the last position
    assert "band 0 would pass" in Q.lib().qpsk_last_error().decode()
    assert call(st, rows, 2 * n, out, 2 * n * D, -1, None) == A
    assert call(st, rows, 2 * n, out, 2 * n * D, n, None, scale=0.0) == Q.QPSK_ERR_OUT_OF_RANGE
    assert st.raw == blob and top_st.raw == top.tobytes() and (out == f32(-5.0)).all() and (big == f32(-5.0)).all()
    assert call(st, rows, 2 * n, out, 2 * n * D, n, None) == 0 and not (out == f32(-5.0)).any()
    assert st.raw != blob
    top["in_pos"][0] -= 1
    top["out_pos"][0] -= D
    top_st = C.create_string_buffer(top.tobytes(), len(blob))
    assert call(top_st, rows, 2 * n, out, 2 * n * D, n, None) == 0                        # exactly up to it
    assert np.frombuffer(top_st.raw, Q.sfb_state_dtype(M, K))["in_pos"][0] == 2 ** 50 // D


# The yardstick's largest error against the filter-bank sum in complex128, as a
# multiple of eps * scale_out * sum_c sum_m |g[i - m D]| |s_c[m]| (eps = 2^-24),
# measured per M on the rows of the test below (K = 2, 8 frames, scale_out = D,
# every output sample up to M = 64 and 256 drawn ones above; DESIGN.md 3.20 has
# the table).  The test asserts 4 x these, so that another summation order
# within the rule's freedom still passes.
MEASURED_EPS = {8: 0.53, 16: 0.73, 32: 0.54, 64: 0.44, 128: 0.40, 256: 0.37, 512: 0.30, 1024: 0.14, 2048: 0.14,
                4096: 0.07}


@pytest.mark.parametrize("M", PC.CHANNELS)
def test_the_definition_equals_the_filter_bank_sum_in_float64(M):
    K, frames = 2, 8
    D = M // 2
    # normal floats only: a denormal's rounding error is absolute, 2^-150, not 2^-24 of its size
    x = np.random.default_rng(100 + M).standard_normal((M, 2 * frames)).astype(f32)
    g = design(M, K)
    y = SC.sfb_reference(x, M, K, g, Q.pfb_twiddles(M), scale_out=f32(D))
    i = np.arange(1, frames * D)                         # sample 0 reads g[0] = +0 alone: no scale
    if M > 64:
        i = np.sort(np.random.default_rng(M).choice(i, 256, replace=False))
    exact, scale = SC.sfb_exact(x, M, K, g, i)
    got = y[0::2].astype(np.float64)[i] + 1j * y[1::2].astype(np.float64)[i]
    err = float((np.abs(got - D * exact) / (D * scale)).max() / 2.0 ** -24)
    print(f"M = {M}: yardstick error {err:.3f} eps of scale_out sum |g||s|")
    assert err <= 4 * MEASURED_EPS[M]


@pytest.mark.parametrize("fmt", ["cf32", "cs16", "cs8"])
def test_the_cpu_chain_receives_every_frame(fmt):
    """The condition of tests/test_gpu_sfb.py's chain, so that it is no equality
    of nothing: oracle.modulate_bytes -> sfb_reference (+ quantiser) ->
    pfb_reference -> OracleDemod.DeModulateBytes receives all 48 frames, round 0
    included, and the integer hops do not clip."""
    n, peak, want = SC.wideband_case(fmt)
    for c in range(SC.E2E["M"]):
        for k in range(SC.E2E["rounds"]):
            assert want[c][k] == SC.payload(c, k), f"the CPU chain lost carrier {c} round {k}"
    print(f"{fmt}: {n} frames a round, largest wideband element {peak}")
    assert fmt == "cf32" or peak < {"cs16": 32767, "cs8": 127}[fmt]
