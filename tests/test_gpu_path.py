"""The propagation path on the device (qpsk_path_*, csrc/qpsk_path.hip) against
the numpy yardstick (path_cases.path_reference), byte for byte against its own
host form (qpsk_path_apply_host), and its state against the Python model after
every call.  Every comparison is at tolerance 0; inputs are finite (a NaN's
payload is the one thing an x86 host and gfx950 do not share).

The kernel gives a workgroup QPSK_PATH_TILE_OUTPUTS = 1024 outputs of a call;
the call lengths below straddle that, the 16-sample history and the sizes at
which the 16-byte loads begin and end."""
import functools

import numpy as np
import pytest

import common as K
import gpu_harness as H
import oracle as O
import path_cases as PC
import qpsk_amd
from gpu_harness import Q, dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

T = qpsk_amd.PATH_TILE_OUTPUTS
DT = qpsk_amd.PATH_STATE_DTYPE
# a stream's calls in order, rotated by its index: 4000 samples in all
CUTS = [0, 1, 2, 3, 5, 16, 17, 63, 64, 65, 1023, 1024, 1025, 692]
assert sum(CUTS) == 4000
FULL = {"cf32": 1.0, "cs16": 32767.0, "cs8": 127.0, "cu8": 127.0}
CLOCKS = [(1 - 1e-3, 0.25), (1.0, 0.0), (1 + 1e-3, 0.75)]


def calls_for(S, cuts=CUTS):
    return [[cuts[(c + s) % len(cuts)] for s in range(S)] for c in range(len(cuts))]


@functools.lru_cache(maxsize=None)
def random_rows(S, n, seed=0):
    """[S, 2 n] float32 with +-0 and denormals up front."""
    x = np.random.default_rng(seed).standard_normal((S, 2 * n)).astype(np.float32)
    head = np.array([0.0, -0.0, 1e-45, -1e-40, 1.0, -1.0, -0.0, 3e-39], np.float32)
    x[:, : head.size] = head
    x[1::2, : head.size] = head[::-1]
    x.setflags(write=False)
    return x


def taps_of(L, seed=3):
    t = (np.random.default_rng(seed + L).standard_normal((L, 2)) * 0.3).astype(np.float32)
    t[0] = [1.0, 0.0] if L == 1 else [0.9, -0.1]
    return t


def sentinel_rows(torch, S, n_cap, dtype="float32", lead_bytes=0):
    """Device rows [S, 2 n_cap] of dtype whose every byte is 0xAA; row 0 starts
    lead_bytes into a 16-byte aligned allocation and the pitch is a multiple of
    16 bytes plus lead_bytes' residue, so lead_bytes = 0 gives rows the 16-byte
    loads take and any other value rows they cannot."""
    dt = getattr(torch, dtype)
    size = torch.empty(0, dtype=dt).element_size()
    pitch = (2 * n_cap * size + 15) // 16 * 16 + (16 if lead_bytes else 0)
    buf = torch.full((S * pitch + 16,), 0xAA, dtype=torch.uint8, device="cuda")
    flat = buf[lead_bytes: lead_bytes + (S * pitch) // size * size].view(dt)
    rows = torch.as_strided(flat, (S, 2 * n_cap), (pitch // size, 1))
    assert rows.data_ptr() % 16 == lead_bytes
    return rows


def make(Q, S, clocks=None, taps=None, **fields):
    """A handle whose stream s has clocks[s] = (r, tau) and taps[s] ([L, 2]), set through its state."""
    pa = Q.Path(S, **fields)
    if clocks is not None or taps is not None:
        st = pa.states()
        for s in range(S):
            if clocks is not None:
                st["r"][s], st["tau"][s] = clocks[s]
            if taps is not None:
                st["n_taps"][s] = taps[s].shape[0]
                st["taps"][s] = 0
                st["taps"][s, : taps[s].shape[0]] = taps[s]
        pa.set_state(st.tobytes())
    return pa


def device_calls(torch, pa, x, calls, models=None, fmt="cf32", out_fmt=None, lead_bytes=0, scale_in=None):
    """The call sequence on device rows of their own (0xAA behind every row's
    count); per call the [S] list of output rows.  models: per stream a PyPath
    (fed the widened floats wx); the handle's state is compared after every call."""
    S = x.shape[0]
    F, FO = H.FORMATS[fmt], H.FORMATS[out_fmt or fmt]
    pos = np.zeros(S, np.int64)
    out = []
    for ci, lens in enumerate(calls):
        n = max(lens)
        rows = sentinel_rows(torch, S, max(n, 1), F.torch_dtype, lead_bytes)
        host = rows.cpu().numpy().copy()
        for s in range(S):
            host[s, : 2 * lens[s]] = x[s, 2 * pos[s]: 2 * (pos[s] + lens[s])]
        rows.copy_(torch.from_numpy(host))
        cap = pa.out_bound(n)
        o = sentinel_rows(torch, S, cap, FO.torch_dtype, lead_bytes)
        n_out = pa.apply_device(rows, n, o, fmt=fmt, out_fmt=out_fmt, lengths=H.lengths_of(lens), out_cap=cap,
                                scale_in=scale_in)
        got = o.cpu().numpy()
        assert np.array_equal(rows.cpu().numpy(), host), f"call {ci}: the input rows changed"
        for s in range(S):
            assert (got[s, 2 * n_out[s]:].view(np.uint8) == 0xAA).all(), f"call {ci} stream {s}: written past its count"
        out.append([got[s, : 2 * n_out[s]].copy() for s in range(S)])
        if models:
            st = pa.states()
            for s in range(S):
                w = host[s, : 2 * lens[s]] if fmt == "cf32" else H.widened(host[s, : 2 * lens[s]], fmt, scale_in)
                assert models[s].call(w) == n_out[s], (ci, s)
                assert st[s].tobytes() == models[s].record(DT).tobytes(), f"state after call {ci}, stream {s}"
        pos += np.array(lens)
    return out


def joined(outs, s):
    return np.concatenate([c[s] for c in outs])


def assert_bits(got, want, what):
    assert got.shape == want.shape, f"{what}: {got.size // 2} outputs vs {want.size // 2}"
    if not K.bitwise_equal(got, want):
        bad = np.flatnonzero(got != want) if got.dtype.kind != "f" else np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        pytest.fail(f"{what}: {bad.size} elements differ, first at output {bad[0] // 2}: {got[bad[0]]!r} vs {want[bad[0]]!r}")


# ---------------------------------------------------------------------------
# 1. the kernel against the yardstick and against the host form
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("lead_bytes", [0, 4], ids=["16-byte rows", "4-byte rows"])
def test_kernel_equals_the_yardstick_and_the_host_form_over_a_ragged_cut(Q, dev, lead_bytes):
    S, n = 3, 4000
    x, calls = random_rows(S, n), calls_for(S)
    taps = [taps_of(1), PC.project_taps(), taps_of(8)]
    models = [PC.PyPath(*CLOCKS[s], taps[s]) for s in range(S)]
    pa = make(Q, S, CLOCKS, taps)
    state = pa.get_state()
    got = device_calls(dev, pa, x, calls, models, lead_bytes=lead_bytes)
    pa.close()
    # the host form over the same calls
    pos = np.zeros(S, np.int64)
    for ci, lens in enumerate(calls):
        rows = H.call_rows(np.array(x), lens, pos)
        if rows.shape[1] == 0:
            rows = np.zeros((S, 2), np.float32)
        state, out, n_out = Q.path_apply_host(state, np.ascontiguousarray(rows), lengths=lens, n=max(lens))
        for s in range(S):
            assert out[s, : 2 * n_out[s]].tobytes() == got[ci][s].tobytes(), f"call {ci} stream {s}: device vs host form"
        pos += np.array(lens)
    for s in range(S):
        assert_bits(joined(got, s), PC.path_reference(x[s], *CLOCKS[s], taps[s]), f"stream {s}")


def test_identity_returns_the_rows_two_samples_short(Q, dev):
    S, n = 2, 2500
    x = random_rows(S, n, seed=1)
    pa = Q.Path(S)
    got = device_calls(dev, pa, x, [[n] * S])
    pa.close()
    for s in range(S):
        back = np.array(x[s, : 2 * (n - 2)])
        back[H.is_neg_zero(back)] = 0.0
        assert_bits(got[0][s], back, f"stream {s}")
        assert H.is_neg_zero(np.array(x[s])).any() and not H.is_neg_zero(got[0][s]).any()


# ---------------------------------------------------------------------------
# 2. tile edges and index slips
# ---------------------------------------------------------------------------
def lens_emitting(model, counts):
    """Call lengths after which a stream like model (copied) emits counts[i] in
    call i.  Where a count cannot be had (r < 1: one more input can add two
    outputs) a call of one sample goes first.  Returns the lengths and which
    of the calls are the counted ones."""
    m = PC.PyPath(model.r, model.tau, model.taps)
    lens, counted = [], []
    for c in counts:
        for _ in range(4):
            fit = [n for n in range(max(c - 8, 0), c + 12) if PC.py_count(m.r, m.tau, m.out_pos, m.in_pos + n) == c]
            if fit:
                break
            lens.append(1)
            m.call(np.zeros(2, np.float32))
        assert fit, c
        counted.append(len(lens))
        lens.append(fit[0])
        assert m.call(np.zeros(2 * fit[0], np.float32)) == c
    return lens, counted


@pytest.mark.parametrize("side", [0, 1], ids=["slip on a tile's last output", "slip on a tile's first output"])
@pytest.mark.parametrize("r", [1 - 1e-3, 1 + 1e-3], ids=["an index repeats", "an index is skipped"])
def test_tile_edges_with_an_index_slip_on_either_side(Q, dev, r, side):
    tau, k = PC.slip_clock(r, T - 1, side)
    step = int(np.floor(PC.p_of(r, tau, k))) - int(np.floor(PC.p_of(r, tau, k - 1)))
    assert k == T - 1 + side and step == (0 if r < 1 else 2)
    taps = PC.project_taps()
    model = PC.PyPath(r, tau, taps)
    counts = [2 * T + 3, T - 1, T, T + 1]             # the first call's tiles end at outputs T - 1 and 2 T - 1
    lens, counted = lens_emitting(model, counts)
    x = random_rows(1, sum(lens), seed=2)
    pa = make(Q, 1, [(r, tau)], [taps])
    got = device_calls(dev, pa, x, [[n] for n in lens], [model])
    pa.close()
    assert [got[ci][0].size // 2 for ci in counted] == counts
    assert_bits(joined(got, 0), PC.path_reference(x[0], r, tau, taps), "tile edges")


# ---------------------------------------------------------------------------
# 3. batches, taps of every length
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 3])
def test_batches_with_distinct_clocks_and_per_stream_taps_of_every_length(Q, dev, S):
    n = 300
    x = random_rows(S, n, seed=3)
    calls = [[7 + s for s in range(S)], [150] * S, [143 - s for s in range(S)]]
    for L in range(1, qpsk_amd.PATH_MAX_TAPS + 1):
        clocks = [PC.clock(10 + s, 100.0 * (L - 4), 200.0, 42, 0.0, True) for s in range(S)]
        taps = [taps_of(L, seed=10 * s) for s in range(S)]
        pa = Q.Path(S, clock_ppm=100.0 * (L - 4), clock_spread=200.0, clock_seed=42, tau_random=1, first_stream=10)
        pa.set_taps(np.stack(taps).view(np.complex64)[..., 0], per_stream=True)
        models = [PC.PyPath(*clocks[s], taps[s]) for s in range(S)]
        got = device_calls(dev, pa, x, calls, models)
        pa.close()
        assert len(set(clocks)) == S
        for s in range(S):
            assert_bits(joined(got, s), PC.path_reference(x[s], *clocks[s], taps[s]), f"L = {L}, stream {s}")


def test_set_taps_for_all_streams_takes_effect_behind_the_calls_so_far(Q, dev):
    S, n = 2, 400
    x = random_rows(S, n, seed=4)
    pa = make(Q, S, CLOCKS[:S])
    a = device_calls(dev, pa, x, [[200] * S])
    t = taps_of(3)
    pa.set_taps(t.view(np.complex64)[:, 0])
    for bad, exc in (([np.nan + 0j], ValueError), ([1.0] * 9, ValueError), ([], ValueError)):
        with pytest.raises(exc):
            pa.set_taps(bad)
    b = device_calls(dev, pa, x[:, 400:], [[200] * S])
    pa.close()
    for s in range(S):
        na = a[0][s].size
        assert_bits(a[0][s], PC.path_reference(x[s], *CLOCKS[s], PC.IDENTITY)[:na], f"before, stream {s}")
        assert_bits(b[0][s], PC.path_reference(x[s], *CLOCKS[s], t)[na:], f"after, stream {s}")


# ---------------------------------------------------------------------------
# 4. formats
# ---------------------------------------------------------------------------
MIN_LEAD = {"cf32": 4, "cs16": 4, "cs8": 2, "cu8": 2}


@functools.lru_cache(maxsize=None)
def fmt_case(fmt):
    """2 streams x 2100 samples of fmt, their widened floats and the yardstick's rows."""
    S, n = 2, 2100
    xi = np.array(random_rows(S, n, seed=5)) if fmt == "cf32" else H.random_rows(S, n, 6, fmt)
    w = xi if fmt == "cf32" else H.widened(xi, fmt)
    clocks = [CLOCKS[0], CLOCKS[2]]
    want = [PC.path_reference(w[s], *clocks[s], PC.project_taps()) for s in range(S)]
    return xi, clocks, want


@pytest.mark.parametrize("fmt_out", ["cf32", "cs16", "cs8", "cu8"])
@pytest.mark.parametrize("fmt_in", ["cf32", "cs16", "cs8", "cu8"])
def test_every_format_pair_on_device_rows_of_both_alignments_and_host_rows(Q, dev, fmt_in, fmt_out):
    xi, clocks, want32 = fmt_case(fmt_in)
    S, n = xi.shape[0], xi.shape[1] // 2
    want = [Q.quantise_iq(want32[s], fmt_out, "fixed", FULL[fmt_out])[0] for s in range(S)]
    taps = [PC.project_taps()] * S
    for lead in (0, max(MIN_LEAD[fmt_in], MIN_LEAD[fmt_out])):
        pa = make(Q, S, clocks, taps)
        got = device_calls(dev, pa, xi, [[n] * S], fmt=fmt_in, out_fmt=fmt_out, lead_bytes=lead)
        pa.close()
        for s in range(S):
            assert_bits(got[0][s], want[s], f"{fmt_in} -> {fmt_out}, lead {lead}, stream {s}")
    # host rows: what lies past a row's count comes back as it was
    FO = H.FORMATS[fmt_out]
    pa = make(Q, S, clocks, taps)
    cap = pa.out_bound(n)
    out = np.frombuffer(b"\xaa" * (S * 2 * cap * np.dtype(FO.np_dtype).itemsize), FO.np_dtype).reshape(S, 2 * cap).copy()
    _, n_out = pa.apply(np.array(xi), fmt=fmt_in, out_fmt=fmt_out, out=out, lengths=[n, n - 100])
    pa.close()
    w1 = xi[1, : 2 * (n - 100)] if fmt_in == "cf32" else H.widened(xi[1, : 2 * (n - 100)], fmt_in)
    short = Q.quantise_iq(PC.path_reference(w1, *clocks[1], PC.project_taps()), fmt_out, "fixed", FULL[fmt_out])[0]
    for s, w in enumerate((want[0], short)):
        assert n_out[s] == w.size // 2
        assert_bits(out[s, : w.size], w, f"host rows {fmt_in} -> {fmt_out}, stream {s}")
        assert (out[s, w.size:].view(np.uint8) == 0xAA).all()


def test_scales_other_than_the_defaults(Q, dev):
    S, n = 2, 500
    xi = H.random_rows(S, n, 7, "cs16")
    scale = H.FORMATS["cs16"].odd_scale
    w = H.widened(xi, "cs16", scale)
    pa = make(Q, S, CLOCKS[:S])
    o = sentinel_rows(dev, S, pa.out_bound(n), "int8")
    n_out = pa.apply_device(dev.from_numpy(xi).cuda(), n, o, fmt="cs16", out_fmt="cs8", scale_in=scale, scale_out=47.0)
    pa.close()
    for s in range(S):
        want = Q.quantise_iq(PC.path_reference(w[s], *CLOCKS[s], PC.IDENTITY), "cs8", "fixed", 47.0)[0]
        assert_bits(o.cpu().numpy()[s, : 2 * n_out[s]], want, f"stream {s}")


# ---------------------------------------------------------------------------
# 5. state
# ---------------------------------------------------------------------------
def test_positions_near_2_40_through_set_state(Q, dev):
    S, n, base = 3, 2 * T + 50, 2 ** 40 - 1000
    taps = [taps_of(8), taps_of(4), taps_of(1)]
    x = random_rows(S, n + 16, seed=8)                 # the first 16 samples are the history
    models = [PC.PyPath(*CLOCKS[s], taps[s]).at(base, x[s, :32]) for s in range(S)]
    k0 = [m.out_pos for m in models]
    pa = Q.Path(S)
    pa.set_state(b"".join(m.record(DT).tobytes() for m in models))
    got = device_calls(dev, pa, x[:, 32:], [[n // 2] * S, [n - n // 2] * S], models)
    st = pa.states()
    pa.close()
    assert (st["in_pos"] == base + n).all() and (st["in_pos"] > 2 ** 40).all()
    for s in range(S):
        want = PC.path_reference(x[s], *CLOCKS[s], taps[s], k0=k0[s], in0=base - 16)
        assert_bits(joined(got, s), want, f"stream {s} across 2^40")


def host_form_calls(Q, state, x, lens):
    """Calls of lens[i] samples on every stream through qpsk_path_apply_host;
    per call the [S] list of output rows, and the state behind them."""
    out, pos = [], 0
    for n in lens:
        state, o, n_out = Q.path_apply_host(state, np.ascontiguousarray(x[:, 2 * pos: 2 * (pos + n)]))
        out.append([o[s, : 2 * n_out[s]].copy() for s in range(x.shape[0])])
        pos += n
    return out, state


def assert_calls_equal_the_host_form(got, want):
    for ci, (ga, wa) in enumerate(zip(got, want)):
        for s, (g, w) in enumerate(zip(ga, wa)):
            assert_bits(g, w, f"call {ci} stream {s}: device vs host form")


def test_host_rows_whose_staging_grows_and_is_reused(Q, dev):
    """Host-memory calls of 40, 1100 and 40 samples on one handle: the staging
    buffers are made, freed for larger ones, and then serve a shorter call.
    1100 samples pass one tile edge."""
    S, lens = 2, [40, 1100, 40]
    x = random_rows(S, sum(lens), seed=11)
    pa = make(Q, S, CLOCKS[:S], [PC.project_taps(), taps_of(8)])
    want, state = host_form_calls(Q, pa.get_state(), x, lens)
    assert max(w.size // 2 for w in want[1]) > T
    got, pos = [], 0
    for n in lens:
        out, n_out = pa.apply(np.ascontiguousarray(x[:, 2 * pos: 2 * (pos + n)]))
        got.append([out[s, : 2 * n_out[s]].copy() for s in range(S)])
        pos += n
    assert pa.get_state() == state
    pa.close()
    assert_calls_equal_the_host_form(got, want)


def test_set_stream_back_to_none_after_a_bound_call(Q, dev):
    """A device call on a bound torch stream, then set_stream(None) and a second
    one on the handle's own stream again, then close(): the caller's stream
    outlives the handle."""
    torch = dev
    S, lens = 2, [40, 1100]
    x = random_rows(S, sum(lens), seed=12)
    pa = make(Q, S, CLOCKS[:S], [PC.project_taps(), taps_of(8)])
    want, state = host_form_calls(Q, pa.get_state(), x, lens)
    cuts = [np.ascontiguousarray(x[:, : 2 * lens[0]]), np.ascontiguousarray(x[:, 2 * lens[0]:])]
    got = []
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        pa.set_stream(st.cuda_stream)
        o = torch.zeros((S, 2 * pa.out_bound(lens[0])), dtype=torch.float32, device="cuda")
        n_out = pa.apply_device(torch.from_numpy(cuts[0]).cuda(), lens[0], o)
        first = o.cpu().numpy()
    got.append([first[s, : 2 * n_out[s]] for s in range(S)])
    pa.set_stream(None)
    o = torch.zeros((S, 2 * pa.out_bound(lens[1])), dtype=torch.float32, device="cuda")
    n_out = pa.apply_device(torch.from_numpy(cuts[1]).cuda(), lens[1], o)
    second = o.cpu().numpy()
    got.append([second[s, : 2 * n_out[s]] for s in range(S)])
    assert pa.get_state() == state
    pa.close()
    st.synchronize()
    assert_calls_equal_the_host_form(got, want)


def test_reset_a_subset_and_move_the_state_to_a_second_handle(Q, dev):
    S, n = 4, 900
    x = random_rows(S, n, seed=9)
    clocks = [CLOCKS[s % 3] for s in range(S)]
    taps = [taps_of(1 + 2 * s) for s in range(S)]
    a = make(Q, S, clocks, taps)
    first = device_calls(dev, a, x, [[300, 17, 300, 5]])
    blob = a.get_state()
    b = Q.Path(S, clock_ppm=500.0, multipath=1)        # what it was made with does not matter
    b.set_state(blob)
    used = np.array([300, 17, 300, 5])
    rest = np.stack([np.roll(x[s], -2 * used[s]) for s in range(S)])
    tail_a = device_calls(dev, a, rest, [[100] * S, [400] * S])
    tail_b = device_calls(dev, b, rest, [[63] * S, [437] * S])
    assert a.get_state() == b.get_state()
    for s in range(S):
        whole = PC.path_reference(x[s, : 2 * (used[s] + 500)], *clocks[s], taps[s])
        assert_bits(np.concatenate([first[0][s], joined(tail_a, s)]), whole, f"stream {s}")
        assert_bits(joined(tail_b, s), joined(tail_a, s), f"second handle, stream {s}")
    # reset streams 2 and 0: their created clock, positions 0, no history, their taps
    for streams in ([], [0, 0], [S], [-1]):
        with pytest.raises(ValueError):
            a.reset_streams(streams)
    before = a.states()
    a.reset_streams([2, 0])
    st = a.states()
    assert (st["in_pos"] == [0, before["in_pos"][1], 0, before["in_pos"][3]]).all()
    assert (st["out_pos"][[0, 2]] == 0).all() and (st["hist"][[0, 2]] == 0).all()
    assert (st["r"][[0, 2]] == 1.0).all() and (st["tau"][[0, 2]] == 0.0).all()
    assert st[[1, 3]].tobytes() == before[[1, 3]].tobytes() and (st["taps"] == before["taps"]).all()
    again = device_calls(dev, a, x, [[200] * S])
    a.close()
    b.close()
    for s in (0, 2):
        assert_bits(again[0][s], PC.path_reference(x[s, :400], 1.0, 0.0, taps[s]), f"reset stream {s}")


def test_what_a_live_handle_refuses_changes_nothing(Q, dev):
    torch = dev
    S, n = 3, 40
    pa = make(Q, S, CLOCKS)
    x = random_rows(S, 100, seed=10)
    device_calls(dev, pa, x, [[30] * S])
    before = pa.get_state()
    rows = sentinel_rows(torch, S, n)
    big = sentinel_rows(torch, S, 4 * n)
    o = sentinel_rows(torch, S, pa.out_bound(n))
    i16 = sentinel_rows(torch, S, 2 * n, "int16")
    need = max(qpsk_amd.path_count(float(r["r"]), float(r["tau"]), int(r["out_pos"]), int(r["in_pos"]) + n)
               for r in pa.states())
    bad = pa.states()
    bad["out_pos"][1] += 1
    with pytest.raises(ValueError, match="stream 1: out_pos"):
        pa.set_state(bad.tobytes())
    bad = pa.states()
    bad["reserved"][2, 3] = 1
    with pytest.raises(ValueError, match="stream 2: reserved"):
        pa.set_state(bad.tobytes())
    with pytest.raises(ValueError):
        pa.set_state(before[:-1])
    refused = [
        lambda: pa.apply_device(rows, n, o, out_cap=need - 1),                                    # one short
        lambda: pa.apply_device(torch.as_strided(rows, (S, 2 * n - 2), (rows.stride(0) - 1, 1)), n - 1, o),   # odd stride
        lambda: pa.apply_device(torch.as_strided(rows, (S, 2 * n), (2 * n - 2, 1)), n, o),        # stride < 2 n
        lambda: pa.apply_device(i16[:, 1: 2 * n + 1], n, o, fmt="cs16", out_fmt="cf32"),          # 2-byte aligned
        lambda: pa.apply_device(rows, n, i16[:, 1: 2 * (n + 4) + 1], out_fmt="cs16", out_cap=n + 4),
        lambda: pa.apply_device(big[:, : 2 * n], n, big[:, 2 * n - 2:], out_cap=n + 4),           # rows overlap
        lambda: pa.apply_device(big[:, 2 * n:], n, big[:, : 2 * n + 2], out_cap=n + 1),
        lambda: pa.apply_device(rows, n, o, lengths=[1, 2, n + 1]),
        lambda: pa.apply_device(rows, n, o, lengths=[1, -1, 2]),
        lambda: pa.apply_device(rows, n, o, norm="peak"),
        lambda: pa.apply_device(rows, n, o, norm=7),
        lambda: pa.apply_device(rows, n, o, scale_out=0.0),
        lambda: pa.apply_device(i16, n, o, fmt="cs16", out_fmt="cf32", scale_in=float("inf")),
        lambda: pa.apply(np.zeros((S, 2 * n), np.float32), norm="peak"),
    ]
    for k, call in enumerate(refused):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"refusal {k} was accepted")
    torch.cuda.synchronize()
    for t in (rows, big, o, i16):
        assert (t.cpu().numpy().view(np.uint8) == 0xAA).all()
    assert pa.get_state() == before
    n_out = pa.apply_device(rows, n, o, out_cap=need)  # and with the capacity it needs it runs
    assert n_out.max() == need
    pa.close()


def test_a_shard_equals_its_rows_of_the_whole_batch(Q, dev):
    S, k, n = 5, 3, 600
    x = random_rows(S, n, seed=11)
    kw = dict(clock_ppm=50.0, clock_spread=100.0, tau_random=1, multipath=1)
    whole, shard = Q.Path(S, **kw), Q.Path(S - k, first_stream=k, **kw)
    a = device_calls(dev, whole, x, [[250] * S, [350] * S])
    b = device_calls(dev, shard, x[k:], [[250] * (S - k), [350] * (S - k)])
    assert whole.get_state()[256 * k:] == shard.get_state()
    whole.close()
    shard.close()
    for s in range(k, S):
        assert_bits(joined(b, s - k), joined(a, s), f"stream {s}")


# ---------------------------------------------------------------------------
# 6. the chain: modulator -> path -> channel -> demodulator -> framer
# ---------------------------------------------------------------------------
START, STOP = b"MESSAGE_START", b"MESSAGE_STOP"
TAD = dict(fs=K.FS, rs=K.FS // 2, span=10)
FRAMES, S_CHAIN = 3, 8
PATH_KW = dict(clock_spread=100.0, multipath=1, tau_random=1)


def payload(s, k):
    return (f"stream {s} frame {k}: " + K.PAYLOAD * 3)[:48].encode("utf-8")


@functools.lru_cache(maxsize=None)
def oracle_chain():
    """Per stream and frame what the oracle chain returns when the path between
    its modulator and its LO pair is path_reference, cut as the calls cut it."""
    fs, rs, span = TAD["fs"], TAD["rs"], TAD["span"]
    out = []
    for s in range(S_CHAIN):
        r, tau = PC.clock(s, 0.0, PATH_KW["clock_spread"], 3000, 0.0, True)
        frames = [O.modulate_bytes(fs, rs, payload(s, k), START, STOP, rrc_alpha=K.ALPHA, rrc_span=span, tsc=K.TSC)
                  for k in range(FRAMES)]
        y = PC.path_reference(np.concatenate(frames), r, tau, PC.project_taps())
        m = PC.PyPath(r, tau, PC.project_taps())
        tx, rx = O.OracleNCO(100e6, float(fs), 1.0, 0.0, seed=1000 + s), O.OracleNCO(100e6, float(fs), 1.0, 0.0, seed=2000 + s)
        dm = O.OracleDemod(fs, rs, K.ALPHA, span, tsc=K.TSC)
        got, pos = [], 0
        for f in frames:
            cnt = m.call(f)
            got.append(dm.DeModulateBytes(O.apply_lo_pair(tx, rx, y[2 * pos: 2 * (pos + cnt)]), START, STOP))
            pos += cnt
        out.append(got)
    return out


def test_the_chain_on_device_rows_equals_the_oracle_chain(Q, dev):
    """Bits and frames equal the oracle's, lost frames included: the equality
    is what is asserted, not that frames survive a 100 ppm clock."""
    torch = dev
    fs, rs, span, S = TAD["fs"], TAD["rs"], TAD["span"], S_CHAIN
    assert len(payload(0, 0)) == 48
    want = oracle_chain()
    m = Q.QPSKModulator(fs, rs, K.ALPHA, span, tsc=K.TSC)
    n_cap = m.output_floats(8 * (len(START) + 48 + len(STOP))) // 2
    pa = Q.Path(S, **PATH_KW)
    cap = pa.out_bound(n_cap)
    ch = Q.Channel(S, sample_rate=float(fs))
    dm = Q.BatchDemodulator(S, Q.params(fs, rs, K.ALPHA, span, max_samples_per_call=cap))
    fr = Q.DeviceFramer(S, START, STOP)
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    for h in (m, pa, ch, dm, fr):
        h.set_stream(st.cuda_stream)
    ms = dm.max_symbols(cap)
    rows = torch.zeros((S, 2 * n_cap), dtype=torch.float32, device="cuda")
    prop = torch.zeros((S, 2 * cap), dtype=torch.float32, device="cuda")
    n_out = torch.zeros(S, dtype=torch.int64, device="cuda")
    bits = torch.zeros((S, (2 * ms + 7) // 8 + 8), dtype=torch.uint8, device="cuda")
    nbits = torch.zeros(S, dtype=torch.int64, device="cuda")
    offs = torch.zeros(S, dtype=torch.int64, device="cuda")
    pay = torch.zeros((S, 256), dtype=torch.uint8, device="cuda")
    npay = torch.zeros(S, dtype=torch.int64, device="cuda")
    try:
        for k in range(FRAMES):
            host = np.stack([np.frombuffer(payload(s, k), np.uint8) for s in range(S)])
            lens = np.full(S, 48, np.int64)
            m.modulate_bytes_device(torch.from_numpy(host.copy()).cuda(), torch.from_numpy(lens).cuda(), START, STOP, rows,
                                    n_out)
            ns = n_out.cpu().numpy() // 2
            np_out = pa.apply_device(rows, int(ns.max()), prop, lengths=ns)
            ch.apply_device(prop, int(np_out.max()), lengths=np_out)
            dm.process_device_fmt(prop, int(np_out.max()), bits, nbits, "cf32", lengths=np_out)
            Q.tsc_find_device(bits, nbits, K.TSC, offs, st.cuda_stream)
            fr.push(bits, nbits, pay, npay, offs)
            n, pb = npay.cpu().numpy(), pay.cpu().numpy()
            for s in range(S):
                assert bytes(pb[s, : int(n[s])]) == want[s][k], (s, k)
        assert dm.status() == 0
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream())
        for h in (m, pa, ch, dm):
            h.close()
