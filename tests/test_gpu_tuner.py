"""The tuner on the device (qpsk_tuner_*, csrc/qpsk_tuner.hip) against the numpy
yardstick (tuner_cases.tuner_reference), byte for byte against its own host
form (qpsk_tuner_apply_host), and its state against the Python model after
every call.  Every comparison is at tolerance 0; inputs are finite (a NaN's
payload is the one thing an x86 host and gfx950 do not share).

The kernel gives a workgroup QPSK_TUNER_TILE_OUTPUTS = 1024 outputs of a call;
the output counts below straddle that, the call lengths the 32-sample history
and the sizes at which the 16-byte loads begin and end."""
import functools

import numpy as np
import pytest

import common as K
import gpu_harness as H
import oracle as O
import qpsk_amd
import tuner_cases as TC
from gpu_harness import Q, dev  # noqa: F401  (fixtures)
from test_gpu_path import assert_bits, joined, sentinel_rows

pytestmark = pytest.mark.gpu

TILE = qpsk_amd.TUNER_TILE_OUTPUTS
DT = qpsk_amd.TUNER_STATE_DTYPE
# a stream's calls in order, rotated by its index: 4000 samples in all
CUTS = [0, 1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 1023, 1024, 1654]
assert sum(CUTS) == 4000
FULL = {"cf32": 1.0, "cs16": 32767.0, "cs8": 127.0, "cu8": 127.0}
# (r, tau, freq) of the streams of a batch: all differ
STREAMS = [(0.8, 0.25, 0.03), (1.0, 0.0, -0.5), (1.25, 0.75, 0.4999), (3.7, 0.5, 2.0 ** -60), (0.25, 0.1, -0.2),
           (4.0, 0.9, 0.11), (1.0 + 1e-4, 0.3, 0.0), (2.0, 0.0, -0.01)]


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


def taps_of(T, fc=0.4):
    return np.array(TC.design(T, fc))


def make(Q, streams, T=16, cutoff=0.4, **fields):
    """A handle whose stream s has streams[s] = (r, tau, freq), and its models."""
    S = len(streams)
    tu = Q.Tuner(S, taps_per_phase=T, cutoff=cutoff, freq=[f for _, _, f in streams], rate=[r for r, _, _ in streams],
                 **fields)
    st = tu.states()
    for s in range(S):
        st["tau"][s] = streams[s][1]
    tu.set_state(st.tobytes())
    return tu, [TC.PyTuner(r, tau, T, f) for r, tau, f in streams]


def reference(x, model_args, T, h, **kw):
    r, tau, f = model_args
    return TC.tuner_reference(x, r, tau, T, h, TC.freq_word(f), **kw)


def device_calls(torch, tu, x, calls, models=None, fmt="cf32", out_fmt=None, lead_bytes=0, scale_in=None,
                 scale_out=None):
    """The call sequence on device rows of their own (0xAA behind every row's
    count); per call the [S] list of output rows.  models: per stream a PyTuner
    (fed the widened floats); the handle's state is compared after every call."""
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
        cap = tu.out_bound(n)
        o = sentinel_rows(torch, S, cap, FO.torch_dtype, lead_bytes)
        n_out = tu.apply_device(rows, n, o, fmt=fmt, out_fmt=out_fmt, lengths=H.lengths_of(lens), out_cap=cap,
                                scale_in=scale_in, scale_out=scale_out)
        got = o.cpu().numpy()
        assert np.array_equal(rows.cpu().numpy(), host), f"call {ci}: the input rows changed"
        for s in range(S):
            assert (got[s, 2 * n_out[s]:].view(np.uint8) == 0xAA).all(), f"call {ci} stream {s}: written past its count"
        out.append([got[s, : 2 * n_out[s]].copy() for s in range(S)])
        if models:
            st = tu.states()
            for s in range(S):
                w = host[s, : 2 * lens[s]] if fmt == "cf32" else H.widened(host[s, : 2 * lens[s]], fmt, scale_in)
                assert models[s].call(w) == n_out[s], (ci, s)
                assert st[s].tobytes() == models[s].record(DT).tobytes(), f"state after call {ci}, stream {s}"
        pos += np.array(lens)
    return out


def host_form_calls(Q, p, state, x, calls, taps=None):
    """The same calls through qpsk_tuner_apply_host; per call the [S] list of rows, and the state."""
    S = x.shape[0]
    pos, out = np.zeros(S, np.int64), []
    for lens in calls:
        rows = H.call_rows(np.array(x), lens, pos)
        if rows.shape[1] == 0:
            rows = np.zeros((S, 2), np.float32)
        state, o, n_out = Q.tuner_apply_host(p, state, np.ascontiguousarray(rows), lengths=lens, n=max(lens), taps=taps)
        out.append([o[s, : 2 * n_out[s]].copy() for s in range(S)])
        pos += np.array(lens)
    return out, state


# ---------------------------------------------------------------------------
# 1. the kernel against the yardstick and against the host form
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("lead_bytes", [0, 4], ids=["16-byte rows", "4-byte rows"])
def test_kernel_equals_the_yardstick_and_the_host_form_over_a_ragged_cut(Q, dev, lead_bytes):
    streams = STREAMS[:4]
    S, n = len(streams), 4000
    x = random_rows(S, n)
    calls = [[c[s] for s in range(S)] for c in calls_for(S)]
    tu, models = make(Q, streams)
    state = tu.get_state()
    got = device_calls(dev, tu, x, calls, models, lead_bytes=lead_bytes)
    p = tu.p
    tu.close()
    want, state = host_form_calls(Q, p, state, x, calls)
    for ci in range(len(calls)):
        for s in range(S):
            assert got[ci][s].tobytes() == want[ci][s].tobytes(), f"call {ci} stream {s}: device vs host form"
    for s in range(S):
        assert_bits(joined(got, s), reference(x[s], streams[s], 16, taps_of(16)), f"stream {s}")


@pytest.mark.parametrize("lead_bytes", [0, 4], ids=["16-byte rows", "4-byte rows"])
def test_a_ragged_three_call_cut(Q, dev, lead_bytes):
    streams = STREAMS
    S = len(streams)
    x = random_rows(S, 3000, seed=1)
    calls = [[700 + 13 * s for s in range(S)], [29 - s for s in range(S)], [2000 - 7 * s for s in range(S)]]
    tu, models = make(Q, streams)
    got = device_calls(dev, tu, x, calls, models, lead_bytes=lead_bytes)
    tu.close()
    for s in range(S):
        n = sum(c[s] for c in calls)
        assert_bits(joined(got, s), reference(x[s, : 2 * n], streams[s], 16, taps_of(16)), f"stream {s}")


# ---------------------------------------------------------------------------
# 2. tile edges
# ---------------------------------------------------------------------------
def lens_emitting(model, counts):
    """Call lengths after which a stream like model (copied) emits counts[i] in
    call i.  Where a count cannot be had (r < 1: one more input can add several
    outputs) a call of one sample goes first."""
    m = TC.PyTuner(model.r, model.tau, model.T)
    lens, counted = [], []
    for c in counts:
        for _ in range(8):
            guess = int(c * m.r)
            fit = [n for n in range(max(guess - 40, 0), guess + 60)
                   if TC.py_count(m.r, m.tau, m.T, m.out_pos, m.in_pos + n) == c]
            if fit:
                break
            lens.append(1)
            m.call(np.zeros(2, np.float32))
        assert fit, c
        counted.append(len(lens))
        lens.append(fit[0])
        assert m.call(np.zeros(2 * fit[0], np.float32)) == c
    return lens, counted


@pytest.mark.parametrize("r", [4.0, 1.0, 2.0], ids=["the widest window", "rate 1", "rate 2"])
def test_output_counts_around_a_tile(Q, dev, r):
    """Per-call output counts of 1023, 1024, 1025 and 2049; at r = 4 a tile of
    1024 outputs has the widest LDS window."""
    stream = (r, 0.37, 0.123)
    tu, models = make(Q, [stream], T=32, cutoff=0.1)
    counts = [TILE - 1, TILE, TILE + 1, 2 * TILE + 1]
    lens, counted = lens_emitting(models[0], counts)
    x = random_rows(1, sum(lens), seed=2)
    got = device_calls(dev, tu, x, [[n] for n in lens], models)
    tu.close()
    assert [got[ci][0].size // 2 for ci in counted] == counts
    assert_bits(joined(got, 0), reference(x[0], stream, 32, taps_of(32, 0.1)), "tile edges")


def test_output_counts_around_a_tile_at_the_narrowest_window(Q, dev):
    """r = 0.25: four outputs an input, so counts step by four; calls that emit
    1020, 1024, 1028 and 2052 and one-sample calls in between."""
    stream = (0.25, 0.0, -0.3)
    tu, models = make(Q, [stream], T=4)
    lens = [255 + 2, 256, 257, 513, 1, 1]
    x = random_rows(1, sum(lens), seed=3)
    got = device_calls(dev, tu, x, [[n] for n in lens], models)
    tu.close()
    assert [g[0].size // 2 for g in got] == [1020, 1024, 1028, 2052, 4, 4]
    assert_bits(joined(got, 0), reference(x[0], stream, 4, taps_of(4)), "r = 0.25")


@pytest.mark.parametrize("side", [0, 1], ids=["slip on a tile's last output", "slip on a tile's first output"])
@pytest.mark.parametrize("r", [1 - 1e-3, 1 + 1e-3], ids=["an index repeats", "an index is skipped"])
def test_tile_edges_with_an_index_slip_on_either_side(Q, dev, r, side):
    tau, k = TC.slip_clock(r, 16, TILE - 1, side)
    step = int(np.floor(TC.p_of(r, tau, k))) - int(np.floor(TC.p_of(r, tau, k - 1)))
    assert k == TILE - 1 + side and step == (0 if r < 1 else 2)
    stream = (r, tau, 0.25)
    tu, models = make(Q, [stream])
    counts = [2 * TILE + 3, TILE - 1, TILE, TILE + 1]
    lens, counted = lens_emitting(models[0], counts)
    x = random_rows(1, sum(lens), seed=4)
    got = device_calls(dev, tu, x, [[n] for n in lens], models)
    tu.close()
    assert [got[ci][0].size // 2 for ci in counted] == counts
    assert_bits(joined(got, 0), reference(x[0], stream, 16, taps_of(16)), "tile edges")


# ---------------------------------------------------------------------------
# 3. T and phase edges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("T", [4, 8, 12, 16, 32])
def test_every_kernel_form_and_the_phase_edges(Q, dev, T):
    """T = 8 and 16 are unrolled, the others take the general loop.  Stream 0:
    tau = 0 and an integer r, so q = 0 and f = 0 at every output; stream 1: q =
    63 with f just under 1; stream 2: every q."""
    streams = [(2.0, 0.0, 0.05), (1.0, 1.0 - 2.0 ** -30, -0.05), (1.0 + 1.0 / 64 + 1e-5, 0.0, 0.2)]
    S, n = len(streams), 1500
    x = random_rows(S, n, seed=5)
    tu, models = make(Q, streams, T=T, cutoff=0.3)
    got = device_calls(dev, tu, x, [[700, 33, 5], [800, 1467, 1495]], models)
    tu.close()
    for s in range(S):
        assert_bits(joined(got, s), reference(x[s], streams[s], T, taps_of(T, 0.3)), f"T = {T}, stream {s}")


# ---------------------------------------------------------------------------
# 4. the oscillator
# ---------------------------------------------------------------------------
def test_oscillator_edges_and_a_phase_that_wraps_inside_a_tile(Q, dev):
    streams = [(1.0, 0.0, -0.5), (1.0, 0.5, 0.0), (1.25, 0.0, 2.0 ** -60), (0.8, 0.0, 0.4999), (1.0, 0.0, 1.0 / 700)]
    S, n = len(streams), 2300
    x = random_rows(S, n, seed=6)
    tu, models = make(Q, streams)
    # stream 4 starts just below a wrap: the phase passes 2^64 175 samples into the first tile
    st = tu.states()
    st["ph0"][4] = 2 ** 63 + 2 ** 62
    tu.set_state(st.tobytes())
    models[4].ph0 = 2 ** 63 + 2 ** 62
    assert models[4].phase(100) > models[4].phase(400)
    got = device_calls(dev, tu, x, [[n] * S], models)
    tu.close()
    for s in range(S):
        assert_bits(joined(got, s), reference(x[s], streams[s], 16, taps_of(16), ph0=models[s].ph0), f"stream {s}")


def test_positions_near_2_40_through_set_state(Q, dev):
    streams = [(0.25, 0.7, 0.4999), (1.0 + 1e-4, 0.7, -0.5), (3.7, 0.7, 0.03)]
    S, n, base, T = len(streams), 2 * TILE + 50, 2 ** 40 - 1000, 16
    x = random_rows(S, n + 32, seed=8)                 # the first 32 samples are the history
    tu, models = make(Q, streams, cutoff=0.2)
    for s, m in enumerate(models):
        m.at(base, x[s, :64])
        m.ph0 = 0x0123456789ABCDEF * (s + 1)
    k0 = [m.out_pos for m in models]
    tu.set_state(b"".join(m.record(DT).tobytes() for m in models))
    got = device_calls(dev, tu, x[:, 64:], [[n // 2] * S, [n - n // 2] * S], models)
    st = tu.states()
    tu.close()
    assert (st["in_pos"] == base + n).all() and (st["in_pos"] > 2 ** 40).all()
    for s in range(S):
        want = reference(x[s], streams[s], T, taps_of(T, 0.2), ph0=models[s].ph0, k0=k0[s], in0=base - 32)
        assert_bits(joined(got, s), want, f"stream {s} across 2^40")


# ---------------------------------------------------------------------------
# 5. formats
# ---------------------------------------------------------------------------
MIN_LEAD = {"cf32": 4, "cs16": 4, "cs8": 2, "cu8": 2}
FMT_STREAMS = [STREAMS[0], STREAMS[2]]


@functools.lru_cache(maxsize=None)
def fmt_case(fmt):
    """2 streams x 2100 samples of fmt and the yardstick's rows of their widened floats."""
    S, n = 2, 2100
    xi = np.array(random_rows(S, n, seed=9)) if fmt == "cf32" else H.random_rows(S, n, 10, fmt)
    w = xi if fmt == "cf32" else H.widened(xi, fmt)
    return xi, [reference(w[s], FMT_STREAMS[s], 16, taps_of(16)) for s in range(S)]


@pytest.mark.parametrize("fmt_out", ["cf32", "cs16", "cs8", "cu8"])
@pytest.mark.parametrize("fmt_in", ["cf32", "cs16", "cs8", "cu8"])
def test_every_format_pair_on_device_rows_of_both_alignments_and_host_rows(Q, dev, fmt_in, fmt_out):
    xi, want32 = fmt_case(fmt_in)
    S, n = xi.shape[0], xi.shape[1] // 2
    want = [Q.quantise_iq(want32[s], fmt_out, "fixed", FULL[fmt_out])[0] for s in range(S)]
    for lead in (0, max(MIN_LEAD[fmt_in], MIN_LEAD[fmt_out])):
        tu, _ = make(Q, FMT_STREAMS)
        got = device_calls(dev, tu, xi, [[n] * S], fmt=fmt_in, out_fmt=fmt_out, lead_bytes=lead)
        tu.close()
        for s in range(S):
            assert_bits(got[0][s], want[s], f"{fmt_in} -> {fmt_out}, lead {lead}, stream {s}")
    # host rows: what lies past a row's count comes back as it was
    FO = H.FORMATS[fmt_out]
    tu, _ = make(Q, FMT_STREAMS)
    cap = tu.out_bound(n)
    out = np.frombuffer(b"\xaa" * (S * 2 * cap * np.dtype(FO.np_dtype).itemsize), FO.np_dtype).reshape(S, 2 * cap).copy()
    _, n_out = tu.apply_host(np.array(xi), fmt=fmt_in, out_fmt=fmt_out, out=out, lengths=[n, n - 100])
    tu.close()
    w1 = xi[1, : 2 * (n - 100)] if fmt_in == "cf32" else H.widened(xi[1, : 2 * (n - 100)], fmt_in)
    short = Q.quantise_iq(reference(w1, FMT_STREAMS[1], 16, taps_of(16)), fmt_out, "fixed", FULL[fmt_out])[0]
    for s, w in enumerate((want[0], short)):
        assert n_out[s] == w.size // 2
        assert_bits(out[s, : w.size], w, f"host rows {fmt_in} -> {fmt_out}, stream {s}")
        assert (out[s, w.size:].view(np.uint8) == 0xAA).all()


def test_scales_other_than_the_defaults(Q, dev):
    S, n = 2, 500
    xi = H.random_rows(S, n, 7, "cs16")
    scale = H.FORMATS["cs16"].odd_scale
    w = H.widened(xi, "cs16", scale)
    tu, _ = make(Q, FMT_STREAMS)
    o = sentinel_rows(dev, S, tu.out_bound(n), "int8")
    n_out = tu.apply_device(dev.from_numpy(xi).cuda(), n, o, fmt="cs16", out_fmt="cs8", scale_in=scale, scale_out=47.0)
    tu.close()
    for s in range(S):
        want = Q.quantise_iq(reference(w[s], FMT_STREAMS[s], 16, taps_of(16)), "cs8", "fixed", 47.0)[0]
        assert_bits(o.cpu().numpy()[s, : 2 * n_out[s]], want, f"stream {s}")


# ---------------------------------------------------------------------------
# 6. set_freq and set_taps with calls queued
# ---------------------------------------------------------------------------
def test_set_freq_and_set_taps_take_effect_behind_the_queued_calls(Q, dev):
    """Two device calls without lengths on a bound stream are only queued; the
    retune and the new prototype between them land behind the first."""
    torch = dev
    streams = STREAMS[:3]
    S, n1, n2, T = len(streams), 1100, 900, 16
    x = random_rows(S, n1 + n2, seed=12)
    tu, models = make(Q, streams)
    new_taps = (taps_of(T, 0.25) * np.float32(0.5)).astype(np.float32)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        tu.set_stream(st.cuda_stream)
        a_in, b_in = torch.from_numpy(np.array(x[:, : 2 * n1])).cuda(), torch.from_numpy(np.array(x[:, 2 * n1:])).cuda()
        a = torch.zeros((S, 2 * tu.out_bound(n1)), dtype=torch.float32, device="cuda")
        b = torch.zeros((S, 2 * tu.out_bound(n2)), dtype=torch.float32, device="cuda")
        na = tu.apply_device(a_in, n1, a)
        tu.set_freq([2, 0], [-0.31, 0.2])
        for bad in ([0.5], [float("nan")]):
            with pytest.raises(ValueError):
                tu.set_freq([1], bad)
        with pytest.raises(ValueError):
            tu.set_freq([S], [0.0])
        tu.set_taps(new_taps)
        for bad in (new_taps[:-1], np.full(new_taps.size, np.inf, np.float32), []):
            with pytest.raises(ValueError):
                tu.set_taps(bad)
        nb = tu.apply_device(b_in, n2, b)
        a, b = a.cpu().numpy(), b.cpu().numpy()
    for s in range(S):
        assert models[s].call(x[s, : 2 * n1]) == na[s]
    models[2].set_freq(-0.31)
    models[0].set_freq(0.2)
    for s in range(S):
        assert models[s].call(x[s, 2 * n1:]) == nb[s]
    assert tu.get_state() == b"".join(m.record(DT).tobytes() for m in models)
    tu.set_stream(None)
    tu.close()
    st.synchronize()
    for s in range(S):
        r, tau, f = streams[s]
        assert_bits(a[s, : 2 * na[s]], TC.tuner_reference(x[s, : 2 * n1], r, tau, T, taps_of(T), TC.freq_word(f)), f"before, {s}")
        want = TC.tuner_reference(x[s], r, tau, T, new_taps, models[s].fw, models[s].ph0, k0=int(na[s]))
        assert_bits(b[s, : 2 * nb[s]], want, f"after, {s}")
    assert models[1].ph0 == 0 and models[0].ph0 != 0


# ---------------------------------------------------------------------------
# 7. state
# ---------------------------------------------------------------------------
def test_reset_a_subset_and_move_the_state_to_a_second_handle(Q, dev):
    streams = STREAMS[:4]
    S, n = len(streams), 900
    x = random_rows(S, n, seed=13)
    a, models = make(Q, streams)
    first = device_calls(dev, a, x, [[300, 17, 300, 5]], models)
    a.set_freq([1], [0.125])
    models[1].set_freq(0.125)
    blob = a.get_state()
    # the tuning and tau it was made with do not matter; out_bound goes by the rates a handle was made with
    b = Q.Tuner(S, freq=[0.3] * S, rate=[r for r, _, _ in streams], tau0=0.5, cutoff=0.4)
    b.set_state(blob)
    used = np.array([300, 17, 300, 5])
    rest = np.stack([np.roll(x[s], -2 * used[s]) for s in range(S)])
    tail_a = device_calls(dev, a, rest, [[100] * S, [400] * S], models)
    tail_b = device_calls(dev, b, rest, [[63] * S, [437] * S])
    assert a.get_state() == b.get_state()
    for s in range(S):
        assert_bits(joined(tail_b, s), joined(tail_a, s), f"second handle, stream {s}")
        if s != 1:
            whole = reference(x[s, : 2 * (used[s] + 500)], streams[s], 16, taps_of(16))
            assert_bits(np.concatenate([first[0][s], joined(tail_a, s)]), whole, f"stream {s}")
    # reset streams 2 and 0: their created r, the params' tau0, ph0 = 0, positions 0, no history, their fw
    for bad in ([], [0, 0], [S], [-1]):
        with pytest.raises(ValueError):
            a.reset_streams(bad)
    before = a.states()
    a.reset_streams([2, 0])
    st = a.states()
    assert (st["in_pos"] == [0, before["in_pos"][1], 0, before["in_pos"][3]]).all()
    assert (st["out_pos"][[0, 2]] == 0).all() and (st["hist"][[0, 2]] == 0).all() and (st["ph0"][[0, 2]] == 0).all()
    assert (st["r"] == before["r"]).all() and (st["tau"][[0, 2]] == 0.0).all() and (st["fw"] == before["fw"]).all()
    assert st[[1, 3]].tobytes() == before[[1, 3]].tobytes()
    again = device_calls(dev, a, x, [[200] * S])
    a.close()
    b.close()
    for s in (0, 2):
        r, _, f = streams[s]
        assert_bits(again[0][s], TC.tuner_reference(x[s, :400], r, 0.0, 16, taps_of(16), TC.freq_word(f)), f"reset stream {s}")


def test_a_shard_equals_its_rows_of_the_whole_batch(Q, dev):
    S, k, n = 5, 3, 600
    x = random_rows(S, n, seed=14)
    fr, rt = [f for _, _, f in STREAMS[:S]], [r for r, _, _ in STREAMS[:S]]
    whole = Q.Tuner(S, freq=fr, rate=rt, tau0=0.3)
    shard = Q.Tuner(S - k, freq=fr[k:], rate=rt[k:], tau0=0.3, first_stream=k)
    a = device_calls(dev, whole, x, [[250] * S, [350] * S])
    b = device_calls(dev, shard, x[k:], [[250] * (S - k), [350] * (S - k)])
    assert whole.get_state()[320 * k:] == shard.get_state()
    whole.close()
    shard.close()
    for s in range(k, S):
        assert_bits(joined(b, s - k), joined(a, s), f"stream {s}")


def test_what_a_live_handle_refuses_changes_nothing(Q, dev):
    torch = dev
    streams = STREAMS[:3]
    S, n = 3, 40
    tu, _ = make(Q, streams)
    x = random_rows(S, 100, seed=10)
    device_calls(dev, tu, x, [[50] * S])
    before = tu.get_state()
    rows = sentinel_rows(torch, S, n)
    big = sentinel_rows(torch, S, 8 * n)
    o = sentinel_rows(torch, S, tu.out_bound(n))
    i16 = sentinel_rows(torch, S, 4 * n, "int16")
    need = max(qpsk_amd.tuner_count(float(r["r"]), float(r["tau"]), 16, int(r["out_pos"]), int(r["in_pos"]) + n)
               for r in tu.states())
    bad = tu.states()
    bad["out_pos"][1] += 1
    with pytest.raises(ValueError, match="stream 1: out_pos"):
        tu.set_state(bad.tobytes())
    bad = tu.states()
    bad["reserved"][2, 3] = 1
    with pytest.raises(ValueError, match="stream 2: reserved"):
        tu.set_state(bad.tobytes())
    bad = tu.states()
    bad["r"][0] = 4.5
    with pytest.raises(ValueError, match="stream 0: r"):
        tu.set_state(bad.tobytes())
    with pytest.raises(ValueError):
        tu.set_state(before[:-1])
    refused = [
        lambda: tu.apply_device(rows, n, o, out_cap=need - 1),                                    # one short
        lambda: tu.apply_device(torch.as_strided(rows, (S, 2 * n - 2), (rows.stride(0) - 1, 1)), n - 1, o),   # odd stride
        lambda: tu.apply_device(torch.as_strided(rows, (S, 2 * n), (2 * n - 2, 1)), n, o),        # stride < 2 n
        lambda: tu.apply_device(i16[:, 1: 2 * n + 1], n, o, fmt="cs16", out_fmt="cf32"),          # 2-byte aligned
        lambda: tu.apply_device(rows, n, i16[:, 1: 2 * need + 1], out_fmt="cs16", out_cap=need),
        lambda: tu.apply_device(big[:, : 2 * n], n, big[:, 2 * n - 2:], out_cap=need),            # rows overlap
        lambda: tu.apply_device(big[:, 2 * need:], n, big[:, : 2 * need + 2], out_cap=need + 1),
        lambda: tu.apply_device(rows, n, o, lengths=[1, 2, n + 1]),
        lambda: tu.apply_device(rows, n, o, lengths=[1, -1, 2]),
        lambda: tu.apply_device(rows, n, o, norm="peak"),
        lambda: tu.apply_device(rows, n, o, norm=7),
        lambda: tu.apply_device(rows, n, o, scale_out=0.0),
        lambda: tu.apply_device(i16, n, o, fmt="cs16", out_fmt="cf32", scale_in=float("inf")),
        lambda: tu.apply_host(np.zeros((S, 2 * n), np.float32), norm="peak"),
    ]
    for k, call in enumerate(refused):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"refusal {k} was accepted")
    torch.cuda.synchronize()
    for t in (rows, big, o, i16):
        assert (t.cpu().numpy().view(np.uint8) == 0xAA).all()
    assert tu.get_state() == before
    n_out = tu.apply_device(rows, n, o, out_cap=need)  # and with the capacity it needs it runs
    assert n_out.max() == need
    tu.close()


def test_host_rows_whose_staging_grows_and_is_reused(Q, dev):
    """Host-memory calls of 40, 1100 and 40 samples on one handle: the staging
    buffers are made, freed for larger ones, and then serve a shorter call."""
    streams = [STREAMS[0], STREAMS[2]]
    S, lens = 2, [40, 1100, 40]
    x = random_rows(S, sum(lens), seed=11)
    tu, _ = make(Q, streams)
    want, state = host_form_calls(Q, tu.p, tu.get_state(), x, [[n] * S for n in lens])
    assert max(w.size // 2 for w in want[1]) > TILE
    got, pos = [], 0
    for n in lens:
        out, n_out = tu.apply_host(np.ascontiguousarray(x[:, 2 * pos: 2 * (pos + n)]))
        got.append([out[s, : 2 * n_out[s]].copy() for s in range(S)])
        pos += n
    assert tu.get_state() == state
    tu.close()
    for ci in range(len(lens)):
        for s in range(S):
            assert_bits(got[ci][s], want[ci][s], f"call {ci} stream {s}: device vs host form")


def test_set_stream_back_to_none_after_a_bound_call(Q, dev):
    torch = dev
    streams = [STREAMS[0], STREAMS[2]]
    S, lens = 2, [40, 1100]
    x = random_rows(S, sum(lens), seed=12)
    tu, _ = make(Q, streams)
    want, state = host_form_calls(Q, tu.p, tu.get_state(), x, [[n] * S for n in lens])
    cuts = [np.ascontiguousarray(x[:, : 2 * lens[0]]), np.ascontiguousarray(x[:, 2 * lens[0]:])]
    got = []
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        tu.set_stream(st.cuda_stream)
        o = torch.zeros((S, 2 * tu.out_bound(lens[0])), dtype=torch.float32, device="cuda")
        n_out = tu.apply_device(torch.from_numpy(cuts[0]).cuda(), lens[0], o)
        first = o.cpu().numpy()
    got.append([first[s, : 2 * n_out[s]] for s in range(S)])
    tu.set_stream(None)
    o = torch.zeros((S, 2 * tu.out_bound(lens[1])), dtype=torch.float32, device="cuda")
    n_out = tu.apply_device(torch.from_numpy(cuts[1]).cuda(), lens[1], o)
    second = o.cpu().numpy()
    got.append([second[s, : 2 * n_out[s]] for s in range(S)])
    assert tu.get_state() == state
    tu.close()
    st.synchronize()
    for ci in range(2):
        for s in range(S):
            assert_bits(got[ci][s], want[ci][s], f"call {ci} stream {s}: device vs host form")


# ---------------------------------------------------------------------------
# 8. the chain: modulator -> two tuners (an off-grid carrier) -> tuner -> demodulator -> framer
# ---------------------------------------------------------------------------
START, STOP = b"MESSAGE_START", b"MESSAGE_STOP"
FS, RS, SPAN = K.FS, K.FS // 4, 10
ROUNDS, GAP = 8, 256
# (samples a symbol, carrier offset in cycles per sample) of each stream's carrier
PAIRS = [(5, 0.03), (3.2, -0.05), (4.7, 0.011), (6.3, 0.02), (4, 0.04), (2.9, 0.06), (8, -0.01), (4.0003, 0.0301)]
S_CHAIN = len(PAIRS)
U1 = dict(rate=[4.0 / s for s, _ in PAIRS])
U2 = dict(freq=[-f0 for _, f0 in PAIRS])
RX = dict(freq=[f0 for _, f0 in PAIRS], rate=[s / 4.0 for s, _ in PAIRS], tau0=0.3, taps_per_phase=16)


def payload(s, k):
    return (f"stream {s} frame {k}: " + K.PAYLOAD * 3)[:48].encode("utf-8")


def round_rows(frames):
    """A round's input rows: the rest of the gap before, the frames, the first half of the gap behind."""
    n = frames[0].size // 2
    rows = np.zeros((len(frames), 2 * (n + GAP)), np.float32)
    for s, f in enumerate(frames):
        rows[s, GAP: GAP + 2 * n] = f
    return rows


@functools.lru_cache(maxsize=None)
def cpu_chain():
    """Per stream and round what the CPU chain returns: the oracle's modulator,
    qpsk_tuner_apply_host three times, the oracle's demodulator, cut as the
    device calls are."""
    Qh = qpsk_amd
    S = S_CHAIN
    ps = [Qh.tuner_params(), Qh.tuner_params(), Qh.tuner_params(tau0=RX["tau0"], taps_per_phase=RX["taps_per_phase"])]
    states = [Qh.tuner_state_init(ps[0], S, rate=U1["rate"]), Qh.tuner_state_init(ps[1], S, freq=U2["freq"]),
              Qh.tuner_state_init(ps[2], S, freq=RX["freq"], rate=RX["rate"])]
    dms = [O.OracleDemod(FS, RS, K.ALPHA, SPAN, tsc=K.TSC) for _ in range(S)]
    got = [[] for _ in range(S)]
    for k in range(ROUNDS):
        rows = round_rows([O.modulate_bytes(FS, RS, payload(s, k), START, STOP, rrc_alpha=K.ALPHA, rrc_span=SPAN, tsc=K.TSC)
                           for s in range(S)])
        lens = None
        for i in range(3):
            states[i], rows, lens = Qh.tuner_apply_host(ps[i], states[i], np.ascontiguousarray(rows), lengths=lens,
                                                        n=rows.shape[1] // 2 if lens is None else int(max(lens)))
        for s in range(S):
            got[s].append(dms[s].DeModulateBytes(rows[s, : 2 * int(lens[s])], START, STOP))
    return got


def test_the_chain_on_device_rows_equals_the_cpu_chain(Q, dev):
    """Frames equal the CPU chain's frame for frame, lost ones included; and the
    CPU chain itself returns every payload from round 2 on (round 1 may be lost
    while the loops acquire)."""
    torch = dev
    S = S_CHAIN
    want = cpu_chain()
    for s in range(S):
        for k in range(1, ROUNDS):
            assert want[s][k] == payload(s, k), f"CPU chain, stream {s} (sps {PAIRS[s][0]}, offset {PAIRS[s][1]}) round {k + 1}"
    m = Q.QPSKModulator(FS, RS, K.ALPHA, SPAN, tsc=K.TSC)
    n_mod = m.output_floats(8 * (len(START) + 48 + len(STOP))) // 2
    n0 = n_mod + GAP
    u1, u2, rx = Q.Tuner(S, **U1), Q.Tuner(S, **U2), Q.Tuner(S, **RX)
    c1 = u1.out_bound(n0)
    c2 = u2.out_bound(c1)
    c3 = rx.out_bound(c2)
    dm = Q.BatchDemodulator(S, Q.params(FS, RS, K.ALPHA, SPAN, max_samples_per_call=c3))
    fr = Q.DeviceFramer(S, START, STOP)
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    handles = (m, u1, u2, rx, dm, fr)
    for h in handles:
        h.set_stream(st.cuda_stream)
    ms = dm.max_symbols(c3)
    mod = torch.zeros((S, 2 * n_mod), dtype=torch.float32, device="cuda")
    rows = torch.zeros((S, 2 * n0), dtype=torch.float32, device="cuda")
    b1 = torch.zeros((S, 2 * c1), dtype=torch.float32, device="cuda")
    b2 = torch.zeros((S, 2 * c2), dtype=torch.float32, device="cuda")
    b3 = torch.zeros((S, 2 * c3), dtype=torch.float32, device="cuda")
    n_out = torch.zeros(S, dtype=torch.int64, device="cuda")
    bits = torch.zeros((S, (2 * ms + 7) // 8 + 8), dtype=torch.uint8, device="cuda")
    nbits = torch.zeros(S, dtype=torch.int64, device="cuda")
    offs = torch.zeros(S, dtype=torch.int64, device="cuda")
    pay = torch.zeros((S, 256), dtype=torch.uint8, device="cuda")
    npay = torch.zeros(S, dtype=torch.int64, device="cuda")
    try:
        for k in range(ROUNDS):
            host = np.stack([np.frombuffer(payload(s, k), np.uint8) for s in range(S)])
            lens = np.full(S, 48, np.int64)
            m.modulate_bytes_device(torch.from_numpy(host.copy()).cuda(), torch.from_numpy(lens).cuda(), START, STOP, mod,
                                    n_out)
            ns = n_out.cpu().numpy() // 2
            assert (ns == n_mod).all()
            rows.zero_()
            rows[:, GAP: GAP + 2 * n_mod] = mod
            k1 = u1.apply_device(rows, n0, b1)
            k2 = u2.apply_device(b1, int(k1.max()), b2, lengths=k1)
            k3 = rx.apply_device(b2, int(k2.max()), b3, lengths=k2)
            dm.process_device_fmt(b3, int(k3.max()), bits, nbits, "cf32", lengths=rx.lengths_for_demod(k3))
            Q.tsc_find_device(bits, nbits, K.TSC, offs, st.cuda_stream)
            fr.push(bits, nbits, pay, npay, offs)
            n, pb = npay.cpu().numpy(), pay.cpu().numpy()
            for s in range(S):
                assert bytes(pb[s, : int(n[s])]) == want[s][k], (s, k)
        assert dm.status() == 0
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream())
        for h in handles[:-1]:
            h.close()
