"""The test bench's channel on the device (qpsk_channel_*, csrc/qpsk_channel.hip)
against the CPU oracle's NCO pair (oracle.OracleNCO, oracle.apply_lo_pair).
Unless a test says otherwise the tolerance is 0 and bit patterns are compared.

The kernel holds QPSK_CHANNEL_TILE_STREAMS = 16 streams a workgroup and scans
the phases in blocks of QPSK_CHANNEL_BLOCK_SAMPLES = 64 samples; the batch
sizes and the cuts below straddle both.
"""
import functools

import numpy as np
import pytest

import channel_cases as CC
import common as K
import gpu_harness as H
import oracle as O
import qpsk_amd
from gpu_harness import Q, dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

LO = 100e6
TX0, RX0 = 1000, 2000                 # tests/common.py's seeds
BLOCK = qpsk_amd.CHANNEL_BLOCK_SAMPLES
# a stream's calls in order, rotated by its index: cuts at 1, 7, 8 and 9 (the
# drift interval at fs = 8000 is 8) and one below, at and above one and two
# blocks of the phase scan; 600 samples in all
CUTS = [1, 7, 8, 9, BLOCK - 1, BLOCK, BLOCK + 1, 0, 2 * BLOCK + 2, 3 * BLOCK + 1, 60]
assert sum(CUTS) == 600
FLT_MAX = float(np.finfo(np.float32).max)


def calls_for(S):
    return [[CUTS[(c + s) % len(CUTS)] for s in range(S)] for c in range(len(CUTS))]


@functools.lru_cache(maxsize=None)
def random_rows(S, n, seed=0):
    """[S, 2 n] float32 with +-0, denormals and values near FLT_MAX / 4 up front."""
    x = np.random.default_rng(seed).standard_normal((S, 2 * n)).astype(np.float32)
    head = np.array([0.0, -0.0, 1e-45, -1e-40, FLT_MAX / 4, -0.99 * FLT_MAX / 4, 1.0, -1.0], np.float32)
    k = min(head.size, 2 * n)
    x[:, :k] = head[:k]
    x[1::2, :k] = head[:k][::-1]
    x.setflags(write=False)
    return x


def oracle_pair(fs, g, lo=LO, tx_ppm=1.0, rx_ppm=1.0, tx_seed=TX0, rx_seed=RX0, ph=(0.0, 0.0)):
    return (O.OracleNCO(lo, fs, tx_ppm, ph[0], seed=tx_seed + g), O.OracleNCO(lo, fs, rx_ppm, ph[1], seed=rx_seed + g))


def oracle_calls(x, calls, fs, first=0, **kw):
    """Per call the [S] list of output rows of the oracle's LO pairs over the same cuts."""
    S = x.shape[0]
    pairs = [oracle_pair(fs, first + s, **kw) for s in range(S)]
    pos = np.zeros(S, np.int64)
    out = []
    for lens in calls:
        out.append([O.apply_lo_pair(*pairs[s], x[s, 2 * pos[s]: 2 * (pos[s] + lens[s])]) for s in range(S)])
        pos += np.array(lens)
    return out


def sentinel_rows(torch, S, n_cap, dtype="float32", lead_bytes=0):
    """Device rows [S, 2 n_cap] of dtype whose every byte is 0xAA; row 0 starts
    lead_bytes into a 16-byte aligned allocation and the pitch is a multiple of
    16 bytes (the bytes between the rows are sentinels too)."""
    dt = getattr(torch, dtype)
    size = torch.empty(0, dtype=dt).element_size()
    pitch = (2 * n_cap * size + lead_bytes + 15) // 16 * 16
    buf = torch.full((S * pitch,), 0xAA, dtype=torch.uint8, device="cuda")
    flat = buf[lead_bytes: lead_bytes + (S * pitch - lead_bytes) // size * size].view(dt)
    return torch.as_strided(flat, (S, 2 * n_cap), (pitch // size, 1))


def device_calls(torch, ch, x, calls, sync_states=None):
    """The call sequence in place on device rows; per call the [S] list of output rows.
    Bytes past a row's length must stay 0xAA."""
    S = x.shape[0]
    pos = np.zeros(S, np.int64)
    out = []
    for ci, lens in enumerate(calls):
        n = max(max(lens), 1)
        rows = sentinel_rows(torch, S, n)
        host = H.call_rows(x, lens, pos)
        keep = rows.cpu().numpy().copy()
        for s in range(S):
            keep[s, : 2 * lens[s]] = host[s, : 2 * lens[s]]
        rows.copy_(torch.from_numpy(keep))
        ch.apply_device(rows, max(lens), lengths=H.lengths_of(lens))
        got = rows.cpu().numpy()
        for s in range(S):
            assert (got[s, 2 * lens[s]:].view(np.uint8) == 0xAA).all(), f"call {ci} stream {s}: written past its length"
        out.append([got[s, : 2 * lens[s]].copy() for s in range(S)])
        pos += np.array(lens)
        if sync_states:
            sync_states(ci, lens)
    return out


def assert_calls_equal(got, want, what=""):
    assert len(got) == len(want)
    for ci, (ra, rb) in enumerate(zip(got, want)):
        for s, (a, b) in enumerate(zip(ra, rb)):
            if not K.bitwise_equal(a, b):
                bad = np.flatnonzero(a.view(np.uint32) != b.view(np.uint32))
                pytest.fail(f"{what} call {ci} stream {s} ({a.size // 2} samples): {bad.size} floats differ, first at "
                            f"sample {bad[0] // 2}: {a[bad[0]]!r} vs {b[bad[0]]!r}")


# ---------------------------------------------------------------------------
# 1. the LO pair against the oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 3, 64, 65, 130])
def test_lo_pair_equals_the_oracle_over_ragged_calls(Q, dev, S):
    fs = 8000.0
    x, calls = random_rows(S, 600), calls_for(S)
    ch = Q.Channel(S, sample_rate=fs)
    got = device_calls(dev, ch, x, calls)
    ch.close()
    assert_calls_equal(got, oracle_calls(x, calls, fs), f"S = {S}")


def test_lo_pair_at_the_references_rate_across_drift_updates(Q, dev):
    fs, S, n = 10e6, 17, 20001           # interval 10000: two drift updates inside the call
    x = random_rows(S, n, seed=1)
    ch = Q.Channel(S, sample_rate=fs)
    got = device_calls(dev, ch, x, [[n] * S])
    st = ch.states()
    ch.close()
    assert_calls_equal(got, oracle_calls(x, [[n] * S], fs), "fs = 10 MHz")
    assert (st["tx"]["counter"] == 1).all() and (st["tx"]["drift_ppm"] != 0).all() and (st["pos"] == n).all()


# ---------------------------------------------------------------------------
# 2. wrap and clamp
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_seeds():
    return CC.seed_near(+1), CC.seed_near(-1)


@pytest.mark.parametrize("edge", [0, 1], ids=["static near +max", "static near -max"])
def test_drift_every_sample_reaches_the_clamp(Q, dev, edge):
    fs, n = 1000.0, 4096                  # interval 1
    seed = edge_seeds()[edge]
    py = CC.PyNCO(LO, fs, 1.0, 0.0, seed=seed)
    assert abs(py.static_ppm - (1.0, -1.0)[edge]) <= 0.0005
    for _ in range(n):
        py.next()
    assert (py.clamped_hi, py.clamped_lo)[edge] >= 1, "the clamp never engaged: the test would pass vacuously"
    x = random_rows(1, n, seed=2)
    ch = Q.Channel(1, sample_rate=fs, tx_seed=seed)
    got = device_calls(dev, ch, x, [[n]])
    st = ch.states()
    ch.close()
    assert_calls_equal(got, oracle_calls(x, [[n]], fs, tx_seed=seed), "clamp")
    assert tuple(st["tx"][0]) == py.fields()


@pytest.mark.parametrize("kw", [dict(lo=-LO), dict(tx_ppm=0.0, rx_ppm=5.0), dict(lo=-LO, ph=(-7.5, 100.0)),
                                dict(lo=12345.678, tx_ppm=20.0, rx_ppm=10.0, ph=(120.0, 30.0))],
                         ids=["negative LO", "ideal tx LO", "negative LO and phase0", "small LO"])
def test_negative_phase_branch_and_ideal_lo(Q, dev, kw):
    fs, S, n = 1000.0, 3, 700
    x = random_rows(S, n, seed=3)
    ph = kw.get("ph", (0.0, 0.0))
    ch = Q.Channel(S, sample_rate=fs, lo_hz=kw.get("lo", LO), tx_ppm=kw.get("tx_ppm", 1.0), rx_ppm=kw.get("rx_ppm", 1.0),
                   tx_phase0=ph[0], rx_phase0=ph[1])
    calls = [[300] * S, [1, 0, 400], [399, 400, 0]]
    got = device_calls(dev, ch, x, calls)
    st = ch.states()
    ch.close()
    assert_calls_equal(got, oracle_calls(x, calls, fs, **kw), str(kw))
    if kw.get("tx_ppm") == 0.0:
        assert (st["tx"]["rng"] == TX0 + np.arange(S)).all(), "an ideal LO draws nothing"


# ---------------------------------------------------------------------------
# 3. per-stream lengths, in place, layouts
# ---------------------------------------------------------------------------
def test_lengths_with_0_and_1_host_rows_and_in_place(Q, dev):
    fs, S, n = 8000.0, 5, 150
    lens = [0, 1, 150, 64, 65]
    x = random_rows(S, n, seed=4)
    want = oracle_calls(x, [lens], fs)[0]
    # host rows, out of place: what lies past a row's length comes back as it was
    ch = Q.Channel(S, sample_rate=fs)
    out = np.full((S, 2 * n), np.frombuffer(b"\xaa" * 4, np.float32)[0], np.float32)
    ch.apply(np.array(x), out=out, lengths=lens)
    for s in range(S):
        assert K.bitwise_equal(out[s, : 2 * lens[s]], want[s]), s
        assert (out[s, 2 * lens[s]:].view(np.uint8) == 0xAA).all(), s
    ch.close()
    # host rows, in place
    ch = Q.Channel(S, sample_rate=fs)
    rows = np.array(x)
    assert ch.apply(rows, out=rows, lengths=lens) is rows
    for s in range(S):
        assert K.bitwise_equal(rows[s, : 2 * lens[s]], want[s]), s
        assert K.bitwise_equal(rows[s, 2 * lens[s]:], x[s, 2 * lens[s]:]), s
    ch.close()
    # device rows, out of place, input untouched
    torch = dev
    ch = Q.Channel(S, sample_rate=fs)
    xin = torch.from_numpy(np.array(x)).cuda()
    o = sentinel_rows(torch, S, n)
    ch.apply_device(xin, n, out_dev=o, lengths=lens)
    got = o.cpu().numpy()
    for s in range(S):
        assert K.bitwise_equal(got[s, : 2 * lens[s]], want[s]), s
        assert (got[s, 2 * lens[s]:].view(np.uint8) == 0xAA).all(), s
    assert K.bitwise_equal(xin.cpu().numpy(), x)
    ch.close()


@pytest.mark.parametrize("lead_bytes", [0, 8, 4], ids=["16-byte rows", "8-byte rows", "4-byte rows (scalar)"])
def test_cf32_device_rows_of_every_alignment(Q, dev, lead_bytes):
    torch = dev
    fs, S, n = 8000.0, 18, 131
    x = random_rows(S, n, seed=5)
    rows = sentinel_rows(torch, S, n + 1, lead_bytes=lead_bytes)
    assert rows.data_ptr() % 16 == lead_bytes
    rows[:, : 2 * n].copy_(torch.from_numpy(np.array(x)))
    ch = Q.Channel(S, sample_rate=fs)
    ch.apply_device(rows, n)
    ch.close()
    got = rows.cpu().numpy()
    want = oracle_calls(x, [[n] * S], fs)[0]
    for s in range(S):
        assert K.bitwise_equal(got[s, : 2 * n], want[s]), s
    assert (got[:, 2 * n:].view(np.uint8) == 0xAA).all()


def test_a_row_that_starts_past_2_31_elements(Q, dev):
    """Row 1 of a CS8 batch pitched 2^31 + 16 elements: its offset needs 64-bit
    arithmetic in elements and in bytes alike (4.3 GB allocated, 2 x 130 samples touched)."""
    torch = dev
    S, n, stride = 2, 130, 2 ** 31 + 16
    xi = H.random_rows(S, n, 12, "cs8")
    buf = torch.empty(S * stride, dtype=torch.int8, device="cuda")
    rows = torch.as_strided(buf, (S, 2 * n + 16), (stride, 1))
    rows.fill_(-86)                                   # 0xAA
    rows[:, : 2 * n].copy_(torch.from_numpy(np.array(xi)))
    ch = Q.Channel(S, sample_rate=8000.0)
    ch.apply_device(rows, n, fmt="cs8")
    ch.close()
    got = rows.cpu().numpy()
    del rows, buf
    want = oracle_calls(H.widened(xi, "cs8"), [[n] * S], 8000.0)[0]
    for s in range(S):
        assert np.array_equal(got[s, : 2 * n], qpsk_amd.quantise_iq(want[s], "cs8", "fixed", 127.0)[0]), s
    assert (got[:, 2 * n:] == -86).all()


def test_rows_the_library_refuses_change_nothing(Q, dev):
    torch = dev
    S, n = 3, 40
    ch = Q.Channel(S, sample_rate=8000.0)
    before = ch.get_state()
    rows = sentinel_rows(torch, S, n)
    i16 = sentinel_rows(torch, S, n + 1, "int16")
    refused = [
        lambda: ch.apply_device(torch.as_strided(rows, (S, 2 * n - 2), (rows.stride(0) - 1, 1)), n - 1),   # odd stride
        lambda: ch.apply_device(torch.as_strided(rows, (S, 2 * n), (2 * n - 2, 1)), n),                    # stride < 2 n
        lambda: ch.apply_device(i16[:, 1: 2 * n + 1], n, fmt="cs16"),                                      # 2-byte aligned
        lambda: ch.apply_device(rows, n, out_dev=i16[:, 1: 2 * n + 1], out_fmt="cs16"),
        lambda: ch.apply_device(rows, n, lengths=[1, 2, n + 1]),
        lambda: ch.apply_device(rows, n, lengths=[1, -1, 2]),
        lambda: ch.apply_device(rows, n, norm="peak"),
        lambda: ch.apply_device(i16, n, fmt="cs16", norm="peak"),
        lambda: ch.apply_device(rows, n, norm=7),
        lambda: ch.apply_device(rows, n, scale_out=0.0),
        lambda: ch.apply_device(rows, n, scale_out=float("nan")),
        lambda: ch.apply_device(i16, n, fmt="cs16", scale_in=float("inf")),
        lambda: ch.apply(np.zeros((S, 2 * n), np.float32), norm="peak"),
    ]
    for k, call in enumerate(refused):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"refusal {k} was accepted")
    torch.cuda.synchronize()
    assert (rows.cpu().numpy().view(np.uint8) == 0xAA).all() and (i16.cpu().numpy().view(np.uint8) == 0xAA).all()
    assert ch.get_state() == before
    ch.close()


# ---------------------------------------------------------------------------
# 4. formats
# ---------------------------------------------------------------------------
FULL = {"cf32": 1.0, "cs16": 32767.0, "cs8": 127.0, "cu8": 127.0}


@functools.lru_cache(maxsize=None)
def cf32_result(fmt, odd):
    """The integer rows, their widened floats and the oracle's result for them (S = 18, n = 200)."""
    F = H.FORMATS[fmt]
    S, n = 18, 200
    xi = H.random_rows(S, n, 6, fmt)
    scale = F.odd_scale if odd else F.scale
    w = H.widened(xi, fmt, scale)
    want = oracle_calls(w, [[n] * S], 8000.0)[0]
    return xi, scale, w, np.stack(want)


@pytest.mark.parametrize("odd", [False, True], ids=["default scale", "odd scale"])
@pytest.mark.parametrize("layout", ["vector", "scalar"])
@pytest.mark.parametrize("fmt", ["cs16", "cs8", "cu8"])
def test_integer_input_equals_the_widened_floats(Q, dev, fmt, layout, odd):
    torch = dev
    xi, scale, w, want = cf32_result(fmt, odd)
    S, n = xi.shape[0], xi.shape[1] // 2
    rows = H.device_rows(S, n, layout, fmt)
    rows.copy_(torch.from_numpy(np.array(xi)))
    out = torch.zeros((S, 2 * n), dtype=torch.float32, device="cuda")
    ch = Q.Channel(S, sample_rate=8000.0)
    ch.apply_device(rows, n, out_dev=out, fmt=fmt, out_fmt="cf32", scale_in=scale)
    ch.close()
    assert K.bitwise_equal(out.cpu().numpy(), want)
    # and through host rows
    ch = Q.Channel(S, sample_rate=8000.0)
    assert K.bitwise_equal(ch.apply(np.array(xi), fmt=fmt, out_fmt="cf32", scale_in=scale), want)
    ch.close()


@pytest.mark.parametrize("layout", ["vector", "scalar"])
@pytest.mark.parametrize("fmt", ["cs16", "cs8", "cu8"])
def test_integer_output_is_the_quantiser_of_the_cf32_output(Q, dev, fmt, layout):
    torch = dev
    S, n = 18, 200
    x = np.array(random_rows(S, n, seed=7))
    x[:, 4:6] = [[2.5, -2.5]]                      # past full scale: the clamp
    want32 = np.stack(oracle_calls(x, [[n] * S], 8000.0)[0])
    for scale in (FULL[fmt], FULL[fmt] * 0.37):
        want = np.stack([Q.quantise_iq(want32[s], fmt, "fixed", scale)[0] for s in range(S)])
        out = H.device_rows(S, n, layout, fmt)
        ch = Q.Channel(S, sample_rate=8000.0)
        ch.apply_device(torch.from_numpy(x).cuda(), n, out_dev=out, fmt="cf32", out_fmt=fmt, scale_out=scale)
        ch.close()
        assert np.array_equal(out.cpu().numpy(), want), (fmt, scale)
    # integer to integer in place, and CF32 out at a scale
    xi = H.random_rows(S, n, 8, fmt)
    w = np.stack(oracle_calls(H.widened(xi, fmt), [[n] * S], 8000.0)[0])
    rows = H.device_rows(S, n, layout, fmt)
    rows.copy_(torch.from_numpy(np.array(xi)))
    ch = Q.Channel(S, sample_rate=8000.0)
    ch.apply_device(rows, n, fmt=fmt)
    ch.close()
    assert np.array_equal(rows.cpu().numpy(), np.stack([Q.quantise_iq(w[s], fmt, "fixed", FULL[fmt])[0] for s in range(S)]))
    ch = Q.Channel(S, sample_rate=8000.0)
    got = ch.apply(x, scale_out=0.3)
    ch.close()
    assert K.bitwise_equal(got, np.stack([Q.quantise_iq(want32[s], "cf32", "fixed", 0.3)[0] for s in range(S)]))


# ---------------------------------------------------------------------------
# 5. state
# ---------------------------------------------------------------------------
def py_states(fs, S, first=0, **kw):
    return [(CC.PyNCO(kw.get("lo", LO), fs, kw.get("tx_ppm", 1.0), 0.0, seed=TX0 + first + s),
             CC.PyNCO(kw.get("lo", LO), fs, kw.get("rx_ppm", 1.0), 0.0, seed=RX0 + first + s)) for s in range(S)]


def test_state_after_every_call_and_restore_into_a_fresh_handle(Q, dev):
    fs, S = 8000.0, 3
    x, calls = random_rows(S, 600), calls_for(S)
    py = py_states(fs, S)
    pos = np.zeros(S, np.int64)
    ch = Q.Channel(S, sample_rate=fs)
    blobs = []

    def after(ci, lens):
        blob = ch.get_state()
        st = ch.states(blob)
        for s in range(S):
            for _ in range(lens[s]):
                py[s][0].next()
                py[s][1].next()
            pos[s] += lens[s]
            assert tuple(st["tx"][s]) == py[s][0].fields(), (ci, s)
            assert tuple(st["rx"][s]) == py[s][1].fields(), (ci, s)
            assert st["pos"][s] == pos[s] and st["reserved"][s] == 0
        Q.channel_state_check(ch.p, S, blob)
        blobs.append(blob)

    got = device_calls(dev, ch, x, calls, sync_states=after)
    ch.close()
    for k in (0, 4, len(calls) - 2):
        fresh = Q.Channel(S, sample_rate=fs)
        fresh.set_state(blobs[k])
        used = np.sum(np.array(calls[: k + 1]), axis=0)
        rest = np.stack([np.roll(x[s], -2 * used[s]) for s in range(S)])
        cont = device_calls(dev, fresh, rest, calls[k + 1:])
        assert fresh.get_state() == blobs[-1]
        fresh.close()
        assert_calls_equal(cont, got[k + 1:], f"restored after call {k}")


def assert_state_after(ch, fs, S, n):
    """The handle's state is the Python model's after n samples a stream."""
    st = ch.states()
    for s, (tx, rx) in enumerate(py_states(fs, S)):
        for _ in range(n):
            tx.next()
            rx.next()
        assert tuple(st["tx"][s]) == tx.fields() and tuple(st["rx"][s]) == rx.fields(), s
        assert st["pos"][s] == n


def test_host_rows_whose_staging_grows_and_is_reused(Q, dev):
    """Host-memory calls of 70, 300 and 70 samples on one handle: the staging
    buffers are made, freed for larger ones, and then serve a shorter call.
    300 samples pass a 64-sample block edge."""
    fs, S, lens = 8000.0, 3, [70, 300, 70]
    x = random_rows(S, sum(lens), seed=13)
    calls = [[n] * S for n in lens]
    ch = Q.Channel(S, sample_rate=fs)
    got, pos = [], 0
    for n in lens:
        out = ch.apply(np.ascontiguousarray(x[:, 2 * pos: 2 * (pos + n)]))
        got.append([out[s] for s in range(S)])
        pos += n
    assert_state_after(ch, fs, S, sum(lens))
    ch.close()
    assert_calls_equal(got, oracle_calls(x, calls, fs), "host rows")


def test_set_stream_back_to_none_after_a_bound_call(Q, dev):
    """A device call on a bound torch stream, then set_stream(None) and a second
    one on the handle's own stream again, then close(): the caller's stream
    outlives the handle."""
    torch = dev
    fs, S, lens = 8000.0, 3, [70, 300]
    x = random_rows(S, sum(lens), seed=14)
    ch = Q.Channel(S, sample_rate=fs)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ch.set_stream(st.cuda_stream)
        a = torch.from_numpy(np.ascontiguousarray(x[:, : 2 * lens[0]])).cuda()
        ch.apply_device(a, lens[0])
        first = a.cpu().numpy()
    ch.set_stream(None)
    b = torch.from_numpy(np.ascontiguousarray(x[:, 2 * lens[0]:])).cuda()
    ch.apply_device(b, lens[1])
    second = b.cpu().numpy()
    assert_state_after(ch, fs, S, sum(lens))
    ch.close()
    st.synchronize()
    got = [[first[s] for s in range(S)], [second[s] for s in range(S)]]
    assert_calls_equal(got, oracle_calls(x, [[n] * S for n in lens], fs), "bound, then unbound")


def test_reset_streams_and_refusals_on_a_live_handle(Q, dev):
    fs, S = 8000.0, 4
    x = random_rows(S, 300, seed=9)
    ch = Q.Channel(S, sample_rate=fs)
    first = device_calls(dev, ch, x, [[100] * S])
    before = ch.get_state()
    bad = ch.states(before)
    bad["rx"]["phase"][2] = 7.0
    with pytest.raises(ValueError, match="stream 2: rx.phase"):
        ch.set_state(bad.tobytes())
    with pytest.raises(ValueError):
        ch.set_state(before[:-1])
    for streams in ([], [0, 0], [S], [-1], list(range(S + 1))):
        with pytest.raises(ValueError):
            ch.reset_streams(streams)
    assert ch.get_state() == before
    ch.reset_streams([2, 0])
    st = ch.states()
    assert (st["pos"] == [0, 100, 0, 100]).all()
    rest = np.stack([x[s, 200:] for s in range(S)])
    got = device_calls(dev, ch, rest, [[37] * S, [163] * S])
    ch.close()
    whole = oracle_calls(x, [[100] * S, [37] * S, [163] * S], fs)
    anew = oracle_calls(rest, [[37] * S, [163] * S], fs)
    assert_calls_equal(first, whole[:1])
    for ci in range(2):
        for s in range(S):
            want = anew[ci][s] if s in (0, 2) else whole[ci + 1][s]
            assert K.bitwise_equal(got[ci][s], want), (ci, s)


def test_a_shard_equals_its_rows_of_the_whole_batch(Q, dev):
    fs, S, k, n = 8000.0, 21, 15, 200
    x = random_rows(S, n, seed=10)
    kw = dict(sample_rate=fs, noise_rms=0.05, noise_seed=77)
    whole, shard = Q.Channel(S, **kw), Q.Channel(S - k, first_stream=k, **kw)
    calls = [[70] * S, [130] * S]
    a = device_calls(dev, whole, x, calls)
    b = device_calls(dev, shard, x[k:], [c[k:] for c in calls])
    assert whole.get_state()[128 * k:] == shard.get_state()
    whole.close()
    shard.close()
    assert_calls_equal([r[k:] for r in a], b, "shard")


# ---------------------------------------------------------------------------
# 6. noise
# ---------------------------------------------------------------------------
def ordered(v):
    """float32 bit patterns as integers that order like the values (+-0 -> 0)."""
    i = v.view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def test_noise_floats_against_the_float64_restatement(Q, dev):
    """Both ppm 0, lo_hz 0, phases 0: the LO product is exactly 1 + 0j, and an
    all-zero input leaves the noise floats.  The restatement (numpy float64)
    and the kernel round doubles that agree to a few ulps (log, cos and sin of
    either side are accurate to about an ulp of double), so a float differs
    only where such a double lies within ~2^-50 relative of a float rounding
    boundary, about 2^-50 / 2^-24 = 1.5e-8 of the samples, and then by one float:
    every sample equal or adjacent, at most 0.1 % different at all."""
    torch = dev
    S, n, rms, seed = 64, 4096, 0.1, 0xC0FFEE
    rows = torch.zeros((S, 2 * n), dtype=torch.float32, device="cuda")
    ch = Q.Channel(S, sample_rate=10e6, lo_hz=0.0, tx_ppm=0.0, rx_ppm=0.0, noise_rms=rms, noise_seed=seed,
                   first_stream=5)
    ch.apply_device(rows, n)
    got = rows.cpu().numpy()
    want = np.stack([CC.noise_reference(seed, 5 + s, 0, n, rms) for s in range(S)])
    d = np.abs(ordered(got) - ordered(want))
    frac = np.count_nonzero(d) / d.size
    print(f"noise: max distance {d.max()} floats, {np.count_nonzero(d)} of {d.size} differ ({frac:.3g})")
    assert d.max() <= 1
    assert frac <= 1e-3
    assert abs(float(np.sqrt(np.mean(got.astype(np.float64) ** 2))) - rms) < 0.01 * rms
    # the second call draws from pos = n on
    rows.zero_()
    ch.apply_device(rows, 100)
    ch.close()
    want2 = np.stack([CC.noise_reference(seed, 5 + s, n, 100, rms) for s in range(S)])
    assert np.abs(ordered(rows.cpu().numpy()[:, :200]) - ordered(want2)).max() <= 1


def test_noise_clamp_at_rms_4(Q, dev):
    torch = dev
    S, n = 4, 4096
    rows = torch.zeros((S, 2 * n), dtype=torch.float32, device="cuda")
    ch = Q.Channel(S, sample_rate=10e6, lo_hz=0.0, tx_ppm=0.0, rx_ppm=0.0, noise_rms=4.0, noise_seed=3)
    ch.apply_device(rows, n)
    ch.close()
    got = rows.cpu().numpy()
    want = np.stack([CC.noise_reference(3, s, 0, n, 4.0) for s in range(S)])
    assert np.abs(got).max() == 1.0 and (got == 1.0).sum() > 1000 and (got == -1.0).sum() > 1000
    assert np.abs(ordered(got) - ordered(want)).max() <= 1
    assert ((np.abs(want) == 1.0) == (np.abs(got) == 1.0)).mean() > 0.999


def test_noise_does_not_depend_on_the_cut_and_rms_0_is_the_plain_channel(Q, dev):
    fs, S = 8000.0, 5
    x, calls = random_rows(S, 600, seed=11), calls_for(S)
    x = np.clip(x, -4.0, 4.0)
    kw = dict(sample_rate=fs, noise_rms=0.25, noise_seed=123456789)
    a, b = Q.Channel(S, **kw), Q.Channel(S, **kw)
    cut = device_calls(dev, a, x, calls)
    one = device_calls(dev, b, x, [[600] * S])
    assert a.get_state() == b.get_state()
    a.close()
    b.close()
    for s in range(S):
        assert K.bitwise_equal(np.concatenate([c[s] for c in cut]), one[0][s]), s
    quiet = Q.Channel(S, sample_rate=fs, noise_rms=0.0, noise_seed=123456789)
    plain = device_calls(dev, quiet, x, [[600] * S])
    quiet.close()
    assert_calls_equal(plain, oracle_calls(x, [[600] * S], fs), "noise_rms = 0")
    assert not K.bitwise_equal(plain[0][0], one[0][0])


# ---------------------------------------------------------------------------
# 7. the reference's test on the device
# ---------------------------------------------------------------------------
START, STOP = b"MESSAGE_START", b"MESSAGE_STOP"
TAD = dict(fs=K.FS, rs=K.FS // 2, span=10)         # testAtDataLevel.cs:17-28
FRAMES = 6


def payload(s, k):
    return (f"stream {s} frame {k}: " + K.PAYLOAD[: 20 + 3 * s]).encode("utf-8")


@functools.lru_cache(maxsize=None)
def oracle_chain(fmt):
    """Per stream and frame what the oracle chain returns: modulate_bytes,
    (the format's quantiser,) apply_lo_pair, (the quantiser,) DeModulateBytes."""
    fs, rs, span = TAD["fs"], TAD["rs"], TAD["span"]

    def through(v):
        return v if fmt == "cf32" else H.widened(qpsk_amd.quantise_iq(v, fmt, "fixed", FULL[fmt])[0], fmt)

    out = []
    for s in range(8):
        tx, rx = oracle_pair(float(fs), s)
        dm = O.OracleDemod(fs, rs, K.ALPHA, span, tsc=K.TSC)
        out.append([dm.DeModulateBytes(through(O.apply_lo_pair(tx, rx, through(
            O.modulate_bytes(fs, rs, payload(s, k), START, STOP, rrc_alpha=K.ALPHA, rrc_span=span, tsc=K.TSC)))),
            START, STOP) for k in range(FRAMES)])
    return out


@pytest.mark.parametrize("fmt", ["cf32", "cs16"])
def test_the_references_test_on_the_device(Q, dev, fmt):
    """testAtDataLevel.cs:24-46 at batch size: ModulateBytes, the LO pair,
    DeModulateBytes, frame after frame with all state carried, every stage on
    device rows of fmt.  The frames returned, recovered and lost alike, are
    the oracle chain's."""
    torch = dev
    fs, rs, span, S = TAD["fs"], TAD["rs"], TAD["span"], 8
    want = oracle_chain(fmt)
    recovered = sum(want[s][k] == payload(s, k) for s in range(S) for k in range(FRAMES))
    assert recovered >= 30, "the reference's own chain recovers most frames"
    F = H.FORMATS[fmt]
    m = Q.QPSKModulator(fs, rs, K.ALPHA, span, tsc=K.TSC)
    n_cap = m.output_floats(8 * (len(START) + len(payload(S - 1, 0)) + len(STOP))) // 2
    pitch = -(-n_cap // F.per_load) * F.per_load
    ch = Q.Channel(S, sample_rate=float(fs))
    dm = Q.BatchDemodulator(S, Q.params(fs, rs, K.ALPHA, span, max_samples_per_call=pitch))
    fr = Q.DeviceFramer(S, START, STOP)
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    for h in (m, ch, dm, fr):
        h.set_stream(st.cuda_stream)
    ms = dm.max_symbols(pitch)
    rows = torch.zeros((S, 2 * pitch), dtype=getattr(torch, F.torch_dtype), device="cuda")
    n_out = torch.zeros(S, dtype=torch.int64, device="cuda")
    bits = torch.zeros((S, (2 * ms + 7) // 8 + 8), dtype=torch.uint8, device="cuda")
    nbits = torch.zeros(S, dtype=torch.int64, device="cuda")
    offs = torch.zeros(S, dtype=torch.int64, device="cuda")
    pay = torch.zeros((S, 256), dtype=torch.uint8, device="cuda")
    npay = torch.zeros(S, dtype=torch.int64, device="cuda")
    try:
        for k in range(FRAMES):
            texts = [payload(s, k) for s in range(S)]
            host = np.zeros((S, max(map(len, texts))), np.uint8)
            for s, t in enumerate(texts):
                host[s, : len(t)] = np.frombuffer(t, np.uint8)
            lens = np.array([len(t) for t in texts], np.int64)
            m.modulate_bytes_device(torch.from_numpy(host).cuda(), torch.from_numpy(lens).cuda(), START, STOP, rows, n_out,
                                    fmt=fmt, scale=FULL[fmt])
            ns = n_out.cpu().numpy() // 2              # the rows' lengths, not their samples
            ch.apply_device(rows, int(ns.max()), fmt=fmt, lengths=ns)
            dm.process_device_fmt(rows, int(ns.max()), bits, nbits, fmt, lengths=ns)
            Q.tsc_find_device(bits, nbits, K.TSC, offs, st.cuda_stream)
            fr.push(bits, nbits, pay, npay, offs)
            n, pb = npay.cpu().numpy(), pay.cpu().numpy()
            for s in range(S):
                assert bytes(pb[s, : int(n[s])]) == want[s][k], (fmt, s, k)
        assert dm.status() == 0
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream())
        for h in (m, ch, dm):
            h.close()
