"""The polyphase channeliser on the device (qpsk_pfb_*, csrc/qpsk_pfb.hip) against
the numpy yardstick (pfb_cases.pfb_reference), byte for byte against its own
host form (qpsk_pfb_apply_host), and its state against the Python model after
every call.  Every comparison is at tolerance 0; inputs are finite (a NaN's
payload is the one thing an x86 host and gfx950 do not share).

The kernel gives a workgroup qpsk_pfb_tile_frames(M) = 4096 / M frames of a
call; the calls below emit one frame fewer, exactly that and one more, start at
an odd frame, and are shorter than the history."""
import functools

import numpy as np
import pytest

import common as K
import gpu_harness as H
import oracle as O
import pfb_cases as PC
import qpsk_amd
from gpu_harness import Q, dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
f32 = np.float32


def sentinel_rows(torch, R, n_cap, dtype="float32", lead_bytes=0):
    """Device rows [R, 2 n_cap] of dtype inside a buffer whose every byte is
    0xAA; row 0 starts lead_bytes into a 16-byte aligned allocation and the
    pitch is a multiple of 16 bytes (16 more than the rows need when
    lead_bytes != 0), so lead_bytes = 0 gives rows the 16-byte loads take and
    any other value rows they cannot.  Returns (rows, the buffer, the pitch in bytes)."""
    dt = getattr(torch, dtype)
    size = torch.empty(0, dtype=dt).element_size()
    pitch = (2 * n_cap * size + 15) // 16 * 16 + (16 if lead_bytes else 0)
    buf = torch.full((R * pitch + 32,), 0xAA, dtype=torch.uint8, device="cuda")
    flat = buf[lead_bytes: lead_bytes + (R * pitch) // size * size].view(dt)
    rows = torch.as_strided(flat, (R, 2 * n_cap), (pitch // size, 1))
    assert rows.data_ptr() % 16 == lead_bytes % 16
    return rows, buf, pitch


def assert_only_counts_written(buf, pitch, lead_bytes, counts, what):
    """Every byte of an output buffer outside row r's first counts[r] samples is still 0xAA."""
    full = buf.cpu().numpy()
    keep = np.ones(full.size, bool)
    for r, c in enumerate(counts):
        keep[lead_bytes + r * pitch: lead_bytes + r * pitch + 8 * int(c)] = False
    assert (full[keep] == 0xAA).all(), f"{what}: written past a row's count or between rows"


def device_calls(torch, pf, x, calls, models=None, fmt="cf32", lead_bytes=0, scale_in=None):
    """The call sequence on device rows of their own; per call the [B] list of
    [M, 2 n_out] blocks.  models: per band a PyPfb (fed the widened floats);
    the handle's state is compared after every call."""
    B, M = x.shape[0], pf.channels
    F = H.FORMATS[fmt]
    dt = qpsk_amd.pfb_state_dtype(M, pf.p.taps_per_branch)
    pos = np.zeros(B, np.int64)
    out = []
    for ci, lens in enumerate(calls):
        n = max(lens)
        rows, _, _ = sentinel_rows(torch, B, max(n, 1), F.torch_dtype, lead_bytes)
        host = rows.cpu().numpy().copy()
        for b in range(B):
            host[b, : 2 * lens[b]] = x[b, 2 * pos[b]: 2 * (pos[b] + lens[b])]
        rows.copy_(torch.from_numpy(host))
        cap = pf.out_bound(n)
        out_lead = lead_bytes if lead_bytes % 4 == 0 else 4     # float rows are 4-byte aligned at the least
        o, obuf, opitch = sentinel_rows(torch, B * M, cap, "float32", out_lead)
        n_out = pf.apply_device(rows, n, o, fmt=fmt, lengths=H.lengths_of(lens), out_cap=cap, scale_in=scale_in)
        got = o.cpu().numpy()
        assert np.array_equal(rows.cpu().numpy(), host), f"call {ci}: the input rows changed"
        assert_only_counts_written(obuf, opitch, out_lead, np.repeat(n_out, M), f"call {ci}")
        out.append([got[b * M: (b + 1) * M, : 2 * n_out[b]].copy() for b in range(B)])
        if models:
            st = pf.states()
            for b in range(B):
                w = host[b, : 2 * lens[b]] if fmt == "cf32" else H.widened(host[b, : 2 * lens[b]], fmt, scale_in)
                assert models[b].call(w) == n_out[b], (ci, b)
                assert st[b].tobytes() == models[b].record(dt).tobytes(), f"state after call {ci}, band {b}"
        pos += np.array(lens)
    return out


def host_calls(Q, p, x, calls, taps=None):
    """The same sequence through qpsk_pfb_apply_host."""
    B, M = x.shape[0], p.channels
    state = Q.pfb_state_init(p, B)
    pos = np.zeros(B, np.int64)
    out = []
    for lens in calls:
        rows = np.ascontiguousarray(H.call_rows(np.array(x), lens, pos))
        if rows.shape[1] == 0:
            rows = np.zeros((B, 2), f32)
        state, o, n_out = Q.pfb_apply_host(p, state, rows, lengths=lens, n=max(lens), taps=taps)
        out.append([o[b * M: (b + 1) * M, : 2 * n_out[b]].copy() for b in range(B)])
        pos += np.array(lens)
    return out, state


def joined(outs, b):
    return np.concatenate([c[b] for c in outs], axis=1)


def assert_bits(got, want, what):
    assert got.shape == want.shape, f"{what}: {got.shape} vs {want.shape}"
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        c, k = bad[0]
        pytest.fail(f"{what}: {len(bad)} floats differ, first at channel {c} frame {k // 2}: {got[c, k]!r} vs {want[c, k]!r}")


def tile_calls(M, K, B):
    """Per call the [B] lengths.  Band 0: one sample (frame 0 alone, so the next
    call starts at an odd frame), then calls that emit tile - 1, 0 (no sample),
    tile and tile + 1 frames, a call shorter than the history that ends one
    sample short of a frame, one sample that completes nothing new, and a tail.
    Band b takes the same calls b places on."""
    D, F = M // 2, PC.tile_frames(M)
    base = [1, (F - 1) * D, 0, F * D, (F + 1) * D, min(D - 2, M * K - 1), 1, 2 * D + 3]
    return [[base[(i + b) % len(base)] for b in range(B)] for i in range(len(base))]


# ---------------------------------------------------------------------------
# 1. the kernel against the yardstick and against the host form
# ---------------------------------------------------------------------------
SHAPES = [(M, 2, 3 if i % 2 == 0 else 1) for i, M in enumerate(PC.CHANNELS)] + \
         [(16, k, 1 if i % 2 == 0 else 3) for i, k in enumerate(PC.BRANCH_TAPS) if k != 2]


@pytest.mark.parametrize("M,K_,B", SHAPES, ids=[f"M{m}-K{k}-B{b}" for m, k, b in SHAPES])
def test_kernel_equals_the_yardstick_and_the_host_form_at_the_tile_edges(Q, dev, M, K_, B):
    calls = tile_calls(M, K_, B)
    n = max(sum(c[b] for c in calls) for b in range(B))
    x = PC.random_rows(B, n, seed=3 * M + K_)
    models = [PC.PyPfb(M, K_) for _ in range(B)]
    pf = Q.Channeliser(B, channels=M, taps_per_branch=K_)
    got = device_calls(dev, pf, x, calls, models, lead_bytes=0 if M != 64 else 8)
    state = pf.get_state()
    pf.close()
    F = PC.tile_frames(M)
    assert [c[0].shape[1] // 2 for c in got[:5]] == [1, F - 1, 0, F, F + 1]
    host, host_state = host_calls(Q, pf.p, x, calls)
    assert state == host_state
    h, W = Q.pfb_design(pf.p), Q.pfb_twiddles(M)
    for b in range(B):
        for ci in range(len(calls)):
            assert got[ci][b].tobytes() == host[ci][b].tobytes(), f"call {ci} band {b}: device vs host form"
        nb = sum(c[b] for c in calls)
        assert_bits(joined(got, b), PC.pfb_reference(x[b, : 2 * nb], M, K_, h, W), f"band {b}")


def test_the_largest_transform_with_the_longest_prototype(Q, dev):
    M, K_, frames = 4096, 8, 5
    x = PC.random_rows(1, frames * M // 2, seed=41)
    pf = Q.Channeliser(1, channels=M, taps_per_branch=K_)
    models = [PC.PyPfb(M, K_)]
    got = device_calls(dev, pf, x, [[frames * M // 2]], models)
    pf.close()
    assert got[0][0].shape == (M, 2 * frames)
    host, _ = host_calls(Q, pf.p, x, [[frames * M // 2]])
    assert got[0][0].tobytes() == host[0][0].tobytes()
    assert_bits(got[0][0], PC.pfb_reference(x[0], M, K_, Q.pfb_design(pf.p), Q.pfb_twiddles(M)), "M = 4096, K = 8")


# ---------------------------------------------------------------------------
# 2. formats, scales, the gain
# ---------------------------------------------------------------------------
MIN_LEAD = {"cf32": 4, "cs16": 4, "cs8": 2, "cu8": 2}
GAIN = f32(np.sqrt(8.0))


@functools.lru_cache(maxsize=None)
def fmt_case(fmt):
    """2 bands x 700 samples of fmt at a scale of its own, their widened floats and the yardstick's rows."""
    B, n, M, K_ = 2, 700, 32, 3
    xi = np.array(PC.random_rows(B, n, seed=5)) if fmt == "cf32" else H.random_rows(B, n, 6, fmt)
    scale = None if fmt == "cf32" else H.FORMATS[fmt].odd_scale
    w = xi if fmt == "cf32" else H.widened(xi, fmt, scale)
    p = qpsk_amd.pfb_params(channels=M, taps_per_branch=K_, gain=GAIN)
    h, W = qpsk_amd.pfb_design(p), qpsk_amd.pfb_twiddles(M)
    want = [PC.pfb_reference(w[b], M, K_, h, W, gain=GAIN) for b in range(B)]
    short = PC.pfb_reference(w[1, : 2 * (n - 100)], M, K_, h, W, gain=GAIN)
    return xi, scale, p, want, short


@pytest.mark.parametrize("fmt", ["cf32", "cs16", "cs8", "cu8"])
def test_every_input_format_on_device_rows_of_both_alignments_and_host_rows(Q, dev, fmt):
    xi, scale, p, want, short = fmt_case(fmt)
    B, n, M = xi.shape[0], xi.shape[1] // 2, p.channels
    for lead in (0, MIN_LEAD[fmt]):
        pf = Q.Channeliser(B, p)
        got = device_calls(dev, pf, xi, [[n] * B], fmt=fmt, lead_bytes=lead, scale_in=scale)
        pf.close()
        for b in range(B):
            assert_bits(got[0][b], want[b], f"{fmt}, lead {lead}, band {b}")
    # host rows: what lies past a row's count comes back as it was
    pf = Q.Channeliser(B, p)
    cap = pf.out_bound(n)
    out = np.frombuffer(b"\xaa" * (B * M * 2 * cap * 4), f32).reshape(B * M, 2 * cap).copy()
    _, n_out = pf.apply(np.array(xi), fmt=fmt, out=out, lengths=[n, n - 100], scale_in=scale)
    pf.close()
    for b, w in enumerate((want[0], short)):
        assert n_out[b] == w.shape[1] // 2
        blk = out[b * M: (b + 1) * M]
        assert_bits(blk[:, : w.shape[1]], w, f"host rows {fmt}, band {b}")
        assert (blk[:, w.shape[1]:].view(np.uint8) == 0xAA).all()


def test_set_taps_takes_effect_behind_the_calls_so_far(Q, dev):
    M, K_, n = 16, 3, 400
    x = PC.random_rows(1, n, seed=7)
    taps = (np.random.default_rng(8).standard_normal(M * K_) * 0.2).astype(f32)
    pf = Q.Channeliser(1, channels=M, taps_per_branch=K_)
    a = device_calls(dev, pf, x, [[200]])
    pf.set_taps(taps)
    for bad in (taps[:-1], np.append(taps, 1.0), np.where(np.arange(M * K_) == 5, np.nan, taps), []):
        with pytest.raises(ValueError):
            pf.set_taps(bad)
    b = device_calls(dev, pf, x[:, 400:], [[200]])
    pf.close()
    W = Q.pfb_twiddles(M)
    na = a[0][0].shape[1]
    assert_bits(a[0][0], PC.pfb_reference(x[0], M, K_, Q.pfb_design(pf.p), W)[:, :na], "before")
    assert_bits(b[0][0], PC.pfb_reference(x[0], M, K_, taps, W)[:, na:], "after")


# ---------------------------------------------------------------------------
# 3. state
# ---------------------------------------------------------------------------
def test_reset_a_subset_and_move_the_state_to_a_second_handle(Q, dev):
    B, M, K_, n = 3, 16, 8, 900
    x = PC.random_rows(B, n, seed=9)
    a = Q.Channeliser(B, channels=M, taps_per_branch=K_)
    used = np.array([300, 17, 5])
    first = device_calls(dev, a, x, [list(used)])
    blob = a.get_state()
    b = Q.Channeliser(B, channels=M, taps_per_branch=K_)
    b.set_state(blob)
    rest = np.stack([np.roll(x[s], -2 * used[s]) for s in range(B)])
    tail_a = device_calls(dev, a, rest, [[100] * B, [400] * B])
    tail_b = device_calls(dev, b, rest, [[63] * B, [437] * B])
    assert a.get_state() == b.get_state()
    h, W = Q.pfb_design(a.p), Q.pfb_twiddles(M)
    for s in range(B):
        whole = PC.pfb_reference(x[s, : 2 * (used[s] + 500)], M, K_, h, W)
        assert_bits(np.concatenate([first[0][s], joined(tail_a, s)], axis=1), whole, f"band {s}")
        assert_bits(joined(tail_b, s), joined(tail_a, s), f"second handle, band {s}")
    for bands in ([], [0, 0], [B], [-1]):
        with pytest.raises(ValueError):
            a.reset_bands(bands)
    before = a.states()
    a.reset_bands([2, 0])
    st = a.states()
    assert (st["in_pos"] == [0, before["in_pos"][1], 0]).all() and (st["out_pos"][[0, 2]] == 0).all()
    assert (st["hist"][[0, 2]].view(np.uint32) == 0).all() and st[1].tobytes() == before[1].tobytes()
    again = device_calls(dev, a, x, [[200] * B])
    a.close()
    b.close()
    for s in (0, 2):
        assert_bits(again[0][s], PC.pfb_reference(x[s, :400], M, K_, h, W), f"reset band {s}")


def test_host_rows_whose_staging_grows_and_is_reused(Q, dev):
    """Host-memory calls of 40, 2100 and 40 samples on one handle: the staging
    buffers are made, freed for larger ones, and then serve a shorter call.
    At M = 8 a tile is 512 frames of 4 samples: 2100 samples pass one tile edge."""
    B, M, K_, lens = 2, 8, 2, [40, 2100, 40]
    assert PC.tile_frames(M) * (M // 2) < lens[1]
    x = PC.random_rows(B, sum(lens), seed=51)
    pf = Q.Channeliser(B, channels=M, taps_per_branch=K_)
    want, state = host_calls(Q, pf.p, x, [[n] * B for n in lens])
    pos = 0
    for ci, n in enumerate(lens):
        out, n_out = pf.apply(np.ascontiguousarray(x[:, 2 * pos: 2 * (pos + n)]))
        for b in range(B):
            assert_bits(out[b * M: (b + 1) * M, : 2 * n_out[b]], want[ci][b], f"call {ci} band {b}: device vs host form")
        pos += n
    assert pf.get_state() == state
    pf.close()


def test_set_stream_back_to_none_after_a_bound_call(Q, dev):
    """A device call on a bound torch stream, then set_stream(None) and a second
    one on the handle's own stream again, then close(): the caller's stream
    outlives the handle."""
    torch = dev
    B, M, K_, lens = 2, 8, 2, [40, 2100]
    x = PC.random_rows(B, sum(lens), seed=52)
    pf = Q.Channeliser(B, channels=M, taps_per_branch=K_)
    want, state = host_calls(Q, pf.p, x, [[n] * B for n in lens])
    cuts = [np.ascontiguousarray(x[:, : 2 * lens[0]]), np.ascontiguousarray(x[:, 2 * lens[0]:])]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        pf.set_stream(st.cuda_stream)
        o = torch.zeros((B * M, 2 * pf.out_bound(lens[0])), dtype=torch.float32, device="cuda")
        n_first = pf.apply_device(torch.from_numpy(cuts[0]).cuda(), lens[0], o)
        first = o.cpu().numpy()
    pf.set_stream(None)
    o = torch.zeros((B * M, 2 * pf.out_bound(lens[1])), dtype=torch.float32, device="cuda")
    n_second = pf.apply_device(torch.from_numpy(cuts[1]).cuda(), lens[1], o)
    second = o.cpu().numpy()
    assert pf.get_state() == state
    pf.close()
    st.synchronize()
    for ci, (rows, n_out) in enumerate(((first, n_first), (second, n_second))):
        for b in range(B):
            assert_bits(rows[b * M: (b + 1) * M, : 2 * n_out[b]], want[ci][b], f"call {ci} band {b}: device vs host form")


def test_what_a_live_handle_refuses_changes_nothing(Q, dev):
    torch = dev
    B, M, K_, n = 2, 16, 2, 40
    pf = Q.Channeliser(B, channels=M, taps_per_branch=K_)
    x = PC.random_rows(B, 100, seed=10)
    device_calls(dev, pf, x, [[30] * B])
    before = pf.get_state()
    need = qpsk_amd.pfb_count(M, 4, 30 + n)
    rows, rbuf, _ = sentinel_rows(torch, B, n)
    o, obuf, _ = sentinel_rows(torch, B * M, need)
    big, bbuf, _ = sentinel_rows(torch, B * M, 4 * n)
    i16, ibuf, _ = sentinel_rows(torch, B, 2 * n, "int16")
    bad = pf.states()
    bad["out_pos"][1] += 1
    with pytest.raises(ValueError, match="band 1: out_pos"):
        pf.set_state(bad.tobytes())
    bad = pf.states()
    bad["reserved"][0, 3] = 1
    with pytest.raises(ValueError, match="band 0: reserved"):
        pf.set_state(bad.tobytes())
    with pytest.raises(ValueError):
        pf.set_state(before[:-1])
    L_ = Q.lib()

    def raw(fmt_tag):
        n_out = np.zeros(B, np.int64)
        return L_.qpsk_pfb_apply_fmt(pf._h, fmt_tag, rows.data_ptr(), rows.stride(0), 1.0, o.data_ptr(), o.stride(0), need, n,
                                     None, n_out.ctypes.data_as(qpsk_amd._i64p), qpsk_amd.MEM_DEVICE)

    assert raw(4) == Q.QPSK_ERR_ARGUMENT and raw(-1) == Q.QPSK_ERR_ARGUMENT                     # a bad format
    refused = [
        lambda: pf.apply_device(rows, n, o, out_cap=need - 1),                                    # one short
        lambda: pf.apply_device(torch.as_strided(rows, (B, 2 * n - 2), (rows.stride(0) - 1, 1)), n - 1, o),   # odd stride
        lambda: pf.apply_device(torch.as_strided(rows, (B, 2 * n), (2 * n - 2, 1)), n, o),        # stride < 2 n
        lambda: pf.apply_device(i16[:, 1: 2 * n + 1], n, o, fmt="cs16"),                          # 2-byte aligned
        lambda: pf.apply_device(big[:B, : 2 * n], n, big[:, 2 * n - 2:], out_cap=need),           # rows overlap
        lambda: pf.apply_device(big[B * M - B:, 2 * n:], n, big[:, : 2 * n + 2], out_cap=need),
        lambda: pf.apply_device(rows, n, o, lengths=[1, n + 1]),
        lambda: pf.apply_device(rows, n, o, lengths=[-1, 2]),
        lambda: pf.apply_device(i16, n, o, fmt="cs16", scale_in=float("inf")),
        lambda: pf.apply_device(i16, n, o, fmt="cs16", scale_in=0.0),
    ]
    for k, call in enumerate(refused):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"refusal {k} was accepted")
    torch.cuda.synchronize()
    for t in (rbuf, obuf, bbuf, ibuf):
        assert (t.cpu().numpy() == 0xAA).all()
    assert pf.get_state() == before
    n_out = pf.apply_device(rows, n, o, out_cap=need)  # and with the capacity it needs it runs
    assert (n_out == need).all()
    pf.close()


# ---------------------------------------------------------------------------
# 4. the chain: a wideband row of 16 carriers -> channeliser -> demodulator -> framer
# ---------------------------------------------------------------------------
START, STOP = b"MESSAGE_START", b"MESSAGE_STOP"
E2E = dict(M=16, K=8, rounds=3, span=8)


def payload(c, k):
    return (f"carrier {c} round {k}: " + K.PAYLOAD * 3)[:48].encode("utf-8")


@functools.lru_cache(maxsize=None)
def wideband_case(fmt):
    """Per round the wideband row (of fmt) that carries one 48-byte frame on each
    of the 16 carriers, the scale it is read with, and per channel and round
    what the oracle chain returns: OracleDemod.DeModulateBytes on the
    yardstick's rows, cut as the calls cut them."""
    M, K_, rounds, span = E2E["M"], E2E["K"], E2E["rounds"], E2E["span"]
    D, fs = M // 2, K.FS
    rs = fs // (2 * M)
    wide, pos = [], 0
    for k in range(rounds):
        sigs = [O.modulate_bytes(fs, rs, payload(c, k), START, STOP, rrc_alpha=K.ALPHA, rrc_span=span, tsc=K.TSC)
                for c in range(M)]
        n = max(s.size // 2 for s in sigs) + 64 * D
        n = (n + D - 1) // D * D
        idx = pos + np.arange(n, dtype=np.int64)
        acc = np.zeros(n, np.complex128)
        for c, s in enumerate(sigs):
            z = np.zeros(n, np.complex128)
            z[: s.size // 2] = s[0::2].astype(np.float64) + 1j * s[1::2].astype(np.float64)
            acc += z * np.exp(2j * np.pi * ((c * idx) % M) / M)
        row = np.zeros(2 * n, f32)
        row[0::2], row[1::2] = acc.real.astype(f32), acc.imag.astype(f32)
        wide.append(row)
        pos += n
    scale = None
    if fmt == "cs16":
        peak = max(float(np.abs(r).max()) for r in wide)
        wide = [np.round(r.astype(np.float64) * (32000.0 / peak)).astype(np.int16) for r in wide]
        scale = f32(peak / 32000.0)
    widened = [r if fmt == "cf32" else H.widened(r, fmt, scale) for r in wide]
    p = qpsk_amd.pfb_params(channels=M, taps_per_branch=K_, gain=GAIN)
    y = PC.pfb_reference(np.concatenate(widened), M, K_, qpsk_amd.pfb_design(p), qpsk_amd.pfb_twiddles(M), gain=GAIN)
    model = PC.PyPfb(M, K_)
    cuts = [model.call(w) for w in widened]
    want = []
    for c in range(M):
        dm = O.OracleDemod(fs // D, rs, K.ALPHA, span, tsc=K.TSC)
        at, frames = 0, []
        for cnt in cuts:
            frames.append(dm.DeModulateBytes(y[c, 2 * at: 2 * (at + cnt)], START, STOP))
            at += cnt
        want.append(frames)
    return wide, scale, p, cuts, want


@pytest.mark.parametrize("fmt", ["cf32", "cs16"])
def test_the_chain_on_device_rows_equals_the_oracle_chain(Q, dev, fmt):
    """Every frame equals the oracle chain's, lost frames included: the equality
    is what is asserted.  That it is no equality of nothing: the oracle chain
    itself receives all 32 frames of rounds 1 and 2."""
    torch = dev
    M, span = E2E["M"], E2E["span"]
    wide, scale, p, cuts, want = wideband_case(fmt)
    for c in range(M):
        for k in (1, 2):
            assert want[c][k] == payload(c, k), f"the oracle chain lost carrier {c} round {k}"
    fs_out, rs = K.FS // (M // 2), K.FS // (2 * M)
    n_cap = max(w.size // 2 for w in wide)
    pf = Q.Channeliser(1, p)
    cap = pf.out_bound(n_cap)
    dm = Q.BatchDemodulator(M, Q.params(fs_out, rs, K.ALPHA, span, max_samples_per_call=cap))
    fr = Q.DeviceFramer(M, START, STOP)
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    for h in (pf, dm, fr):
        h.set_stream(st.cuda_stream)
    ms = dm.max_symbols(cap)
    rows = torch.zeros((1, 2 * n_cap), dtype=getattr(torch, H.FORMATS[fmt].torch_dtype), device="cuda")
    chans = torch.zeros((M, 2 * cap), dtype=torch.float32, device="cuda")
    bits = torch.zeros((M, (2 * ms + 7) // 8 + 8), dtype=torch.uint8, device="cuda")
    nbits = torch.zeros(M, dtype=torch.int64, device="cuda")
    offs = torch.zeros(M, dtype=torch.int64, device="cuda")
    pay = torch.zeros((M, 256), dtype=torch.uint8, device="cuda")
    npay = torch.zeros(M, dtype=torch.int64, device="cuda")
    try:
        for k, w in enumerate(wide):
            n = w.size // 2
            rows[0, : 2 * n].copy_(torch.from_numpy(w), non_blocking=False)
            n_out = pf.apply_device(rows, n, chans, fmt=fmt, scale_in=scale)
            assert n_out[0] == cuts[k]
            lens = pf.lengths_for_demod(n_out)
            dm.process_device_fmt(chans, int(n_out.max()), bits, nbits, "cf32", lengths=lens)
            Q.tsc_find_device(bits, nbits, K.TSC, offs, st.cuda_stream)
            fr.push(bits, nbits, pay, npay, offs)
            cnt, pb = npay.cpu().numpy(), pay.cpu().numpy()
            for c in range(M):
                assert bytes(pb[c, : int(cnt[c])]) == want[c][k], (c, k)
        assert dm.status() == 0
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream())
        for h in (pf, dm):
            h.close()
