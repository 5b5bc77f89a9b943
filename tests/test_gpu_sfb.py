"""The polyphase synthesis bank on the device (qpsk_sfb_*, csrc/qpsk_sfb.hip)
against the numpy yardstick (sfb_cases.sfb_reference), byte for byte against
its own host form (qpsk_sfb_apply_host), and its state against the Python model
after every call.  Every comparison is at tolerance 0; inputs are finite (a
NaN's payload is the one thing an x86 host and gfx950 do not share).

qpsk_sfb_tile_frames names the per-call frame counts at which a kernel takes
another workgroup (the transform kernel's tiles, the sum kernel's runs) or the
call another pass (the slab); the calls below are one frame shorter, exactly
that and one longer, start at an odd frame, and are shorter than the history."""
import functools

import numpy as np
import pytest

import common as K
import gpu_harness as H
import pfb_cases as PC
import qpsk_amd
import sfb_cases as SC
from gpu_harness import Q, dev  # noqa: F401  (fixtures)
from test_gpu_pfb import sentinel_rows

pytestmark = pytest.mark.gpu
f32 = np.float32
MIN_LEAD = {"cf32": 4, "cs16": 4, "cs8": 2, "cu8": 2}


def design(M, K_):
    return qpsk_amd.pfb_design(qpsk_amd.pfb_params(channels=M, taps_per_branch=K_))


def assert_only_samples_written(buf, pitch, lead_bytes, counts, sample_bytes, what):
    """Every byte of an output buffer outside row r's first counts[r] samples is still 0xAA."""
    full = buf.cpu().numpy()
    keep = np.ones(full.size, bool)
    for r, c in enumerate(counts):
        keep[lead_bytes + r * pitch: lead_bytes + r * pitch + sample_bytes * int(c)] = False
    assert (full[keep] == 0xAA).all(), f"{what}: written past a row's samples or between rows"


def device_calls(torch, sf, x, calls, models=None, fmt="cf32", out_fmt="cf32", lead_bytes=0, scale_in=None,
                 scale_out=None):
    """The call sequence (x [B M, 2 n] of fmt; calls: per call the [B] lengths in
    frames) on device rows of their own; per call the [B] list of output rows
    cut to their samples.  models: per band a PySfb (fed the widened floats);
    the handle's state is compared after every call."""
    B, M = sf.n_bands, sf.channels
    D = M // 2
    Fi, Fo = H.FORMATS[fmt], H.FORMATS[out_fmt]
    dt = qpsk_amd.sfb_state_dtype(M, sf.p.taps_per_branch)
    pos = np.zeros(B, np.int64)
    out = []
    for ci, lens in enumerate(calls):
        n = max(lens)
        rows, _, _ = sentinel_rows(torch, B * M, max(n, 1), Fi.torch_dtype, lead_bytes)
        host = rows.cpu().numpy().copy()
        for b in range(B):
            host[b * M: (b + 1) * M, : 2 * lens[b]] = x[b * M: (b + 1) * M, 2 * pos[b]: 2 * (pos[b] + lens[b])]
        rows.copy_(torch.from_numpy(host))
        out_lead = MIN_LEAD[out_fmt] if lead_bytes else 0
        o, obuf, opitch = sentinel_rows(torch, B, max(n, 1) * D, Fo.torch_dtype, out_lead)
        assert sf.apply_device(rows, n, o, fmt=fmt, out_fmt=out_fmt, lengths=H.lengths_of(lens), scale_in=scale_in,
                               scale_out=scale_out) is o
        got = o.cpu().numpy()
        assert np.array_equal(rows.cpu().numpy(), host), f"call {ci}: the input rows changed"
        assert_only_samples_written(obuf, opitch, out_lead, [l * D for l in lens], 2 * got.itemsize, f"call {ci}")
        out.append([got[b, : 2 * lens[b] * D].copy() for b in range(B)])
        if models:
            st = sf.states()
            for b in range(B):
                w = host[b * M: (b + 1) * M, : 2 * lens[b]]
                w = w if fmt == "cf32" else H.widened(w, fmt, scale_in)
                assert models[b].call(w) == lens[b] * D, (ci, b)
                assert st[b].tobytes() == models[b].record(dt).tobytes(), f"state after call {ci}, band {b}"
        pos += np.array(lens)
    return out


def host_calls(Q, p, x, calls, taps=None, scale_out=1.0):
    """The same sequence through qpsk_sfb_apply_host."""
    M = p.channels
    B, D = x.shape[0] // M, M // 2
    state = Q.sfb_state_init(p, B)
    pos = np.zeros(B, np.int64)
    out = []
    for lens in calls:
        n = max(lens)
        rows = np.zeros((B * M, 2 * max(n, 1)), f32)
        for b in range(B):
            rows[b * M: (b + 1) * M, : 2 * lens[b]] = x[b * M: (b + 1) * M, 2 * pos[b]: 2 * (pos[b] + lens[b])]
        state, o = Q.sfb_apply_host(p, state, rows, lengths=lens, n=n, taps=taps, scale_out=scale_out)
        out.append([o[b, : 2 * lens[b] * D].copy() for b in range(B)])
        pos += np.array(lens)
    return out, state


def joined(outs, b):
    return np.concatenate([c[b] for c in outs])


def assert_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} vs {want.shape} {want.dtype}"
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got != want) if got.dtype != f32 else np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        pytest.fail(f"{what}: {bad.size} elements differ, first at sample {bad[0] // 2}: {got[bad[0]]!r} vs {want[bad[0]]!r}")


def tile_calls(M, K_, B):
    """Per call the [B] lengths in frames.  Band 0: one frame (so the next call
    starts at an odd frame), then calls of T - 1, 0, T and T + 1 frames for the
    transform kernel's tile T, then 127, 128 and 129 for the sum kernel's run, a
    call shorter than the history, and one frame.  Band b takes the same calls
    b places on."""
    T = qpsk_amd.sfb_tile_frames(M, K_, qpsk_amd.SFB_TILE_TRANSFORM)
    R = qpsk_amd.sfb_tile_frames(M, K_, qpsk_amd.SFB_TILE_SUM)
    base = [1, T - 1, 0, T, T + 1, R - 1, R, R + 1, max(1, 2 * K_ - 2), 1]
    return [[base[(i + b) % len(base)] for b in range(B)] for i in range(len(base))]


# ---------------------------------------------------------------------------
# 1. the kernels against the yardstick and against the host form
# ---------------------------------------------------------------------------
SHAPES = [(M, 2, 3 if i % 2 == 0 else 1) for i, M in enumerate(PC.CHANNELS)] + \
         [(16, k, 1 if i % 2 == 0 else 3) for i, k in enumerate(PC.BRANCH_TAPS) if k != 2]


@pytest.mark.parametrize("M,K_,B", SHAPES, ids=[f"M{m}-K{k}-B{b}" for m, k, b in SHAPES])
def test_kernels_equal_the_yardstick_and_the_host_form_at_the_tile_edges(Q, dev, M, K_, B):
    calls = tile_calls(M, K_, B)
    n = max(sum(c[b] for c in calls) for b in range(B))
    x = SC.random_rows(B, M, n, seed=3 * M + K_)
    models = [SC.PySfb(M, K_) for _ in range(B)]
    scale = f32(M // 2)
    sf = Q.SynthesisBank(B, channels=M, taps_per_branch=K_)
    got = device_calls(dev, sf, x, calls, models, lead_bytes=0 if M != 64 else 8, scale_out=scale)
    state = sf.get_state()
    sf.close()
    host, host_state = host_calls(Q, sf.p, x, calls, scale_out=scale)
    assert state == host_state
    g, W = design(M, K_), Q.pfb_twiddles(M)
    for b in range(B):
        for ci in range(len(calls)):
            assert got[ci][b].tobytes() == host[ci][b].tobytes(), f"call {ci} band {b}: device vs host form"
        nb = sum(c[b] for c in calls)
        assert_bits(joined(got, b), SC.sfb_reference(x[b * M: (b + 1) * M, : 2 * nb], M, K_, g, W, scale_out=scale), f"band {b}")


def test_the_largest_transform_with_the_longest_prototype(Q, dev):
    M, K_ = 4096, 8
    frames = 2 * K_ + 2
    x = SC.random_rows(1, M, frames, seed=41)
    sf = Q.SynthesisBank(1, channels=M, taps_per_branch=K_)
    got = device_calls(dev, sf, x, [[frames]], [SC.PySfb(M, K_)], scale_out=3.0)
    sf.close()
    host, _ = host_calls(Q, sf.p, x, [[frames]], scale_out=3.0)
    assert got[0][0].tobytes() == host[0][0].tobytes()
    assert_bits(got[0][0], SC.sfb_reference(x, M, K_, design(M, K_), Q.pfb_twiddles(M), scale_out=3.0), "M = 4096, K = 8")


def test_a_call_of_more_than_one_workgroup_of_the_sum_kernel_at_the_smallest_m(Q, dev):
    """At M = 8 a workgroup of the sum kernel's 256 lanes holds 32 runs, 4096
    frames: the call passes that edge, with the register rings of K = 8 walking
    whole runs."""
    M, K_, B = 8, 8, 2
    edge = 256 // M * qpsk_amd.sfb_tile_frames(M, K_, qpsk_amd.SFB_TILE_SUM)
    calls = [[edge + 129, edge - 1], [3, edge + 1]]
    x = SC.random_rows(B, M, 2 * edge + 200, seed=43)
    sf = Q.SynthesisBank(B, channels=M, taps_per_branch=K_)
    got = device_calls(dev, sf, x, calls, [SC.PySfb(M, K_) for _ in range(B)])
    sf.close()
    g, W = design(M, K_), Q.pfb_twiddles(M)
    for b in range(B):
        nb = sum(c[b] for c in calls)
        assert_bits(joined(got, b), SC.sfb_reference(x[b * M: (b + 1) * M, : 2 * nb], M, K_, g, W), f"band {b}")


def test_a_call_of_more_than_one_slab(Q, dev):
    """Two bands of M = 2048 take slabs of 1024 frames: a call of one frame more
    (its second pass transforms the 2K - 1 frames in front of its one frame
    again, from the call's rows), then one of exactly a slab from an odd frame."""
    M, K_, B = 2048, 2, 2
    S = qpsk_amd.sfb_tile_frames(M, K_, qpsk_amd.SFB_TILE_SLAB) // B
    assert S == SC.slab_frames(M, B) == 1024
    calls = [[S + 1, S - 1], [S, 2]]
    x = SC.random_rows(B, M, 2 * S + 1, seed=44)
    sf = Q.SynthesisBank(B, channels=M, taps_per_branch=K_)
    got = device_calls(dev, sf, x, calls, [SC.PySfb(M, K_) for _ in range(B)])
    sf.close()
    g, W = design(M, K_), Q.pfb_twiddles(M)
    for b in range(B):
        nb = sum(c[b] for c in calls)
        assert_bits(joined(got, b), SC.sfb_reference(x[b * M: (b + 1) * M, : 2 * nb], M, K_, g, W), f"band {b}")


# ---------------------------------------------------------------------------
# 2. formats and scales
# ---------------------------------------------------------------------------
FMT = dict(B=2, n=70, M=32, K=3)
# no powers of two, so the multiply rounds; the yardstick's sums on these rows have a standard deviation of 0.2 and
# reach 0.8, so the integer scales put full scale at 0.4: both clamps take part
SCALE_OUT = {"cf32": 0.3, "cs16": 80011.3, "cs8": 317.3, "cu8": 317.3}


@functools.lru_cache(maxsize=None)
def fmt_case(fmt):
    """2 bands x 32 rows x 70 frames of fmt at a scale of its own, their widened
    floats, and per band the yardstick's sums before the output's scale."""
    B, n, M, K_ = FMT["B"], FMT["n"], FMT["M"], FMT["K"]
    xi = np.array(SC.random_rows(B, M, n, seed=5)) if fmt == "cf32" else H.random_rows(B * M, n, 6, fmt)
    scale = None if fmt == "cf32" else H.FORMATS[fmt].odd_scale
    w = xi if fmt == "cf32" else H.widened(xi, fmt, scale)
    g, W = design(M, K_), qpsk_amd.pfb_twiddles(M)
    acc = [SC.sfb_reference(w[b * M: (b + 1) * M], M, K_, g, W, scale_out=None) for b in range(B)]
    return xi, scale, acc


@pytest.mark.parametrize("fmt", ["cf32", "cs16", "cs8", "cu8"])
def test_every_input_format_on_device_rows_of_both_alignments_and_host_rows(Q, dev, fmt):
    xi, scale, acc = fmt_case(fmt)
    B, n, M, K_ = FMT["B"], FMT["n"], FMT["M"], FMT["K"]
    D = M // 2
    for lead in (0, MIN_LEAD[fmt]):
        sf = Q.SynthesisBank(B, channels=M, taps_per_branch=K_)
        got = device_calls(dev, sf, xi, [[n] * B], fmt=fmt, lead_bytes=lead, scale_in=scale, scale_out=SCALE_OUT["cf32"])
        sf.close()
        for b in range(B):
            assert_bits(got[0][b], SC.quantised(acc[b], "cf32", SCALE_OUT["cf32"]), f"{fmt}, lead {lead}, band {b}")
    # host rows: what lies past a band's samples comes back as it was
    sf = Q.SynthesisBank(B, channels=M, taps_per_branch=K_)
    out = np.frombuffer(b"\xaa" * (B * 2 * n * D * 4), f32).reshape(B, 2 * n * D).copy()
    assert sf.apply_host(np.array(xi), fmt=fmt, out=out, lengths=[n, n - 10], scale_in=scale,
                         scale_out=SCALE_OUT["cf32"]) is out
    sf.close()
    for b, keep in enumerate((n, n - 10)):
        assert_bits(out[b, : 2 * keep * D], SC.quantised(acc[b], "cf32", SCALE_OUT["cf32"])[: 2 * keep * D], f"host rows {fmt}, band {b}")
        assert (out[b, 2 * keep * D:].view(np.uint8) == 0xAA).all()


@pytest.mark.parametrize("fmt,out_fmt", [("cf32", "cs16"), ("cf32", "cs8"), ("cf32", "cu8"), ("cs16", "cs8")])
def test_every_output_format_is_the_quantiser_of_the_sums(Q, dev, fmt, out_fmt):
    xi, scale, acc = fmt_case(fmt)
    B, n, M, K_ = FMT["B"], FMT["n"], FMT["M"], FMT["K"]
    D = M // 2
    so = SCALE_OUT[out_fmt]
    want = [SC.quantised(acc[b], out_fmt, so) for b in range(B)]
    lo, hi = (0, 255) if out_fmt == "cu8" else (np.iinfo(want[0].dtype).min, np.iinfo(want[0].dtype).max)
    hit = np.concatenate(want)
    assert ((hit == lo).any() and (hit == hi).any()) and ((hit > lo) & (hit < hi)).mean() > 0.5
    for lead in (0, MIN_LEAD[fmt]):
        sf = Q.SynthesisBank(B, channels=M, taps_per_branch=K_)
        got = device_calls(dev, sf, xi, [[n] * B], fmt=fmt, out_fmt=out_fmt, lead_bytes=lead, scale_in=scale, scale_out=so)
        sf.close()
        for b in range(B):
            assert_bits(got[0][b], want[b], f"{fmt} -> {out_fmt}, lead {lead}, band {b}")
    sf = Q.SynthesisBank(B, channels=M, taps_per_branch=K_)
    out = sf.apply_host(np.array(xi), fmt=fmt, out_fmt=out_fmt, scale_in=scale, scale_out=so)
    with pytest.raises(ValueError, match="does not normalise"):
        sf.apply_host(np.array(xi), fmt=fmt, out_fmt=out_fmt, scale_in=scale, scale_out=so, norm="peak")
    sf.close()
    for b in range(B):
        assert_bits(out[b, : 2 * n * D], want[b], f"host rows {fmt} -> {out_fmt}, band {b}")


def test_set_taps_takes_effect_behind_the_calls_so_far(Q, dev):
    torch = dev
    M, K_, n = 16, 3, 40
    D = M // 2
    x = SC.random_rows(1, M, 2 * n, seed=7)
    taps = (np.random.default_rng(8).standard_normal(M * K_) * 0.2).astype(f32)
    sf = Q.SynthesisBank(1, channels=M, taps_per_branch=K_)
    # two calls queued on a bound stream, then the taps, then a third call
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        sf.set_stream(st.cuda_stream)
        xd = torch.from_numpy(np.array(x)).cuda()
        outs = [torch.zeros((1, 2 * 20 * D), dtype=torch.float32, device="cuda") for _ in range(3)]
        sf.apply_device(xd[:, :40].contiguous(), 20, outs[0])
        sf.apply_device(xd[:, 40:80].contiguous(), 20, outs[1])
        sf.set_taps(taps)
        for bad in (taps[:-1], np.append(taps, 1.0), np.where(np.arange(M * K_) == 5, np.nan, taps), []):
            with pytest.raises(ValueError):
                sf.set_taps(bad)
        sf.apply_device(xd[:, 80:120].contiguous(), 20, outs[2])
        st.synchronize()
        got = [o.cpu().numpy()[0] for o in outs]
    sf.set_stream(None)
    sf.close()
    W = Q.pfb_twiddles(M)
    before = SC.sfb_reference(x[:, :80], M, K_, design(M, K_), W)
    assert_bits(np.concatenate(got[:2]), before, "before")
    # behind set_taps the history is kept and the new prototype reads it
    p = Q.sfb_params(channels=M, taps_per_branch=K_)
    state, _ = Q.sfb_apply_host(p, Q.sfb_state_init(p, 1), np.ascontiguousarray(x[:, :80]))
    _, after = Q.sfb_apply_host(p, state, np.ascontiguousarray(x[:, 80:120]), taps=taps)
    assert_bits(got[2], after[0], "after (host form)")
    assert_bits(got[2], SC.sfb_reference(x[:, :120], M, K_, taps, W)[2 * 40 * D:], "after")


# ---------------------------------------------------------------------------
# 3. state
# ---------------------------------------------------------------------------
def test_reset_a_subset_and_move_the_state_to_a_second_handle(Q, dev):
    B, M, K_, n = 3, 16, 8, 90
    x = SC.random_rows(B, M, n, seed=9)
    a = Q.SynthesisBank(B, channels=M, taps_per_branch=K_)
    used = np.array([30, 17, 5])
    first = device_calls(dev, a, x, [list(used)])
    blob = a.get_state()
    b = Q.SynthesisBank(B, channels=M, taps_per_branch=K_)
    b.set_state(blob)
    rest = np.concatenate([np.roll(x[s * M: (s + 1) * M], -2 * used[s], axis=1) for s in range(B)])
    tail_a = device_calls(dev, a, rest, [[10] * B, [40] * B])
    tail_b = device_calls(dev, b, rest, [[7] * B, [43] * B])
    assert a.get_state() == b.get_state()
    g, W = design(M, K_), Q.pfb_twiddles(M)
    for s in range(B):
        whole = SC.sfb_reference(x[s * M: (s + 1) * M, : 2 * (used[s] + 50)], M, K_, g, W)
        assert_bits(np.concatenate([first[0][s], joined(tail_a, s)]), whole, f"band {s}")
        assert_bits(joined(tail_b, s), joined(tail_a, s), f"second handle, band {s}")
    for bands in ([], [0, 0], [B], [-1]):
        with pytest.raises(ValueError):
            a.reset_bands(bands)
    before = a.states()
    a.reset_bands([2, 0])
    st = a.states()
    assert (st["in_pos"] == [0, before["in_pos"][1], 0]).all() and (st["out_pos"][[0, 2]] == 0).all()
    assert (st["hist"][[0, 2]].view(np.uint32) == 0).all() and st[1].tobytes() == before[1].tobytes()
    again = device_calls(dev, a, x, [[20] * B])
    a.close()
    b.close()
    for s in (0, 2):
        assert_bits(again[0][s], SC.sfb_reference(x[s * M: (s + 1) * M, :40], M, K_, g, W), f"reset band {s}")


def test_host_rows_whose_staging_grows_and_is_reused_then_set_stream_back_to_none(Q, dev):
    """Host-memory calls of 4, 600 and 4 frames on one handle: the staging and
    scratch buffers are made, freed for larger ones, and then serve a shorter
    call.  Then a device call on a bound torch stream, set_stream(None), one on
    the handle's own stream again, and close(): the caller's stream outlives
    the handle."""
    torch = dev
    B, M, K_, lens = 2, 8, 2, [4, 600, 4, 30, 50]
    D = M // 2
    x = SC.random_rows(B, M, sum(lens), seed=51)
    sf = Q.SynthesisBank(B, channels=M, taps_per_branch=K_)
    want, state = host_calls(Q, sf.p, x, [[n] * B for n in lens])
    pos = 0
    for ci, n in enumerate(lens[:3]):
        out = sf.apply_host(np.ascontiguousarray(x[:, 2 * pos: 2 * (pos + n)]))
        for b in range(B):
            assert_bits(out[b, : 2 * n * D], want[ci][b], f"call {ci} band {b}: device vs host form")
        pos += n
    cuts = [np.ascontiguousarray(x[:, 2 * pos: 2 * (pos + lens[3])]), np.ascontiguousarray(x[:, 2 * (pos + lens[3]):])]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        sf.set_stream(st.cuda_stream)
        o = torch.zeros((B, 2 * sf.out_len(lens[3])), dtype=torch.float32, device="cuda")
        sf.apply_device(torch.from_numpy(cuts[0]).cuda(), lens[3], o)
        first = o.cpu().numpy()
    sf.set_stream(None)
    o = torch.zeros((B, 2 * sf.out_len(lens[4])), dtype=torch.float32, device="cuda")
    sf.apply_device(torch.from_numpy(cuts[1]).cuda(), lens[4], o)
    second = o.cpu().numpy()
    assert sf.get_state() == state
    sf.close()
    st.synchronize()
    for ci, rows in ((3, first), (4, second)):
        for b in range(B):
            assert_bits(rows[b], want[ci][b], f"call {ci} band {b}: device vs host form")


def test_what_a_live_handle_refuses_changes_nothing(Q, dev):
    torch = dev
    B, M, K_, n = 2, 16, 2, 5
    D = M // 2
    sf = Q.SynthesisBank(B, channels=M, taps_per_branch=K_)
    x = SC.random_rows(B, M, 20, seed=10)
    device_calls(dev, sf, x, [[4] * B])
    before = sf.get_state()
    rows, rbuf, _ = sentinel_rows(torch, B * M, n)
    o, obuf, _ = sentinel_rows(torch, B, n * D)
    big, bbuf, _ = sentinel_rows(torch, B * M, 2 * n * D)
    i16, ibuf, _ = sentinel_rows(torch, B * M, 2 * n, "int16")
    o16, o16buf, _ = sentinel_rows(torch, B, 2 * n * D, "int16")
    bad = sf.states()
    bad["out_pos"][1] += 1
    with pytest.raises(ValueError, match="band 1: out_pos"):
        sf.set_state(bad.tobytes())
    bad = sf.states()
    bad["reserved"][0, 3] = 1
    with pytest.raises(ValueError, match="band 0: reserved"):
        sf.set_state(bad.tobytes())
    with pytest.raises(ValueError):
        sf.set_state(before[:-1])
    L_ = Q.lib()

    def raw(fmt_in, fmt_out, norm=qpsk_amd.NORM_FIXED, mem=qpsk_amd.MEM_DEVICE):
        return L_.qpsk_sfb_apply_fmt(sf._h, fmt_in, rows.data_ptr(), rows.stride(0), 1.0, fmt_out, norm, o.data_ptr(),
                                     o.stride(0), 1.0, n, None, mem)

    A = Q.QPSK_ERR_ARGUMENT
    assert raw(4, 0) == A and raw(-1, 0) == A and raw(0, 4) == A                 # a bad format
    assert raw(0, 0, norm=qpsk_amd.NORM_PEAK) == A and raw(0, 0, norm=7) == A and raw(0, 0, mem=9) == A
    refused = [
        lambda: sf.apply_device(torch.as_strided(rows, (B * M, 2 * n - 2), (rows.stride(0) - 1, 1)), n - 1, o),   # odd stride
        lambda: sf.apply_device(torch.as_strided(rows, (B * M, 2 * n), (2 * n - 2, 1)), n, o),    # stride < 2 n
        lambda: sf.apply_device(rows, n, torch.as_strided(o, (B, 2 * n * D), (2 * n * D - 2, 1))),  # stride < 2 n D
        lambda: sf.apply_device(i16[:, 1: 2 * n + 1], n, o, fmt="cs16"),                          # 2-byte aligned
        lambda: sf.apply_device(rows, n, o16[:, 1: 2 * n * D + 1], out_fmt="cs16"),
        lambda: sf.apply_device(big[:, : 2 * n], n, big[B * M - B:, 2 * n - 2:]),                 # rows overlap
        lambda: sf.apply_device(big[:, 2 * n * D:], n, big[:B, : 2 * n * D + 2]),
        lambda: sf.apply_device(rows, n, o, lengths=[1, n + 1]),
        lambda: sf.apply_device(rows, n, o, lengths=[-1, 2]),
        lambda: sf.apply_device(i16, n, o, fmt="cs16", scale_in=float("inf")),
        lambda: sf.apply_device(i16, n, o, fmt="cs16", scale_in=0.0),
        lambda: sf.apply_device(rows, n, o, scale_out=0.0),
        lambda: sf.apply_device(rows, n, o, scale_out=float("nan")),
        lambda: sf.apply_device(rows, n, o, norm="peak"),
    ]
    for k, call in enumerate(refused):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"refusal {k} was accepted")
    torch.cuda.synchronize()
    for t in (rbuf, obuf, bbuf, ibuf, o16buf):
        assert (t.cpu().numpy() == 0xAA).all()
    assert sf.get_state() == before
    rows.zero_()
    sf.apply_device(rows, n, o)                          # and a call that is in order runs
    assert sf.states()["in_pos"].tolist() == [4 + n] * B
    sf.close()


# ---------------------------------------------------------------------------
# 4. the chain: modulator -> synthesis bank -> channeliser -> demodulator -> framer
# ---------------------------------------------------------------------------
START, STOP, E2E, HOPS, payload = SC.START, SC.STOP, SC.E2E, SC.HOPS, SC.payload


@pytest.mark.parametrize("fmt", ["cf32", "cs16", "cs8"])
def test_the_chain_on_device_rows_equals_the_cpu_chain(Q, dev, fmt):
    """Every frame equals the CPU chain's, which receives all 48
    (tests/test_sfb_abi.py::test_the_cpu_chain_receives_every_frame)."""
    torch = dev
    M, K_, span, tail = E2E["M"], E2E["K"], E2E["span"], E2E["tail"]
    D = M // 2
    fs_ch, rs = K.FS // D, K.FS // (2 * M)
    mult, scale_in = HOPS[fmt]
    n, _, want = SC.wideband_case(fmt)
    m = Q.QPSKModulator(fs_ch, rs, K.ALPHA, span, tsc=K.TSC)
    assert m.output_floats(8 * (len(START) + 48 + len(STOP))) // 2 == n - tail
    sf = Q.SynthesisBank(1, channels=M, taps_per_branch=K_)
    pf = Q.Channeliser(1, channels=M, taps_per_branch=K_, gain=1.0)
    dm = Q.BatchDemodulator(M, Q.params(fs_ch, rs, K.ALPHA, span, max_samples_per_call=n))
    fr = Q.DeviceFramer(M, START, STOP)
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    for h in (m, sf, pf, dm, fr):
        h.set_stream(st.cuda_stream)
    ms = dm.max_symbols(n)
    rows = torch.zeros((M, 2 * n), dtype=torch.float32, device="cuda")       # the tail stays zero
    wide = torch.zeros((1, 2 * n * D), dtype=getattr(torch, H.FORMATS[fmt].torch_dtype), device="cuda")
    chans = torch.zeros((M, 2 * n), dtype=torch.float32, device="cuda")
    n_mod = torch.zeros(M, dtype=torch.int64, device="cuda")
    bits = torch.zeros((M, (2 * ms + 7) // 8 + 8), dtype=torch.uint8, device="cuda")
    nbits = torch.zeros(M, dtype=torch.int64, device="cuda")
    offs = torch.zeros(M, dtype=torch.int64, device="cuda")
    pay = torch.zeros((M, 256), dtype=torch.uint8, device="cuda")
    npay = torch.zeros(M, dtype=torch.int64, device="cuda")
    try:
        for k in range(E2E["rounds"]):
            host = np.stack([np.frombuffer(payload(c, k), np.uint8) for c in range(M)])
            m.modulate_bytes_device(torch.from_numpy(host.copy()).cuda(), torch.from_numpy(np.full(M, 48, np.int64)).cuda(),
                                    START, STOP, rows, n_mod)
            sf.apply_device(rows, n, wide, out_fmt=fmt, scale_out=mult * D)
            n_out = pf.apply_device(wide, n * D, chans, fmt=fmt, scale_in=scale_in, out_cap=n)
            assert n_out[0] == n
            dm.process_device_fmt(chans, n, bits, nbits, "cf32")
            Q.tsc_find_device(bits, nbits, K.TSC, offs, st.cuda_stream)
            fr.push(bits, nbits, pay, npay, offs)
            cnt, pb = npay.cpu().numpy(), pay.cpu().numpy()
            assert (n_mod.cpu().numpy() == 2 * (n - tail)).all()
            for c in range(M):
                assert bytes(pb[c, : int(cnt[c])]) == want[c][k], (c, k)
        assert dm.status() == 0
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream())
        for h in (m, sf, pf, dm):
            h.close()
