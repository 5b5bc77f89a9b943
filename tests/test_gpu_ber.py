"""The bit-error counter on the device (qpsk_ber_count_device, ber_count_kernel)
against the host function, byte for byte on the 64-byte rows: the cases of
tests/ber_cases.py batched by parameter set, streams cycling through them, in
rows of several strides and base offsets; the reserved words; a launch on a
stream of its own behind a queued fill; every rejection; more streams than the
grid holds waves; and the chain end to end (synthesise, demodulate, count, all
in device memory) against bench.ber_after_lock on the downloaded rows.  The
counts are integers: the tolerance is 0.
"""
import ctypes as C

import numpy as np
import pytest

import bench
import ber_cases as B
import common as K
from gpu_harness import as_fmt, dev, need_gpu  # noqa: F401  (dev is a fixture)

pytestmark = pytest.mark.gpu

# (bytes added to the stride, base offset): strides of the row bytes, + 1 and + 3 against bases 0, 1 and 3, so a
# row's alignment also changes from row to row behind an aligned base, and stays put behind an odd one
LAYOUTS = [(0, 0), (1, 1), (3, 3), (1, 0), (0, 1), (3, 1), (3, 0)]


def device_view(torch, view, buf):
    """The host view of laid_out() as the same view into a device copy of its buffer."""
    t = torch.from_numpy(buf).cuda()
    base = view.__array_interface__["data"][0] - buf.__array_interface__["data"][0]
    return torch.as_strided(t, view.shape, view.strides, storage_offset=base), t


def device_rows_of(torch, Q, cs, pad, base, **kw):
    """ber_count_device over cases cs in the given layout, between two sentinel
    rows; returns (the S rows, the inputs unchanged?, sentinels unchanged?)."""
    rx, n_rx, rx_buf = B.laid_out([c.rx for c in cs], pad, base)
    ref, n_ref, ref_buf = B.laid_out([c.ref for c in cs], pad, base)
    rx_d, rx_t = device_view(torch, rx, rx_buf)
    ref_d, ref_t = device_view(torch, ref, ref_buf)
    assert rx_d.data_ptr() % 4 == base % 4 and rx_d.stride(0) == rx.shape[1] + pad
    out = torch.full((len(cs) + 2, 64), 0xAA, dtype=torch.uint8, device="cuda")
    got = Q.ber_count_device(rx_d, torch.from_numpy(n_rx).cuda(), ref_d, torch.from_numpy(n_ref).cuda(),
                             out_dev=out[1:-1], **(kw or cs[0].params))
    assert got.data_ptr() == out[1:-1].data_ptr()
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    same_in = bool((rx_t.cpu().numpy() == rx_buf).all() and (ref_t.cpu().numpy() == ref_buf).all())
    return host[1:-1].copy().view(Q.BER_ROW_DTYPE).reshape(-1), same_in, bool((host[[0, -1]] == 0xAA).all())


@pytest.fixture(scope="module")
def host_rows():
    """Per group, the host rows of its cases (computed once)."""
    return [B.host_rows(cs) for _, cs in B.groups()]


@pytest.mark.parametrize("S", [1, 5, 65, 130])
def test_device_equals_host(dev, host_rows, S):
    Q = need_gpu()
    for g, (params, cs) in enumerate(B.groups()):
        pad, base = LAYOUTS[(g + S) % len(LAYOUTS)]
        # streams cycle through the group's cases from a start that moves with S,
        # so one call mixes empty rows, rows that never locate and long rows
        pick = [(s + S) % len(cs) for s in range(S)]
        got, same_in, same_guard = device_rows_of(dev, Q, [cs[k] for k in pick], pad, base)
        want = host_rows[g][pick]
        assert same_in and same_guard, (params, S)
        bad = [cs[k].name for s, k in enumerate(pick) if got[s].tobytes() != want[s].tobytes()]
        assert not bad, (params, S, pad, base, bad[:5], B.row_dict(got[0]), B.row_dict(want[0]))


def test_every_layout_on_every_group(dev, host_rows):
    Q = need_gpu()
    for g, (params, cs) in enumerate(B.groups()):
        for pad, base in LAYOUTS:
            got, same_in, same_guard = device_rows_of(dev, Q, cs, pad, base)
            assert same_in and same_guard
            assert got.tobytes() == host_rows[g].tobytes(), (params, pad, base)


def test_reserved_words_are_written_as_zero(dev):
    Q = need_gpu()
    cs = B.groups()[0][1]
    got, _, _ = device_rows_of(dev, Q, cs, 0, 0)      # over a buffer prefilled with 0xAA
    assert (got["reserved"] == 0).all() and set(np.unique(got["located"])) == {0, 1}


def test_more_streams_than_the_grid_holds_waves(dev):
    """16384 waves run at once at the most; stream 16384 + k is a wave's second."""
    Q = need_gpu()
    cs = [c for c in B.groups()[0][1] if c.rx.size <= 400]   # the short cases: R of 0 .. 201, one window
    assert len(cs) >= 6
    S = 16384 + 133
    pick = [s % len(cs) for s in range(S)]
    got, same_in, same_guard = device_rows_of(dev, Q, [cs[k] for k in pick], 1, 1)
    want = B.host_rows(cs)[pick]
    assert same_in and same_guard and got.tobytes() == want.tobytes()
    assert int(want["windows"].sum()) > S // 2


def test_ordered_on_the_stream_it_is_given(dev):
    """rx_dev is filled on a stream of its own, behind other work queued there;
    the count launched on that stream sees the filled rows."""
    Q = need_gpu()
    torch = dev
    params, cs = B.groups()[0]
    rx, n_rx, rx_buf = B.laid_out([c.rx for c in cs])
    ref, n_ref, ref_buf = B.laid_out([c.ref for c in cs])
    want = B.host_rows(cs)
    src = torch.from_numpy(np.ascontiguousarray(rx)).cuda()
    ref_d = torch.from_numpy(np.ascontiguousarray(ref)).cuda()
    n_rx_d, n_ref_d = torch.from_numpy(n_rx).cuda(), torch.from_numpy(n_ref).cuda()
    for explicit in (True, False):
        rx_d = torch.zeros_like(src)
        ballast = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()               # non-blocking: the null stream does not wait for it
        with torch.cuda.stream(stream):
            for k in range(8):                     # 4 GiB of fills (milliseconds) ahead of the rows' own fill
                ballast.fill_(k)
            rx_d.copy_(src)
            out = Q.ber_count_device(rx_d, n_rx_d, ref_d, n_ref_d,
                                     hip_stream=stream.cuda_stream if explicit else None, **params)
        stream.synchronize()
        got = out.cpu().numpy().view(Q.BER_ROW_DTYPE).reshape(-1)
        assert got.tobytes() == want.tobytes(), explicit


def test_rejections_leave_out_dev_untouched(dev):
    Q = need_gpu()
    torch = dev
    L = Q.lib()
    rows = torch.zeros((2, 16), dtype=torch.uint8, device="cuda")
    counts = torch.full((2,), 100, dtype=torch.int64, device="cuda")
    out = torch.full((4 * 64 + 8,), 0xAA, dtype=torch.uint8, device="cuda")
    good = dict(skip_bits=0, window=32, key_bits=8, search=4)

    def call(p=None, null=None, S=2, rx_stride=16, ref_stride=16, out_off=0, params=True):
        par = Q.ber_params(**dict(good, **(p or {})))
        a = dict(rx=rows.data_ptr(), n_rx=counts.data_ptr(), ref=rows.data_ptr(), n_ref=counts.data_ptr(),
                 out=out.data_ptr() + out_off)
        if null:
            a[null] = None
        return L.qpsk_ber_count_device(C.byref(par) if params else None, a["rx"], rx_stride, a["n_rx"], a["ref"],
                                       ref_stride, a["n_ref"], S, a["out"], None)

    E = Q.QPSK_ERR_ARGUMENT, Q.QPSK_ERR_ARGUMENT_NULL, Q.QPSK_ERR_OUT_OF_RANGE
    assert call(params=False) == E[1]
    for name in ("rx", "n_rx", "ref", "n_ref", "out"):
        assert call(null=name) == E[1], name
    assert call(S=-1) == E[0] and call(rx_stride=-1) == E[0] and call(ref_stride=-16) == E[0]
    assert call(out_off=4) == E[0] and call(out_off=1) == E[0]
    for p in (dict(key_bits=0), dict(key_bits=65, window=100), dict(window=7), dict(window=(1 << 20) + 1),
              dict(search=-1), dict(search=(1 << 20) + 1), dict(skip_bits=-1)):
        assert call(p=p) == E[2], p
    assert call(S=0) == Q.QPSK_OK
    torch.cuda.synchronize()
    assert bool((out == 0xAA).all())
    assert call(out_off=8) == Q.QPSK_OK               # the same call, accepted, writes its two rows
    torch.cuda.synchronize()
    assert not bool((out[8: 8 + 128] == 0xAA).all()) and bool((out[:8] == 0xAA).all())
    assert bool((out[8 + 128:] == 0xAA).all())


def test_counts_the_row_cannot_hold_read_as_no_bits(dev):
    """The device form cannot refuse a count: R < 0 or past the stride is R = 0
    (a row of zeros), N likewise is N = 0 (every window lost)."""
    Q = need_gpu()
    torch = dev
    c = next(c for c in B.cases() if c.name == "clean")
    rx, n_rx, _ = B.laid_out([c.rx] * 5)
    ref, n_ref, _ = B.laid_out([c.ref] * 5)
    n_rx = n_rx.copy()
    n_ref = n_ref.copy()
    n_rx[1], n_rx[2] = -1, 8 * rx.shape[1] + 1
    n_ref[3], n_ref[4] = -7, 8 * ref.shape[1] + 1
    out = Q.ber_count_device(torch.from_numpy(np.ascontiguousarray(rx)).cuda(), torch.from_numpy(n_rx).cuda(),
                             torch.from_numpy(np.ascontiguousarray(ref)).cuda(), torch.from_numpy(n_ref).cuda(),
                             **c.params)
    torch.cuda.synchronize()
    got = [B.row_dict(r) for r in out.cpu().numpy().view(Q.BER_ROW_DTYPE).reshape(-1)]
    assert got[0] == c.hand
    zero = dict.fromkeys(B.FIELDS, 0)
    assert got[1] == zero and got[2] == zero
    assert got[3] == got[4] == dict(zero, windows=38, lost_windows=38)


@pytest.mark.parametrize("fmt", ["cf32", "cs8"])
def test_end_to_end_in_device_memory(dev, fmt):
    """Synthesise, demodulate and count with nothing copied in between; the
    rows equal ber_after_lock on the downloaded bits, stream by stream."""
    Q = need_gpu()
    torch = dev
    S, n, sps, span = 8, 1 << 16, 4, 8
    rs = K.FS // sps
    iq, tx = Q.synth_generate(S, n, K.FS, rs, rrc_alpha=K.ALPHA, rrc_span=span, esn0_db=10.0)
    b = Q.BatchDemodulator(S, Q.params(K.FS, rs, K.ALPHA, span, max_samples_per_call=n))
    stream = torch.cuda.Stream()
    try:
        b.set_stream(stream.cuda_stream)
        ms = b.max_symbols(n)
        with torch.cuda.stream(stream):
            bits = torch.zeros((S, (2 * ms + 7) // 8 + 8), dtype=torch.uint8, device="cuda")
            nbits = torch.zeros(S, dtype=torch.int64, device="cuda")
            if fmt == "cf32":
                torch.cuda.synchronize()
                b.process_device(iq, n, bits, nbits)
            else:
                x = iq.cpu().numpy()
                q = np.clip(np.round(x * (64.0 / np.abs(x).max())), -128, 127).astype(np.int8)
                xd = torch.from_numpy(as_fmt(q, fmt)).cuda()
                torch.cuda.synchronize()
                b.process_device_fmt(xd, n, bits, nbits, fmt=fmt)
            n_ref = torch.full((S,), 8 * tx.shape[1], dtype=torch.int64, device="cuda")
            out = Q.ber_count_device(bits, nbits, tx, n_ref)          # the default parameters
        stream.synchronize()
    finally:
        b.close()
    rows = out.cpu().numpy().view(Q.BER_ROW_DTYPE).reshape(-1)
    per_stream = [bench.ber_after_lock(bits[s: s + 1], nbits[s: s + 1], tx[s: s + 1], 1) for s in range(S)]
    for s, want in enumerate(per_stream):
        got = (int(rows["bit_errors"][s]), int(rows["bits"][s]), int(rows["lost_windows"][s]), int(rows["slips"][s]))
        print(fmt, s, got)
        assert got == want, (s, got, want)
    assert sum(int(r["bits"]) > 0 for r in rows) >= S // 2, "the batch never locked"
    errs, total, lost, slips = bench.ber_after_lock(bits, nbits, tx, S)
    assert Q.ber_summary(rows) == {"bit_errors": errs, "bits": total, "ber": (errs / total) if total else None,
                                   "lost_windows": lost, "symbol_slips": slips, "streams": S}
    # the host form on the downloaded rows agrees too
    host = Q.ber_count(bits.cpu().numpy(), nbits.cpu().numpy(), tx.cpu().numpy())
    assert host.tobytes() == rows.tobytes()
