"""qpsk_state_blob_check, the host check every state blob passes before
qpsk_demod_set_state copies it to the device: no GPU here, the checker alone.

A blob is external input, and the kernels use a record's integers and its
timing phase as addresses.  Blobs are built in numpy (header, STREAM_STATE_DTYPE
records, carries, histories, delay lines).  The allowed ranges asserted here are
derived, not read from the checker:

  carry_n  [0, 256]   the carry array and the MF prefix hold 256 samples
  fll_pos  [0, 40)    the delay line is 2 x 40 entries, written at pos and pos + 40
  tofs     0          a blob is taken between calls; a call's last chunk resets it
  has_prev, diff_have 0 or 1; error 0..3 (bit 0 carry overflow, bit 1 truncated row)
  base     [0, 1 + ceil(sps + 0.1)]: the M&M loop exits with count - 2 <= base <=
           count - 2 + ceil(sps + 0.1), the drop rule then removes count - 3
           samples; 0 is what the reference's NaN timing leaves
  mu       [+0, 1): floor's remainder of a finite time

Every rejection must name the stream and the field; the bad record is never in
stream 0, so a checker that stops after the first record fails.
"""
import math
import re

import numpy as np
import pytest

import common as K
import qpsk_amd as Q
from state_blobs import CARRY_MAX, FLL_TAPS, fresh_records, make_blob

I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1
# (sps, span): the two shapes of the GPU tests, and a fractional sps
SHAPES = [(8, 8), (4, 32)]
S = 5


def taps_of(sps, span):
    return span * sps + 1


def params_of(sps, span):
    return Q.params(K.FS, K.FS // sps, K.ALPHA, span)


def base_hi(sps):
    return 1 + math.ceil(sps + 0.1)


def edited(sps, span, stream, **fields):
    rec = fresh_records(S)
    for k, v in fields.items():
        rec[k][stream] = v
    return make_blob(rec, taps_of(sps, span))


def check(sps, span, blob, n=S):
    Q.state_blob_check(params_of(sps, span), n, blob)


def status(sps, span, blob, n=S):
    import ctypes as C
    buf = C.create_string_buffer(bytes(blob), max(len(blob), 1))
    return Q.lib().qpsk_state_blob_check(C.byref(params_of(sps, span)), n, buf, len(blob))


def test_layout_matches_the_blob_dtype():
    assert Q.STREAM_STATE_DTYPE.itemsize == 112
    assert Q.STATE_CARRY_MAX == CARRY_MAX and Q.STATE_FLL_TAPS == FLL_TAPS
    blob = make_blob(fresh_records(S), 65)
    assert len(blob) == 32 + S * (112 + 8 * 256 + 8 * 64 + 8 * 80)
    rec, carry, hist, dl = Q.state_blob_parts(blob, S, 65)
    assert rec.tobytes() == fresh_records(S).tobytes()
    assert carry.shape == (S, 256, 2) and hist.shape == (S, 64, 2) and dl.shape == (S, 80, 2)


@pytest.mark.parametrize("sps,span", SHAPES)
def test_fresh_state_is_accepted(sps, span):
    check(sps, span, make_blob(fresh_records(S), taps_of(sps, span)))
    check(sps, span, make_blob(fresh_records(1), taps_of(sps, span)), n=1)


def valid_edges(sps):
    sub = 5e-324
    return [("carry_n", 0), ("carry_n", CARRY_MAX), ("fll_pos", 0), ("fll_pos", FLL_TAPS - 1),
            ("has_prev", 0), ("has_prev", 1), ("diff_have", 0), ("diff_have", 1),
            ("error", 0), ("error", 1), ("error", 2), ("error", 3),
            ("base", 0), ("base", 1), ("base", base_hi(sps)),
            ("mu", 0.0), ("mu", sub), ("mu", 0.5), ("mu", float(np.nextafter(1.0, 0.0)))]


@pytest.mark.parametrize("sps,span", SHAPES)
def test_every_edge_of_every_range_is_accepted(sps, span):
    for stream in (1, S - 1):
        for field, v in valid_edges(sps):
            check(sps, span, edited(sps, span, stream, **{field: v}))
    # all upper edges at once, in every stream
    rec = fresh_records(S)
    rec["carry_n"], rec["fll_pos"], rec["has_prev"], rec["diff_have"] = CARRY_MAX, FLL_TAPS - 1, 1, 1
    rec["error"], rec["base"], rec["mu"] = 3, base_hi(sps), np.nextafter(1.0, 0.0)
    check(sps, span, make_blob(rec, taps_of(sps, span)))


def invalid_cases(sps):
    hi = base_hi(sps)
    return [("carry_n", -1), ("carry_n", CARRY_MAX + 1), ("carry_n", I32_MIN), ("carry_n", I32_MAX),
            ("fll_pos", -1), ("fll_pos", FLL_TAPS), ("fll_pos", I32_MAX), ("fll_pos", I32_MIN),
            ("tofs", 1), ("tofs", -1), ("tofs", 2 ** 40), ("tofs", -(2 ** 63)),
            ("has_prev", 2), ("has_prev", -1), ("diff_have", 2), ("diff_have", -1),
            ("error", 4), ("error", -1),
            ("base", -1), ("base", hi + 1), ("base", I32_MIN), ("base", I32_MAX),
            ("mu", -0.0), ("mu", float(np.nextafter(0.0, -1.0))), ("mu", 1.0),
            ("mu", float(np.nextafter(1.0, 2.0))), ("mu", -1.0), ("mu", float("nan")), ("mu", float("inf")),
            ("mu", float("-inf"))]


@pytest.mark.parametrize("sps,span", SHAPES)
@pytest.mark.parametrize("stream", [1, S - 1])
def test_one_bad_field_is_rejected_and_named(sps, span, stream):
    for field, v in invalid_cases(sps):
        blob = edited(sps, span, stream, **{field: v})
        assert status(sps, span, blob) == Q.QPSK_ERR_ARGUMENT, (field, v)
        msg = Q.lib().qpsk_last_error().decode()
        assert re.search(r"stream %d: %s = " % (stream, field), msg), (field, v, msg)
        assert "stream 0" not in msg
        with pytest.raises(ValueError, match=r"stream %d: %s" % (stream, field)):
            check(sps, span, blob)


def test_base_range_follows_sps():
    """1 + ceil(sps + 0.1): 10 at sps 8, 6 at sps 4, 5 at 10/3 samples a symbol."""
    assert base_hi(8) == 10 and base_hi(4) == 6
    for fs, rs, span, hi in ((K.FS, K.FS // 8, 8, 10), (K.FS, K.FS // 4, 32, 6), (K.FS, 3_000_000, 6, 5)):
        p = Q.params(fs, rs, K.ALPHA, span)
        taps = Q.design(p)[0].size
        for v, ok in ((hi, True), (hi + 1, False)):
            rec = fresh_records(2)
            rec["base"][1] = v
            blob = make_blob(rec, taps)
            if ok:
                Q.state_blob_check(p, 2, blob)
            else:
                with pytest.raises(ValueError, match="stream 1: base = %d" % v):
                    Q.state_blob_check(p, 2, blob)


@pytest.mark.parametrize("sps,span", SHAPES)
def test_header_and_length_cases(sps, span):
    """The cases test_state_checkpoint_roundtrip puts to set_state, here put to
    the checker: truncated, padded, wrong magic, wrong format, another stream
    count, another tap count."""
    taps = taps_of(sps, span)
    blob = make_blob(fresh_records(S), taps)
    check(sps, span, blob)
    bad = {
        "truncated": blob[:-8], "padded": blob + b"\0" * 8, "empty": b"", "header only": blob[:32],
        "31 bytes": blob[:31],
        "magic": b"\0" * 4 + blob[4:], "format": blob[:4] + b"\1\0\0\0" + blob[8:],
        "format 3": make_blob(fresh_records(S), taps, fmt=3),
        "streams field": make_blob(fresh_records(S), taps, streams=S + 1),
        "taps field": make_blob(fresh_records(S), taps, hdr_taps=taps + 2),
    }
    for name, b in bad.items():
        assert status(sps, span, b) == Q.QPSK_ERR_ARGUMENT, name
    # a whole blob of another shape: one stream more, one fewer, another tap count
    assert status(sps, span, blob, n=S + 1) == Q.QPSK_ERR_ARGUMENT
    assert status(sps, span, blob, n=S - 1) == Q.QPSK_ERR_ARGUMENT
    assert status(sps, span, make_blob(fresh_records(S), taps + 2)) == Q.QPSK_ERR_ARGUMENT
    other = (4, 32) if (sps, span) == (8, 8) else (8, 8)
    assert status(*other, blob) == Q.QPSK_ERR_ARGUMENT
    assert status(sps, span, blob, n=0) == Q.QPSK_ERR_ARGUMENT
    assert status(sps, span, blob, n=-1) == Q.QPSK_ERR_ARGUMENT


FLOAT_FIELDS = ["integ", "theta", "freq", "psi", "psq", "pdi", "pdq", "diff_pi", "diff_pq", "fll_phase",
                "fll_freq", "iqb_re", "iqb_im"]
ODD_FLOATS = [float("nan"), float("inf"), float("-inf"), -0.0, 1e-45, -1e-45, 5e-324, 3e38, -3e38]


@pytest.mark.parametrize("sps,span", SHAPES)
def test_floats_the_reference_can_hold_are_accepted(sps, span):
    """NaN, +-Inf, -0 and subnormals in every float the reference defines but
    mu (whose range is an address range), and in every sample of the carry,
    the history and the delay line."""
    taps = taps_of(sps, span)
    for v in ODD_FLOATS:
        rec = fresh_records(S)
        for f in FLOAT_FIELDS:
            rec[f] = v
        f32 = np.float32(v)
        blob = make_blob(rec, taps, carry=np.full((S, CARRY_MAX, 2), f32),
                         hist=np.full((S, taps - 1, 2), f32), delay=np.full((S, 2 * FLL_TAPS, 2), f32))
        check(sps, span, blob)
        back = Q.state_blob_parts(blob, S, taps)[0]
        assert back.tobytes() == rec.tobytes()
    for f in FLOAT_FIELDS:   # and one field at a time
        check(sps, span, edited(sps, span, 2, **{f: float("nan")}))


def test_null_arguments_are_argument_errors():
    import ctypes as C
    blob = make_blob(fresh_records(S), 65)
    buf = C.create_string_buffer(blob, len(blob))
    L = Q.lib()
    assert L.qpsk_state_blob_check(None, S, buf, len(blob)) == Q.QPSK_ERR_ARGUMENT
    assert L.qpsk_state_blob_check(C.byref(params_of(8, 8)), S, None, len(blob)) == Q.QPSK_ERR_ARGUMENT
    bad = Q.params(K.FS, 2 * K.FS, K.ALPHA, 8)   # params create would refuse
    assert L.qpsk_state_blob_check(C.byref(bad), S, buf, len(blob)) == Q.QPSK_ERR_ARGUMENT
