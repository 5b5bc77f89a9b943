"""Reset, read and write the state of selected streams, at the drop-in boundary
and on the host (no GPU): the header declares the entry points, libqpsk_demod.so
exports them, the binding lists them, and the three host-only functions
(qpsk_stream_list_check, qpsk_state_blob_select, qpsk_state_blob_merge) cut
and join blobs byte for byte.

The blobs are built in numpy (tests/state_blobs.py).  Every 32-bit word of a
carry, a history and a delay line holds (section, stream, index), and so does
every field of a record the checker takes as data, its padding included; the
fields it holds to a range get in-range values that differ from stream to
stream.  A row that lands in the wrong place, or a section cut at the wrong
offset, therefore shows in the bytes.  The expected sub-blob is numpy fancy
indexing of state_blob_parts, put together again by make_blob: tolerance 0.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import common as K
import qpsk_amd as Q
from state_blobs import CARRY_MAX, FLL_TAPS, fresh_records, make_blob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HOST_ONLY = ["qpsk_stream_list_check", "qpsk_state_blob_select", "qpsk_state_blob_merge"]
ON_A_HANDLE = ["reset_streams", "streams_state_bytes", "get_streams_state", "set_streams_state"]
ENTRY_POINTS = HOST_ONLY + ["qpsk_demod_" + n for n in ON_A_HANDLE] + ["qpsk_demod_group_" + n for n in ON_A_HANDLE]

# (sps, span) -> taps 65, 129 and 16: an even tap count leaves a history row of
# 8 * 15 bytes, no multiple of 16
SHAPES = [(8, 8), (4, 32), (3, 5)]
TAPS = {(8, 8): 65, (4, 32): 129, (3, 5): 16}
S = 7
DATA_FIELDS = ["integ", "theta", "freq", "psi", "psq", "pdi", "pdq", "diff_pi", "diff_pq", "fll_phase", "fll_freq",
               "iqb_re", "iqb_im"]


def params_of(sps, span):
    return Q.params(K.FS, K.FS // sps, K.ALPHA, span)


def words(section, n, per_row):
    """[n, per_row] uint32: section in the top 4 bits, stream in the next 12, index below."""
    s = np.arange(n, dtype=np.uint32)[:, None]
    i = np.arange(per_row, dtype=np.uint32)[None, :]
    return (np.uint32(section) << np.uint32(28)) | (s << np.uint32(16)) | i


def coded_blob(n, taps, first=0):
    """A valid blob of n streams that numbers its own words; first: the number
    the first stream carries (so two blobs share no row)."""
    rec = fresh_records(n)
    sid = np.arange(first, first + n)
    for k, f in enumerate(DATA_FIELDS):
        dt = rec.dtype.fields[f][0]
        u = np.uint64 if dt.itemsize == 8 else np.uint32
        rec[f] = ((np.uint64(1) << np.uint64(60 if dt.itemsize == 8 else 28)) | (sid.astype(np.uint64) << np.uint64(16))
                  | np.uint64(k)).astype(u).view(dt)
    rec["mu"] = (sid % 63 + 1) / 64.0
    rec["base"] = sid % 5
    rec["carry_n"] = 3 + sid
    rec["fll_pos"] = sid % FLL_TAPS
    rec["has_prev"] = sid & 1
    rec["diff_have"] = (sid >> 1) & 1
    rec["error"] = sid % 4
    rec.view(np.uint8).reshape(n, -1)[:, -8:] = (0xA0 + sid % 16)[:, None]   # the record's padding is moved too
    sec = [(words(k + 2, n, 2 * per) + (np.uint32(first) << np.uint32(16))).view(np.float32).reshape(n, per, 2)
           for k, per in enumerate((CARRY_MAX, taps - 1, 2 * FLL_TAPS))]
    return make_blob(rec, taps, *sec)


def picked(blob, n, taps, ids):
    """Rows ids of blob by numpy fancy indexing, as a blob of len(ids) streams."""
    rec, carry, hist, dl = Q.state_blob_parts(blob, n, taps)
    ids = np.asarray(ids, dtype=np.int64)
    return make_blob(rec[ids], taps, carry[ids], hist[ids], dl[ids])


def lists(n):
    return [[0], [n - 1], [4, 3], list(range(n - 1, -1, -1))]


def raw(fn, p, n_streams, blob, ids, sub, n=None, blob_len=None, sub_len=None):
    """The C call on exact-size copies: (status, blob after, sub after, message)."""
    a = C.create_string_buffer(bytes(blob), max(len(blob), 1))
    b = C.create_string_buffer(bytes(sub), max(len(sub), 1))
    arr = (C.c_int32 * max(len(ids), 1))(*ids)
    rc = fn(C.byref(p), n_streams, a, len(blob) if blob_len is None else blob_len, arr, len(ids) if n is None else n,
            b, len(sub) if sub_len is None else sub_len)
    return rc, a.raw[:len(blob)], b.raw[:len(sub)], Q.lib().qpsk_last_error().decode()


def header_text():
    with open(os.path.join(ROOT, "include", "qpsk_demod.h")) as f:
        return f.read()


def test_header_declares_every_entry_point():
    text = header_text()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = lambda n: " ".join(re.search(r"\b" + n + r"\s*\(([^;]*)\)\s*;", src).group(1).split())
    for n in ENTRY_POINTS:
        kind = "int64_t" if n.endswith("_bytes") else "int"
        assert re.search(r"\b" + kind + r"\s+" + n + r"\s*\(", src), n
    assert decl("qpsk_stream_list_check") == "int32_t n_streams, const int32_t *streams, int32_t n"
    assert decl("qpsk_state_blob_select") == ("const qpsk_demod_params *p, int32_t n_streams, const void *blob, "
                                              "int64_t blob_bytes, const int32_t *streams, int32_t n, void *sub, "
                                              "int64_t sub_bytes")
    assert decl("qpsk_state_blob_merge") == ("const qpsk_demod_params *p, int32_t n_streams, void *blob, "
                                             "int64_t blob_bytes, const int32_t *streams, int32_t n, const void *sub, "
                                             "int64_t sub_bytes")
    for owner, arg in (("qpsk_demod", "qpsk_demod *h"), ("qpsk_demod_group", "qpsk_demod_group *g")):
        assert decl(owner + "_reset_streams") == arg + ", const int32_t *streams, int32_t n"
        assert decl(owner + "_streams_state_bytes") == "const " + arg + ", int32_t n"
        assert decl(owner + "_get_streams_state") == arg + ", const int32_t *streams, int32_t n, void *host_buf, int64_t buf_bytes"
        assert decl(owner + "_set_streams_state") == (arg + ", const int32_t *streams, int32_t n, const void *host_buf, "
                                                      "int64_t buf_bytes")
    assert re.search(r"#define\s+QPSK_ABI_VERSION\s+3\b", text), "additive only: the ABI version stays"
    block = text[text.index("Selected streams"): text.index("int qpsk_demod_reset_streams(")]
    for phrase in ("QPSKDeModulator.cs:11-56", "QPSKDeModulator.cs:20-73", "leaves the link sums alone", "qpsk_rx ring",
                   "names the position and the value"):
        assert phrase in block, phrase


def test_library_exports_them_and_the_binding_lists_them():
    out = subprocess.check_output(["nm", "-D", "--defined-only", Q.LIB_PATH]).decode()
    L = Q.lib()
    for n in ENTRY_POINTS:
        assert re.search(r"\bT " + n + r"\b", out), n
        assert hasattr(L, n), n
        assert n in Q.EXPORTED_SYMBOLS, n
    for cls in (Q.BatchDemodulator, Q.DemodGroup):
        for m in ("reset_streams", "get_streams_state", "set_streams_state"):
            assert callable(getattr(cls, m)), (cls, m)
    for f in ("stream_list_check", "state_blob_select", "state_blob_merge"):
        assert callable(getattr(Q, f)), f
    assert L.qpsk_abi_version() == 3
    assert len(set(Q.EXPORTED_SYMBOLS)) == len(Q.EXPORTED_SYMBOLS)


def test_null_arguments_are_argument_null():
    L = Q.lib()
    p = params_of(8, 8)
    blob = coded_blob(S, 65)
    sub = picked(blob, S, 65, [1])
    a, b = C.create_string_buffer(blob, len(blob)), C.create_string_buffer(sub, len(sub))
    ids = (C.c_int32 * 1)(1)
    NULL = Q.QPSK_ERR_ARGUMENT_NULL
    assert L.qpsk_stream_list_check(S, None, 1) == NULL
    for fn in (L.qpsk_state_blob_select, L.qpsk_state_blob_merge):
        assert fn(C.byref(p), S, a, len(blob), ids, 1, b, len(sub)) == Q.QPSK_OK
        assert fn(None, S, a, len(blob), ids, 1, b, len(sub)) == NULL
        assert fn(C.byref(p), S, None, len(blob), ids, 1, b, len(sub)) == NULL
        assert fn(C.byref(p), S, a, len(blob), None, 1, b, len(sub)) == NULL
        assert fn(C.byref(p), S, a, len(blob), ids, 1, None, len(sub)) == NULL
    for owner in ("qpsk_demod", "qpsk_demod_group"):
        assert getattr(L, owner + "_reset_streams")(None, ids, 1) == NULL
        assert getattr(L, owner + "_reset_streams")(None, None, 0) == NULL
        assert getattr(L, owner + "_get_streams_state")(None, ids, 1, b, len(sub)) == NULL
        assert getattr(L, owner + "_set_streams_state")(None, ids, 1, b, len(sub)) == NULL
        assert getattr(L, owner + "_streams_state_bytes")(None, 1) == 0
    assert b"null" in L.qpsk_last_error()


def test_blob_sizes():
    for (sps, span), taps in TAPS.items():
        assert Q.design(params_of(sps, span))[0].size == taps
        for n in (1, 3):
            assert Q.state_blob_bytes(n, taps) == len(make_blob(fresh_records(n), taps)) \
                == 32 + n * (112 + 2048 + 8 * (taps - 1) + 640)


@pytest.mark.parametrize("sps,span", SHAPES)
def test_select_is_fancy_indexing(sps, span):
    p, taps = params_of(sps, span), TAPS[(sps, span)]
    blob = coded_blob(S, taps)
    Q.state_blob_check(p, S, blob)
    for ids in lists(S):
        sub = Q.state_blob_select(p, S, blob, ids)
        assert sub == picked(blob, S, taps, ids), ids
        Q.state_blob_check(p, len(ids), sub)
        assert np.frombuffer(sub, np.int32, 8)[2] == len(ids)
    # one stream of a one-stream blob is the blob
    one = coded_blob(1, taps, first=9)
    assert Q.state_blob_select(p, 1, one, [0]) == one


@pytest.mark.parametrize("sps,span", SHAPES)
def test_merge_undoes_select_and_touches_only_the_listed_rows(sps, span):
    p, taps = params_of(sps, span), TAPS[(sps, span)]
    blob = coded_blob(S, taps)
    for ids in lists(S):
        assert Q.state_blob_merge(p, S, blob, ids, Q.state_blob_select(p, S, blob, ids)) == blob, ids
    other = coded_blob(S, taps, first=100)
    for src, dst in (([0], [S - 1]), ([4, 3], [1, 6]), ([6, 0, 2], [2, 5, 0]), (list(range(S)), list(range(S - 1, -1, -1)))):
        sub = Q.state_blob_select(p, S, other, src)
        got = Q.state_blob_merge(p, S, blob, dst, sub)
        assert len(got) == len(blob) and got[:32] == blob[:32]
        Q.state_blob_check(p, S, got)
        want, new = Q.state_blob_parts(blob, S, taps), Q.state_blob_parts(other, S, taps)
        for sec_want, sec_new in zip(want, new):
            sec_want[dst] = sec_new[src]
        assert got == make_blob(want[0], taps, *want[1:]), (src, dst)
        # stated once more on the bytes: every section's other rows are the old ones
        for sec_got, sec_old in zip(Q.state_blob_parts(got, S, taps), Q.state_blob_parts(blob, S, taps)):
            keep = [s for s in range(S) if s not in dst]
            assert sec_got[keep].tobytes() == sec_old[keep].tobytes()


def bad_lists():
    """(list, n or None, position or None, the value the message must hold)"""
    return [([1, -1, 2], None, 1, -1), ([1, 2, S], None, 2, S), ([3, 1, 5, 1], None, 3, 1), ([2, 2], None, 1, 2),
            ([0], 0, None, 0), (list(range(S)) + [0], None, None, S + 1), ([0], -1, None, -1)]


def test_list_check():
    for ids in lists(S) + [[2, 0, 6]]:
        Q.stream_list_check(S, ids)
    Q.stream_list_check(1, [0])
    for ids, n, pos, value in bad_lists():
        arr = (C.c_int32 * len(ids))(*ids)
        assert Q.lib().qpsk_stream_list_check(S, arr, len(ids) if n is None else n) == Q.QPSK_ERR_ARGUMENT, ids
        msg = Q.lib().qpsk_last_error().decode()
        if pos is None:
            assert "n = %d" % value in msg, msg
        else:
            assert "position %d: index %d " % (pos, value) in msg, msg
    with pytest.raises(ValueError, match="position 1: index -1"):
        Q.stream_list_check(S, [1, -1])
    with pytest.raises(ValueError, match="n = 0"):
        Q.stream_list_check(S, [])


@pytest.mark.parametrize("sps,span", SHAPES)
def test_rejected_calls_change_nothing(sps, span):
    L = Q.lib()
    p, taps = params_of(sps, span), TAPS[(sps, span)]
    blob = coded_blob(S, taps)
    fill = lambda n: b"\xaa" * Q.state_blob_bytes(n, taps)

    def refused(fn, ids, sub, **kw):
        rc, a, b, msg = raw(fn, p, S, blob, ids, sub, **kw)
        assert rc == Q.QPSK_ERR_ARGUMENT, (ids, kw, msg)
        assert a == blob and b == sub, "a rejected call wrote"
        return msg

    for ids, n, pos, value in bad_lists():
        k = len(ids) if n is None else max(n, 1)
        for fn, sub in ((L.qpsk_state_blob_select, fill(k)), (L.qpsk_state_blob_merge, coded_blob(k, taps, first=50))):
            msg = refused(fn, ids, sub, n=n)
            assert ("n = %d" % value if pos is None else "position %d: index %d " % (pos, value)) in msg, msg
    # either length off by one, both ways
    ids = [4, 3]
    good = coded_blob(2, taps, first=50)
    for fn, sub in ((L.qpsk_state_blob_select, fill(2)), (L.qpsk_state_blob_merge, good)):
        for d in (-1, 1):
            refused(fn, ids, sub, blob_len=len(blob) + d)
            refused(fn, ids, sub, sub_len=len(sub) + d)
        assert raw(fn, p, S, blob, ids, sub)[0] == Q.QPSK_OK
    # a sub-blob of another tap count, whole and in its header alone
    refused(L.qpsk_state_blob_merge, ids, coded_blob(2, taps + 2, first=50))
    refused(L.qpsk_state_blob_merge, ids, make_blob(fresh_records(2), taps, hdr_taps=taps + 2))
    refused(L.qpsk_state_blob_merge, ids, make_blob(fresh_records(2), taps, streams=3))
    # a sub-blob row a kernel would misuse: named by its position in the sub-blob
    for field, v in (("carry_n", 257), ("mu", 1.0)):
        rec = fresh_records(2)
        rec[field][1] = v
        msg = refused(L.qpsk_state_blob_merge, ids, make_blob(rec, taps))
        assert re.search(r"stream 1: %s = " % field, msg), msg
        with pytest.raises(ValueError, match="stream 1: %s" % field):
            Q.state_blob_merge(p, S, blob, ids, make_blob(rec, taps))
    # and a blob with such a row is no source and no target
    rec = fresh_records(S)
    rec["carry_n"][5] = 257
    bad = make_blob(rec, taps)
    for fn, sub in ((L.qpsk_state_blob_select, fill(2)), (L.qpsk_state_blob_merge, good)):
        rc, a, b, msg = raw(fn, p, S, bad, ids, sub)
        assert rc == Q.QPSK_ERR_ARGUMENT and a == bad and b == sub and "stream 5: carry_n" in msg
