"""The bit-error counter (qpsk_ber_count, include/qpsk_demod.h "Bit errors,
counted where the bits are") without a GPU: the header declares it, the
library exports it, the binding lists it, the 64-byte row has one layout in
the header, the library, ctypes and numpy; the host function equals
bench.ber_after_lock, the definition it restates, on seeded and hand-worked
cases (tests/ber_cases.py), in every row layout; every rejection answers with
its code and writes nothing.  All counts are integers: the tolerance is 0.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ber_cases as B
import qpsk_amd as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["qpsk_ber_params_init", "qpsk_ber_row_size", "qpsk_ber_count", "qpsk_ber_count_device"]
# the header's row, in order: (name, C type, numpy type, offset)
FIELDS = [("bit_errors", "int64_t", "i8", 0), ("bits", "int64_t", "i8", 8), ("lost_windows", "int64_t", "i8", 16),
          ("slips", "int64_t", "i8", 24), ("windows", "int64_t", "i8", 32), ("last_offset", "int64_t", "i8", 40),
          ("located", "int32_t", "i4", 48), ("reserved[3]", "int32_t", "i4", 52)]
CASES = B.cases()
WITH_YARDSTICK = [c for c in CASES if c.ref.size and c.ref.size % 8 == 0]


def header_text():
    with open(os.path.join(ROOT, "include", "qpsk_demod.h")) as f:
        return f.read()


def test_header_declares_the_structs_and_the_entry_points():
    text = header_text()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"typedef\s+struct\s+qpsk_ber_row\s*\{(.*?)\}\s*qpsk_ber_row\s*;", src, flags=re.S).group(1)
    assert [tuple(m.split()) for m in body.split(";") if m.strip()] == [(ctype, name) for name, ctype, _, _ in FIELDS]
    body = re.search(r"typedef\s+struct\s+qpsk_ber_params\s*\{(.*?)\}\s*qpsk_ber_params\s*;", src, flags=re.S).group(1)
    assert [tuple(m.split()) for m in body.split(";") if m.strip()] == [
        ("int64_t", "skip_bits"), ("int32_t", "window"), ("int32_t", "key_bits"), ("int32_t", "search"),
        ("int32_t", "reserved[3]")]
    decl = lambda n: " ".join(re.search(r"\b" + n + r"\s*\(([^;]*)\)\s*;", src).group(1).split())
    assert decl("qpsk_ber_params_init") == "qpsk_ber_params *p"
    assert decl("qpsk_ber_row_size") == "void"
    rows = ("const qpsk_ber_params *p, const uint8_t *rx_bits, int64_t rx_stride_bytes, const int64_t *n_rx_bits, "
            "const uint8_t *ref_bits, int64_t ref_stride_bytes, const int64_t *n_ref_bits, int32_t n_streams, ")
    assert decl("qpsk_ber_count") == rows + "qpsk_ber_row *out"
    assert decl("qpsk_ber_count_device") == rows + "qpsk_ber_row *out_dev, void *hip_stream"
    assert re.search(r"#define\s+QPSK_ABI_VERSION\s+3\b", text), "additive only: the ABI version stays"
    block = text[text.index("Bit errors, counted where the bits are"): text.index("int qpsk_ber_count(")]
    for phrase in ("testAtDataLevel.cs:44-46", "testFullDemodChain.cs", "ber_after_lock", "smallest i",
                   "e > m / 8", "R = 0 or N = 0", "no byte at or past ceil(n / 8)"):
        assert phrase in block, phrase


def test_library_exports_them_and_the_binding_lists_them():
    out = subprocess.check_output(["nm", "-D", "--defined-only", Q.LIB_PATH]).decode()
    L = Q.lib()
    for n in ENTRY_POINTS:
        assert re.search(r"\bT " + n + r"\b", out), n
        assert hasattr(L, n), n
        assert n in Q.EXPORTED_SYMBOLS, n
    for f in ("ber_count", "ber_count_device", "ber_summary", "ber_params"):
        assert callable(getattr(Q, f)), f
    assert L.qpsk_abi_version() == 3


def test_one_row_layout_everywhere():
    assert Q.lib().qpsk_ber_row_size() == 64 == Q.BER_ROW_DTYPE.itemsize == C.sizeof(Q.BerRow) == Q.ber_row_size()
    names = [f[0].split("[")[0] for f in FIELDS]
    assert list(Q.BER_ROW_DTYPE.names) == names == [f[0] for f in Q.BerRow._fields_]
    for (_, _, npt, off), name in zip(FIELDS, names):
        assert Q.BER_ROW_DTYPE.fields[name][1] == off, name
        assert Q.BER_ROW_DTYPE.fields[name][0].base == np.dtype(npt), name
        assert getattr(Q.BerRow, name).offset == off, name
    assert Q.BER_ROW_DTYPE.fields["reserved"][0].shape == (3,)
    assert C.sizeof(Q.BerParams) == 32 and Q.BerParams.window.offset == 8 and Q.BerParams.reserved.offset == 20


def test_params_init_gives_the_bench_values():
    p = Q.BerParams(-1, -1, -1, -1, (C.c_int32 * 3)(7, 7, 7))
    Q.lib().qpsk_ber_params_init(C.byref(p))
    assert (p.skip_bits, p.window, p.key_bits, p.search, list(p.reserved)) == (8000, 2048, 64, 512, [0, 0, 0])
    Q.lib().qpsk_ber_params_init(None)              # a null pointer is ignored


# ---------------------------------------------------------------------------
# equivalence with the bench
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def expected():
    """name -> ber_after_lock's (errs, bits, lost, slips), each case on its own."""
    return {c.name: B.yardstick(c) for c in WITH_YARDSTICK}


@pytest.fixture(scope="module")
def rows():
    """name -> the row Q.ber_count gives the case, batched by parameter set, plain layout."""
    out = {}
    for params, cs in B.groups():
        for c, r in zip(cs, B.host_rows(cs)):
            out[c.name] = B.row_dict(r)
    return out


def test_ber_count_equals_ber_after_lock(expected, rows):
    assert len(WITH_YARDSTICK) >= 30
    for c in WITH_YARDSTICK:
        r = rows[c.name]
        got = (r["bit_errors"], r["bits"], r["lost_windows"], r["slips"])
        print(c.name, got)
        assert got == expected[c.name], c.name
    # the set as a whole exercises every count
    total = np.sum([expected[c.name] for c in WITH_YARDSTICK], axis=0)
    assert all(total > 0), total
    # first match is part of the definition: slips on clean periodic data
    assert expected["period24"][3] > 0 and expected["period24"][0] == 0 and expected["period24"][2] == 0


def test_the_restated_definition_equals_ber_after_lock(expected):
    """A check of the tests' own model, not of the library (it calls no new
    entry point beyond importing the cases): tests/ber_cases.model serves the
    cases ber_after_lock cannot take (N no multiple of 8), and
    test_every_field_of_every_case holds Q.ber_count to it; where both the
    model and ber_after_lock apply they must agree, or that test proves nothing."""
    for c in WITH_YARDSTICK:
        m = B.model(c.rx, c.ref, **c.params)
        assert (m["bit_errors"], m["bits"], m["lost_windows"], m["slips"]) == expected[c.name], c.name


def test_every_field_of_every_case(rows):
    for c in CASES:
        assert rows[c.name] == B.model(c.rx, c.ref, **c.params), c.name
        if c.hand is not None:
            assert rows[c.name] == c.hand, c.name
    assert sum(c.hand is not None for c in CASES) >= 12
    assert rows["negative_offset"]["last_offset"] == -50
    assert rows["N_zero"] == dict(bit_errors=0, bits=0, lost_windows=38, slips=0, windows=38, last_offset=0, located=0)
    assert rows["R199"]["windows"] == 0 and rows["R200"]["windows"] == 1 and rows["R201"]["windows"] == 1
    assert rows["ref_ends_in_window"]["bits"] % 100 == 58        # the last counted window has m = 2960 - 2902


@pytest.mark.parametrize("skip", [2 ** 63 - 1, 2 ** 63 - 6, 2 ** 63 - 2049, 2 ** 63 - 1 - (1 << 20), 1 << 62, 3999])
@pytest.mark.parametrize("window", [64, 2048, 1 << 20])
def test_any_skip_bits_up_to_int64_max_leaves_a_row_of_zeros(skip, window):
    """skip_bits is any int64 >= 0.  Past the row there is no window: the call
    returns, with a row of zeros (w + W must not be formed: it would wrap)."""
    c = next(c for c in CASES if c.name == "clean")
    rx, n_rx, _ = B.laid_out([c.rx])
    ref, n_ref, _ = B.laid_out([c.ref])
    row = Q.ber_count(rx, n_rx, ref, n_ref, skip_bits=skip, window=window, key_bits=16, search=32)
    assert B.row_dict(row[0]) == dict.fromkeys(B.FIELDS, 0)


@pytest.mark.parametrize("pad,base", [(0, 0), (1, 1), (3, 3), (13, 0), (1, 0), (0, 1), (3, 1)])
def test_row_layouts_do_not_matter(rows, pad, base):
    """Strides beyond the rows, base pointers off by 1 and 3 bytes, and 0xFF in
    every bit that is not a row's own (the rest of its last byte included)."""
    for params, cs in B.groups():
        for c, r in zip(cs, B.host_rows(cs, pad, base)):
            assert B.row_dict(r) == rows[c.name], (c.name, pad, base)


def test_whole_reference_row_by_default():
    c = next(c for c in CASES if c.name == "flips30")
    rx, n_rx, _ = B.laid_out([c.rx])
    ref = np.packbits(c.ref)[None, :]
    a = Q.ber_count(rx, n_rx, ref, **c.params)
    b = Q.ber_count(rx, n_rx, ref, np.array([8 * ref.shape[1]]), **c.params)
    assert a.tobytes() == b.tobytes() and int(a["bits"][0]) > 0
    s = Q.ber_summary(a)
    assert s == {"bit_errors": int(a["bit_errors"][0]), "bits": int(a["bits"][0]),
                 "ber": int(a["bit_errors"][0]) / int(a["bits"][0]), "lost_windows": int(a["lost_windows"][0]),
                 "symbol_slips": int(a["slips"][0]), "streams": 1}
    assert Q.ber_summary(np.zeros(3, Q.BER_ROW_DTYPE))["ber"] is None
    assert Q.ber_count(np.zeros((0, 4), np.uint8), [], np.zeros((0, 4), np.uint8)).size == 0


# ---------------------------------------------------------------------------
# rejections
# ---------------------------------------------------------------------------
def _call(p=None, rx=True, n_rx=True, ref=True, n_ref=True, S=2, out=True, rx_stride=16, ref_stride=16,
          counts=(100, 100), ref_counts=(128, 128)):
    """One raw qpsk_ber_count call over two 16-byte rows; returns (rc, whether out is untouched)."""
    L = Q.lib()
    par = Q.ber_params(skip_bits=0, window=32, key_bits=8, search=4)
    for k, v in (p if isinstance(p, dict) else {}).items():
        setattr(par, k, v)
    rxa, refa = np.zeros(32, np.uint8), np.zeros(32, np.uint8)
    nrx, nref = np.array(counts, np.int64), np.array(ref_counts, np.int64)
    sentinel = np.full(4 * 64, 0xAA, np.uint8)
    rc = L.qpsk_ber_count(C.byref(par) if p != "null" else None, rxa.ctypes.data if rx else None, rx_stride,
                          nrx.ctypes.data if n_rx else None, refa.ctypes.data if ref else None, ref_stride,
                          nref.ctypes.data if n_ref else None, S, sentinel.ctypes.data if out else None)
    return rc, bool((sentinel == 0xAA).all())


REJECTED = [
    (dict(p="null"), Q.QPSK_ERR_ARGUMENT_NULL), (dict(rx=False), Q.QPSK_ERR_ARGUMENT_NULL),
    (dict(n_rx=False), Q.QPSK_ERR_ARGUMENT_NULL), (dict(ref=False), Q.QPSK_ERR_ARGUMENT_NULL),
    (dict(n_ref=False), Q.QPSK_ERR_ARGUMENT_NULL), (dict(out=False), Q.QPSK_ERR_ARGUMENT_NULL),
    (dict(S=-1), Q.QPSK_ERR_ARGUMENT), (dict(rx_stride=-16), Q.QPSK_ERR_ARGUMENT),
    (dict(ref_stride=-1), Q.QPSK_ERR_ARGUMENT),
    (dict(p=dict(key_bits=0)), Q.QPSK_ERR_OUT_OF_RANGE), (dict(p=dict(key_bits=65, window=100)), Q.QPSK_ERR_OUT_OF_RANGE),
    (dict(p=dict(window=7)), Q.QPSK_ERR_OUT_OF_RANGE), (dict(p=dict(window=(1 << 20) + 1)), Q.QPSK_ERR_OUT_OF_RANGE),
    (dict(p=dict(search=-1)), Q.QPSK_ERR_OUT_OF_RANGE), (dict(p=dict(search=(1 << 20) + 1)), Q.QPSK_ERR_OUT_OF_RANGE),
    (dict(p=dict(skip_bits=-1)), Q.QPSK_ERR_OUT_OF_RANGE),
    # the host form sees the counts: the second row's is refused after the first row's was fine
    (dict(counts=(100, -1)), Q.QPSK_ERR_ARGUMENT), (dict(counts=(100, 129)), Q.QPSK_ERR_ARGUMENT),
    (dict(ref_counts=(128, -5)), Q.QPSK_ERR_ARGUMENT), (dict(ref_counts=(128, 129)), Q.QPSK_ERR_ARGUMENT),
    (dict(counts=(100, 2 ** 63 - 1)), Q.QPSK_ERR_ARGUMENT),
    # no row holds 2^61 bits, whatever stride the caller claims
    (dict(counts=(100, 1 << 61), rx_stride=1 << 59), Q.QPSK_ERR_ARGUMENT),
    (dict(ref_counts=(128, 1 << 61), ref_stride=1 << 59), Q.QPSK_ERR_ARGUMENT),
]


@pytest.mark.parametrize("kw,code", REJECTED, ids=[str(i) for i in range(len(REJECTED))])
def test_rejections_write_nothing(kw, code):
    rc, untouched = _call(**kw)
    assert rc == code and untouched, (kw, rc)
    assert Q.lib().qpsk_last_error()


def test_accepted_edges_of_the_ranges():
    for p in (dict(key_bits=64, window=64), dict(key_bits=1, window=1), dict(window=1 << 20), dict(search=1 << 20),
              dict(search=0)):
        rc, untouched = _call(p=p)
        assert rc == Q.QPSK_OK and not untouched, p
    assert _call(S=0) == (Q.QPSK_OK, True)          # no stream: nothing is written
    assert _call(counts=(128, 128))[0] == Q.QPSK_OK  # a count of exactly 8 * stride fits
    with pytest.raises(ValueError):
        Q.ber_count(np.zeros((1, 4), np.uint8), [40], np.zeros((1, 4), np.uint8))
