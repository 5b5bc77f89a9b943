"""qpsk_quantise_iq and the format-tagged modulator entry points at the drop-in
boundary, without a GPU: the symbols exist, the host quantiser equals the numpy
restatement of its two rules on oracle modulator rows (tolerance 0), and what
needs no device answers as documented.

The numpy restatement (quantise_ref) is the reference of tests/test_gpu_mod_fmt.py
too:
  FIXED  float32 multiply, np.clip, np.trunc (CU8: + 128; CF32: the product)
  PEAK   float64 x / m * full with m the row's largest |component|, 1.0 when
         < 1e-12; np.clip, np.trunc
"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import common as K
import oracle as O
import qpsk_amd as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ["qpsk_quantise_iq", "qpsk_mod_modulate_fmt", "qpsk_mod_modulate_bytes_fmt"]
RANGE = {"cs16": (-32768, 32767), "cs8": (-128, 127), "cu8": (-128, 127)}
INT_FORMATS = ("cs16", "cs8", "cu8")
# full scale; no power of two (the multiply rounds); saturating (the rows' peaks are 0.36 ... 0.75)
SCALES = {"cs16": (32767.0, 20011.3, 100000.0), "cs8": (127.0, 100.3, 400.0), "cu8": (127.0, 100.3, 400.0),
          "cf32": (1.0, 0.3, 32767.0)}
# (sps, span, alpha, payload bits): the third is the 16 256-float row
CONFIGS = [(8, 8, 0.4, 1001), (2, 10, 0.9, 2000), (4, 32, 0.35, 4000)]


def quantise_ref(x, fmt, norm="fixed", scale=1.0, rounding=np.trunc, peak_type=np.float64):
    """(row, peak) by the rules in numpy; rounding and peak_type build the
    neighbouring rules the data must tell apart from the right one."""
    assert x.dtype == np.float32
    if norm == "fixed":
        v = x * np.float32(scale)
        assert v.dtype == np.float32
        if fmt == "cf32":
            return v, None
        peak = None
    else:
        peak = np.abs(x).max(initial=np.float32(0))
        m = peak_type(peak) if peak >= 1e-12 else peak_type(1.0)
        v = x.astype(peak_type) / m * peak_type(RANGE[fmt][1])
        assert v.dtype == peak_type
    lo, hi = RANGE[fmt]
    q = rounding(np.clip(v, lo, hi)).astype(np.int32) + (128 if fmt == "cu8" else 0)
    return q.astype(Q._format(fmt)[1]), peak


@functools.lru_cache(maxsize=None)
def oracle_row(sps, span, alpha, n_bits):
    x = O.modulate(K.FS, K.FS // sps, K.random_bits(np.random.default_rng(sps * 100 + span), n_bits),
                   rrc_alpha=alpha, rrc_span=span)
    x.setflags(write=False)
    return x


def test_symbols_are_exported_declared_and_listed():
    out = subprocess.check_output(["nm", "-D", "--defined-only", Q.LIB_PATH]).decode()
    with open(os.path.join(ROOT, "include", "qpsk_demod.h")) as f:
        text = f.read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in NEW_ENTRY_POINTS:
        assert re.search(r"\bT " + n + r"\b", out), n
        assert hasattr(Q.lib(), n) and n in Q.EXPORTED_SYMBOLS, n
        assert re.search(r"\bint\s+" + n + r"\s*\(", src), n
    for name, value in (("QPSK_MOD_NORM_FIXED", Q.NORM_FIXED), ("QPSK_MOD_NORM_PEAK", Q.NORM_PEAK),
                        ("QPSK_MOD_TILE_SAMPLES", Q.MOD_TILE_SAMPLES), ("QPSK_MOD_SCAN_DIBITS", Q.MOD_SCAN_DIBITS)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", text), name
    assert re.search(r"#define\s+QPSK_ABI_VERSION\s+3\b", text) and Q.lib().qpsk_abi_version() == 3
    for m in ("modulate_batch", "modulate_bytes_batch", "modulate_device", "modulate_bytes_device"):
        assert callable(getattr(Q.QPSKModulator, m)), m


def test_the_quantiser_header_needs_no_hip():
    """csrc/qpsk_quantise.h and qpsk_quantise.cpp include no HIP header and call no HIP function."""
    for name in ("qpsk_quantise.h", "qpsk_quantise.cpp"):
        with open(os.path.join(ROOT, "qpsk-modulator-demodulator_amd", "csrc", name)) as f:
            text = f.read()
        assert "hip_runtime" not in text and not re.search(r"\bhip[A-Z]\w*\s*\(", text), name


@pytest.mark.parametrize("fmt", ["cf32", "cs16", "cs8", "cu8"])
def test_fixed_equals_numpy(fmt):
    for cfg in CONFIGS:
        x = oracle_row(*cfg)
        for scale in SCALES[fmt]:
            got, peak = Q.quantise_iq(x, fmt, "fixed", scale)
            want, _ = quantise_ref(x, fmt, "fixed", scale)
            assert peak is None and K.bitwise_equal(got, want), (fmt, cfg, scale)


@pytest.mark.parametrize("fmt", INT_FORMATS)
def test_peak_equals_numpy_and_stores_full_scale_at_the_peak(fmt):
    full = RANGE[fmt][1]
    for cfg in CONFIGS:
        x = oracle_row(*cfg)
        got, peak = Q.quantise_iq(x, fmt, "peak", scale=-1.0)   # scale is ignored
        want, m = quantise_ref(x, fmt, "peak")
        assert K.bitwise_equal(got, want), (fmt, cfg)
        assert peak.dtype == np.float32 and peak == m == np.abs(x).max()
        at = int(np.argmax(np.abs(x)))
        assert int(got[at]) - (128 if fmt == "cu8" else 0) == (full if x[at] > 0 else -full)


def test_the_data_separates_the_rule_from_its_neighbours():
    for fmt in INT_FORMATS:
        lo, hi = RANGE[fmt]
        zero = 128 if fmt == "cu8" else 0
        for cfg in CONFIGS:
            x = oracle_row(*cfg)
            full, odd, sat = SCALES[fmt]
            for scale in (full, odd):
                want, _ = quantise_ref(x, fmt, "fixed", scale)
                for other in (np.rint, np.floor):
                    assert not np.array_equal(want, quantise_ref(x, fmt, "fixed", scale, rounding=other)[0])
            clipped = quantise_ref(x, fmt, "fixed", sat)[0].astype(np.int32) - zero
            v = x * np.float32(sat)
            assert (v > hi).any() and (v < lo).any(), "the saturating scale clips at both ends"
            assert (clipped[v > hi] == hi).all() and (clipped[v < lo] == lo).all()
            for other in (np.rint, np.floor):
                assert not np.array_equal(quantise_ref(x, fmt, "peak")[0],
                                          quantise_ref(x, fmt, "peak", rounding=other)[0])
    # PEAK in float32 is another rule: the double division and multiplication show
    x = oracle_row(4, 32, 0.35, 4000)
    assert x.size == 16256
    n = np.count_nonzero(quantise_ref(x, "cs16", "peak")[0] != quantise_ref(x, "cs16", "peak", peak_type=np.float32)[0])
    assert n >= 1, "float32 x / m * full equals the double one on this row"


def test_rows_of_zeros_and_tiny_rows_divide_by_one():
    x = np.zeros(10, np.float32)
    got, peak = Q.quantise_iq(x, "cu8", "peak")
    assert peak == 0 and (got == 128).all()
    x = np.array([1e-13, -5e-13], np.float32)
    got, peak = Q.quantise_iq(x, "cs16", "peak")
    assert peak == np.abs(x).max() and K.bitwise_equal(got, quantise_ref(x, "cs16", "peak")[0]) and (got == 0).all()


def test_empty_row_gives_peak_zero_and_writes_nothing():
    L = Q.lib()
    out = np.full(8, 0x5A, np.uint8)
    peak = np.full(1, 7.0, np.float32)
    for fmt in (Q.FMT_CS16, Q.FMT_CS8, Q.FMT_CU8):
        peak[0] = 7.0
        assert L.qpsk_quantise_iq(fmt, Q.NORM_PEAK, 1.0, None, 0, out.ctypes.data, peak.ctypes.data) == Q.QPSK_OK
        assert peak[0] == 0 and (out == 0x5A).all()
    assert L.qpsk_quantise_iq(Q.FMT_CS16, Q.NORM_FIXED, 1.0, None, 0, out.ctypes.data, None) == Q.QPSK_OK
    assert (out == 0x5A).all()
    got, pk = Q.quantise_iq(np.zeros(0, np.float32), "cs8", "peak")
    assert got.size == 0 and pk == 0


def test_rejections_leave_out_and_peak_as_they_were():
    L = Q.lib()
    x = oracle_row(*CONFIGS[0])[:64].copy()
    out = np.full(4 * x.size, 0xA5, np.uint8)
    peak = np.full(1, 7.0, np.float32)

    def call(fmt, norm, scale):
        return L.qpsk_quantise_iq(fmt, norm, C.c_float(scale), x.ctypes.data, x.size, out.ctypes.data,
                                  peak.ctypes.data)

    cases = [(4, Q.NORM_FIXED, 1.0, Q.QPSK_ERR_ARGUMENT), (-1, Q.NORM_FIXED, 1.0, Q.QPSK_ERR_ARGUMENT),
             (Q.FMT_CS16, 2, 1.0, Q.QPSK_ERR_ARGUMENT), (Q.FMT_CS16, -1, 1.0, Q.QPSK_ERR_ARGUMENT),
             (Q.FMT_CF32, Q.NORM_PEAK, 1.0, Q.QPSK_ERR_ARGUMENT)]
    cases += [(fmt, Q.NORM_FIXED, bad, Q.QPSK_ERR_OUT_OF_RANGE) for fmt in (Q.FMT_CF32, Q.FMT_CS16, Q.FMT_CS8, Q.FMT_CU8)
              for bad in (0.0, -0.0, -1.0, float("inf"), float("-inf"), float("nan"))]
    for fmt, norm, scale, want in cases:
        assert call(fmt, norm, scale) == want, (fmt, norm, scale)
        assert (out == 0xA5).all() and peak[0] == 7.0, (fmt, norm, scale)
        assert Q.lib().qpsk_last_error()
    assert call(Q.FMT_CS16, Q.NORM_PEAK, float("nan")) == Q.QPSK_OK    # PEAK ignores scale
    with pytest.raises(ValueError):
        Q.quantise_iq(x, "cs16", "fixed", 0.0)
    with pytest.raises(ValueError):
        Q.quantise_iq(x, "cf32", "peak")


def test_modulate_fmt_on_a_null_handle():
    L = Q.lib()
    n = np.zeros(1, np.int64)
    out = np.zeros(8, np.float32)
    assert L.qpsk_mod_modulate_fmt(None, Q.FMT_CS16, Q.NORM_FIXED, 1.0, 1, None, 0, n.ctypes.data, 1, Q.MEM_HOST,
                                   out.ctypes.data, 8, n.ctypes.data, None) == Q.QPSK_ERR_ARGUMENT_NULL
    mark = (C.c_uint8 * 1)(2)
    assert L.qpsk_mod_modulate_bytes_fmt(None, Q.FMT_CS16, Q.NORM_FIXED, 1.0, 1, None, 1, n.ctypes.data, mark, 1, mark, 1,
                                         1, Q.MEM_HOST, out.ctypes.data, 8, n.ctypes.data,
                                         None) == Q.QPSK_ERR_ARGUMENT_NULL
