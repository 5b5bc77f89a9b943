"""The format-tagged entry points (CF32 / CS16 / CS8 / CU8) at the drop-in
boundary, without a GPU: the header declares them, libqpsk_demod.so exports
them, the binding lists them, and what needs no device answers as documented.
"""
import os
import re
import subprocess

import numpy as np

import qpsk_amd as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FMT_ENTRY_POINTS = [
    "qpsk_fmt_sample_bytes", "qpsk_demod_process_fmt", "qpsk_demod_process_async_fmt",
    "qpsk_demod_set_input_scale", "qpsk_demod_get_input_scale", "qpsk_rx_create_fmt", "qpsk_rx_next_slot_fmt",
    "qpsk_rx_submit_fmt", "qpsk_demod_group_process_fmt",
]


def header_text():
    with open(os.path.join(ROOT, "include", "qpsk_demod.h")) as f:
        return f.read()


def test_header_declares_the_format_tagged_entry_points():
    text = header_text()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in FMT_ENTRY_POINTS:
        assert re.search(r"\bint\s+" + n + r"\s*\(", src), n
    # untyped rows and a stride in elements of the format
    for n in ("qpsk_demod_process_fmt", "qpsk_demod_process_async_fmt", "qpsk_rx_submit_fmt",
              "qpsk_demod_group_process_fmt"):
        decl = " ".join(re.search(n + r"\s*\(([^;]*)\)\s*;", src).group(1).split())
        assert "int32_t fmt" in decl and "const void *iq" in decl and "int64_t stride_elems" in decl, n
    assert re.search(r"qpsk_rx_next_slot_fmt\s*\(\s*qpsk_rx \*r,\s*int32_t fmt,\s*void \*\*iq,\s*"
                     r"int64_t \*stride_elems\s*\)", src)
    assert re.search(r"qpsk_rx_create_fmt\s*\(\s*qpsk_demod \*h,\s*int32_t depth,\s*int32_t fmt,", src)
    for name, tag in (("CF32", 0), ("CS16", 1), ("CS8", 2), ("CU8", 3)):
        assert re.search(rf"#define\s+QPSK_FMT_{name}\s+{tag}\b", text), name
        assert getattr(Q, "FMT_" + name) == tag
    assert re.search(r"#define\s+QPSK_ABI_VERSION\s+3\b", text), "additive only: the ABI version stays"


def test_header_cites_what_the_block_replaces_and_stands_beside():
    text = header_text()
    # behind the CS16 blocks, whose phrases stay the first of their kind
    block = text[text.index("Format-tagged entry points"): text.index("qpsk_demod_group_process_fmt(")]
    assert text.index("CS16 input") < text.index("The same ring for CS16") < text.index("Format-tagged entry points")
    assert "ModDemodOverSDR.cs:63-64" in block and ":116-183" in block
    assert "S8toF32" in block and "U8toS8" in block
    for beside in ("qpsk_demod_process / qpsk_demod_process_async", "qpsk_rx_create / qpsk_rx_next_slot / qpsk_rx_submit",
                   "qpsk_demod_group_process for rows of any format", "qpsk_demod_set_cs16_scale"):
        assert beside in block, beside


def test_library_exports_them_and_the_binding_lists_them():
    out = subprocess.check_output(["nm", "-D", "--defined-only", Q.LIB_PATH]).decode()
    L = Q.lib()
    for n in FMT_ENTRY_POINTS:
        assert re.search(r"\bT " + n + r"\b", out), n
        assert hasattr(L, n), n
        assert n in Q.EXPORTED_SYMBOLS, n
    for m in ("process_fmt", "process_device_fmt", "process_device_async_fmt", "set_input_scale", "input_scale"):
        assert callable(getattr(Q.BatchDemodulator, m)), m
    assert callable(Q.DemodGroup.process_fmt) and callable(Q.HostRing.create_fmt)
    assert L.qpsk_abi_version() == 3


def test_sample_bytes_needs_no_device():
    L = Q.lib()
    assert [L.qpsk_fmt_sample_bytes(f) for f in (Q.FMT_CF32, Q.FMT_CS16, Q.FMT_CS8, Q.FMT_CU8)] == [8, 4, 2, 2]
    assert L.qpsk_fmt_sample_bytes(-1) < 0 and L.qpsk_fmt_sample_bytes(4) < 0
    assert Q.fmt_sample_bytes(Q.FMT_CU8) == 2


def test_null_handle_group_and_ring_are_argument_null():
    L, C = Q.lib(), Q.C
    v = C.c_float()
    x = np.zeros(8, np.int8)
    nb = np.zeros(1, np.int64)
    bits = np.zeros(64, np.uint8)
    for fmt in (Q.FMT_CF32, Q.FMT_CS16, Q.FMT_CS8, Q.FMT_CU8, 4):   # the null check comes before the format's
        assert L.qpsk_demod_set_input_scale(None, fmt, C.c_float(1.0)) == Q.QPSK_ERR_ARGUMENT_NULL
        assert L.qpsk_demod_get_input_scale(None, fmt, C.byref(v)) == Q.QPSK_ERR_ARGUMENT_NULL
        assert L.qpsk_demod_process_fmt(None, fmt, 0, x.ctypes.data, 8, 4, None, Q.MEM_HOST, bits.ctypes.data, 64,
                                        nb.ctypes.data, None, 0, None) == Q.QPSK_ERR_ARGUMENT_NULL
        assert L.qpsk_demod_process_async_fmt(None, fmt, 0, x.ctypes.data, 8, 4, None, bits.ctypes.data, 64,
                                              nb.ctypes.data, None, 0, None) == Q.QPSK_ERR_ARGUMENT_NULL
        assert L.qpsk_demod_group_process_fmt(None, fmt, 0, x.ctypes.data, 8, 4, None, Q.MEM_HOST, bits.ctypes.data,
                                              64, nb.ctypes.data, None, 0, None) == Q.QPSK_ERR_ARGUMENT_NULL
        r, p = C.c_void_p(), C.c_void_p()
        assert L.qpsk_rx_create_fmt(None, 2, fmt, C.byref(r)) == Q.QPSK_ERR_ARGUMENT_NULL
        assert L.qpsk_rx_next_slot_fmt(None, fmt, C.byref(p), None) == Q.QPSK_ERR_ARGUMENT_NULL
        assert L.qpsk_rx_submit_fmt(None, fmt, x.ctypes.data, 8, 4, None, None) == Q.QPSK_ERR_ARGUMENT_NULL
