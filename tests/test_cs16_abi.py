"""CS16 (int16 I,Q) input at the drop-in boundary, without a GPU: the header
declares the entry points, libqpsk_demod.so exports them, the binding lists
them, and the argument checks that need no device answer as documented.
"""
import os
import re
import subprocess

import numpy as np

import qpsk_amd as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CS16_ENTRY_POINTS = [
    "qpsk_demod_set_cs16_scale", "qpsk_demod_get_cs16_scale", "qpsk_demod_process_cs16",
    "qpsk_demod_process_async_cs16", "qpsk_rx_create_cs16", "qpsk_rx_next_slot_cs16", "qpsk_rx_submit_cs16",
]


def header_text():
    with open(os.path.join(ROOT, "include", "qpsk_demod.h")) as f:
        return f.read()


def test_header_declares_the_cs16_entry_points():
    src = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    for n in CS16_ENTRY_POINTS:
        assert re.search(r"\bint\s+" + n + r"\s*\(", src), n
    # int16 rows and an int16 stride where the float entry points take floats
    for n in ("qpsk_demod_process_cs16", "qpsk_demod_process_async_cs16", "qpsk_rx_submit_cs16"):
        decl = re.search(n + r"\s*\(([^;]*)\)\s*;", src).group(1)
        assert "const int16_t *iq" in decl and "int64_t stride_i16" in decl, n
    assert re.search(r"qpsk_rx_next_slot_cs16\s*\(\s*qpsk_rx \*r,\s*int16_t \*\*iq,\s*int64_t \*stride_i16\s*\)", src)
    assert re.search(r"#define\s+QPSK_ABI_VERSION\s+3\b", header_text()), "additive only: the ABI version stays"


def test_header_cites_what_each_entry_point_replaces():
    """As throughout the header: the comment above the CS16 block names the
    reference code and the float entry points it stands beside."""
    src = header_text()
    block = src[src.index("CS16 input"): src.index("qpsk_demod_process_async_cs16(")]
    assert "ModDemodOverSDR.cs:116-183" in block
    assert "qpsk_demod_process / qpsk_demod_process_async" in block
    ring = src[src.index("The same ring for CS16"): src.index("qpsk_rx_create_cs16(")]
    assert "qpsk_rx_create / qpsk_rx_next_slot / qpsk_rx_submit" in ring


def test_library_exports_the_cs16_entry_points():
    out = subprocess.check_output(["nm", "-D", "--defined-only", Q.LIB_PATH]).decode()
    L = Q.lib()
    for n in CS16_ENTRY_POINTS:
        assert re.search(r"\bT " + n + r"\b", out), n
        assert hasattr(L, n), n


def test_binding_lists_them_and_has_the_methods():
    for n in CS16_ENTRY_POINTS:
        assert n in Q.EXPORTED_SYMBOLS, n
    for m in ("set_cs16_scale", "cs16_scale", "process_cs16", "process_device_cs16", "process_device_async_cs16"):
        assert callable(getattr(Q.BatchDemodulator, m)), m
    import inspect
    assert "fmt" in inspect.signature(Q.HostRing.__init__).parameters


def test_null_handle_and_null_ring_are_argument_null():
    L = Q.lib()
    v = Q.C.c_float()
    assert L.qpsk_demod_set_cs16_scale(None, Q.C.c_float(1.0)) == Q.QPSK_ERR_ARGUMENT_NULL
    assert L.qpsk_demod_get_cs16_scale(None, Q.C.byref(v)) == Q.QPSK_ERR_ARGUMENT_NULL
    x = np.zeros(8, np.int16)
    nb = np.zeros(1, np.int64)
    bits = np.zeros(64, np.uint8)
    assert L.qpsk_demod_process_cs16(None, 0, x.ctypes.data, 8, 4, None, Q.MEM_HOST, bits.ctypes.data, 64,
                                     nb.ctypes.data, None, 0, None) == Q.QPSK_ERR_ARGUMENT_NULL
    assert L.qpsk_demod_process_async_cs16(None, 0, x.ctypes.data, 8, 4, None, bits.ctypes.data, 64,
                                           nb.ctypes.data, None, 0, None) == Q.QPSK_ERR_ARGUMENT_NULL
    r = Q.C.c_void_p()
    assert L.qpsk_rx_create_cs16(None, 2, Q.C.byref(r)) == Q.QPSK_ERR_ARGUMENT_NULL
    p = Q.C.c_void_p()
    assert L.qpsk_rx_next_slot_cs16(None, Q.C.byref(p), None) == Q.QPSK_ERR_ARGUMENT_NULL
    assert L.qpsk_rx_submit_cs16(None, x.ctypes.data, 8, 4, None, None) == Q.QPSK_ERR_ARGUMENT_NULL
