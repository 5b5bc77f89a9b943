"""Per-stream link statistics (qpsk_link_stats, qpsk_demod_link_stats) at the
drop-in boundary, without a GPU: the header declares them, libqpsk_demod.so
exports them, the binding lists them, the 64-byte row has one layout in the
header, the library, ctypes and numpy, and null arguments answer as documented.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import qpsk_amd as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = [
    "qpsk_link_stats_size", "qpsk_demod_enable_link_stats", "qpsk_demod_link_stats",
    "qpsk_demod_group_enable_link_stats", "qpsk_demod_group_link_stats",
]
# the header's struct, in order: (name, C type, numpy type, offset)
FIELDS = [
    ("n_symbols", "int64_t", "i8", 0), ("sum_dist2", "double", "f8", 8), ("sum_power", "double", "f8", 16),
    ("costas_freq", "double", "f8", 24), ("costas_theta", "double", "f8", 32), ("mm_mu", "double", "f8", 40),
    ("mm_rate", "double", "f8", 48), ("fll_freq", "float", "f4", 56), ("error", "int32_t", "i4", 60),
]


def header_text():
    with open(os.path.join(ROOT, "include", "qpsk_demod.h")) as f:
        return f.read()


def test_header_declares_the_struct_and_the_entry_points():
    text = header_text()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"typedef\s+struct\s+qpsk_link_stats\s*\{(.*?)\}\s*qpsk_link_stats\s*;", src, flags=re.S).group(1)
    members = [tuple(m.split()) for m in body.split(";") if m.strip()]
    assert members == [(ctype, name) for name, ctype, _, _ in FIELDS]
    for n in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + n + r"\s*\(", src), n
    decl = lambda n: " ".join(re.search(n + r"\s*\(([^;]*)\)\s*;", src).group(1).split())
    assert decl("qpsk_link_stats_size") == "void"
    assert decl("qpsk_demod_enable_link_stats") == "qpsk_demod *h, int32_t on"
    assert decl("qpsk_demod_link_stats") == "qpsk_demod *h, qpsk_link_stats *out, int32_t mem, int32_t reset"
    assert decl("qpsk_demod_group_enable_link_stats") == "qpsk_demod_group *g, int32_t on"
    assert decl("qpsk_demod_group_link_stats") == "qpsk_demod_group *g, qpsk_link_stats *out_host, int32_t reset"
    assert re.search(r"#define\s+QPSK_ABI_VERSION\s+3\b", text), "additive only: the ABI version stays"
    # what the header promises about the sums
    block = text[text.index("Per-stream link statistics"): text.index("int qpsk_demod_link_stats(")]
    for phrase in ("QPSKDeModulator.cs:381-384", "CostasLoopQpsk.cs:127-130", "qpsk_demod_set_state leaves the sums alone",
                   "qpsk_rx ring", "no fused multiply-add"):
        assert phrase in block, phrase


def test_library_exports_them_and_the_binding_lists_them():
    out = subprocess.check_output(["nm", "-D", "--defined-only", Q.LIB_PATH]).decode()
    L = Q.lib()
    for n in ENTRY_POINTS:
        assert re.search(r"\bT " + n + r"\b", out), n
        assert hasattr(L, n), n
        assert n in Q.EXPORTED_SYMBOLS, n
    for m in ("enable_link_stats", "link_stats", "link_stats_device"):
        assert callable(getattr(Q.BatchDemodulator, m)), m
    for m in ("enable_link_stats", "link_stats"):
        assert callable(getattr(Q.DemodGroup, m)), m
    assert L.qpsk_abi_version() == 3


def test_one_row_layout_everywhere():
    assert Q.lib().qpsk_link_stats_size() == 64 == Q.LINK_STATS_DTYPE.itemsize == C.sizeof(Q.LinkStats)
    assert Q.link_stats_size() == 64
    assert list(Q.LINK_STATS_DTYPE.names) == [f[0] for f in FIELDS] == [f[0] for f in Q.LinkStats._fields_]
    for name, _, npt, off in FIELDS:
        assert Q.LINK_STATS_DTYPE.fields[name][1] == off, name
        assert Q.LINK_STATS_DTYPE.fields[name][0] == np.dtype(npt), name
        assert getattr(Q.LinkStats, name).offset == off, name
    assert [f[3] for f in FIELDS] == [0, 8, 16, 24, 32, 40, 48, 56, 60]


def test_null_arguments_are_argument_null():
    L = Q.lib()
    rows = np.zeros(4, Q.LINK_STATS_DTYPE)
    assert L.qpsk_demod_enable_link_stats(None, 1) == Q.QPSK_ERR_ARGUMENT_NULL
    assert L.qpsk_demod_group_enable_link_stats(None, 1) == Q.QPSK_ERR_ARGUMENT_NULL
    for mem in (Q.MEM_HOST, Q.MEM_DEVICE):
        for reset in (0, 1):
            assert L.qpsk_demod_link_stats(None, rows.ctypes.data, mem, reset) == Q.QPSK_ERR_ARGUMENT_NULL
    assert L.qpsk_demod_group_link_stats(None, rows.ctypes.data, 0) == Q.QPSK_ERR_ARGUMENT_NULL
    # a null out with a handle in hand needs a device to make the handle: tests/test_gpu_link_stats.py
    assert L.qpsk_demod_link_stats(None, None, Q.MEM_HOST, 0) == Q.QPSK_ERR_ARGUMENT_NULL
    assert L.qpsk_demod_group_link_stats(None, None, 0) == Q.QPSK_ERR_ARGUMENT_NULL
    assert b"null" in L.qpsk_last_error()
