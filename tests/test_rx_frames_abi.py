"""Frames on the device at the drop-in boundary (no GPU): the header declares
the new entry points with the documented arguments, libqpsk_demod.so exports
them, the binding lists them, and each returns QPSK_ERR_ARGUMENT_NULL on null
handles and pointers before any device call.  The packing rule the GPU tests
compare against (frame_cases.pack_rule) is pinned on hand-worked cases.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import qpsk_amd as Q
from frame_cases import pack_rule, packed_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = ["qpsk_frames_pack_device", "qpsk_framer_dev_reset_streams", "qpsk_rx_attach_framer",
                "qpsk_rx_set_markers", "qpsk_rx_frames_bytes", "qpsk_rx_collect_frames", "qpsk_rx_reset_streams"]


def test_header_declares_every_entry_point():
    with open(os.path.join(ROOT, "include", "qpsk_demod.h")) as f:
        text = f.read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = lambda n: " ".join(re.search(r"\b" + n + r"\s*\(([^;]*)\)\s*;", src).group(1).split())   # noqa: E731
    for n in ENTRY_POINTS:
        kind = "int64_t" if n.endswith("_bytes") else "int"
        assert re.search(r"\b" + kind + r"\s+" + n + r"\s*\(", src), n
    assert decl("qpsk_frames_pack_device") == (
        "const uint8_t *payload, int64_t payload_stride, const int64_t *n_payload, int32_t n_streams, "
        "uint8_t *packed, int64_t packed_cap, int64_t *offsets, int64_t *head, void *hip_stream")
    assert decl("qpsk_framer_dev_reset_streams") == "qpsk_framer_dev *f, const int32_t *streams, int32_t n"
    assert decl("qpsk_rx_attach_framer") == (
        "qpsk_rx *r, const uint8_t *start, int32_t n_start, const uint8_t *end, int32_t n_end, const char *tsc, "
        "int64_t ring_capacity, int64_t max_frame_bytes, int64_t chunk_frame_bytes, int32_t keep_bits")
    assert decl("qpsk_rx_set_markers") == ("qpsk_rx *r, const uint8_t *start, int32_t n_start, const uint8_t *end, "
                                           "int32_t n_end")
    assert decl("qpsk_rx_frames_bytes") == "const qpsk_rx *r"
    assert decl("qpsk_rx_collect_frames") == (
        "qpsk_rx *r, uint8_t *frames, int64_t frames_cap, int64_t *frame_offset, int64_t *frame_len, uint8_t *bits, "
        "int64_t bits_stride_bytes, int64_t *n_bits, int64_t *ticket")
    assert decl("qpsk_rx_reset_streams") == "qpsk_rx *r, const int32_t *streams, int32_t n"
    assert re.search(r"#define\s+QPSK_ABI_VERSION\s+3\b", text), "additive only: the ABI version stays"
    assert re.search(r"#define\s+QPSK_FRAMES_TRUNCATED\s+1\b", text) and re.search(r"#define\s+QPSK_FRAMES_DROPPED\s+2\b", text)
    block = text[text.index("Frames on the device"): text.index("int qpsk_rx_reset_streams(")]
    for phrase in ("QPSKDeModulator.cs:169-259", ":412-422", "ModDemodOverSDR.cs:136", "rounded up to 16",
                   "QPSK_ERR_CAPACITY", "the chunk stays outstanding", "neither waits nor fetches"):
        assert phrase in block, phrase


def test_library_exports_them_and_the_binding_lists_them():
    out = subprocess.check_output(["nm", "-D", "--defined-only", Q.LIB_PATH]).decode()
    L = Q.lib()
    for n in ENTRY_POINTS:
        assert re.search(r"\bT " + n + r"\b", out), n
        assert hasattr(L, n), n
        assert n in Q.EXPORTED_SYMBOLS, n
    for m in ("attach_framer", "set_markers", "collect_frames", "reset_streams", "frames_bytes"):
        assert callable(getattr(Q.HostRing, m)), m
    assert callable(Q.DeviceFramer.reset_streams) and callable(Q.frames_pack_device)
    assert (Q.FRAMES_TRUNCATED, Q.FRAMES_DROPPED) == (1, 2)
    assert L.qpsk_abi_version() == 3
    assert len(set(Q.EXPORTED_SYMBOLS)) == len(Q.EXPORTED_SYMBOLS)


def test_null_arguments_are_argument_null():
    """Host buffers stand in for the device pointers: a call that is refused for
    a null argument returns before it looks at any of them."""
    L = Q.lib()
    NULL = Q.QPSK_ERR_ARGUMENT_NULL
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data
    ids = (C.c_int32 * 1)(0)
    m = (C.c_uint8 * 2)(2, 3)
    good = [p, 16, p, 1, p, 16, p, p, None]
    for k in (0, 2, 4, 6, 7):                       # payload, n_payload, packed (cap > 0), offsets, head
        args = list(good)
        args[k] = None
        assert L.qpsk_frames_pack_device(*args) == NULL, k
        assert b"null" in L.qpsk_last_error()
    assert not buf.any(), "a refused call wrote"
    assert L.qpsk_framer_dev_reset_streams(None, ids, 1) == NULL
    assert L.qpsk_framer_dev_reset_streams(None, None, 0) == NULL
    assert L.qpsk_rx_attach_framer(None, m, 1, m, 1, None, 64, 64, 0, 0) == NULL
    assert L.qpsk_rx_set_markers(None, m, 1, m, 1) == NULL
    assert L.qpsk_rx_frames_bytes(None) == 0
    u8 = buf.ctypes.data_as(C.POINTER(C.c_uint8))
    i64 = buf.ctypes.data_as(C.POINTER(C.c_int64))
    assert L.qpsk_rx_collect_frames(None, u8, 64, i64, i64, None, 0, None, None) == NULL
    assert L.qpsk_rx_reset_streams(None, ids, 1) == NULL
    assert L.qpsk_rx_reset_streams(None, None, 0) == NULL
    assert b"null" in L.qpsk_last_error()


def test_bad_pack_arguments_are_refused_on_the_host():
    """Strides, capacities and alignment are checked before anything is launched."""
    L = Q.lib()
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data
    assert p % 16 == 0 or (p + 8) % 16 == 0
    p16 = p if p % 16 == 0 else p + 8
    for args in ([p16, 0, p, 1, p16, 16, p, p, None], [p16, 24, p, 1, p16, 16, p, p, None],
                 [p16, -16, p, 1, p16, 16, p, p, None], [p16, 16, p, 1, p16, 8, p, p, None],
                 [p16, 16, p, 1, p16, -16, p, p, None], [p16, 16, p, 1, p16 + 8, 16, p, p, None],
                 [p16, 16, p, 1, p16, 16, p + 4, p, None], [p16, 16, p, 1, p16, 16, p, p + 4, None],
                 [p16, 16, p, 0, p16, 16, p, p, None]):
        assert L.qpsk_frames_pack_device(*args) == Q.QPSK_ERR_ARGUMENT, args
    assert not buf.any()


def test_pack_rule_on_hand_worked_cases():
    # P = 16: lengths 0, 1, 16, 17 (truncated), 80 (truncated) -> one word each
    k, a, off, total, flags = pack_rule([0, 1, 16, 17, 80], 16, 1 << 20)
    assert (list(k), list(a), list(off), total, flags) == ([0, 1, 16, 16, 16], [0, 16, 16, 16, 16],
                                                           [-1, 0, 16, 32, 48], 64, 1)
    # P = 48, C = 64: 17 -> 32 bytes at 0; 40 -> 48 bytes would end at 80 > 64; the 1 behind it starts at 80
    k, a, off, total, flags = pack_rule([17, 0, 40, 1], 48, 64)
    assert (list(a), list(off), total, flags) == ([32, 0, 48, 16], [0, -1, -1, -1], 32, 2)
    o0, o64 = pack_rule([0, 0], 16, 0), pack_rule([0, 0], 16, 64)
    assert list(o0[2]) == list(o64[2]) == [-1, -1] and o0[3:] == o64[3:] == (0, 0)
    assert pack_rule([5], 16, 0)[3:] == (0, 2)
    rows = np.full((4, 48), 0xAA, np.uint8)
    rows[0, :17] = np.arange(1, 18)
    got = packed_bytes(rows, [17, 0, 40, 1], 48, 64)
    assert got.size == 32 and list(got[:17]) == list(range(1, 18)) and not got[17:].any()
