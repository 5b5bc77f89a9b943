"""Every per-call argument rule, through every entry point that takes a call.

One rule set guards qpsk_demod_process, qpsk_demod_process_async, their CS16
twins, the host ring's submits and the group call (include/qpsk_demod.h: "a bad
argument fails the call before any shard's state moves").  Each row below makes
one argument bad and names the status and the exact qpsk_last_error text; the
calls go through the raw C entry points, so the binding's own checks stay out
of the way.  Every row must fail in the check, before any launch or copy: the
pointers are small host buffers whatever `mem` says, and afterwards every
handle's state blob is what it was and a valid call still gives the oracle's
bits and symbols.

The ring answers a chunk above its slot length (at most 2^30 samples) before
the 2^31 - 129 sample limit can, so that rule reads "chunk longer ..." there.
"""
import ctypes as C

import numpy as np
import pytest

import common as K
import qpsk_amd as Q
from gpu_harness import dev

pytestmark = pytest.mark.gpu

S, SPS, SPAN, N = 4, 8, 8, 64
ARG, NULL, RANGE, STATE = Q.QPSK_ERR_ARGUMENT, Q.QPSK_ERR_ARGUMENT_NULL, Q.QPSK_ERR_OUT_OF_RANGE, Q.QPSK_ERR_STATE
LIMIT = "calls above 2^31 - 129 samples per stream (a C# span holds 2^30)"
BITS_STRIDE = "bits_stride_bytes smaller than 2*max_symbols/8"
SYMS_STRIDE = "syms_stride_floats smaller than 2*max_symbols"
WRONG_FORMAT = "the ring was created for the other sample format (CF32 / CS16)"
TOO_LONG = "chunk longer than the ring slots (max_samples_per_call)"
SLOT_STRIDE = "a ring slot has a stride of 2 * max_samples_per_call elements"
RING_FULL = "every ring slot holds an uncollected chunk"

HANDLE_ENTRIES = ("process", "process_cs16", "process_async", "process_async_cs16")
CALL_ENTRIES = HANDLE_ENTRIES + ("group",)
RING_ENTRIES = ("rx_submit", "rx_submit_cs16")
CS16 = ("process_cs16", "process_async_cs16", "rx_submit_cs16")
ASYNC = ("process_async", "process_async_cs16")


def _rows():
    rows = []

    def add(entry, what, rc, text, **bad):
        rows.append(pytest.param(entry, bad, rc, text, id=f"{entry}-{what}"))

    for e in CALL_ENTRIES:
        add(e, "null_handle", NULL, "null group" if e == "group" else "null handle", handle=None)
        add(e, "mode", ARG, "unknown mode", mode=7)
        if e not in ASYNC:
            add(e, "mem", ARG, "unknown mem", mem=5)
        add(e, "negative_length", ARG, "negative length", lengths=[N, -1, N, N])
        add(e, "negative_n", ARG, "negative n_samples", n=-1)
        if e == "group":
            # the shard that a build without the group's own limit check still
            # runs gets an empty call; row and bit strides past every other check
            add(e, "limit", RANGE, LIMIT, lengths=[0, 0, 0, 1 << 31], stride=1 << 33, bstride=1 << 40)
        else:
            add(e, "limit_n", RANGE, LIMIT, n=(1 << 31) - 128)
            add(e, "limit_lengths", RANGE, LIMIT, lengths=[0, 0, 0, 1 << 31])
        add(e, "null_iq", NULL, "SamplesIQ is null", iq=None)
        add(e, "stride", ARG, "stride too small", stride=2 * N - 2)
        add(e, "no_bits", NULL, "bits / n_bits required", bits=None)
        add(e, "no_n_bits", NULL, "bits / n_bits required", n_bits=None)
        add(e, "no_syms", NULL, "syms / n_syms required", mode=Q.MODE_CONSTELLATION)
        add(e, "no_n_syms", NULL, "syms / n_syms required", mode=Q.MODE_CONSTELLATION, syms="buf", sstride=96)
        add(e, "bits_stride", ARG, BITS_STRIDE, bstride="short")
        add(e, "syms_stride", ARG, SYMS_STRIDE, syms="buf", n_syms="buf", sstride="short")
        add(e, "odd_device_stride", ARG,
            "device stride_i16 must be even" if e in CS16 else "device stride_floats must be even",
            mem=Q.MEM_DEVICE, stride=2 * N + 1)
        if e in CS16:
            add(e, "cs16_alignment", ARG, "device CS16 rows must be 4-byte aligned", mem=Q.MEM_DEVICE, iq="odd")
    for e in RING_ENTRIES:
        add(e, "null_ring", NULL, "null ring", handle=None)
        add(e, "wrong_format", STATE, WRONG_FORMAT, handle="other")
        add(e, "negative_length", ARG, "negative length", lengths=[N, -1, N, N])
        add(e, "negative_n", ARG, "negative n_samples", n=-1)
        add(e, "too_long", ARG, TOO_LONG, n=N + 1, stride=2 * N + 2)
        add(e, "too_long_lengths", ARG, TOO_LONG, lengths=[N, N, N + 1, N], stride=2 * N + 2)
        add(e, "limit", ARG, TOO_LONG, n=(1 << 31) - 128, stride=1 << 33)
        add(e, "null_iq", NULL, "SamplesIQ is null", iq=None)
        add(e, "stride", ARG, "stride too small", stride=2 * N - 2)
        add(e, "slot_stride", ARG, SLOT_STRIDE, iq="slot", stride=2 * N + 2)
    return rows


class Env:
    def __init__(self):
        self.L = Q.lib()
        p = Q.params(K.FS, K.FS // SPS, K.ALPHA, SPAN, max_samples_per_call=N)
        self.one = Q.BatchDemodulator(S, p)
        self.grp = Q.DemodGroup(S, p, [0, 0])
        self.ring_demods = {e: Q.BatchDemodulator(S, p) for e in RING_ENTRIES}
        self.rings = {"rx_submit": Q.HostRing(self.ring_demods["rx_submit"], depth=2),
                      "rx_submit_cs16": Q.HostRing(self.ring_demods["rx_submit_cs16"], depth=2, fmt="cs16")}
        self.max_sym = self.one.max_symbols(N)
        # dummy rows: never read or written by a rejected call
        self.iq = np.zeros((S, 2 * N + 8), np.float32)
        self.bits = np.zeros((S, 64), np.uint8)
        self.syms = np.zeros((S, 2 * self.max_sym + 8), np.float32)
        self.n_bits = np.zeros(S, np.int64)
        self.n_syms = np.zeros(S, np.int64)
        self.before = self.states()

    def states(self):
        return ([self.one.get_state()] + [self.grp.get_state(k) for k in range(2)] +
                [d.get_state() for d in self.ring_demods.values()])

    def call(self, entry, bad):
        """(status, qpsk_last_error text) of one valid call with `bad` overriding its arguments."""
        L = self.L
        a = dict(handle="own", mode=Q.MODE_DEMODULATE, iq="buf", stride=2 * N, n=N, lengths=None, mem=Q.MEM_HOST,
                 bits="buf", bstride=(2 * self.max_sym + 7) // 8, n_bits="buf", syms=None, sstride=0, n_syms=None)
        a.update(bad)
        if a["bstride"] == "short":
            a["bstride"] = (2 * self.max_sym + 7) // 8 - 1
        if a["sstride"] == "short":
            a["sstride"] = 2 * self.max_sym - 1
        lens = None if a["lengths"] is None else (C.c_int64 * S)(*a["lengths"])
        ring = entry in RING_ENTRIES
        if a["handle"] is None:
            h = None
        elif ring:
            h = self.rings[entry if a["handle"] == "own" else RING_ENTRIES[1 - RING_ENTRIES.index(entry)]]._r
        else:
            h = self.grp._g if entry == "group" else self.one._h
        if a["iq"] == "slot":
            slot, stride = C.c_void_p(), C.c_int64()
            next_slot = L.qpsk_rx_next_slot_cs16 if entry in CS16 else L.qpsk_rx_next_slot
            assert next_slot(h, C.byref(slot), C.byref(stride)) == 0 and stride.value == 2 * N
            iq = slot.value
        else:
            iq = {None: None, "buf": self.iq.ctypes.data, "odd": self.iq.ctypes.data + 2}[a["iq"]]
        if ring:
            rc = getattr(L, "qpsk_" + entry)(h, iq, a["stride"], a["n"], lens, None)
        else:
            ptr = lambda v, buf: buf.ctypes.data if v == "buf" else None   # noqa: E731
            head = (h, a["mode"], iq, a["stride"], a["n"], lens)
            tail = (ptr(a["bits"], self.bits), a["bstride"], ptr(a["n_bits"], self.n_bits),
                    ptr(a["syms"], self.syms), a["sstride"], ptr(a["n_syms"], self.n_syms))
            fn = L.qpsk_demod_group_process if entry == "group" else getattr(L, "qpsk_demod_" + entry)
            rc = fn(*head, *tail) if entry in ASYNC else fn(*head, a["mem"], *tail)
        return rc, L.qpsk_last_error().decode()

    def close(self):
        for r in self.rings.values():
            r.close()
        for d in self.ring_demods.values():
            d.close()
        self.grp.close()
        self.one.close()


@pytest.fixture(scope="module")
def env(dev):
    e = Env()
    yield e
    e.close()


@pytest.mark.parametrize("entry,bad,rc,text", _rows())
def test_bad_argument_is_rejected_with_its_status_and_text(env, entry, bad, rc, text):
    got = env.call(entry, bad)
    print(f"{entry} {bad}: {got}")
    assert got == (rc, text)


def test_rejected_calls_left_every_state_blob_as_it_was(env):
    names = ["handle", "shard 0", "shard 1", "CF32 ring's handle", "CS16 ring's handle"]
    moved = [n for n, a, b in zip(names, env.before, env.states()) if a != b]
    assert not moved, f"state moved: {moved}"


def test_valid_call_after_the_rejections_matches_the_oracle(env):
    iq = K.batch_signals(S, seed0=70, sps=SPS, span=SPAN, n_bits=200, snr_db=18)[:, : 2 * N]
    bits, nb, syms, ns = env.one.process(iq, want_syms=True)
    for s in range(S):
        ob, osy, _ = K.oracle_for(SPS, SPAN).demodulate_ex(iq[s])
        assert Q.unpack_bits(bits[s], int(nb[s])) == ob, s
        assert K.bitwise_equal(syms[s, : 2 * int(ns[s])], osy), s


@pytest.mark.parametrize("entry", RING_ENTRIES)
def test_full_ring_rejects_a_submit_and_keeps_its_chunks(env, entry):
    ring = env.rings[entry]
    # the rejected submits above took no slot: the first tickets are 0 and 1
    assert [ring.submit(n=0), ring.submit(n=0)] == [0, 1]
    assert env.call(entry, {}) == (STATE, RING_FULL)
    for t in (0, 1):
        _, nb, ticket = ring.collect()
        assert ticket == t and not nb.any()
