"""The channel's C ABI without a GPU: the declarations and exports, the
parameter defaults, the state size, qpsk_channel_state_check on records built
in numpy at and just past every range edge, the argument checks that come
before a device is touched, and the pure-Python oscillator the GPU tests read
state fields from, held to the oracle's sample for sample."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import channel_cases as CC
import oracle as O
import qpsk_amd as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["qpsk_channel_params_init", "qpsk_channel_create", "qpsk_channel_destroy", "qpsk_channel_set_stream",
           "qpsk_channel_apply_fmt", "qpsk_channel_state_size", "qpsk_channel_get_state", "qpsk_channel_set_state",
           "qpsk_channel_reset_streams", "qpsk_channel_state_check"]
FS = 8000.0
TWO_PI = 2.0 * math.pi


def test_header_declares_and_library_exports_the_entries():
    src = open(os.path.join(ROOT, "include", "qpsk_demod.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", Q.LIB_PATH]).decode()
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert re.search(r"\bT " + name + r"\b", nm), name
        assert name in Q.EXPORTED_SYMBOLS
    assert re.search(r"#define\s+QPSK_ABI_VERSION\s+3\b", src)
    assert Q.lib().qpsk_abi_version() == 3


def test_params_init_defaults_and_state_size():
    p = Q.ChannelParams()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    Q.lib().qpsk_channel_params_init(C.byref(p), 10e6)
    assert (p.sample_rate, p.lo_hz, p.tx_ppm, p.rx_ppm) == (10e6, 100e6, 1.0, 1.0)
    assert (p.tx_phase0, p.rx_phase0, p.noise_rms) == (0.0, 0.0, 0.0)
    assert (p.tx_seed, p.rx_seed, p.noise_seed, p.first_stream, p.device) == (1000, 2000, 0, 0, 0)
    assert list(p.reserved) == [0] * 7
    assert C.sizeof(p) == 120
    assert Q.channel_state_size() == 128 == Q.CHANNEL_STATE_DTYPE.itemsize
    assert Q.lib().qpsk_channel_state_size() == 128


@pytest.mark.parametrize("seed", [1, 5, 1000, 2 ** 64 - 3])
@pytest.mark.parametrize("fs,lo,ppm,phase0", [(8000.0, 100e6, 1.0, 0.0), (1000.0, -100e6, 5.0, -7.5),
                                              (10e6, 100e6, 0.0, 1.25), (10e6, 935e6, 20.0, 120.0)])
def test_python_nco_equals_the_oracle(seed, fs, lo, ppm, phase0):
    a, b = CC.PyNCO(lo, fs, ppm, phase0, seed=seed), O.OracleNCO(lo, fs, ppm, phase0, seed=seed)
    n = 3 * a.interval + 50 if a.interval < 2000 else a.interval + 50
    for i in range(n):
        za, zb = a.next(), b.next()
        assert (za.real.hex(), za.imag.hex()) == (zb.real.hex(), zb.imag.hex()), i


def fresh(p, S):
    """The records qpsk_channel_create gives S streams, from the Python oscillator."""
    st = np.zeros(S, Q.CHANNEL_STATE_DTYPE)
    for s in range(S):
        g = p.first_stream + s
        for osc, ppm, ph, seed in (("tx", p.tx_ppm, p.tx_phase0, p.tx_seed), ("rx", p.rx_ppm, p.rx_phase0, p.rx_seed)):
            st[osc][s] = CC.PyNCO(p.lo_hz, p.sample_rate, ppm, ph, seed=seed + g).fields()
    return st


def check(p, st):
    return Q.lib().qpsk_channel_state_check(C.byref(p), st.size, st.tobytes(), st.nbytes)


def last_error():
    return Q.lib().qpsk_last_error().decode()


def with_total(rec, p, osc, total):
    """rec's oscillator moved to total_ppm = total, consistently."""
    rec[osc]["total_ppm"] = total
    rec[osc]["drift_ppm"] = total - rec[osc]["static_ppm"]
    rec[osc]["cur_hz"] = p.lo_hz * (1.0 + total * 1e-6)


def test_state_check_accepts_fresh_and_stepped_states():
    p = Q.channel_params(FS, tx_ppm=2.0, rx_ppm=1.0)
    st = fresh(p, 3)
    assert check(p, st) == 0, last_error()
    # after 100 samples, drift updates included
    n = CC.PyNCO(p.lo_hz, FS, 2.0, 0.0, seed=p.tx_seed)
    for _ in range(100):
        n.next()
    st["tx"][0] = n.fields()
    st["pos"][0] = 100
    assert check(p, st) == 0, last_error()
    Q.channel_state_check(p, 3, st.tobytes())


EDGE = np.nextafter
ACCEPT = [
    ("tx", "phase", 0.0), ("rx", "phase", TWO_PI), ("tx", "phase", EDGE(TWO_PI, 0.0)),
    ("tx", "phase", -0.0), ("tx", "counter", 0), ("rx", "counter", 7),
]
REJECT = [
    ("tx", "phase", EDGE(TWO_PI, 10.0)), ("rx", "phase", -EDGE(0.0, 1.0)),
    ("tx", "phase", float("nan")), ("rx", "phase", float("inf")),
    ("tx", "counter", -1), ("rx", "counter", 8),
    ("tx", "static_ppm", float("nan")), ("rx", "drift_ppm", float("inf")), ("tx", "total_ppm", float("nan")),
    ("rx", "cur_hz", float("-inf")),
    ("tx", "cur_hz", EDGE(100e6, 0.0)),
]


@pytest.mark.parametrize("osc,field,value", ACCEPT)
def test_state_check_accepts_range_edges(osc, field, value):
    p = Q.channel_params(FS)                       # interval 8
    st = fresh(p, 2)
    st[osc][field][1] = value
    assert check(p, st) == 0, last_error()


@pytest.mark.parametrize("osc,field,value", REJECT)
def test_state_check_rejects_past_range_edges(osc, field, value):
    p = Q.channel_params(FS)
    st = fresh(p, 2)
    st[osc][field][1] = value
    assert check(p, st) == Q.QPSK_ERR_ARGUMENT
    msg = last_error()
    assert "stream 1" in msg and osc + "." + field in msg, msg
    with pytest.raises(ValueError, match=field):
        Q.channel_state_check(p, 2, st.tobytes())


@pytest.mark.parametrize("osc,ppm", [("tx", 2.0), ("rx", 1.0)])
def test_state_check_total_ppm_edges(osc, ppm):
    p = Q.channel_params(FS, tx_ppm=2.0, rx_ppm=-1.0)   # the sign of ppm is dropped
    for total in (ppm, -ppm):
        st = fresh(p, 1)
        with_total(st[0], p, osc, total)
        assert check(p, st) == 0, last_error()
        with_total(st[0], p, osc, float(EDGE(total, 10 * total)))
        assert check(p, st) == Q.QPSK_ERR_ARGUMENT
        assert osc + ".total_ppm" in last_error() and "stream 0" in last_error()
    st = fresh(p, 1)
    st[osc]["static_ppm"][0] = EDGE(ppm, 10.0)
    assert check(p, st) == Q.QPSK_ERR_ARGUMENT and osc + ".static_ppm" in last_error()
    # total = static + drift: the clamp's two roundings pass, a drift that is off does not
    st = fresh(p, 1)
    st[osc]["drift_ppm"][0] = 1e-9 * ppm
    assert check(p, st) == Q.QPSK_ERR_ARGUMENT and osc + ".drift_ppm" in last_error()
    st = fresh(p, 1)
    st[osc]["drift_ppm"][0] = 2.0 ** -52 * ppm
    assert check(p, st) == 0, last_error()


def test_state_check_ideal_oscillator_and_pos():
    p = Q.channel_params(FS, tx_ppm=0.0, rx_ppm=5.0)
    st = fresh(p, 2)
    assert st["tx"]["static_ppm"][0] == 0.0 and st["tx"]["cur_hz"][0] == 100e6 and st["tx"]["rng"][0] == p.tx_seed
    assert check(p, st) == 0, last_error()
    st["tx"]["total_ppm"][1] = EDGE(0.0, 1.0)
    assert check(p, st) == Q.QPSK_ERR_ARGUMENT and "tx.total_ppm" in last_error()
    st = fresh(p, 2)
    st["pos"][1] = 2 ** 62
    assert check(p, st) == 0, last_error()
    st["pos"][1] = -1
    assert check(p, st) == Q.QPSK_ERR_ARGUMENT and "stream 1: pos" in last_error()
    st = fresh(p, 2)
    st["reserved"][0] = 1
    assert check(p, st) == Q.QPSK_ERR_ARGUMENT and "stream 0: reserved" in last_error()


def test_state_check_sizes_and_nulls():
    p = Q.channel_params(FS)
    st = fresh(p, 2)
    L = Q.lib()
    assert L.qpsk_channel_state_check(C.byref(p), 2, st.tobytes(), st.nbytes - 1) == Q.QPSK_ERR_ARGUMENT
    assert "length" in last_error()
    assert L.qpsk_channel_state_check(C.byref(p), 3, st.tobytes(), st.nbytes) == Q.QPSK_ERR_ARGUMENT
    assert L.qpsk_channel_state_check(C.byref(p), 2, None, st.nbytes) == Q.QPSK_ERR_ARGUMENT_NULL
    assert L.qpsk_channel_state_check(None, 2, st.tobytes(), st.nbytes) == Q.QPSK_ERR_ARGUMENT_NULL
    assert L.qpsk_channel_state_check(C.byref(p), 0, st.tobytes(), 0) == Q.QPSK_ERR_ARGUMENT


@pytest.mark.parametrize("field,value", [("sample_rate", 0.0), ("sample_rate", float("nan")), ("lo_hz", float("inf")),
                                         ("tx_ppm", float("nan")), ("rx_phase0", float("inf")), ("noise_rms", -1.0),
                                         ("noise_rms", float("nan")), ("first_stream", -1)])
def test_create_rejects_bad_params_before_touching_a_device(field, value):
    p = Q.channel_params(FS)
    setattr(p, field, value)
    h = C.c_void_p()
    assert Q.lib().qpsk_channel_create(C.byref(p), 4, C.byref(h)) == Q.QPSK_ERR_OUT_OF_RANGE
    assert field in last_error() and not h.value
    assert Q.lib().qpsk_channel_create(C.byref(Q.channel_params(FS)), 0, C.byref(h)) == Q.QPSK_ERR_ARGUMENT


def test_seed_scan_finds_static_errors_at_both_ends():
    hi, lo = CC.seed_near(+1), CC.seed_near(-1)
    assert CC.PyNCO(100e6, 1000.0, 1.0, seed=hi).static_ppm >= 1.0 - 0.0005
    assert CC.PyNCO(100e6, 1000.0, 1.0, seed=lo).static_ppm <= -1.0 + 0.0005
