"""What the path tests share (tests/test_path_abi.py, tests/test_gpu_path.py):
the yardstick of the propagation path (include/qpsk_demod.h, "The propagation
path on the device").  Needs no GPU and no library.

path_reference    the definition as numpy array operations on np.float32 /
                  np.float64: numpy fuses nothing, so every operation rounds
                  once, in the order the definition writes them.
py_count          the emit count in Python ints and float64, by its predicate.
PyPath            one stream's state over a call sequence, pure Python.
"""
import math

import numpy as np

from channel_cases import splitmix64, u01

f32, f64 = np.float32, np.float64
MAX_TAPS, HIST, TILE = 8, 16, 1024
R_MIN, R_MAX = 1.0 + -1000.0 * 1e-6, 1.0 + 1000.0 * 1e-6
IDENTITY = np.array([[1.0, 0.0]], f32)


def project_taps():
    """[1, .25 e^{j.7}, .1 e^{-j1.9}, .05] formed in double and rounded to float once, as [4, 2]."""
    mr = [1.0, 0.25 * math.cos(0.7), 0.1 * math.cos(-1.9), 0.05]
    mi = [0.0, 0.25 * math.sin(0.7), 0.1 * math.sin(-1.9), 0.0]
    return np.array([mr, mi], f64).T.astype(f32)


def clock(g, clock_ppm=0.0, clock_spread=0.0, clock_seed=3000, tau0=0.0, tau_random=False):
    """(r, tau) of global stream g."""
    st, z1 = splitmix64((clock_seed + g) & ((1 << 64) - 1))
    st, z2 = splitmix64(st)
    u1, u2 = u01(z1), u01(z2)
    ppm = clock_ppm + ((u1 * 2.0 - 1.0) * clock_spread if clock_spread > 0 else 0.0)
    r = 1.0 + ppm * 1e-6
    return min(max(r, R_MIN), R_MAX), (u2 if tau_random else tau0)


def p_of(r, tau, k):
    """p_k = tau + (double)k * r: Python floats are doubles, each operation rounds once."""
    return tau + float(k) * r


def py_emitted(r, tau, in_end):
    """How many k >= 0 have floor(p_k) <= in_end - 3.  p_k does not decrease in
    k, so a bisection on the predicate itself finds the count: no division."""
    if math.floor(p_of(r, tau, 0)) > in_end - 3:
        return 0
    lo, hi = 0, 2 * in_end + 4            # lo emits; hi does not (r > 0.5)
    assert math.floor(p_of(r, tau, hi)) > in_end - 3
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if math.floor(p_of(r, tau, mid)) <= in_end - 3:
            lo = mid
        else:
            hi = mid
    return hi


def py_count(r, tau, out_pos, in_end):
    return max(0, py_emitted(r, tau, in_end) - out_pos)


def py_out_bound(n_in, clock_ppm=0.0, clock_spread=0.0):
    return int(math.ceil(float(n_in) / (1.0 - (abs(clock_ppm) + clock_spread) * 1e-6))) + 2


def multipath(x, taps):
    """z over a whole stream: x [2 n] float32 interleaved from index 0 (zeros
    before it), taps [L, 2] float32.  Returns (z.re, z.im), float32 [n]."""
    x = np.asarray(x, f32)
    taps = np.asarray(taps, f32)
    n, L = x.size // 2, taps.shape[0]
    xr = np.concatenate([np.zeros(L - 1, f32), x[0::2]])
    xi = np.concatenate([np.zeros(L - 1, f32), x[1::2]])
    zr, zi = np.zeros(n, f32), np.zeros(n, f32)
    with np.errstate(all="ignore"):
        for j in range(L):
            dr, di = xr[L - 1 - j: L - 1 - j + n], xi[L - 1 - j: L - 1 - j + n]     # x[i - j]
            hr, hi = taps[j, 0], taps[j, 1]
            zr = zr + (hr * dr - hi * di)
            zi = zi + (hr * di + hi * dr)
    assert zr.dtype == f32 and zi.dtype == f32
    return zr, zi


def path_reference(x, r, tau, taps, k0=0, in0=0):
    """Every output the stream can emit from inputs x [2 n] float32 (absolute
    indices in0 .. in0 + n - 1, zeros before them) from output k0 on:
    interleaved float32 [2 (count - k0)]."""
    n = np.asarray(x).size // 2
    zr, zi = multipath(x, taps)
    count = py_emitted(r, tau, in0 + n)
    k = np.arange(k0, count, dtype=np.int64)
    p = f64(tau) + k.astype(f64) * f64(r)
    nf = np.floor(p)
    t = (p - nf).astype(f32)
    ni = nf.astype(np.int64) - in0
    one, two = f32(1), f32(2)
    tm1, tm2, tp1 = t - one, t - two, t + one
    c_m1 = -(t * tm1 * tm2) * (one / f32(6))
    c_0 = (tp1 * tm1 * tm2) * (one / two)
    c_1 = -(tp1 * t * tm2) * (one / two)
    c_2 = (tp1 * t * tm1) * (one / f32(6))

    def at(z, i):        # z[i], +0 before the row
        return np.where(i >= 0, z[np.maximum(i, 0)], f32(0)).astype(f32)

    out = np.zeros(2 * k.size, f32)
    with np.errstate(all="ignore"):
        for c, z in ((0, zr), (1, zi)):
            out[c::2] = c_m1 * at(z, ni - 1) + c_0 * at(z, ni) + c_1 * at(z, ni + 1) + c_2 * at(z, ni + 2)
    return out


class PyPath:
    """One stream's state record over calls, and the record as the library lays it out."""

    def __init__(self, r, tau, taps=IDENTITY):
        self.r, self.tau = float(r), float(tau)
        self.in_pos = self.out_pos = 0
        self.taps = np.asarray(taps, f32).reshape(-1, 2)
        self.hist = np.zeros((HIST, 2), f32)

    def call(self, x):
        """Takes x [2 len] float32; returns the number of outputs the call emits."""
        x = np.asarray(x, f32).reshape(-1, 2)
        cnt = py_count(self.r, self.tau, self.out_pos, self.in_pos + x.shape[0])
        self.hist = np.concatenate([self.hist, x])[-HIST:]
        self.in_pos += x.shape[0]
        self.out_pos += cnt
        return cnt

    def record(self, dtype):
        rec = np.zeros(1, dtype)
        rec["r"], rec["tau"], rec["in_pos"], rec["out_pos"] = self.r, self.tau, self.in_pos, self.out_pos
        rec["n_taps"] = self.taps.shape[0]
        rec["taps"][0, : self.taps.shape[0]] = self.taps
        rec["hist"][0] = self.hist
        return rec

    def at(self, in_pos, hist=None):
        """The state of a stream that has taken in_pos samples whose last 16 were hist."""
        self.in_pos = int(in_pos)
        self.out_pos = py_emitted(self.r, self.tau, self.in_pos)
        self.hist = np.zeros((HIST, 2), f32) if hist is None else np.asarray(hist, f32).reshape(HIST, 2)
        return self


def slip_clock(r, tile_edge_k, side):
    """tau such that the index slip nearest output tile_edge_k (a repeat of
    floor(p) for r < 1, a skip for r > 1) lands on that output (side 0: it is
    the last of its tile when tile_edge_k = m T - 1) or the next (side 1).
    Returns (tau, k of the slip): floor(p_k) - floor(p_{k-1}) != 1 at that k."""
    want = tile_edge_k + side
    for tau in np.linspace(0.0, 1.0, 4001)[:-1]:
        tau = float(tau)
        d = math.floor(p_of(r, tau, want)) - math.floor(p_of(r, tau, want - 1))
        if d != 1:
            return tau, want
    raise AssertionError("no tau puts a slip there")
