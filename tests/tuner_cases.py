"""What the tuner tests share (tests/test_tuner_abi.py, tests/test_gpu_tuner.py):
the yardstick of the tuner (include/qpsk_demod.h, "The tuner on the device"),
written from that text alone.  Needs no GPU and no library.

tables, design    the oscillator's two tables and the prototype from their
                  formulas, libm's cos / sin through the math module.
tuner_reference   the definition as numpy array operations on np.uint64,
                  np.float32 and np.float64: numpy fuses nothing, so every
                  operation rounds once, in the order the definition writes them.
py_emitted        the emit count in Python ints and float64, by its predicate.
PyTuner           one stream's state over a call sequence, pure Python.
ideal_output      a float64 ideal: the exact exponential and the continuous
                  windowed sinc at the exact position.
"""
import functools
import math

import numpy as np

f32, f64, u64 = np.float32, np.float64, np.uint64
PHASES, HIST, TILE = 64, 32, 1024
R_MIN, R_MAX = 0.25, 4.0
MASK = (1 << 64) - 1
PI = 3.14159265358979323846

# the cases of the host form against the yardstick
TAPS = [4, 8, 16, 32]
RATES = [0.25, 0.8, 1.0, 1.0 + 1e-4, 1.25, 3.7, 4.0]
FREQS = [0.0, -0.5, 2.0 ** -60, 0.03, 0.4999]

# (T, r, freq, tone): a unit tone at `tone` cycles per input sample, tuned by
# freq, so that it leaves at (tone - freq) * r cycles per output sample, inside
# the passband of the default cutoff 0.4 * min(1, 1 / r)
IDEAL_CASES = [(16, 1.0, 0.03, 0.05), (16, 1.25, -0.1, 0.02), (16, 4.0, 0.2, 0.21), (16, 0.25, 0.0, 0.1),
               (8, 0.8, 0.03, 0.1), (32, 3.7, -0.4999, -0.47), (4, 1.0 + 1e-4, 0.4, 0.35)]
# 10 log10 of the mean |yardstick - expected tone|^2 of each case above, measured
# with the yardstick on the CPU (tests/test_tuner_abi.py prints them); the bound
# the test asserts is the worst of them plus 3 dB.  The Hamming window sets the
# figure: its stopband (what the resampler's images leave) and, for the short
# filters (T = 4, or cutoff 0.1 over 16 taps), the passband's ripple.
IDEAL_RESIDUAL_DB = [-58.2, -62.5, -46.5, -53.9, -51.5, -69.0, -43.9]
IDEAL_BOUND_DB = max(IDEAL_RESIDUAL_DB) + 3.0


@functools.lru_cache(maxsize=None)
def tables():
    """(C, F): float32 [1024, 2] each."""
    C, F = np.zeros((1024, 2), f32), np.zeros((1024, 2), f32)
    for a in range(1024):
        tc = 2.0 * PI * float(a) / 1024.0
        tf = 2.0 * PI * float(a) / 1048576.0
        C[a] = [math.cos(tc), math.sin(tc)]
        F[a] = [math.cos(tf), math.sin(tf)]
    C[0] = F[0] = [1.0, 0.0]
    return C, F


def default_cutoff(rate):
    return 0.4 * (1.0 / rate if rate > 1.0 else 1.0)


@functools.lru_cache(maxsize=None)
def design_double(T, fc):
    """G[m] and their left-to-right sum, Python floats."""
    N = PHASES * T
    g = 2.0 * fc
    G = [0.0] * (N + 1)
    for m in range(N // 2 + 1):
        t = float(m - N // 2) / 64.0
        x = g * t
        sinc = 1.0 if x == 0.0 else math.sin(PI * x) / (PI * x)
        G[m] = g * sinc * (0.54 - 0.46 * math.cos(2.0 * PI * float(m) / float(N)))
    for m in range(N // 2 + 1, N + 1):
        G[m] = G[N - m]
    total = 0.0
    for v in G:
        total = total + v
    return tuple(G), total


@functools.lru_cache(maxsize=None)
def design(T, fc):
    """h[0 .. 64 T], float32."""
    G, total = design_double(T, fc)
    h = np.array([f32(v * 64.0 / total) for v in G], f32)
    h.setflags(write=False)
    return h


def freq_word(freq):
    """(int64) rint(freq * 2^64) as a Python int: the scaling is exact, round() is to nearest even."""
    return int(round(freq * 2.0 ** 64))


def phases(ph0, fw, i):
    """ph(i) of int64 indices i, uint64, wrapping."""
    return (u64(ph0 & MASK) + u64(fw & MASK) * np.asarray(i, np.int64).view(u64)).astype(u64)


def osc(ph):
    """w of uint64 phases: (re, im) float32 arrays."""
    C, F = tables()
    ph = np.asarray(ph, u64)
    a = (ph >> u64(54)).astype(np.int64)
    b = ((ph >> u64(44)) & u64(1023)).astype(np.int64)
    cr, ci, fr, fi = C[a, 0], C[a, 1], F[b, 0], F[b, 1]
    return cr * fr - ci * fi, cr * fi + ci * fr


def p_of(r, tau, k):
    """p_k = tau + (double)k * r: Python floats are doubles, each operation rounds once."""
    return tau + float(k) * r


def py_emitted(r, tau, T, in_end):
    """How many k >= 0 have floor(p_k) <= in_end - 1 - T/2.  p_k does not
    decrease in k, so a bisection on the predicate itself finds the count."""
    lim = in_end - 1 - T // 2
    if math.floor(p_of(r, tau, 0)) > lim:
        return 0
    lo, hi = 0, 4 * in_end + 8            # lo emits; hi does not (r >= 0.25)
    assert math.floor(p_of(r, tau, hi)) > lim
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if math.floor(p_of(r, tau, mid)) <= lim:
            lo = mid
        else:
            hi = mid
    return hi


def py_count(r, tau, T, out_pos, in_end):
    return max(0, py_emitted(r, tau, T, in_end) - out_pos)


def py_out_bound(n_in, r_min):
    return int(math.ceil(float(n_in) / r_min)) + 4


def tuner_reference(x, r, tau, T, h, fw=0, ph0=0, k0=0, in0=0):
    """Every output the stream can emit from inputs x [2 n] float32 (absolute
    indices in0 .. in0 + n - 1, +0 before them) from output k0 on: interleaved
    float32 [2 (count - k0)].  h: float32 [64 T + 1]."""
    x = np.asarray(x, f32)
    h = np.asarray(h, f32)
    assert h.size == PHASES * T + 1
    d = h[1:] - h[:-1]
    n = x.size // 2
    # z over absolute indices in0 - T .. in0 + n - 1
    xr = np.concatenate([np.zeros(T, f32), x[0::2]])
    xi = np.concatenate([np.zeros(T, f32), x[1::2]])
    wr, wi = osc(phases(ph0, fw, np.arange(in0 - T, in0 + n, dtype=np.int64)))
    with np.errstate(all="ignore"):
        zr = xr * wr + xi * wi
        zi = xi * wr - xr * wi
    assert zr.dtype == f32 and zi.dtype == f32
    count = py_emitted(r, tau, T, in0 + n)
    k = np.arange(k0, count, dtype=np.int64)
    p = f64(tau) + k.astype(f64) * f64(r)
    nf = np.floor(p)
    u = (p - nf) * f64(64.0)
    uq = np.floor(u)
    q = uq.astype(np.int64)
    f = (u - uq).astype(f32)
    base = nf.astype(np.int64) - T // 2 + 1 - (in0 - T)
    assert k.size == 0 or (base.min() >= 0 and base.max() + T - 1 < zr.size)
    ar, ai = np.zeros(k.size, f32), np.zeros(k.size, f32)
    with np.errstate(all="ignore"):
        for j in range(T):
            m = PHASES * (T - 1 - j) + q
            c = h[m] + f * d[m]
            ar = ar + c * zr[base + j]
            ai = ai + c * zi[base + j]
    assert ar.dtype == f32 and c.dtype == f32
    out = np.zeros(2 * k.size, f32)
    out[0::2], out[1::2] = ar, ai
    return out


class PyTuner:
    """One stream's state record over calls, and the record as the library lays it out."""

    def __init__(self, r, tau, T, freq=0.0):
        self.r, self.tau, self.T = float(r), float(tau), int(T)
        self.fw, self.ph0 = freq_word(freq), 0
        self.in_pos = self.out_pos = 0
        self.hist = np.zeros((HIST, 2), f32)

    def call(self, x):
        """Takes x [2 len] float32; returns the number of outputs the call emits."""
        x = np.asarray(x, f32).reshape(-1, 2)
        cnt = py_count(self.r, self.tau, self.T, self.out_pos, self.in_pos + x.shape[0])
        self.hist = np.concatenate([self.hist, x])[-HIST:]
        self.in_pos += x.shape[0]
        self.out_pos += cnt
        return cnt

    def set_freq(self, freq):
        """ph0' = ph0 + (fw_old - fw_new) * in_pos, wrapping: ph(in_pos) stays."""
        new = freq_word(freq)
        self.ph0 = (self.ph0 + (self.fw - new) * self.in_pos) & MASK
        self.fw = new

    def phase(self, i):
        return (self.ph0 + self.fw * i) & MASK

    def reset(self, r, tau):
        self.r, self.tau, self.ph0 = float(r), float(tau), 0
        self.in_pos = self.out_pos = 0
        self.hist = np.zeros((HIST, 2), f32)

    def record(self, dtype):
        rec = np.zeros(1, dtype)
        rec["r"], rec["tau"], rec["in_pos"], rec["out_pos"] = self.r, self.tau, self.in_pos, self.out_pos
        rec["fw"] = self.fw
        rec["ph0"] = self.ph0 & MASK
        rec["hist"][0] = self.hist
        return rec

    def at(self, in_pos, hist=None):
        """The state of a stream that has taken in_pos samples whose last 32 were hist."""
        self.in_pos = int(in_pos)
        self.out_pos = py_emitted(self.r, self.tau, self.T, self.in_pos)
        self.hist = np.zeros((HIST, 2), f32) if hist is None else np.asarray(hist, f32).reshape(HIST, 2)
        return self


def slip_clock(r, T, tile_edge_k, side):
    """tau such that an index slip (a repeat of floor(p) for r < 1, a skip for
    r > 1, r near 1) lands on output tile_edge_k + side.  Returns (tau, k)."""
    want = tile_edge_k + side
    for tau in np.linspace(0.0, 1.0, 4001)[:-1]:
        tau = float(tau)
        if math.floor(p_of(r, tau, want)) - math.floor(p_of(r, tau, want - 1)) != 1:
            return tau, want
    raise AssertionError("no tau puts a slip there")


def ideal_output(tone, r, tau, T, fc, freq, n_in):
    """(y, expected): the float64 ideal of a unit tone e^{j 2 pi tone i}, i in
    [0, n_in), for the outputs whose filter lies wholly inside the row: mixed by
    the exact exponential, filtered by the continuous windowed sinc at the exact
    position p_k - i; and the tone the output should be, e^{j 2 pi (tone - freq)
    p_k}.  Also returns the k of those outputs."""
    _, total = design_double(T, fc)
    count = py_emitted(r, tau, T, n_in)
    k = np.arange(count, dtype=np.int64)
    p = tau + k.astype(f64) * r
    nf = np.floor(p).astype(np.int64)
    keep = nf - T // 2 + 1 >= 0
    k, p, nf = k[keep], p[keep], nf[keep]
    y = np.zeros(k.size, np.complex128)
    g = 2.0 * fc
    for j in range(T):
        i = nf - T // 2 + 1 + j
        t = p - i                                    # the tap's time, in input samples from the filter's centre
        m = t * 64.0 + 32.0 * T                      # its place on the prototype's grid
        xg = g * t
        sinc = np.where(xg == 0.0, 1.0, np.sin(PI * xg) / np.where(xg == 0.0, 1.0, PI * xg))
        c = g * sinc * (0.54 - 0.46 * np.cos(2.0 * PI * m / (64.0 * T))) * 64.0 / total
        y += c * np.exp(2j * np.pi * (tone - freq) * i)
    return y, np.exp(2j * np.pi * (tone - freq) * p), k
