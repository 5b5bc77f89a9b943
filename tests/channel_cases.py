"""What the channel tests share (tests/test_channel_abi.py, tests/test_gpu_channel.py):
the oscillator of LocalOscilator.cs:5-194 in pure Python, whose fields can be
read (the oracle keeps its own private), seed scans with it, and the numpy
restatement of the noise sample.  Needs no GPU and no library.
"""
import math

import numpy as np

M64 = (1 << 64) - 1
TWO_PI = 2.0 * math.pi


def splitmix64(st):
    """(new state, output)"""
    st = (st + 0x9E3779B97F4A7C15) & M64
    z = st
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return st, z ^ (z >> 31)


def u01(z):
    return float(z >> 11) * 2.0 ** -53


def wrap(x):
    r = math.fmod(x, TWO_PI)
    return r + TWO_PI if r < 0 else r


class PyNCO:
    """new NCO(freq_hz, fs, ppm, phase0) drawing from splitmix64(seed)."""

    def __init__(self, freq_hz, fs, ppm=0.0, phase0=0.0, seed=1):
        self.base_hz, self.fs, self.max_ppm = float(freq_hz), float(fs), abs(float(ppm))
        self.rng = seed & M64
        self.interval = int(max(fs * 1e-3, 1))
        self.counter = 0
        self.static_ppm = (self._draw() * 2.0 - 1.0) * self.max_ppm if self.max_ppm > 0.0 else 0.0
        self.drift_ppm = 0.0
        self.total_ppm = self.static_ppm
        self.cur_hz = self.base_hz * (1.0 + self.total_ppm * 1e-6)
        self.phase = wrap(float(phase0))
        self.clamped_hi = self.clamped_lo = 0

    def _draw(self):
        self.rng, z = splitmix64(self.rng)
        return u01(z)

    def next(self):
        if self.max_ppm <= 0.0:
            self.cur_hz = self.base_hz
        else:
            self.counter += 1
            if self.counter >= self.interval:
                self.counter = 0
                self.drift_ppm += (self._draw() * 2.0 - 1.0) * (self.max_ppm * 0.001)
                self.total_ppm = self.static_ppm + self.drift_ppm
                if self.total_ppm > self.max_ppm:
                    self.total_ppm = self.max_ppm
                    self.drift_ppm = self.total_ppm - self.static_ppm
                    self.clamped_hi += 1
                elif self.total_ppm < -self.max_ppm:
                    self.total_ppm = -self.max_ppm
                    self.drift_ppm = self.total_ppm - self.static_ppm
                    self.clamped_lo += 1
                self.cur_hz = self.base_hz * (1.0 + self.total_ppm * 1e-6)
        self.phase = wrap(self.phase + TWO_PI * self.cur_hz / self.fs)
        return complex(math.cos(self.phase), math.sin(self.phase))

    def fields(self):
        return (self.static_ppm, self.drift_ppm, self.total_ppm, self.cur_hz, self.phase, self.counter, self.rng)


def static_fraction(seed):
    """static_ppm / max_ppm of an oscillator seeded with seed: its first draw."""
    return u01(splitmix64(seed & M64)[1]) * 2.0 - 1.0


def seed_near(edge, start=1, margin=0.0005):
    """The first seed >= start whose static error lies within margin * max of
    edge * max (edge = +1 or -1)."""
    s = start
    while True:
        f = static_fraction(s)
        if (edge > 0 and f >= 1.0 - margin) or (edge < 0 and f <= -1.0 + margin):
            return s
        s += 1


def noise_reference(noise_seed, g, pos0, n, rms):
    """The n noise samples of stream g from position pos0 on, as interleaved
    float32 (HelperModels.cs:17-45 over the counter-based draws), in float64
    numpy arithmetic."""
    pos = np.arange(pos0, pos0 + n, dtype=np.uint64)
    h = np.uint64(noise_seed & M64) ^ np.uint64((g << 40) & M64) ^ pos ^ np.uint64(0xA5A5A5A5)

    def draw(st):
        with np.errstate(over="ignore"):
            st = st + np.uint64(0x9E3779B97F4A7C15)
            z = st
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return st, z ^ (z >> np.uint64(31))

    h, z1 = draw(h)
    h, z2 = draw(h)
    u1 = 1.0 - (z1 >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    u2 = 1.0 - (z2 >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    mag = np.sqrt(-2.0 * np.log(u1)) * rms
    ph = TWO_PI * u2
    out = np.empty(2 * n, np.float32)
    out[0::2] = np.clip((mag * np.cos(ph)).astype(np.float32), -1.0, 1.0)
    out[1::2] = np.clip((mag * np.sin(ph)).astype(np.float32), -1.0, 1.0)
    return out
