// qpsk_channel.h -- the oscillator of the test bench's channel
// (include/qpsk_demod.h, "The test bench's channel on the device";
// LocalOscilator.cs:5-194), once: the kernel's scan lanes (qpsk_channel.hip)
// and the host (qpsk_channel.cpp: construction, reset, the state check, and
// the stand-alone tools/channel_state_main.cpp) step the same function, so the
// device cannot drift from what the host can be held to.  Also the state
// record and the noise draw.  No HIP header: plain C++ sees plain inline
// functions.  Compile with -ffp-contract=off; the one fma is explicit.
#pragma once
#include <cmath>
#include <cstdint>

#include "qpsk_demod.h"

#ifdef __HIP__
#define QPSK_HD __host__ __device__ inline
#else
#define QPSK_HD inline
#endif

namespace qpsk {

// One oscillator as the state holds it (56 bytes), and one stream (128 bytes).
struct ChanNco {
    double static_ppm, drift_ppm, total_ppm, cur_hz, phase;
    int64_t counter;
    uint64_t rng;
};
struct ChanState {
    ChanNco tx, rx;
    int64_t pos;        // samples the stream has taken: the noise draw's counter
    int64_t reserved;
};
static_assert(sizeof(ChanNco) == 56 && sizeof(ChanState) == 128, "the state layout of include/qpsk_demod.h");

// What an oscillator's constructor fixes (LocalOscilator.cs:20-60).
struct ChanNcoConst {
    double base_hz, fs, max_ppm;
    int64_t interval;
};

constexpr double kChanTwoPi = 2.0 * 3.14159265358979311600;   // 2.0 * Math.PI
constexpr double kChanInvTwoPi = 0.15915494309189534561;

QPSK_HD ChanNcoConst chan_nco_const(double lo_hz, double fs, double ppm) {
    const double iv = fs * 1e-3;
    // (int)(iv > 1 ? iv : 1); a rate past 2^31 kHz has no meaning and is held to INT32_MAX
    const double ivc = iv > 1 ? (iv < 2147483647.0 ? iv : 2147483647.0) : 1;
    return ChanNcoConst{lo_hz, fs, fabs(ppm), static_cast<int64_t>(static_cast<int>(ivc))};
}

QPSK_HD uint64_t chan_splitmix64(uint64_t &st) {
    uint64_t z = (st += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
QPSK_HD double chan_next_double(uint64_t &st) { return static_cast<double>(chan_splitmix64(st) >> 11) * 0x1.0p-53; }

// fmod(x, 2 pi), then + 2 pi if that is negative (LocalOscilator.cs wrap).
// fmod is exact, r = x - q * 2 pi with q = trunc(x / 2 pi), and r is a double;
// so one fma of the right q gives it with no rounding.  q comes from a
// multiplication by 1 / 2 pi and may be one off either way (|x| < 2^40 keeps
// its error far below 1): r then lies outside [0, 2 pi) on x's side, by its
// sign or size, both of which the fma's single rounding preserves, and the
// neighbouring q is taken.  A zero remainder carries x's sign, as fmod's does.
QPSK_HD double chan_wrap(double x) {
    const double y = kChanTwoPi;
    double r;
    if (fabs(x) < 0x1p40) {
        // the three candidates side by side and two selects: on the device the
        // step is one lone wave's dependent chain, and a branch costs it more
        // than an fma it may not need
        const double q = trunc(x * kChanInvTwoPi);
        const double r0 = fma(-q, y, x), rm = fma(-(q - 1.0), y, x), rp = fma(-(q + 1.0), y, x);
        const bool pos = x >= 0;
        const bool down = pos ? r0 < 0 : r0 <= -y;      // q one too large: take q - 1
        const bool up = pos ? r0 >= y : r0 > 0;         // q one too small: take q + 1
        r = down ? rm : (up ? rp : r0);
        r = r == 0 ? copysign(0.0, x) : r;
    } else {
        r = fmod(x, y);   // also NaN and Inf
    }
    if (r < 0) r += y;
    return r;
}

QPSK_HD double chan_cur_hz(const ChanNcoConst &c, double total_ppm) { return c.base_hz * (1.0 + total_ppm * 1e-6); }
// the phase increment of a sample: 2.0 * Math.PI * cur_hz / fs, left to right
QPSK_HD double chan_inc(const ChanNcoConst &c, double cur_hz) { return kChanTwoPi * cur_hz / c.fs; }

// new NCO(base_hz, fs, ppm, phase0) drawing from seed
QPSK_HD ChanNco chan_nco_new(const ChanNcoConst &c, double phase0, uint64_t seed) {
    ChanNco n{};
    n.rng = seed;
    n.static_ppm = c.max_ppm > 0.0 ? (chan_next_double(n.rng) * 2.0 - 1.0) * c.max_ppm : 0.0;
    n.drift_ppm = 0.0;
    n.total_ppm = n.static_ppm;
    n.cur_hz = chan_cur_hz(c, n.total_ppm);
    n.phase = chan_wrap(phase0);
    n.counter = 0;
    return n;
}

// NextSample's state update; returns the new phase, whose cos and sin are the
// sample.  inc is the caller's copy of chan_inc(c, n.cur_hz): cur_hz moves only
// in a drift update, and the division need not be repeated in between.
QPSK_HD double chan_nco_step(const ChanNcoConst &c, ChanNco &n, double &inc) {
    if (c.max_ppm > 0.0 && ++n.counter >= c.interval) {
        n.counter = 0;
        const double step = (chan_next_double(n.rng) * 2.0 - 1.0) * (c.max_ppm * 0.001);
        n.drift_ppm += step;
        n.total_ppm = n.static_ppm + n.drift_ppm;
        if (n.total_ppm > c.max_ppm) {
            n.total_ppm = c.max_ppm;
            n.drift_ppm = n.total_ppm - n.static_ppm;
        } else if (n.total_ppm < -c.max_ppm) {
            n.total_ppm = -c.max_ppm;
            n.drift_ppm = n.total_ppm - n.static_ppm;
        }
        n.cur_hz = chan_cur_hz(c, n.total_ppm);
        inc = chan_inc(c, n.cur_hz);
    }
    n.phase = chan_wrap(n.phase + inc);
    return n.phase;
}

// The two uniforms of the noise sample of stream g at position pos, both in (0, 1].
QPSK_HD void chan_noise_uniforms(uint64_t noise_seed, uint64_t g, int64_t pos, double *u1, double *u2) {
    uint64_t h = noise_seed ^ (g << 40) ^ static_cast<uint64_t>(pos) ^ 0xA5A5A5A5ULL;
    *u1 = 1.0 - chan_next_double(h);
    *u2 = 1.0 - chan_next_double(h);
}

// the state of row `row` of a handle with parameters p, as its constructor leaves it
ChanState chan_state_new(const qpsk_channel_params &p, int32_t row);
// the checks of qpsk_channel_create on p and n_streams
int chan_check_params(const qpsk_channel_params *p, int32_t n_streams);

}  // namespace qpsk
