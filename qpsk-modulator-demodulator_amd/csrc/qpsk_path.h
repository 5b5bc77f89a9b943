// qpsk_path.h -- the propagation path (include/qpsk_demod.h, "The propagation
// path on the device"), once: the position of an output and its mu, the four
// weights of MuellerMuller.CubicLagrange4 (MuellerMuller.cs:177-189), one step
// of the tap sum and the emit count.  The kernels (qpsk_path.hip) and the host
// (qpsk_path.cpp: construction, the state check, qpsk_path_apply_host, and the
// stand-alone tools/path_main.cpp) run the same functions, so the device cannot
// drift from what the host can be held to.  Also the state record.  No HIP
// header: plain C++ sees plain inline functions.  Compile with
// -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstdint>

#include "qpsk_channel.h"   // chan_next_double: the draw the oscillators use
#include "qpsk_demod.h"

namespace qpsk {

constexpr int kPathMaxTaps = QPSK_PATH_MAX_TAPS;
constexpr int kPathHist = QPSK_PATH_HIST;
constexpr int64_t kPathMaxPos = int64_t{1} << 50;   // positions stay exact doubles with room to spare
static_assert(kPathMaxTaps - 1 + 3 <= kPathHist, "the history covers the taps and the interpolator's reach");

// One stream as the state holds it (256 bytes).
struct PathState {
    double r, tau;
    int64_t in_pos, out_pos;
    int32_t n_taps;
    float taps[kPathMaxTaps][2];
    float hist[kPathHist][2];     // inputs in_pos - 16 .. in_pos - 1, widened
    uint8_t reserved[28];
};
static_assert(sizeof(PathState) == 256, "the state layout of include/qpsk_demod.h");

struct PathC {
    float re, im;
};

// the limits of r: 1000 ppm either way, formed as a stream's r is
QPSK_HD double path_r_min() { return 1.0 + -QPSK_PATH_MAX_PPM * 1e-6; }
QPSK_HD double path_r_max() { return 1.0 + QPSK_PATH_MAX_PPM * 1e-6; }
QPSK_HD bool path_clock_ok(double r, double tau) {
    return r >= path_r_min() && r <= path_r_max() && tau >= 0.0 && tau < 1.0;   // a NaN fails
}

// (r, tau) of global stream g
QPSK_HD void path_clock(double clock_ppm, double clock_spread, uint64_t clock_seed, double tau0, int tau_random,
                        uint64_t g, double *r, double *tau) {
    uint64_t st = clock_seed + g;
    const double u1 = chan_next_double(st), u2 = chan_next_double(st);
    const double ppm = clock_ppm + (clock_spread > 0.0 ? (u1 * 2.0 - 1.0) * clock_spread : 0.0);
    *r = 1.0 + ppm * 1e-6;
    *tau = tau_random ? u2 : tau0;
}

// p_k = tau + (double)k * r: the product rounds, then the sum
QPSK_HD double path_p(double r, double tau, int64_t k) { return tau + static_cast<double>(k) * r; }

// output k: n = floor(p_k) and t = (float)(p_k - n)
QPSK_HD void path_pos(double r, double tau, int64_t k, int64_t *n, float *t) {
    const double p = path_p(r, tau, k);
    const double fl = floor(p);
    *n = static_cast<int64_t>(fl);
    *t = static_cast<float>(p - fl);
}

// CubicLagrange4's basis for points at {-1, 0, 1, 2} (MuellerMuller.cs:177-186)
QPSK_HD void path_weights(float t, float c[4]) {
    const float tm1 = t - 1.0f, tm2 = t - 2.0f, tp1 = t + 1.0f;
    c[0] = -(t * tm1 * tm2) * (1.0f / 6.0f);
    c[1] = (tp1 * tm1 * tm2) * (1.0f / 2.0f);
    c[2] = -(tp1 * t * tm2) * (1.0f / 2.0f);
    c[3] = (tp1 * t * tm1) * (1.0f / 6.0f);
}

// :188-189, one component
QPSK_HD float path_interp(const float c[4], float zm1, float z0, float z1, float z2) {
    return c[0] * zm1 + c[1] * z0 + c[2] * z1 + c[3] * z2;
}

// one tap of z[i]: acc + h * x
QPSK_HD void path_tap(PathC &acc, float hre, float him, float xre, float xim) {
    acc.re = acc.re + (hre * xre - him * xim);
    acc.im = acc.im + (hre * xim + him * xre);
}

// The outputs k >= 0 with floor(p_k) <= in_end - 3, i.e. p_k < in_end - 2: p_k
// does not decrease in k (a rounded product and a rounded sum are monotone), so
// that is the smallest k with p_k >= in_end - 2.  The guess comes from a
// division, whose error stays below one output for positions below 2^50 (the
// ulp of p is at most 2^-2 there); the predicate itself moves it to the exact
// answer, in a bounded number of steps.  r, tau as path_clock_ok accepts them,
// 0 <= in_end <= 2^50.
QPSK_HD int64_t path_emitted(double r, double tau, int64_t in_end) {
    if (in_end < 3) return 0;                       // p_k >= 0 = in_end - 2 at best
    const double lim = static_cast<double>(in_end - 2);
    int64_t k = static_cast<int64_t>(ceil((lim - tau) / r));
    if (k < 0) k = 0;
    for (int it = 0; it < 8 && k > 0 && path_p(r, tau, k - 1) >= lim; ++it) --k;
    for (int it = 0; it < 8 && path_p(r, tau, k) < lim; ++it) ++k;
    return k;
}

// what a stream at out_pos emits once it has taken in_end inputs
QPSK_HD int64_t path_count(double r, double tau, int64_t out_pos, int64_t in_end) {
    const int64_t k = path_emitted(r, tau, in_end);
    return k > out_pos ? k - out_pos : 0;
}

// One output of a stream whose z is read through z_at(i), i the absolute index.
template <typename Z>
QPSK_HD PathC path_output(double r, double tau, int64_t k, Z z_at) {
    int64_t n;
    float t, c[4];
    path_pos(r, tau, k, &n, &t);
    path_weights(t, c);
    const PathC a = z_at(n - 1), b = z_at(n), d = z_at(n + 1), e = z_at(n + 2);
    return PathC{path_interp(c, a.re, b.re, d.re, e.re), path_interp(c, a.im, b.im, d.im, e.im)};
}

// the state of row `row` of a handle with parameters p, as its constructor leaves it
PathState path_state_new(const qpsk_path_params &p, int32_t row);
// the checks of qpsk_path_create on p and n_streams
int path_check_params(const qpsk_path_params *p, int32_t n_streams);
// the checks of qpsk_path_set_taps; fills st's taps (unused ones +0) from taps_iq
int path_check_taps(const float *taps_iq, int32_t n_taps);
void path_put_taps(PathState &st, const float *taps_iq, int32_t n_taps);
// The argument checks a call makes before anything moves (host or device form):
// lengths within [0, n_samples], strides, capacity; fills n_out[s] and the
// longest row.  st: the [S] records the counts come from.
int path_check_call(const PathState *st, int32_t S, int64_t stride_in, int64_t stride_out, int64_t out_cap,
                    int64_t n_samples, const int64_t *lengths, int64_t *n_out, int64_t *n_call, int64_t *n_out_max);
// one stream's call on host float rows; advances st
void path_apply_stream(PathState &st, const float *in, int64_t len, float *out);

}  // namespace qpsk
