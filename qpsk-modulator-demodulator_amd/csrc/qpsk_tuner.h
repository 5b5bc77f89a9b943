// qpsk_tuner.h -- the tuner (include/qpsk_demod.h, "The tuner on the device"),
// once: the frequency word, the phase of an absolute index, the oscillator's
// table lookup and the mixer, the position of an output and its (n, q, f), one
// tap step of the polyphase filter, the emit count, and the state record.  The
// kernels (qpsk_tuner.hip) and the host (qpsk_tuner.cpp: the design, the
// tables, the checks, qpsk_tuner_apply_host, and the stand-alone
// tools/tuner_main.cpp) run the same functions, so the device cannot drift from
// what the host can be held to.  No HIP header: plain C++ sees plain inline
// functions.  Compile with -ffp-contract=off.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "qpsk_demod.h"
#include "qpsk_path.h"  // path_p: the closed form of an output's position

namespace qpsk {

constexpr int kTunerHist = QPSK_TUNER_HIST;
constexpr int kTunerPhases = QPSK_TUNER_PHASES;
constexpr int kTunerMinTaps = QPSK_TUNER_MIN_TAPS;
constexpr int kTunerMaxTaps = QPSK_TUNER_MAX_TAPS;
constexpr int kTunerTable = 1024;                    // entries of the coarse and of the fine table
constexpr int64_t kTunerMaxPos = kPathMaxPos;        // input positions, as the path holds them
constexpr int64_t kTunerMaxOut = int64_t{1} << 52;   // output positions at r = 0.25
static_assert(kTunerMaxTaps - 1 <= kTunerHist, "the history covers the filter's reach");

// One stream as the state holds it (320 bytes).
struct TunerState {
    double r, tau;
    int64_t fw;
    uint64_t ph0;
    int64_t in_pos, out_pos;
    uint8_t reserved[16];
    float hist[kTunerHist][2];    // inputs in_pos - 32 .. in_pos - 1, widened, not mixed
};
static_assert(sizeof(TunerState) == 320 && offsetof(TunerState, hist) == 64, "the state layout of include/qpsk_demod.h");

struct TunerC {
    float re, im;
};

// the number of prototype points of a handle with T taps a phase
QPSK_HD int tuner_points(int T) { return kTunerPhases * T + 1; }
QPSK_HD bool tuner_taps_ok(int T) { return T >= kTunerMinTaps && T <= kTunerMaxTaps && T % 2 == 0; }
QPSK_HD bool tuner_freq_ok(double freq) { return freq >= -0.5 && freq < 0.5; }   // a NaN fails
QPSK_HD bool tuner_clock_ok(double r, double tau) {
    return r >= QPSK_TUNER_MIN_RATE && r <= QPSK_TUNER_MAX_RATE && tau >= 0.0 && tau < 1.0;
}

// fw = (int64) rint(freq * 2^64): the scaling is exact, and -0.5 <= freq < 0.5
// keeps the result within int64
QPSK_HD int64_t tuner_freq_word(double freq) { return static_cast<int64_t>(rint(ldexp(freq, 64))); }

// the phase of absolute input index i (negative before the stream's start), wrapping
QPSK_HD uint64_t tuner_phase(uint64_t ph0, int64_t fw, int64_t i) {
    return ph0 + static_cast<uint64_t>(fw) * static_cast<uint64_t>(i);
}

// what set_freq leaves in ph0 so that the phase of in_pos stays what it was
QPSK_HD uint64_t tuner_retune(uint64_t ph0, int64_t fw_old, int64_t fw_new, int64_t in_pos) {
    return ph0 + (static_cast<uint64_t>(fw_old) - static_cast<uint64_t>(fw_new)) * static_cast<uint64_t>(in_pos);
}

// w of phase ph: the coarse entry times the fine one
QPSK_HD TunerC tuner_osc(uint64_t ph, const float (*coarse)[2], const float (*fine)[2]) {
    const uint32_t a = static_cast<uint32_t>(ph >> 54), b = static_cast<uint32_t>(ph >> 44) & 1023u;
    const float cr = coarse[a][0], ci = coarse[a][1], fr = fine[b][0], fi = fine[b][1];
    return TunerC{cr * fr - ci * fi, cr * fi + ci * fr};
}

// z = x * conj(w)
QPSK_HD TunerC tuner_mix(TunerC x, TunerC w) { return TunerC{x.re * w.re + x.im * w.im, x.im * w.re - x.re * w.im}; }

// output k: n = floor(p_k), q = floor(64 mu), f = (float)(64 mu - q)
QPSK_HD void tuner_pos(double r, double tau, int64_t k, int64_t *n, int *q, float *f) {
    const double p = path_p(r, tau, k);
    const double fl = floor(p);
    const double u = (p - fl) * 64.0;
    const double uq = floor(u);
    *n = static_cast<int64_t>(fl);
    *q = static_cast<int>(uq);
    *f = static_cast<float>(u - uq);
}

// one tap: the coefficient between two prototype points, then acc + c * z
QPSK_HD void tuner_tap(TunerC &acc, float h, float d, float f, float zre, float zim) {
    const float c = h + f * d;
    acc.re = acc.re + c * zre;
    acc.im = acc.im + c * zim;
}

// The outputs k >= 0 with floor(p_k) <= in_end - 1 - T/2, i.e. p_k < in_end -
// T/2: p_k does not decrease in k, so that is the smallest k with p_k >= in_end
// - T/2.  The guess is the path's division; the predicate itself moves it to
// the exact answer (for positions below 2^50 the ulp of p is at most 2^-3 and r
// at least 2^-2, so the guess is a few outputs off at most).
QPSK_HD int64_t tuner_emitted(double r, double tau, int T, int64_t in_end) {
    if (in_end <= T / 2) return 0;                  // p_k >= 0 >= in_end - T/2
    const double lim = static_cast<double>(in_end - T / 2);
    int64_t k = static_cast<int64_t>(ceil((lim - tau) / r));
    if (k < 0) k = 0;
    for (int it = 0; it < 16 && k > 0 && path_p(r, tau, k - 1) >= lim; ++it) --k;
    for (int it = 0; it < 16 && path_p(r, tau, k) < lim; ++it) ++k;
    return k;
}

// what a stream at out_pos emits once it has taken in_end inputs
QPSK_HD int64_t tuner_count(double r, double tau, int T, int64_t out_pos, int64_t in_end) {
    const int64_t k = tuner_emitted(r, tau, T, in_end);
    return k > out_pos ? k - out_pos : 0;
}

// One output of a stream whose mixed input is read through z_at(i), i the
// absolute index; hd[m] = (h[m], d[m]).
template <typename Z>
QPSK_HD TunerC tuner_output(double r, double tau, int T, int64_t k, const float (*hd)[2], Z z_at) {
    int64_t n;
    int q;
    float f;
    tuner_pos(r, tau, k, &n, &q, &f);
    TunerC acc{0.0f, 0.0f};
    for (int j = 0; j < T; ++j) {
        const int m = kTunerPhases * (T - 1 - j) + q;
        const TunerC z = z_at(n - T / 2 + 1 + j);
        tuner_tap(acc, hd[m][0], hd[m][1], f, z.re, z.im);
    }
    return acc;
}

// the cutoff a handle of p designs for
double tuner_cutoff(const qpsk_tuner_params &p);
// the prototype h[0 .. 64 T] of (T, fc)
void tuner_design(int T, double fc, float *h);
// (h, d) side by side from h
void tuner_pairs(int T, const float *h, float (*hd)[2]);
// the two oscillator tables, formed once
const float (*tuner_coarse())[2];
const float (*tuner_fine())[2];
// the checks of qpsk_tuner_create on p, n_streams and the optional per-stream arrays
int tuner_check_params(const qpsk_tuner_params *p, int32_t n_streams, const double *freq, const double *rate);
// the checks of qpsk_tuner_set_taps
int tuner_check_taps(const float *taps, int64_t n_taps, int T);
// the state of a stream as its constructor leaves it
TunerState tuner_state_new(const qpsk_tuner_params &p, double freq, double rate);
// The argument checks a call makes before anything moves (host or device form),
// as path_check_call.
int tuner_check_call(const TunerState *st, int32_t S, int T, int64_t stride_in, int64_t stride_out, int64_t out_cap,
                     int64_t n_samples, const int64_t *lengths, int64_t *n_out, int64_t *n_call, int64_t *n_out_max);
// one stream's call on host float rows; advances st
void tuner_apply_stream(TunerState &st, int T, const float (*hd)[2], const float *in, int64_t len, float *out);

}  // namespace qpsk
