// qpsk_tuner.cpp -- the host half of the tuner (include/qpsk_demod.h, "The
// tuner on the device"): the parameter defaults and checks, the prototype's
// design, the oscillator's two tables, the construction of a stream's state, the
// checks of a call, qpsk_tuner_count and qpsk_tuner_out_bound,
// qpsk_tuner_state_check, which qpsk_tuner_set_state runs on a blob before
// anything reaches the device, and qpsk_tuner_apply_host, the call itself on
// host rows.  No HIP, no device: a stand-alone CPU program links this file and
// qpsk_error.cpp (tools/tuner_main.cpp runs it under the sanitizers).
#include "qpsk_tuner.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "qpsk_demod.h"
#include "qpsk_internal.h"
#include "qpsk_row_call.h"

namespace qpsk {
namespace {

constexpr double kPi = 3.14159265358979323846;

std::string num(double v) {
    char b[40];
    snprintf(b, sizeof(b), "%.17g", v);
    return b;
}

int bad_field(int s, const std::string &field, const std::string &value, const std::string &range) {
    return fail(QPSK_ERR_ARGUMENT, "tuner state stream " + std::to_string(s) + ": " + field + " = " + value +
                                       " outside " + range);
}

bool plus_zero(float v) {
    uint32_t u;
    std::memcpy(&u, &v, sizeof(u));
    return u == 0;
}

int check_state(int s, int T, const TunerState &st) {
    if (!(st.r >= QPSK_TUNER_MIN_RATE && st.r <= QPSK_TUNER_MAX_RATE)) return bad_field(s, "r", num(st.r), "[0.25, 4]");
    if (!(st.tau >= 0.0 && st.tau < 1.0)) return bad_field(s, "tau", num(st.tau), "[0, 1)");
    if (st.in_pos < 0 || st.in_pos > kTunerMaxPos) return bad_field(s, "in_pos", std::to_string(st.in_pos), "[0, 2^50]");
    const int64_t want = tuner_emitted(st.r, st.tau, T, st.in_pos);
    if (st.out_pos != want)
        return bad_field(s, "out_pos", std::to_string(st.out_pos),
                         "qpsk_tuner_count(r, tau, T, 0, in_pos) = " + std::to_string(want));
    for (int h = 0; h < kTunerHist; ++h)
        if (st.in_pos - kTunerHist + h < 0 && !(plus_zero(st.hist[h][0]) && plus_zero(st.hist[h][1])))
            return bad_field(s, "hist[" + std::to_string(h) + "]", num(st.hist[h][0]) + ", " + num(st.hist[h][1]),
                             "+0 (an index before the stream's start)");
    for (size_t b = 0; b < sizeof(st.reserved); ++b)
        if (st.reserved[b]) return bad_field(s, "reserved", std::to_string(st.reserved[b]), "[0, 0]");
    return QPSK_OK;
}

struct Tables {
    float coarse[kTunerTable][2], fine[kTunerTable][2];
    Tables() {
        for (int a = 0; a < kTunerTable; ++a) {
            const double tc = 2.0 * kPi * static_cast<double>(a) / 1024.0;
            const double tf = 2.0 * kPi * static_cast<double>(a) / 1048576.0;
            coarse[a][0] = static_cast<float>(std::cos(tc)), coarse[a][1] = static_cast<float>(std::sin(tc));
            fine[a][0] = static_cast<float>(std::cos(tf)), fine[a][1] = static_cast<float>(std::sin(tf));
        }
        coarse[0][0] = fine[0][0] = 1.0f;
        coarse[0][1] = fine[0][1] = 0.0f;
    }
};

const Tables &tables() {
    static const Tables t;
    return t;
}

int check_design_args(int32_t T, double cutoff) {
    if (!tuner_taps_ok(T))
        return fail(QPSK_ERR_OUT_OF_RANGE, "taps_per_phase must be even and lie in 4 .. 32, got " + std::to_string(T));
    if (!(cutoff > 0.0 && cutoff <= 0.5)) return fail(QPSK_ERR_OUT_OF_RANGE, "cutoff must lie in (0, 0.5], got " + num(cutoff));
    return QPSK_OK;
}

}  // namespace

const float (*tuner_coarse())[2] { return tables().coarse; }
const float (*tuner_fine())[2] { return tables().fine; }

double tuner_cutoff(const qpsk_tuner_params &p) {
    return p.cutoff == 0.0 ? 0.4 * (p.rate > 1.0 ? 1.0 / p.rate : 1.0) : p.cutoff;
}

void tuner_design(int T, double fc, float *h) {
    const int N = kTunerPhases * T;
    const double g = 2.0 * fc;
    std::vector<double> G(N + 1);
    for (int m = 0; m <= N / 2; ++m) {
        const double t = static_cast<double>(m - N / 2) / 64.0;
        const double x = g * t;
        const double sinc = x == 0.0 ? 1.0 : std::sin(kPi * x) / (kPi * x);
        G[m] = g * sinc * (0.54 - 0.46 * std::cos(2.0 * kPi * static_cast<double>(m) / static_cast<double>(N)));
    }
    for (int m = N / 2 + 1; m <= N; ++m) G[m] = G[N - m];
    double sum = 0.0;
    for (int m = 0; m <= N; ++m) sum = sum + G[m];
    for (int m = 0; m <= N; ++m) h[m] = static_cast<float>(G[m] * 64.0 / sum);
}

void tuner_pairs(int T, const float *h, float (*hd)[2]) {
    const int N = kTunerPhases * T;
    for (int m = 0; m < N; ++m) hd[m][0] = h[m], hd[m][1] = h[m + 1] - h[m];
    hd[N][0] = h[N], hd[N][1] = 0.0f;
}

int tuner_check_params(const qpsk_tuner_params *p, int32_t n_streams, const double *freq, const double *rate) {
    if (!p) return fail(QPSK_ERR_ARGUMENT_NULL, "tuner params are null");
    if (!tuner_freq_ok(p->freq)) return fail(QPSK_ERR_OUT_OF_RANGE, "freq must lie in [-0.5, 0.5), got " + num(p->freq));
    if (!(p->rate >= QPSK_TUNER_MIN_RATE && p->rate <= QPSK_TUNER_MAX_RATE))
        return fail(QPSK_ERR_OUT_OF_RANGE, "rate must lie in [0.25, 4], got " + num(p->rate));
    if (!(p->tau0 >= 0.0 && p->tau0 < 1.0)) return fail(QPSK_ERR_OUT_OF_RANGE, "tau0 must lie in [0, 1), got " + num(p->tau0));
    if (!(p->cutoff >= 0.0)) return fail(QPSK_ERR_OUT_OF_RANGE, "cutoff must lie in (0, 0.5] or be 0, got " + num(p->cutoff));
    int rc;
    if ((rc = check_design_args(p->taps_per_phase, tuner_cutoff(*p)))) return rc;
    if (p->first_stream < 0) return fail(QPSK_ERR_OUT_OF_RANGE, "first_stream must be >= 0");
    if (n_streams < 1) return fail(QPSK_ERR_ARGUMENT, "n_streams must be positive");
    for (int32_t s = 0; s < n_streams; ++s) {
        if (freq && !tuner_freq_ok(freq[s]))
            return fail(QPSK_ERR_OUT_OF_RANGE, "freq[" + std::to_string(s) + "] must lie in [-0.5, 0.5), got " + num(freq[s]));
        if (rate && !(rate[s] >= QPSK_TUNER_MIN_RATE && rate[s] <= QPSK_TUNER_MAX_RATE))
            return fail(QPSK_ERR_OUT_OF_RANGE, "rate[" + std::to_string(s) + "] must lie in [0.25, 4], got " + num(rate[s]));
    }
    return QPSK_OK;
}

int tuner_check_taps(const float *taps, int64_t n_taps, int T) {
    if (!taps) return fail(QPSK_ERR_ARGUMENT_NULL, "taps are null");
    if (n_taps != tuner_points(T))
        return fail(QPSK_ERR_ARGUMENT, "n_points must be 64 * taps_per_phase + 1 = " + std::to_string(tuner_points(T)) +
                                           ", got " + std::to_string(n_taps));
    for (int64_t n = 0; n < n_taps; ++n)
        if (!std::isfinite(taps[n])) return fail(QPSK_ERR_OUT_OF_RANGE, "tap " + std::to_string(n) + " is not finite");
    return QPSK_OK;
}

TunerState tuner_state_new(const qpsk_tuner_params &p, double freq, double rate) {
    TunerState st{};
    st.r = rate;
    st.tau = p.tau0;
    st.fw = tuner_freq_word(freq);
    return st;
}

int tuner_check_call(const TunerState *st, int32_t S, int T, int64_t stride_in, int64_t stride_out, int64_t out_cap,
                     int64_t n_samples, const int64_t *lengths, int64_t *n_out, int64_t *n_call, int64_t *n_out_max) {
    if (n_samples < 0) return fail(QPSK_ERR_ARGUMENT, "n_samples must not be negative");
    if (out_cap < 0) return fail(QPSK_ERR_ARGUMENT, "out_cap must not be negative");
    if (n_samples > (INT64_MAX >> 4) || out_cap > (INT64_MAX >> 4)) return fail(QPSK_ERR_ARGUMENT, "stride too small");
    int rc;
    if ((rc = check_lengths(S, n_samples, lengths, n_call))) return rc;
    if (*n_call > 0 && (stride_in < 2 * n_samples || stride_out < 2 * out_cap))
        return fail(QPSK_ERR_ARGUMENT, "stride too small");
    return check_counts(st, S, n_samples, lengths, out_cap, kTunerMaxPos, "stream", "samples",
                        [T](const TunerState &r, int64_t in_end) { return tuner_count(r.r, r.tau, T, r.out_pos, in_end); },
                        n_out, n_out_max);
}

void tuner_apply_stream(TunerState &st, int T, const float (*hd)[2], const float *in, int64_t len, float *out) {
    const int64_t in_pos = st.in_pos;
    const float(*coarse)[2] = tuner_coarse(), (*fine)[2] = tuner_fine();
    // x at absolute index i: the call's row, the history, +0 before the start
    auto x_at = [&](int64_t i) {
        if (i >= in_pos) return TunerC{in[2 * (i - in_pos)], in[2 * (i - in_pos) + 1]};
        const int64_t h = kTunerHist - (in_pos - i);
        return h >= 0 ? TunerC{st.hist[h][0], st.hist[h][1]} : TunerC{0.0f, 0.0f};
    };
    auto z_at = [&](int64_t i) { return tuner_mix(x_at(i), tuner_osc(tuner_phase(st.ph0, st.fw, i), coarse, fine)); };
    const int64_t cnt = tuner_count(st.r, st.tau, T, st.out_pos, in_pos + len);
    for (int64_t o = 0; o < cnt; ++o) {
        const TunerC y = tuner_output(st.r, st.tau, T, st.out_pos + o, hd, z_at);
        out[2 * o] = y.re;
        out[2 * o + 1] = y.im;
    }
    float hist[kTunerHist][2];
    for (int h = 0; h < kTunerHist; ++h) {
        const TunerC x = x_at(in_pos + len - kTunerHist + h);
        hist[h][0] = x.re, hist[h][1] = x.im;
    }
    std::memcpy(st.hist, hist, sizeof(hist));
    st.in_pos = in_pos + len;
    st.out_pos += cnt;
}

}  // namespace qpsk

extern "C" {

void qpsk_tuner_params_init(qpsk_tuner_params *p) {
    if (!p) return;
    *p = qpsk_tuner_params{};
    p->rate = 1.0;
    p->taps_per_phase = 16;
}

int qpsk_tuner_state_size(void) { return static_cast<int>(sizeof(qpsk::TunerState)); }

int qpsk_tuner_design(int32_t taps_per_phase, double cutoff, float *h, int64_t n_points) {
    using namespace qpsk;
    int rc;
    if ((rc = check_design_args(taps_per_phase, cutoff))) return rc;
    if (!h) return fail(QPSK_ERR_ARGUMENT_NULL, "h is null");
    if (n_points != tuner_points(taps_per_phase))
        return fail(QPSK_ERR_ARGUMENT, "n_points must be 64 * taps_per_phase + 1 = " +
                                           std::to_string(tuner_points(taps_per_phase)));
    tuner_design(taps_per_phase, cutoff, h);
    return QPSK_OK;
}

int qpsk_tuner_tables(float *coarse, float *fine) {
    using namespace qpsk;
    if (!coarse || !fine) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    std::memcpy(coarse, tuner_coarse(), sizeof(float) * 2 * kTunerTable);
    std::memcpy(fine, tuner_fine(), sizeof(float) * 2 * kTunerTable);
    return QPSK_OK;
}

int qpsk_tuner_osc(const uint64_t *ph, int64_t n, float *w) {
    using namespace qpsk;
    if (n < 0) return fail(QPSK_ERR_ARGUMENT, "n must not be negative");
    if (n > 0 && (!ph || !w)) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    for (int64_t i = 0; i < n; ++i) {
        const TunerC v = tuner_osc(ph[i], tuner_coarse(), tuner_fine());
        w[2 * i] = v.re, w[2 * i + 1] = v.im;
    }
    return QPSK_OK;
}

int64_t qpsk_tuner_out_bound(const qpsk_tuner_params *p, const double *rates, int32_t n_streams, int64_t n_in) {
    using namespace qpsk;
    int rc;
    if ((rc = tuner_check_params(p, n_streams, nullptr, rates))) return rc;
    if (n_in < 0 || n_in > kTunerMaxPos) return fail(QPSK_ERR_ARGUMENT, "n_in outside [0, 2^50]");
    double r_min = rates ? rates[0] : p->rate;
    for (int32_t s = 1; rates && s < n_streams; ++s) r_min = rates[s] < r_min ? rates[s] : r_min;
    return static_cast<int64_t>(std::ceil(static_cast<double>(n_in) / r_min)) + 4;
}

int64_t qpsk_tuner_count(double r, double tau, int32_t taps_per_phase, int64_t out_pos, int64_t in_end) {
    using namespace qpsk;
    if (!tuner_clock_ok(r, tau)) return fail(QPSK_ERR_ARGUMENT, "r must lie in [0.25, 4] and tau in [0, 1)");
    if (!tuner_taps_ok(taps_per_phase)) return fail(QPSK_ERR_ARGUMENT, "taps_per_phase must be even and lie in 4 .. 32");
    if (out_pos < 0 || out_pos > kTunerMaxOut + 2 || in_end < 0 || in_end > kTunerMaxPos)
        return fail(QPSK_ERR_ARGUMENT, "in_end must lie in [0, 2^50] and out_pos in [0, 2^52 + 2]");
    return tuner_count(r, tau, taps_per_phase, out_pos, in_end);
}

int qpsk_tuner_state_init(const qpsk_tuner_params *p, int32_t n_streams, const double *freq, const double *rate,
                          void *buf, int64_t buf_bytes) {
    using namespace qpsk;
    int rc;
    if ((rc = tuner_check_params(p, n_streams, freq, rate))) return rc;
    if (!buf) return fail(QPSK_ERR_ARGUMENT_NULL, "tuner state buffer is null");
    if (buf_bytes != static_cast<int64_t>(n_streams) * static_cast<int64_t>(sizeof(TunerState)))
        return fail(QPSK_ERR_ARGUMENT, "tuner state length does not match n_streams");
    for (int32_t s = 0; s < n_streams; ++s) {
        const TunerState st = tuner_state_new(*p, freq ? freq[s] : p->freq, rate ? rate[s] : p->rate);
        std::memcpy(static_cast<char *>(buf) + sizeof(TunerState) * s, &st, sizeof(st));
    }
    return QPSK_OK;
}

int qpsk_tuner_state_check(const qpsk_tuner_params *p, int32_t n_streams, const void *buf, int64_t buf_bytes) {
    using namespace qpsk;
    int rc;
    if ((rc = tuner_check_params(p, n_streams, nullptr, nullptr))) return rc;
    if (!buf) return fail(QPSK_ERR_ARGUMENT_NULL, "tuner state buffer is null");
    if ((rc = check_state_bytes("tuner", buf_bytes, static_cast<int64_t>(n_streams) * static_cast<int64_t>(sizeof(TunerState)))))
        return rc;
    const char *rec = static_cast<const char *>(buf);
    for (int32_t s = 0; s < n_streams; ++s, rec += sizeof(TunerState)) {
        TunerState st;
        std::memcpy(&st, rec, sizeof(st));
        if ((rc = check_state(s, p->taps_per_phase, st))) return rc;
    }
    return QPSK_OK;
}

int qpsk_tuner_apply_host(const qpsk_tuner_params *p, const float *h, void *state, int64_t state_bytes,
                          int32_t n_streams, const float *in, int64_t stride_in, float *out, int64_t stride_out,
                          int64_t out_cap, int64_t n_samples, const int64_t *lengths, int64_t *n_out) {
    using namespace qpsk;
    int rc;
    if ((rc = qpsk_tuner_state_check(p, n_streams, state, state_bytes))) return rc;
    const int T = p->taps_per_phase;
    if (h && (rc = tuner_check_taps(h, tuner_points(T), T))) return rc;
    std::vector<TunerState> st(n_streams);
    std::memcpy(st.data(), state, state_bytes);
    if (!n_out) return fail(QPSK_ERR_ARGUMENT_NULL, "n_out is null");
    int64_t n_call, n_out_max;
    std::vector<int64_t> cnt(n_streams);   // n_out is written once nothing can refuse the call any more
    if ((rc = tuner_check_call(st.data(), n_streams, T, stride_in, stride_out, out_cap, n_samples, lengths, cnt.data(),
                               &n_call, &n_out_max)))
        return rc;
    if (n_call > 0 && !in) return fail(QPSK_ERR_ARGUMENT_NULL, "in is null");
    if (n_out_max > 0 && !out) return fail(QPSK_ERR_ARGUMENT_NULL, "out is null");
    if (n_call > 0 && n_out_max > 0 &&
        rows_overlap(in, n_streams, stride_in, n_samples, sizeof(float), out, n_streams, stride_out, out_cap, sizeof(float)))
        return fail(QPSK_ERR_ARGUMENT, "out must not overlap in");
    std::vector<float> own(h ? 0 : tuner_points(T));
    if (!h) tuner_design(T, tuner_cutoff(*p), own.data());
    std::vector<float> hd(2 * static_cast<size_t>(tuner_points(T)));
    tuner_pairs(T, h ? h : own.data(), reinterpret_cast<float(*)[2]>(hd.data()));
    std::memcpy(n_out, cnt.data(), sizeof(int64_t) * n_streams);
    for (int32_t s = 0; s < n_streams; ++s)
        tuner_apply_stream(st[s], T, reinterpret_cast<const float(*)[2]>(hd.data()), in ? in + s * stride_in : nullptr,
                           lengths ? lengths[s] : n_samples, out ? out + s * stride_out : nullptr);
    std::memcpy(state, st.data(), state_bytes);
    return QPSK_OK;
}

}  // extern "C"
