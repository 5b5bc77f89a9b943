// qpsk_path.cpp -- the host half of the propagation path (include/qpsk_demod.h,
// "The propagation path on the device"): the parameter defaults and checks, the
// construction of a stream's state, the checks of a call, qpsk_path_count and
// qpsk_path_out_bound, qpsk_path_state_check, which qpsk_path_set_state runs on
// a blob before anything reaches the device, and qpsk_path_apply_host, the call
// itself on host rows.  No HIP, no device: a stand-alone CPU program links this
// file and qpsk_error.cpp (tools/path_main.cpp runs it under the sanitizers).
#include "qpsk_path.h"

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

std::string num(double v) {
    char b[40];
    snprintf(b, sizeof(b), "%.17g", v);
    return b;
}

int bad_field(int s, const std::string &field, const std::string &value, const std::string &range) {
    return fail(QPSK_ERR_ARGUMENT, "path state stream " + std::to_string(s) + ": " + field + " = " + value +
                                       " outside " + range);
}

bool plus_zero(float v) {
    uint32_t u;
    std::memcpy(&u, &v, sizeof(u));
    return u == 0;
}

int check_state(int s, const PathState &st) {
    if (!(st.r >= path_r_min() && st.r <= path_r_max()))
        return bad_field(s, "r", num(st.r), "[" + num(path_r_min()) + ", " + num(path_r_max()) + "]");
    if (!(st.tau >= 0.0 && st.tau < 1.0)) return bad_field(s, "tau", num(st.tau), "[0, 1)");
    if (st.in_pos < 0 || st.in_pos > kPathMaxPos) return bad_field(s, "in_pos", std::to_string(st.in_pos), "[0, 2^50]");
    if (st.out_pos < 0 || st.out_pos > 2 * kPathMaxPos)
        return bad_field(s, "out_pos", std::to_string(st.out_pos), "[0, 2^51]");
    const int64_t want = path_emitted(st.r, st.tau, st.in_pos);
    if (st.out_pos != want)
        return bad_field(s, "out_pos", std::to_string(st.out_pos),
                         "qpsk_path_count(r, tau, 0, in_pos) = " + std::to_string(want));
    if (st.n_taps < 1 || st.n_taps > kPathMaxTaps) return bad_field(s, "n_taps", std::to_string(st.n_taps), "[1, 8]");
    for (int j = 0; j < kPathMaxTaps; ++j)
        for (int c = 0; c < 2; ++c) {
            const float v = st.taps[j][c];
            const std::string name = "taps[" + std::to_string(j) + "]" + (c ? ".im" : ".re");
            if (j < st.n_taps ? !std::isfinite(v) : !plus_zero(v))
                return bad_field(s, name, num(v), j < st.n_taps ? "the finite floats" : "+0 (an unused tap)");
        }
    for (int h = 0; h < kPathHist; ++h)
        if (st.in_pos - kPathHist + h < 0 && !(plus_zero(st.hist[h][0]) && plus_zero(st.hist[h][1])))
            return bad_field(s, "hist[" + std::to_string(h) + "]", num(st.hist[h][0]) + ", " + num(st.hist[h][1]),
                             "+0 (an index before the stream's start)");
    for (size_t b = 0; b < sizeof(st.reserved); ++b)
        if (st.reserved[b]) return bad_field(s, "reserved", std::to_string(st.reserved[b]), "[0, 0]");
    return QPSK_OK;
}

}  // namespace

int path_check_params(const qpsk_path_params *p, int32_t n_streams) {
    if (!p) return fail(QPSK_ERR_ARGUMENT_NULL, "path params are null");
    if (!std::isfinite(p->clock_ppm))
        return fail(QPSK_ERR_OUT_OF_RANGE, "clock_ppm must be finite, got " + num(p->clock_ppm));
    if (!(std::isfinite(p->clock_spread) && p->clock_spread >= 0.0))
        return fail(QPSK_ERR_OUT_OF_RANGE, "clock_spread must be finite and >= 0, got " + num(p->clock_spread));
    if (!(std::fabs(p->clock_ppm) + p->clock_spread <= QPSK_PATH_MAX_PPM))
        return fail(QPSK_ERR_OUT_OF_RANGE, "|clock_ppm| + clock_spread must not exceed 1000, got " +
                                               num(std::fabs(p->clock_ppm) + p->clock_spread));
    if (!(p->tau0 >= 0.0 && p->tau0 < 1.0)) return fail(QPSK_ERR_OUT_OF_RANGE, "tau0 must lie in [0, 1), got " + num(p->tau0));
    if (p->first_stream < 0) return fail(QPSK_ERR_OUT_OF_RANGE, "first_stream must be >= 0");
    if (n_streams < 1) return fail(QPSK_ERR_ARGUMENT, "n_streams must be positive");
    return QPSK_OK;
}

PathState path_state_new(const qpsk_path_params &p, int32_t row) {
    PathState st{};
    path_clock(p.clock_ppm, p.clock_spread, p.clock_seed, p.tau0, p.tau_random,
               static_cast<uint64_t>(p.first_stream) + static_cast<uint64_t>(row), &st.r, &st.tau);
    // a spread draw lands within the limits by construction; the last rounding
    // of r may not, and then it is the limit
    st.r = st.r < path_r_min() ? path_r_min() : (st.r > path_r_max() ? path_r_max() : st.r);
    if (p.multipath) {
        // [1, 0.25 e^{j0.7}, 0.1 e^{-j1.9}, 0.05], in double as qpsk_synth_generate forms them
        const double mr[4] = {1.0, 0.25 * std::cos(0.7), 0.1 * std::cos(-1.9), 0.05};
        const double mi[4] = {0.0, 0.25 * std::sin(0.7), 0.1 * std::sin(-1.9), 0.0};
        st.n_taps = 4;
        for (int j = 0; j < 4; ++j) {
            st.taps[j][0] = static_cast<float>(mr[j]);
            st.taps[j][1] = static_cast<float>(mi[j]);
        }
    } else {
        st.n_taps = 1;
        st.taps[0][0] = 1.0f;
    }
    return st;
}

int path_check_taps(const float *taps_iq, int32_t n_taps) {
    if (!taps_iq) return fail(QPSK_ERR_ARGUMENT_NULL, "taps are null");
    if (n_taps < 1 || n_taps > kPathMaxTaps) return fail(QPSK_ERR_ARGUMENT, "n_taps must lie in [1, 8]");
    for (int32_t j = 0; j < 2 * n_taps; ++j)
        if (!std::isfinite(taps_iq[j]))
            return fail(QPSK_ERR_OUT_OF_RANGE, "tap " + std::to_string(j / 2) + " is not finite");
    return QPSK_OK;
}

void path_put_taps(PathState &st, const float *taps_iq, int32_t n_taps) {
    st.n_taps = n_taps;
    std::memset(st.taps, 0, sizeof(st.taps));
    std::memcpy(st.taps, taps_iq, sizeof(float) * 2 * n_taps);
}

int path_check_call(const PathState *st, int32_t S, int64_t stride_in, int64_t stride_out, int64_t out_cap,
                    int64_t n_samples, const int64_t *lengths, int64_t *n_out, int64_t *n_call, int64_t *n_out_max) {
    if (n_samples < 0) return fail(QPSK_ERR_ARGUMENT, "n_samples must not be negative");
    if (out_cap < 0) return fail(QPSK_ERR_ARGUMENT, "out_cap must not be negative");
    if (n_samples > (INT64_MAX >> 4) || out_cap > (INT64_MAX >> 4)) return fail(QPSK_ERR_ARGUMENT, "stride too small");
    int rc;
    if ((rc = check_lengths(S, n_samples, lengths, n_call))) return rc;
    if (*n_call > 0 && (stride_in < 2 * n_samples || stride_out < 2 * out_cap))
        return fail(QPSK_ERR_ARGUMENT, "stride too small");
    return check_counts(st, S, n_samples, lengths, out_cap, kPathMaxPos, "stream", "samples",
                        [](const PathState &r, int64_t in_end) { return path_count(r.r, r.tau, r.out_pos, in_end); },
                        n_out, n_out_max);
}

void path_apply_stream(PathState &st, const float *in, int64_t len, float *out) {
    const int64_t in_pos = st.in_pos;
    const int L = st.n_taps;
    // x at absolute index i: the call's row, the history, +0 before the start
    auto x_at = [&](int64_t i) {
        if (i >= in_pos) return PathC{in[2 * (i - in_pos)], in[2 * (i - in_pos) + 1]};
        const int64_t h = kPathHist - (in_pos - i);
        return h >= 0 ? PathC{st.hist[h][0], st.hist[h][1]} : PathC{0.0f, 0.0f};
    };
    auto z_at = [&](int64_t i) {
        PathC acc{0.0f, 0.0f};
        for (int j = 0; j < L; ++j) {
            const PathC x = x_at(i - j);
            path_tap(acc, st.taps[j][0], st.taps[j][1], x.re, x.im);
        }
        return acc;
    };
    const int64_t cnt = path_count(st.r, st.tau, st.out_pos, in_pos + len);
    for (int64_t o = 0; o < cnt; ++o) {
        const PathC y = path_output(st.r, st.tau, st.out_pos + o, z_at);
        out[2 * o] = y.re;
        out[2 * o + 1] = y.im;
    }
    float hist[kPathHist][2];
    for (int h = 0; h < kPathHist; ++h) {
        const PathC x = x_at(in_pos + len - kPathHist + h);
        hist[h][0] = x.re, hist[h][1] = x.im;
    }
    std::memcpy(st.hist, hist, sizeof(hist));
    st.in_pos = in_pos + len;
    st.out_pos += cnt;
}

}  // namespace qpsk

extern "C" {

void qpsk_path_params_init(qpsk_path_params *p) {
    if (!p) return;
    *p = qpsk_path_params{};
    p->clock_seed = 3000;
}

int qpsk_path_state_size(void) { return static_cast<int>(sizeof(qpsk::PathState)); }

int64_t qpsk_path_out_bound(const qpsk_path_params *p, int64_t n_in) {
    int rc;
    if ((rc = qpsk::path_check_params(p, 1))) return rc;
    if (n_in < 0 || n_in > qpsk::kPathMaxPos) return qpsk::fail(QPSK_ERR_ARGUMENT, "n_in outside [0, 2^50]");
    const double r_min = 1.0 - (std::fabs(p->clock_ppm) + p->clock_spread) * 1e-6;
    return static_cast<int64_t>(std::ceil(static_cast<double>(n_in) / r_min)) + 2;
}

int64_t qpsk_path_count(double r, double tau, int64_t out_pos, int64_t in_end) {
    using namespace qpsk;
    if (!path_clock_ok(r, tau)) return fail(QPSK_ERR_ARGUMENT, "r must lie within 1000 ppm of 1 and tau in [0, 1)");
    if (out_pos < 0 || out_pos > 2 * kPathMaxPos || in_end < 0 || in_end > kPathMaxPos)
        return fail(QPSK_ERR_ARGUMENT, "in_end must lie in [0, 2^50] and out_pos in [0, 2^51]");
    return path_count(r, tau, out_pos, in_end);
}

int qpsk_path_state_init(const qpsk_path_params *p, int32_t n_streams, void *buf, int64_t buf_bytes) {
    using namespace qpsk;
    int rc;
    if ((rc = path_check_params(p, n_streams))) return rc;
    if (!buf) return fail(QPSK_ERR_ARGUMENT_NULL, "path state buffer is null");
    if (buf_bytes != static_cast<int64_t>(n_streams) * static_cast<int64_t>(sizeof(PathState)))
        return fail(QPSK_ERR_ARGUMENT, "path state length does not match n_streams");
    for (int32_t s = 0; s < n_streams; ++s) {
        const PathState st = path_state_new(*p, s);
        std::memcpy(static_cast<char *>(buf) + sizeof(PathState) * s, &st, sizeof(st));
    }
    return QPSK_OK;
}

int qpsk_path_state_check(int32_t n_streams, const void *buf, int64_t buf_bytes) {
    using namespace qpsk;
    if (n_streams < 1) return fail(QPSK_ERR_ARGUMENT, "n_streams must be positive");
    if (!buf) return fail(QPSK_ERR_ARGUMENT_NULL, "path state buffer is null");
    int rc;
    if ((rc = check_state_bytes("path", buf_bytes, static_cast<int64_t>(n_streams) * static_cast<int64_t>(sizeof(PathState)))))
        return rc;
    const char *rec = static_cast<const char *>(buf);
    for (int32_t s = 0; s < n_streams; ++s, rec += sizeof(PathState)) {
        PathState st;
        std::memcpy(&st, rec, sizeof(st));
        if ((rc = check_state(s, st))) return rc;
    }
    return QPSK_OK;
}

int qpsk_path_apply_host(void *state, int64_t state_bytes, int32_t n_streams, const float *in, int64_t stride_in,
                         float *out, int64_t stride_out, int64_t out_cap, int64_t n_samples,
                         const int64_t *lengths, int64_t *n_out) {
    using namespace qpsk;
    int rc;
    if ((rc = qpsk_path_state_check(n_streams, state, state_bytes))) return rc;
    std::vector<PathState> st(n_streams);
    std::memcpy(st.data(), state, state_bytes);
    if (!n_out) return fail(QPSK_ERR_ARGUMENT_NULL, "n_out is null");
    int64_t n_call, n_out_max;
    std::vector<int64_t> cnt(n_streams);   // n_out is written once nothing can refuse the call any more
    if ((rc = path_check_call(st.data(), n_streams, stride_in, stride_out, out_cap, n_samples, lengths, cnt.data(), &n_call,
                              &n_out_max)))
        return rc;
    if (n_call > 0 && !in) return fail(QPSK_ERR_ARGUMENT_NULL, "in is null");
    if (n_out_max > 0 && !out) return fail(QPSK_ERR_ARGUMENT_NULL, "out is null");
    if (n_call > 0 && n_out_max > 0 &&
        rows_overlap(in, n_streams, stride_in, n_samples, sizeof(float), out, n_streams, stride_out, out_cap, sizeof(float)))
        return fail(QPSK_ERR_ARGUMENT, "out must not overlap in");
    std::memcpy(n_out, cnt.data(), sizeof(int64_t) * n_streams);
    for (int32_t s = 0; s < n_streams; ++s)
        path_apply_stream(st[s], in ? in + s * stride_in : nullptr, lengths ? lengths[s] : n_samples,
                          out ? out + s * stride_out : nullptr);
    std::memcpy(state, st.data(), state_bytes);
    return QPSK_OK;
}

}  // extern "C"
