// qpsk_pfb.cpp -- the host half of the polyphase channeliser (include/qpsk_demod.h,
// "The polyphase channeliser on the device"): the parameter defaults and
// checks, the prototype's design, the twiddles, the checks of a call,
// qpsk_pfb_count, qpsk_pfb_out_bound and qpsk_pfb_tile_frames,
// qpsk_pfb_state_check, which qpsk_pfb_set_state runs on a blob before anything
// reaches the device, and qpsk_pfb_apply_host, the call itself on host rows.  No
// HIP, no device: a stand-alone CPU program links this file and qpsk_error.cpp
// (tools/pfb_main.cpp runs it under the sanitizers).
#include "qpsk_pfb.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "qpsk_demod.h"
#include "qpsk_internal.h"
#include "qpsk_row_call.h"

namespace qpsk {
namespace {

constexpr double kPi = 3.14159265358979323846;

bool plus_zero(float v) {
    uint32_t u;
    std::memcpy(&u, &v, sizeof(u));
    return u == 0;
}

int bad_field(int b, const std::string &field, const std::string &value, const std::string &range) {
    return fail(QPSK_ERR_ARGUMENT, "pfb state band " + std::to_string(b) + ": " + field + " = " + value + " outside " +
                                       range);
}

int check_shape(int M, int K) {
    if (M < kPfbMinChannels || M > kPfbMaxChannels || (M & (M - 1)))
        return fail(QPSK_ERR_OUT_OF_RANGE, "channels must be a power of two in 8 .. 4096, got " + std::to_string(M));
    if (K < 1 || K > kPfbMaxBranchTaps)
        return fail(QPSK_ERR_OUT_OF_RANGE, "taps_per_branch must lie in 1 .. 16, got " + std::to_string(K));
    if (M * K > kPfbMaxTaps)
        return fail(QPSK_ERR_OUT_OF_RANGE, "channels * taps_per_branch must not exceed 32768, got " + std::to_string(M * K));
    return QPSK_OK;
}

int check_band(const qpsk_pfb_params &p, int b, const char *rec) {
    const int M = p.channels, L = M * p.taps_per_branch;
    PfbHead hd;
    std::memcpy(&hd, rec, sizeof(hd));
    if (hd.in_pos < 0 || hd.in_pos > kPfbMaxPos) return bad_field(b, "in_pos", std::to_string(hd.in_pos), "[0, 2^50]");
    const int64_t want = pfb_emitted(M, hd.in_pos);
    if (hd.out_pos != want)
        return bad_field(b, "out_pos", std::to_string(hd.out_pos), "ceil(in_pos / D) = " + std::to_string(want));
    for (size_t k = 0; k < sizeof(hd.reserved); ++k)
        if (hd.reserved[k]) return bad_field(b, "reserved", std::to_string(hd.reserved[k]), "[0, 0]");
    // entries at indices before the band's start
    const int64_t before = hd.in_pos < L ? L - hd.in_pos : 0;
    for (int64_t h = 0; h < before; ++h) {
        float v[2];
        std::memcpy(v, rec + sizeof(PfbHead) + 8 * h, sizeof(v));
        if (!(plus_zero(v[0]) && plus_zero(v[1])))
            return bad_field(b, "hist[" + std::to_string(h) + "]", std::to_string(v[0]) + ", " + std::to_string(v[1]),
                             "+0 (an index before the band's start)");
    }
    return QPSK_OK;
}

}  // namespace

int pfb_check_params(const qpsk_pfb_params *p, int32_t n_bands) {
    if (!p) return fail(QPSK_ERR_ARGUMENT_NULL, "pfb params are null");
    int rc;
    if ((rc = check_shape(p->channels, p->taps_per_branch))) return rc;
    if (!std::isfinite(p->gain)) return fail(QPSK_ERR_OUT_OF_RANGE, "gain must be finite");
    if (n_bands < 1 || n_bands > 65535) return fail(QPSK_ERR_ARGUMENT, "n_bands must lie in 1 .. 65535");
    return QPSK_OK;
}

int pfb_check_taps(const float *taps, int64_t n_taps, int L) {
    if (!taps) return fail(QPSK_ERR_ARGUMENT_NULL, "taps are null");
    if (n_taps != L)
        return fail(QPSK_ERR_ARGUMENT, "n_taps must be channels * taps_per_branch = " + std::to_string(L) + ", got " +
                                           std::to_string(n_taps));
    for (int64_t n = 0; n < n_taps; ++n)
        if (!std::isfinite(taps[n])) return fail(QPSK_ERR_OUT_OF_RANGE, "tap " + std::to_string(n) + " is not finite");
    return QPSK_OK;
}

void pfb_design(int M, int K, float *h) {
    const int L = M * K;
    std::vector<double> g(L, 0.0);
    for (int n = 1; n <= L / 2; ++n) {
        const double t = static_cast<double>(n - L / 2) / static_cast<double>(M);
        const double sinc = t == 0.0 ? 1.0 : std::sin(kPi * t) / (kPi * t);
        g[n] = sinc * (0.54 - 0.46 * std::cos(2.0 * kPi * static_cast<double>(n - 1) / static_cast<double>(L - 2)));
    }
    for (int n = L / 2 + 1; n < L; ++n) g[n] = g[L - n];
    double sum = 0.0;
    for (int n = 1; n < L; ++n) sum = sum + g[n];
    h[0] = 0.0f;
    for (int n = 1; n < L; ++n) h[n] = static_cast<float>(g[n] / sum);
}

void pfb_twiddles(int M, float *w) {
    for (int q = 0; q < M / 2; ++q) {
        const double a = 2.0 * kPi * static_cast<double>(q) / static_cast<double>(M);
        w[2 * q] = static_cast<float>(std::cos(a));
        w[2 * q + 1] = static_cast<float>(std::sin(a));
    }
    w[0] = 1.0f, w[1] = 0.0f;
    w[2 * (M / 4)] = 0.0f, w[2 * (M / 4) + 1] = 1.0f;
}

int pfb_check_call(const qpsk_pfb_params &p, const PfbHead *heads, int32_t B, int64_t stride_in, int64_t stride_out,
                   int64_t out_cap, int64_t n_samples, const int64_t *lengths, int64_t *n_out, int64_t *n_call,
                   int64_t *n_out_max) {
    if (n_samples < 0) return fail(QPSK_ERR_ARGUMENT, "n_samples must not be negative");
    if (out_cap < 0) return fail(QPSK_ERR_ARGUMENT, "out_cap must not be negative");
    if (n_samples > kPfbMaxPos || out_cap > kPfbMaxPos) return fail(QPSK_ERR_ARGUMENT, "stride too small");
    int rc;
    if ((rc = check_lengths(B, n_samples, lengths, n_call))) return rc;
    if (*n_call > 0 && (stride_in < 2 * n_samples || stride_out < 2 * out_cap))
        return fail(QPSK_ERR_ARGUMENT, "stride too small");
    const int M = p.channels;
    return check_counts(heads, B, n_samples, lengths, out_cap, kPfbMaxPos, "band", "frames",
                        [M](const PfbHead &r, int64_t in_end) { return pfb_count(M, r.out_pos, in_end); }, n_out,
                        n_out_max);
}

void pfb_apply_band(const qpsk_pfb_params &p, const float *h, const float *w, PfbHead &head, float *hist, const float *in,
                    int64_t len, float *out, int64_t stride_out) {
    const int M = p.channels, K = p.taps_per_branch, L = M * K, bits = pfb_log2(M);
    const int64_t in_pos = head.in_pos;
    // x at absolute index i: the call's row, the history, +0 before the start
    auto x_at = [&](int64_t i) {
        if (i >= in_pos) return PfbC{in[2 * (i - in_pos)], in[2 * (i - in_pos) + 1]};
        const int64_t k = L - (in_pos - i);
        return k >= 0 ? PfbC{hist[2 * k], hist[2 * k + 1]} : PfbC{0.0f, 0.0f};
    };
    const int64_t cnt = pfb_count(M, head.out_pos, in_pos + len);
    std::vector<PfbC> a(M);
    for (int64_t o = 0; o < cnt; ++o) {
        const int64_t m = head.out_pos + o;
        for (int q = 0; q < M; ++q) {
            PfbC acc{0.0f, 0.0f};
            for (int k = 0; k < K; ++k) {
                const PfbC x = x_at(pfb_index(M, m, q, k));
                pfb_step(acc, h[q + k * M], x.re, x.im);
            }
            a[pfb_bitrev(q, bits)] = acc;
        }
        for (int half = 1; half < M; half *= 2)
            for (int j0 = 0; j0 < M; j0 += 2 * half)
                for (int j = 0; j < half; ++j) {
                    const int q = j * (M / (2 * half));
                    pfb_butterfly(a[j0 + j], a[j0 + j + half], w[2 * q], w[2 * q + 1]);
                }
        for (int c = 0; c < M; ++c) {
            const PfbC y = pfb_output(a[c], c, m, p.gain);
            out[c * stride_out + 2 * o] = y.re;
            out[c * stride_out + 2 * o + 1] = y.im;
        }
    }
    std::vector<float> next(2 * static_cast<size_t>(L));
    for (int k = 0; k < L; ++k) {
        const PfbC x = x_at(in_pos + len - L + k);
        next[2 * k] = x.re, next[2 * k + 1] = x.im;
    }
    std::memcpy(hist, next.data(), sizeof(float) * next.size());
    head.in_pos = in_pos + len;
    head.out_pos += cnt;
}

}  // namespace qpsk

extern "C" {

void qpsk_pfb_params_init(qpsk_pfb_params *p) {
    if (!p) return;
    *p = qpsk_pfb_params{};
    p->channels = 64;
    p->taps_per_branch = 8;
    p->gain = 1.0f;
}

int qpsk_pfb_design(const qpsk_pfb_params *p, float *taps, int64_t n_taps) {
    using namespace qpsk;
    int rc;
    if ((rc = pfb_check_params(p, 1))) return rc;
    if (!taps) return fail(QPSK_ERR_ARGUMENT_NULL, "taps are null");
    if (n_taps != static_cast<int64_t>(p->channels) * p->taps_per_branch)
        return fail(QPSK_ERR_ARGUMENT, "n_taps must be channels * taps_per_branch");
    pfb_design(p->channels, p->taps_per_branch, taps);
    return QPSK_OK;
}

int qpsk_pfb_twiddles(int32_t channels, float *w, int64_t n_floats) {
    using namespace qpsk;
    int rc;
    if ((rc = check_shape(channels, 1))) return rc;
    if (!w) return fail(QPSK_ERR_ARGUMENT_NULL, "w is null");
    if (n_floats != channels) return fail(QPSK_ERR_ARGUMENT, "n_floats must be channels");
    pfb_twiddles(channels, w);
    return QPSK_OK;
}

int64_t qpsk_pfb_count(int32_t channels, int64_t out_pos, int64_t in_end) {
    using namespace qpsk;
    int rc;
    if ((rc = check_shape(channels, 1))) return rc;
    if (out_pos < 0 || in_end < 0 || in_end > kPfbMaxPos)
        return fail(QPSK_ERR_ARGUMENT, "in_end must lie in [0, 2^50] and out_pos must not be negative");
    return pfb_count(channels, out_pos, in_end);
}

int64_t qpsk_pfb_out_bound(int32_t channels, int64_t n_in) {
    using namespace qpsk;
    int rc;
    if ((rc = check_shape(channels, 1))) return rc;
    if (n_in < 0 || n_in > kPfbMaxPos) return fail(QPSK_ERR_ARGUMENT, "n_in outside [0, 2^50]");
    return n_in / (channels / 2) + 1;
}

int qpsk_pfb_tile_frames(int32_t channels) {
    int rc;
    if ((rc = qpsk::check_shape(channels, 1))) return rc;
    return qpsk::pfb_tile_frames(channels);
}

int64_t qpsk_pfb_state_size(const qpsk_pfb_params *p) {
    int rc;
    if ((rc = qpsk::pfb_check_params(p, 1))) return rc;
    return qpsk::pfb_state_bytes(p->channels, p->taps_per_branch);
}

int qpsk_pfb_state_init(const qpsk_pfb_params *p, int32_t n_bands, void *buf, int64_t buf_bytes) {
    using namespace qpsk;
    int rc;
    if ((rc = pfb_check_params(p, n_bands))) return rc;
    if (!buf) return fail(QPSK_ERR_ARGUMENT_NULL, "pfb state buffer is null");
    if (buf_bytes != n_bands * pfb_state_bytes(p->channels, p->taps_per_branch))
        return fail(QPSK_ERR_ARGUMENT, "pfb state length does not match n_bands");
    std::memset(buf, 0, buf_bytes);
    return QPSK_OK;
}

int qpsk_pfb_state_check(const qpsk_pfb_params *p, int32_t n_bands, const void *buf, int64_t buf_bytes) {
    using namespace qpsk;
    int rc;
    if ((rc = pfb_check_params(p, n_bands))) return rc;
    if (!buf) return fail(QPSK_ERR_ARGUMENT_NULL, "pfb state buffer is null");
    const int64_t each = pfb_state_bytes(p->channels, p->taps_per_branch);
    if ((rc = check_state_bytes("pfb", buf_bytes, n_bands * each))) return rc;
    const char *rec = static_cast<const char *>(buf);
    for (int32_t b = 0; b < n_bands; ++b, rec += each)
        if ((rc = check_band(*p, b, rec))) return rc;
    return QPSK_OK;
}

int qpsk_pfb_apply_host(const qpsk_pfb_params *p, const float *taps, void *state, int64_t state_bytes, int32_t n_bands,
                        const float *in, int64_t stride_in, float *out, int64_t stride_out, int64_t out_cap,
                        int64_t n_samples, const int64_t *lengths, int64_t *n_out) {
    using namespace qpsk;
    int rc;
    if ((rc = qpsk_pfb_state_check(p, n_bands, state, state_bytes))) return rc;
    const int M = p->channels, K = p->taps_per_branch, L = M * K;
    if (taps && (rc = pfb_check_taps(taps, L, L))) return rc;
    const int64_t each = pfb_state_bytes(M, K);
    char *rec = static_cast<char *>(state);
    std::vector<PfbHead> heads(n_bands);
    for (int32_t b = 0; b < n_bands; ++b) std::memcpy(&heads[b], rec + b * each, sizeof(PfbHead));
    if (!n_out) return fail(QPSK_ERR_ARGUMENT_NULL, "n_out is null");
    int64_t n_call, n_out_max;
    std::vector<int64_t> cnt(n_bands);   // n_out is written once nothing can refuse the call any more
    if ((rc = pfb_check_call(*p, heads.data(), n_bands, stride_in, stride_out, out_cap, n_samples, lengths, cnt.data(),
                             &n_call, &n_out_max)))
        return rc;
    if (n_call > 0 && !in) return fail(QPSK_ERR_ARGUMENT_NULL, "in is null");
    if (n_out_max > 0 && !out) return fail(QPSK_ERR_ARGUMENT_NULL, "out is null");
    if (n_call > 0 && n_out_max > 0 &&
        rows_overlap(in, n_bands, stride_in, n_samples, sizeof(float), out, static_cast<int64_t>(n_bands) * M, stride_out,
                     out_cap, sizeof(float)))
        return fail(QPSK_ERR_ARGUMENT, "out must not overlap in");
    std::vector<float> h(L), w(M), hist(2 * static_cast<size_t>(L));
    if (taps) std::memcpy(h.data(), taps, sizeof(float) * L);
    else pfb_design(M, K, h.data());
    pfb_twiddles(M, w.data());
    std::memcpy(n_out, cnt.data(), sizeof(int64_t) * n_bands);
    for (int32_t b = 0; b < n_bands; ++b) {
        // the history through a copy: a blob need not be aligned for floats
        std::memcpy(hist.data(), rec + b * each + sizeof(PfbHead), sizeof(float) * hist.size());
        pfb_apply_band(*p, h.data(), w.data(), heads[b], hist.data(), in ? in + b * stride_in : nullptr,
                       lengths ? lengths[b] : n_samples, out ? out + static_cast<int64_t>(b) * M * stride_out : nullptr,
                       stride_out);
        std::memcpy(rec + b * each, &heads[b], sizeof(PfbHead));
        std::memcpy(rec + b * each + sizeof(PfbHead), hist.data(), sizeof(float) * hist.size());
    }
    return QPSK_OK;
}

}  // extern "C"
