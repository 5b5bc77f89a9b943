// qpsk_sfb.cpp -- the host half of the polyphase synthesis bank
// (include/qpsk_demod.h, "The polyphase synthesis bank on the device"): the
// parameter defaults and checks, the checks of a call, qpsk_sfb_tile_frames,
// qpsk_sfb_state_check, which qpsk_sfb_set_state runs on a blob before anything
// reaches the device, and qpsk_sfb_apply_host, the call itself on host rows.
// The prototype and the twiddles are the channeliser's (qpsk_pfb.cpp).  No HIP,
// no device: a stand-alone CPU program links this file, qpsk_pfb.cpp and
// qpsk_error.cpp (tools/sfb_main.cpp runs it under the sanitizers).
#include "qpsk_sfb.h"

#include <cstring>
#include <string>
#include <vector>

#include "qpsk_demod.h"
#include "qpsk_internal.h"
#include "qpsk_row_call.h"

namespace qpsk {
namespace {

bool plus_zero(float v) {
    uint32_t u;
    std::memcpy(&u, &v, sizeof(u));
    return u == 0;
}

int bad_field(int b, const std::string &field, const std::string &value, const std::string &range) {
    return fail(QPSK_ERR_ARGUMENT, "sfb state band " + std::to_string(b) + ": " + field + " = " + value + " outside " +
                                       range);
}

// the limits are the channeliser's: its check on its own record
int check_shape(int M, int K, int32_t n_bands) {
    qpsk_pfb_params q{};
    q.channels = M;
    q.taps_per_branch = K;
    q.gain = 1.0f;
    return pfb_check_params(&q, n_bands);
}

int check_band(const qpsk_sfb_params &p, int b, const char *rec) {
    const int M = p.channels, H = sfb_hist_frames(p.taps_per_branch);
    SfbHead hd;
    std::memcpy(&hd, rec, sizeof(hd));
    if (hd.in_pos < 0 || hd.in_pos > sfb_max_frames(M))
        return bad_field(b, "in_pos", std::to_string(hd.in_pos), "[0, 2^50 / D]");
    const int64_t want = sfb_emitted(M, hd.in_pos);
    if (hd.out_pos != want)
        return bad_field(b, "out_pos", std::to_string(hd.out_pos), "in_pos * D = " + std::to_string(want));
    for (size_t k = 0; k < sizeof(hd.reserved); ++k)
        if (hd.reserved[k]) return bad_field(b, "reserved", std::to_string(hd.reserved[k]), "[0, 0]");
    // frames before the band's start
    const int64_t before = hd.in_pos < H ? H - hd.in_pos : 0;
    for (int64_t h = 0; h < before * M; ++h) {
        float v[2];
        std::memcpy(v, rec + sizeof(SfbHead) + 8 * h, sizeof(v));
        if (!(plus_zero(v[0]) && plus_zero(v[1])))
            return bad_field(b, "hist[" + std::to_string(h / M) + "][" + std::to_string(h % M) + "]",
                             std::to_string(v[0]) + ", " + std::to_string(v[1]), "+0 (a frame before the band's start)");
    }
    return QPSK_OK;
}

}  // namespace

int sfb_check_params(const qpsk_sfb_params *p, int32_t n_bands) {
    if (!p) return fail(QPSK_ERR_ARGUMENT_NULL, "sfb params are null");
    return check_shape(p->channels, p->taps_per_branch, n_bands);
}

int sfb_check_call(const qpsk_sfb_params &p, const SfbHead *heads, int32_t B, int64_t stride_in, int64_t stride_out,
                   int64_t n_frames, const int64_t *lengths, int64_t *n_call) {
    const int M = p.channels;
    const int64_t D = M / 2;
    if (n_frames < 0) return fail(QPSK_ERR_ARGUMENT, "n_frames must not be negative");
    if (n_frames > sfb_max_frames(M)) return fail(QPSK_ERR_ARGUMENT, "stride too small");
    int rc;
    if ((rc = check_lengths(B, n_frames, lengths, n_call))) return rc;
    if (*n_call > 0 && (stride_in < 2 * n_frames || stride_out < 2 * n_frames * D))
        return fail(QPSK_ERR_ARGUMENT, "stride too small");
    for (int b = 0; b < B; ++b)
        if ((lengths ? lengths[b] : n_frames) > sfb_max_frames(M) - heads[b].in_pos)
            return fail(QPSK_ERR_ARGUMENT, "band " + std::to_string(b) + " would pass position 2^50");
    return QPSK_OK;
}

void sfb_apply_band(int M, int K, const float *g, const float *w, SfbHead &head, float *hist, const float *in,
                    int64_t stride_in, int64_t len, float *out, float scale_out) {
    const int D = M / 2, H = sfb_hist_frames(K), bits = pfb_log2(M), ring = 2 * K;
    const int64_t in_pos = head.in_pos;
    if (len == 0) return;
    // row c's sample of the call's frame t: the call's rows, or the history in front of them
    auto s_at = [&](int c, int64_t t) {
        if (t >= 0) return PfbC{in[c * stride_in + 2 * t], in[c * stride_in + 2 * t + 1]};
        const int64_t h = (H + t) * M + c;
        return PfbC{hist[2 * h], hist[2 * h + 1]};
    };
    // u of the last 2K frames, frame t at slot (t + H) mod 2K
    std::vector<PfbC> u(static_cast<size_t>(ring) * M);
    for (int64_t t = -H; t < len; ++t) {
        PfbC *a = u.data() + static_cast<size_t>((t + H) % ring) * M;
        for (int c = 0; c < M; ++c) a[pfb_bitrev(c, bits)] = sfb_input(s_at(c, t), c, in_pos + t);
        for (int half = 1; half < M; half *= 2)
            for (int j0 = 0; j0 < M; j0 += 2 * half)
                for (int j = 0; j < half; ++j) {
                    const int q = j * (M / (2 * half));
                    pfb_butterfly(a[j0 + j], a[j0 + j + half], w[2 * q], w[2 * q + 1]);
                }
        if (t < 0) continue;
        // a frame before the band's start is a transform of +0: zeros, which add nothing
        for (int r = 0; r < D; ++r) {
            PfbC acc{0.0f, 0.0f};
            for (int j = 0; j < 2 * K; ++j)
                sfb_step(acc, g[j * D + r], u[static_cast<size_t>((t - j + H) % ring) * M + sfb_index(M, r, j)]);
            out[2 * (t * D + r)] = quant_scaled(acc.re, scale_out);
            out[2 * (t * D + r) + 1] = quant_scaled(acc.im, scale_out);
        }
    }
    std::vector<float> next(2 * static_cast<size_t>(H) * M);
    for (int k = 0; k < H; ++k)
        for (int c = 0; c < M; ++c) {
            const PfbC s = s_at(c, len - H + k);
            next[2 * (static_cast<size_t>(k) * M + c)] = s.re, next[2 * (static_cast<size_t>(k) * M + c) + 1] = s.im;
        }
    std::memcpy(hist, next.data(), sizeof(float) * next.size());
    head.in_pos = in_pos + len;
    head.out_pos += sfb_emitted(M, len);
}

}  // namespace qpsk

extern "C" {

void qpsk_sfb_params_init(qpsk_sfb_params *p) {
    if (!p) return;
    *p = qpsk_sfb_params{};
    p->channels = 64;
    p->taps_per_branch = 8;
}

int qpsk_sfb_tile_frames(int32_t channels, int32_t taps_per_branch, int32_t which) {
    using namespace qpsk;
    int rc;
    if ((rc = check_shape(channels, taps_per_branch, 1))) return rc;
    switch (which) {
    case QPSK_SFB_TILE_TRANSFORM: return sfb_transform_tile(channels, taps_per_branch);
    case QPSK_SFB_TILE_SUM: return kSfbSumRun;
    case QPSK_SFB_TILE_SLAB: return static_cast<int>(sfb_slab_frames(channels, 1));
    default: return fail(QPSK_ERR_ARGUMENT, "which must be one of QPSK_SFB_TILE_*");
    }
}

int64_t qpsk_sfb_state_size(const qpsk_sfb_params *p) {
    int rc;
    if ((rc = qpsk::sfb_check_params(p, 1))) return rc;
    return qpsk::sfb_state_bytes(p->channels, p->taps_per_branch);
}

int qpsk_sfb_state_init(const qpsk_sfb_params *p, int32_t n_bands, void *buf, int64_t buf_bytes) {
    using namespace qpsk;
    int rc;
    if ((rc = sfb_check_params(p, n_bands))) return rc;
    if (!buf) return fail(QPSK_ERR_ARGUMENT_NULL, "sfb state buffer is null");
    if (buf_bytes != n_bands * sfb_state_bytes(p->channels, p->taps_per_branch))
        return fail(QPSK_ERR_ARGUMENT, "sfb state length does not match n_bands");
    std::memset(buf, 0, buf_bytes);
    return QPSK_OK;
}

int qpsk_sfb_state_check(const qpsk_sfb_params *p, int32_t n_bands, const void *buf, int64_t buf_bytes) {
    using namespace qpsk;
    int rc;
    if ((rc = sfb_check_params(p, n_bands))) return rc;
    if (!buf) return fail(QPSK_ERR_ARGUMENT_NULL, "sfb state buffer is null");
    const int64_t each = sfb_state_bytes(p->channels, p->taps_per_branch);
    if ((rc = check_state_bytes("sfb", buf_bytes, n_bands * each))) return rc;
    const char *rec = static_cast<const char *>(buf);
    for (int32_t b = 0; b < n_bands; ++b, rec += each)
        if ((rc = check_band(*p, b, rec))) return rc;
    return QPSK_OK;
}

int qpsk_sfb_apply_host(const qpsk_sfb_params *p, const float *taps, void *state, int64_t state_bytes, int32_t n_bands,
                        const float *in, int64_t stride_in, float *out, int64_t stride_out, float scale_out,
                        int64_t n_frames, const int64_t *lengths) {
    using namespace qpsk;
    int rc;
    if ((rc = qpsk_sfb_state_check(p, n_bands, state, state_bytes))) return rc;
    const int M = p->channels, K = p->taps_per_branch, L = M * K, D = M / 2;
    if (taps && (rc = pfb_check_taps(taps, L, L))) return rc;
    if (!quant_scale_ok(scale_out)) return fail(QPSK_ERR_OUT_OF_RANGE, "scale_out must be finite and > 0");
    const int64_t each = sfb_state_bytes(M, K);
    char *rec = static_cast<char *>(state);
    std::vector<SfbHead> heads(n_bands);
    for (int32_t b = 0; b < n_bands; ++b) std::memcpy(&heads[b], rec + b * each, sizeof(SfbHead));
    int64_t n_call;
    if ((rc = sfb_check_call(*p, heads.data(), n_bands, stride_in, stride_out, n_frames, lengths, &n_call))) return rc;
    if (n_call == 0) return QPSK_OK;   // nothing taken: nothing emitted, no state moves
    if (!in || !out) return fail(QPSK_ERR_ARGUMENT_NULL, "in or out is null");
    if (rows_overlap(in, static_cast<int64_t>(n_bands) * M, stride_in, n_frames, sizeof(float), out, n_bands, stride_out,
                     n_frames * D, sizeof(float)))
        return fail(QPSK_ERR_ARGUMENT, "out must not overlap in");
    std::vector<float> g(L), w(M), hist(2 * static_cast<size_t>(M) * sfb_hist_frames(K));
    if (taps) std::memcpy(g.data(), taps, sizeof(float) * L);
    else pfb_design(M, K, g.data());
    pfb_twiddles(M, w.data());
    for (int32_t b = 0; b < n_bands; ++b) {
        // the history through a copy: a blob need not be aligned for floats
        std::memcpy(hist.data(), rec + b * each + sizeof(SfbHead), sizeof(float) * hist.size());
        sfb_apply_band(M, K, g.data(), w.data(), heads[b], hist.data(), in + static_cast<int64_t>(b) * M * stride_in,
                       stride_in, lengths ? lengths[b] : n_frames, out + b * stride_out, scale_out);
        std::memcpy(rec + b * each, &heads[b], sizeof(SfbHead));
        std::memcpy(rec + b * each + sizeof(SfbHead), hist.data(), sizeof(float) * hist.size());
    }
    return QPSK_OK;
}

}  // extern "C"
