// qpsk_state_blob.cpp -- qpsk_state_blob_check: what a state blob must satisfy
// before qpsk_demod_set_state copies it to the device; and the rows of
// selected streams as a blob of their own (qpsk_stream_list_check,
// qpsk_state_blob_select, qpsk_state_blob_merge).  Host-only (no HIP): a
// stand-alone CPU program links this file, qpsk_error.cpp and qpsk_design.cpp
// (tools/state_blob_check_main.cpp and tools/state_blob_rows_main.cpp run it
// under the sanitizers).
//
// A blob is external input.  The kernels take a record's integers, and the
// timing phase, as addresses without looking at them, so each such field is
// held to the range a finished call can itself leave (derivations below, and
// DESIGN.md "State blob").  Every other float is data: whatever the reference
// can hold is accepted, NaN and Inf included.
#include "qpsk_state_blob.h"

#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "qpsk_demod.h"
#include "qpsk_design.h"
#include "qpsk_internal.h"

namespace qpsk {
namespace {

int bad_field(int s, const char *field, const std::string &value, const std::string &range) {
    return fail(QPSK_ERR_ARGUMENT, "state blob stream " + std::to_string(s) + ": " + field + " = " + value +
                                       " outside " + range);
}

template <typename I>
int check_int(int s, const char *field, I v, int64_t lo, int64_t hi) {
    if (static_cast<int64_t>(v) >= lo && static_cast<int64_t>(v) <= hi) return QPSK_OK;
    return bad_field(s, field, std::to_string(v), "[" + std::to_string(lo) + ", " + std::to_string(hi) + "]");
}

}  // namespace

int state_blob_check(int32_t S, int32_t T, double sps, const void *buf, int64_t buf_bytes) {
    if (!buf || S <= 0 || T <= 0) return fail(QPSK_ERR_ARGUMENT, "state blob check: null buffer or empty shape");
    // the length first: nothing below reads past it
    const int64_t want_bytes = state_blob_bytes(S, T);
    if (buf_bytes != want_bytes)
        return fail(QPSK_ERR_ARGUMENT, "state blob length does not match this handle (" +
                                           std::to_string(buf_bytes) + " vs " + std::to_string(want_bytes) +
                                           " bytes)");
    const StateHeader want = state_header(S, T);
    StateHeader got;
    std::memcpy(&got, buf, sizeof(got));
    if (got.magic != want.magic || got.format != want.format)
        return fail(QPSK_ERR_ARGUMENT, "not a state blob of this library version (format " +
                                           std::to_string(got.format) + ", expected " +
                                           std::to_string(want.format) + ")");
    if (got.streams != want.streams || got.taps != want.taps || got.carry_max != want.carry_max ||
        got.fll_taps != want.fll_taps || got.record_bytes != want.record_bytes)
        return fail(QPSK_ERR_ARGUMENT, "state blob layout (streams, taps, carry, record size) does not "
                                       "match this handle");

    // base: the M&M loop runs while base + 2 < count (qpsk_loop.hip, more();
    // MuellerMuller.cs:66) and each symbol moves the time base + mu, mu < 1, on
    // by at most sps + 0.1 (the clamped correction).  The last symbol of a call
    // starts at base <= count - 3, so the loop exits with count - 2 <= base <=
    // count - 2 + ceil(sps + 0.1) (the ceiling also covers the sum's rounding).
    // The drop rule (qpsk_loop.hip "drop consumed samples", MuellerMuller.cs:
    // 123-133) then takes min(base - 1, count - 3) samples away: count - 3 of
    // them here, which leaves 1 <= base <= 1 + ceil(sps + 0.1).  A call that
    // stops at the output capacity leaves base = 1; one too short to step
    // leaves base where it was or moves it down to no less than 1.  The
    // reference's NaN timing pins baseIndex at (int)Math.Floor(NaN) = 0
    // (MuellerMuller.cs:113-115), which the drop rule keeps: 0 is the lower
    // end.  (A carry overflow, error bit 0, may leave base below 0: that stream
    // has lost samples, its call returned QPSK_ERR_STATE, and the record is no
    // state of the reference; it is rejected.)
    const double base_hi = 1.0 + std::ceil(sps + 0.1);

    const char *rec = static_cast<const char *>(buf) + sizeof(StateHeader);
    for (int32_t s = 0; s < S; ++s, rec += sizeof(StreamState)) {
        StreamState st;
        std::memcpy(&st, rec, sizeof(st));
        int rc;
        // carry_n entries of the carry are copied to mf + kMfPrefix - carry_n
        // (carry_prefix_kernel) and the loop's tail reads from there: the carry
        // array and the MF prefix both hold kCarryMax = kMfPrefix samples
        if ((rc = check_int(s, "carry_n", st.carry_n, 0, kCarryMax))) return rc;
        // both FLL kernels write delay[fll_pos] and delay[fll_pos + kFllTaps] of
        // a 2 kFllTaps line and wrap the position at kFllTaps only
        if ((rc = check_int(s, "fll_pos", st.fll_pos, 0, kFllTaps - 1))) return rc;
        // the queue offset inside a call split into internal chunks; the call's
        // last chunk resets it, and a blob is taken between calls (get_state
        // waits for the queued ones)
        if ((rc = check_int(s, "tofs", st.tofs, 0, 0))) return rc;
        // the loop stores has_prev as it loaded it or 1, diff_have likewise
        if ((rc = check_int(s, "has_prev", st.has_prev, 0, 1))) return rc;
        if ((rc = check_int(s, "diff_have", st.diff_have, 0, 1))) return rc;
        // sticky bits the loop kernel ORs in: 1 = carry overflow (M&M wave),
        // 2 = an output row was truncated (decode wave)
        if ((rc = check_int(s, "error", st.error, 0, 3))) return rc;
        if (!(static_cast<double>(st.base) >= 0.0 && static_cast<double>(st.base) <= base_hi))
            return bad_field(s, "base", std::to_string(st.base),
                             "[0, " + std::to_string(static_cast<int64_t>(std::fmin(base_hi, 2147483647.0))) + "]");
        // mu: the loop stores nt - floor(nt) of a finite nt (the correction is
        // clamped, a NaN one included), exact and in [+0, 1); the tap address is
        // formed from floor(base + mu), and a NaN's payload would become one
        if (!(st.mu >= 0.0 && st.mu < 1.0) || std::signbit(st.mu))
            return bad_field(s, "mu", std::to_string(st.mu) + (std::signbit(st.mu) ? " (sign bit set)" : ""),
                             "[+0, 1)");
    }
    return QPSK_OK;
}

int stream_list_check(int32_t S, const int32_t *streams, int32_t n) {
    if (!streams) return fail(QPSK_ERR_ARGUMENT_NULL, "stream list is null");
    if (S <= 0 || n < 1 || n > S)
        return fail(QPSK_ERR_ARGUMENT, "stream list: n = " + std::to_string(n) + " outside [1, " + std::to_string(S) +
                                           "] (the streams of the batch)");
    std::vector<int32_t> first(static_cast<size_t>(S), -1);   // position an index was first seen at
    for (int32_t i = 0; i < n; ++i) {
        const int32_t v = streams[i];
        if (v < 0 || v >= S)
            return fail(QPSK_ERR_ARGUMENT, "stream list position " + std::to_string(i) + ": index " + std::to_string(v) +
                                               " outside [0, " + std::to_string(S) + ")");
        if (first[v] >= 0)
            return fail(QPSK_ERR_ARGUMENT, "stream list position " + std::to_string(i) + ": index " + std::to_string(v) +
                                               " repeated (first at position " + std::to_string(first[v]) + ")");
        first[v] = i;
    }
    return QPSK_OK;
}

namespace {

// One section after the other: row src_row(i) of the section in `from` (a
// blob of S_from streams) to row dst_row(i) of the section in `to`.
template <typename SrcRow, typename DstRow>
void copy_rows(int32_t T, const char *from, int64_t S_from, char *to, int64_t S_to, int32_t n, SrcRow src_row,
               DstRow dst_row) {
    int64_t words[kStateSections];
    state_row_words(T, words);
    from += sizeof(StateHeader);
    to += sizeof(StateHeader);
    for (int k = 0; k < kStateSections; ++k) {
        const int64_t row = 8 * words[k];
        for (int32_t i = 0; i < n; ++i) std::memcpy(to + dst_row(i) * row, from + src_row(i) * row, row);
        from += S_from * row;
        to += S_to * row;
    }
}

}  // namespace

void state_blob_gather_rows(int32_t S, int32_t T, const void *blob, const int32_t *streams, int32_t n, void *sub) {
    const StateHeader hd = state_header(n, T);
    std::memcpy(sub, &hd, sizeof(hd));
    copy_rows(T, static_cast<const char *>(blob), S, static_cast<char *>(sub), n, n,
              [&](int32_t i) { return static_cast<int64_t>(streams[i]); }, [](int32_t i) { return static_cast<int64_t>(i); });
}

void state_blob_scatter_rows(int32_t S, int32_t T, void *blob, const int32_t *streams, int32_t n, const void *sub) {
    copy_rows(T, static_cast<const char *>(sub), n, static_cast<char *>(blob), S, n,
              [](int32_t i) { return static_cast<int64_t>(i); }, [&](int32_t i) { return static_cast<int64_t>(streams[i]); });
}

namespace {

// the tap count and the M&M samples per symbol of p, as qpsk_demod_design
int shape_of(const qpsk_demod_params *p, const char *who, int32_t *T, double *sps) {
    LoopDesign d;
    std::string err;
    if (design_loops(p->sample_rate, p->symbol_rate, p->rrc_alpha, p->rrc_span, p->symbol_sync_bandwidth,
                     p->costas_loop_bandwidth, p->cfo_loop_bandwidth, &d, &err) != QPSK_OK)
        return fail(QPSK_ERR_ARGUMENT, std::string(who) + ": " + err);
    *T = static_cast<int32_t>(d.rrc_f32.size());
    *sps = d.mm_sps;
    return QPSK_OK;
}

}  // namespace

}  // namespace qpsk

extern "C" int qpsk_stream_list_check(int32_t n_streams, const int32_t *streams, int32_t n) {
    return qpsk::stream_list_check(n_streams, streams, n);
}

extern "C" int qpsk_state_blob_select(const qpsk_demod_params *p, int32_t n_streams, const void *blob,
                                      int64_t blob_bytes, const int32_t *streams, int32_t n, void *sub,
                                      int64_t sub_bytes) {
    using namespace qpsk;
    if (!p || !blob || !streams || !sub) return fail(QPSK_ERR_ARGUMENT_NULL, "state blob select: null argument");
    int rc;
    int32_t T;
    double sps;
    if ((rc = stream_list_check(n_streams, streams, n)) || (rc = shape_of(p, "state blob select", &T, &sps)) ||
        (rc = state_blob_check(n_streams, T, sps, blob, blob_bytes)))
        return rc;
    if (sub_bytes != state_blob_bytes(n, T))
        return fail(QPSK_ERR_ARGUMENT, "state blob select: the sub-blob buffer holds " + std::to_string(sub_bytes) +
                                           " bytes, " + std::to_string(n) + " streams take " +
                                           std::to_string(state_blob_bytes(n, T)));
    state_blob_gather_rows(n_streams, T, blob, streams, n, sub);
    return QPSK_OK;
}

extern "C" int qpsk_state_blob_merge(const qpsk_demod_params *p, int32_t n_streams, void *blob, int64_t blob_bytes,
                                     const int32_t *streams, int32_t n, const void *sub, int64_t sub_bytes) {
    using namespace qpsk;
    if (!p || !blob || !streams || !sub) return fail(QPSK_ERR_ARGUMENT_NULL, "state blob merge: null argument");
    int rc;
    int32_t T;
    double sps;
    // every check before the first byte moves: a rejected call changes nothing
    if ((rc = stream_list_check(n_streams, streams, n)) || (rc = shape_of(p, "state blob merge", &T, &sps)) ||
        (rc = state_blob_check(n, T, sps, sub, sub_bytes)) ||
        (rc = state_blob_check(n_streams, T, sps, blob, blob_bytes)))
        return rc;
    state_blob_scatter_rows(n_streams, T, blob, streams, n, sub);
    return QPSK_OK;
}

extern "C" int qpsk_state_blob_check(const qpsk_demod_params *p, int32_t n_streams, const void *buf,
                                     int64_t buf_bytes) {
    using namespace qpsk;
    if (!p || !buf) return fail(QPSK_ERR_ARGUMENT, "state blob check: null argument");
    if (n_streams <= 0) return fail(QPSK_ERR_ARGUMENT, "state blob check: n_streams must be > 0");
    LoopDesign d;
    std::string err;
    if (design_loops(p->sample_rate, p->symbol_rate, p->rrc_alpha, p->rrc_span, p->symbol_sync_bandwidth,
                     p->costas_loop_bandwidth, p->cfo_loop_bandwidth, &d, &err) != QPSK_OK)
        return fail(QPSK_ERR_ARGUMENT, "state blob check: " + err);
    return state_blob_check(n_streams, static_cast<int32_t>(d.rrc_f32.size()), d.mm_sps, buf, buf_bytes);
}
