// qpsk_row_call.h -- what the test-bench stages that take rows of samples and
// keep a state per row (the channel, the propagation path, the polyphase
// channeliser) check of a call on the CPU side, once: the lengths, the counts a
// call would emit, whether two sets of rows overlap, and a state blob's length.
// A stage composes them with its own checks in its own order ("The
// test-bench stages' shared pieces").  No HIP and nothing to link beyond
// qpsk_error.cpp: the host forms (qpsk_path.cpp, qpsk_pfb.cpp), the device
// entry points and the stand-alone CPU programs under tools/ all include it.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "qpsk_demod.h"
#include "qpsk_internal.h"

namespace qpsk {

// lengths, where given, within [0, n_samples]; *n_call is the longest row
inline int check_lengths(int rows, int64_t n_samples, const int64_t *lengths, int64_t *n_call) {
    *n_call = lengths ? 0 : n_samples;
    if (lengths)
        for (int s = 0; s < rows; ++s) {
            if (lengths[s] < 0 || lengths[s] > n_samples)
                return fail(QPSK_ERR_ARGUMENT, "lengths[" + std::to_string(s) + "] = " + std::to_string(lengths[s]) +
                                                   " outside [0, n_samples]");
            *n_call = lengths[s] > *n_call ? lengths[s] : *n_call;
        }
    return QPSK_OK;
}

// What each row would emit: count(recs[s], in_end) of a record with in_pos and
// out_pos.  No row may pass max_pos or emit more than out_cap.  The counts go
// into a copy first: a rejected call leaves n_out as it was.  `row` and `unit`
// are the stage's words ("stream" and "samples", "band" and "frames").
template <typename Rec, typename Count>
int check_counts(const Rec *recs, int rows, int64_t n_samples, const int64_t *lengths, int64_t out_cap, int64_t max_pos,
                 const char *row, const char *unit, Count count, int64_t *n_out, int64_t *n_out_max) {
    std::vector<int64_t> cnt(rows);
    *n_out_max = 0;
    for (int s = 0; s < rows; ++s) {
        const int64_t len = lengths ? lengths[s] : n_samples;
        if (len > max_pos - recs[s].in_pos)
            return fail(QPSK_ERR_ARGUMENT, std::string(row) + " " + std::to_string(s) + " would pass position 2^50");
        cnt[s] = count(recs[s], recs[s].in_pos + len);
        if (cnt[s] > out_cap)
            return fail(QPSK_ERR_ARGUMENT, std::string(row) + " " + std::to_string(s) + " would emit " +
                                               std::to_string(cnt[s]) + " " + unit + ", out_cap is " + std::to_string(out_cap));
        *n_out_max = cnt[s] > *n_out_max ? cnt[s] : *n_out_max;
    }
    std::memcpy(n_out, cnt.data(), sizeof(int64_t) * rows);
    return QPSK_OK;
}

// the records behind a call that was accepted: each row took its length and
// emitted its count
template <typename Rec>
void advance_rows(Rec *recs, int rows, int64_t n_samples, const int64_t *lengths, const int64_t *cnt) {
    for (int s = 0; s < rows; ++s) {
        recs[s].in_pos += lengths ? lengths[s] : n_samples;
        recs[s].out_pos += cnt[s];
    }
}

// whether `rows` rows of n samples, stride elements of elem_bytes apart, share a
// byte with the other set
inline bool rows_overlap(const void *a, int64_t rows_a, int64_t stride_a, int64_t n_a, int64_t elem_a, const void *b,
                         int64_t rows_b, int64_t stride_b, int64_t n_b, int64_t elem_b) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    const uintptr_t a1 = a0 + static_cast<uintptr_t>(((rows_a - 1) * stride_a + 2 * n_a) * elem_a);
    const uintptr_t b1 = b0 + static_cast<uintptr_t>(((rows_b - 1) * stride_b + 2 * n_b) * elem_b);
    return a0 < b1 && b0 < a1;
}

// a state blob of `got` bytes against the `want` bytes of a handle of `stage`
inline int check_state_bytes(const char *stage, int64_t got, int64_t want) {
    if (got == want) return QPSK_OK;
    return fail(QPSK_ERR_ARGUMENT, std::string(stage) + " state length does not match this handle (" +
                                       std::to_string(got) + " vs " + std::to_string(want) + " bytes)");
}

}  // namespace qpsk
