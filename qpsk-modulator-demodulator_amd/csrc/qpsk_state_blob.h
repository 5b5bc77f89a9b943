// qpsk_state_blob.h -- the layout of a qpsk_demod_get_state blob and the host
// check every blob passes before set_state copies it to the device
// (qpsk_state_blob.cpp: host-only, no HIP).
//
// Format 2: a header naming the layout, then the per-stream records, the M&M
// carries, the FIR histories and the FLL delay lines.  Format 1 (round 3 and
// before) had no header and a 64-sample carry.
#pragma once
#include <cstdint>

#include "qpsk_state.h"

namespace qpsk {

constexpr uint32_t kStateMagic = 0x4b535051u;   // "QPSK"
constexpr uint32_t kStateFormat = 2;
struct StateHeader {
    uint32_t magic, format;
    int32_t streams, taps, carry_max, fll_taps, record_bytes, reserved;
};
static_assert(sizeof(StateHeader) == 32, "state blob header");

inline StateHeader state_header(int32_t S, int32_t T) {
    return StateHeader{kStateMagic, kStateFormat, S, T, kCarryMax, kFllTaps,
                       static_cast<int32_t>(sizeof(StreamState)), 0};
}

// S streams of a T-tap matched filter
inline int64_t state_blob_bytes(int64_t S, int64_t T) {
    return static_cast<int64_t>(sizeof(StateHeader)) +
           S * (static_cast<int64_t>(sizeof(StreamState)) + 8 * kCarryMax + 8 * (T - 1) + 8 * 2 * kFllTaps);
}

// The checks of qpsk_state_blob_check once the tap count T and the M&M samples
// per symbol are known.  QPSK_OK or QPSK_ERR_ARGUMENT (message in qpsk_last_error).
int state_blob_check(int32_t S, int32_t T, double sps, const void *buf, int64_t buf_bytes);

// Rows of selected streams.  The rows of n streams, laid out as header,
// records, carries, histories and delay lines, are a format-2 blob of an
// n-stream handle with the same tap count (a "sub-blob").
//
// The 8-byte words of one stream's row in each of the four sections
constexpr int kStateSections = 4;
inline void state_row_words(int32_t T, int64_t words[kStateSections]) {
    words[0] = static_cast<int64_t>(sizeof(StreamState)) / 8;
    words[1] = kCarryMax;
    words[2] = T - 1;
    words[3] = 2 * kFllTaps;
}
static_assert(sizeof(StreamState) % 8 == 0, "a record is moved in 8-byte words");
// 1 <= n <= S, every index in [0, S), none twice; else QPSK_ERR_ARGUMENT
// naming the position and the value
int stream_list_check(int32_t S, const int32_t *streams, int32_t n);
// Row i of the n-stream blob sub <- row streams[i] of the S-stream blob, and
// sub's header (gather); row streams[i] of blob <- row i of sub (scatter).
// Both blobs hold T taps and their exact lengths, and the list has passed
// stream_list_check: nothing is checked here.
void state_blob_gather_rows(int32_t S, int32_t T, const void *blob, const int32_t *streams, int32_t n, void *sub);
void state_blob_scatter_rows(int32_t S, int32_t T, void *blob, const int32_t *streams, int32_t n, const void *sub);

}  // namespace qpsk
