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

}  // namespace qpsk
