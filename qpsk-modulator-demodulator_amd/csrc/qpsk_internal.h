// qpsk_internal.h -- what the host code behind the C ABI shares between its
// translation units: the error channel, the per-call argument check and the
// few things the ring (qpsk_rx.hip) and the group (qpsk_group.cpp) need from a
// handle.  Private and host-only; the error channel is defined in
// qpsk_error.cpp (no HIP), the rest in qpsk_runtime.hip.
#pragma once
#include <cstdint>
#include <string>

#include "qpsk_demod.h"

namespace qpsk {

// msg becomes the calling thread's qpsk_last_error; returns code
int fail(int code, const std::string &msg);

// One call as its caller gave it (the arguments of qpsk_demod_process).
struct CallArgs {
    int32_t mode;
    const void *iq;          // float rows, int16 rows (CS16) or byte rows (CS8 / CU8)
    int64_t stride_floats;   // row stride in elements of iq: two per sample in every format
    int64_t n_samples;
    const int64_t *lengths;
    int32_t mem;
    uint8_t *bits;
    int64_t bits_stride_bytes;
    int64_t *n_bits;
    float *syms;
    int64_t syms_stride_floats;
    int64_t *n_syms;
    int32_t fmt = 0;         // QPSK_FMT_* (= kFmt*, qpsk_kernels.h)
    int64_t n_call = 0;      // derived by check_call: the longest row, and
    int64_t max_sym = 0;     // qpsk_demod_max_symbols of it
};

// The longest of a call's S rows (n_samples, or the largest of lengths); a
// negative count is QPSK_ERR_ARGUMENT.
int call_length(int S, int64_t n_samples, const int64_t *lengths, int64_t *n_call);
// The checks every call over S rows makes before anything is launched, copied
// or allocated, in one order and with one text per rule: the format, mode, mem,
// call_length, the sample limit, iq and its stride, the outputs the mode needs
// and their strides, and what device rows must satisfy.  h gives the symbol
// bound (a group's shards share it).  Fills c.n_call and c.max_sym.
int check_call(const qpsk_demod *h, int S, CallArgs &c);

int handle_streams(const qpsk_demod *h);
int64_t handle_max_samples(const qpsk_demod *h);
int handle_device(const qpsk_demod *h);
int handle_taps(const qpsk_demod *h);   // of the matched filter
// the host waits for every call queued on the handle, pipelined or stream-ordered
int handle_sync(qpsk_demod *h);

}  // namespace qpsk

#ifdef __HIP__   // qpsk_group.cpp is plain C++
#include <hip/hip_runtime.h>

#include "qpsk_device.h"

namespace qpsk {
// the pipelined path's front-stage stream (qpsk_rx.hip records "input consumed"
// on it); nullptr before the first pipelined call
hipStream_t pipe_front_stream(const qpsk_demod *h);

// What the rows of selected streams (qpsk_stream_state.hip) need from a handle:
// its shape and stream, the four per-stream arrays of a state blob (hist: the
// current one of the ping-pong pair, good until the next call is issued), the
// link sums (nullptr until first enabled) and the staging buffer it keeps for
// them, a member of the handle like its other buffers.
struct StreamState;
struct LinkAcc;
struct StreamRows {
    const qpsk_demod_params *p;
    int S, T;
    hipStream_t stream;
    StreamState *state;
    float *carry, *hist, *fll_delay;
    LinkAcc *link;
    DevBuf<char> *staging;
};
StreamRows handle_rows(qpsk_demod *h);
}  // namespace qpsk

#define QPSK_HIP_TRY(expr)                                                                    \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return ::qpsk::fail(QPSK_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
#endif
