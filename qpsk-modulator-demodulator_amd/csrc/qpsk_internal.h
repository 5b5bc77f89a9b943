// qpsk_internal.h -- what the host code behind the C ABI shares between its
// translation units: the error channel, the per-call argument check and the
// two things the plain-C++ group (qpsk_group.cpp) needs from a handle it
// cannot see (HIP files include qpsk_handle.h and read the members).  Private
// and host-only; the error channel is defined in qpsk_error.cpp (no HIP), the
// rest in qpsk_runtime.hip.
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
    int32_t fmt = 0;         // QPSK_FMT_*
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

int handle_taps(const qpsk_demod *h);   // of the matched filter
// the host waits for every call queued on the handle, pipelined or stream-ordered
int handle_sync(qpsk_demod *h);

}  // namespace qpsk

#ifdef __HIP__   // qpsk_group.cpp is plain C++
#include <hip/hip_runtime.h>

namespace qpsk {
// The status of a device allocation (a DevBuf's alloc or grow).  Without a
// label the text carries HIP's own: "hipMalloc: <error>"; with one it names
// what was being made: "hipMalloc (<label>)".
inline int alloc_status(hipError_t e, const char *label = nullptr) {
    if (e == hipSuccess) return QPSK_OK;
    return fail(QPSK_ERR_DEVICE, label ? std::string("hipMalloc (") + label + ")"
                                       : std::string("hipMalloc: ") + hipGetErrorString(e));
}
}  // namespace qpsk

#define QPSK_HIP_TRY(expr)                                                                    \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return ::qpsk::fail(QPSK_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
#endif
