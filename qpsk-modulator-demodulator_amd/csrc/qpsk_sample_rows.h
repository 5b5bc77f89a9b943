// qpsk_sample_rows.h -- rows of samples of any QPSK_FMT_* between two kernels
// of the test bench (the channel, qpsk_channel.hip, and the propagation path,
// qpsk_path.hip): one sample read as the demodulator reads it, one float sample
// stored as the modulator's quantiser stores it (qpsk_quantise.h), and what the
// host asks of device rows before a kernel sees them.  HIP files only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "qpsk_demod.h"
#include "qpsk_internal.h"
#include "qpsk_quantise.h"

namespace qpsk {

// sample i of a row of fmt as the demodulator reads it
__device__ __forceinline__ float2 load_sample(const void *row, int fmt, int pair, int64_t i, float scale) {
    switch (fmt) {
    case QPSK_FMT_CF32: {
        const float *r = static_cast<const float *>(row) + 2 * i;
        if (pair) return *reinterpret_cast<const float2 *>(r);
        return make_float2(r[0], r[1]);
    }
    case QPSK_FMT_CS16: {
        const short2 v = *reinterpret_cast<const short2 *>(static_cast<const int16_t *>(row) + 2 * i);
        return make_float2(static_cast<float>(v.x) * scale, static_cast<float>(v.y) * scale);
    }
    case QPSK_FMT_CS8: {
        const char2 v = *reinterpret_cast<const char2 *>(static_cast<const int8_t *>(row) + 2 * i);
        return make_float2(static_cast<float>(v.x) * scale, static_cast<float>(v.y) * scale);
    }
    default: {
        const uchar2 v = *reinterpret_cast<const uchar2 *>(static_cast<const uint8_t *>(row) + 2 * i);
        return make_float2(static_cast<float>(static_cast<int>(v.x) - 128) * scale,
                           static_cast<float>(static_cast<int>(v.y) - 128) * scale);
    }
    }
}

__device__ __forceinline__ void store_sample(void *row, int fmt, int pair, int64_t i, float2 y, float scale) {
    switch (fmt) {
    case QPSK_FMT_CF32: {
        float *r = static_cast<float *>(row) + 2 * i;
        const float2 v = make_float2(qpsk::quant_scaled(y.x, scale), qpsk::quant_scaled(y.y, scale));
        if (pair) *reinterpret_cast<float2 *>(r) = v;
        else r[0] = v.x, r[1] = v.y;
        return;
    }
    case QPSK_FMT_CS16:
        *reinterpret_cast<short2 *>(static_cast<int16_t *>(row) + 2 * i) =
            make_short2(static_cast<short>(qpsk::quant_fixed(QPSK_FMT_CS16, y.x, scale)),
                        static_cast<short>(qpsk::quant_fixed(QPSK_FMT_CS16, y.y, scale)));
        return;
    case QPSK_FMT_CS8:
        *reinterpret_cast<char2 *>(static_cast<int8_t *>(row) + 2 * i) =
            make_char2(static_cast<signed char>(qpsk::quant_fixed(QPSK_FMT_CS8, y.x, scale)),
                       static_cast<signed char>(qpsk::quant_fixed(QPSK_FMT_CS8, y.y, scale)));
        return;
    default:
        *reinterpret_cast<uchar2 *>(static_cast<uint8_t *>(row) + 2 * i) =
            make_uchar2(static_cast<unsigned char>(qpsk::quant_fixed(QPSK_FMT_CU8, y.x, scale)),
                        static_cast<unsigned char>(qpsk::quant_fixed(QPSK_FMT_CU8, y.y, scale)));
        return;
    }
}

// the caller's current device, put back when a call returns
struct DeviceGuard {
    int prev = -1;
    DeviceGuard() {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// what device rows of fmt must satisfy (qpsk_demod_process_fmt's rules)
inline int check_device_rows(const char *what, int fmt, const void *rows, int64_t stride) {
    if (stride & 1) return fail(QPSK_ERR_ARGUMENT, std::string("device ") + what + " stride must be even");
    const uintptr_t align = fmt == QPSK_FMT_CS8 || fmt == QPSK_FMT_CU8 ? 2 : 4;
    if (reinterpret_cast<uintptr_t>(rows) % align)
        return fail(QPSK_ERR_ARGUMENT, std::string("device ") + what + " rows must be " + std::to_string(align) +
                                           "-byte aligned");
    return QPSK_OK;
}

// CF32 rows 8-byte aligned: one access a sample
inline bool pair_rows(int fmt, const void *rows, int64_t stride) {
    return fmt != QPSK_FMT_CF32 || (reinterpret_cast<uintptr_t>(rows) % 8 == 0 && stride % 2 == 0);
}

}  // namespace qpsk
