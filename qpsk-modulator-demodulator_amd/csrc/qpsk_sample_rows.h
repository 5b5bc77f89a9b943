// qpsk_sample_rows.h -- rows of samples of any QPSK_FMT_* in the kernels of the
// test bench (the channel, qpsk_channel.hip, the propagation path,
// qpsk_path.hip, and the polyphase channeliser, qpsk_pfb.hip): one sample read
// as the demodulator reads it, one float sample stored as the modulator's
// quantiser stores it (qpsk_quantise.h), a row's length, a window of a row and
// its history staged into LDS, and what the host asks of device rows before a
// kernel sees them.  HIP files only.
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

// row s of a call whose kernel arguments are a (Args has lengths and n): its
// checked length where the call gave lengths, else n
template <typename Args>
__device__ __forceinline__ int64_t row_length(const Args &a, int s) { return a.lengths ? a.lengths[s] : a.n; }

// xs[m] = x at index j0 + m of the call's row, m in [0, xlen): the row (irow,
// len samples), the L samples of history in front of it, +0 before the history
// and behind the row.  Coalesced: 16 bytes a lane where the rows are 16-byte
// aligned and pitched (a.in_wide), else a sample a lane.  Every one of the
// workgroup's kThreads threads calls it.  Args is the kernel's argument block,
// with the input row's fmt_in, scale_in, in_pair and in_wide.
template <int kThreads, typename Args>
__device__ __forceinline__ void stage_window(float2 *xs, int64_t j0, int xlen, int64_t len, const char *irow,
                                             const float (*hist)[2], int L, const Args &a, int tid) {
    if (a.in_wide) {
        const int64_t j1 = j0 + xlen < len ? j0 + xlen : len;   // the row's part of the window: [jr0, j1)
        const int64_t jr0 = j0 > 0 ? j0 : 0;
        // what precedes the row, and (never, in a checked state) what follows it
        for (int m = tid; m < xlen; m += kThreads) {
            const int64_t j = j0 + m;
            if (j >= 0 && j < len) continue;
            const int64_t h = L + j;
            xs[m] = j < 0 && h >= 0 ? make_float2(hist[h][0], hist[h][1]) : make_float2(0.0f, 0.0f);
        }
        const int64_t eb = qpsk::fmt_elem_bytes(a.fmt_in);
        const int V = static_cast<int>(16 / (2 * eb));   // samples in 16 bytes: 2, 4 or 8
        const int64_t c_hi = (j1 + V - 1) / V;
        for (int64_t c = jr0 / V + tid; c < c_hi; c += kThreads) {
            const int64_t jb = c * V;
            if (jb + V <= len) {
                // 16 bytes of the row in registers, read sample by sample as a row is
                const uint4 w = *reinterpret_cast<const uint4 *>(irow + jb * 2 * eb);
#pragma unroll
                for (int v = 0; v < 8; ++v) {
                    const int64_t j = jb + v;
                    if (v < V && j >= jr0 && j < j1) xs[j - j0] = load_sample(&w, a.fmt_in, 1, v, a.scale_in);
                }
            } else {
                for (int v = 0; v < V; ++v) {
                    const int64_t j = jb + v;
                    if (j >= jr0 && j < j1) xs[j - j0] = load_sample(irow, a.fmt_in, a.in_pair, j, a.scale_in);
                }
            }
        }
    } else {
        for (int m = tid; m < xlen; m += kThreads) {
            const int64_t j = j0 + m;
            const int64_t h = L + j;
            if (j >= 0 && j < len) xs[m] = load_sample(irow, a.fmt_in, a.in_pair, j, a.scale_in);
            else xs[m] = j < 0 && h >= 0 ? make_float2(hist[h][0], hist[h][1]) : make_float2(0.0f, 0.0f);
        }
    }
}

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

// rows 16-byte aligned and pitched: stage_window reads 16 bytes a lane
inline bool wide_rows(int fmt, const void *rows, int64_t stride) {
    return reinterpret_cast<uintptr_t>(rows) % 16 == 0 && (stride * qpsk::fmt_elem_bytes(fmt)) % 16 == 0;
}

}  // namespace qpsk
