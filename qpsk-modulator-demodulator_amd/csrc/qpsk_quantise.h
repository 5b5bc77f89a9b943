// qpsk_quantise.h -- the one definition of how a float component of the
// modulator's output becomes a CS16 / CS8 / CU8 (or scaled CF32) element.  The
// sample kernel (qpsk_mod.hip) and the host function (qpsk_quantise.cpp) both
// include it, so the device path and its reference cannot drift apart.  It also
// holds the two facts every file asks of a sample format (fmt_known,
// fmt_elem_bytes).  No HIP header: plain C++ sees plain inline functions.
//
//   FIXED  v = x * scale, one float multiply rounded once; clamp to [lo, hi];
//          truncate toward zero -- the reference's
//          (short)Math.Max(short.MinValue, Math.Min(short.MaxValue, ...))
//          (HelperFunctions.cs:97-101).  CF32 stores v itself.
//   PEAK   SaveAsCs16 (HelperFunctions.cs:75-106) per row, in double as there:
//          (double)x / maxVal * (double)full, a division and then a
//          multiplication; clamp; truncate.  maxVal is the row's largest
//          |component|, 1.0 when < 1e-12 (:88).
//   CU8 is the CS8 value + 128.
#pragma once
#include <cstdint>

#include "qpsk_demod.h"

#ifdef __HIP__
#define QPSK_HD __host__ __device__ inline
#else
#define QPSK_HD inline
#endif

namespace qpsk {

// full scale: what PEAK maps the row's peak to, and FIXED's natural scale
QPSK_HD int quant_full(int fmt) { return fmt == QPSK_FMT_CS16 ? 32767 : 127; }
QPSK_HD int quant_lo(int fmt) { return fmt == QPSK_FMT_CS16 ? -32768 : -128; }
// what is added to the clamped, truncated value before it is stored
QPSK_HD int quant_zero(int fmt) { return fmt == QPSK_FMT_CU8 ? 128 : 0; }

// The sample formats (QPSK_FMT_*), for every file that takes one, host or
// device: whether a tag is one, and the bytes of one element of a row (two
// elements a sample).
constexpr int kFmts = 4;
static_assert(QPSK_FMT_CF32 == 0 && QPSK_FMT_CS16 == 1 && QPSK_FMT_CS8 == 2 && QPSK_FMT_CU8 == kFmts - 1,
              "the format tags count from 0 (CallArgs.fmt defaults to CF32)");
QPSK_HD bool fmt_known(int fmt) { return fmt >= 0 && fmt < kFmts; }
QPSK_HD int fmt_elem_bytes(int fmt) { return fmt == QPSK_FMT_CF32 ? 4 : (fmt == QPSK_FMT_CS16 ? 2 : 1); }

// finite and > 0 (NaN fails both comparisons)
QPSK_HD bool quant_scale_ok(float scale) { return scale > 0.0f && scale <= 3.4028234663852886e38f; }

// FIXED's multiply: kept in a function of its own so that no caller can fold it
// into the arithmetic that made x
QPSK_HD float quant_scaled(float x, float scale) { return x * scale; }

// FIXED, integer formats: +-inf saturate at the clamp
QPSK_HD int quant_fixed(int fmt, float x, float scale) {
    const float lo = static_cast<float>(quant_lo(fmt)), hi = static_cast<float>(quant_full(fmt));
    float v = quant_scaled(x, scale);
    v = v < lo ? lo : (v > hi ? hi : v);
    return static_cast<int>(v) + quant_zero(fmt);
}

// the divisor PEAK uses for a row whose largest |component| is peak
QPSK_HD double quant_peak_divisor(float peak) {
    const double m = static_cast<double>(peak);
    return m < 1e-12 ? 1.0 : m;
}

// PEAK, integer formats; max_val from quant_peak_divisor
QPSK_HD int quant_peak(int fmt, float x, double max_val) {
    const double lo = static_cast<double>(quant_lo(fmt)), hi = static_cast<double>(quant_full(fmt));
    double v = static_cast<double>(x) / max_val * hi;
    v = v < lo ? lo : (v > hi ? hi : v);
    return static_cast<int>(v) + quant_zero(fmt);
}

}  // namespace qpsk
