// qpsk_quantise.cpp -- qpsk_quantise_iq: one row of host floats to CS16 / CS8 /
// CU8 (or scaled CF32) by the rules of qpsk_quantise.h.  It is the reference
// the modulator's device path is held to (tests/test_gpu_mod_fmt.py), and what
// a host calls for a float buffer it already has: the reference's SaveAsCs16
// (HelperFunctions.cs:75-106) is PEAK with CS16.  No HIP, no device.
#include <cmath>
#include <cstdint>

#include "qpsk_demod.h"
#include "qpsk_internal.h"
#include "qpsk_quantise.h"

namespace {

using qpsk::fail;

template <typename Out, typename Fn>
void store_row(const float *iq, int64_t n, void *out, Fn value) {
    Out *o = static_cast<Out *>(out);
    for (int64_t i = 0; i < n; ++i) o[i] = static_cast<Out>(value(iq[i]));
}

template <typename Fn>
void store_int(int fmt, const float *iq, int64_t n, void *out, Fn value) {
    if (fmt == QPSK_FMT_CS16) store_row<int16_t>(iq, n, out, value);
    else if (fmt == QPSK_FMT_CS8) store_row<int8_t>(iq, n, out, value);
    else store_row<uint8_t>(iq, n, out, value);
}

}  // namespace

extern "C" int qpsk_quantise_iq(int32_t fmt, int32_t norm, float scale, const float *iq, int64_t n_floats, void *out,
                                float *peak) {
    if (!qpsk::fmt_known(fmt)) return fail(QPSK_ERR_ARGUMENT, "unknown sample format");
    if (norm != QPSK_MOD_NORM_FIXED && norm != QPSK_MOD_NORM_PEAK) return fail(QPSK_ERR_ARGUMENT, "unknown norm");
    if (norm == QPSK_MOD_NORM_PEAK && fmt == QPSK_FMT_CF32)
        return fail(QPSK_ERR_ARGUMENT, "QPSK_MOD_NORM_PEAK needs an integer format");
    if (norm == QPSK_MOD_NORM_FIXED && !qpsk::quant_scale_ok(scale))
        return fail(QPSK_ERR_OUT_OF_RANGE, "scale must be finite and > 0");
    if (n_floats < 0) return fail(QPSK_ERR_ARGUMENT, "negative length");
    if (norm == QPSK_MOD_NORM_PEAK && !peak) return fail(QPSK_ERR_ARGUMENT_NULL, "peak is null");
    if (n_floats > 0 && (!iq || !out)) return fail(QPSK_ERR_ARGUMENT_NULL, "data is null");
    if (norm == QPSK_MOD_NORM_FIXED) {
        if (fmt == QPSK_FMT_CF32)
            store_row<float>(iq, n_floats, out, [=](float x) { return qpsk::quant_scaled(x, scale); });
        else
            store_int(fmt, iq, n_floats, out, [=](float x) { return qpsk::quant_fixed(fmt, x, scale); });
        return QPSK_OK;
    }
    float mx = 0.0f;   // maxVal (:82-86); |float| is exact, so the float maximum is the double one
    for (int64_t i = 0; i < n_floats; ++i) mx = std::fabs(iq[i]) > mx ? std::fabs(iq[i]) : mx;
    *peak = mx;
    const double max_val = qpsk::quant_peak_divisor(mx);
    store_int(fmt, iq, n_floats, out, [=](float x) { return qpsk::quant_peak(fmt, x, max_val); });
    return QPSK_OK;
}
