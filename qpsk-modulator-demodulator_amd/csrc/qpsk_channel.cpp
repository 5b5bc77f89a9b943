// qpsk_channel.cpp -- the host half of the channel (include/qpsk_demod.h, "The
// test bench's channel on the device"): the parameter defaults and checks, the
// construction of a stream's state (new NCO(...) twice), and
// qpsk_channel_state_check, which qpsk_channel_set_state runs on a blob before
// anything reaches the device.  No HIP, no device: a stand-alone CPU program
// links this file and qpsk_error.cpp (tools/channel_state_main.cpp runs it
// under the sanitizers).
#include "qpsk_channel.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "qpsk_demod.h"
#include "qpsk_internal.h"
#include "qpsk_row_call.h"

namespace qpsk {
namespace {

int bad_field(int s, const char *osc, const char *field, const std::string &value, const std::string &range) {
    return fail(QPSK_ERR_ARGUMENT, "channel state stream " + std::to_string(s) + ": " + osc + field + " = " + value +
                                       " outside " + range);
}

std::string num(double v) {
    char b[40];
    snprintf(b, sizeof(b), "%.17g", v);
    return b;
}

int check_nco(int s, const char *osc, const ChanNcoConst &c, const ChanNco &n) {
    const struct { const char *name; double v; } f[] = {{"static_ppm", n.static_ppm}, {"drift_ppm", n.drift_ppm},
                                                        {"total_ppm", n.total_ppm}, {"cur_hz", n.cur_hz},
                                                        {"phase", n.phase}};
    for (const auto &e : f)
        if (!std::isfinite(e.v)) return bad_field(s, osc, e.name, num(e.v), "the finite doubles");
    const std::string lim = "[" + num(-c.max_ppm) + ", " + num(c.max_ppm) + "]";
    if (!(std::fabs(n.static_ppm) <= c.max_ppm)) return bad_field(s, osc, "static_ppm", num(n.static_ppm), lim);
    if (!(std::fabs(n.total_ppm) <= c.max_ppm)) return bad_field(s, osc, "total_ppm", num(n.total_ppm), lim);
    // total = static + drift, or after the clamp total = +-max and drift =
    // total - static: two roundings of values no larger than 2 max
    const double sum = n.static_ppm + n.drift_ppm;
    if (!(std::fabs(n.total_ppm - sum) <= 0x1p-50 * c.max_ppm))
        return bad_field(s, osc, "drift_ppm", num(n.drift_ppm), "total_ppm - static_ppm = " + num(n.total_ppm - n.static_ppm));
    const double hz = chan_cur_hz(c, n.total_ppm);
    if (n.cur_hz != hz) return bad_field(s, osc, "cur_hz", num(n.cur_hz), "lo_hz * (1 + total_ppm * 1e-6) = " + num(hz));
    // -0 is what fmod leaves of a negative multiple of 2 pi, and it is not < 0
    if (!(n.phase >= 0.0 && n.phase <= kChanTwoPi)) return bad_field(s, osc, "phase", num(n.phase), "[0, 2 pi]");
    if (n.counter < 0 || n.counter >= c.interval)
        return bad_field(s, osc, "counter", std::to_string(n.counter), "[0, " + std::to_string(c.interval - 1) + "]");
    return QPSK_OK;
}

}  // namespace

int chan_check_params(const qpsk_channel_params *p, int32_t n_streams) {
    if (!p) return fail(QPSK_ERR_ARGUMENT_NULL, "channel params are null");
    if (!(std::isfinite(p->sample_rate) && p->sample_rate > 0.0))
        return fail(QPSK_ERR_OUT_OF_RANGE, "sample_rate must be finite and > 0, got " + num(p->sample_rate));
    const struct { const char *name; double v; } f[] = {{"lo_hz", p->lo_hz}, {"tx_ppm", p->tx_ppm}, {"rx_ppm", p->rx_ppm},
                                                        {"tx_phase0", p->tx_phase0}, {"rx_phase0", p->rx_phase0}};
    for (const auto &e : f)
        if (!std::isfinite(e.v)) return fail(QPSK_ERR_OUT_OF_RANGE, std::string(e.name) + " must be finite, got " + num(e.v));
    if (!(std::isfinite(p->noise_rms) && p->noise_rms >= 0.0))
        return fail(QPSK_ERR_OUT_OF_RANGE, "noise_rms must be finite and >= 0, got " + num(p->noise_rms));
    if (p->first_stream < 0) return fail(QPSK_ERR_OUT_OF_RANGE, "first_stream must be >= 0");
    if (n_streams < 1) return fail(QPSK_ERR_ARGUMENT, "n_streams must be positive");
    return QPSK_OK;
}

ChanState chan_state_new(const qpsk_channel_params &p, int32_t row) {
    const uint64_t g = static_cast<uint64_t>(p.first_stream) + static_cast<uint64_t>(row);
    ChanState st{};
    st.tx = chan_nco_new(chan_nco_const(p.lo_hz, p.sample_rate, p.tx_ppm), p.tx_phase0, p.tx_seed + g);
    st.rx = chan_nco_new(chan_nco_const(p.lo_hz, p.sample_rate, p.rx_ppm), p.rx_phase0, p.rx_seed + g);
    return st;
}

}  // namespace qpsk

extern "C" {

void qpsk_channel_params_init(qpsk_channel_params *p, double sample_rate) {
    if (!p) return;
    *p = qpsk_channel_params{};
    p->sample_rate = sample_rate;
    p->lo_hz = 100e6;            // testAtDataLevel.cs:27-28
    p->tx_ppm = 1.0;
    p->rx_ppm = 1.0;
    p->tx_seed = 1000;
    p->rx_seed = 2000;
}

int qpsk_channel_state_size(void) { return static_cast<int>(sizeof(qpsk::ChanState)); }

int qpsk_channel_state_check(const qpsk_channel_params *p, int32_t n_streams, const void *buf, int64_t buf_bytes) {
    using namespace qpsk;
    int rc;
    if ((rc = chan_check_params(p, n_streams))) return rc;
    if (!buf) return fail(QPSK_ERR_ARGUMENT_NULL, "channel state buffer is null");
    if ((rc = check_state_bytes("channel", buf_bytes, static_cast<int64_t>(n_streams) * static_cast<int64_t>(sizeof(ChanState)))))
        return rc;
    const ChanNcoConst ct = chan_nco_const(p->lo_hz, p->sample_rate, p->tx_ppm);
    const ChanNcoConst cr = chan_nco_const(p->lo_hz, p->sample_rate, p->rx_ppm);
    const char *rec = static_cast<const char *>(buf);
    for (int32_t s = 0; s < n_streams; ++s, rec += sizeof(ChanState)) {
        ChanState st;
        std::memcpy(&st, rec, sizeof(st));
        if ((rc = check_nco(s, "tx.", ct, st.tx))) return rc;
        if ((rc = check_nco(s, "rx.", cr, st.rx))) return rc;
        if (st.pos < 0) return bad_field(s, "", "pos", std::to_string(st.pos), "[0, 2^63)");
        if (st.reserved != 0) return bad_field(s, "", "reserved", std::to_string(st.reserved), "[0, 0]");
    }
    return QPSK_OK;
}

}  // extern "C"
