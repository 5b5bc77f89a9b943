// qpsk_ber.cpp -- qpsk_ber_count: bit errors between received and reference
// bit rows in host memory, by the definition in include/qpsk_demod.h ("Bit
// errors, counted where the bits are"), which is bench.py's ber_after_lock.
// It is the reference the kernel (qpsk_ber.hip) is held to byte for byte, and
// is itself held to ber_after_lock (tests/test_ber_abi.py).  The window walk is
// qpsk_ber.h's; the three bit operations here are the definition's own words,
// one bit at a time.  Also the argument checks both entry points share, and
// the two functions that need neither rows nor a device.  No HIP, no device.
#include <cstdint>
#include <string>

#include "qpsk_ber.h"
#include "qpsk_demod.h"
#include "qpsk_internal.h"

namespace {

using qpsk::fail;

// One stream's rows.  Bit j of a row is bit 7 - j % 8 of byte j / 8; only the
// byte that holds an asked-for bit is read.
struct HostOps {
    const uint8_t *rx, *ref;
    int64_t K;
    static int bit(const uint8_t *row, int64_t j) { return (row[j >> 3] >> (7 - (j & 7))) & 1; }
    bool same(int64_t w, int64_t i) const {
        for (int64_t t = 0; t < K; ++t)
            if (bit(rx, w + t) != bit(ref, i + t)) return false;
        return true;
    }
    int64_t find(int64_t w, int64_t lo, int64_t hi) const {   // bytes.find(key, lo, hi)
        for (int64_t i = lo; i + K <= hi; ++i)
            if (same(w, i)) return i;
        return -1;
    }
    int64_t errors(int64_t w, int64_t i, int64_t m) const {
        int64_t e = 0;
        for (int64_t t = 0; t < m; ++t) e += bit(rx, w + t) != bit(ref, i + t);
        return e;
    }
};

}  // namespace

int qpsk::ber_check_args(const qpsk_ber_params *p, const void *rx_bits, int64_t rx_stride_bytes,
                         const void *n_rx_bits, const void *ref_bits, int64_t ref_stride_bytes,
                         const void *n_ref_bits, int32_t n_streams, const void *out, int out_align) {
    if (!p) return fail(QPSK_ERR_ARGUMENT_NULL, "ber params are null");
    if (!rx_bits || !n_rx_bits) return fail(QPSK_ERR_ARGUMENT_NULL, "rx_bits or n_rx_bits is null");
    if (!ref_bits || !n_ref_bits) return fail(QPSK_ERR_ARGUMENT_NULL, "ref_bits or n_ref_bits is null");
    if (!out) return fail(QPSK_ERR_ARGUMENT_NULL, "out is null");
    if (n_streams < 0) return fail(QPSK_ERR_ARGUMENT, "n_streams must not be negative");
    if (rx_stride_bytes < 0 || ref_stride_bytes < 0) return fail(QPSK_ERR_ARGUMENT, "a row stride must not be negative");
    if (reinterpret_cast<uintptr_t>(out) % static_cast<uintptr_t>(out_align))
        return fail(QPSK_ERR_ARGUMENT, "out_dev must be 8-byte aligned");
    if (p->skip_bits < 0) return fail(QPSK_ERR_OUT_OF_RANGE, "skip_bits must be >= 0, got " + std::to_string(p->skip_bits));
    if (p->key_bits < 1 || p->key_bits > kBerMaxKey)
        return fail(QPSK_ERR_OUT_OF_RANGE, "key_bits must be 1 .. 64, got " + std::to_string(p->key_bits));
    if (p->window < p->key_bits || p->window > kBerMaxWindow)
        return fail(QPSK_ERR_OUT_OF_RANGE, "window must be key_bits .. 2^20, got " + std::to_string(p->window));
    if (p->search < 0 || p->search > kBerMaxSearch)
        return fail(QPSK_ERR_OUT_OF_RANGE, "search must be 0 .. 2^20, got " + std::to_string(p->search));
    return QPSK_OK;
}

extern "C" {

void qpsk_ber_params_init(qpsk_ber_params *p) {
    if (!p) return;
    *p = qpsk_ber_params{};
    p->skip_bits = 8000;
    p->window = 2048;
    p->key_bits = 64;
    p->search = 512;
}

int qpsk_ber_row_size(void) { return static_cast<int>(sizeof(qpsk_ber_row)); }

int qpsk_ber_count(const qpsk_ber_params *p, const uint8_t *rx_bits, int64_t rx_stride_bytes,
                   const int64_t *n_rx_bits, const uint8_t *ref_bits, int64_t ref_stride_bytes,
                   const int64_t *n_ref_bits, int32_t n_streams, qpsk_ber_row *out) {
    int rc;
    if ((rc = qpsk::ber_check_args(p, rx_bits, rx_stride_bytes, n_rx_bits, ref_bits, ref_stride_bytes, n_ref_bits,
                                   n_streams, out, 1)))
        return rc;
    for (int32_t s = 0; s < n_streams; ++s) {
        if (!qpsk::ber_count_fits(n_rx_bits[s], rx_stride_bytes))
            return fail(QPSK_ERR_ARGUMENT, "n_rx_bits[" + std::to_string(s) + "] = " + std::to_string(n_rx_bits[s]) +
                                               " is negative or past the row stride");
        if (!qpsk::ber_count_fits(n_ref_bits[s], ref_stride_bytes))
            return fail(QPSK_ERR_ARGUMENT, "n_ref_bits[" + std::to_string(s) + "] = " + std::to_string(n_ref_bits[s]) +
                                               " is negative or past the row stride");
    }
    for (int32_t s = 0; s < n_streams; ++s) {
        HostOps ops{rx_bits + s * rx_stride_bytes, ref_bits + s * ref_stride_bytes, p->key_bits};
        out[s] = qpsk::ber_walk(*p, n_rx_bits[s], n_ref_bits[s], ops);
    }
    return QPSK_OK;
}

}  // extern "C"
