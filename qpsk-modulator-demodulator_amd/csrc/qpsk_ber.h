// qpsk_ber.h -- the window walk of the bit-error counter (include/qpsk_demod.h,
// "Bit errors, counted where the bits are"; bench.py's ber_after_lock), once:
// the host function (qpsk_ber.cpp) runs it over plain bit loops, the kernel
// (qpsk_ber.hip) runs it with one wave's search, count and compare, and
// neither owns a second copy of which window is lost, a slip or counted.  No
// HIP header: plain C++ sees plain inline functions.
#pragma once
#include <cstdint>

#include "qpsk_demod.h"

#ifdef __HIP__
#define QPSK_HD __host__ __device__ inline
#else
#define QPSK_HD inline
#endif

namespace qpsk {

constexpr int32_t kBerMaxKey = 64;
constexpr int32_t kBerMaxWindow = 1 << 20;
constexpr int32_t kBerMaxSearch = 1 << 20;

// bytes that hold the first n bits of a row (n >= 0)
QPSK_HD int64_t ber_row_bytes(int64_t n) { return n / 8 + (n % 8 != 0); }
// No row holds 2^61 bits (2^58 bytes); below that bound every sum of positions
// the walk forms (w + 4 W, w + off + D + K with off = i - w') stays inside int64.
constexpr int64_t kBerMaxBits = int64_t{1} << 61;
// a bit count a row of stride bytes can hold
QPSK_HD bool ber_count_fits(int64_t n, int64_t stride) {
    return n >= 0 && n < kBerMaxBits && ber_row_bytes(n) <= stride;
}

// One stream's row from R received and N reference bits.  ops supplies the
// three things that touch bits:
//   find(w, lo, hi)    smallest i, lo <= i, i + K <= hi, ref[i, i+K) == rx[w, w+K), or -1
//   errors(w, i, m)    #{ t < m : rx(w + t) != ref(i + t) }
//   same(w, i)         rx[w, w+K) == ref[i, i+K)
// Every position it passes lies inside the rows: w + W <= R, i + m <= N.
// R and N are counts ber_count_fits accepted (0 <= n < 2^61); skip_bits is any
// int64 >= 0, so the loop asks w <= R - W and never forms w + W past R.
template <class Ops>
QPSK_HD qpsk_ber_row ber_walk(const qpsk_ber_params &p, int64_t R, int64_t N, Ops &ops) {
    const int64_t W = p.window, K = p.key_bits, D = p.search;
    qpsk_ber_row r{};
    int64_t off = 0;
    for (int64_t w = p.skip_bits; w <= R - W; w += W) {
        ++r.windows;
        const int64_t lo = r.located ? (w + off - D > 0 ? w + off - D : 0) : 0;
        const int64_t want = r.located ? w + off + D + K : w + 4 * W;
        const int64_t i = ops.find(w, lo, want < N ? want : N);
        if (i < 0) {
            ++r.lost_windows;
            continue;
        }
        if (r.located && i - w != off) ++r.slips;
        r.located = 1;
        off = i - w;
        const int64_t m = W < N - i ? W : N - i;             // >= K: the key lies inside ref
        const int64_t e = ops.errors(w, i, m);
        if (!ops.same(w + m - K, i + m - K) || e > m / 8) {
            ++r.lost_windows;
        } else {
            r.bit_errors += e;
            r.bits += m;
        }
    }
    r.last_offset = off;
    return r;
}

// The argument checks both entry points make before anything is launched or
// written (qpsk_ber.cpp); out_align: the alignment out must have, 1 = any.
int ber_check_args(const qpsk_ber_params *p, const void *rx_bits, int64_t rx_stride_bytes, const void *n_rx_bits,
                   const void *ref_bits, int64_t ref_stride_bytes, const void *n_ref_bits, int32_t n_streams,
                   const void *out, int out_align);

}  // namespace qpsk
