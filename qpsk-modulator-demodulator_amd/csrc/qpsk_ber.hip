// qpsk_ber.hip -- qpsk_ber_count_device: the bit-error counter of
// include/qpsk_demod.h ("Bit errors, counted where the bits are") on bit rows
// in device memory, where process() and qpsk_synth_generate leave them.
//
// One wave64 per stream.  A stream's windows run in sequence, because each one
// is searched for around the offset the one before was found at; the wave runs
// qpsk_ber.h's window walk, the same code the host function runs, and supplies
// the three operations on bits with its 64 lanes:
//
//   find     one step tests 64 consecutive positions, one per lane: the lane
//            forms the K bits of ref at its position from two big-endian
//            64-bit words and a funnel shift and compares them with the key,
//            which every lane holds.  __ballot and its lowest set lane give
//            the step's first match; the search stops at the first step that
//            has one.  Lanes whose position breaks i + K <= hi stay out.
//   errors   lane l takes the 64-bit words l, l + 64, ... of the window: XOR
//            of the two shifted words, the last partial word masked,
//            __popcll; a butterfly over the wave sums the lanes.
//   same     one K-bit compare.
//
// Everything that decides the control flow is the same in every lane (the
// ballot, the reduced sum, loads from one address), so the wave never splits
// and needs no barrier and no LDS.  Lane 0 writes the row.
//
// A workgroup is four such waves, which share nothing; the waves of the grid
// take streams round robin, so any n_streams runs in a bounded grid.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "qpsk_ber.h"
#include "qpsk_bits_dev.h"
#include "qpsk_demod.h"
#include "qpsk_internal.h"

namespace {

constexpr int kBerWaves = 4;                    // streams a workgroup holds, one per wave
constexpr int kBerThreads = 64 * kBerWaves;
constexpr int kBerMaxBlocks = 4096;             // 16384 waves: more than the chip holds at once

struct BerArgs {
    qpsk_ber_params p;
    const uint8_t *rx;
    int64_t rx_stride;
    const int64_t *n_rx;
    const uint8_t *ref;
    int64_t ref_stride;
    const int64_t *n_ref;
    int32_t n_streams;
    qpsk_ber_row *out;
};

// 64 bits from bit position q on (MSB-first) of a row whose valid bytes end at
// nbytes; bits of bytes past it read as 0, and no such byte is loaded.
__device__ inline uint64_t bits64_at(const uint8_t *row, int64_t q, int64_t nbytes) {
    const int64_t b = q >> 3;
    const int sh = static_cast<int>(q & 7);
    const uint64_t w0 = qpsk::load_be64_any(row, b, nbytes);
    const uint64_t w1 = qpsk::load_be64_any(row, b + 8, nbytes);
    return sh ? (w0 << sh) | (w1 >> (64 - sh)) : w0;
}

// One stream's rows as the wave sees them.
struct WaveOps {
    const uint8_t *rx, *ref;
    int64_t rx_bytes, ref_bytes;                // ceil(R / 8), ceil(N / 8)
    int K;
    int lane;

    // the K bits at q as the low bits of the result
    __device__ uint64_t rx_key(int64_t q) const { return bits64_at(rx, q, rx_bytes) >> (64 - K); }
    __device__ uint64_t ref_key(int64_t q) const { return bits64_at(ref, q, ref_bytes) >> (64 - K); }

    __device__ bool same(int64_t w, int64_t i) const { return rx_key(w) == ref_key(i); }

    __device__ int64_t find(int64_t w, int64_t lo, int64_t hi) const {
        const uint64_t key = rx_key(w);
        const int64_t last = hi - K;                         // last start position
        for (int64_t base = lo; base <= last; base += 64) {
            const int64_t i = base + lane;
            const unsigned long long hits = __ballot(i <= last && ref_key(i) == key);
            if (hits) return base + (__ffsll(hits) - 1);
        }
        return -1;
    }

    __device__ int64_t errors(int64_t w, int64_t i, int64_t m) const {
        int e = 0;                                           // m <= 2^20
        for (int64_t j = 64 * static_cast<int64_t>(lane); j < m; j += 64 * 64) {
            uint64_t x = bits64_at(rx, w + j, rx_bytes) ^ bits64_at(ref, i + j, ref_bytes);
            if (m - j < 64) x &= ~0ull << (64 - (m - j));    // the window's last, partial word
            e += __popcll(x);
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) e += __shfl_xor(e, o, 64);
        return __builtin_amdgcn_readfirstlane(e);            // every lane holds the sum: say so to the compiler
    }
};

__global__ void __launch_bounds__(kBerThreads) ber_count_kernel(BerArgs a) {
    const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
    const int lane = threadIdx.x & 63;
    for (int64_t s = static_cast<int64_t>(blockIdx.x) * kBerWaves + wave; s < a.n_streams;
         s += static_cast<int64_t>(gridDim.x) * kBerWaves) {
        // a count the row cannot hold reads as no bits at all (the host form refuses it)
        const int64_t nr = a.n_rx[s], nf = a.n_ref[s];
        const int64_t R = qpsk::ber_count_fits(nr, a.rx_stride) ? nr : 0;
        const int64_t N = qpsk::ber_count_fits(nf, a.ref_stride) ? nf : 0;
        WaveOps ops{a.rx + s * a.rx_stride, a.ref + s * a.ref_stride, qpsk::ber_row_bytes(R), qpsk::ber_row_bytes(N),
                    a.p.key_bits, lane};
        const qpsk_ber_row row = qpsk::ber_walk(a.p, R, N, ops);
        if (lane == 0) a.out[s] = row;
    }
}

}  // namespace

extern "C" int qpsk_ber_count_device(const qpsk_ber_params *p, const uint8_t *rx_bits, int64_t rx_stride_bytes,
                                     const int64_t *n_rx_bits, const uint8_t *ref_bits, int64_t ref_stride_bytes,
                                     const int64_t *n_ref_bits, int32_t n_streams, qpsk_ber_row *out_dev,
                                     void *hip_stream) {
    int rc;
    if ((rc = qpsk::ber_check_args(p, rx_bits, rx_stride_bytes, n_rx_bits, ref_bits, ref_stride_bytes, n_ref_bits,
                                   n_streams, out_dev, 8)))
        return rc;
    if (n_streams == 0) return QPSK_OK;
    BerArgs a{*p, rx_bits, rx_stride_bytes, n_rx_bits, ref_bits, ref_stride_bytes, n_ref_bits, n_streams, out_dev};
    const int blocks = (n_streams + kBerWaves - 1) / kBerWaves;
    hipLaunchKernelGGL(ber_count_kernel, dim3(blocks < kBerMaxBlocks ? blocks : kBerMaxBlocks), dim3(kBerThreads), 0,
                       static_cast<hipStream_t>(hip_stream), a);
    QPSK_HIP_TRY(hipGetLastError());
    return QPSK_OK;
}
