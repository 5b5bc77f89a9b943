// qpsk_bits_dev.h -- device-side readers of packed bit rows (MSB-first: bit j
// of a row is bit 7 - j % 8 of byte j / 8, BitPacker order,
// HelperFunctions.cs:14-29), shared by the device framer and TSC search
// (qpsk_framer_dev.hip) and the bit-error counter (qpsk_ber.hip).  Device code
// only; every function is inlined into its kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace qpsk {

__device__ inline uint32_t bit_at(const uint8_t *row, int64_t p) {
    return (row[p >> 3] >> (7 - (p & 7))) & 1u;
}

// n bits (0 <= n <= 8) at bit position p, as the low bits of the result.  Only
// the bytes that hold them are read, none for n == 0: a byte that straddles an
// edge (carry | row, packer | row, a string's end) is two such pieces.  The
// second load repeats the first byte where the bits end in it (the shift drops
// it), so both loads are in flight together, not one behind a branch.
__device__ inline uint32_t bits_at(const uint8_t *row, int64_t p, int n) {
    if (n <= 0) return 0;
    const int64_t b = p >> 3;
    const int sh = static_cast<int>(p & 7);
    const uint32_t v = (static_cast<uint32_t>(row[b]) << 8) | row[b + (sh + n > 8)];
    return (v >> (16 - sh - n)) & ((1u << n) - 1);
}

// 64 bits from byte b on (MSB-first), bytes at or past nbytes read as 0.
__device__ inline uint64_t load_be64(const uint8_t *row, int64_t b, int64_t nbytes) {
    uint64_t w = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) w = (w << 8) | (b + i < nbytes ? row[b + i] : 0u);
    return w;
}

// 64 bits from byte b on (MSB-first) of a 4-byte aligned buffer holding at
// least b + 8 bytes: two dword loads and a byte swap instead of 8 byte loads
__device__ inline uint64_t load_be64_aligned(const uint8_t *buf, int64_t b) {
    const uint32_t *w = reinterpret_cast<const uint32_t *>(buf + b);
    return (static_cast<uint64_t>(__builtin_bswap32(w[0])) << 32) | __builtin_bswap32(w[1]);
}

// 64 bits from byte b on (MSB-first) of a row at any alignment whose valid
// bytes end at nbytes (bytes past it read as 0).  Windows whose 12 bytes lie
// inside the row take three aligned dword loads and a funnel shift; the rest
// (the row's last bytes) go byte by byte, so nothing past the row is read.
__device__ inline uint64_t load_be64_any(const uint8_t *row, int64_t b, int64_t nbytes) {
    const uintptr_t addr = reinterpret_cast<uintptr_t>(row + b);
    const int m = static_cast<int>(addr & 3);
    if (b + 12 <= nbytes) {
        const uint32_t *w = reinterpret_cast<const uint32_t *>(addr - m);
        const uint64_t lo = static_cast<uint64_t>(w[0]) | (static_cast<uint64_t>(w[1]) << 32);
        const uint64_t hi = w[2];
        // little-endian bytes m .. m+7 of the 12 loaded
        const uint64_t v = m ? (lo >> (8 * m)) | (hi << (64 - 8 * m)) : lo;
        return __builtin_bswap64(v);
    }
    return load_be64(row, b, nbytes);
}

}  // namespace qpsk
