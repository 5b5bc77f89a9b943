// qpsk_framer_dev.hip -- device-resident byte framer (DeModulateBytes,
// QPSKDeModulator.cs:169-259) and batched TSC search (:413-422), SURVEY.md §8f
// rank 1.
//
// One 256-thread workgroup per stream runs one DeModulateBytes step on the
// packed bit row process() left in HBM.  The reference walks the bits as a
// '0'/'1' string; here every stage is a data-parallel pass over the packed row:
//
//   start hunt   BitsToBytes(cand, off) + IndexOf for off = 0..7 (:187-200)
//                == the first bit position q of the marker's bit pattern with
//                the smallest q mod 8 (the offset loop runs first, the byte
//                index second); each thread scans 32 positions from one 64-bit
//                window and the smallest (q mod 8, q) reduces in LDS
//   keep carry   no start: the candidate string's tail stays for the next call
//   pack         AppendBitsToRing (:108-129) == a funnel-shifted view of the
//                bit row behind the packer's partial byte, cut into bytes
//   end search   RingIndexOf from count - (appended + |end|) (:133-149, :246)
//   close        RingCopyOut + ResetFramer (:151-167)
//   append       else the bytes go into the ring
//
// framer_step is that state machine; all three searches are first_match.
//
// Work per call is O(bits) with no serial walk, and the scans stop at the
// first match (the chunk holding it): on real traffic the start and end
// markers sit near the start of a call's bits, and a frame that closes in the
// call never writes its bytes to the ring (its payload is copied straight from
// the bits).  The framer moves ~2 bits per symbol of traffic, noise next to
// the demod chain's 8 B/sample.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "qpsk_bits_dev.h"
#include "qpsk_demod.h"
#include "qpsk_device.h"
#include "qpsk_internal.h"

namespace {

constexpr int kFrThreads = 256;
constexpr int64_t kRefRing = 300000000;   // FrameBuffer = new byte[300_000_000] (:58)

struct FrState {            // one reference instance's framer fields (:59-70)
    int32_t in_frame;       // _inFrame
    int32_t locked_off;     // _lockedBitOffset
    int32_t pack_byte;      // _packByte
    int32_t pack_bits;      // _packBits
    int64_t count;          // _rbCount (head == count: RingClear zeroes both, nothing pops)
    int64_t carry_bits;     // _searchCarryBits.Length (bits kept packed, MSB-first)
};

struct FrArgs {
    const uint8_t *bits;
    int64_t bits_stride;
    const int64_t *bit_offset;
    const int64_t *n_bits;
    uint8_t *payload;
    int64_t payload_stride;
    int64_t *n_payload;
    FrState *st;
    uint8_t *carry;         // [S][carry_stride]
    int64_t carry_stride;
    uint8_t *scratch;       // [S][scr_stride]  candidate bits of a start hunt
    int64_t scr_stride;
    uint8_t *ring;          // [S][ring_cap]
    int64_t ring_cap;
    const uint8_t *start;   // markers (device)
    int32_t ns;
    const uint8_t *end;
    int32_t ne;
};

// the packed-row readers (qpsk_bits_dev.h)
using qpsk::bit_at;
using qpsk::bits_at;
using qpsk::load_be64;
using qpsk::load_be64_aligned;
using qpsk::load_be64_any;

// 8 bits at bit position p (p + 8 <= valid bits of row).
__device__ inline uint32_t bits8(const uint8_t *row, int64_t p) { return bits_at(row, p, 8); }

// Positions a search chunk covers before the workgroup looks at its result:
// the reference's scans stop at the first match (IndexOf, RingIndexOf), and on
// real traffic that sits near the start of the row.
constexpr int kHuntWindows = kFrThreads;        // 32 positions each: 1 KB of candidate bits
constexpr int kEndPerThread = 8;                // ring positions per thread and chunk
constexpr unsigned long long kNoMatch = ULLONG_MAX;


// The workgroup's smallest match key over the positions [first, last]
// (first >= 0), kNoMatch if there is none; every thread calls it and gets the
// answer.  Positions are taken in ascending chunks.  Per chunk prepare(c0) runs
// first, a step of the whole workgroup (ending in a barrier if the probes read
// what it wrote); then probe(c0) returns the smallest key among the calling
// thread's share of [c0, c0 + chunk), or kNoMatch.  A key is its position, with
// or without a rank in the high bits: never smaller than the position.  So once
// the minimum lies below the next chunk's first position the search stops.
template <class Prepare, class Probe>
__device__ unsigned long long first_match(int64_t first, int64_t last, int64_t chunk, Prepare prepare,
                                          Probe probe) {
    __shared__ unsigned long long best;
    if (threadIdx.x == 0) best = kNoMatch;
    __syncthreads();                       // an empty range reads nothing, a first chunk reads this
    unsigned long long found = kNoMatch;
    for (int64_t c0 = first; c0 <= last; c0 += chunk) {
        prepare(c0);
        const unsigned long long mine = probe(c0);
        if (mine != kNoMatch) atomicMin(&best, mine);
        __syncthreads();
        // The exit must be one decision for the whole workgroup: every wave
        // reads the minimum, and only after a second barrier may any wave go
        // on to the next chunk's atomicMin.  Without it a wave late to read
        // could see a match a faster wave had already posted for the NEXT
        // chunk and leave with a partial minimum.  (The window is a few
        // instructions inside one workgroup, so no test goes red on it
        // reliably; the chunk edge cases of tests/test_framer.py put matches
        // where it would bite.)
        found = best;
        __syncthreads();
        if (found < static_cast<unsigned long long>(c0 + chunk)) break;
    }
    return found;
}

// The candidate bit string of a hunt: carry bits, then the row from bit off0,
// n bits in all.  Inside a frame it is rxBits alone (no carry).
struct Cand {
    const uint8_t *carry;
    int64_t ncarry;
    const uint8_t *row;
    int64_t off0;
    int64_t n;
    // bits [q, q + k) as the low bits of the result (k <= 8, q + k <= n)
    __device__ uint32_t bits(int64_t q, int k) const {
        if (q >= ncarry) return bits_at(row, off0 + q - ncarry, k);
        const int kc = static_cast<int>(ncarry - q < k ? ncarry - q : k);    // of them in the carry
        return (bits_at(carry, q, kc) << (k - kc)) | bits_at(row, off0, k - kc);
    }
    // bits [q, q + 8), zero past n (q < n)
    __device__ uint32_t bits8_at(int64_t q) const {
        const int k = static_cast<int>(n - q < 8 ? n - q : 8);
        return bits(q, k) << (8 - k);
    }
};

// The candidate string as bytes in the stream's scratch row, where the hunt's
// windows are aligned loads: bytes [0, mat) are there, zero behind the string.
struct CandRow {
    uint8_t *bytes;
    Cand src;
    int64_t mat;
    __device__ int64_t pad_end() const { return ((src.n + 7) >> 3) + 8; }   // zero bytes behind the string (scratch slack)
    // bytes [mat, min(upto, pad_end())) by the whole workgroup
    __device__ void fill(int64_t upto) {
        const int64_t ncb = (src.n + 7) >> 3;
        upto = upto < pad_end() ? upto : pad_end();
        for (int64_t j = mat + threadIdx.x; j < upto; j += kFrThreads)
            bytes[j] = static_cast<uint8_t>(j < ncb ? src.bits8_at(8 * j) : 0u);
        mat = upto > mat ? upto : mat;
        __syncthreads();
    }
};

// W, the bit string a call cuts into ring bytes: the packer's P held bits,
// then the candidate string from bit `base` on.  A call that enters a frame
// has an empty packer and base = the first bit behind the start marker (:203-214);
// inside a frame the candidate string is rxBits and base = 0 (:238-246).
struct Packed {
    Cand c;
    int64_t base;
    uint32_t pack_byte;
    int P;
    // bits [w, w + k) of W as the low bits of the result (k <= 8, w + k <= |W|)
    __device__ uint32_t bits(int64_t w, int k) const {
        if (w >= P) return c.bits(base + w - P, k);
        const int kp = static_cast<int>(P - w < k ? P - w : k);              // of them in the packer
        return (((pack_byte >> (P - w - kp)) & ((1u << kp) - 1)) << (k - kp)) | c.bits(base, k - kp);
    }
    __device__ uint32_t byte(int64_t j) const { return bits(8 * j, 8); }     // 8j + 8 <= |W|
};

__device__ void reset_state(FrState &s) {   // ResetFramer (:159-167)
    s.in_frame = 0;
    s.locked_off = -1;
    s.pack_byte = 0;
    s.pack_bits = 0;
    s.count = 0;
    s.carry_bits = 0;
}

constexpr int kOffShift = 61;               // a hunt key: q mod 8 above bit 61, q below

// Start hunt over carry + rxBits (:183-236).  BitsToBytes(cand, off) + IndexOf
// for off = 0..7 == the first bit position q of the marker pattern with the
// smallest q mod 8, so the key is (q mod 8, q) and the search stops after the
// first chunk with an offset-0 match.  Every thread tests the 32 positions of
// one 64-bit window; the chunk's candidate bytes go into the scratch row first.
__device__ unsigned long long hunt_start(CandRow &cr, const uint8_t *start, int ns) {
    const int64_t limit = cr.src.n - 8 * static_cast<int64_t>(ns);   // last start position
    const uint32_t m0 = start[0];
    return first_match(
        0, limit, 32 * kHuntWindows,
        // the chunk's windows read bytes < c0 / 8 + 4 kHuntWindows + 8, the
        // marker checks up to ns + 1 bytes beyond
        [&](int64_t c0) { cr.fill((c0 >> 3) + 4 * kHuntWindows + 8 + ns + 1); },
        [&](int64_t c0) {
            unsigned long long mine = kNoMatch;
            const int64_t w = (c0 >> 5) + threadIdx.x;
            if (32 * w > limit) return mine;
            const uint64_t win = load_be64_aligned(cr.bytes, 4 * w);
            const int jmax = static_cast<int>(limit - 32 * w < 31 ? limit - 32 * w : 31);
            uint32_t hits = 0;                               // bit j: position j starts with the marker's first byte
#pragma unroll
            for (int j = 0; j < 32; ++j) hits |= static_cast<uint32_t>(((win >> (56 - j)) & 0xffu) == m0) << j;
            for (hits &= 0xffffffffu >> (31 - jmax); hits; hits &= hits - 1) {
                const int j = __ffs(hits) - 1;
                const int64_t q = 32 * w + j;
                int k = 1;
                while (k < ns && bits8(cr.bytes, q + 8 * k) == start[k]) ++k;
                const unsigned long long key = (static_cast<unsigned long long>(j & 7) << kOffShift) | q;
                if (k == ns && key < mine) mine = key;
            }
            return mine;
        });
}

// No start: keep min(|cand|, 8|start|+7) tail bits (:233-235), copied from the
// scratch row (the carry is rewritten in place; both are zero behind their bits).
__device__ int64_t keep_carry(CandRow &cr, uint8_t *carry, int ns) {
    cr.fill(cr.pad_end());
    const int64_t nc = cr.src.n;
    const int64_t keep = nc < 8 * static_cast<int64_t>(ns) + 7 ? nc : 8 * static_cast<int64_t>(ns) + 7;
    for (int64_t j = threadIdx.x; j < (keep + 7) >> 3; j += kFrThreads)
        carry[j] = static_cast<uint8_t>(bits8(cr.bytes, nc - keep + 8 * j));
    return keep;
}

// End search: RingIndexOf from count - (appended + |end|) (:133-149, :246) over
// the ring as it is after the append; the position of the end marker or -1.
template <class RingByte>
__device__ int64_t end_search(RingByte ring_byte, int64_t count, int64_t produced, const uint8_t *end, int ne) {
    const int64_t from = count - (produced + ne) > 0 ? count - (produced + ne) : 0;
    const int64_t last = count - ne;                         // last start position of the end marker
    const uint32_t e0 = end[0];
    const unsigned long long at = first_match(from, last, kFrThreads * kEndPerThread, [](int64_t) {}, [&](int64_t c0) {
        unsigned long long mine = kNoMatch;
        for (int k = 0; k < kEndPerThread; ++k) {
            const int64_t i = c0 + k * kFrThreads + threadIdx.x;
            if (i > last || ring_byte(i) != e0) continue;
            int m = 1;
            while (m < ne && ring_byte(i + m) == end[m]) ++m;
            if (m == ne && static_cast<unsigned long long>(i) < mine) mine = i;
        }
        return mine;
    });
    return at == kNoMatch ? -1 : static_cast<int64_t>(at);
}

// dst[i] = byte(i), i < n, by the workgroup: RingCopyOut, and the append to the ring
template <class Byte>
__device__ void store_bytes(uint8_t *dst, int64_t n, Byte byte) {
    for (int64_t i = threadIdx.x; i < n; i += kFrThreads) dst[i] = static_cast<uint8_t>(byte(i));
}

// One DeModulateBytes step on non-empty rxBits: the state it leaves in st, the
// payload length it returns.  Every thread runs it with the same state, so each
// return below is taken by the whole workgroup and no barrier is left waiting.
__device__ int64_t framer_step(const FrArgs &a, int s, int64_t off0, int64_t nb, FrState &st) {
    uint8_t *ring = a.ring + s * a.ring_cap;
    Packed w{Cand{nullptr, 0, a.bits + s * a.bits_stride, off0, nb}, 0, static_cast<uint32_t>(st.pack_byte),
             st.pack_bits};
    if (!st.in_frame) {
        uint8_t *carry = a.carry + s * a.carry_stride;
        w.c.carry = carry;
        w.c.ncarry = st.carry_bits;
        w.c.n = st.carry_bits + nb;
        CandRow cr{a.scratch + s * a.scr_stride, w.c, 0};
        const unsigned long long key = hunt_start(cr, a.start, a.ns);
        if (key == kNoMatch) {
            st.carry_bits = keep_carry(cr, carry, a.ns);
            return 0;
        }
        // enter the frame: ring cleared, W = cand bits after the marker (:203-214)
        w.base = static_cast<int64_t>(key & ((1ull << kOffShift) - 1)) + 8 * static_cast<int64_t>(a.ns);
        w.P = 0;
        st.in_frame = 1;
        st.locked_off = static_cast<int32_t>(key >> kOffShift);
        st.count = 0;                                        // the ring restarts (RingClear)
    }
    // pack W behind the ring's bytes (AppendBitsToRing): whole bytes to the
    // ring, the leftover bits W[8 produced, |W|) stay in the packer
    const int64_t len = w.P + w.c.n - w.base;
    const int64_t produced = len >> 3;
    if (st.count + produced > a.ring_cap) {                  // overflow -> drop + resync (:215-220, :241-245)
        reset_state(st);
        return 0;
    }
    st.pack_bits = static_cast<int32_t>(len & 7);
    st.pack_byte = static_cast<int32_t>(w.bits(8 * produced, st.pack_bits));
    const int64_t old_count = st.count;
    // ring byte i after the append (i < old_count + produced), without writing the ring
    auto ring_byte = [&](int64_t i) -> uint32_t { return i < old_count ? ring[i] : w.byte(i - old_count); };

    const int64_t end_at = end_search(ring_byte, old_count + produced, produced, a.end, a.ne);
    if (end_at >= 0) {                                       // RingCopyOut + ResetFramer (:223-226)
        // the frame closes: its payload comes straight from the ring and this
        // call's bits; the appended bytes never need to be stored
        if (a.payload)
            store_bytes(a.payload + s * a.payload_stride, end_at < a.payload_stride ? end_at : a.payload_stride,
                        ring_byte);
        reset_state(st);
        return end_at;
    }
    // the frame stays open: the appended bytes go into the ring
    store_bytes(ring + old_count, produced, [&](int64_t j) { return w.byte(j); });
    st.count = old_count + produced;
    return 0;
}

__global__ void __launch_bounds__(kFrThreads) framer_push_kernel(FrArgs a) {
    const int s = blockIdx.x;
    const int64_t off0 = a.bit_offset ? a.bit_offset[s] : 0;
    const int64_t nb = a.n_bits[s] - off0;
    FrState st = a.st[s];
    __syncthreads();                       // every wave holds st before thread 0 rewrites it
    int64_t n_payload = 0;
    if (off0 >= 0 && nb > 0) n_payload = framer_step(a, s, off0, nb, st);   // else rxBits empty (:179-180)
    if (threadIdx.x == 0) {
        a.n_payload[s] = n_payload;
        a.st[s] = st;
    }
}

// Pattern bits ride by value in the kernel arguments up to 4096 bits (the
// reference's TSC is 64, testAtDataLevel.cs:20-22); longer ones in a buffer.
struct TscPat {
    uint8_t b[512];
};

// rx.IndexOf(tsc, Ordinal) per stream (:413-422).  Each thread tests 32
// positions against the first min(m, 32) pattern bits from one 64-bit window,
// the rest bit by bit; first_match takes chunks of kFrThreads windows and
// stops after the one holding the first match.
__global__ void __launch_bounds__(kFrThreads)
tsc_find_kernel(const uint8_t *bits, int64_t stride, const int64_t *n_bits, TscPat small,
                const uint8_t *big, int32_t m, int64_t *offsets) {
    const uint8_t *pat = big ? big : small.b;
    const int s = blockIdx.x;
    const uint8_t *row = bits + s * stride;
    const int64_t n = n_bits[s];
    const int64_t limit = n - m;
    const int64_t nbytes = (n + 7) >> 3;
    const int km = m < 32 ? m : 32;
    uint32_t key = 0;
    for (int i = 0; i < km; ++i) key = (key << 1) | bit_at(pat, i);
    const uint64_t kmask = km == 32 ? 0xffffffffull : ((1ull << km) - 1);
    const unsigned long long at = first_match(0, limit, 32 * kFrThreads, [](int64_t) {}, [&](int64_t c0) {
        const int64_t w = (c0 >> 5) + threadIdx.x;
        if (32 * w > limit) return kNoMatch;
        const uint64_t win = load_be64_any(row, 4 * w, nbytes);
        const int jmax = static_cast<int>(limit - 32 * w < 31 ? limit - 32 * w : 31);
        // position j of the window matches the first km pattern bits
        auto full = [&](int j) -> bool {
            if (j > jmax || ((win >> (64 - km - j)) & kmask) != key) return false;
            const int64_t q = 32 * w + j;
            int k = km;
            while (k < m && bit_at(row, q + k) == bit_at(pat, k)) ++k;
            return k == m;
        };
        int first = 64;                                      // the window's first match
        if (m >= 16) {
            // a 16-bit prefix filter on two positions per 32-bit word: the
            // word of bits [o, o + 32) holds the 16-bit values at o (high
            // half) and o + 16 (low half), so 16 funnel shifts cover the
            // window's 32 positions; a half equal to the prefix (haszero on
            // the XOR, false positives possible, never false negatives) is
            // checked in full.  ~5 ops per two positions instead of ~6 per one
            const uint32_t k16 = key >> (km - 16);
            const uint32_t kk = (k16 << 16) | k16;
            const uint32_t whi = static_cast<uint32_t>(win >> 32), wlo = static_cast<uint32_t>(win);
#pragma unroll
            for (int o = 0; o < 16; ++o) {
                const uint32_t x = o ? (whi << o) | (wlo >> (32 - o)) : whi;
                const uint32_t z = x ^ kk;
                const uint32_t hz = (z - 0x00010001u) & ~z & 0x80008000u;
                if (__builtin_expect(hz != 0, 0)) {
                    if ((hz & 0x80000000u) && o < first && full(o)) first = o;
                    if ((hz & 0x00008000u) && o + 16 < first && full(o + 16)) first = o + 16;
                }
            }
        } else {
            for (int j = 0; j <= jmax && first == 64; ++j)
                if (full(j)) first = j;
        }
        return first < 64 ? static_cast<unsigned long long>(32 * w + first) : kNoMatch;
    });
    if (threadIdx.x == 0) offsets[s] = at == kNoMatch ? -1 : static_cast<int64_t>(at) + m;
}

// `new QPSKDeModulator(...)` on the listed rows: the framer fields as
// qpsk_framer_dev_create leaves them (an empty ring, no carry, not in a frame)
__global__ void framer_reset_rows_kernel(FrState *st, const int32_t *rows, int32_t n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) st[rows[i]] = FrState{0, -1, 0, 0, 0, 0};
}

using qpsk::fail;

}  // namespace

struct qpsk_framer_dev {
    int32_t n_streams = 0;
    int32_t device = 0;
    qpsk::Stream stream;             // in front of the buffers, which go first
    qpsk::DevBuf<FrState> st;
    qpsk::DevBuf<uint8_t> carry;
    int64_t carry_stride = 0;
    qpsk::DevBuf<uint8_t> scratch;
    int64_t scr_stride = 0;
    qpsk::DevBuf<uint8_t> ring;
    int64_t ring_cap = kRefRing;
    qpsk::DevBuf<uint8_t> markers;   // start bytes then end bytes
    int32_t ns = 0, ne = 0;
    qpsk::DevBuf<int32_t> rows;      // the list of a reset_streams call

    ~qpsk_framer_dev() {
        if (stream) hipStreamSynchronize(stream);
    }
};

namespace {
// Markers go to device memory after the stream drained; a longer start marker
// widens every stream's carry row (8|start|+7 bits), keeping the bits held.
int load_markers(qpsk_framer_dev *f, const uint8_t *start, int32_t ns, const uint8_t *end, int32_t ne) {
    if (!start || !end) return fail(QPSK_ERR_ARGUMENT_NULL, "marker is null");
    if (ns <= 0) return fail(QPSK_ERR_ARGUMENT, "startMarker cannot be empty.");   // :174
    if (ne <= 0) return fail(QPSK_ERR_ARGUMENT, "endMarker cannot be empty.");     // :175
    QPSK_HIP_TRY(hipSetDevice(f->device));
    if (f->stream) QPSK_HIP_TRY(hipStreamSynchronize(f->stream));
    QPSK_HIP_TRY(f->markers.grow(static_cast<size_t>(ns) + ne));
    std::vector<uint8_t> m(start, start + ns);
    m.insert(m.end(), end, end + ne);
    QPSK_HIP_TRY(hipMemcpy(f->markers, m.data(), m.size(), hipMemcpyHostToDevice));
    const int64_t need = ((static_cast<int64_t>(ns) + 1 + 15) / 16) * 16;
    if (need > f->carry_stride) {
        qpsk::DevBuf<uint8_t> c;   // the old rows go with it, once theirs are in the new
        QPSK_HIP_TRY(c.alloc(need * f->n_streams));
        QPSK_HIP_TRY(hipMemset(c, 0, need * f->n_streams));
        if (f->carry)
            QPSK_HIP_TRY(hipMemcpy2D(c, need, f->carry, f->carry_stride, f->carry_stride, f->n_streams,
                                     hipMemcpyDeviceToDevice));
        f->carry.swap(c);
        f->carry_stride = need;
    }
    f->ns = ns;
    f->ne = ne;
    return QPSK_OK;
}
}  // namespace

extern "C" {

int qpsk_framer_dev_create(int32_t n_streams, const uint8_t *start_marker, int32_t n_start,
                           const uint8_t *end_marker, int32_t n_end, int64_t ring_capacity,
                           int32_t device, qpsk_framer_dev **out) {
    if (!out) return fail(QPSK_ERR_ARGUMENT_NULL, "out is null");
    *out = nullptr;
    if (n_streams <= 0) return fail(QPSK_ERR_ARGUMENT, "n_streams must be positive");
    auto *f = new qpsk_framer_dev();
    f->n_streams = n_streams;
    f->device = device;
    if (ring_capacity > 0) f->ring_cap = ring_capacity;
    int rc = load_markers(f, start_marker, n_start, end_marker, n_end);
    if (rc != QPSK_OK) {
        delete f;
        return rc;
    }
    hipError_t e = f->stream.create(hipStreamNonBlocking);
    if (e == hipSuccess) e = f->ring.alloc(f->ring_cap * n_streams);
    if (e == hipSuccess) e = f->st.alloc(n_streams);
    if (e == hipSuccess) {
        std::vector<FrState> init(n_streams, FrState{0, -1, 0, 0, 0, 0});
        e = hipMemcpy(f->st, init.data(), sizeof(FrState) * n_streams, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        delete f;
        return fail(QPSK_ERR_DEVICE, std::string("framer allocation: ") + hipGetErrorString(e));
    }
    *out = f;
    return QPSK_OK;
}

int qpsk_framer_dev_destroy(qpsk_framer_dev *f) {
    delete f;
    return QPSK_OK;
}

int qpsk_framer_dev_set_stream(qpsk_framer_dev *f, void *hip_stream) {
    if (!f) return fail(QPSK_ERR_ARGUMENT_NULL, "null framer");
    QPSK_HIP_TRY(hipSetDevice(f->device));
    QPSK_HIP_TRY(hipStreamSynchronize(f->stream));
    QPSK_HIP_TRY(f->stream.rebind(hip_stream));
    return QPSK_OK;
}

int qpsk_framer_dev_set_markers(qpsk_framer_dev *f, const uint8_t *start_marker, int32_t n_start,
                                const uint8_t *end_marker, int32_t n_end) {
    if (!f) return fail(QPSK_ERR_ARGUMENT_NULL, "null framer");
    return load_markers(f, start_marker, n_start, end_marker, n_end);
}

int qpsk_framer_dev_push(qpsk_framer_dev *f, const uint8_t *bits, int64_t bits_stride_bytes,
                         const int64_t *bit_offset, const int64_t *n_bits, uint8_t *payload,
                         int64_t payload_stride, int64_t *n_payload) {
    if (!f || !bits || !n_bits || !n_payload) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    if (bits_stride_bytes <= 0 || payload_stride < 0) return fail(QPSK_ERR_ARGUMENT, "bad stride");
    QPSK_HIP_TRY(hipSetDevice(f->device));
    // candidate row: carry (<= carry_stride bytes) + one row of bits, 8 B slack
    const int64_t need = ((f->carry_stride + bits_stride_bytes + 8 + 15) / 16) * 16;
    if (need > f->scr_stride) {
        QPSK_HIP_TRY(hipStreamSynchronize(f->stream));
        f->scr_stride = 0;
        QPSK_HIP_TRY(f->scratch.grow(need * f->n_streams));
        f->scr_stride = need;
    }
    FrArgs a;
    a.bits = bits;
    a.bits_stride = bits_stride_bytes;
    a.bit_offset = bit_offset;
    a.n_bits = n_bits;
    a.payload = payload_stride > 0 ? payload : nullptr;
    a.payload_stride = payload_stride;
    a.n_payload = n_payload;
    a.st = f->st;
    a.carry = f->carry;
    a.carry_stride = f->carry_stride;
    a.scratch = f->scratch;
    a.scr_stride = f->scr_stride;
    a.ring = f->ring;
    a.ring_cap = f->ring_cap;
    a.start = f->markers;
    a.ns = f->ns;
    a.end = f->markers + f->ns;
    a.ne = f->ne;
    hipLaunchKernelGGL(framer_push_kernel, dim3(f->n_streams), dim3(kFrThreads), 0, f->stream, a);
    QPSK_HIP_TRY(hipGetLastError());
    return QPSK_OK;
}

int qpsk_framer_dev_status(const qpsk_framer_dev *f, int32_t *in_frame, int64_t *ring_count,
                           int64_t *carry_bits) {
    if (!f) return fail(QPSK_ERR_ARGUMENT_NULL, "null framer");
    QPSK_HIP_TRY(hipSetDevice(f->device));
    QPSK_HIP_TRY(hipStreamSynchronize(f->stream));
    std::vector<FrState> h(f->n_streams);
    QPSK_HIP_TRY(hipMemcpy(h.data(), f->st, sizeof(FrState) * f->n_streams, hipMemcpyDeviceToHost));
    for (int32_t s = 0; s < f->n_streams; ++s) {
        if (in_frame) in_frame[s] = h[s].in_frame;
        if (ring_count) ring_count[s] = h[s].count;
        if (carry_bits) carry_bits[s] = h[s].carry_bits;
    }
    return QPSK_OK;
}

int qpsk_framer_dev_reset_streams(qpsk_framer_dev *f, const int32_t *streams, int32_t n) {
    if (!f) return fail(QPSK_ERR_ARGUMENT_NULL, "null framer");
    if (n == 0) return QPSK_OK;
    int rc;
    if ((rc = qpsk_stream_list_check(f->n_streams, streams, n))) return rc;
    QPSK_HIP_TRY(hipSetDevice(f->device));
    if (f->rows.bytes() < sizeof(int32_t) * n) {
        QPSK_HIP_TRY(hipStreamSynchronize(f->stream));           // an earlier reset may still read the list
        QPSK_HIP_TRY(f->rows.grow(sizeof(int32_t) * f->n_streams));
    }
    QPSK_HIP_TRY(hipMemcpyAsync(f->rows, streams, sizeof(int32_t) * n, hipMemcpyHostToDevice, f->stream));
    hipLaunchKernelGGL(framer_reset_rows_kernel, dim3((n + kFrThreads - 1) / kFrThreads), dim3(kFrThreads), 0,
                       f->stream, f->st.get(), f->rows.get(), n);
    QPSK_HIP_TRY(hipGetLastError());
    QPSK_HIP_TRY(hipStreamSynchronize(f->stream));               // pageable source outlives the copy
    return QPSK_OK;
}

int qpsk_tsc_find_device(const uint8_t *bits, int64_t bits_stride_bytes, const int64_t *n_bits,
                         int32_t n_streams, const char *tsc, int64_t *offsets, void *hip_stream) {
    if (!offsets || !n_bits) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    if (n_streams <= 0) return QPSK_OK;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const int64_t m = tsc ? static_cast<int64_t>(std::strlen(tsc)) : 0;
    bool blank = true;                                       // string.IsNullOrWhiteSpace (:21)
    bool binary = true;
    for (int64_t i = 0; i < m; ++i) {
        if (!std::strchr(" \t\r\n\v\f", tsc[i])) blank = false;
        if (tsc[i] != '0' && tsc[i] != '1') binary = false;
    }
    if (blank) {                                             // no TSC: payload = every bit
        QPSK_HIP_TRY(hipMemsetAsync(offsets, 0, sizeof(int64_t) * n_streams, stream));
        return QPSK_OK;
    }
    if (!binary || m > INT32_MAX) {                          // '0'/'1' rows never match other chars
        QPSK_HIP_TRY(hipMemsetAsync(offsets, 0xff, sizeof(int64_t) * n_streams, stream));
        return QPSK_OK;
    }
    if (!bits) return fail(QPSK_ERR_ARGUMENT_NULL, "bits is null");
    if (bits_stride_bytes <= 0) return fail(QPSK_ERR_ARGUMENT, "bad stride");
    std::vector<uint8_t> packed((m + 7) / 8, 0);
    for (int64_t i = 0; i < m; ++i)
        if (tsc[i] == '1') packed[i >> 3] |= static_cast<uint8_t>(0x80u >> (i & 7));
    TscPat small{};
    uint8_t *big = nullptr;
    if (packed.size() <= sizeof(small.b)) {
        std::memcpy(small.b, packed.data(), packed.size());
    } else {                                                 // rare: stream-ordered buffer
        QPSK_HIP_TRY(hipMallocAsync(reinterpret_cast<void **>(&big), packed.size(), stream));
        QPSK_HIP_TRY(hipMemcpyAsync(big, packed.data(), packed.size(), hipMemcpyHostToDevice, stream));
    }
    hipLaunchKernelGGL(tsc_find_kernel, dim3(n_streams), dim3(kFrThreads), 0, stream, bits,
                       bits_stride_bytes, n_bits, small, static_cast<const uint8_t *>(big),
                       static_cast<int32_t>(m), offsets);
    QPSK_HIP_TRY(hipGetLastError());
    if (big) {
        QPSK_HIP_TRY(hipFreeAsync(big, stream));
        QPSK_HIP_TRY(hipStreamSynchronize(stream));               // pageable source outlives the copy
    }
    return QPSK_OK;
}

}  // extern "C"
