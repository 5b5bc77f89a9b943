// qpsk_mod.hip -- the reference's QPSKModulator (QPSKModulator.cs:18-167) behind
// the C ABI, batched: one handle = the constructor (RRC taps, TSC, differential
// flag), one call = Modulate / ModulateBytes on S independent bit strings, the
// output in CF32, CS16, CS8 or CU8 (csrc/qpsk_quantise.h).
//
//   mod_symbols_kernel  one workgroup per stream.  The logical bit string is
//                       tsc | bits[s] (Modulate) or tsc | START | payload[s] |
//                       END (ModulateBytes, :54-72), addressed by index from
//                       its pieces: no framed copy exists.  A lane takes four
//                       dibits (consecutive lanes read consecutive bytes of one
//                       row).  Differential encoding (DibitToDelta :92-102, sym
//                       = prev * delta, reference (1/sqrt2)(1+j) :126) is a
//                       running sum mod 4 of quarter turns: a scan inside the
//                       wave, across the workgroup's waves, and a carried
//                       offset from one pass of QPSK_MOD_SCAN_DIBITS dibits to
//                       the next.  Direct mapping (:140-144) needs no scan.
//                       The symbol of every dibit is +-InvSqrt2 on both axes,
//                       exactly, so it is kept as a quadrant, one byte each.
//   mod_samples_kernel  one workgroup per stream x tile of QPSK_MOD_TILE_SAMPLES
//                       output samples.  It stages the taps (as the exact
//                       doubles (double)tap * (double)InvSqrt2) and the
//                       quadrants the tile touches in LDS; a lane computes the
//                       run of consecutive samples that fills 16 bytes of the
//                       output format.  The impulse train (symbol d at delay +
//                       d*sps, :129-152) is filtered in double, the terms added
//                       tap by tap in ascending tap order from 0.0 and rounded
//                       to float once -- the oracle's restatement of fftFilter
//                       (FIRFilter.cs:96-141; MathNet's FFT itself is absent
//                       here) -- and then quantised.
//                       QPSK_MOD_NORM_PEAK runs it twice: a pass that only forms
//                       each row's largest |component|, then the pass that
//                       quantises by it (the convolution is recomputed, no float
//                       scratch row: DESIGN.md §3.14).
//
// Not the demodulation hot path: it generates transmit baseband on the GPU the
// way the reference's TX does.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "qpsk_demod.h"
#include "qpsk_design.h"
#include "qpsk_device.h"
#include "qpsk_internal.h"
#include "qpsk_quantise.h"

struct qpsk_mod {
    qpsk_mod_params p{};
    int T = 0;
    int sps = 0;
    int delay = 0;
    std::string tsc;           // "" = none (string.IsNullOrWhiteSpace)
    qpsk::Stream stream;           // in front of the buffers, which go first
    qpsk::DevBuf<double> d_hs;     // (double)(float)tap * (double)InvSqrt2, T: exact products
    qpsk::DevBuf<uint8_t> d_tsc;   // TSC as packed bits
    // per-call device staging (grown as needed)
    qpsk::DevBuf<uint8_t> d_marks;   // START then END
    qpsk::DevBuf<uint8_t> d_quad;
    qpsk::DevBuf<uint8_t> d_rows;    // host calls: the bit or payload rows
    qpsk::DevBuf<int64_t> d_counts;  // every call: the checked per-stream counts
    qpsk::DevBuf<uint8_t> d_out;     // host calls: 16-byte-pitched output rows
    qpsk::DevBuf<float> d_peak;      // host calls: the rows' peaks
};

namespace {

using qpsk::fail;

constexpr float kInvSqrt2 = 0.7071067811865475f;   // QPSKModulator.cs:36
constexpr int kTile = QPSK_MOD_TILE_SAMPLES;
constexpr int kScanThreads = 256;
constexpr int kScanDibits = QPSK_MOD_SCAN_DIBITS;   // four a lane
static_assert(kScanDibits == 4 * kScanThreads, "a lane of the scan takes one byte of dibits");
constexpr int kMaxStreams = 65535;      // the streams run on grid dimension y
// what one workgroup may stage: five workgroups share a CU's 160 KiB; a filter
// past about 4000 taps is read from global memory instead
constexpr size_t kLdsBudget = 32 * 1024;
enum { kPassFixed = 0, kPassMax = 1, kPassPeak = 2 };

// The logical bit string of stream s: tsc | START | row[s] | END.  Modulate has
// empty markers and counts bits (unit 1), ModulateBytes counts bytes (unit 8).
struct BitString {
    const uint8_t *tsc;
    const uint8_t *marks;      // START's bytes, then END's
    const uint8_t *rows;       // [S][row_stride]
    int64_t row_stride;
    const int64_t *counts;     // [S], checked on the host
    int64_t tsc_bits, start_bits, end_bits;
    int unit;
};

__device__ __forceinline__ int64_t string_bits(const BitString &b, int s) {
    return b.tsc_bits + b.start_bits + b.counts[s] * b.unit + b.end_bits;
}

struct SymArgs {
    BitString str;
    int differential;
    uint8_t *quad;             // [S][quad_stride] symbol quadrants, stride = 0 mod 4
    int64_t quad_stride;
};

struct SampArgs {
    BitString str;
    const uint8_t *quad;
    int64_t quad_stride;
    const double *hs;
    int T, sps, delay, pulse;
    void *out;                 // [S][out_stride] elements of the format
    int64_t out_stride;
    int vec;                   // rows take 16-byte stores
    int pass;
    float scale;
    float *peak;               // [S]: kPassMax raises it, kPassPeak reads it
    int stage;                 // taps and quadrants fit in LDS
};

// bits [a, b) of a packed MSB-first piece, right-aligned; 0 < b - a <= 8
__device__ __forceinline__ uint32_t piece_bits(const uint8_t *p, int64_t a, int64_t b) {
    const int sh = static_cast<int>(a & 7), n = static_cast<int>(b - a);
    uint32_t w = static_cast<uint32_t>(p[a >> 3]) << 8;
    if (sh + n > 8) w |= p[(a >> 3) + 1];   // bit b - 1 lies in that byte
    return (w >> (16 - sh - n)) & ((1u << n) - 1u);
}

// logical bits [i0, i0 + 8) of stream s, bit i0 in bit 7; 0 past the string
__device__ __forceinline__ uint32_t window8(const BitString &b, int s, int64_t i0) {
    uint32_t w = 0;
    int64_t start = 0;
    auto take = [&](const uint8_t *p, int64_t len) {
        const int64_t lo = i0 > start ? i0 : start, hi = i0 + 8 < start + len ? i0 + 8 : start + len;
        if (lo < hi) w |= piece_bits(p, lo - start, hi - start) << (i0 + 8 - hi);
        start += len;
    };
    take(b.tsc, b.tsc_bits);
    take(b.marks, b.start_bits);
    take(b.rows + s * b.row_stride, b.counts[s] * b.unit);
    take(b.marks + (b.start_bits >> 3), b.end_bits);
    return w;
}

// quadrant k <-> (+-InvSqrt2, +-InvSqrt2): 0 (+,+), 1 (-,+), 2 (-,-), 3 (+,-)
__global__ __launch_bounds__(kScanThreads) void mod_symbols_kernel(SymArgs a) {
    __shared__ int wave_sum[kScanThreads / 64];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t nd = string_bits(a.str, s) >> 1;   // "must have pairs of bits" (:113)
    uint32_t *q = reinterpret_cast<uint32_t *>(a.quad + s * a.quad_stride);
    int carry = 0;                   // the differential reference (1/sqrt2)(1+j) is quadrant 0
    for (int64_t c0 = 0; c0 < nd; c0 += kScanDibits) {
        const int64_t d0 = c0 + 4 * tid;
        const uint32_t w = d0 < nd ? window8(a.str, s, 2 * d0) : 0u;
        uint32_t packed = 0;
        if (a.differential) {
            // DibitToDelta: 00 -> +1, 01 -> +j, 11 -> -1, 10 -> -j, i.e. a rotation
            // by 0, 1, 2, 3 quarter turns (the dibit's Gray decoding); prev * delta
            // of +-InvSqrt2 components with a unit axis phasor is exact in float
            int run[4], acc = 0;
            for (int j = 0; j < 4; ++j) {
                const uint32_t k = (w >> (6 - 2 * j)) & 3u;
                acc += static_cast<int>(k ^ (k >> 1));
                run[j] = acc;
            }
            int x = acc;             // inclusive scan of the lanes' sums over the wave
            for (int off = 1; off < 64; off <<= 1) {
                const int v = __shfl_up(x, off, 64);
                if (lane >= off) x += v;
            }
            if (lane == 63) wave_sum[wave] = x;
            __syncthreads();
            int before = carry + x - acc, all = 0;
            for (int k = 0; k < kScanThreads / 64; ++k) {
                if (k < wave) before += wave_sum[k];
                all += wave_sum[k];
            }
            __syncthreads();         // wave_sum is rewritten in the next pass
            carry = (carry + all) & 3;
            for (int j = 0; j < 4; ++j) packed |= static_cast<uint32_t>((before + run[j]) & 3) << (8 * j);
        } else {
            // symI = bi == 0 ? -InvSqrt2 : InvSqrt2, symQ likewise with bq
            for (int j = 0; j < 4; ++j) {
                const uint32_t bi = (w >> (7 - 2 * j)) & 1u, bq = (w >> (6 - 2 * j)) & 1u;
                packed |= (bi ? (bq ? 0u : 3u) : (bq ? 1u : 2u)) << (8 * j);
            }
        }
        if (d0 < nd) q[d0 >> 2] = packed;   // up to three bytes past nd, inside the padded row
    }
}

// what a format stores: its element, the samples in 16 bytes, and one sample as
// a single word
template <int kFmt> struct Elem;
template <> struct Elem<QPSK_FMT_CF32> { using type = float; using sample = float2; };
template <> struct Elem<QPSK_FMT_CS16> { using type = int16_t; using sample = uint32_t; };
template <> struct Elem<QPSK_FMT_CS8> { using type = int8_t; using sample = uint16_t; };
template <> struct Elem<QPSK_FMT_CU8> { using type = uint8_t; using sample = uint16_t; };
template <int kFmt> constexpr int kRun = 8 / static_cast<int>(sizeof(typename Elem<kFmt>::type));

template <int kFmt>
__device__ __forceinline__ typename Elem<kFmt>::type stored(float x, int pass, float scale, double max_val) {
    using E = typename Elem<kFmt>::type;
    if constexpr (kFmt == QPSK_FMT_CF32) return qpsk::quant_scaled(x, scale);
    else return static_cast<E>(pass == kPassPeak ? qpsk::quant_peak(kFmt, x, max_val) : qpsk::quant_fixed(kFmt, x, scale));
}

// One lane's run of samples of tile [t0, ...) of stream s: hs and q come from
// LDS (q holds the quadrants from q0 on) or from global memory (q0 = 0).
template <int kFmt>
__device__ __forceinline__ void tile_body(const SampArgs &a, int s, int64_t nd, int64_t total, int64_t t0,
                                          const double *hs, const uint8_t *q, int64_t q0) {
    using E = typename Elem<kFmt>::type;
    using Sample = typename Elem<kFmt>::sample;
    constexpr int R = kRun<kFmt>;
    const int64_t i0 = t0 + static_cast<int64_t>(threadIdx.x) * R;
    float v[2 * R];
    for (int r = 0; r < R; ++r) {
        const int64_t i = i0 + r;
        float vi = 0.f, vq = 0.f;
        if (i < total && !a.pulse) {
            // the impulse train itself (:160-161)
            const int64_t rel = i - a.delay;
            if (rel >= 0 && rel % a.sps == 0 && rel / a.sps < nd) {
                const int k = q[rel / a.sps - q0];
                vi = (k == 1 || k == 2) ? -kInvSqrt2 : kInvSqrt2;
                vq = k >= 2 ? -kInvSqrt2 : kInvSqrt2;
            }
        } else if (i < total) {
            // y[i] = sum_m taps[m] * up[T-1+i-m], m ascending; up[j] holds symbol d at
            // j = delay + d*sps (zeros elsewhere add nothing), fftFilter's slice at T-1
            double ar = 0.0, ai = 0.0;
            const int64_t top = a.T - 1 + i - a.delay;      // = m + d*sps for the tap m of symbol d
            // m ascending <=> d descending; m = top - d*sps in [0, T) and d in [0, nd)
            int64_t dhi = top / a.sps;
            if (dhi > nd - 1) dhi = nd - 1;
            const int64_t dlo = i > a.delay ? (i - a.delay + a.sps - 1) / a.sps : 0;
            int m = static_cast<int>(top - dhi * a.sps);
            int64_t qi = dhi - q0;
            for (int64_t n = dhi - dlo; n >= 0; --n, --qi, m += a.sps) {
                const int k = q[qi];
                // (double)tap * (double)(+-InvSqrt2): the product of two floats is exact
                // in double, so its sign is the only thing the quadrant decides
                const double h = hs[m];
                ar += (k == 1 || k == 2) ? -h : h;
                ai += k >= 2 ? -h : h;
            }
            vi = static_cast<float>(ar);
            vq = static_cast<float>(ai);
        }
        v[2 * r] = vi;
        v[2 * r + 1] = vq;
    }
    if (a.pass == kPassMax) {
        // |x| of a non-negative float orders as its bit pattern does
        float mx = 0.f;
        for (int r = 0; r < 2 * R; ++r) mx = fmaxf(mx, fabsf(v[r]));   // 0 past the row
        for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        if ((threadIdx.x & 63) == 0 && mx > 0.f) atomicMax(reinterpret_cast<unsigned int *>(a.peak + s), __float_as_uint(mx));
        return;
    }
    if (i0 >= total) return;
    const double max_val = a.pass == kPassPeak ? qpsk::quant_peak_divisor(a.peak[s]) : 1.0;
    alignas(16) E e[2 * R];
    for (int r = 0; r < 2 * R; ++r) e[r] = stored<kFmt>(v[r], a.pass, a.scale, max_val);
    E *row = static_cast<E *>(a.out) + s * a.out_stride;
    if (a.vec && i0 + R <= total) {
        uint4 w;
        __builtin_memcpy(&w, e, sizeof(w));
        *reinterpret_cast<uint4 *>(row + 2 * i0) = w;
    } else {
        // the scalar layout, and the last partial vector of a row
        for (int r = 0; r < R && i0 + r < total; ++r) {
            Sample w;
            __builtin_memcpy(&w, e + 2 * r, sizeof(w));
            *reinterpret_cast<Sample *>(row + 2 * (i0 + r)) = w;
        }
    }
}

template <int kFmt>
__global__ __launch_bounds__(kTile / kRun<kFmt>) void mod_samples_kernel(SampArgs a) {
    extern __shared__ double lds_hs[];   // T taps, then the tile's quadrants
    const int s = blockIdx.y;
    const int64_t nd = string_bits(a.str, s) >> 1;
    const int64_t base_c = a.delay + nd * a.sps;
    const int64_t total = nd == 0 ? 0 : (a.pulse ? base_c + a.delay : base_c);
    const int64_t t0 = static_cast<int64_t>(blockIdx.x) * kTile;
    if (t0 >= total) return;             // the whole workgroup
    const uint8_t *qrow = a.quad + s * a.quad_stride;
    if (!a.stage) {
        tile_body<kFmt>(a, s, nd, total, t0, a.hs, qrow, 0);
        return;
    }
    // quadrants sample i touches: ceil((i - delay) / sps) ... min((T-1+i-delay) / sps, nd-1)
    const int64_t t1 = (t0 + kTile < total ? t0 + kTile : total) - 1;
    const int64_t q0 = t0 > a.delay ? (t0 - a.delay + a.sps - 1) / a.sps : 0;
    int64_t q1 = (a.T - 1 + t1 - a.delay) / a.sps;
    if (q1 > nd - 1) q1 = nd - 1;
    uint8_t *lds_q = reinterpret_cast<uint8_t *>(lds_hs + a.T);
    if (a.pulse)
        for (int m = threadIdx.x; m < a.T; m += blockDim.x) lds_hs[m] = a.hs[m];
    for (int64_t k = threadIdx.x; k <= q1 - q0; k += blockDim.x) lds_q[k] = qrow[q0 + k];
    __syncthreads();
    tile_body<kFmt>(a, s, nd, total, t0, lds_hs, lds_q, q0);
}

template <int kFmt>
void launch_samples(const SampArgs &a, dim3 grid, size_t lds, hipStream_t st) {
    hipLaunchKernelGGL(mod_samples_kernel<kFmt>, grid, dim3(kTile / kRun<kFmt>), lds, st, a);
}

void launch_samples(int fmt, const SampArgs &a, dim3 grid, size_t lds, hipStream_t st) {
    switch (fmt) {
    case QPSK_FMT_CF32: return launch_samples<QPSK_FMT_CF32>(a, grid, lds, st);
    case QPSK_FMT_CS16: return launch_samples<QPSK_FMT_CS16>(a, grid, lds, st);
    case QPSK_FMT_CS8: return launch_samples<QPSK_FMT_CS8>(a, grid, lds, st);
    default: return launch_samples<QPSK_FMT_CU8>(a, grid, lds, st);
    }
}

// what a failed grow of a staging buffer names (alloc_status)
constexpr const char *kStaging = "modulator staging";

bool blank(const char *s) {
    if (!s) return true;
    for (; *s; ++s)
        if (!(*s == ' ' || (*s >= '\t' && *s <= '\r'))) return false;
    return true;
}

// complex samples of a row whose logical bit string has n_bits bits
int64_t out_complex(const qpsk_mod *m, int64_t n_bits, int pulse) {
    const int64_t nd = n_bits >> 1;
    if (nd == 0) return 0;
    const int64_t base_c = m->delay + nd * m->sps;
    return pulse ? base_c + m->delay : base_c;
}

// One call of either entry point.  rows holds counts[s] bits (unit 1) or bytes
// (unit 8) a stream; the markers are empty for Modulate.
struct Call {
    int32_t fmt, norm;
    float scale;
    int32_t S;
    const uint8_t *rows;
    int64_t row_stride;
    const int64_t *counts;
    int unit;
    const uint8_t *start;
    int32_t n_start;
    const uint8_t *end;
    int32_t n_end;
    int32_t pulse, mem;
    void *out;
    int64_t out_stride;
    int64_t *n_out;
    float *peak;
};

// the checks that need no handle and no device, in one order for both entry points
int check_format(const Call &c) {
    if (!qpsk::fmt_known(c.fmt)) return fail(QPSK_ERR_ARGUMENT, "unknown sample format");
    if (c.norm != QPSK_MOD_NORM_FIXED && c.norm != QPSK_MOD_NORM_PEAK) return fail(QPSK_ERR_ARGUMENT, "unknown norm");
    if (c.norm == QPSK_MOD_NORM_PEAK && c.fmt == QPSK_FMT_CF32)
        return fail(QPSK_ERR_ARGUMENT, "QPSK_MOD_NORM_PEAK needs an integer format");
    if (c.norm == QPSK_MOD_NORM_FIXED && !qpsk::quant_scale_ok(c.scale))
        return fail(QPSK_ERR_OUT_OF_RANGE, "scale must be finite and > 0");
    return QPSK_OK;
}

int modulate(qpsk_mod *m, const Call &c) {
    int rc;
    if ((rc = check_format(c))) return rc;
    if (c.S <= 0) return fail(QPSK_ERR_ARGUMENT, "n_streams must be positive");
    if (c.S > kMaxStreams) return fail(QPSK_ERR_ARGUMENT, "n_streams exceeds 65535, the grid dimension the streams run on");
    if (!c.counts || !c.out || !c.n_out) return fail(QPSK_ERR_ARGUMENT_NULL, "data is null");
    if (c.norm == QPSK_MOD_NORM_PEAK && !c.peak) return fail(QPSK_ERR_ARGUMENT_NULL, "peak is null");
    if (c.mem != QPSK_MEM_HOST && c.mem != QPSK_MEM_DEVICE) return fail(QPSK_ERR_ARGUMENT, "unknown mem");
    const int S = c.S;
    const bool host = c.mem == QPSK_MEM_HOST, peak_norm = c.norm == QPSK_MOD_NORM_PEAK;
    const int pulse = c.pulse != 0;
    const int64_t elem = qpsk::fmt_elem_bytes(c.fmt);
    std::vector<int64_t> cnt(S);
    if (host) std::memcpy(cnt.data(), c.counts, S * sizeof(int64_t));
    else QPSK_HIP_TRY(hipMemcpy(cnt.data(), c.counts, S * sizeof(int64_t), hipMemcpyDeviceToHost));
    const int64_t fixed_bits = static_cast<int64_t>(m->tsc.size()) + 8 * (static_cast<int64_t>(c.n_start) + c.n_end);
    int64_t cnt_max = 0;
    for (int s = 0; s < S; ++s) {
        if (cnt[s] < 0) return fail(QPSK_ERR_ARGUMENT, c.unit == 1 ? "negative bit count" : "negative payload length");
        if (cnt[s] > (INT64_MAX >> 8)) return fail(QPSK_ERR_ARGUMENT, "row too long");
        cnt_max = std::max(cnt_max, cnt[s]);
    }
    const int64_t row_bytes = c.unit == 1 ? (cnt_max + 7) / 8 : cnt_max;   // of the longest row
    if (cnt_max > 0 && (!c.rows || c.row_stride < row_bytes))
        return c.unit == 1 ? fail(c.rows ? QPSK_ERR_ARGUMENT : QPSK_ERR_ARGUMENT_NULL, "bit rows too short")
                           : fail(QPSK_ERR_ARGUMENT, "payload rows too short");
    const int64_t nd_max = (fixed_bits + cnt_max * c.unit) >> 1;
    const int64_t tot_max = out_complex(m, fixed_bits + cnt_max * c.unit, pulse);
    if (c.out_stride < 2 * tot_max) return fail(QPSK_ERR_ARGUMENT, "out_stride too small");
    const int64_t tiles = (tot_max + kTile - 1) / kTile;
    if (tiles > INT32_MAX) return fail(QPSK_ERR_ARGUMENT, "rows too long for one launch");
    if (!host) {
        // one complex sample is one store at the least
        if (reinterpret_cast<uintptr_t>(c.out) % (2 * elem) || (c.out_stride & 1))
            return fail(QPSK_ERR_ARGUMENT, "device output rows must be aligned to one complex sample, with an even stride");
        if (peak_norm && reinterpret_cast<uintptr_t>(c.peak) % sizeof(float))
            return fail(QPSK_ERR_ARGUMENT, "peak must be 4-byte aligned");
    }
    QPSK_HIP_TRY(hipSetDevice(m->p.device));
    hipStream_t st = m->stream;
    SampArgs a{};
    BitString &str = a.str;
    str.tsc = m->d_tsc;
    str.tsc_bits = static_cast<int64_t>(m->tsc.size());
    str.start_bits = 8 * static_cast<int64_t>(c.n_start);
    str.end_bits = 8 * static_cast<int64_t>(c.n_end);
    str.unit = c.unit;
    str.rows = c.rows;
    str.row_stride = c.row_stride;
    // the kernels read the counts the host checked, never the caller's device copy
    if ((rc = qpsk::alloc_status(m->d_counts.grow(S * sizeof(int64_t)), kStaging))) return rc;
    QPSK_HIP_TRY(hipMemcpyAsync(m->d_counts, cnt.data(), S * sizeof(int64_t), hipMemcpyHostToDevice, st));
    str.counts = m->d_counts;
    std::vector<uint8_t> marks(static_cast<size_t>(c.n_start) + c.n_end);   // lives until the call's synchronise
    if (!marks.empty()) {
        std::memcpy(marks.data(), c.start, c.n_start);
        std::memcpy(marks.data() + c.n_start, c.end, c.n_end);
        if ((rc = qpsk::alloc_status(m->d_marks.grow(marks.size()), kStaging))) return rc;
        QPSK_HIP_TRY(hipMemcpyAsync(m->d_marks, marks.data(), marks.size(), hipMemcpyHostToDevice, st));
    }
    str.marks = m->d_marks;
    a.out = c.out;
    a.out_stride = c.out_stride;
    a.peak = c.peak;
    if (host) {
        const size_t brow = static_cast<size_t>(row_bytes + 1);
        if ((rc = qpsk::alloc_status(m->d_rows.grow(S * brow), kStaging))) return rc;
        if (cnt_max > 0)
            QPSK_HIP_TRY(hipMemcpy2DAsync(m->d_rows, brow, c.rows, c.row_stride, row_bytes, S, hipMemcpyHostToDevice, st));
        str.rows = m->d_rows;
        str.row_stride = static_cast<int64_t>(brow);
        // 16-byte-pitched rows: the wide stores
        const int64_t pitch = (2 * std::max<int64_t>(tot_max, 1) * elem + 15) / 16 * 16;
        if ((rc = qpsk::alloc_status(m->d_out.grow(static_cast<size_t>(S) * pitch), kStaging))) return rc;
        a.out = m->d_out;
        a.out_stride = pitch / elem;
        if (peak_norm) {
            if ((rc = qpsk::alloc_status(m->d_peak.grow(S * sizeof(float)), kStaging))) return rc;
            a.peak = m->d_peak;
        }
    }
    a.vec = reinterpret_cast<uintptr_t>(a.out) % 16 == 0 && (a.out_stride * elem) % 16 == 0;
    const int64_t quad_stride = (std::max<int64_t>(nd_max, 1) + 3) / 4 * 4;
    if ((rc = qpsk::alloc_status(m->d_quad.grow(static_cast<size_t>(S) * quad_stride), kStaging))) return rc;
    a.quad = m->d_quad;
    a.quad_stride = quad_stride;
    a.hs = m->d_hs;
    a.T = m->T;
    a.sps = m->sps;
    a.delay = m->delay;
    a.pulse = pulse;
    a.scale = c.scale;
    // T doubles and the quadrants of one tile: (T - 1 + kTile - 1) / sps + 2 at the most
    const size_t lds = static_cast<size_t>(m->T) * sizeof(double) + static_cast<size_t>((m->T + kTile) / m->sps + 2);
    a.stage = lds <= kLdsBudget;
    if (peak_norm) QPSK_HIP_TRY(hipMemsetAsync(a.peak, 0, S * sizeof(float), st));   // the maximum starts at +0
    if (tot_max > 0) {
        SymArgs sy{};
        sy.str = str;
        sy.differential = m->p.differential;
        sy.quad = m->d_quad;
        sy.quad_stride = quad_stride;
        hipLaunchKernelGGL(mod_symbols_kernel, dim3(S), dim3(kScanThreads), 0, st, sy);
        const dim3 grid(static_cast<unsigned>(tiles), static_cast<unsigned>(S));
        const size_t dyn = a.stage ? lds : 0;
        if (peak_norm) {
            a.pass = kPassMax;
            launch_samples(c.fmt, a, grid, dyn, st);
        }
        a.pass = peak_norm ? kPassPeak : kPassFixed;
        launch_samples(c.fmt, a, grid, dyn, st);
        QPSK_HIP_TRY(hipGetLastError());
    }
    std::vector<int64_t> nout(S);
    for (int s = 0; s < S; ++s) nout[s] = 2 * out_complex(m, fixed_bits + cnt[s] * c.unit, pulse);
    if (host) {
        if (tot_max > 0)
            QPSK_HIP_TRY(hipMemcpy2DAsync(c.out, c.out_stride * elem, a.out, a.out_stride * elem, 2 * tot_max * elem, S,
                                          hipMemcpyDeviceToHost, st));
        if (peak_norm) QPSK_HIP_TRY(hipMemcpyAsync(c.peak, a.peak, S * sizeof(float), hipMemcpyDeviceToHost, st));
        QPSK_HIP_TRY(hipStreamSynchronize(st));
        std::memcpy(c.n_out, nout.data(), S * sizeof(int64_t));
    } else {
        QPSK_HIP_TRY(hipMemcpyAsync(c.n_out, nout.data(), S * sizeof(int64_t), hipMemcpyHostToDevice, st));
        QPSK_HIP_TRY(hipStreamSynchronize(st));   // cnt, marks and nout are host temporaries
    }
    return QPSK_OK;
}

}  // namespace

extern "C" {

void qpsk_mod_params_init(qpsk_mod_params *p, int32_t sample_rate, int32_t symbol_rate) {
    std::memset(p, 0, sizeof(*p));
    p->sample_rate = sample_rate;
    p->symbol_rate = symbol_rate;
    p->rrc_alpha = 0.9;          // QPSKModulator.cs:18-24 defaults
    p->rrc_span = 6;
    p->differential = 1;
    p->device = 0;
}

int qpsk_mod_create(const qpsk_mod_params *p, const char *tsc, qpsk_mod **out) {
    if (!p || !out) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    *out = nullptr;
    if (p->symbol_rate <= 0) return fail(QPSK_ERR_OUT_OF_RANGE, "SymbolRate must be positive");
    if (tsc && !blank(tsc))
        for (const char *c = tsc; *c; ++c)
            if (*c != '0' && *c != '1') return fail(QPSK_ERR_ARGUMENT, "tsc must be a '0'/'1' string");
    std::vector<double> h = qpsk::rrc_coefficients(static_cast<double>(p->rrc_span), p->rrc_alpha,
                                                   p->sample_rate, p->symbol_rate);
    if (h.empty()) return fail(QPSK_ERR_ARGUMENT, "RRC design failed");
    auto *m = new qpsk_mod();
    m->p = *p;
    m->T = static_cast<int>(h.size());
    m->sps = p->sample_rate / p->symbol_rate;                  // :115 (integer division)
    m->delay = (m->T - 1) / 2;                                  // :119
    m->tsc = blank(tsc) ? std::string() : std::string(tsc);    // :26
    std::vector<double> hs(m->T);
    for (int k = 0; k < m->T; ++k)   // the float tap (ToInterleavedIQRealTapsStatic) times the float InvSqrt2, in double
        hs[k] = static_cast<double>(static_cast<float>(h[k])) * static_cast<double>(kInvSqrt2);
    std::vector<uint8_t> tb((m->tsc.size() + 7) / 8 + 1, 0);
    for (size_t i = 0; i < m->tsc.size(); ++i)
        if (m->tsc[i] == '1') tb[i >> 3] |= static_cast<uint8_t>(0x80u >> (i & 7));
    if (hipSetDevice(p->device) != hipSuccess || m->stream.create(hipStreamNonBlocking) != hipSuccess ||
        m->d_hs.alloc(m->T) != hipSuccess || m->d_tsc.alloc(tb.size()) != hipSuccess ||
        m->d_marks.alloc(16) != hipSuccess ||
        hipMemcpy(m->d_hs, hs.data(), m->T * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(m->d_tsc, tb.data(), tb.size(), hipMemcpyHostToDevice) != hipSuccess) {
        qpsk_mod_destroy(m);
        return fail(QPSK_ERR_DEVICE, "modulator device set-up failed (no GPU?)");
    }
    *out = m;
    return QPSK_OK;
}

int qpsk_mod_destroy(qpsk_mod *m) {
    if (!m) return QPSK_OK;
    if (m->stream) hipStreamSynchronize(m->stream);
    delete m;
    return QPSK_OK;
}

int qpsk_mod_set_stream(qpsk_mod *m, void *hip_stream) {
    if (!m) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    QPSK_HIP_TRY(hipStreamSynchronize(m->stream));
    QPSK_HIP_TRY(m->stream.rebind(hip_stream));
    return QPSK_OK;
}

int64_t qpsk_mod_output_floats(const qpsk_mod *m, int64_t n_bits, int32_t pulse_shaping) {
    if (!m) return 0;
    return 2 * out_complex(m, static_cast<int64_t>(m->tsc.size()) + std::max<int64_t>(0, n_bits), pulse_shaping != 0);
}

int qpsk_mod_modulate_fmt(qpsk_mod *m, int32_t fmt, int32_t norm, float scale, int32_t n_streams, const uint8_t *bits,
                          int64_t bits_stride_bytes, const int64_t *n_bits, int32_t pulse_shaping, int32_t mem,
                          void *out, int64_t out_stride_elems, int64_t *n_out_elems, float *peak) {
    if (!m) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    return modulate(m, Call{fmt, norm, scale, n_streams, bits, bits_stride_bytes, n_bits, 1, nullptr, 0, nullptr, 0,
                            pulse_shaping, mem, out, out_stride_elems, n_out_elems, peak});
}

int qpsk_mod_modulate_bytes_fmt(qpsk_mod *m, int32_t fmt, int32_t norm, float scale, int32_t n_streams,
                                const uint8_t *payload, int64_t payload_stride, const int64_t *n_payload,
                                const uint8_t *start_marker, int32_t n_start, const uint8_t *end_marker, int32_t n_end,
                                int32_t pulse_shaping, int32_t mem, void *out, int64_t out_stride_elems,
                                int64_t *n_out_elems, float *peak) {
    if (!m) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    if (n_start <= 0 || !start_marker) return fail(QPSK_ERR_ARGUMENT, "startMarker cannot be empty.");
    if (n_end <= 0 || !end_marker) return fail(QPSK_ERR_ARGUMENT, "endMarker cannot be empty.");
    if (n_streams <= 0 || !n_payload) return fail(QPSK_ERR_ARGUMENT_NULL, "payload is null");
    // START + payload + END (QPSKModulator.cs:54-72), bits MSB-first
    // (BitPacker.BytesToBitString, HelperFunctions.cs:14-29)
    return modulate(m, Call{fmt, norm, scale, n_streams, payload, payload_stride, n_payload, 8, start_marker, n_start,
                            end_marker, n_end, pulse_shaping, mem, out, out_stride_elems, n_out_elems, peak});
}

int qpsk_mod_modulate(qpsk_mod *m, int32_t n_streams, const uint8_t *bits, int64_t bits_stride_bytes,
                      const int64_t *n_bits, int32_t pulse_shaping, int32_t mem, float *out,
                      int64_t out_stride_floats, int64_t *n_out_floats) {
    return qpsk_mod_modulate_fmt(m, QPSK_FMT_CF32, QPSK_MOD_NORM_FIXED, 1.0f, n_streams, bits, bits_stride_bytes,
                                 n_bits, pulse_shaping, mem, out, out_stride_floats, n_out_floats, nullptr);
}

int qpsk_mod_modulate_bytes(qpsk_mod *m, int32_t n_streams, const uint8_t *payload, int64_t payload_stride,
                            const int64_t *n_payload, const uint8_t *start_marker, int32_t n_start,
                            const uint8_t *end_marker, int32_t n_end, int32_t pulse_shaping, float *out,
                            int64_t out_stride_floats, int64_t *n_out_floats) {
    return qpsk_mod_modulate_bytes_fmt(m, QPSK_FMT_CF32, QPSK_MOD_NORM_FIXED, 1.0f, n_streams, payload, payload_stride,
                                       n_payload, start_marker, n_start, end_marker, n_end, pulse_shaping,
                                       QPSK_MEM_HOST, out, out_stride_floats, n_out_floats, nullptr);
}

}  // extern "C"
