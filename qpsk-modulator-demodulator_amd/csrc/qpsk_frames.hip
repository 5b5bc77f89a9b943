// qpsk_frames.hip -- the frames one DeModulateBytes step returned over a batch,
// packed densely (qpsk_frames_pack_device).
//
// qpsk_framer_dev_push leaves [S][P] payload rows and [S] lengths; on real
// traffic almost every row is empty (a chunk completes a frame on few
// streams).  A caller that wants the frames and nothing else would still read
// S * P bytes back.  Here the rows that hold a frame are copied behind one
// another into one buffer, so the read-back is the frames' bytes.
//
// The packing rule (include/qpsk_demod.h), with L_s =
// n_payload[s]:
//     k_s = min(L_s, P)      bytes of the frame the row holds
//     a_s = k_s rounded up to 16
//     E_s = sum of a_t over t < s               (int64)
//     stream s is stored iff k_s > 0 and E_s + a_s <= C
//     offsets[s] = E_s if stored, else -1
//     packed[E_s .. E_s + a_s) = the k_s bytes, then zeros
//     head[0] = the largest E_s + a_s over stored streams (0 if none)
//     head[1] = 1 * (some L_s > P)  |  2 * (some k_s > 0 not stored)
// E_s counts the earlier frames whether stored or not, so once one frame does
// not fit no later one does, and packed[0 .. head[0]) is dense.
//
// Two kernels: an exclusive scan of a_s over the streams (one workgroup, wave
// scan by shuffles, wave totals and the running carry through LDS), then the
// copy, whole 16-byte words over a (stream, segment) grid with the row's
// stale bytes past k_s masked to zero.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "qpsk_demod.h"
#include "qpsk_internal.h"

namespace {
using qpsk::fail;

constexpr int kScanThreads = 1024;                 // streams per scan block
constexpr int kScanWaves = kScanThreads / 64;
constexpr int kCopyThreads = 256;                  // 16-byte words per segment

__device__ inline int64_t held_bytes(int64_t L, int64_t P) { return L <= 0 ? 0 : (L < P ? L : P); }

__global__ void __launch_bounds__(kScanThreads)
frames_scan_kernel(const int64_t *n_payload, int32_t S, int64_t P, int64_t C, int64_t *offsets, int64_t *head) {
    __shared__ int64_t wave_sum[kScanWaves];
    __shared__ unsigned long long total;
    __shared__ unsigned int flags;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    if (tid == 0) {
        total = 0;
        flags = 0;
    }
    int64_t carry = 0;                              // a_t summed over the earlier blocks
    int64_t my_total = 0;
    unsigned int my_flags = 0;
    for (int64_t s0 = 0; s0 < S; s0 += kScanThreads) {
        const int64_t s = s0 + tid;
        const int64_t L = s < S ? n_payload[s] : 0;
        const int64_t k = held_bytes(L, P);
        const int64_t a = (k + 15) & ~static_cast<int64_t>(15);
        // inclusive scan of a over the wave's 64 lanes
        int64_t incl = a;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        __syncthreads();                            // the previous block's wave_sum has been read
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        int64_t before = carry;                     // earlier blocks, then the earlier waves of this one
        int64_t block = 0;
        for (int w = 0; w < kScanWaves; ++w) {
            if (w < wave) before += wave_sum[w];
            block += wave_sum[w];
        }
        carry += block;
        if (s < S) {
            const int64_t E = before + incl - a;
            const bool stored = k > 0 && E + a <= C;
            offsets[s] = stored ? E : -1;
            if (stored && E + a > my_total) my_total = E + a;
            if (L > P) my_flags |= QPSK_FRAMES_TRUNCATED;
            if (k > 0 && !stored) my_flags |= QPSK_FRAMES_DROPPED;
        }
    }
    __syncthreads();                                // total and flags are zeroed
    if (my_total) atomicMax(&total, static_cast<unsigned long long>(my_total));
    if (my_flags) atomicOr(&flags, my_flags);
    __syncthreads();
    if (tid == 0) {
        head[0] = static_cast<int64_t>(total);
        head[1] = flags;
    }
}

// 16 bytes of a row from byte b on, at any alignment of the row
__device__ inline uint4 load16(const uint8_t *row, int64_t b, bool aligned) {
    if (aligned) return *reinterpret_cast<const uint4 *>(row + b);
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
        w[i] = static_cast<uint32_t>(row[b + 4 * i]) | (static_cast<uint32_t>(row[b + 4 * i + 1]) << 8) |
               (static_cast<uint32_t>(row[b + 4 * i + 2]) << 16) | (static_cast<uint32_t>(row[b + 4 * i + 3]) << 24);
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// the low `keep` bytes (0..4) of a little-endian word
__device__ inline uint32_t keep_bytes(uint32_t w, int64_t keep) {
    return keep >= 4 ? w : (keep <= 0 ? 0u : w & ((1u << (8 * static_cast<int>(keep))) - 1u));
}

// blockIdx.x = stream, blockIdx.y = first segment of kCopyThreads words; a
// stored frame's a_s / 16 words go to packed + offsets[s]
__global__ void __launch_bounds__(kCopyThreads)
frames_copy_kernel(const uint8_t *payload, int64_t P, const int64_t *n_payload, const int64_t *offsets,
                   uint8_t *packed, int aligned) {
    const int64_t s = blockIdx.x;
    const int64_t off = offsets[s];
    if (off < 0) return;
    const int64_t k = held_bytes(n_payload[s], P);
    const int64_t words = (k + 15) >> 4;
    const uint8_t *row = payload + s * P;
    uint4 *out = reinterpret_cast<uint4 *>(packed + off);
    for (int64_t w = static_cast<int64_t>(blockIdx.y) * kCopyThreads + threadIdx.x; w < words;
         w += static_cast<int64_t>(gridDim.y) * kCopyThreads) {
        uint4 v = load16(row, 16 * w, aligned != 0);
        const int64_t keep = k - 16 * w;            // > 0; the frame's last word holds fewer than 16
        if (keep < 16) {
            v.x = keep_bytes(v.x, keep);
            v.y = keep_bytes(v.y, keep - 4);
            v.z = keep_bytes(v.z, keep - 8);
            v.w = keep_bytes(v.w, keep - 12);
        }
        out[w] = v;
    }
}

}  // namespace

extern "C" int qpsk_frames_pack_device(const uint8_t *payload, int64_t payload_stride, const int64_t *n_payload,
                                       int32_t n_streams, uint8_t *packed, int64_t packed_cap, int64_t *offsets,
                                       int64_t *head, void *hip_stream) {
    if (!payload || !n_payload || !offsets || !head) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    if (!packed && packed_cap != 0) return fail(QPSK_ERR_ARGUMENT_NULL, "packed is null");
    if (n_streams <= 0) return fail(QPSK_ERR_ARGUMENT, "n_streams must be positive");
    if (payload_stride <= 0 || payload_stride % 16)
        return fail(QPSK_ERR_ARGUMENT, "payload_stride must be a positive multiple of 16");
    if (packed_cap < 0 || packed_cap % 16) return fail(QPSK_ERR_ARGUMENT, "packed_cap must be a multiple of 16, >= 0");
    if (reinterpret_cast<uintptr_t>(packed) % 16) return fail(QPSK_ERR_ARGUMENT, "packed must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(offsets) % 8 || reinterpret_cast<uintptr_t>(head) % 8 ||
        reinterpret_cast<uintptr_t>(n_payload) % 8)
        return fail(QPSK_ERR_ARGUMENT, "offsets, head and n_payload must be 8-byte aligned");
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    hipLaunchKernelGGL(frames_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, n_payload, n_streams,
                       payload_stride, packed_cap, offsets, head);
    QPSK_HIP_TRY(hipGetLastError());
    if (packed_cap > 0) {
        const int64_t row_words = payload_stride / 16;
        const int64_t segs = (row_words + kCopyThreads - 1) / kCopyThreads;
        const int aligned = reinterpret_cast<uintptr_t>(payload) % 16 == 0;
        hipLaunchKernelGGL(frames_copy_kernel, dim3(n_streams, static_cast<unsigned>(segs < 65535 ? segs : 65535)),
                           dim3(kCopyThreads), 0, stream, payload, payload_stride, n_payload, offsets, packed, aligned);
        QPSK_HIP_TRY(hipGetLastError());
    }
    return QPSK_OK;
}
