// qpsk_pfb.hip -- the polyphase channeliser (include/qpsk_demod.h, "The polyphase
// channeliser on the device") on n_bands wideband rows: the two kernels and the
// entry points that need a device.  The per-element functions, the state
// record, the checks, the design and the host form of the call are qpsk_pfb.h /
// qpsk_pfb.cpp.
//
// pfb_kernel: every frame is independent, so one workgroup of 256 threads takes
// one band's run of F = 4096 / M frames, m0 .. m0 + F - 1 (qpsk_pfb_tile_frames):
// F * M = 4096 elements, 16 a thread, whatever M is.
//
//   sums    element e = tid + 256 i is branch p = e mod M of frame f = e / M; its
//           polyphase sum stays in a register over the K taps.  Tap k of the
//           tile's frames reads one window of (F + 1) D inputs,
//           x[(m0 - 2k - 2) D + 1 .. (m0 + F - 1 - 2k) D]: it is staged, widened,
//           into LDS (coalesced, 16 bytes a lane where the rows are 16-byte
//           aligned and pitched, else a sample a lane; indices before the call's
//           first sample come from the state's history), and consecutive p read
//           consecutive LDS addresses.  Two barriers a tap.
//   fft     the sums go to LDS at their bit-reversed places (the window's array,
//           reused), frame f at f * (M + 1): log2 M stages of 2048 butterflies, 8
//           a thread, a barrier a stage.
//   store   transposed: element e is frame e mod F of channel e / F, so a row
//           receives F consecutive samples (the pitch M + 1 keeps that LDS read
//           free of bank conflicts).  Frames past the band's count are computed
//           (on +0 where the row has ended) and not stored.
//
// A workgroup finds its band's frame count itself (pfb_count of the state and
// the call's length, as the host did), so no count is uploaded and a call
// without lengths is queued whole.
//
// pfb_state_kernel runs behind pfb_kernel, when nobody reads the old history
// any more: one workgroup a band moves the new history in, from the call's last
// L samples, or, when the call was shorter than L, the old history down by the
// call's length in chunks of 256 in ascending order (a chunk's reads lie at or
// above its own writes and above every earlier chunk's), then the call's
// samples; lane 0 advances the positions behind a barrier.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "qpsk_demod.h"
#include "qpsk_device.h"
#include "qpsk_internal.h"
#include "qpsk_pfb.h"
#include "qpsk_quantise.h"
#include "qpsk_row_call.h"
#include "qpsk_row_handle.h"
#include "qpsk_sample_rows.h"

struct qpsk_pfb : qpsk::RowHandle {
    qpsk_pfb_params p{};
    int B = 0, M = 0, K = 0, L = 0;
    int64_t each = 0;                        // bytes of one band's state
    qpsk::DevBuf<uint8_t> d_state;           // [B][64 + 8 L]
    qpsk::DevBuf<float> d_taps;              // [L]
    qpsk::DevBuf<float2> d_tw;               // [M / 2]
    std::vector<qpsk::PfbHead> host;         // [B]: the positions as the device will hold them behind the calls
                                             // queued so far
};

namespace {

using qpsk::check_device_rows;
using qpsk::DeviceGuard;
using qpsk::fail;
using qpsk::kPfbTileElems;
using qpsk::load_sample;
using qpsk::pair_rows;
using qpsk::PfbC;
using qpsk::PfbHead;
using qpsk::row_length;

constexpr int kThreads = 256;
constexpr int kPer = kPfbTileElems / kThreads;                         // elements a thread
constexpr int kLds = kPfbTileElems + kPfbTileElems / QPSK_PFB_MIN_CHANNELS;   // F (M + 1) at M = 8
static_assert(kPer * kThreads == kPfbTileElems && kPer % 2 == 0, "a thread's elements and butterflies");
static_assert(kPfbTileElems / 2 + QPSK_PFB_MAX_CHANNELS / 2 <= kLds, "a tap's window of (F + 1) D fits");

struct PfbArgs {
    const void *in;
    float *out;
    int64_t in_stride, out_stride;   // elements
    float scale_in, gain;
    int fmt_in;
    int in_pair, out_pair;           // CF32 rows 8-byte aligned: one access a sample
    int in_wide;                     // input rows 16-byte aligned and pitched
    const int64_t *lengths;          // device, checked; nullptr: n for every band
    int64_t n;
    uint8_t *state;
    int64_t each;                    // bytes of one band's state
    const float *taps;
    const float2 *tw;
    int B, M, K, bits;
};

__global__ __launch_bounds__(kThreads) void pfb_kernel(PfbArgs a) {
    __shared__ float2 lds[kLds];
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const int M = a.M, D = M >> 1, K = a.K, L = M * K, bits = a.bits;
    const int F = kPfbTileElems >> bits;
    const uint8_t *rec = a.state + static_cast<int64_t>(b) * a.each;
    const PfbHead *hd = reinterpret_cast<const PfbHead *>(rec);
    const float(*hist)[2] = reinterpret_cast<const float(*)[2]>(rec + sizeof(PfbHead));
    const int64_t in_pos = hd->in_pos, out_pos = hd->out_pos;
    const int64_t len = row_length(a, b);
    const int64_t total = qpsk::pfb_count(M, out_pos, in_pos + len);
    const int64_t o0 = static_cast<int64_t>(blockIdx.x) * F;
    if (o0 >= total) return;
    const int cnt = total - o0 < F ? static_cast<int>(total - o0) : F;
    const int64_t m0 = out_pos + o0;
    const char *irow = static_cast<const char *>(a.in) + static_cast<int64_t>(b) * a.in_stride * qpsk::fmt_elem_bytes(a.fmt_in);

    // 1. the polyphase sums, a tap at a time
    PfbC acc[kPer];
#pragma unroll
    for (int i = 0; i < kPer; ++i) acc[i] = PfbC{0.0f, 0.0f};
    const int xlen = (F + 1) * D;
    for (int k = 0; k < K; ++k) {
        // lds[0] is x at (m0 - 2k - 2) D + 1 = pfb_index(M, m0, M - 1, k)
        const int64_t j0 = qpsk::pfb_index(M, m0, M - 1, k) - in_pos;
        qpsk::stage_window<kThreads>(lds, j0, xlen, len, irow, hist, L, a, tid);
        __syncthreads();
        const float *hk = a.taps + k * M;
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const int e = tid + kThreads * i;
            const int f = e >> bits, p = e & (M - 1);
            const float2 x = lds[(f + 2) * D - 1 - p];   // pfb_index(M, m0 + f, p, k) - pfb_index(M, m0, M - 1, k)
            qpsk::pfb_step(acc[i], hk[p], x.x, x.y);
        }
        __syncthreads();
    }

    // 2. the transforms: frame f at lds[f * P ..]
    const int P = F > 1 ? M + 1 : M;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const int e = tid + kThreads * i;
        const int f = e >> bits, p = e & (M - 1);
        lds[f * P + (__brev(static_cast<unsigned>(p)) >> (32 - bits))] = make_float2(acc[i].re, acc[i].im);
    }
    __syncthreads();
    for (int hb = 0; hb < bits; ++hb) {
        const int half = 1 << hb;
#pragma unroll
        for (int i = 0; i < kPer / 2; ++i) {
            const int u = tid + kThreads * i;                  // butterfly u of the tile's F * D
            const int f = u >> (bits - 1), within = u & (D - 1);
            const int j = within & (half - 1);
            const int at = f * P + ((within - j) << 1) + j;    // j0 + j, j0 = (within / half) * 2 half
            const float2 w = a.tw[j << (bits - 1 - hb)];       // W[j * (M / (2 half))]
            const float2 lo2 = lds[at], hi2 = lds[at + half];
            PfbC lo{lo2.x, lo2.y}, hi{hi2.x, hi2.y};
            qpsk::pfb_butterfly(lo, hi, w.x, w.y);
            lds[at] = make_float2(lo.re, lo.im);
            lds[at + half] = make_float2(hi.re, hi.im);
        }
        __syncthreads();
    }

    // 3. the outputs, a row's frames side by side
    const int fbits = 12 - bits;   // F = 2^fbits
    static_assert(kPfbTileElems == 1 << 12, "F * M");
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const int e = tid + kThreads * i;
        const int f = e & (F - 1), c = e >> fbits;
        if (f >= cnt) continue;
        const float2 v = lds[f * P + c];
        const PfbC y = qpsk::pfb_output(PfbC{v.x, v.y}, c, m0 + f, a.gain);
        float *o = a.out + (static_cast<int64_t>(b) * M + c) * a.out_stride + 2 * (o0 + f);
        if (a.out_pair) *reinterpret_cast<float2 *>(o) = make_float2(y.re, y.im);
        else o[0] = y.re, o[1] = y.im;
    }
}

__global__ __launch_bounds__(kThreads) void pfb_state_kernel(PfbArgs a) {
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int M = a.M, L = M * a.K;
    uint8_t *rec = a.state + static_cast<int64_t>(b) * a.each;
    PfbHead *hd = reinterpret_cast<PfbHead *>(rec);
    float(*hist)[2] = reinterpret_cast<float(*)[2]>(rec + sizeof(PfbHead));
    const int64_t in_pos = hd->in_pos, out_pos = hd->out_pos;
    const int64_t len = row_length(a, b);
    const int64_t cnt = qpsk::pfb_count(M, out_pos, in_pos + len);
    const char *irow = static_cast<const char *>(a.in) + static_cast<int64_t>(b) * a.in_stride * qpsk::fmt_elem_bytes(a.fmt_in);
    if (len > 0) {
        // the new hist[h] is index len - L + h of the call's row, or the old hist[h + len]
        for (int base = 0; base < L; base += kThreads) {
            const int h = base + tid;
            const int64_t j = len - L + h;
            float2 v = make_float2(0.0f, 0.0f);
            if (h < L) v = j >= 0 ? load_sample(irow, a.fmt_in, a.in_pair, j, a.scale_in) : make_float2(hist[h + len][0], hist[h + len][1]);
            __syncthreads();   // the chunk's reads of the old history are done
            if (h < L) hist[h][0] = v.x, hist[h][1] = v.y;
        }
    }
    __syncthreads();   // every lane has read the old positions
    if (tid == 0) {
        hd->in_pos = in_pos + len;
        hd->out_pos = out_pos + cnt;
    }
}

// what a failed grow of a staging buffer names (alloc_status)
constexpr const char *kStaging = "pfb staging";

}  // namespace

extern "C" {

int qpsk_pfb_create(const qpsk_pfb_params *p, int32_t n_bands, qpsk_pfb **out) {
    if (!out) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    *out = nullptr;
    int rc;
    if ((rc = qpsk::pfb_check_params(p, n_bands))) return rc;
    DeviceGuard guard;
    auto *pf = new qpsk_pfb();
    pf->p = *p;
    pf->B = n_bands;
    pf->M = p->channels;
    pf->K = p->taps_per_branch;
    pf->L = pf->M * pf->K;
    pf->each = qpsk::pfb_state_bytes(pf->M, pf->K);
    pf->host.assign(n_bands, PfbHead{});
    std::vector<float> h(pf->L), w(pf->M);
    qpsk::pfb_design(pf->M, pf->K, h.data());
    qpsk::pfb_twiddles(pf->M, w.data());
    const size_t state_bytes = static_cast<size_t>(n_bands) * pf->each;
    if (pf->open(p->device, n_bands) != hipSuccess || pf->d_state.alloc(state_bytes) != hipSuccess ||
        pf->d_taps.alloc(pf->L) != hipSuccess || pf->d_tw.alloc(pf->M / 2) != hipSuccess ||
        hipMemset(pf->d_state, 0, state_bytes) != hipSuccess ||
        hipMemcpy(pf->d_taps, h.data(), sizeof(float) * pf->L, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(pf->d_tw, w.data(), sizeof(float) * pf->M, hipMemcpyHostToDevice) != hipSuccess) {
        delete pf;
        return fail(QPSK_ERR_DEVICE, "pfb device set-up failed (no GPU?)");
    }
    *out = pf;
    return QPSK_OK;
}

int qpsk_pfb_destroy(qpsk_pfb *pf) { return qpsk::row_handle_destroy(pf); }

int qpsk_pfb_set_stream(qpsk_pfb *pf, void *hip_stream) {
    if (!pf) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    return pf->set_stream(hip_stream);
}

int qpsk_pfb_set_taps(qpsk_pfb *pf, const float *taps, int64_t n_taps) {
    if (!pf) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    int rc;
    if ((rc = qpsk::pfb_check_taps(taps, n_taps, pf->L))) return rc;
    DeviceGuard guard;
    QPSK_HIP_TRY(hipSetDevice(pf->device));
    QPSK_HIP_TRY(hipMemcpyAsync(pf->d_taps, taps, sizeof(float) * pf->L, hipMemcpyHostToDevice, pf->stream));
    QPSK_HIP_TRY(hipStreamSynchronize(pf->stream));
    return QPSK_OK;
}

int qpsk_pfb_apply_fmt(qpsk_pfb *pf, int32_t fmt_in, const void *in, int64_t stride_in, float scale_in, float *out,
                       int64_t stride_out, int64_t out_cap, int64_t n_samples, const int64_t *lengths, int64_t *n_out,
                       int32_t mem) {
    if (!pf) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    int rc;
    // the output is CF32 rows at the handle's gain: nothing of it for a caller to get wrong
    if ((rc = qpsk::check_row_formats("channeliser", fmt_in, scale_in, QPSK_FMT_CF32, QPSK_MOD_NORM_FIXED, 1.0f, mem)))
        return rc;
    if (!n_out) return fail(QPSK_ERR_ARGUMENT_NULL, "n_out is null");
    const int B = pf->B, M = pf->M;
    const int64_t rows_out = static_cast<int64_t>(B) * M;
    const bool host = mem == QPSK_MEM_HOST;
    const int64_t ieb = qpsk::fmt_elem_bytes(fmt_in), oeb = sizeof(float);
    int64_t n_call, n_out_max;
    std::vector<int64_t> cnt(B);
    if ((rc = qpsk::pfb_check_call(pf->p, pf->host.data(), B, stride_in, stride_out, out_cap, n_samples, lengths, cnt.data(),
                                   &n_call, &n_out_max)))
        return rc;
    if (n_call > 0) {
        if (!in || (n_out_max > 0 && !out)) return fail(QPSK_ERR_ARGUMENT_NULL, "in or out is null");
        if (!host && ((rc = check_device_rows("input", fmt_in, in, stride_in)) ||
                      (out && (rc = check_device_rows("output", QPSK_FMT_CF32, out, stride_out)))))
            return rc;
        if (out && qpsk::rows_overlap(in, B, stride_in, n_samples, ieb, out, rows_out, stride_out, out_cap, oeb))
            return fail(QPSK_ERR_ARGUMENT, "out must not overlap in");
    }
    std::memcpy(n_out, cnt.data(), sizeof(int64_t) * B);
    if (n_call == 0) return QPSK_OK;   // nothing taken: nothing emitted, no state moves

    DeviceGuard guard;
    QPSK_HIP_TRY(hipSetDevice(pf->device));
    hipStream_t st = pf->stream;
    PfbArgs a{};
    a.in = in;
    a.out = out;
    a.in_stride = stride_in;
    a.out_stride = stride_out;
    a.scale_in = scale_in;
    a.gain = pf->p.gain;
    a.fmt_in = fmt_in;
    a.n = n_samples;
    a.state = pf->d_state;
    a.each = pf->each;
    a.taps = pf->d_taps;
    a.tw = pf->d_tw;
    a.B = B;
    a.M = M;
    a.K = pf->K;
    a.bits = qpsk::pfb_log2(M);
    if ((rc = pf->upload_lengths(lengths, B, &a.lengths))) return rc;
    if (host && ((rc = pf->stage_out(kStaging, oeb, std::max<int64_t>(n_out_max, 1), rows_out, &a.out, &a.out_stride)) ||
                 (rc = pf->stage_in(kStaging, in, stride_in, ieb, n_call, B, &a.in, &a.in_stride))))
        return rc;
    a.in_pair = pair_rows(fmt_in, a.in, a.in_stride);
    a.out_pair = pair_rows(QPSK_FMT_CF32, a.out, a.out_stride);
    a.in_wide = qpsk::wide_rows(fmt_in, a.in, a.in_stride);
    if (n_out_max > 0) {
        const int F = qpsk::pfb_tile_frames(M);
        const dim3 grid(static_cast<unsigned>((n_out_max + F - 1) / F), B);
        hipLaunchKernelGGL(pfb_kernel, grid, dim3(kThreads), 0, st, a);
        QPSK_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(pfb_state_kernel, dim3(B), dim3(kThreads), 0, st, a);
    QPSK_HIP_TRY(hipGetLastError());
    qpsk::advance_rows(pf->host.data(), B, n_samples, lengths, cnt.data());
    if (host && n_out_max > 0) {
        // row by row what each band emitted: what lies past a row's count stays as it was
        for (int b = 0; b < B; ++b)
            if (cnt[b] > 0)
                QPSK_HIP_TRY(hipMemcpy2DAsync(out + static_cast<int64_t>(b) * M * stride_out, stride_out * oeb,
                                              a.out + static_cast<int64_t>(b) * M * a.out_stride, a.out_stride * oeb,
                                              2 * cnt[b] * oeb, M, hipMemcpyDeviceToHost, st));
    }
    if (host || lengths) QPSK_HIP_TRY(hipStreamSynchronize(st));
    return QPSK_OK;
}

int qpsk_pfb_get_state(qpsk_pfb *pf, void *host_buf, int64_t buf_bytes) {
    if (!pf || !host_buf) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    int rc;
    if ((rc = qpsk::check_state_bytes("pfb", buf_bytes, pf->B * pf->each))) return rc;
    return pf->state_out(host_buf, pf->d_state, buf_bytes);
}

int qpsk_pfb_set_state(qpsk_pfb *pf, const void *host_buf, int64_t buf_bytes) {
    if (!pf) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    int rc;
    if ((rc = qpsk_pfb_state_check(&pf->p, pf->B, host_buf, buf_bytes)) || (rc = pf->state_in(pf->d_state, host_buf, buf_bytes)))
        return rc;
    for (int b = 0; b < pf->B; ++b)
        std::memcpy(&pf->host[b], static_cast<const char *>(host_buf) + b * pf->each, sizeof(PfbHead));
    return QPSK_OK;
}

int qpsk_pfb_reset_bands(qpsk_pfb *pf, const int32_t *bands, int32_t n) {
    if (!pf) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    int rc;
    if ((rc = qpsk_stream_list_check(pf->B, bands, n))) return rc;
    DeviceGuard guard;
    QPSK_HIP_TRY(hipSetDevice(pf->device));
    for (int32_t k = 0; k < n; ++k)
        QPSK_HIP_TRY(hipMemsetAsync(pf->d_state.get() + bands[k] * pf->each, 0, pf->each, pf->stream));
    QPSK_HIP_TRY(hipStreamSynchronize(pf->stream));
    for (int32_t k = 0; k < n; ++k) pf->host[bands[k]] = PfbHead{};
    return QPSK_OK;
}

}  // extern "C"
