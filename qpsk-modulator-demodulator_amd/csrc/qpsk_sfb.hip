// qpsk_sfb.hip -- the polyphase synthesis bank (include/qpsk_demod.h, "The
// polyphase synthesis bank on the device") on n_bands bands of M rows: the
// three kernels and the entry points that need a device.  The per-element
// functions, the state record, the checks and the host form of the call are
// qpsk_sfb.h / qpsk_sfb.cpp; the butterfly, the prototype and the twiddles are
// the channeliser's (qpsk_pfb.h).
//
// An output sample reads the transforms of 2K frames, so a fused kernel would
// transform 2K - 1 frames more than its tile emits.  The transforms go through
// a scratch row the handle owns instead, u[B][rows][M], and a call runs in
// slabs of sfb_slab_frames frames so that u (32 MiB at the most, all bands
// together) stays in the last-level cache between the kernel that writes it and
// the one that reads it.  Row e of a slab that starts at the call's frame t0 is
// the transform of frame t0 - (2K - 1) + e: a slab transforms its own frames and
// the 2K - 1 in front of them again, from the call's rows or, before the call's
// first frame, from the state's history.
//
// sfb_transform_kernel: one workgroup of 256 threads takes F = 4096 / M rows of
//   one band's slab, 16 elements a thread whatever M is.
//   stage   element e = tid + 256 i is frame e mod F of row e / F, so that an
//           input row gives F consecutive samples; widened, signed (sfb_input)
//           and put at its bit-reversed place in LDS, frame f at f * (M + 1).
//   fft     log2 M stages of 2048 butterflies, 8 a thread, a barrier a stage:
//           the channeliser's stage loop on pfb_butterfly.
//   store   element e is q = e mod M of frame e / M: u is written frame-major,
//           consecutive lanes consecutive addresses.
// sfb_sum_kernel<K>: no LDS.  A lane owns one r in [0, D) and the frames of one
//   parity of a run of kSfbSumRun frames: term j of frame f reads u_{f-j} at r
//   (j even) or r + D (j odd), so the frames of one parity read only u[.][r] of
//   that parity's rows and u[.][r + D] of the other's.  The lane keeps those 2K
//   values and its 2K taps in registers as two rings of K whose slots rotate at
//   compile time (the loop is unrolled K steps): two coalesced loads and one
//   coalesced store a frame.  K = 8 and K = 16 are specialised; K = 0 names the
//   generic form, which rereads the 2K values of every frame (they stay in L2
//   within a run).  Both add the terms in the definition's order.
// sfb_state_kernel runs behind the last slab, when nobody reads the old
//   history any more: one workgroup a band moves the new history in, from the
//   call's last 2K - 1 frames, or, when the call was shorter than that, the old
//   history down by the call's frames in chunks of 256 elements in ascending
//   order (a chunk's reads lie at or above its own writes and above every
//   earlier chunk's), then the call's frames; lane 0 advances the positions
//   behind a barrier.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "qpsk_demod.h"
#include "qpsk_device.h"
#include "qpsk_internal.h"
#include "qpsk_quantise.h"
#include "qpsk_row_call.h"
#include "qpsk_row_handle.h"
#include "qpsk_sample_rows.h"
#include "qpsk_sfb.h"

struct qpsk_sfb : qpsk::RowHandle {
    qpsk_sfb_params p{};
    int B = 0, M = 0, K = 0, L = 0;
    int64_t each = 0;                        // bytes of one band's state
    qpsk::DevBuf<uint8_t> d_state;           // [B][64 + 8 M (2K - 1)]
    qpsk::DevBuf<float> d_taps;              // [L]
    qpsk::DevBuf<float2> d_tw;               // [M / 2]
    qpsk::DevBuf<float2> d_u;                // [B][u_rows][M]: the transforms of one slab
    std::vector<qpsk::SfbHead> host;         // [B]: the positions as the device will hold them behind the calls
                                             // queued so far
};

namespace {

using qpsk::check_device_rows;
using qpsk::DeviceGuard;
using qpsk::fail;
using qpsk::kPfbTileElems;
using qpsk::kSfbSumRun;
using qpsk::load_sample;
using qpsk::pair_rows;
using qpsk::PfbC;
using qpsk::row_length;
using qpsk::SfbHead;

constexpr int kThreads = 256;
constexpr int kPer = kPfbTileElems / kThreads;                         // elements a thread
constexpr int kLds = kPfbTileElems + kPfbTileElems / QPSK_PFB_MIN_CHANNELS;   // F (M + 1) at M = 8
static_assert(kPer * kThreads == kPfbTileElems && kPer % 2 == 0, "a thread's elements and butterflies");
static_assert(kSfbSumRun % 2 == 0, "a run holds as many frames of either parity");

struct SfbArgs {
    const void *in;
    void *out;
    int64_t in_stride, out_stride;   // elements
    float scale_in, scale_out;
    int fmt_in, fmt_out;
    int in_pair, out_pair;           // CF32 rows 8-byte aligned: one access a sample
    const int64_t *lengths;          // device, checked; nullptr: n for every band
    int64_t n;
    uint8_t *state;
    int64_t each;                    // bytes of one band's state
    const float *taps;
    const float2 *tw;
    float2 *u;
    int64_t u_rows;                  // rows of u a band has
    int64_t t0;                      // the slab's first frame in the call
    int nt;                          // and its frames
    int B, M, K, bits;
};

// the frames of the slab band b takes part in with: its length cuts the slab
__device__ __forceinline__ int slab_frames(const SfbArgs &a, int b) {
    const int64_t left = row_length(a, b) - a.t0;
    return left < a.nt ? static_cast<int>(left > 0 ? left : 0) : a.nt;
}

__global__ __launch_bounds__(kThreads) void sfb_transform_kernel(SfbArgs a) {
    __shared__ float2 lds[kLds];
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const int M = a.M, D = M >> 1, bits = a.bits, H = qpsk::sfb_hist_frames(a.K);
    const int fbits = 12 - bits, F = 1 << fbits;
    static_assert(kPfbTileElems == 1 << 12, "F * M");
    const int need = slab_frames(a, b);
    if (need == 0) return;
    const int rows = need + H;
    const int e0 = blockIdx.x * F;
    if (e0 >= rows) return;
    const uint8_t *rec = a.state + static_cast<int64_t>(b) * a.each;
    const int64_t in_pos = reinterpret_cast<const SfbHead *>(rec)->in_pos;
    const float2 *hist = reinterpret_cast<const float2 *>(rec + sizeof(SfbHead));
    const int64_t eb = qpsk::fmt_elem_bytes(a.fmt_in);
    const char *irow = static_cast<const char *>(a.in) + static_cast<int64_t>(b) * M * a.in_stride * eb;
    const int P = F > 1 ? M + 1 : M;

    // 1. the frames' inputs, signed, at their bit-reversed places
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const int e = tid + kThreads * i;
        const int f = e & (F - 1), c = e >> fbits;
        float2 v = make_float2(0.0f, 0.0f);
        if (e0 + f < rows) {
            const int64_t t = a.t0 - H + e0 + f;   // the call's frame: below t0 + need, so inside the row
            if (t >= 0) v = load_sample(irow + c * a.in_stride * eb, a.fmt_in, a.in_pair, t, a.scale_in);
            else v = hist[(H + t) * M + c];
            const PfbC s = qpsk::sfb_input(PfbC{v.x, v.y}, c, in_pos + t);
            v = make_float2(s.re, s.im);
        }
        lds[f * P + (__brev(static_cast<unsigned>(c)) >> (32 - bits))] = v;
    }
    __syncthreads();

    // 2. the transforms: frame f at lds[f * P ..].  pfb_kernel's stage loop, written out a second time: called from
    // one shared function, pfb_kernel keeps its instructions and registers but not their order, and it is to stay
    // as it is
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

    // 3. u, frame-major
    float2 *u = a.u + (static_cast<int64_t>(b) * a.u_rows + e0) * M;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const int e = tid + kThreads * i;
        const int f = e >> bits, q = e & (M - 1);
        if (e0 + f < rows) u[e] = lds[f * P + q];   // e = f * M + q
    }
}

// K > 0: the register rings; K = 0: the generic form, any a.K
template <int K>
__global__ __launch_bounds__(kThreads) void sfb_sum_kernel(SfbArgs a) {
    const int b = blockIdx.y;
    const int M = a.M, D = M >> 1, bits = a.bits;
    const int need = slab_frames(a, b);
    const int64_t lane = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const int r = static_cast<int>(lane & (D - 1)), par = static_cast<int>(lane >> (bits - 1)) & 1;
    const int64_t run = lane >> bits;
    const int64_t f0 = run * kSfbSumRun + par;                 // the lane's first frame in the slab
    if (f0 >= need) return;
    const int f1 = (run + 1) * kSfbSumRun < need ? static_cast<int>((run + 1) * kSfbSumRun) : need;
    const int KK = K ? K : a.K, H = qpsk::sfb_hist_frames(KK);
    // row R of u is the slab's frame R - H; this lane reads columns r and r + D
    const float2 *ue = a.u + static_cast<int64_t>(b) * a.u_rows * M + r;
    const float2 *uo = ue + D;
    const float *g = a.taps + r;
    void *orow = static_cast<char *>(a.out) + static_cast<int64_t>(b) * a.out_stride * qpsk::fmt_elem_bytes(a.fmt_out);
    const int64_t i0 = a.t0 * D + r;                           // the output of the slab's frame 0
    if constexpr (K == 0) {
        for (int f = static_cast<int>(f0); f < f1; f += 2) {
            PfbC acc{0.0f, 0.0f};
            for (int j = 0; j < 2 * KK; ++j) {
                const float2 v = ((j & 1) ? uo : ue)[static_cast<int64_t>(f + H - j) * M];
                qpsk::sfb_step(acc, g[j * D], PfbC{v.x, v.y});
            }
            qpsk::store_sample(orow, a.fmt_out, a.out_pair, i0 + static_cast<int64_t>(f) * D, make_float2(acc.re, acc.im),
                               a.scale_out);
        }
    } else {
        // slot p of a ring holds, at step n, the value of logical place (p + n) mod K: place k is u_{f - 2k}[r] in ev
        // and u_{f - 2k - 1}[r + D] in od
        float2 ev[K], od[K];
        float ge[K], go[K];
#pragma unroll
        for (int k = 0; k < K; ++k) ge[k] = g[2 * k * D], go[k] = g[(2 * k + 1) * D];
        const int64_t R0 = f0 + H;
#pragma unroll
        for (int p = 1; p < K; ++p) {
            ev[p] = ue[(R0 - 2 * p) * M];
            od[p] = uo[(R0 - 1 - 2 * p) * M];
        }
        ev[0] = od[0] = make_float2(0.0f, 0.0f);
        for (int fb = static_cast<int>(f0); fb < f1; fb += 2 * K) {
#pragma unroll
            for (int s = 0; s < K; ++s) {
                const int f = fb + 2 * s;
                if (f < f1) {
                    const int64_t R = f + H;
                    ev[(K - s) % K] = ue[R * M];
                    od[(K - s) % K] = uo[(R - 1) * M];
                    PfbC acc{0.0f, 0.0f};
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const float2 x = ev[(k + K - s) % K], y = od[(k + K - s) % K];
                        qpsk::sfb_step(acc, ge[k], PfbC{x.x, x.y});
                        qpsk::sfb_step(acc, go[k], PfbC{y.x, y.y});
                    }
                    qpsk::store_sample(orow, a.fmt_out, a.out_pair, i0 + static_cast<int64_t>(f) * D,
                                       make_float2(acc.re, acc.im), a.scale_out);
                }
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void sfb_state_kernel(SfbArgs a) {
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int M = a.M, bits = a.bits, H = qpsk::sfb_hist_frames(a.K);
    uint8_t *rec = a.state + static_cast<int64_t>(b) * a.each;
    SfbHead *hd = reinterpret_cast<SfbHead *>(rec);
    float2 *hist = reinterpret_cast<float2 *>(rec + sizeof(SfbHead));
    const int64_t in_pos = hd->in_pos, out_pos = hd->out_pos;
    const int64_t len = row_length(a, b);
    const int64_t eb = qpsk::fmt_elem_bytes(a.fmt_in);
    const char *irow = static_cast<const char *>(a.in) + static_cast<int64_t>(b) * M * a.in_stride * eb;
    if (len > 0) {
        // the new hist[k][c] is frame len - H + k of the call's row c, or the old hist[k + len][c]
        const int n = H << bits;
        for (int base = 0; base < n; base += kThreads) {
            const int h = base + tid;
            const int c = h & (M - 1);
            const int64_t t = len - H + (h >> bits);
            float2 v = make_float2(0.0f, 0.0f);
            if (h < n) v = t >= 0 ? load_sample(irow + c * a.in_stride * eb, a.fmt_in, a.in_pair, t, a.scale_in) : hist[h + len * M];
            __syncthreads();   // the chunk's reads of the old history are done
            if (h < n) hist[h] = v;
        }
    }
    __syncthreads();   // every lane has read the old positions
    if (tid == 0) {
        hd->in_pos = in_pos + len;
        hd->out_pos = out_pos + qpsk::sfb_emitted(M, len);
    }
}

void launch_sum(int K, dim3 grid, hipStream_t st, const SfbArgs &a) {
    switch (K) {
    case 8: hipLaunchKernelGGL(sfb_sum_kernel<8>, grid, dim3(kThreads), 0, st, a); break;
    case 16: hipLaunchKernelGGL(sfb_sum_kernel<16>, grid, dim3(kThreads), 0, st, a); break;
    default: hipLaunchKernelGGL(sfb_sum_kernel<0>, grid, dim3(kThreads), 0, st, a); break;
    }
}

// what a failed grow of a buffer names (alloc_status)
constexpr const char *kStaging = "sfb staging";
constexpr const char *kScratch = "sfb transforms";

}  // namespace

extern "C" {

int qpsk_sfb_create(const qpsk_sfb_params *p, int32_t n_bands, qpsk_sfb **out) {
    if (!out) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    *out = nullptr;
    int rc;
    if ((rc = qpsk::sfb_check_params(p, n_bands))) return rc;
    DeviceGuard guard;
    auto *sf = new qpsk_sfb();
    sf->p = *p;
    sf->B = n_bands;
    sf->M = p->channels;
    sf->K = p->taps_per_branch;
    sf->L = sf->M * sf->K;
    sf->each = qpsk::sfb_state_bytes(sf->M, sf->K);
    sf->host.assign(n_bands, SfbHead{});
    std::vector<float> g(sf->L), w(sf->M);
    qpsk::pfb_design(sf->M, sf->K, g.data());
    qpsk::pfb_twiddles(sf->M, w.data());
    const size_t state_bytes = static_cast<size_t>(n_bands) * sf->each;
    if (sf->open(p->device, n_bands) != hipSuccess || sf->d_state.alloc(state_bytes) != hipSuccess ||
        sf->d_taps.alloc(sf->L) != hipSuccess || sf->d_tw.alloc(sf->M / 2) != hipSuccess ||
        hipMemset(sf->d_state, 0, state_bytes) != hipSuccess ||
        hipMemcpy(sf->d_taps, g.data(), sizeof(float) * sf->L, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(sf->d_tw, w.data(), sizeof(float) * sf->M, hipMemcpyHostToDevice) != hipSuccess) {
        delete sf;
        return fail(QPSK_ERR_DEVICE, "sfb device set-up failed (no GPU?)");
    }
    *out = sf;
    return QPSK_OK;
}

int qpsk_sfb_destroy(qpsk_sfb *sf) { return qpsk::row_handle_destroy(sf); }

int qpsk_sfb_set_stream(qpsk_sfb *sf, void *hip_stream) {
    if (!sf) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    return sf->set_stream(hip_stream);
}

int qpsk_sfb_set_taps(qpsk_sfb *sf, const float *taps, int64_t n_taps) {
    if (!sf) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    int rc;
    if ((rc = qpsk::pfb_check_taps(taps, n_taps, sf->L))) return rc;
    DeviceGuard guard;
    QPSK_HIP_TRY(hipSetDevice(sf->device));
    QPSK_HIP_TRY(hipMemcpyAsync(sf->d_taps, taps, sizeof(float) * sf->L, hipMemcpyHostToDevice, sf->stream));
    QPSK_HIP_TRY(hipStreamSynchronize(sf->stream));
    return QPSK_OK;
}

int qpsk_sfb_apply_fmt(qpsk_sfb *sf, int32_t fmt_in, const void *in, int64_t stride_in, float scale_in, int32_t fmt_out,
                       int32_t norm_out, void *out, int64_t stride_out, float scale_out, int64_t n_frames,
                       const int64_t *lengths, int32_t mem) {
    if (!sf) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    int rc;
    if ((rc = qpsk::check_row_formats("synthesis bank", fmt_in, scale_in, fmt_out, norm_out, scale_out, mem))) return rc;
    const int B = sf->B, M = sf->M, K = sf->K, D = M / 2, H = qpsk::sfb_hist_frames(K);
    const int64_t rows_in = static_cast<int64_t>(B) * M;
    const bool host = mem == QPSK_MEM_HOST;
    const int64_t ieb = qpsk::fmt_elem_bytes(fmt_in), oeb = qpsk::fmt_elem_bytes(fmt_out);
    int64_t n_call;
    if ((rc = qpsk::sfb_check_call(sf->p, sf->host.data(), B, stride_in, stride_out, n_frames, lengths, &n_call))) return rc;
    if (n_call == 0) return QPSK_OK;   // nothing taken: nothing emitted, no state moves
    if (!in || !out) return fail(QPSK_ERR_ARGUMENT_NULL, "in or out is null");
    if (!host && ((rc = check_device_rows("input", fmt_in, in, stride_in)) ||
                  (rc = check_device_rows("output", fmt_out, out, stride_out))))
        return rc;
    if (qpsk::rows_overlap(in, rows_in, stride_in, n_frames, ieb, out, B, stride_out, n_frames * D, oeb))
        return fail(QPSK_ERR_ARGUMENT, "out must not overlap in");

    DeviceGuard guard;
    QPSK_HIP_TRY(hipSetDevice(sf->device));
    hipStream_t st = sf->stream;
    SfbArgs a{};
    a.in = in;
    a.out = out;
    a.in_stride = stride_in;
    a.out_stride = stride_out;
    a.scale_in = scale_in;
    a.scale_out = scale_out;
    a.fmt_in = fmt_in;
    a.fmt_out = fmt_out;
    a.n = n_frames;
    a.state = sf->d_state;
    a.each = sf->each;
    a.taps = sf->d_taps;
    a.tw = sf->d_tw;
    a.B = B;
    a.M = M;
    a.K = K;
    a.bits = qpsk::pfb_log2(M);
    const int64_t slab = std::min(qpsk::sfb_slab_frames(M, B), n_call);
    a.u_rows = slab + H;
    // every allocation in front of the first copy: none is queued while one can still refuse the call (a buffer
    // that grows is freed first, and hipFree waits for the calls queued on it)
    if ((rc = qpsk::alloc_status(sf->d_u.grow(sizeof(float2) * static_cast<size_t>(B) * a.u_rows * M), kScratch))) return rc;
    a.u = sf->d_u;
    if (host && ((rc = sf->stage_out(kStaging, oeb, n_call * D, B, &a.out, &a.out_stride)) ||
                 (rc = sf->stage_in(kStaging, in, stride_in, ieb, n_call, rows_in, &a.in, &a.in_stride))))
        return rc;
    if ((rc = sf->upload_lengths(lengths, B, &a.lengths))) return rc;
    a.in_pair = pair_rows(fmt_in, a.in, a.in_stride);
    a.out_pair = pair_rows(fmt_out, a.out, a.out_stride);
    const int F = qpsk::pfb_tile_frames(M);
    for (int64_t t0 = 0; t0 < n_call; t0 += slab) {
        a.t0 = t0;
        a.nt = static_cast<int>(std::min(slab, n_call - t0));
        hipLaunchKernelGGL(sfb_transform_kernel, dim3(static_cast<unsigned>((a.nt + H + F - 1) / F), B), dim3(kThreads), 0, st,
                           a);
        QPSK_HIP_TRY(hipGetLastError());
        const int64_t lanes = ((a.nt + kSfbSumRun - 1) / kSfbSumRun) * static_cast<int64_t>(M);
        launch_sum(K, dim3(static_cast<unsigned>((lanes + kThreads - 1) / kThreads), B), st, a);
        QPSK_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(sfb_state_kernel, dim3(B), dim3(kThreads), 0, st, a);
    QPSK_HIP_TRY(hipGetLastError());
    for (int b = 0; b < B; ++b) {
        const int64_t len = lengths ? lengths[b] : n_frames;
        sf->host[b].in_pos += len;
        sf->host[b].out_pos += qpsk::sfb_emitted(M, len);
    }
    if (host) {
        // row by row what each band emitted: what lies past a row's samples stays as it was
        char *o = static_cast<char *>(out);
        const char *d = static_cast<const char *>(a.out);
        for (int b = 0; b < B; ++b) {
            const int64_t len = lengths ? lengths[b] : n_frames;
            if (len > 0)
                QPSK_HIP_TRY(hipMemcpyAsync(o + b * stride_out * oeb, d + b * a.out_stride * oeb, 2 * len * D * oeb,
                                            hipMemcpyDeviceToHost, st));
        }
    }
    if (host || lengths) QPSK_HIP_TRY(hipStreamSynchronize(st));
    return QPSK_OK;
}

int qpsk_sfb_get_state(qpsk_sfb *sf, void *host_buf, int64_t buf_bytes) {
    if (!sf || !host_buf) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    int rc;
    if ((rc = qpsk::check_state_bytes("sfb", buf_bytes, sf->B * sf->each))) return rc;
    return sf->state_out(host_buf, sf->d_state, buf_bytes);
}

int qpsk_sfb_set_state(qpsk_sfb *sf, const void *host_buf, int64_t buf_bytes) {
    if (!sf) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    int rc;
    if ((rc = qpsk_sfb_state_check(&sf->p, sf->B, host_buf, buf_bytes)) || (rc = sf->state_in(sf->d_state, host_buf, buf_bytes)))
        return rc;
    for (int b = 0; b < sf->B; ++b)
        std::memcpy(&sf->host[b], static_cast<const char *>(host_buf) + b * sf->each, sizeof(SfbHead));
    return QPSK_OK;
}

int qpsk_sfb_reset_bands(qpsk_sfb *sf, const int32_t *bands, int32_t n) {
    if (!sf) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    int rc;
    if ((rc = qpsk_stream_list_check(sf->B, bands, n))) return rc;
    DeviceGuard guard;
    QPSK_HIP_TRY(hipSetDevice(sf->device));
    for (int32_t k = 0; k < n; ++k)
        QPSK_HIP_TRY(hipMemsetAsync(sf->d_state.get() + bands[k] * sf->each, 0, sf->each, sf->stream));
    QPSK_HIP_TRY(hipStreamSynchronize(sf->stream));
    for (int32_t k = 0; k < n; ++k) sf->host[bands[k]] = SfbHead{};
    return QPSK_OK;
}

}  // extern "C"
