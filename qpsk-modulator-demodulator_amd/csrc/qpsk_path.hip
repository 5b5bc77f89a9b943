// qpsk_path.hip -- the propagation path (include/qpsk_demod.h, "The propagation
// path on the device") on S streams: the two kernels and the entry points that
// need a device.  The per-sample functions, the state record, the checks and
// the host form of the call are qpsk_path.h / qpsk_path.cpp.
//
// path_kernel: every output is independent, so one workgroup of 256 threads
// takes one stream's run of QPSK_PATH_TILE_OUTPUTS = 1024 outputs, k0 .. k0 +
// cnt - 1.  Their positions do not decrease, so the inputs they read are one
// window: z[floor(p_k0) - 1 .. floor(p_last) + 2], and L - 1 samples of x in
// front of it, at most 1023 * 1.001 + 1 + 4 + 7 = 1037 samples.
//
//   stage   the window of x, widened, into LDS: coalesced, 16 bytes a lane where
//           the rows are 16-byte aligned and pitched, else a sample a lane.
//           Indices before the call's first sample come from the state's
//           history, and are +0 there before the stream's start.
//   taps    after a barrier, z over the window into a second LDS array.
//   interp  after one more barrier, a lane takes every 256th output: position
//           and mu in double, the four weights, four z from LDS, the quantiser,
//           one coalesced store.
//
// A workgroup finds its stream's output count itself (path_count of the state
// and the call's length, as the host did), so no count is uploaded and a call
// without lengths is queued whole.
//
// path_state_kernel runs behind path_kernel, when nobody reads the old history
// any more: 16 lanes a stream read the new history's samples (from the call's
// last samples, or from the old history when the call was shorter than 16), and
// write them behind a barrier; lane 0 advances the positions.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "qpsk_demod.h"
#include "qpsk_device.h"
#include "qpsk_internal.h"
#include "qpsk_path.h"
#include "qpsk_quantise.h"
#include "qpsk_row_call.h"
#include "qpsk_row_handle.h"
#include "qpsk_sample_rows.h"

struct qpsk_path : qpsk::RowHandle {
    qpsk_path_params p{};
    int S = 0;
    qpsk::DevBuf<qpsk::PathState> d_state;   // [S]
    std::vector<qpsk::PathState> host;       // [S]: clock, positions and taps as the device will hold them
                                             // behind the calls queued so far (the history is not kept here)
};

namespace {

using qpsk::check_device_rows;
using qpsk::DeviceGuard;
using qpsk::fail;
using qpsk::kPathHist;
using qpsk::load_sample;
using qpsk::pair_rows;
using qpsk::PathC;
using qpsk::PathState;
using qpsk::row_length;
using qpsk::store_sample;

constexpr int kTile = QPSK_PATH_TILE_OUTPUTS;
constexpr int kThreads = 256;
constexpr int kWin = 1040;                   // >= (kTile - 1) * 1.001 + 1 + 4 + (8 - 1), rounded up
constexpr int kGridY = 65535;
static_assert((kTile - 1) * 1001 / 1000 + 2 + 4 + QPSK_PATH_MAX_TAPS - 1 <= kWin, "a tile's window fits");
static_assert(kThreads % kPathHist == 0, "a stream's history lanes share a workgroup");

struct PathArgs {
    const void *in;
    void *out;
    int64_t in_stride, out_stride;   // elements
    float scale_in, scale_out;
    int fmt_in, fmt_out;
    int in_pair, out_pair;           // CF32 rows 8-byte aligned: one access a sample
    int in_wide;                     // input rows 16-byte aligned and pitched
    const int64_t *lengths;          // device, checked; nullptr: n for every stream
    int64_t n;
    PathState *state;
    int S;
};

__global__ __launch_bounds__(kThreads) void path_kernel(PathArgs a) {
    __shared__ float2 xs[kWin];
    __shared__ float2 zs[kWin];
    const int tid = threadIdx.x;
    const int s = blockIdx.z * kGridY + blockIdx.y;
    if (s >= a.S) return;
    const PathState &st = a.state[s];
    const double r = st.r, tau = st.tau;
    const int64_t in_pos = st.in_pos, out_pos = st.out_pos;
    const int L = st.n_taps;
    const int64_t len = row_length(a, s);
    const int64_t total = qpsk::path_count(r, tau, out_pos, in_pos + len);
    const int64_t o0 = static_cast<int64_t>(blockIdx.x) * kTile;
    if (o0 >= total) return;
    const int cnt = total - o0 < kTile ? static_cast<int>(total - o0) : kTile;
    const int64_t k0 = out_pos + o0;
    int64_t n_first, n_last;
    float t_unused;
    qpsk::path_pos(r, tau, k0, &n_first, &t_unused);
    qpsk::path_pos(r, tau, k0 + cnt - 1, &n_last, &t_unused);
    const int64_t zlen64 = n_last - n_first + 4;
    // a state that qpsk_path_state_check accepted cannot fail this
    if (L < 1 || L > QPSK_PATH_MAX_TAPS || zlen64 < 4 || zlen64 + L - 1 > kWin) return;
    const int zlen = static_cast<int>(zlen64), xlen = zlen + L - 1;
    const int64_t j0 = n_first - 1 - (L - 1) - in_pos;   // xs[0] as an index into the call's row

    const int64_t in_eb = qpsk::fmt_elem_bytes(a.fmt_in), out_eb = qpsk::fmt_elem_bytes(a.fmt_out);
    const char *irow = static_cast<const char *>(a.in) + static_cast<int64_t>(s) * a.in_stride * in_eb;
    qpsk::stage_window<kThreads>(xs, j0, xlen, len, irow, st.hist, kPathHist, a, tid);
    __syncthreads();

    // zs[q] is z at n_first - 1 + q, whose newest input is xs[q + L - 1]
    for (int q = tid; q < zlen; q += kThreads) {
        PathC acc{0.0f, 0.0f};
        for (int j = 0; j < L; ++j) {
            const float2 x = xs[q + (L - 1) - j];
            qpsk::path_tap(acc, st.taps[j][0], st.taps[j][1], x.x, x.y);
        }
        zs[q] = make_float2(acc.re, acc.im);
    }
    __syncthreads();

    char *orow = static_cast<char *>(a.out) + static_cast<int64_t>(s) * a.out_stride * out_eb;
    const int64_t z0 = n_first - 1;
    for (int o = tid; o < cnt; o += kThreads) {
        const PathC y = qpsk::path_output(r, tau, k0 + o, [&](int64_t i) {
            // p does not decrease in k: i - z0 lies in [0, zlen); held there all the same
            int64_t q = i - z0;
            q = q < 0 ? 0 : (q >= zlen ? zlen - 1 : q);
            const float2 v = zs[q];
            return PathC{v.x, v.y};
        });
        store_sample(orow, a.fmt_out, a.out_pair, o0 + o, make_float2(y.re, y.im), a.scale_out);
    }
}

__global__ __launch_bounds__(kThreads) void path_state_kernel(PathArgs a) {
    const int64_t g = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const int s = static_cast<int>(g / kPathHist), h = static_cast<int>(g % kPathHist);
    const bool live = s < a.S;
    float2 v = make_float2(0.0f, 0.0f);
    int64_t len = 0, cnt = 0;
    if (live) {
        const PathState &st = a.state[s];
        len = row_length(a, s);
        cnt = qpsk::path_count(st.r, st.tau, st.out_pos, st.in_pos + len);
        const int64_t j = len - kPathHist + h;   // the new hist[h] as an index into the call's row
        if (j >= 0) {
            const char *irow = static_cast<const char *>(a.in) +
                               static_cast<int64_t>(s) * a.in_stride * qpsk::fmt_elem_bytes(a.fmt_in);
            v = load_sample(irow, a.fmt_in, a.in_pair, j, a.scale_in);
        } else {
            v = make_float2(st.hist[len + h][0], st.hist[len + h][1]);   // 0 <= len + h < 16
        }
    }
    __syncthreads();   // every lane has read the old history and the old positions
    if (live) {
        PathState &st = a.state[s];
        st.hist[h][0] = v.x;
        st.hist[h][1] = v.y;
        if (h == 0) {
            st.in_pos += len;
            st.out_pos += cnt;
        }
    }
}

// what a failed grow of a staging buffer names (alloc_status)
constexpr const char *kStaging = "path staging";

}  // namespace

extern "C" {

int qpsk_path_create(const qpsk_path_params *p, int32_t n_streams, qpsk_path **out) {
    if (!out) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    *out = nullptr;
    int rc;
    if ((rc = qpsk::path_check_params(p, n_streams))) return rc;
    DeviceGuard guard;
    auto *pa = new qpsk_path();
    pa->p = *p;
    pa->S = n_streams;
    pa->host.resize(n_streams);
    for (int32_t s = 0; s < n_streams; ++s) pa->host[s] = qpsk::path_state_new(*p, s);
    if (pa->open(p->device, n_streams) != hipSuccess || pa->d_state.alloc(n_streams) != hipSuccess ||
        hipMemcpy(pa->d_state, pa->host.data(), pa->host.size() * sizeof(PathState), hipMemcpyHostToDevice) !=
            hipSuccess) {
        delete pa;
        return fail(QPSK_ERR_DEVICE, "path device set-up failed (no GPU?)");
    }
    *out = pa;
    return QPSK_OK;
}

int qpsk_path_destroy(qpsk_path *pa) { return qpsk::row_handle_destroy(pa); }

int qpsk_path_set_stream(qpsk_path *pa, void *hip_stream) {
    if (!pa) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    return pa->set_stream(hip_stream);
}

int qpsk_path_set_taps(qpsk_path *pa, const float *taps_iq, int32_t n_taps, int32_t per_stream) {
    if (!pa) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    int rc;
    if ((rc = qpsk::path_check_taps(taps_iq, n_taps))) return rc;
    if (per_stream)
        for (int s = 1; s < pa->S; ++s)
            if ((rc = qpsk::path_check_taps(taps_iq + static_cast<int64_t>(s) * 2 * n_taps, n_taps))) return rc;
    // n_taps and taps lie side by side in a record: one strided copy of that part
    constexpr size_t kPart = sizeof(int32_t) + sizeof(PathState::taps);
    static_assert(offsetof(PathState, taps) == offsetof(PathState, n_taps) + sizeof(int32_t), "one part");
    std::vector<PathState> next = pa->host;
    std::vector<uint8_t> part(static_cast<size_t>(pa->S) * kPart);
    for (int s = 0; s < pa->S; ++s) {
        qpsk::path_put_taps(next[s], taps_iq + (per_stream ? static_cast<int64_t>(s) * 2 * n_taps : 0), n_taps);
        std::memcpy(&part[s * kPart], &next[s].n_taps, kPart);
    }
    DeviceGuard guard;
    QPSK_HIP_TRY(hipSetDevice(pa->device));
    QPSK_HIP_TRY(hipMemcpy2DAsync(reinterpret_cast<char *>(pa->d_state.get()) + offsetof(PathState, n_taps),
                                  sizeof(PathState), part.data(), kPart, kPart, pa->S, hipMemcpyHostToDevice,
                                  pa->stream));
    QPSK_HIP_TRY(hipStreamSynchronize(pa->stream));
    pa->host.swap(next);
    return QPSK_OK;
}

int qpsk_path_apply_fmt(qpsk_path *pa, int32_t fmt_in, const void *in, int64_t stride_in, float scale_in,
                        int32_t fmt_out, int32_t norm_out, void *out, int64_t stride_out, int64_t out_cap,
                        float scale_out, int64_t n_samples, const int64_t *lengths, int64_t *n_out, int32_t mem) {
    if (!pa) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    int rc;
    if ((rc = qpsk::check_row_formats("path", fmt_in, scale_in, fmt_out, norm_out, scale_out, mem))) return rc;
    if (!n_out) return fail(QPSK_ERR_ARGUMENT_NULL, "n_out is null");
    const int S = pa->S;
    const bool host = mem == QPSK_MEM_HOST;
    const int64_t ieb = qpsk::fmt_elem_bytes(fmt_in), oeb = qpsk::fmt_elem_bytes(fmt_out);
    int64_t n_call, n_out_max;
    std::vector<int64_t> cnt(S);
    if ((rc = qpsk::path_check_call(pa->host.data(), S, stride_in, stride_out, out_cap, n_samples, lengths, cnt.data(),
                                    &n_call, &n_out_max)))
        return rc;
    if (n_call > 0) {
        if (!in || (n_out_max > 0 && !out)) return fail(QPSK_ERR_ARGUMENT_NULL, "in or out is null");
        if (!host && ((rc = check_device_rows("input", fmt_in, in, stride_in)) ||
                      (out && (rc = check_device_rows("output", fmt_out, out, stride_out)))))
            return rc;
        if (out && qpsk::rows_overlap(in, S, stride_in, n_samples, ieb, out, S, stride_out, out_cap, oeb))
            return fail(QPSK_ERR_ARGUMENT, "out must not overlap in");
    }
    std::memcpy(n_out, cnt.data(), sizeof(int64_t) * S);
    if (n_call == 0) return QPSK_OK;   // nothing taken: nothing emitted, no state moves

    DeviceGuard guard;
    QPSK_HIP_TRY(hipSetDevice(pa->device));
    hipStream_t st = pa->stream;
    PathArgs a{};
    a.in = in;
    a.out = out;
    a.in_stride = stride_in;
    a.out_stride = stride_out;
    a.scale_in = scale_in;
    a.scale_out = scale_out;
    a.fmt_in = fmt_in;
    a.fmt_out = fmt_out;
    a.n = n_samples;
    a.state = pa->d_state;
    a.S = S;
    if ((rc = pa->upload_lengths(lengths, S, &a.lengths))) return rc;
    if (host) {
        if ((rc = pa->stage_out(kStaging, oeb, std::max<int64_t>(n_out_max, 1), S, &a.out, &a.out_stride)) ||
            (rc = pa->stage_in(kStaging, in, stride_in, ieb, n_call, S, &a.in, &a.in_stride)))
            return rc;
        // what lies past a row's emitted length comes back as it was
        if (n_out_max > 0)
            QPSK_HIP_TRY(hipMemcpy2DAsync(a.out, a.out_stride * oeb, out, stride_out * oeb, 2 * n_out_max * oeb, S,
                                          hipMemcpyHostToDevice, st));
    }
    a.in_pair = pair_rows(fmt_in, a.in, a.in_stride);
    a.out_pair = pair_rows(fmt_out, a.out, a.out_stride);
    a.in_wide = qpsk::wide_rows(fmt_in, a.in, a.in_stride);
    if (n_out_max > 0) {
        const unsigned tiles = static_cast<unsigned>((n_out_max + kTile - 1) / kTile);
        const dim3 grid(tiles, std::min(S, kGridY), (S + kGridY - 1) / kGridY);
        hipLaunchKernelGGL(path_kernel, grid, dim3(kThreads), 0, st, a);
        QPSK_HIP_TRY(hipGetLastError());
    }
    const int64_t lanes = static_cast<int64_t>(S) * kPathHist;
    hipLaunchKernelGGL(path_state_kernel, dim3(static_cast<unsigned>((lanes + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       st, a);
    QPSK_HIP_TRY(hipGetLastError());
    qpsk::advance_rows(pa->host.data(), S, n_samples, lengths, cnt.data());
    if (host && n_out_max > 0)
        QPSK_HIP_TRY(hipMemcpy2DAsync(out, stride_out * oeb, a.out, a.out_stride * oeb, 2 * n_out_max * oeb, S,
                                      hipMemcpyDeviceToHost, st));
    if (host || lengths) QPSK_HIP_TRY(hipStreamSynchronize(st));
    return QPSK_OK;
}

int qpsk_path_get_state(qpsk_path *pa, void *host_buf, int64_t buf_bytes) {
    if (!pa || !host_buf) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    const int64_t want = static_cast<int64_t>(pa->S) * static_cast<int64_t>(sizeof(PathState));
    int rc;
    if ((rc = qpsk::check_state_bytes("path", buf_bytes, want))) return rc;
    return pa->state_out(host_buf, pa->d_state, want);
}

int qpsk_path_set_state(qpsk_path *pa, const void *host_buf, int64_t buf_bytes) {
    if (!pa) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    int rc;
    if ((rc = qpsk_path_state_check(pa->S, host_buf, buf_bytes)) || (rc = pa->state_in(pa->d_state, host_buf, buf_bytes)))
        return rc;
    std::memcpy(pa->host.data(), host_buf, buf_bytes);
    return QPSK_OK;
}

int qpsk_path_reset_streams(qpsk_path *pa, const int32_t *streams, int32_t n) {
    if (!pa) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    int rc;
    if ((rc = qpsk_stream_list_check(pa->S, streams, n))) return rc;
    DeviceGuard guard;
    QPSK_HIP_TRY(hipSetDevice(pa->device));
    std::vector<PathState> st(n);   // lives until the synchronise below
    for (int32_t k = 0; k < n; ++k) {
        st[k] = qpsk::path_state_new(pa->p, streams[k]);
        st[k].n_taps = pa->host[streams[k]].n_taps;   // the taps stay
        std::memcpy(st[k].taps, pa->host[streams[k]].taps, sizeof(st[k].taps));
        QPSK_HIP_TRY(hipMemcpyAsync(pa->d_state.get() + streams[k], &st[k], sizeof(PathState), hipMemcpyHostToDevice,
                                    pa->stream));
    }
    QPSK_HIP_TRY(hipStreamSynchronize(pa->stream));
    for (int32_t k = 0; k < n; ++k) pa->host[streams[k]] = st[k];
    return QPSK_OK;
}

}  // extern "C"
