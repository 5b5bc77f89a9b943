// qpsk_tuner.hip -- the tuner (include/qpsk_demod.h, "The tuner on the device")
// on S streams: the two kernels and the entry points that need a device.  The
// per-sample functions, the state record, the design, the checks and the host
// form of the call are qpsk_tuner.h / qpsk_tuner.cpp.
//
// tuner_kernel: every output is independent, so, as in path_kernel, one
// workgroup of 256 threads takes one stream's run of QPSK_TUNER_TILE_OUTPUTS =
// 1024 outputs, k0 .. k0 + cnt - 1.  Their positions do not decrease, so the
// inputs they read are one window: x[floor(p_k0) - T/2 + 1 .. floor(p_last) +
// T/2], at most 1023 * 4 + 2 + 32 = 4126 samples.
//
//   stage   the window of x, widened, into LDS (stage_window: 16 bytes a lane
//           where the rows allow it; the state's history in front of the call's
//           first sample, +0 before the stream's start), and the prototype as
//           (h, d) pairs, 64 T + 1 of them, beside it.
//   mix     after a barrier, in place: a lane forms ph of its sample's absolute
//           index with one 64-bit multiply, reads the two table entries from
//           global memory (16 KB that every workgroup shares: they stay in the
//           cache) and writes z over x.
//   filter  after one more barrier, a lane takes every 256th output: position,
//           q and f in double, then T steps of one (h, d) pair and one z, both
//           8-byte LDS reads, the quantiser, one coalesced store.  The pairs lie
//           phase-minor (index 64 (T - 1 - j) + q), so lanes whose q differ by
//           one read neighbouring banks.  T = 8 and 16 are unrolled.
//
// LDS: 4128 * 8 bytes of window and 8 (64 T + 1) of pairs: 37128 bytes at T = 8,
// 41224 at T = 16, 49416 in the general form; three workgroups a CU, four at
// T = 8.  A workgroup
// finds its stream's output count itself (tuner_count of the state and the
// call's length, as the host did), so no count is uploaded and a call without
// lengths is queued whole.
//
// tuner_state_kernel runs behind tuner_kernel, when nobody reads the old
// history any more: 32 lanes a stream read the new history's samples (from the
// call's last samples, or from the old history when the call was shorter than
// 32), and write them behind a barrier; lane 0 advances the positions.
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
#include "qpsk_tuner.h"

struct qpsk_tuner : qpsk::RowHandle {
    qpsk_tuner_params p{};
    int S = 0, T = 0;
    qpsk::DevBuf<qpsk::TunerState> d_state;   // [S]
    qpsk::DevBuf<float2> d_hd;                // [64 T + 1]: (h, d)
    qpsk::DevBuf<float2> d_osc;               // [2][1024]: the coarse table, then the fine one
    std::vector<qpsk::TunerState> host;       // [S]: the records as the device will hold them behind the calls
                                              // queued so far (the history is not kept here)
    std::vector<double> r0;                   // [S]: each stream's created r, for reset_streams
};

namespace {

using qpsk::check_device_rows;
using qpsk::DeviceGuard;
using qpsk::fail;
using qpsk::kTunerHist;
using qpsk::kTunerTable;
using qpsk::load_sample;
using qpsk::pair_rows;
using qpsk::row_length;
using qpsk::store_sample;
using qpsk::TunerC;
using qpsk::TunerState;

constexpr int kTile = QPSK_TUNER_TILE_OUTPUTS;
constexpr int kThreads = 256;
constexpr int kWin = 4128;                    // >= (kTile - 1) * 4 + 2 + 32
constexpr int kPoints = QPSK_TUNER_PHASES * QPSK_TUNER_MAX_TAPS + 1;
constexpr int kGridY = 65535;
static_assert((kTile - 1) * 4 + 2 + QPSK_TUNER_MAX_TAPS <= kWin, "a tile's window fits");
static_assert(kThreads % kTunerHist == 0, "a stream's history lanes share a workgroup");

struct TunerArgs {
    const void *in;
    void *out;
    int64_t in_stride, out_stride;   // elements
    float scale_in, scale_out;
    int fmt_in, fmt_out;
    int in_pair, out_pair;           // CF32 rows 8-byte aligned: one access a sample
    int in_wide;                     // input rows 16-byte aligned and pitched
    const int64_t *lengths;          // device, checked; nullptr: n for every stream
    int64_t n;
    TunerState *state;
    const float2 *hd;                // [64 T + 1]
    const float2 *osc;               // [2][1024]
    int S, T;
};

// the filter of one output: TT taps unrolled, or T of them where TT = 0
template <int TT>
__device__ __forceinline__ TunerC filter_one(const float2 *hs, const float2 *zs, int T, int base, int q, float f) {
    TunerC acc{0.0f, 0.0f};
    const int taps = TT ? TT : T;
#pragma unroll
    for (int j = 0; j < taps; ++j) {
        const float2 c = hs[QPSK_TUNER_PHASES * (taps - 1 - j) + q];
        const float2 z = zs[base + j];
        qpsk::tuner_tap(acc, c.x, c.y, f, z.x, z.y);
    }
    return acc;
}

template <int TT>
__global__ __launch_bounds__(kThreads) void tuner_kernel(TunerArgs a) {
    __shared__ float2 xs[kWin];
    __shared__ float2 hs[TT ? QPSK_TUNER_PHASES * TT + 1 : kPoints];
#ifdef QPSK_TUNER_OSC_LDS
    __shared__ float2 os[2 * kTunerTable];   // the A/B of profiles/tuner_tables_ab.txt: the tables staged too
#endif
    const int tid = threadIdx.x;
    const int s = blockIdx.z * kGridY + blockIdx.y;
    if (s >= a.S) return;
    const TunerState &st = a.state[s];
    const double r = st.r, tau = st.tau;
    const int64_t in_pos = st.in_pos, out_pos = st.out_pos;
    const int T = TT ? TT : a.T;
    const int64_t len = row_length(a, s);
    const int64_t total = qpsk::tuner_count(r, tau, T, out_pos, in_pos + len);
    const int64_t o0 = static_cast<int64_t>(blockIdx.x) * kTile;
    if (o0 >= total) return;
    const int cnt = total - o0 < kTile ? static_cast<int>(total - o0) : kTile;
    const int64_t k0 = out_pos + o0;
    int64_t n_first, n_last;
    int q_unused;
    float f_unused;
    qpsk::tuner_pos(r, tau, k0, &n_first, &q_unused, &f_unused);
    qpsk::tuner_pos(r, tau, k0 + cnt - 1, &n_last, &q_unused, &f_unused);
    const int64_t xlen64 = n_last - n_first + T;
    // a state that qpsk_tuner_state_check accepted cannot fail this
    if (!qpsk::tuner_taps_ok(T) || xlen64 < T || xlen64 > kWin) return;
    const int xlen = static_cast<int>(xlen64);
    const int64_t i0 = n_first - T / 2 + 1;   // xs[0] as an absolute index
    const int64_t j0 = i0 - in_pos;           // and as an index into the call's row

    const int64_t in_eb = qpsk::fmt_elem_bytes(a.fmt_in), out_eb = qpsk::fmt_elem_bytes(a.fmt_out);
    const char *irow = static_cast<const char *>(a.in) + static_cast<int64_t>(s) * a.in_stride * in_eb;
    qpsk::stage_window<kThreads>(xs, j0, xlen, len, irow, st.hist, kTunerHist, a, tid);
    for (int m = tid; m < qpsk::tuner_points(T); m += kThreads) hs[m] = a.hd[m];
#ifdef QPSK_TUNER_OSC_LDS
    for (int m = tid; m < 2 * kTunerTable; m += kThreads) os[m] = a.osc[m];
    const float2 *osc = os;
#else
    const float2 *osc = a.osc;
#endif
    __syncthreads();

    // the mixer is pointwise: a lane rewrites the samples it read itself
    const uint64_t ph0 = st.ph0;
    const int64_t fw = st.fw;
    const float(*coarse)[2] = reinterpret_cast<const float(*)[2]>(osc);
    const float(*fine)[2] = reinterpret_cast<const float(*)[2]>(osc + kTunerTable);
    for (int m = tid; m < xlen; m += kThreads) {
        const float2 x = xs[m];
        const TunerC z = qpsk::tuner_mix(TunerC{x.x, x.y}, qpsk::tuner_osc(qpsk::tuner_phase(ph0, fw, i0 + m), coarse, fine));
        xs[m] = make_float2(z.re, z.im);
    }
    __syncthreads();

    char *orow = static_cast<char *>(a.out) + static_cast<int64_t>(s) * a.out_stride * out_eb;
    for (int o = tid; o < cnt; o += kThreads) {
        int64_t n;
        int q;
        float f;
        qpsk::tuner_pos(r, tau, k0 + o, &n, &q, &f);
        // p does not decrease in k: n - n_first lies in [0, xlen - T]; held there all the same
        int64_t base = n - n_first;
        base = base < 0 ? 0 : (base > xlen - T ? xlen - T : base);
        const TunerC y = filter_one<TT>(hs, xs, T, static_cast<int>(base), q, f);
        store_sample(orow, a.fmt_out, a.out_pair, o0 + o, make_float2(y.re, y.im), a.scale_out);
    }
}

__global__ __launch_bounds__(kThreads) void tuner_state_kernel(TunerArgs a) {
    const int64_t g = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x;
    const int s = static_cast<int>(g / kTunerHist), h = static_cast<int>(g % kTunerHist);
    const bool live = s < a.S;
    float2 v = make_float2(0.0f, 0.0f);
    int64_t len = 0, cnt = 0;
    if (live) {
        const TunerState &st = a.state[s];
        len = row_length(a, s);
        cnt = qpsk::tuner_count(st.r, st.tau, a.T, st.out_pos, st.in_pos + len);
        const int64_t j = len - kTunerHist + h;   // the new hist[h] as an index into the call's row
        if (j >= 0) {
            const char *irow = static_cast<const char *>(a.in) +
                               static_cast<int64_t>(s) * a.in_stride * qpsk::fmt_elem_bytes(a.fmt_in);
            v = load_sample(irow, a.fmt_in, a.in_pair, j, a.scale_in);
        } else {
            v = make_float2(st.hist[len + h][0], st.hist[len + h][1]);   // 0 <= len + h < 32
        }
    }
    __syncthreads();   // every lane has read the old history and the old positions
    if (live) {
        TunerState &st = a.state[s];
        st.hist[h][0] = v.x;
        st.hist[h][1] = v.y;
        if (h == 0) {
            st.in_pos += len;
            st.out_pos += cnt;
        }
    }
}

// what a failed grow of a staging buffer names (alloc_status)
constexpr const char *kStaging = "tuner staging";

// (h, d) of prototype h behind the calls queued so far; complete on return
int upload_taps(qpsk_tuner *tu, const float *h) {
    std::vector<float2> hd(qpsk::tuner_points(tu->T));
    qpsk::tuner_pairs(tu->T, h, reinterpret_cast<float(*)[2]>(hd.data()));
    QPSK_HIP_TRY(hipMemcpyAsync(tu->d_hd, hd.data(), hd.size() * sizeof(float2), hipMemcpyHostToDevice, tu->stream));
    QPSK_HIP_TRY(hipStreamSynchronize(tu->stream));
    return QPSK_OK;
}

}  // namespace

extern "C" {

int qpsk_tuner_create(const qpsk_tuner_params *p, int32_t n_streams, const double *freq, const double *rate,
                      qpsk_tuner **out) {
    if (!out) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    *out = nullptr;
    int rc;
    if ((rc = qpsk::tuner_check_params(p, n_streams, freq, rate))) return rc;
    DeviceGuard guard;
    auto *tu = new qpsk_tuner();
    tu->p = *p;
    tu->S = n_streams;
    tu->T = p->taps_per_phase;
    tu->host.resize(n_streams);
    tu->r0.resize(n_streams);
    for (int32_t s = 0; s < n_streams; ++s) {
        tu->r0[s] = rate ? rate[s] : p->rate;
        tu->host[s] = qpsk::tuner_state_new(*p, freq ? freq[s] : p->freq, tu->r0[s]);
    }
    std::vector<float> h(qpsk::tuner_points(tu->T));
    qpsk::tuner_design(tu->T, qpsk::tuner_cutoff(*p), h.data());
    std::vector<float2> osc(2 * kTunerTable);
    std::memcpy(osc.data(), qpsk::tuner_coarse(), sizeof(float2) * kTunerTable);
    std::memcpy(osc.data() + kTunerTable, qpsk::tuner_fine(), sizeof(float2) * kTunerTable);
    if (tu->open(p->device, n_streams) != hipSuccess || tu->d_state.alloc(n_streams) != hipSuccess ||
        tu->d_hd.alloc(h.size()) != hipSuccess || tu->d_osc.alloc(osc.size()) != hipSuccess ||
        hipMemcpy(tu->d_state, tu->host.data(), tu->host.size() * sizeof(TunerState), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(tu->d_osc, osc.data(), osc.size() * sizeof(float2), hipMemcpyHostToDevice) != hipSuccess ||
        upload_taps(tu, h.data()) != QPSK_OK) {
        delete tu;
        return fail(QPSK_ERR_DEVICE, "tuner device set-up failed (no GPU?)");
    }
    *out = tu;
    return QPSK_OK;
}

int qpsk_tuner_destroy(qpsk_tuner *tu) { return qpsk::row_handle_destroy(tu); }

int qpsk_tuner_set_stream(qpsk_tuner *tu, void *hip_stream) {
    if (!tu) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    return tu->set_stream(hip_stream);
}

int qpsk_tuner_set_taps(qpsk_tuner *tu, const float *h, int64_t n_points) {
    if (!tu) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    int rc;
    if ((rc = qpsk::tuner_check_taps(h, n_points, tu->T))) return rc;
    DeviceGuard guard;
    QPSK_HIP_TRY(hipSetDevice(tu->device));
    return upload_taps(tu, h);
}

int qpsk_tuner_set_freq(qpsk_tuner *tu, const int32_t *streams, int32_t n, const double *freqs) {
    if (!tu) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    int rc;
    if ((rc = qpsk_stream_list_check(tu->S, streams, n))) return rc;
    if (n > 0 && !freqs) return fail(QPSK_ERR_ARGUMENT_NULL, "freqs are null");
    for (int32_t k = 0; k < n; ++k)
        if (!qpsk::tuner_freq_ok(freqs[k]))
            return fail(QPSK_ERR_OUT_OF_RANGE, "freqs[" + std::to_string(k) + "] must lie in [-0.5, 0.5)");
    DeviceGuard guard;
    QPSK_HIP_TRY(hipSetDevice(tu->device));
    // fw and ph0 lie side by side in a record
    struct Osc {
        int64_t fw;
        uint64_t ph0;
    };
    static_assert(offsetof(TunerState, ph0) == offsetof(TunerState, fw) + sizeof(int64_t), "one part");
    std::vector<Osc> next(n);   // lives until the synchronise below
    for (int32_t k = 0; k < n; ++k) {
        const TunerState &st = tu->host[streams[k]];
        next[k].fw = qpsk::tuner_freq_word(freqs[k]);
        next[k].ph0 = qpsk::tuner_retune(st.ph0, st.fw, next[k].fw, st.in_pos);
        QPSK_HIP_TRY(hipMemcpyAsync(reinterpret_cast<char *>(tu->d_state.get() + streams[k]) + offsetof(TunerState, fw),
                                    &next[k], sizeof(Osc), hipMemcpyHostToDevice, tu->stream));
    }
    QPSK_HIP_TRY(hipStreamSynchronize(tu->stream));
    for (int32_t k = 0; k < n; ++k) {
        tu->host[streams[k]].fw = next[k].fw;
        tu->host[streams[k]].ph0 = next[k].ph0;
    }
    return QPSK_OK;
}

int qpsk_tuner_apply_fmt(qpsk_tuner *tu, int32_t fmt_in, const void *in, int64_t stride_in, float scale_in,
                         int32_t fmt_out, int32_t norm_out, void *out, int64_t stride_out, int64_t out_cap,
                         float scale_out, int64_t n_samples, const int64_t *lengths, int64_t *n_out, int32_t mem) {
    if (!tu) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    int rc;
    if ((rc = qpsk::check_row_formats("tuner", fmt_in, scale_in, fmt_out, norm_out, scale_out, mem))) return rc;
    if (!n_out) return fail(QPSK_ERR_ARGUMENT_NULL, "n_out is null");
    const int S = tu->S;
    const bool host = mem == QPSK_MEM_HOST;
    const int64_t ieb = qpsk::fmt_elem_bytes(fmt_in), oeb = qpsk::fmt_elem_bytes(fmt_out);
    int64_t n_call, n_out_max;
    std::vector<int64_t> cnt(S);
    if ((rc = qpsk::tuner_check_call(tu->host.data(), S, tu->T, stride_in, stride_out, out_cap, n_samples, lengths,
                                     cnt.data(), &n_call, &n_out_max)))
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
    QPSK_HIP_TRY(hipSetDevice(tu->device));
    hipStream_t st = tu->stream;
    TunerArgs a{};
    a.in = in;
    a.out = out;
    a.in_stride = stride_in;
    a.out_stride = stride_out;
    a.scale_in = scale_in;
    a.scale_out = scale_out;
    a.fmt_in = fmt_in;
    a.fmt_out = fmt_out;
    a.n = n_samples;
    a.state = tu->d_state;
    a.hd = tu->d_hd;
    a.osc = tu->d_osc;
    a.S = S;
    a.T = tu->T;
    if ((rc = tu->upload_lengths(lengths, S, &a.lengths))) return rc;
    if (host) {
        if ((rc = tu->stage_out(kStaging, oeb, std::max<int64_t>(n_out_max, 1), S, &a.out, &a.out_stride)) ||
            (rc = tu->stage_in(kStaging, in, stride_in, ieb, n_call, S, &a.in, &a.in_stride)))
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
        if (tu->T == 16) hipLaunchKernelGGL(tuner_kernel<16>, grid, dim3(kThreads), 0, st, a);
        else if (tu->T == 8) hipLaunchKernelGGL(tuner_kernel<8>, grid, dim3(kThreads), 0, st, a);
        else hipLaunchKernelGGL(tuner_kernel<0>, grid, dim3(kThreads), 0, st, a);
        QPSK_HIP_TRY(hipGetLastError());
    }
    const int64_t lanes = static_cast<int64_t>(S) * kTunerHist;
    hipLaunchKernelGGL(tuner_state_kernel, dim3(static_cast<unsigned>((lanes + kThreads - 1) / kThreads)), dim3(kThreads),
                       0, st, a);
    QPSK_HIP_TRY(hipGetLastError());
    qpsk::advance_rows(tu->host.data(), S, n_samples, lengths, cnt.data());
    if (host && n_out_max > 0)
        QPSK_HIP_TRY(hipMemcpy2DAsync(out, stride_out * oeb, a.out, a.out_stride * oeb, 2 * n_out_max * oeb, S,
                                      hipMemcpyDeviceToHost, st));
    if (host || lengths) QPSK_HIP_TRY(hipStreamSynchronize(st));
    return QPSK_OK;
}

int qpsk_tuner_get_state(qpsk_tuner *tu, void *host_buf, int64_t buf_bytes) {
    if (!tu || !host_buf) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    const int64_t want = static_cast<int64_t>(tu->S) * static_cast<int64_t>(sizeof(TunerState));
    int rc;
    if ((rc = qpsk::check_state_bytes("tuner", buf_bytes, want))) return rc;
    return tu->state_out(host_buf, tu->d_state, want);
}

int qpsk_tuner_set_state(qpsk_tuner *tu, const void *host_buf, int64_t buf_bytes) {
    if (!tu) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    int rc;
    if ((rc = qpsk_tuner_state_check(&tu->p, tu->S, host_buf, buf_bytes)) ||
        (rc = tu->state_in(tu->d_state, host_buf, buf_bytes)))
        return rc;
    std::memcpy(tu->host.data(), host_buf, buf_bytes);
    return QPSK_OK;
}

int qpsk_tuner_reset_streams(qpsk_tuner *tu, const int32_t *streams, int32_t n) {
    if (!tu) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    int rc;
    if ((rc = qpsk_stream_list_check(tu->S, streams, n))) return rc;
    DeviceGuard guard;
    QPSK_HIP_TRY(hipSetDevice(tu->device));
    std::vector<TunerState> st(n);   // lives until the synchronise below
    for (int32_t k = 0; k < n; ++k) {
        st[k] = qpsk::tuner_state_new(tu->p, 0.0, tu->r0[streams[k]]);
        st[k].fw = tu->host[streams[k]].fw;   // the tuning stays
        QPSK_HIP_TRY(hipMemcpyAsync(tu->d_state.get() + streams[k], &st[k], sizeof(TunerState), hipMemcpyHostToDevice,
                                    tu->stream));
    }
    QPSK_HIP_TRY(hipStreamSynchronize(tu->stream));
    for (int32_t k = 0; k < n; ++k) tu->host[streams[k]] = st[k];
    return QPSK_OK;
}

}  // extern "C"
