// qpsk_channel.hip -- the test bench's channel (include/qpsk_demod.h, "The test
// bench's channel on the device") on S streams: the kernel and the entry points
// that need a device.  The oscillator itself, the state record and the state
// check are qpsk_channel.h / qpsk_channel.cpp.
//
// channel_kernel: one workgroup of four waves holds QPSK_CHANNEL_TILE_STREAMS =
// 16 streams, i.e. 32 oscillators, and walks their rows in blocks of
// QPSK_CHANNEL_BLOCK_SAMPLES = 64 samples.
//
//   wave 0, the scan   lane l steps oscillator l & 1 (0 tx, 1 rx) of stream
//                      l >> 1: chan_nco_step, whose phase add and wrap round in
//                      every sample and so stay one serial chain per oscillator,
//                      with the drift draw and the clamp every `interval`
//                      samples.  It leaves the block's phases in LDS.
//   waves 1..3, trig   take the block the scan finished one step earlier (the
//                      phases are double buffered, one barrier a block): a wave
//                      takes whole rows, a lane one sample, so a row's 64
//                      samples are one coalesced load and one coalesced store.
//                      Two qpsk_glibc_sincos (branch-free form, table in LDS),
//                      the optional noise sample (a third one), the two complex
//                      products in double, one rounding to float, the quantiser.
//
// A lane reads its sample before it writes it and no other lane touches it, so
// out == in works.  Lanes past a row's length load and store nothing.  The
// scan lanes carry the oscillators in registers across the whole call and
// write the state back once, behind the last barrier; pos is read by the trig
// lanes before that and advanced by the tx lane.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "qpsk_channel.h"
#include "qpsk_demod.h"
#include "qpsk_device.h"
#include "qpsk_glibc_trig.h"
#include "qpsk_internal.h"
#include "qpsk_quantise.h"
#include "qpsk_row_call.h"
#include "qpsk_row_handle.h"
#include "qpsk_sample_rows.h"

struct qpsk_channel : qpsk::RowHandle {
    qpsk_channel_params p{};
    int S = 0;
    qpsk::DevBuf<qpsk::ChanState> d_state;   // [S]
};

namespace {

using qpsk::ChanNco;
using qpsk::ChanNcoConst;
using qpsk::ChanState;
using qpsk::check_device_rows;
using qpsk::DeviceGuard;
using qpsk::fail;
using qpsk::load_sample;
using qpsk::pair_rows;
using qpsk::row_length;
using qpsk::store_sample;

constexpr int kStreams = QPSK_CHANNEL_TILE_STREAMS;
constexpr int kBlock = QPSK_CHANNEL_BLOCK_SAMPLES;
constexpr int kThreads = 256;
constexpr int kTrigWaves = kThreads / 64 - 1;
constexpr int kPitch = kBlock + 1;           // doubles a row of phases takes: the scan lanes' stores spread over the banks
static_assert(2 * kStreams <= 64, "one scan lane per oscillator, in one wave");
static_assert(kBlock == 64, "a trig lane takes one sample of a block");

struct ChanArgs {
    ChanNcoConst tx, rx;
    double noise_rms;
    uint64_t noise_seed;
    uint64_t first_stream;
    const void *in;
    void *out;
    int64_t in_stride, out_stride;   // elements
    float scale_in, scale_out;
    int fmt_in, fmt_out;
    int in_pair, out_pair;           // CF32 rows 8-byte aligned: one access a sample
    const int64_t *lengths;          // device, checked; nullptr: n for every stream
    int64_t n;
    ChanState *state;
    int S;
};

// Math.Clamp(v, -1.0f, 1.0f): a NaN stays
__device__ __forceinline__ float clamp1(float v) { return v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v); }

__global__ __launch_bounds__(kThreads) void channel_kernel(ChanArgs a) {
    __shared__ double tab[440];
    __shared__ double ph[2][2 * kStreams][kPitch];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int s0 = blockIdx.x * kStreams;
    for (int k = tid; k < 440; k += kThreads) tab[k] = qpsk_gl_sincostab_dev[k];

    // the longest row of this workgroup's streams: the same in every lane
    int64_t n_wg = 0;
    for (int k = 0; k < kStreams && s0 + k < a.S; ++k) {
        const int64_t len = row_length(a, s0 + k);
        n_wg = len > n_wg ? len : n_wg;
    }
    const int64_t blocks = (n_wg + kBlock - 1) / kBlock;

    // scan lanes: wave 0, one per oscillator of a stream that exists
    const int ss = s0 + (lane >> 1);
    const bool scan = wave == 0 && lane < 2 * kStreams && ss < a.S;
    const bool is_rx = lane & 1;
    const ChanNcoConst c = is_rx ? a.rx : a.tx;
    ChanNco nco{};
    double inc = 0.0;
    int64_t scan_len = 0;
    if (scan) {
        nco = is_rx ? a.state[ss].rx : a.state[ss].tx;
        inc = qpsk::chan_inc(c, nco.cur_hz);
        scan_len = row_length(a, ss);
    }
    __syncthreads();   // the table

    const int64_t in_eb = qpsk::fmt_elem_bytes(a.fmt_in), out_eb = qpsk::fmt_elem_bytes(a.fmt_out);
    for (int64_t b = 0; b <= blocks; ++b) {
        if (wave == 0) {
            if (scan && b < blocks) {
                const int64_t left = scan_len - b * kBlock;
                const int m = left < kBlock ? static_cast<int>(left > 0 ? left : 0) : kBlock;
                double *row = ph[b & 1][lane];
                for (int i = 0; i < m; ++i) row[i] = qpsk::chan_nco_step(c, nco, inc);
            }
        } else if (b > 0) {
            const int64_t i = (b - 1) * kBlock + lane;
            for (int r = wave - 1; r < kStreams && s0 + r < a.S; r += kTrigWaves) {
                const int s = s0 + r;
                if (i >= row_length(a, s)) continue;
                const double pt = ph[(b - 1) & 1][2 * r][lane], pr = ph[(b - 1) & 1][2 * r + 1][lane];
                double ar, ai, br, bi;
                qpsk_glibc_sincos_bf_k(pt, tab, &ai, &ar, 0);   // both phases lie in [0, 2 pi]
                qpsk_glibc_sincos_bf_k(pr, tab, &bi, &br, 0);
                bi = -bi;                                       // Conjugate
                const double lr = (ar * br) - (ai * bi);        // System.Numerics.Complex *
                const double li = (ai * br) + (ar * bi);
                const char *irow = static_cast<const char *>(a.in) + static_cast<int64_t>(s) * a.in_stride * in_eb;
                const float2 x = load_sample(irow, a.fmt_in, a.in_pair, i, a.scale_in);
                double xr = x.x, xi = x.y;
                if (a.noise_rms > 0.0) {
                    double u1, u2, sn, cs;
                    qpsk::chan_noise_uniforms(a.noise_seed, a.first_stream + static_cast<uint64_t>(s),
                                              a.state[s].pos + i, &u1, &u2);
                    const double mag = sqrt(-2.0 * log(u1)) * a.noise_rms;
                    qpsk_glibc_sincos_bf_k(qpsk::kChanTwoPi * u2, tab, &sn, &cs, 0);   // (0, 2 pi]
                    xr += static_cast<double>(clamp1(static_cast<float>(mag * cs)));
                    xi += static_cast<double>(clamp1(static_cast<float>(mag * sn)));
                }
                const double yr = (xr * lr) - (xi * li);
                const double yi = (xi * lr) + (xr * li);
                char *orow = static_cast<char *>(a.out) + static_cast<int64_t>(s) * a.out_stride * out_eb;
                store_sample(orow, a.fmt_out, a.out_pair, i, make_float2(static_cast<float>(yr), static_cast<float>(yi)),
                             a.scale_out);
            }
        }
        __syncthreads();
    }
    // every read of pos lies in front of the last barrier
    if (scan) {
        if (is_rx) {
            a.state[ss].rx = nco;
        } else {
            a.state[ss].tx = nco;
            a.state[ss].pos += scan_len;
        }
    }
}

// what a failed grow of a staging buffer names (alloc_status)
constexpr const char *kStaging = "channel staging";

ChanArgs base_args(const qpsk_channel *ch) {
    ChanArgs a{};
    a.tx = qpsk::chan_nco_const(ch->p.lo_hz, ch->p.sample_rate, ch->p.tx_ppm);
    a.rx = qpsk::chan_nco_const(ch->p.lo_hz, ch->p.sample_rate, ch->p.rx_ppm);
    a.noise_rms = ch->p.noise_rms;
    a.noise_seed = ch->p.noise_seed;
    a.first_stream = static_cast<uint64_t>(ch->p.first_stream);
    a.state = ch->d_state;
    a.S = ch->S;
    return a;
}

}  // namespace

extern "C" {

int qpsk_channel_create(const qpsk_channel_params *p, int32_t n_streams, qpsk_channel **out) {
    if (!out) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    *out = nullptr;
    int rc;
    if ((rc = qpsk::chan_check_params(p, n_streams))) return rc;
    DeviceGuard guard;
    auto *ch = new qpsk_channel();
    ch->p = *p;
    ch->S = n_streams;
    std::vector<ChanState> st(n_streams);
    for (int32_t s = 0; s < n_streams; ++s) st[s] = qpsk::chan_state_new(*p, s);
    if (ch->open(p->device, n_streams) != hipSuccess || ch->d_state.alloc(n_streams) != hipSuccess ||
        hipMemcpy(ch->d_state, st.data(), st.size() * sizeof(ChanState), hipMemcpyHostToDevice) != hipSuccess) {
        delete ch;
        return fail(QPSK_ERR_DEVICE, "channel device set-up failed (no GPU?)");
    }
    *out = ch;
    return QPSK_OK;
}

int qpsk_channel_destroy(qpsk_channel *ch) { return qpsk::row_handle_destroy(ch); }

int qpsk_channel_set_stream(qpsk_channel *ch, void *hip_stream) {
    if (!ch) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    return ch->set_stream(hip_stream);
}

int qpsk_channel_apply_fmt(qpsk_channel *ch, int32_t fmt_in, const void *in, int64_t stride_in, float scale_in,
                           int32_t fmt_out, int32_t norm_out, void *out, int64_t stride_out, float scale_out,
                           int64_t n_samples, const int64_t *lengths, int32_t mem) {
    if (!ch) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    int rc;
    if ((rc = qpsk::check_row_formats("channel", fmt_in, scale_in, fmt_out, norm_out, scale_out, mem))) return rc;
    if (n_samples < 0) return fail(QPSK_ERR_ARGUMENT, "n_samples must not be negative");
    const int S = ch->S;
    int64_t n_call;
    if ((rc = qpsk::check_lengths(S, n_samples, lengths, &n_call))) return rc;
    if (n_call == 0) return QPSK_OK;
    if (!in || !out) return fail(QPSK_ERR_ARGUMENT_NULL, "in or out is null");
    if (n_samples > (INT64_MAX >> 4) || stride_in < 2 * n_samples || stride_out < 2 * n_samples)
        return fail(QPSK_ERR_ARGUMENT, "stride too small");
    if (in == out && (fmt_in != fmt_out || stride_in != stride_out))
        return fail(QPSK_ERR_ARGUMENT, "in place needs one format and one stride");
    const bool host = mem == QPSK_MEM_HOST;
    if (!host && ((rc = check_device_rows("input", fmt_in, in, stride_in)) ||
                  (rc = check_device_rows("output", fmt_out, out, stride_out))))
        return rc;

    DeviceGuard guard;
    QPSK_HIP_TRY(hipSetDevice(ch->device));
    hipStream_t st = ch->stream;
    ChanArgs a = base_args(ch);
    a.in = in;
    a.out = out;
    a.in_stride = stride_in;
    a.out_stride = stride_out;
    a.scale_in = scale_in;
    a.scale_out = scale_out;
    a.fmt_in = fmt_in;
    a.fmt_out = fmt_out;
    a.n = n_samples;
    const int64_t oeb = qpsk::fmt_elem_bytes(fmt_out);
    if ((rc = ch->upload_lengths(lengths, S, &a.lengths))) return rc;
    if (host) {
        if ((rc = ch->stage_out(kStaging, oeb, n_call, S, &a.out, &a.out_stride)) ||
            (rc = ch->stage_in(kStaging, in, stride_in, qpsk::fmt_elem_bytes(fmt_in), n_call, S, &a.in, &a.in_stride)))
            return rc;
        // what lies past a row's length comes back as it was
        if (lengths)
            QPSK_HIP_TRY(hipMemcpy2DAsync(a.out, a.out_stride * oeb, out, stride_out * oeb, 2 * n_call * oeb, S,
                                          hipMemcpyHostToDevice, st));
    }
    a.in_pair = pair_rows(fmt_in, a.in, a.in_stride);
    a.out_pair = pair_rows(fmt_out, a.out, a.out_stride);
    hipLaunchKernelGGL(channel_kernel, dim3((S + kStreams - 1) / kStreams), dim3(kThreads), 0, st, a);
    QPSK_HIP_TRY(hipGetLastError());
    if (host)
        QPSK_HIP_TRY(hipMemcpy2DAsync(out, stride_out * oeb, a.out, a.out_stride * oeb, 2 * n_call * oeb, S,
                                      hipMemcpyDeviceToHost, st));
    if (host || lengths) QPSK_HIP_TRY(hipStreamSynchronize(st));
    return QPSK_OK;
}

int qpsk_channel_get_state(qpsk_channel *ch, void *host_buf, int64_t buf_bytes) {
    if (!ch || !host_buf) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    const int64_t want = static_cast<int64_t>(ch->S) * static_cast<int64_t>(sizeof(ChanState));
    int rc;
    if ((rc = qpsk::check_state_bytes("channel", buf_bytes, want))) return rc;
    return ch->state_out(host_buf, ch->d_state, want);
}

int qpsk_channel_set_state(qpsk_channel *ch, const void *host_buf, int64_t buf_bytes) {
    if (!ch) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    int rc;
    if ((rc = qpsk_channel_state_check(&ch->p, ch->S, host_buf, buf_bytes))) return rc;
    return ch->state_in(ch->d_state, host_buf, buf_bytes);
}

int qpsk_channel_reset_streams(qpsk_channel *ch, const int32_t *streams, int32_t n) {
    if (!ch) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    int rc;
    if ((rc = qpsk_stream_list_check(ch->S, streams, n))) return rc;
    DeviceGuard guard;
    QPSK_HIP_TRY(hipSetDevice(ch->device));
    std::vector<ChanState> st(n);   // lives until the synchronise below
    for (int32_t k = 0; k < n; ++k) {
        st[k] = qpsk::chan_state_new(ch->p, streams[k]);
        QPSK_HIP_TRY(hipMemcpyAsync(ch->d_state.get() + streams[k], &st[k], sizeof(ChanState), hipMemcpyHostToDevice,
                                    ch->stream));
    }
    QPSK_HIP_TRY(hipStreamSynchronize(ch->stream));
    return QPSK_OK;
}

}  // extern "C"
