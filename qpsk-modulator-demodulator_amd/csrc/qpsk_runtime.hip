// qpsk_runtime.hip -- host runtime behind the C ABI (include/qpsk_demod.h):
// handle = a batch of S reference QPSKDeModulator instances living on one
// MI355X.  Owns the device buffers and the per-stream state, orders the kernels
// of one DeModulate call:
//
//     [FLL] -> matched-filter FIR -> FIR history carry -> M&M+Costas+decode
//
// qpsk_demod_process runs them on the handle's stream.  qpsk_demod_process_async
// splits each call into a front and a back stage on two library streams so
// that call k+1's front stage overlaps call k's back stage:
//
//     FLL off:  front = FIR + history        back = carry + loop kernel + copies
//     FLL on:   front = FLL                  back = FIR + history + carry + loop
//
// What the two stages share: the per-stream StreamState (its FLL fields are
// written only by the FLL, every other field only by the loop kernel), and the
// MF rows at the stage boundary, which are double-buffered (mf[2]; the second
// only when pipelined).  The FLL's output rows are one buffer: the FLL of call
// k+1 runs behind the FIR of call k, their only reader, on the front stream.
//
// Every buffer, event and stream is a member that releases itself
// (qpsk_device.h); the handle's destructor only waits for the queued work.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "qpsk_handle.h"

using namespace qpsk;

namespace {
bool fmt_8bit(int32_t fmt) { return fmt == QPSK_FMT_CS8 || fmt == QPSK_FMT_CU8; }
// samples a staged host row's pitch is a multiple of, so that the staged rows
// take the format's 16-byte loads whatever max_samples_per_call is
int64_t stage_pitch(int32_t fmt, int64_t n_max) {
    const int64_t m = fmt == QPSK_FMT_CF32 ? 1 : fmt == QPSK_FMT_CS16 ? 4 : 8;
    return (n_max + m - 1) / m * m;
}
const char *fmt_name(int32_t fmt) {
    return fmt == QPSK_FMT_CS16 ? "CS16" : fmt == QPSK_FMT_CS8 ? "CS8" : fmt == QPSK_FMT_CU8 ? "CU8" : "CF32";
}
}  // namespace

int qpsk::handle_taps(const qpsk_demod *h) { return h->T; }

namespace {

// The newest pipelined call's back stage, or nullptr.
const Event *last_async(const qpsk_demod *h) {
    return h->pipe.last_back >= 0 ? &h->pipe.e_back[h->pipe.last_back] : nullptr;
}

int flush_deferred(qpsk_demod *h);   // issues a deferred back stage (with the stage runners)

// Host wait for every pipelined call issued so far (a deferred back stage is
// issued first: every caller of this waits for all of the handle's work).
int drain_async(qpsk_demod *h) {
    int rc;
    if ((rc = flush_deferred(h))) return rc;
    if (const Event *e = last_async(h)) QPSK_HIP_TRY(e->sync());
    return QPSK_OK;
}

// lazily, for the first call that asks for symbols
int ensure_syms(qpsk_demod *h) {
    if (h->d_syms) return QPSK_OK;
    // on the handle's device whatever the calling thread's current one is
    // (a group's worker threads, qpsk_group.cpp)
    QPSK_HIP_TRY(hipSetDevice(h->p.device));
    return alloc_status(h->d_syms.alloc(static_cast<size_t>(2 * h->S * h->syms_cap)));
}

}  // namespace

// What the members cannot do for themselves: on the handle's device (the
// frees and the stream teardown behind this body too), after all queued work.
qpsk_demod::~qpsk_demod() {
    (void)hipSetDevice(p.device);
    drain_async(this);
    if (stream) hipStreamSynchronize(stream);
}

int qpsk::handle_sync(qpsk_demod *h) {
    int rc;
    if ((rc = drain_async(h))) return rc;
    QPSK_HIP_TRY(hipSetDevice(h->p.device));
    QPSK_HIP_TRY(hipStreamSynchronize(h->stream));
    return QPSK_OK;
}

int qpsk::call_length(int S, int64_t n_samples, const int64_t *lengths, int64_t *n_call) {
    *n_call = 0;
    if (lengths) {   // host memory in every call
        for (int s = 0; s < S; ++s) {
            if (lengths[s] < 0) return fail(QPSK_ERR_ARGUMENT, "negative length");
            *n_call = std::max(*n_call, lengths[s]);
        }
    } else {
        if (n_samples < 0) return fail(QPSK_ERR_ARGUMENT, "negative n_samples");
        *n_call = n_samples;
    }
    return QPSK_OK;
}

int qpsk::check_call(const qpsk_demod *h, int S, CallArgs &c) {
    if (!fmt_known(c.fmt)) return fail(QPSK_ERR_ARGUMENT, "unknown sample format");
    if (c.mode != QPSK_MODE_DEMODULATE && c.mode != QPSK_MODE_CONSTELLATION)
        return fail(QPSK_ERR_ARGUMENT, "unknown mode");
    if (c.mem != QPSK_MEM_HOST && c.mem != QPSK_MEM_DEVICE) return fail(QPSK_ERR_ARGUMENT, "unknown mem");
    int rc;
    int64_t n_call = 0;
    if ((rc = call_length(S, c.n_samples, c.lengths, &n_call))) return rc;
    if (n_call > kMaxCallSamples)
        return fail(QPSK_ERR_OUT_OF_RANGE, "calls above 2^31 - 129 samples per stream (a C# span holds 2^30)");
    if (n_call > 0 && !c.iq) return fail(QPSK_ERR_ARGUMENT_NULL, "SamplesIQ is null");
    if (n_call > 0 && c.stride_floats < 2 * n_call) return fail(QPSK_ERR_ARGUMENT, "stride too small");
    if (c.mode == QPSK_MODE_DEMODULATE && (!c.bits || !c.n_bits))
        return fail(QPSK_ERR_ARGUMENT_NULL, "bits / n_bits required");
    if (c.mode == QPSK_MODE_CONSTELLATION && (!c.syms || !c.n_syms))
        return fail(QPSK_ERR_ARGUMENT_NULL, "syms / n_syms required");
    const int64_t max_sym = qpsk_demod_max_symbols(h, n_call);
    if (c.bits && c.bits_stride_bytes < ((2 * max_sym + 7) / 8))
        return fail(QPSK_ERR_ARGUMENT, "bits_stride_bytes smaller than 2*max_symbols/8");
    if (c.syms && c.syms_stride_floats < 2 * max_sym)
        return fail(QPSK_ERR_ARGUMENT, "syms_stride_floats smaller than 2*max_symbols");
    if (n_call > 0 && c.mem == QPSK_MEM_DEVICE && (c.stride_floats & 1))
        return fail(QPSK_ERR_ARGUMENT, c.fmt == QPSK_FMT_CS16   ? "device stride_i16 must be even"
                                       : fmt_8bit(c.fmt) ? "device stride_elems of 8-bit rows must be even"
                                                         : "device stride_floats must be even");
    if (n_call > 0 && c.mem == QPSK_MEM_DEVICE && c.fmt == QPSK_FMT_CS16 && (reinterpret_cast<uintptr_t>(c.iq) & 3))
        return fail(QPSK_ERR_ARGUMENT, "device CS16 rows must be 4-byte aligned");
    if (n_call > 0 && c.mem == QPSK_MEM_DEVICE && fmt_8bit(c.fmt) && (reinterpret_cast<uintptr_t>(c.iq) & 1))
        return fail(QPSK_ERR_ARGUMENT, "device CS8 / CU8 rows must be 2-byte aligned");
    c.n_call = n_call;
    c.max_sym = max_sym;
    return QPSK_OK;
}

namespace {

// the launch-timestamp slots of the next timed call, or nullptr
unsigned long long *next_kt(qpsk_demod *h) {
    if (!h->probe.timing || !h->probe.d_kt || h->probe.kt_used >= kKtCalls) return nullptr;
    return h->probe.d_kt + static_cast<size_t>(kKtPerCall) * h->probe.kt_used++;
}

// optional IQ_Balancer pre-stage (IQ Balancer.cs:15-25) into d_iqb
void run_iqb(qpsk_demod *h, const float *x, int64_t x_stride, const int64_t *d_len, int64_t n_call,
             hipStream_t st) {
    IqbArgs ia{};
    ia.x = x; ia.x_stride = x_stride;
    ia.y = h->d_iqb; ia.y_stride = h->n_max;
    ia.lengths = d_len; ia.n = n_call;
    ia.state = h->d_state; ia.S = h->S;
    launch_iq_balance(ia, st);
}

// FLL (Band-Edge Filter.cs:64-87), README order FLL -> MF
void run_fll(qpsk_demod *h, const float *x, int64_t x_stride, const int64_t *d_len, int64_t n_call,
             float *y, hipStream_t st, unsigned long long *kt) {
    FllArgs fa{};
    fa.x = x; fa.x_stride = x_stride;
    fa.y = y; fa.y_stride = h->n_max;
    fa.delay = h->d_fll_delay;
    fa.lengths = d_len; fa.n = n_call;
    fa.state = h->d_state; fa.S = h->S;
    fa.kt = kt ? kt + kKtSpan[kKtFll] : nullptr;
    fa.clk = kt ? kt + kKtClk[kKtFll] : nullptr;
    launch_fll(fa, h->fp, st);
}

// CS16 or 8-bit rows ahead of a serial pre-stage (IQ balancer, FLL): widened into the
// call's own MF rows, which nothing reads until the matched filter, the last
// stage in front of the loop, has rewritten them (DESIGN.md, CS16 input).
// Float rows pass through.
const float *float_rows(qpsk_demod *h, InRows *in, const int64_t *d_len, int64_t n_call, float *mf,
                        hipStream_t st) {
    if (in->fmt != QPSK_FMT_CF32) {
        WidenArgs wa{};
        wa.x = in->x; wa.x_stride = in->stride;
        wa.y = mf; wa.y_stride = h->mf_stride; wa.y_offset = kMfPrefix;
        wa.lengths = d_len; wa.n = n_call;
        wa.x_scale = in->scale;
        launch_widen(wa, h->S, n_call, st, in->fmt);
        *in = InRows{mf + 2 * kMfPrefix, h->mf_stride, QPSK_FMT_CF32, 0.0f};
    }
    return static_cast<const float *>(in->x);
}

// The serial stages in front of the matched filter, each on the rows the one
// before it wrote: [CS16 widen ->] IQ balancer, [CS16 widen ->] FLL.  *in
// becomes the rows the matched filter reads; mf = the call's own MF rows.
void pre_stages(qpsk_demod *h, InRows *in, const int64_t *d_len, int64_t n_call, float *mf, hipStream_t st,
                unsigned long long *kt) {
    if (n_call <= 0) return;
    if (h->p.iq_balance) {
        const float *x = float_rows(h, in, d_len, n_call, mf, st);
        run_iqb(h, x, in->stride, d_len, n_call, st);
        *in = InRows{h->d_iqb, h->n_max, QPSK_FMT_CF32, 0.0f};
    }
    if (h->p.enable_fll) {
        const float *x = float_rows(h, in, d_len, n_call, mf, st);
        run_fll(h, x, in->stride, d_len, n_call, h->d_fll_out, st, kt);
        *in = InRows{h->d_fll_out, h->n_max, QPSK_FMT_CF32, 0.0f};
    }
}

// matched filter (QPSKDeModulator.cs:360) + FIR delay-line carry
int run_fir(qpsk_demod *h, const InRows &in, const int64_t *d_len, int64_t n_call,
            float *mf, hipStream_t st, unsigned long long *kt) {
    FirArgs fa{};
    fa.x = static_cast<const float *>(in.x); fa.x_stride = in.stride;
    fa.hist = h->d_hist[h->hist_cur];
    fa.lengths = d_len; fa.n = n_call;
    fa.y = mf; fa.y_stride = h->mf_stride; fa.y_offset = kMfPrefix;
    fa.kt = kt ? kt + kKtSpan[kKtFir] : nullptr;
    fa.clk = kt ? kt + kKtClk[kKtFir] : nullptr;
    if (h->probe.fir_phases) {
        fa.phases = h->probe.d_phases;
        fa.cu_map = h->probe.d_cu_map;
    }
    if (n_call > 0) {
        launch_fir(fa, h->d_hrev, h->T, h->W, h->S, n_call, st, in.fmt, in.scale);
        fa.kt = nullptr;
        fa.clk = nullptr;
        fa.phases = nullptr;
        launch_fir_hist(fa, h->d_hist[h->hist_cur ^ 1], h->T - 1, h->S, st, in.fmt, in.scale);
        h->hist_cur ^= 1;
    }
    return QPSK_OK;
}

// The residency gate of the pipelined path (process_async_one): one wave on
// the front stream, ahead of the FIR, polls the counter the loop kernel's
// workgroups bump as they start (s_sleep between reads) and ends when it
// reaches target -- or when cap wall-clock ticks have passed, counted in
// *timeouts.  The FIR behind it in stream order is dispatched only then, and
// a counter that never arrives (a dispatch serialised by a tool the
// environment predicate does not know) costs one cap per call, not a hang.  The gate orders dispatch only; no result
// depends on it.
__global__ void gate_wait_kernel(const unsigned long long *resident, unsigned long long target,
                                 unsigned long long cap, unsigned *timeouts) {
    if (threadIdx.x != 0) return;
    const unsigned long long t0 = wall_clock64();
    while (__hip_atomic_load(resident, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < target) {
        if (wall_clock64() - t0 > cap) {
            atomicAdd(timeouts, 1u);
            return;
        }
        __builtin_amdgcn_s_sleep(4);
    }
}

int gate_wait(qpsk_demod *h, hipStream_t st) {
    if (!h->pipe.gate_pending) return QPSK_OK;
    h->pipe.gate_pending = false;
    hipLaunchKernelGGL(gate_wait_kernel, dim3(1), dim3(64), 0, st, h->pipe.d_resident,
                       static_cast<unsigned long long>(h->pipe.resident_gate), h->pipe.gate_cap_ticks, h->pipe.d_gate);
    QPSK_HIP_TRY(hipGetLastError());
    return QPSK_OK;
}

// The end of a host-memory call: its counts (counts: device [2][S]) and the
// flags it raised come back, the host waits for the stream, and the caller
// gets the counts.
int host_epilogue(qpsk_demod *h, const Call &c, const int64_t *counts, hipStream_t st) {
    const int S = h->S;
    QPSK_HIP_TRY(hipMemcpyAsync(h->h_counts, counts, 2 * S * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    QPSK_HIP_TRY(hipMemcpyAsync(h->h_flags, h->d_flags + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    QPSK_HIP_TRY(hipStreamSynchronize(st));
    if (c.n_bits) std::memcpy(c.n_bits, h->h_counts, S * sizeof(int64_t));
    if (c.n_syms) std::memcpy(c.n_syms, h->h_counts + S, S * sizeof(int64_t));
    h->status_host |= *h->h_flags;
    return QPSK_OK;
}

// symbol sync + Costas + decode (QPSKDeModulator.cs:364-408) and the output copies
// resident: the pipelined path's residency counter (nullptr otherwise); the
// launch's workgroup count is added to h->pipe.resident_issued
int run_loop(qpsk_demod *h, const Call &c, const int64_t *d_len, float *mf, hipStream_t st,
             unsigned long long *kt, unsigned long long *resident = nullptr) {
    const int S = h->S;
    LoopArgs la{};
    la.mf = mf; la.mf_stride = h->mf_stride;
    la.carry = h->d_carry;
    la.lengths = d_len; la.n = c.n_call;
    la.state = h->d_state;
    la.bits = c.mode == QPSK_MODE_DEMODULATE ? h->d_bits : nullptr;
    la.bits_stride_words = h->bits_words;
    la.bits_cap_words = h->bits_words;
    la.n_bits = h->d_counts;
    la.syms = c.syms ? h->d_syms : nullptr;
    la.syms_stride = h->syms_cap;
    la.syms_cap = h->syms_cap;
    la.n_syms = h->d_counts + S;
    la.set_link(h->link.on ? h->link.d_link : nullptr);
    // device-memory outputs whose rows the kernel can address as its own (4-B
    // aligned word rows holding every word a row can take; float2-aligned
    // symbol rows): written in place, no staging copy behind the kernel
    const int64_t need_words = (2 * c.max_sym + 31) / 32;
    const bool direct_bits = !c.append && c.mem == QPSK_MEM_DEVICE && la.bits && c.n_bits &&
                             (reinterpret_cast<uintptr_t>(c.n_bits) & 7) == 0 &&
                             (reinterpret_cast<uintptr_t>(c.bits) & 3) == 0 && (c.bits_stride_bytes & 3) == 0 &&
                             c.bits_stride_bytes / 4 >= need_words;
    const bool direct_syms = !c.append && c.mem == QPSK_MEM_DEVICE && c.syms &&
                             (reinterpret_cast<uintptr_t>(c.syms) & 7) == 0 && (c.syms_stride_floats & 1) == 0 &&
                             c.syms_stride_floats / 2 >= c.max_sym;
    if (direct_bits) {
        la.bits = reinterpret_cast<uint32_t *>(c.bits);
        la.bits_stride_words = c.bits_stride_bytes / 4;
        la.bits_cap_words = c.bits_stride_bytes / 4;
        la.n_bits = c.n_bits;
    }
    if (direct_syms) {
        la.syms = c.syms;
        la.syms_stride = c.syms_stride_floats / 2;
        la.syms_cap = c.syms_stride_floats / 2;
        if (c.n_syms && (reinterpret_cast<uintptr_t>(c.n_syms) & 7) == 0) la.n_syms = c.n_syms;
    }
    la.S = S;
    // host-memory calls (chunks of one included) raise into slot 1, which the
    // call clears first and reads back at its end; device-memory calls into
    // slot 0, read by qpsk_demod_status
    la.flags = h->d_flags + (c.mem == QPSK_MEM_HOST ? 1 : 0);
    la.chunked = c.append ? 1 : 0;
    la.kt = kt ? kt + kKtSpan[kKtLoop] : nullptr;
    la.clk = kt ? kt + kKtClk[kKtLoop] : nullptr;
    la.cu_map = h->probe.fir_phases ? h->probe.d_cu_map : nullptr;
    la.resident = h->pipe.gate_publish ? resident : nullptr;
    const int grid = launch_loop(la, h->lp, c.mode, h->loop_variant, st, h->cus, h->T);
    QPSK_HIP_TRY(hipGetLastError());
    if (resident) {
        // the next FIR may start once min(grid, CUs) workgroups hold their CUs:
        // at most one 104-147 KB loop workgroup fits a CU, and those are the
        // first ones dispatched (never more than there are)
        h->pipe.resident_gate = h->pipe.resident_issued + static_cast<uint64_t>(std::min(grid, std::max(h->cus, 1)));
        h->pipe.resident_issued += static_cast<uint64_t>(grid);
        h->pipe.gate_pending = true;
    }
    if (c.append) {
        AppendArgs aa{};
        aa.dst_bits = c.mode == QPSK_MODE_DEMODULATE ? c.dst_bits : nullptr;
        aa.dst_bits_stride = c.dst_bits_stride;
        aa.dst_syms = c.syms ? c.dst_syms : nullptr;
        aa.dst_syms_stride = c.dst_syms_stride;
        aa.src_bits = h->d_bits;
        aa.src_bits_words = h->bits_words;
        aa.src_syms = h->d_syms;
        aa.src_syms_cap = h->syms_cap;
        aa.counts = h->d_counts;
        aa.acc = h->d_acc;
        aa.first = c.first ? 1 : 0;
        aa.last = c.last ? 1 : 0;
        aa.state = h->d_state;
        aa.S = S;
        launch_append(aa, st);
        QPSK_HIP_TRY(hipGetLastError());
        if (c.last) {
            if (c.dst_n_bits)
                QPSK_HIP_TRY(hipMemcpyAsync(c.dst_n_bits, h->d_acc, S * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
            if (c.dst_n_syms)
                QPSK_HIP_TRY(hipMemcpyAsync(c.dst_n_syms, h->d_acc + S, S * sizeof(int64_t), hipMemcpyDeviceToDevice,
                                            st));
        }
        return QPSK_OK;
    }
    const hipMemcpyKind kind = c.mem == QPSK_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    const int64_t bytes_row = (2 * c.max_sym + 7) / 8;
    if (c.bits && bytes_row > 0 && !direct_bits)
        QPSK_HIP_TRY(hipMemcpy2DAsync(c.bits, c.bits_stride_bytes, h->d_bits, h->bits_words * 4, bytes_row, S, kind,
                                      st));
    if (c.syms && c.max_sym > 0 && !direct_syms)
        QPSK_HIP_TRY(hipMemcpy2DAsync(c.syms, c.syms_stride_floats * sizeof(float), h->d_syms,
                                      2 * h->syms_cap * sizeof(float), 2 * c.max_sym * sizeof(float), S, kind, st));
    if (c.mem == QPSK_MEM_HOST) return host_epilogue(h, c, h->d_counts, st);
    if (c.n_bits && !direct_bits) QPSK_HIP_TRY(hipMemcpyAsync(c.n_bits, h->d_counts, S * sizeof(int64_t), kind, st));
    if (c.n_syms && !(direct_syms && la.n_syms == c.n_syms))
        QPSK_HIP_TRY(hipMemcpyAsync(c.n_syms, h->d_counts + S, S * sizeof(int64_t), kind, st));
    return QPSK_OK;
}

// A back stage on the back stream: the loop kernel on MF rows buf with its
// output copies, then the event the next user of those rows waits for.
int issue_back(qpsk_demod *h, const Call &c, const int64_t *d_len, int buf, unsigned long long *kt,
               unsigned long long *resident) {
    int rc;
    if ((rc = run_loop(h, c, d_len, h->d_mf[buf], h->s_back, kt, resident))) return rc;
    QPSK_HIP_TRY(h->pipe.e_back[buf].record(h->s_back));
    h->pipe.last_back = buf;
    return QPSK_OK;
}

}  // namespace (stage runners)

namespace {

// Streams, events and the second stage-boundary buffer of the pipelined path.
// The back stream gets the device's highest priority: its loop kernel is the
// latency-bound stage, the front stage fills the CUs it leaves idle.
int pipe_setup(qpsk_demod *h) {
    if (h->pipe.ready) return QPSK_OK;
    // every step makes what is missing and keeps what is there: a set-up that
    // failed part way runs again on the next pipelined call and completes,
    // without re-zeroing the counters it already made
    int least = 0, greatest = 0;
    QPSK_HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
    QPSK_HIP_TRY(h->s_front.create(hipStreamNonBlocking, least));
    QPSK_HIP_TRY(h->s_back.create(hipStreamNonBlocking, greatest));
    QPSK_HIP_TRY(h->pipe.e_in.ensure());
    for (int b = 0; b < 2; ++b) {
        QPSK_HIP_TRY(h->pipe.e_front[b].ensure());
        QPSK_HIP_TRY(h->pipe.e_back[b].ensure());
        QPSK_HIP_TRY(h->pipe.h_len[b].alloc(h->S));
    }
    QPSK_HIP_TRY(h->pipe.e_fll.ensure());
    if (!h->pipe.d_resident) {
        // signal memory: the one allocation made here, released like any other
        unsigned long long *r = nullptr;
        QPSK_HIP_TRY(hipExtMallocWithFlags(reinterpret_cast<void **>(&r), sizeof(*r), hipMallocSignalMemory));
        h->pipe.d_resident.adopt(r, sizeof(*r));
        QPSK_HIP_TRY(hipMemset(h->pipe.d_resident, 0, sizeof(unsigned long long)));
    }
    int rc;
    if (!h->pipe.d_gate) {
        if ((rc = alloc_status(h->pipe.d_gate.alloc(1)))) return rc;
        QPSK_HIP_TRY(hipMemset(h->pipe.d_gate, 0, sizeof(unsigned)));
    }
    if ((rc = alloc_status(h->d_lengths[1].alloc(h->S)))) return rc;
    // the second boundary buffer: MF rows (the FIR of one call writes one while
    // the loop kernel of the previous call reads the other).  No room for it
    // (batches near the 288 GB) -> calls still queue back to back, but each
    // front stage waits for the previous back stage
    const size_t S = static_cast<size_t>(h->S);
    if (!h->d_mf[1]) {
        if (h->d_mf[1].alloc(2 * S * h->mf_stride) != hipSuccess) (void)hipGetLastError();
        else QPSK_HIP_TRY(hipMemset(h->d_mf[1], 0, 2 * S * h->mf_stride * sizeof(float)));
    }
    // as at creation: the memsets above (counter, gate, MF rows) ran on the null
    // stream and are done before any pipelined call uses what they cleared
    QPSK_HIP_TRY(hipStreamSynchronize(nullptr));
    h->pipe.bufs = h->d_mf[1] ? 2 : 1;
    h->pipe.ready = true;
    return QPSK_OK;
}

}  // namespace (pipeline setup)

extern "C" {

int qpsk_abi_version(void) { return QPSK_ABI_VERSION; }

void qpsk_demod_params_init(qpsk_demod_params *p, int32_t sample_rate, int32_t symbol_rate) {
    std::memset(p, 0, sizeof(*p));
    p->sample_rate = sample_rate;
    p->symbol_rate = symbol_rate;
    p->rrc_alpha = 0.9f;                       // QPSKDeModulator.cs:14-18 defaults
    p->rrc_span = 6;
    p->symbol_sync_bandwidth = 0.0001;
    p->costas_loop_bandwidth = 120;
    p->cfo_loop_bandwidth = static_cast<double>(0.0001f);
    p->differential = 1;
    p->enable_fll = 0;
    p->vector_lanes = 8;
    p->device = 0;
    p->max_samples_per_call = 1 << 20;
}

int64_t qpsk_demod_max_symbols(const qpsk_demod *h, int64_t n) {
    if (!h || n <= 0) return 0;
    // every symbol but the first advances the M&M clock by >= sps - 0.1 samples
    const double min_adv = h->lp.sps - 0.1;
    int64_t bound = n;
    if (min_adv > 0.5) {
        const double b = std::ceil(static_cast<double>(n + kCarryMax) / min_adv) + 4.0;
        if (b < static_cast<double>(n)) bound = static_cast<int64_t>(b);
    }
    return bound;
}

int qpsk_demod_create(const qpsk_demod_params *p, int32_t n_streams, qpsk_demod **out) {
    if (!p || !out) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    *out = nullptr;
    if (n_streams <= 0) return fail(QPSK_ERR_ARGUMENT, "n_streams must be positive");
    if (p->max_samples_per_call <= 0) return fail(QPSK_ERR_ARGUMENT, "max_samples_per_call must be positive");
    // the symbol loop counts a chunk's samples in 32-bit integers; a longer
    // call is split into chunks of max_samples_per_call (a C# span holds at
    // most 2^31 - 1 floats anyway)
    if (p->max_samples_per_call > kMaxSamplesPerCall)
        return fail(QPSK_ERR_OUT_OF_RANGE, "max_samples_per_call above 2^30");
    const int W = p->vector_lanes <= 1 ? 1 : p->vector_lanes;
    if (W != 1 && W != 4 && W != 8 && W != 16) return fail(QPSK_ERR_ARGUMENT, "vector_lanes must be 1, 4, 8 or 16");
    if (p->loop_variant < 0 || p->loop_variant > 7) return fail(QPSK_ERR_ARGUMENT, "loop_variant must be 0..7");
    LoopDesign d;
    std::string err;
    int rc = design_loops(p->sample_rate, p->symbol_rate, p->rrc_alpha, p->rrc_span,
                          p->symbol_sync_bandwidth, p->costas_loop_bandwidth, p->cfo_loop_bandwidth,
                          &d, &err);
    if (rc != QPSK_OK) return fail(rc, err);
    if (p->costas_trig != 0 && p->costas_trig != 1)
        return fail(QPSK_ERR_ARGUMENT, "costas_trig must be 0 (portable) or 1 (glibc)");

    // every knob is good: from here on a failure is the device's, and the
    // handle's destructor releases whatever was made before it
    std::unique_ptr<qpsk_demod> h(new qpsk_demod());
    h->p = *p;
    h->S = n_streams;
    h->W = W;
    h->d = std::move(d);
    h->T = static_cast<int>(h->d.rrc_f32.size());
    h->lp.sps = h->d.mm_sps;
    h->lp.kp = h->d.kp;
    h->lp.ki = h->d.ki;
    h->lp.c_alpha = h->d.costas_alpha;
    h->lp.c_beta = h->d.costas_beta;
    h->lp.differential = p->differential ? 1 : 0;
    h->lp.costas_trig = p->costas_trig;
    h->loop_variant = p->loop_variant;   // as requested: the launcher resolves it (resolve_shape, qpsk_loop.hip)
    h->fp.beta = h->d.fll_beta;
    h->fp.alpha = h->d.fll_alpha;
    h->fp.max_freq = h->d.fll_max_freq;
    h->fp.min_freq = -h->d.fll_max_freq;
    h->fp.lanes = h->W;
    for (int k = 0; k < kFllTaps; ++k) {
        const int src = kFllTaps - 1 - k;
        h->fp.lower_rev[2 * k] = h->d.fll_lower_iq[2 * src];
        h->fp.lower_rev[2 * k + 1] = h->d.fll_lower_iq[2 * src + 1];
        h->fp.upper_rev[2 * k] = h->d.fll_upper_iq[2 * src];
        h->fp.upper_rev[2 * k + 1] = h->d.fll_upper_iq[2 * src + 1];
    }
    // the systolic FLL shares the products of both band-edge filters, which needs
    // upper = conj(lower) exactly (Band-Edge Filter.cs:176-178 builds it so)
    h->fp.conj_taps = 1;
    for (int k = 0; k < 2 * kFllTaps; ++k) {
        uint32_t lo, up;
        std::memcpy(&lo, &h->fp.lower_rev[k], 4);
        std::memcpy(&up, &h->fp.upper_rev[k], 4);
        if (up != ((k & 1) ? (lo ^ 0x80000000u) : lo)) h->fp.conj_taps = 0;
    }

    if (hipSetDevice(p->device) != hipSuccess) return fail(QPSK_ERR_DEVICE, "hipSetDevice failed (no GPU?)");
    if (hipDeviceGetAttribute(&h->cus, hipDeviceAttributeMultiprocessorCount, p->device) != hipSuccess)
        h->cus = 0;
    if (hipDeviceGetAttribute(&h->wall_khz, hipDeviceAttributeWallClockRate, p->device) != hipSuccess ||
        h->wall_khz <= 0)
        h->wall_khz = 100000;
    h->pipe.use_gate = qpsk_pipeline_gate_enabled() == 1;
    {
        const char *v = std::getenv("QPSK_GATE_TIMEOUT_MS");
        const long ms = v && *v ? std::strtol(v, nullptr, 10) : 2000;
        h->pipe.gate_cap_ticks = static_cast<unsigned long long>(ms > 0 ? ms : 1) * static_cast<unsigned>(h->wall_khz);
        // test hook, honoured only beside an explicit QPSK_PIPELINE_GATE=1: a
        // stray QPSK_GATE_NO_PUBLISH alone must not make every call wait out the cap
        const char *np = std::getenv("QPSK_GATE_NO_PUBLISH");
        const char *force = std::getenv("QPSK_PIPELINE_GATE");
        const bool forced = force && std::strcmp(force, "1") == 0;
        h->pipe.gate_publish = !(forced && np && *np && std::strcmp(np, "0") != 0);
    }
    if (h->stream.create(hipStreamNonBlocking) != hipSuccess) return fail(QPSK_ERR_DEVICE, "hipStreamCreate failed");

    const int64_t S = n_streams;
    h->n_max = p->max_samples_per_call;
    h->mf_stride = ((kMfPrefix + h->n_max + 2 + 63) / 64) * 64;   // + row slack for the loop loader
    h->syms_cap = qpsk_demod_max_symbols(h.get(), h->n_max);
    h->bits_words = (2 * h->syms_cap + 31) / 32 + 1;
    const int H = h->T - 1;
    hipError_t e;
    if ((e = h->d_hrev.alloc(h->T)) || (e = h->d_hist[0].alloc(2 * S * H)) || (e = h->d_hist[1].alloc(2 * S * H)) ||
        (e = h->d_mf[0].alloc(static_cast<size_t>(2 * S * h->mf_stride))) ||
        (e = h->d_carry.alloc(2 * S * kCarryMax)) || (e = h->d_state.alloc(S)) ||
        (e = h->d_fll_delay.alloc(2 * S * 2 * kFllTaps)) ||
        (e = h->d_bits.alloc(static_cast<size_t>(S * h->bits_words))) || (e = h->d_counts.alloc(2 * S)) ||
        (e = h->d_lengths[0].alloc(S)) ||
        (p->enable_fll && (e = h->d_fll_out.alloc(static_cast<size_t>(2 * S * h->n_max)))) ||
        (p->iq_balance && (e = h->d_iqb.alloc(static_cast<size_t>(2 * S * h->n_max)))))
        return alloc_status(e);
    if (h->h_counts.alloc(2 * S) != hipSuccess || h->h_flags.alloc(1) != hipSuccess)
        return fail(QPSK_ERR_DEVICE, "hipHostMalloc");
    if ((rc = alloc_status(h->d_flags.alloc(2))) || hipMemset(h->d_flags, 0, 2 * sizeof(uint32_t)) != hipSuccess)
        return rc ? rc : fail(QPSK_ERR_DEVICE, "hipMemset");
    std::vector<float> hrev(h->T);
    for (int k = 0; k < h->T; ++k) hrev[k] = h->d.rrc_f32[h->T - 1 - k];
    std::vector<StreamState> st(S, fresh_stream_state());
    if (hipMemcpy(h->d_hrev, hrev.data(), h->T * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->d_state, st.data(), S * sizeof(StreamState), hipMemcpyHostToDevice) != hipSuccess ||
        (H > 0 && hipMemset(h->d_hist[0], 0, 2 * S * H * sizeof(float)) != hipSuccess) ||
        hipMemset(h->d_carry, 0, 2 * S * kCarryMax * sizeof(float)) != hipSuccess ||
        hipMemset(h->d_fll_delay, 0, 2 * S * 2 * kFllTaps * sizeof(float)) != hipSuccess ||
        hipMemset(h->d_mf[0], 0, static_cast<size_t>(2 * S * h->mf_stride) * sizeof(float)) != hipSuccess ||
        // a device memset returns before it is done, and it runs on the null
        // stream, which the handle's non-blocking stream does not wait for:
        // without this the first call's kernels race a multi-GB clear of the
        // MF rows (seen as 4 KB of zero MF samples in the middle of a row)
        hipStreamSynchronize(nullptr) != hipSuccess)
        return fail(QPSK_ERR_DEVICE, "device init failed");
    *out = h.release();
    return QPSK_OK;
}

int qpsk_demod_destroy(qpsk_demod *h) {
    delete h;   // nullptr included; ~qpsk_demod waits for the handle's work
    return QPSK_OK;
}

int qpsk_demod_set_stream(qpsk_demod *h, void *hip_stream) {
    if (!h) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    int rc;
    if ((rc = handle_sync(h))) return rc;
    QPSK_HIP_TRY(h->stream.rebind(hip_stream));
    return QPSK_OK;
}

}  // extern "C"

namespace {

// One validated call of at most max_samples_per_call samples per stream.
int process_one(qpsk_demod *h, const Call &c) {
    int rc;
    const int32_t mem = c.mem;
    const int64_t stride_floats = c.stride_floats;
    const int64_t *lengths = c.lengths;
    const int S = h->S;
    const int64_t n_call = c.n_call;
    hipStream_t st = h->stream;
    QPSK_HIP_TRY(hipSetDevice(h->p.device));
    // pipelined calls issued before this one finish first (they share the state)
    if ((rc = flush_deferred(h))) return rc;
    if (const Event *e = last_async(h)) QPSK_HIP_TRY(e->wait(st));
    unsigned long long *kt = next_kt(h);
    if (mem == QPSK_MEM_HOST && !c.append) QPSK_HIP_TRY(hipMemsetAsync(h->d_flags + 1, 0, sizeof(uint32_t), st));

    // ---- input -----------------------------------------------------------
    InRows in{c.iq, stride_floats / 2, c.fmt, c.scale};   // stride in samples
    if (n_call > 0 && mem == QPSK_MEM_HOST) {
        // staged in the call's own format: a CS16 call uploads 4 bytes a
        // sample, a CS8 / CU8 call 2
        const size_t eb = fmt_elem_bytes(c.fmt);
        const int64_t pitch = stage_pitch(c.fmt, h->n_max);   // samples
        // the last host-memory call has returned, so nothing reads d_in
        if ((rc = alloc_status(h->d_in.grow(static_cast<size_t>(S) * pitch * 2 * eb)))) return rc;
        QPSK_HIP_TRY(hipMemcpy2DAsync(h->d_in, 2 * pitch * eb, c.iq, stride_floats * eb, 2 * n_call * eb, S,
                                      hipMemcpyHostToDevice, st));
        in.x = h->d_in;
        in.stride = pitch;
    }
    const int64_t *d_len = nullptr;
    if (lengths) {
        QPSK_HIP_TRY(hipMemcpyAsync(h->d_lengths[0], lengths, S * sizeof(int64_t), hipMemcpyHostToDevice, st));
        d_len = h->d_lengths[0];
    }

    pre_stages(h, &in, d_len, n_call, h->d_mf[0], st, kt);
    if ((rc = run_fir(h, in, d_len, n_call, h->d_mf[0], st, kt))) return rc;
    return run_loop(h, c, d_len, h->d_mf[0], st, kt);
}

int process_async_one(qpsk_demod *h, const Call &c) {
    int rc;
    const int64_t stride_floats = c.stride_floats;
    const int64_t *lengths = c.lengths;
    QPSK_HIP_TRY(hipSetDevice(h->p.device));
    if ((rc = pipe_setup(h))) return rc;
    const int S = h->S;
    const int64_t n_call = c.n_call;
    const int b = h->pipe.bufs == 2 ? h->pipe.cur : 0;
    h->pipe.cur ^= 1;
    hipStream_t F = h->s_front, B = h->s_back;

    // the front stage starts after the work already on the handle's stream
    // (the producer of iq, earlier synchronous calls) and after the back stage
    // that last used boundary buffer b
    QPSK_HIP_TRY(h->pipe.e_in.record(h->stream));
    QPSK_HIP_TRY(h->pipe.e_in.wait(F));
    const int prev = h->pipe.bufs == 2 ? b : h->pipe.last_back;
    if (prev >= 0) QPSK_HIP_TRY(h->pipe.e_back[prev].wait(F));
    unsigned long long *kt = next_kt(h);
    const int64_t *d_len = nullptr;
    if (lengths) {
        // pinned staging row b is free once the front stage that last read it ran
        QPSK_HIP_TRY(h->pipe.e_front[b].sync());
        std::memcpy(h->pipe.h_len[b], lengths, S * sizeof(int64_t));
        QPSK_HIP_TRY(hipMemcpyAsync(h->d_lengths[b], h->pipe.h_len[b], S * sizeof(int64_t), hipMemcpyHostToDevice, F));
        d_len = h->d_lengths[b];
    }
    InRows in{c.iq, stride_floats / 2, c.fmt, c.scale};
    // MF rows b: the front stage waited above for the back stage that last read
    // them, so a CS16 call's pre-stages may widen into them (float_rows).  The
    // IQ balancer's rows are read only by this call's own front stage (FLL or
    // FIR on F).
    float *mf = h->d_mf[b];
    unsigned long long *resident = h->pipe.use_gate ? h->pipe.d_resident : nullptr;
    pre_stages(h, &in, d_len, n_call, mf, F, kt);
    if (h->p.enable_fll) {
        // FLL on (C5): the FLL keeps every SIMD's VALU busy with one wave each
        // (DESIGN.md 3.3), so a kernel beside it gains what it takes from it,
        // and the launches swing (FIR 48-198, loop 23-218 ms at C5 in round 2).
        // The FIR and the loop kernel overlap well (the FLL-off pipeline).  So:
        //   F: FLL(k) alone -> [B: loop(k-1) after FLL(k)] -> F: FIR(k) once
        //   loop(k-1) holds its CUs (residency gate) -> FIR(k) || loop(k-1)
        // The loop kernel of call k is issued by call k+1 after its FLL, or by
        // a flush (pipeline_wait, a synchronous call, state access, destroy).
        // FLL(k) waited above for loop(k-2), the last reader of MF rows b, and
        // follows FIR(k-1) on F, so it runs alone.
        QPSK_HIP_TRY(h->pipe.e_fll.record(F));
        if (h->pipe.deferred) {
            QPSK_HIP_TRY(h->pipe.e_fll.wait(B));
            h->pipe.deferred = false;
            if ((rc = issue_back(h, h->pipe.dcall, h->pipe.dlen, h->pipe.dbuf, h->pipe.dkt, resident))) return rc;
        }
        if ((rc = gate_wait(h, F))) return rc;
        if ((rc = run_fir(h, in, d_len, n_call, mf, F, kt))) return rc;
        QPSK_HIP_TRY(h->pipe.e_front[b].record(F));
        h->pipe.dcall = c;
        h->pipe.dbuf = b;
        h->pipe.dlen = d_len;
        h->pipe.dkt = kt;
        h->pipe.deferred = true;
        // one MF buffer only: nothing can overlap, issue the back stage now
        return h->pipe.bufs == 2 ? QPSK_OK : flush_deferred(h);
    } else {
        // front = FIR into MF rows b; back = loop.  FIR(k+1) and loop(k) both
        // become ready when a stage of call k-1 or k ends, and whichever is
        // dispatched first takes the CUs: a loop kernel dispatched after the
        // FIR finds no CU with room for its 104-147 KB workgroups and runs
        // after it (measured on MI355X at C3 under rocprofv3: FIR 42 + loop
        // 80 ms a call, against FIR 52 || loop 43 the other way round,
        // profiles/archive/r02_c3_dispatch_race.txt; reproduced by
        // tools/anyorder_probe.hip), and either order then repeats call after
        // call.  So FIR(k+1) waits, on the device, until loop(k)'s workgroups
        // hold their CUs: each adds 1 to the residency counter as it starts,
        // and a wave on the front stream waits for the count (gate_wait_kernel,
        // bounded by a timeout).  The order no longer depends on dispatch
        // timing: the FIR cannot be dispatched before min(grid, CUs) loop
        // workgroups run, and every one of those was dispatched before it.
        if ((rc = gate_wait(h, F))) return rc;
        if ((rc = run_fir(h, in, d_len, n_call, mf, F, kt))) return rc;
        QPSK_HIP_TRY(h->pipe.e_front[b].record(F));
        QPSK_HIP_TRY(h->pipe.e_front[b].wait(B));
    }
    return issue_back(h, c, d_len, b, kt, resident);
}

// The deferred back stage (FLL on) after its own FIR only: nothing follows it.
int flush_deferred(qpsk_demod *h) {
    if (!h->pipe.deferred) return QPSK_OK;
    QPSK_HIP_TRY(hipSetDevice(h->p.device));
    h->pipe.deferred = false;
    QPSK_HIP_TRY(h->pipe.e_front[h->pipe.dbuf].wait(h->s_back));
    return issue_back(h, h->pipe.dcall, h->pipe.dlen, h->pipe.dbuf, h->pipe.dkt, nullptr);
}

// QPSK_STATUS_* raised by the host-memory call that just finished -> status
int host_call_status(qpsk_demod *h) {
    const uint32_t f = *h->h_flags;
    if (f & QPSK_STATUS_CARRY_OVERFLOW)
        return fail(QPSK_ERR_STATE, "symbol-sync queue over 256 retained samples (output capacity hit: sps below ~1?)");
    if (f & QPSK_STATUS_OUTPUT_TRUNCATED) return fail(QPSK_ERR_CAPACITY, "output row truncated");
    if (f & QPSK_STATUS_NONFINITE_TIMING)
        return fail(QPSK_ERR_STATE, "non-finite sample reached the symbol timing loop");
    return QPSK_OK;
}

// A call longer than max_samples_per_call (QPSKDeModulator.cs:345-360 accepts
// any span): consecutive internal chunks of at most n_max samples per stream,
// each chunk's rows appended behind the previous one's, so the caller sees the
// output of one call (the chain carries its state across chunks exactly as
// across calls).  Host-memory outputs are staged in device rows of the whole
// call and copied back once.
int process_chunked(qpsk_demod *h, const Call &c, bool async) {
    const int S = h->S;
    const int64_t N = h->n_max;
    int rc;
    QPSK_HIP_TRY(hipSetDevice(h->p.device));
    if ((rc = alloc_status(h->d_acc.alloc(2 * static_cast<size_t>(S))))) return rc;
    const bool host = c.mem == QPSK_MEM_HOST;   // synchronous calls only: pipelined ones take device memory
    const int64_t bytes_row = (2 * c.max_sym + 7) / 8;
    uint8_t *dbits = c.bits;
    int64_t dbits_stride = c.bits_stride_bytes;
    float *dsyms = c.syms;
    int64_t dsyms_stride = c.syms_stride_floats;
    if (host) {
        if (c.bits) {
            if ((rc = alloc_status(h->d_xbits.grow(static_cast<size_t>(S) * bytes_row)))) return rc;
            dbits = h->d_xbits;
            dbits_stride = bytes_row;
        }
        if (c.syms) {
            const size_t need = static_cast<size_t>(S) * 2 * c.max_sym * sizeof(float);
            if ((rc = alloc_status(h->d_xsyms.grow(need)))) return rc;
            dsyms = h->d_xsyms;
            dsyms_stride = 2 * c.max_sym;
        }
        QPSK_HIP_TRY(hipMemsetAsync(h->d_flags + 1, 0, sizeof(uint32_t), h->stream));
    }
    const int64_t K = (c.n_call + N - 1) / N;
    std::vector<int64_t> len_k(c.lengths ? S : 0);
    for (int64_t k = 0; k < K; ++k) {
        const int64_t off = k * N;
        Call sub = c;
        sub.iq = static_cast<const char *>(c.iq) + 2 * off * static_cast<int64_t>(fmt_elem_bytes(c.fmt));
        if (c.lengths) {
            int64_t m = 0;
            for (int s = 0; s < S; ++s) {
                len_k[s] = std::min(N, std::max<int64_t>(0, c.lengths[s] - off));
                m = std::max(m, len_k[s]);
            }
            sub.lengths = len_k.data();
            sub.n_samples = 0;
            sub.n_call = m;
        } else {
            sub.n_samples = std::min(N, c.n_samples - off);
            sub.n_call = sub.n_samples;
        }
        sub.max_sym = qpsk_demod_max_symbols(h, sub.n_call);
        sub.append = true;
        sub.first = k == 0;
        sub.last = k == K - 1;
        sub.dst_bits = dbits;
        sub.dst_bits_stride = dbits_stride;
        sub.dst_syms = dsyms;
        sub.dst_syms_stride = dsyms_stride;
        sub.dst_n_bits = host ? nullptr : c.n_bits;
        sub.dst_n_syms = host ? nullptr : c.n_syms;
        if ((rc = async ? process_async_one(h, sub) : process_one(h, sub))) {
            // a chunk after the first failed: the chunks that ran left
            // StreamState.tofs (the queue offset inside this call) non-zero,
            // which only the last chunk resets; clear it so the next call's
            // timing runs from its own queue start (best effort after a HIP error)
            // The memset goes behind every kernel that may still write tofs:
            // the pipelined chunks' loop kernels run on the back stream, and
            // with the FLL the newest one is only issued by flush_deferred.
            if (k > 0) {
                (void)flush_deferred(h);
                if (const Event *e = last_async(h)) (void)e->wait(h->stream);
                (void)hipMemset2DAsync(reinterpret_cast<char *>(h->d_state.get()) + offsetof(StreamState, tofs),
                                       sizeof(StreamState), 0, sizeof(int64_t), S, h->stream);
            }
            return rc;
        }
    }
    if (!host) return QPSK_OK;
    hipStream_t st = h->stream;
    if (c.bits && bytes_row > 0)
        QPSK_HIP_TRY(hipMemcpy2DAsync(c.bits, c.bits_stride_bytes, dbits, dbits_stride, bytes_row, S,
                                      hipMemcpyDeviceToHost, st));
    if (c.syms && c.max_sym > 0)
        QPSK_HIP_TRY(hipMemcpy2DAsync(c.syms, c.syms_stride_floats * sizeof(float), dsyms,
                                      dsyms_stride * sizeof(float), 2 * c.max_sym * sizeof(float), S,
                                      hipMemcpyDeviceToHost, st));
    if ((rc = host_epilogue(h, c, h->d_acc, st))) return rc;
    return host_call_status(h);
}

// Every qpsk_demod_process* entry point: check, then the path the call's
// length and kind ask for.
int submit(qpsk_demod *h, Call &c, bool pipelined) {
    if (!h) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    if (!fmt_known(c.fmt)) return fail(QPSK_ERR_ARGUMENT, "unknown sample format");
    c.scale = h->in_scale[c.fmt];   // queued calls keep the scale they were issued with
    int rc;
    if ((rc = check_call(h, h->S, c))) return rc;
    if (c.syms && (rc = ensure_syms(h))) return rc;
    if (c.n_call > h->n_max) return process_chunked(h, c, pipelined);
    if (pipelined) return process_async_one(h, c);
    if ((rc = process_one(h, c))) return rc;
    return c.mem == QPSK_MEM_HOST ? host_call_status(h) : QPSK_OK;
}

}  // namespace (calls)

extern "C" {

int qpsk_demod_process(qpsk_demod *h, int32_t mode, const float *iq, int64_t stride_floats,
                       int64_t n_samples, const int64_t *lengths, int32_t mem, uint8_t *bits,
                       int64_t bits_stride_bytes, int64_t *n_bits, float *syms,
                       int64_t syms_stride_floats, int64_t *n_syms) {
    Call c{{mode, iq, stride_floats, n_samples, lengths, mem, bits, bits_stride_bytes, n_bits, syms,
            syms_stride_floats, n_syms}};
    return submit(h, c, false);
}

int qpsk_demod_process_async(qpsk_demod *h, int32_t mode, const float *iq, int64_t stride_floats,
                             int64_t n_samples, const int64_t *lengths, uint8_t *bits,
                             int64_t bits_stride_bytes, int64_t *n_bits, float *syms,
                             int64_t syms_stride_floats, int64_t *n_syms) {
    Call c{{mode, iq, stride_floats, n_samples, lengths, QPSK_MEM_DEVICE, bits, bits_stride_bytes, n_bits, syms,
            syms_stride_floats, n_syms}};
    return submit(h, c, true);
}

int qpsk_demod_set_input_scale(qpsk_demod *h, int32_t fmt, float scale) {
    if (!h) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    if (!fmt_known(fmt)) return fail(QPSK_ERR_ARGUMENT, "unknown sample format");
    if (fmt == QPSK_FMT_CF32) return fail(QPSK_ERR_ARGUMENT, "CF32 input has no scale");
    if (!std::isfinite(scale) || !(scale > 0.0f))
        return fail(QPSK_ERR_OUT_OF_RANGE, std::string("the ") + fmt_name(fmt) + " scale must be finite and > 0");
    h->in_scale[fmt] = scale;   // calls issued from now on; queued ones carry their own
    return QPSK_OK;
}

int qpsk_demod_get_input_scale(const qpsk_demod *h, int32_t fmt, float *scale) {
    if (!h || !scale) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    if (!fmt_known(fmt)) return fail(QPSK_ERR_ARGUMENT, "unknown sample format");
    if (fmt == QPSK_FMT_CF32) return fail(QPSK_ERR_ARGUMENT, "CF32 input has no scale");
    *scale = h->in_scale[fmt];
    return QPSK_OK;
}

int qpsk_demod_set_cs16_scale(qpsk_demod *h, float scale) {
    return qpsk_demod_set_input_scale(h, QPSK_FMT_CS16, scale);
}

int qpsk_demod_get_cs16_scale(const qpsk_demod *h, float *scale) {
    return qpsk_demod_get_input_scale(h, QPSK_FMT_CS16, scale);
}

int qpsk_fmt_sample_bytes(int32_t fmt) {
    return fmt_known(fmt) ? static_cast<int>(2 * fmt_elem_bytes(fmt)) : QPSK_ERR_ARGUMENT;
}

int qpsk_demod_process_fmt(qpsk_demod *h, int32_t fmt, int32_t mode, const void *iq, int64_t stride_elems,
                           int64_t n_samples, const int64_t *lengths, int32_t mem, uint8_t *bits,
                           int64_t bits_stride_bytes, int64_t *n_bits, float *syms,
                           int64_t syms_stride_floats, int64_t *n_syms) {
    Call c{{mode, iq, stride_elems, n_samples, lengths, mem, bits, bits_stride_bytes, n_bits, syms,
            syms_stride_floats, n_syms, fmt}};
    return submit(h, c, false);
}

int qpsk_demod_process_async_fmt(qpsk_demod *h, int32_t fmt, int32_t mode, const void *iq, int64_t stride_elems,
                                 int64_t n_samples, const int64_t *lengths, uint8_t *bits,
                                 int64_t bits_stride_bytes, int64_t *n_bits, float *syms,
                                 int64_t syms_stride_floats, int64_t *n_syms) {
    Call c{{mode, iq, stride_elems, n_samples, lengths, QPSK_MEM_DEVICE, bits, bits_stride_bytes, n_bits, syms,
            syms_stride_floats, n_syms, fmt}};
    return submit(h, c, true);
}

int qpsk_demod_process_cs16(qpsk_demod *h, int32_t mode, const int16_t *iq, int64_t stride_i16,
                            int64_t n_samples, const int64_t *lengths, int32_t mem, uint8_t *bits,
                            int64_t bits_stride_bytes, int64_t *n_bits, float *syms,
                            int64_t syms_stride_floats, int64_t *n_syms) {
    Call c{{mode, iq, stride_i16, n_samples, lengths, mem, bits, bits_stride_bytes, n_bits, syms,
            syms_stride_floats, n_syms, QPSK_FMT_CS16}};
    return submit(h, c, false);
}

int qpsk_demod_process_async_cs16(qpsk_demod *h, int32_t mode, const int16_t *iq, int64_t stride_i16,
                                  int64_t n_samples, const int64_t *lengths, uint8_t *bits,
                                  int64_t bits_stride_bytes, int64_t *n_bits, float *syms,
                                  int64_t syms_stride_floats, int64_t *n_syms) {
    Call c{{mode, iq, stride_i16, n_samples, lengths, QPSK_MEM_DEVICE, bits, bits_stride_bytes, n_bits, syms,
            syms_stride_floats, n_syms, QPSK_FMT_CS16}};
    return submit(h, c, true);
}

int qpsk_demod_last_mf(qpsk_demod *h, float *out, int64_t stride_floats, int64_t n_samples, int32_t mem) {
    if (!h || !out) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    if (n_samples < 0 || n_samples > h->n_max || stride_floats < 2 * n_samples)
        return fail(QPSK_ERR_ARGUMENT, "n_samples / stride_floats out of range");
    if (mem != QPSK_MEM_HOST && mem != QPSK_MEM_DEVICE) return fail(QPSK_ERR_ARGUMENT, "unknown mem");
    QPSK_HIP_TRY(hipSetDevice(h->p.device));
    QPSK_HIP_TRY(hipStreamSynchronize(h->stream));
    if (n_samples == 0) return QPSK_OK;
    QPSK_HIP_TRY(hipMemcpy2D(out, stride_floats * sizeof(float), h->d_mf[0] + 2 * kMfPrefix,
                             2 * h->mf_stride * sizeof(float), 2 * n_samples * sizeof(float), h->S,
                             mem == QPSK_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice));
    return QPSK_OK;
}

int qpsk_demod_status(qpsk_demod *h, uint32_t *flags) {
    if (!h || !flags) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    int rc;
    if ((rc = handle_sync(h))) return rc;
    QPSK_HIP_TRY(hipMemcpy(h->h_flags, h->d_flags, sizeof(uint32_t), hipMemcpyDeviceToHost));
    QPSK_HIP_TRY(hipMemset(h->d_flags, 0, sizeof(uint32_t)));
    *flags = *h->h_flags | h->status_host;
    h->status_host = 0;
    return QPSK_OK;
}

int qpsk_demod_pipeline_wait(qpsk_demod *h, void *hip_stream) {
    if (!h) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    int rc;
    if ((rc = flush_deferred(h))) return rc;
    const Event *e = last_async(h);
    if (!e) return QPSK_OK;
    if (hip_stream) QPSK_HIP_TRY(e->wait(static_cast<hipStream_t>(hip_stream)));
    else QPSK_HIP_TRY(e->sync());
    return QPSK_OK;
}

int qpsk_demod_gate_timeouts(qpsk_demod *h, uint64_t *count) {
    if (!h || !count) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    *count = 0;
    if (!h->pipe.d_gate) return QPSK_OK;
    int rc;
    if ((rc = drain_async(h))) return rc;
    QPSK_HIP_TRY(hipSetDevice(h->p.device));
    unsigned v = 0;
    QPSK_HIP_TRY(hipMemcpy(&v, h->pipe.d_gate, sizeof(unsigned), hipMemcpyDeviceToHost));
    *count = v;
    return QPSK_OK;
}

int qpsk_demod_pipeline_depth(const qpsk_demod *h) {
    if (!h) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    return h->pipe.ready ? h->pipe.bufs : 0;
}

int qpsk_demod_rrc_taps(const qpsk_demod *h, float *taps, int32_t cap) {
    if (!h || !taps) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    if (cap < h->T) return fail(QPSK_ERR_ARGUMENT, "cap too small");
    std::memcpy(taps, h->d.rrc_f32.data(), h->T * sizeof(float));
    return h->T;
}

int qpsk_demod_gains(const qpsk_demod *h, double *mm_sps, double *kp, double *ki,
                     double *costas_alpha, double *costas_beta) {
    if (!h) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    if (mm_sps) *mm_sps = h->d.mm_sps;
    if (kp) *kp = h->d.kp;
    if (ki) *ki = h->d.ki;
    if (costas_alpha) *costas_alpha = h->d.costas_alpha;
    if (costas_beta) *costas_beta = h->d.costas_beta;
    return QPSK_OK;
}

int qpsk_demod_fll_taps(const qpsk_demod *h, float *lower_iq, float *upper_iq, int32_t cap_floats) {
    if (!h || !lower_iq || !upper_iq) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    const int n = 2 * kFllTaps;
    if (cap_floats < n) return fail(QPSK_ERR_ARGUMENT, "cap too small");
    std::memcpy(lower_iq, h->d.fll_lower_iq.data(), n * sizeof(float));
    std::memcpy(upper_iq, h->d.fll_upper_iq.data(), n * sizeof(float));
    return n;
}

// Residency gate default (process_async_one).  The wait is bounded
// (gate_wait_kernel), but where dispatch is serialised the loop kernel it
// waits for starts only after the waiting FIR, so every wait would run to its
// cap: the gate is off there.
int qpsk_pipeline_gate_enabled(void) {
    auto env = [](const char *name) -> const char * {
        const char *v = std::getenv(name);
        return v && *v ? v : nullptr;
    };
    auto is = [&](const char *name, const char *val) {
        const char *v = env(name);
        return v && std::strcmp(v, val) == 0;
    };
    auto nonzero = [&](const char *name) {
        const char *v = env(name);
        return v && std::strcmp(v, "0") != 0;
    };
    if (is("QPSK_PIPELINE_GATE", "0")) return 0;             // explicit opt-out
    if (is("QPSK_PIPELINE_GATE", "1")) return 1;             // explicit opt-in wins over the rest
    if (nonzero("AMD_SERIALIZE_KERNEL")) return 0;           // HIP runtime: serialised kernel launches
    if (nonzero("AMD_SERIALIZE_COPY")) return 0;             // ... and copies
    if (nonzero("HIP_LAUNCH_BLOCKING")) return 0;            // every launch waits for the previous
    if (nonzero("CUDA_LAUNCH_BLOCKING")) return 0;           // the alias HIP also honours
    if (is("ROCPROF_COUNTER_COLLECTION", "1")) return 0;     // rocprofv3 --pmc: per-dispatch serialisation
    if (nonzero("ROCPROFILER_KERNEL_SERIALIZATION")) return 0;
    if (nonzero("HSA_ENABLE_DEBUG")) return 0;               // debugger-attached runs
    return 1;
}

}  // extern "C"
