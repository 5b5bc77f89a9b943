// qpsk_handle.h -- the demodulator handle (struct qpsk_demod) and what the
// files that work on one share: qpsk_runtime.hip (create, destroy, the call
// paths), qpsk_probe.hip, qpsk_link_stats.hip, qpsk_stream_state.hip and
// qpsk_rx.hip.  Members are read and written directly; the nested structs only
// group them by concern.  Private, HIP-only (plain C++ such as qpsk_group.cpp
// goes through qpsk_internal.h).
//
// Device layout (HBM, stream-major so every stage reads/writes each stream's
// time axis contiguously):
//   in      [S][n_max]              float2  staging for host input (CS16 calls:
//                                           int16 pairs, rows of n_max rounded up to
//                                           4 samples so they take 16-B loads;
//                                           CS8 / CU8 calls: byte pairs, rows
//                                           rounded up to 8 samples)
//   fll_out [S][n_max]              float2  (FLL mode)
//   hist    2 x [S][T-1]            float2  FIR delay line (ping-pong)
//   mf      [2][S][256 + n_max]     float2  matched-filter output; the 256-slot
//                                           prefix receives the M&M carry (the
//                                           2nd only when pipelined)
//   carry   [S][256]                float2  M&M retained samples
//   state   [S]                     StreamState
//   bits    [S][words]              uint32  MSB-first packed bits
//   syms    [S][syms_cap]           float2  rotated symbols (on request)
//   link    [S]                     LinkAcc link statistics' running sums (once enabled)
//   rows    blob of n streams + [n] int32   staging of selected streams' rows (qpsk_stream_state.hip)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "qpsk_demod.h"
#include "qpsk_design.h"
#include "qpsk_device.h"
#include "qpsk_internal.h"
#include "qpsk_kernels.h"
#include "qpsk_quantise.h"

namespace qpsk {

// launch-timestamp slots of one timed call, a pair per kernel: its (start, end)
// span, then its clock sample (shader ticks, wall ticks); each list in the
// order FLL, FIR, loop kernel.  qpsk_demod_enable_timing records the first
// kKtCalls calls
constexpr int kKtSpan[3] = {0, 2, 4};
constexpr int kKtClk[3] = {8, 6, 10};
constexpr int kKtFll = 0, kKtFir = 1, kKtLoop = 2;
constexpr int kKtSpanSlots = 6;   // the slots below this hold spans
constexpr int kKtPerCall = 12;
constexpr int kKtCalls = 4096;
constexpr int64_t kMaxSamplesPerCall = int64_t(1) << 30;
// the symbol loop keeps sample indices of one call in 32-bit integers
constexpr int64_t kMaxCallSamples = (int64_t(1) << 31) - 129;

struct Call : CallArgs {
    // internal chunk of a longer call: outputs appended to dst_* at the running
    // offsets d_acc (first chunk: from 0), totals to n_bits / n_syms after the last
    bool append = false, first = false, last = false;
    uint8_t *dst_bits = nullptr;
    int64_t dst_bits_stride = 0;
    float *dst_syms = nullptr;
    int64_t dst_syms_stride = 0;
    int64_t *dst_n_bits = nullptr;   // device; written after the last chunk
    int64_t *dst_n_syms = nullptr;
    // an integer-format call: the handle's scale of that format when the call was issued
    float scale = 0.0f;
};

// The first stage's input rows: the caller's (or the staged) rows in the
// call's own format, until a pre-stage has rewritten them as float rows.
struct InRows {
    const void *x;
    int64_t stride;   // samples
    int32_t fmt;
    float scale;
};

// A fresh instance's record: zero delay lines and loops (FIRFilter.cs:50-51),
// M&M baseIndex = 1 (MuellerMuller.cs:44), everything else zero.
inline StreamState fresh_stream_state() {
    StreamState s;
    std::memset(&s, 0, sizeof(s));
    s.base = 1;
    return s;
}

}  // namespace qpsk

// Every buffer, event and stream is a member that releases itself
// (qpsk_device.h), and members go in reverse order of declaration.  The one
// rule of the layout: stream, s_front and s_back stand in front of every
// buffer and event, whichever nested struct those live in, so what a stream's
// work used is released first and the streams last.  ~qpsk_demod makes the
// handle's device current, drains the pipelined calls and synchronises before
// any member goes.
struct qpsk_demod {
    // ---- shape and design --------------------------------------------------
    qpsk_demod_params p{};
    int S = 0;
    int T = 0;
    int W = 8;
    qpsk::LoopDesign d;
    qpsk::LoopParams lp{};
    int loop_variant = 0;
    qpsk::FllParams fp{};
    int64_t n_max = 0;
    int64_t mf_stride = 0;       // float2
    int64_t bits_words = 0;      // per stream
    int64_t syms_cap = 0;        // per stream
    int cus = 0;
    int wall_khz = 100000;
    // per input format (CF32 has none): CS16 (float)int16 * scale, SoapySDR's
    // CS16 -> CF32 convention; CS8 / CU8 full scale 128 (S8toF32, U8toS8)
    float in_scale[qpsk::kFmts] = {0.0f, 1.0f / 32768, 1.0f / 128, 1.0f / 128};

    // ---- the streams, in front of every buffer and event (above) -----------
    qpsk::Stream stream;             // the handle's own or its caller's (qpsk_demod_set_stream)
    qpsk::Stream s_front, s_back;    // pipelined calls; s_front is nullptr before the first one

    // ---- the chain's buffers, counts and flags -----------------------------
    qpsk::DevBuf<float> d_hrev;
    qpsk::DevBuf<char> d_in;               // host-input staging, in the call's format
    qpsk::DevBuf<float> d_fll_out;         // [S][n_max] float2, FLL output (enable_fll only)
    qpsk::DevBuf<float> d_iqb;             // [S][n_max] float2, IQ_Balancer output (iq_balance only)
    qpsk::DevBuf<float> d_hist[2];
    int hist_cur = 0;
    qpsk::DevBuf<float> d_mf[2];
    qpsk::DevBuf<float> d_carry;
    qpsk::DevBuf<qpsk::StreamState> d_state;
    qpsk::DevBuf<float> d_fll_delay;
    qpsk::DevBuf<uint32_t> d_bits;
    qpsk::DevBuf<float> d_syms;
    qpsk::DevBuf<int64_t> d_counts;        // [2][S]: n_bits, n_syms
    qpsk::DevBuf<int64_t> d_lengths[2];
    qpsk::PinnedBuf<int64_t> h_counts;
    // status flags (QPSK_STATUS_*): [0] = raised by device-memory calls since the
    // last qpsk_demod_status, [1] = raised by the current host-memory call
    qpsk::DevBuf<uint32_t> d_flags;
    qpsk::PinnedBuf<uint32_t> h_flags;
    uint32_t status_host = 0;        // raised by host-memory calls since the last status
    // chunked calls (longer than max_samples_per_call): running per-stream
    // output offsets [2][S] and, for host-memory calls, device staging of the
    // whole call's output rows
    qpsk::DevBuf<int64_t> d_acc;
    qpsk::DevBuf<uint8_t> d_xbits;
    qpsk::DevBuf<float> d_xsyms;
    // rows of selected streams (qpsk_stream_state.hip): the packed sub-blob and
    // the index list behind it, grown on demand
    qpsk::DevBuf<char> d_rows;

    // ---- pipelined calls (qpsk_demod_process_async, qpsk_runtime.hip) ------
    struct Pipe {
        bool ready = false;
        int bufs = 0;                    // 2 = double-buffered stage boundary, 1 = no room for it
        int cur = 0;
        int last_back = -1;              // boundary buffer of the newest back stage, -1 = none
        qpsk::Event e_in;
        qpsk::Event e_front[2], e_back[2];
        qpsk::PinnedBuf<int64_t> h_len[2];     // staging of per-call lengths
        // FLL on: the back stage (loop kernel) of the newest call is issued by the
        // next call, after that call's FLL, or by a flush (see process_async_one)
        qpsk::Event e_fll;
        bool deferred = false;
        qpsk::Call dcall{};
        int dbuf = 0;
        const int64_t *dlen = nullptr;
        unsigned long long *dkt = nullptr;
        // FLL off: residency counter (signal memory) the loop kernel's workgroups
        // increment as they start; the next call's FIR waits for it to reach
        // resident_gate (see process_async_one)
        qpsk::DevBuf<unsigned long long> d_resident;
        uint64_t resident_issued = 0;    // workgroups of every gated loop launch so far
        uint64_t resident_gate = 0;      // what the newest gated loop launch brings it to, at least
        bool gate_pending = false;       // the next FIR has a loop launch to wait for
        // off under a profiler's counter collection (rocprofv3 --pmc serialises
        // every dispatch, so the wait would run to its cap on every call) or with
        // QPSK_PIPELINE_GATE=0
        bool use_gate = true;
        // the wait is bounded (gate_wait_kernel): at most gate_cap_ticks of the
        // wall clock (QPSK_GATE_TIMEOUT_MS, default 2000 ms), counted in d_gate[0]
        // when it runs out; gate_publish = false (QPSK_GATE_NO_PUBLISH=1 together
        // with QPSK_PIPELINE_GATE=1, tests only) keeps the loop workgroups from
        // counting, so every wait runs out
        qpsk::DevBuf<unsigned> d_gate;
        unsigned long long gate_cap_ticks = 0;
        bool gate_publish = true;
    } pipe;

    // ---- timing and FIR-phase probes (qpsk_probe.hip) ----------------------
    struct Probe {
        bool timing = false;
        // launch timestamps of the timed calls ([call][kKtPerCall] wall-clock ticks,
        // written by the kernels themselves: qpsk_kernels.h kt_start / kt_end)
        qpsk::DevBuf<unsigned long long> d_kt;
        int kt_used = 0;
        // FIR phase sample (qpsk_demod_enable_fir_phases): per-phase cycle sums
        // [2][8] and the map of CUs a loop workgroup holds [kCuKeys]
        bool fir_phases = false;
        qpsk::DevBuf<unsigned long long> d_phases;
        qpsk::DevBuf<unsigned> d_cu_map;
    } probe;

    // ---- link statistics (qpsk_link_stats.hip) ------------------------------
    // the per-stream running sums the loop kernel's decode wave continues while
    // on, and the rows a host-memory read is gathered into (both made by the
    // first enable)
    struct Link {
        bool on = false;
        qpsk::DevBuf<qpsk::LinkAcc> d_link;
        qpsk::DevBuf<qpsk_link_stats> d_link_rows;
    } link;

    ~qpsk_demod();
};
