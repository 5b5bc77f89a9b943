// qpsk_stream_state.hip -- read and write a handle's state: the whole batch as
// one blob (qpsk_demod_get_state / _set_state, qpsk_state_blob.h), and reset,
// read and write the state of selected streams of it (include/qpsk_demod.h
// "Selected streams").
//
// A reference receiver is constructed and dropped on its own
// (QPSKDeModulator.cs:11-56).  A handle's rows are made together; these calls
// give the rows a caller names a lifetime of their own:
//
//     qpsk_demod_reset_streams       row s <- new QPSKDeModulator(...)
//     qpsk_demod_get_streams_state   rows -> a blob of n streams (host)
//     qpsk_demod_set_streams_state   a blob of n streams (host) -> rows
//
// One stream's state is a row in each of four arrays: its StreamState record,
// its M&M carry, its FIR history (the current one of the ping-pong pair) and
// its FLL delay line.  stream_rows_kernel moves those rows between the arrays
// and one packed staging buffer laid out as the blob of the n listed streams
// (qpsk_state_blob.h), index list behind it, so one copy each way crosses the
// bus.  The host side of the same operation, qpsk_state_blob_select / _merge
// (qpsk_state_blob.cpp), is what the tests hold this path to.
//
// Every call checks its arguments on the host, then waits for every queued
// call (handle_sync): StreamState mixes fields the front stage writes (FLL, IQ
// balancer) with fields the back stage writes, so a row written between
// queued calls would race both.  A rejected call neither waits nor changes
// anything.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "qpsk_handle.h"
#include "qpsk_state_blob.h"

using namespace qpsk;

namespace {

constexpr int kRowsThreads = 256;
constexpr int kRecordWords = static_cast<int>(sizeof(StreamState) / 8);
constexpr int kLinkWords = static_cast<int>(sizeof(LinkAcc) / 8);
static_assert(sizeof(LinkAcc) % 8 == 0, "the link sums are cleared in 8-byte words");
static_assert(sizeof(StateHeader) % 8 == 0, "the staged sections start on 8-byte words");

enum RowsMode { kGather = 0, kScatter = 1, kReset = 2 };

// The four per-stream arrays behind a blob's header, in the blob's order:
// records, M&M carries, FIR histories (the current one of the ping-pong pair,
// good until the next call is issued) and FLL delay lines, with the 8-byte
// words of one stream's row in each.
struct Sections {
    void *rows[kStateSections];
    int64_t words[kStateSections];
};
Sections sections(qpsk_demod *h) {
    Sections t{{h->d_state.get(), h->d_carry.get(), h->d_hist[h->hist_cur].get(), h->d_fll_delay.get()}, {}};
    state_row_words(h->T, t.words);
    return t;
}

struct RowsArgs {
    uint2 *rows[kStateSections];        // the handle's arrays: records, carries, histories, delay lines
    int64_t words[kStateSections];      // 8-byte words of one stream's row in each
    int64_t staged[kStateSections];     // word offset of each section in the staging buffer (list entry 0)
    uint2 *staging;                     // the packed sub-blob (gather, scatter)
    const int32_t *list;                // [n] stream indices, every one checked on the host
    uint2 *link;                        // [S] LinkAcc or nullptr (reset)
    uint2 fresh[kRecordWords];          // the record qpsk_demod_create writes (reset)
};

// One workgroup per list entry: that stream's four rows, 8-byte words as
// integer bit patterns (a NaN's payload and -0 pass unchanged), consecutive
// lanes on consecutive words.  Not 16-byte words: a history row is 8 (T - 1)
// bytes, so with an even tap count every other row starts 8 bytes off.
template <int MODE>
__global__ __launch_bounds__(kRowsThreads) void stream_rows_kernel(const RowsArgs a) {
    const int64_t entry = blockIdx.x;
    const int64_t s = a.list[entry];
    const int lane = threadIdx.x;
#pragma unroll
    for (int k = 0; k < kStateSections; ++k) {
        const int64_t w = a.words[k];
        uint2 *row = a.rows[k] + s * w;
        if (MODE == kReset) {
            for (int64_t i = lane; i < w; i += kRowsThreads) row[i] = k == 0 ? a.fresh[i] : make_uint2(0u, 0u);
        } else {
            uint2 *st = a.staging + a.staged[k] + entry * w;
            for (int64_t i = lane; i < w; i += kRowsThreads) {
                if (MODE == kGather) st[i] = row[i];
                else row[i] = st[i];
            }
        }
    }
    if (MODE == kReset && a.link && lane < kLinkWords) a.link[s * kLinkWords + lane] = make_uint2(0u, 0u);
}

// The listed rows in one launch on the handle's stream, which the call then
// waits for.  host: the caller's sub-blob (read by scatter, written by gather).
int move_rows(qpsk_demod *h, int mode, const int32_t *streams, int32_t n, void *host, int64_t bytes) {
    int rc;
    if ((rc = handle_sync(h))) return rc;   // also makes the handle's device current
    const Sections sec = sections(h);
    const size_t blob = mode == kReset ? 0 : static_cast<size_t>(bytes);
    const size_t list_bytes = static_cast<size_t>(n) * sizeof(int32_t);
    // what the staging buffer held is dropped: every user of it has returned
    if ((rc = alloc_status(h->d_rows.grow(blob + list_bytes)))) return rc;
    char *stage = h->d_rows;

    RowsArgs a{};
    int64_t at = sizeof(StateHeader) / 8;
    for (int k = 0; k < kStateSections; ++k) {
        a.rows[k] = static_cast<uint2 *>(sec.rows[k]);
        a.words[k] = sec.words[k];
        a.staged[k] = at;
        at += a.words[k] * n;
    }
    a.staging = reinterpret_cast<uint2 *>(stage);
    a.list = reinterpret_cast<const int32_t *>(stage + blob);   // blob bytes are a multiple of 8
    a.link = reinterpret_cast<uint2 *>(h->link.d_link.get());   // nullptr until first enabled
    const StreamState fresh = fresh_stream_state();
    std::memcpy(a.fresh, &fresh, sizeof(fresh));

    hipStream_t st = h->stream;
    QPSK_HIP_TRY(hipMemcpyAsync(stage + blob, streams, list_bytes, hipMemcpyHostToDevice, st));
    if (mode == kScatter) QPSK_HIP_TRY(hipMemcpyAsync(stage, host, blob, hipMemcpyHostToDevice, st));
    const dim3 grid(static_cast<unsigned>(n)), block(kRowsThreads);
    if (mode == kGather) hipLaunchKernelGGL(stream_rows_kernel<kGather>, grid, block, 0, st, a);
    else if (mode == kScatter) hipLaunchKernelGGL(stream_rows_kernel<kScatter>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(stream_rows_kernel<kReset>, grid, block, 0, st, a);
    QPSK_HIP_TRY(hipGetLastError());
    if (mode == kGather) QPSK_HIP_TRY(hipMemcpyAsync(host, stage, blob, hipMemcpyDeviceToHost, st));
    QPSK_HIP_TRY(hipStreamSynchronize(st));
    if (mode == kGather) {
        const StateHeader hd = state_header(n, h->T);
        std::memcpy(host, &hd, sizeof(hd));
    }
    return QPSK_OK;
}

// The four sections of a whole-batch blob behind its header, each against the
// array of the handle that holds it.
int copy_state(qpsk_demod *h, char *blob, hipMemcpyKind kind) {
    const Sections sec = sections(h);
    char *p = blob + sizeof(StateHeader);
    for (int k = 0; k < kStateSections; ++k) {
        const size_t n = static_cast<size_t>(h->S) * 8 * sec.words[k];
        const bool out = kind == hipMemcpyDeviceToHost;
        if (n) QPSK_HIP_TRY(hipMemcpy(out ? p : sec.rows[k], out ? sec.rows[k] : p, n, kind));
        p += n;
    }
    return QPSK_OK;
}

}  // namespace

extern "C" {

// State blob (qpsk_state_blob.h): set_state rejects, before it touches the
// handle, any blob whose length or header does not match this handle or whose
// records hold a value a kernel would misuse as an address
// (qpsk_state_blob_check, qpsk_state_blob.cpp).
int64_t qpsk_demod_state_bytes(const qpsk_demod *h) {
    if (!h) return 0;
    return state_blob_bytes(h->S, h->T);
}

int qpsk_demod_get_state(qpsk_demod *h, void *host_buf, int64_t buf_bytes) {
    if (!h || !host_buf) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    if (buf_bytes < qpsk_demod_state_bytes(h)) return fail(QPSK_ERR_ARGUMENT, "state buffer too small");
    int rc;
    if ((rc = handle_sync(h))) return rc;
    const StateHeader hd = state_header(h->S, h->T);
    std::memcpy(host_buf, &hd, sizeof(hd));
    return copy_state(h, static_cast<char *>(host_buf), hipMemcpyDeviceToHost);
}

int qpsk_demod_set_state(qpsk_demod *h, const void *host_buf, int64_t buf_bytes) {
    if (!h || !host_buf) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    int rc;
    // on the host, before the handle is waited for or a byte is copied: a
    // rejected blob leaves the handle as it was
    if ((rc = qpsk_state_blob_check(&h->p, h->S, host_buf, buf_bytes))) return rc;
    if ((rc = handle_sync(h))) return rc;
    return copy_state(h, static_cast<char *>(const_cast<void *>(host_buf)), hipMemcpyHostToDevice);
}

int qpsk_demod_reset_streams(qpsk_demod *h, const int32_t *streams, int32_t n) {
    if (!h) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    if (n == 0) return QPSK_OK;
    int rc;
    if ((rc = stream_list_check(h->S, streams, n))) return rc;
    return move_rows(h, kReset, streams, n, nullptr, 0);
}

int64_t qpsk_demod_streams_state_bytes(const qpsk_demod *h, int32_t n) {
    if (!h || n < 1 || n > h->S) return 0;
    return state_blob_bytes(n, h->T);
}

int qpsk_demod_get_streams_state(qpsk_demod *h, const int32_t *streams, int32_t n, void *host_buf,
                                 int64_t buf_bytes) {
    if (!h || !streams || !host_buf) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    int rc;
    if ((rc = stream_list_check(h->S, streams, n))) return rc;
    const int64_t want = state_blob_bytes(n, h->T);
    if (buf_bytes != want)
        return fail(QPSK_ERR_ARGUMENT, "the state buffer holds " + std::to_string(buf_bytes) + " bytes, " +
                                           std::to_string(n) + " streams take " + std::to_string(want));
    return move_rows(h, kGather, streams, n, host_buf, buf_bytes);
}

int qpsk_demod_set_streams_state(qpsk_demod *h, const int32_t *streams, int32_t n, const void *host_buf,
                                 int64_t buf_bytes) {
    if (!h || !streams || !host_buf) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    int rc;
    // on the host, before the handle is waited for or a byte is copied
    if ((rc = stream_list_check(h->S, streams, n)) ||
        (rc = qpsk_state_blob_check(&h->p, n, host_buf, buf_bytes)))
        return rc;
    return move_rows(h, kScatter, streams, n, const_cast<void *>(host_buf), buf_bytes);
}

}  // extern "C"
