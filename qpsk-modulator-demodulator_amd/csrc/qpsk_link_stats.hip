// qpsk_link_stats.hip -- per-stream link statistics of a demodulator handle
// (qpsk_demod_link_stats): the switch, the read and the kernel
// that composes the rows.  The sums themselves are formed by the loop kernel's
// decode wave (qpsk_loop.hip) while the switch is on.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "qpsk_handle.h"

using namespace qpsk;

static_assert(sizeof(qpsk_link_stats) == 64 && offsetof(qpsk_link_stats, fll_freq) == 56 &&
                  offsetof(qpsk_link_stats, error) == 60,
              "qpsk_link_stats is 64 bytes without padding");

namespace qpsk {

// The gather kernel: one qpsk_link_stats row per stream, the three running
// sums from the accumulators and a copy of the loop state from the stream
// record.  One lane per stream; reset zeroes the sums behind the read (the
// lane that read them, so nothing is lost in between).
__global__ __launch_bounds__(256) void link_stats_gather_kernel(LinkGatherArgs a) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.S) return;
    const LinkAcc acc = a.acc[s];
    const StreamState &st = a.state[s];
    qpsk_link_stats r;
    r.n_symbols = acc.n;
    r.sum_dist2 = acc.sum_dist2;
    r.sum_power = acc.sum_power;
    r.costas_freq = st.freq;
    r.costas_theta = st.theta;
    r.mm_mu = st.mu;
    r.mm_rate = st.integ;
    r.fll_freq = a.fll ? st.fll_freq : 0.0f;
    r.error = st.error;
    static_cast<qpsk_link_stats *>(a.out)[s] = r;
    if (a.reset) a.acc[s] = LinkAcc{0.0, 0.0, 0};
}

void launch_link_gather(const LinkGatherArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(link_stats_gather_kernel, dim3((a.S + 255) / 256), dim3(256), 0, stream, a);
}

}  // namespace qpsk

extern "C" {

int qpsk_link_stats_size(void) { return static_cast<int>(sizeof(qpsk_link_stats)); }

int qpsk_demod_enable_link_stats(qpsk_demod *h, int32_t on) {
    if (!h) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    int rc;
    if ((rc = handle_sync(h))) return rc;
    if (on) {
        const size_t S = static_cast<size_t>(h->S);
        if ((rc = alloc_status(h->link.d_link.alloc(S))) || (rc = alloc_status(h->link.d_link_rows.alloc(S))))
            return rc;
        // +0.0, +0.0, 0; on the handle's stream, which every later call and
        // read is ordered behind (a null-stream memset is not: the handle's
        // streams do not synchronise with it)
        QPSK_HIP_TRY(hipMemsetAsync(h->link.d_link, 0, S * sizeof(LinkAcc), h->stream));
    }
    h->link.on = on != 0;
    return QPSK_OK;
}

int qpsk_demod_link_stats(qpsk_demod *h, qpsk_link_stats *out, int32_t mem, int32_t reset) {
    if (!h || !out) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    if (mem != QPSK_MEM_HOST && mem != QPSK_MEM_DEVICE) return fail(QPSK_ERR_ARGUMENT, "unknown mem");
    if (mem == QPSK_MEM_DEVICE && (reinterpret_cast<uintptr_t>(out) & 7))
        return fail(QPSK_ERR_ARGUMENT, "device link-statistics rows must be 8-byte aligned");
    if (!h->link.on) return fail(QPSK_ERR_STATE, "link statistics are not enabled (qpsk_demod_enable_link_stats)");
    int rc;
    // every queued call has run: the loop kernels of pipelined calls add to the
    // sums on the back stream, the gather reads them on the handle's
    if ((rc = handle_sync(h))) return rc;
    LinkGatherArgs ga{};
    ga.state = h->d_state;
    ga.acc = h->link.d_link;
    ga.out = mem == QPSK_MEM_HOST ? h->link.d_link_rows : out;
    ga.S = h->S;
    ga.fll = h->p.enable_fll ? 1 : 0;
    ga.reset = reset ? 1 : 0;
    launch_link_gather(ga, h->stream);
    QPSK_HIP_TRY(hipGetLastError());
    if (mem == QPSK_MEM_HOST) {
        QPSK_HIP_TRY(hipMemcpyAsync(out, h->link.d_link_rows, static_cast<size_t>(h->S) * sizeof(qpsk_link_stats),
                                    hipMemcpyDeviceToHost, h->stream));
        QPSK_HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return QPSK_OK;
}

}  // extern "C"
