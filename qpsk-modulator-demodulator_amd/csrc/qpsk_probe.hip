// qpsk_probe.hip -- the diagnostic read-outs of a demodulator handle: the launch
// timestamps and clock samples of timed calls (qpsk_demod_enable_timing; the
// kernels write them, qpsk_kernels.h kt_start / kt_end / ClkSample) and the
// FIR phase sample (qpsk_demod_enable_fir_phases).  The call paths
// (qpsk_runtime.hip) only hand the kernels the slots; everything that makes,
// clears and reads them is here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "qpsk_handle.h"

using namespace qpsk;

extern "C" {

int qpsk_demod_enable_timing(qpsk_demod *h, int32_t on) {
    if (!h) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    h->probe.kt_used = 0;
    h->probe.timing = on != 0;
    if (!h->probe.timing) return QPSK_OK;
    QPSK_HIP_TRY(hipSetDevice(h->p.device));
    int rc;
    const size_t n = static_cast<size_t>(kKtCalls) * kKtPerCall;
    if ((rc = alloc_status(h->probe.d_kt.alloc(n)))) return rc;
    // spans: start = +inf for the atomic minimum, end = 0 for the maximum;
    // clock sums = 0
    std::vector<unsigned long long> init(n, 0ull);
    for (size_t i = 0; i < n; i += 2)
        if (i % kKtPerCall < kKtSpanSlots) init[i] = ~0ull;
    if ((rc = handle_sync(h))) return rc;
    QPSK_HIP_TRY(hipMemcpy(h->probe.d_kt, init.data(), n * sizeof(unsigned long long), hipMemcpyHostToDevice));
    return QPSK_OK;
}

int qpsk_demod_enable_fir_phases(qpsk_demod *h, int32_t on) {
    if (!h) return fail(QPSK_ERR_ARGUMENT_NULL, "null handle");
    int rc;
    if ((rc = handle_sync(h))) return rc;
    if (on && (!h->probe.d_phases || !h->probe.d_cu_map)) {
        // both or neither: a half-allocated pair would let the sampled FIR
        // workgroups read a null cu_map
        if ((rc = alloc_status(h->probe.d_phases.alloc(kFirPhaseWords))) ||
            (rc = alloc_status(h->probe.d_cu_map.alloc(kCuKeys)))) {
            h->probe.d_phases.reset();
            h->probe.d_cu_map.reset();
            return rc;
        }
        QPSK_HIP_TRY(hipMemset(h->probe.d_cu_map, 0, kCuKeys * sizeof(unsigned)));
    }
    if (on) QPSK_HIP_TRY(hipMemset(h->probe.d_phases, 0, kFirPhaseWords * sizeof(unsigned long long)));
    h->probe.fir_phases = on != 0;
    return QPSK_OK;
}

int qpsk_demod_fir_phases(qpsk_demod *h, uint64_t *out, int32_t n) {
    if (!h || !out) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    if (n < kFirPhaseWords) return fail(QPSK_ERR_ARGUMENT, "n < 16");
    if (!h->probe.d_phases) {
        std::memset(out, 0, kFirPhaseWords * sizeof(uint64_t));
        return kFirPhaseWords;
    }
    int rc;
    if ((rc = handle_sync(h))) return rc;
    QPSK_HIP_TRY(hipMemcpy(out, h->probe.d_phases, kFirPhaseWords * sizeof(uint64_t), hipMemcpyDeviceToHost));
    QPSK_HIP_TRY(hipMemset(h->probe.d_phases, 0, kFirPhaseWords * sizeof(unsigned long long)));
    return kFirPhaseWords;
}

// the timestamp slots of the timed calls so far, once every one of them has run
static int read_kt(qpsk_demod *h, std::vector<unsigned long long> *t) {
    int rc;
    if ((rc = handle_sync(h))) return rc;
    if (h->s_front) QPSK_HIP_TRY(hipStreamSynchronize(h->s_front));
    if (h->s_back) QPSK_HIP_TRY(hipStreamSynchronize(h->s_back));
    t->resize(static_cast<size_t>(h->probe.kt_used) * kKtPerCall);
    QPSK_HIP_TRY(hipMemcpy(t->data(), h->probe.d_kt, t->size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return QPSK_OK;
}

// per timed call: FLL, FIR and loop kernel durations and the call's kernel
// span (earliest start to latest end), ms; 0 for a kernel that did not run
static int read_launch_times(qpsk_demod *h, std::vector<float> *out) {
    out->assign(static_cast<size_t>(h->probe.kt_used) * 4, 0.f);
    if (!h->probe.kt_used) return QPSK_OK;
    int rc;
    std::vector<unsigned long long> t;
    if ((rc = read_kt(h, &t))) return rc;
    const double ms_per_tick = 1.0 / h->wall_khz;
    for (int c = 0; c < h->probe.kt_used; ++c) {
        const unsigned long long *k = t.data() + static_cast<size_t>(kKtPerCall) * c;
        unsigned long long lo = ~0ull, hi = 0;
        for (int j = 0; j < 3; ++j) {
            const unsigned long long s0 = k[kKtSpan[j]], e0 = k[kKtSpan[j] + 1];
            if (s0 == ~0ull || e0 < s0) continue;   // did not run
            (*out)[4 * c + j] = static_cast<float>((e0 - s0) * ms_per_tick);
            lo = std::min(lo, s0);
            hi = std::max(hi, e0);
        }
        if (hi >= lo && lo != ~0ull) (*out)[4 * c + 3] = static_cast<float>((hi - lo) * ms_per_tick);
    }
    return QPSK_OK;
}

int qpsk_demod_stage_times(qpsk_demod *h, float *ms, int32_t n) {
    if (!h || !ms) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    std::vector<float> t;
    int rc;
    if ((rc = read_launch_times(h, &t))) return rc;
    const int k = std::min<int32_t>(n, 4);
    for (int i = 0; i < k; ++i) {
        double sum = 0;
        int cnt = 0;
        for (int c = 0; c < h->probe.kt_used; ++c)
            if (t[4 * c + i] > 0.f) {
                sum += t[4 * c + i];
                ++cnt;
            }
        ms[i] = cnt ? static_cast<float>(sum / cnt) : 0.f;
    }
    return k;
}

int qpsk_demod_kernel_clocks(qpsk_demod *h, float *ghz, int32_t max_calls) {
    if (!h || !ghz) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    if (!h->probe.kt_used) return 0;
    int rc;
    std::vector<unsigned long long> t;
    if ((rc = read_kt(h, &t))) return rc;
    const int k = std::min<int32_t>(max_calls, h->probe.kt_used);
    for (int c = 0; c < k; ++c) {
        const unsigned long long *s = t.data() + static_cast<size_t>(kKtPerCall) * c;
        for (int j = 0; j < 3; ++j) {
            const unsigned long long cy = s[kKtClk[j]], wt = s[kKtClk[j] + 1];
            ghz[3 * c + j] = wt ? static_cast<float>(static_cast<double>(cy) / wt * h->wall_khz * 1e-6) : 0.f;
        }
    }
    return k;
}

int qpsk_demod_launch_times(qpsk_demod *h, float *ms, int32_t max_calls) {
    if (!h || !ms) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    std::vector<float> t;
    int rc;
    if ((rc = read_launch_times(h, &t))) return rc;
    const int k = std::min<int32_t>(max_calls, h->probe.kt_used);
    std::memcpy(ms, t.data(), static_cast<size_t>(k) * 4 * sizeof(float));
    return k;
}

}  // extern "C"
