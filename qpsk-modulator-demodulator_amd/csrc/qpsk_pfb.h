// qpsk_pfb.h -- the polyphase channeliser (include/qpsk_demod.h, "The polyphase
// channeliser on the device"), once: the emit count, the index a frame's branch
// reads, one step of the polyphase sum, the bit reversal, one butterfly, the
// output's sign and gain, and the state record.  The kernels (qpsk_pfb.hip) and
// the host (qpsk_pfb.cpp: the checks, the design, the twiddles, the state check,
// qpsk_pfb_apply_host, and the stand-alone tools/pfb_main.cpp) run the same
// functions, so the device cannot drift from what the host can be held to.  No
// HIP header: plain C++ sees plain inline functions.  Compile with
// -ffp-contract=off.
#pragma once
#include <cstdint>

#include "qpsk_demod.h"
#include "qpsk_quantise.h"   // QPSK_HD

namespace qpsk {

constexpr int kPfbMinChannels = QPSK_PFB_MIN_CHANNELS;
constexpr int kPfbMaxChannels = QPSK_PFB_MAX_CHANNELS;
constexpr int kPfbMaxBranchTaps = QPSK_PFB_MAX_BRANCH_TAPS;
constexpr int kPfbMaxTaps = QPSK_PFB_MAX_TAPS;
constexpr int kPfbTileElems = 4096;                  // frames x channels one workgroup holds
constexpr int64_t kPfbMaxPos = int64_t{1} << 50;
static_assert(kPfbTileElems == kPfbMaxChannels, "the largest transform is one tile");

// One band's state begins with this record (64 bytes); hist[L][2] floats follow.
struct PfbHead {
    int64_t in_pos, out_pos;
    uint8_t reserved[48];
};
static_assert(sizeof(PfbHead) == 64, "the state layout of include/qpsk_demod.h");

struct PfbC {
    float re, im;
};

QPSK_HD int pfb_log2(int M) {
    int l = 0;
    while ((1 << l) < M) ++l;
    return l;
}

// the bytes of one band's state
QPSK_HD int64_t pfb_state_bytes(int M, int K) { return static_cast<int64_t>(sizeof(PfbHead)) + 8 * static_cast<int64_t>(M) * K; }

// frames one workgroup covers
QPSK_HD int pfb_tile_frames(int M) { return kPfbTileElems / M; }

// frames a band has emitted once it has taken in_end inputs: every m with
// m * D <= in_end - 1, i.e. ceil(in_end / D)
QPSK_HD int64_t pfb_emitted(int M, int64_t in_end) {
    const int64_t D = M / 2;
    return (in_end + D - 1) / D;
}

QPSK_HD int64_t pfb_count(int M, int64_t out_pos, int64_t in_end) {
    const int64_t k = pfb_emitted(M, in_end);
    return k > out_pos ? k - out_pos : 0;
}

// the absolute input index that tap k of branch p reads in frame m
QPSK_HD int64_t pfb_index(int M, int64_t m, int p, int k) { return m * (M / 2) - p - static_cast<int64_t>(k) * M; }

// one tap of v[p]: acc + h * x, the parts apart
QPSK_HD void pfb_step(PfbC &acc, float h, float xre, float xim) {
    acc.re = acc.re + h * xre;
    acc.im = acc.im + h * xim;
}

// p's lowest `bits` bits in reverse order
QPSK_HD unsigned pfb_bitrev(unsigned p, int bits) {
    unsigned r = 0;
    for (int b = 0; b < bits; ++b) r |= ((p >> b) & 1u) << (bits - 1 - b);
    return r;
}

// t = w * hi, the whole product whatever w is; hi = lo - t, then lo = lo + t
QPSK_HD void pfb_butterfly(PfbC &lo, PfbC &hi, float wre, float wim) {
    const float tre = wre * hi.re - wim * hi.im;
    const float tim = wre * hi.im + wim * hi.re;
    hi.re = lo.re - tre;
    hi.im = lo.im - tim;
    lo.re = lo.re + tre;
    lo.im = lo.im + tim;
}

// channel c of frame m from a[c]: both parts negated when c * m is odd, then
// each times gain
QPSK_HD PfbC pfb_output(PfbC a, int c, int64_t m, float gain) {
    if (c & static_cast<int>(m & 1)) a.re = -a.re, a.im = -a.im;
    return PfbC{a.re * gain, a.im * gain};
}

// the checks of qpsk_pfb_create on p and n_bands
int pfb_check_params(const qpsk_pfb_params *p, int32_t n_bands);
// the checks of qpsk_pfb_set_taps: L finite floats
int pfb_check_taps(const float *taps, int64_t n_taps, int L);
// the prototype of (M, K) into h[M * K], and W into w[M / 2][2]
void pfb_design(int M, int K, float *h);
void pfb_twiddles(int M, float *w);
// The argument checks a call makes before anything moves (host or device
// form): lengths within [0, n_samples], strides, capacity; fills n_out[b] and
// the longest row.  heads: the [B] records the counts come from.
int pfb_check_call(const qpsk_pfb_params &p, const PfbHead *heads, int32_t B, int64_t stride_in, int64_t stride_out,
                   int64_t out_cap, int64_t n_samples, const int64_t *lengths, int64_t *n_out, int64_t *n_call,
                   int64_t *n_out_max);
// one band's call on host float rows: out is the band's first row, rows
// stride_out floats apart; advances the state
void pfb_apply_band(const qpsk_pfb_params &p, const float *h, const float *w, PfbHead &head, float *hist, const float *in,
                    int64_t len, float *out, int64_t stride_out);

}  // namespace qpsk
