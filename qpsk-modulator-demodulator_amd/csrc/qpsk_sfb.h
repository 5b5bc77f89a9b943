// qpsk_sfb.h -- the polyphase synthesis bank (include/qpsk_demod.h, "The
// polyphase synthesis bank on the device"), once: the sign a frame's input
// takes, the element of a transform an output reads, one step of the polyphase
// sum, the counts and the state record.  The bit reversal, the butterfly, the
// prototype's design and the twiddles are the channeliser's (qpsk_pfb.h): the
// bank is its dual and shares them.  The kernels (qpsk_sfb.hip) and the host
// (qpsk_sfb.cpp: the checks, the state check, qpsk_sfb_apply_host, and the
// stand-alone tools/sfb_main.cpp) run the same functions.  No HIP header: plain
// C++ sees plain inline functions.  Compile with -ffp-contract=off.
#pragma once
#include <cstdint>

#include "qpsk_demod.h"
#include "qpsk_pfb.h"

namespace qpsk {

constexpr int kSfbSumRun = 128;                      // frames one lane pair of the sum kernel walks
constexpr int64_t kSfbSlabElems = int64_t{1} << 22;  // elements of u one slab of a call holds, all bands together
constexpr int kSfbMinSlab = 64;                      // frames a slab holds at the least

// One band's state begins with this record (64 bytes); hist[2K - 1][M][2] floats follow.
struct SfbHead {
    int64_t in_pos, out_pos;
    uint8_t reserved[48];
};
static_assert(sizeof(SfbHead) == QPSK_SFB_STATE_HEAD, "the state layout of include/qpsk_demod.h");

// the frames of history a band keeps, and the bytes of its state
QPSK_HD int sfb_hist_frames(int K) { return 2 * K - 1; }
QPSK_HD int64_t sfb_state_bytes(int M, int K) {
    return static_cast<int64_t>(sizeof(SfbHead)) + 8 * static_cast<int64_t>(M) * sfb_hist_frames(K);
}

// the largest in_pos: out_pos = in_pos * D stays within 2^50
QPSK_HD int64_t sfb_max_frames(int M) { return kPfbMaxPos / (M / 2); }

// samples a band has emitted once it has taken `frames` frames
QPSK_HD int64_t sfb_emitted(int M, int64_t frames) { return frames * (M / 2); }

// step 1: row c's sample of frame m, both parts negated when c * m is odd
QPSK_HD PfbC sfb_input(PfbC s, int c, int64_t m) {
    if (c & static_cast<int>(m & 1)) s.re = -s.re, s.im = -s.im;
    return s;
}

// step 3: the element of u_{f - j} that term j of output r of frame f reads, (r + j D) mod M
QPSK_HD int sfb_index(int M, int r, int j) { return r + (j & 1) * (M / 2); }

// one term of the sum: acc + g * u, the parts apart
QPSK_HD void sfb_step(PfbC &acc, float g, PfbC u) { pfb_step(acc, g, u.re, u.im); }

// the frames of a call that fill the transform kernel's tiles exactly: the
// tiles of 4096 / M frames count from the 2K - 1 frames of history in front of
// the call
QPSK_HD int sfb_transform_tile(int M, int K) {
    const int F = pfb_tile_frames(M), H = sfb_hist_frames(K);
    return ((H + F) / F) * F - H;
}

// the frames of one slab of a call on a handle of B bands
QPSK_HD int64_t sfb_slab_frames(int M, int B) {
    const int64_t s = kSfbSlabElems / M / B;
    return s > kSfbMinSlab ? s : kSfbMinSlab;
}

// the checks of qpsk_sfb_create on p and n_bands
int sfb_check_params(const qpsk_sfb_params *p, int32_t n_bands);
// The argument checks a call makes before anything moves (host or device
// form): lengths within [0, n_frames], strides, positions; fills the longest
// row.  heads: the [B] records.
int sfb_check_call(const qpsk_sfb_params &p, const SfbHead *heads, int32_t B, int64_t stride_in, int64_t stride_out,
                   int64_t n_frames, const int64_t *lengths, int64_t *n_call);
// one band's call on host float rows: in is the band's first row, rows
// stride_in floats apart; advances the state
void sfb_apply_band(int M, int K, const float *g, const float *w, SfbHead &head, float *hist, const float *in,
                    int64_t stride_in, int64_t len, float *out, float scale_out);

}  // namespace qpsk
