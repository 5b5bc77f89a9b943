"""What the synthesis bank's tests share (tests/test_sfb_abi.py,
tests/test_gpu_sfb.py): the yardstick of the polyphase synthesis bank
(include/qpsk_demod.h, "The polyphase synthesis bank on the device").  Needs no
GPU; the taps and the twiddles come from the library as data
(tests/test_pfb_abi.py holds them to their formulas).

sfb_reference     the definition as numpy array operations on np.float32: numpy
                  fuses nothing, so every operation rounds once, in the order
                  the definition writes them.
sfb_exact         chosen output samples from the filter-bank sum itself, in
                  complex128.
PySfb             one band's state over a call sequence, pure Python.
"""
import functools

import numpy as np

import pfb_cases as PC

f32, f64 = np.float32, np.float64
SUM_RUN = 128                           # frames a lane of the sum kernel walks
SLAB_ELEMS = 1 << 22                    # transform elements one pass of a call holds
MIN_SLAB = 64


def transform_tile(M, K):
    """The smallest n >= 1 for which n + 2K - 1 fills the transform kernel's tiles of 4096 / M frames."""
    F, H = PC.tile_frames(M), 2 * K - 1
    n = 1
    while (n + H) % F:
        n += 1
    return n


def slab_frames(M, B=1):
    return max(MIN_SLAB, SLAB_ELEMS // M // B)


def transforms(s, M, W, m0=0):
    """Steps 1 and 2 on rows s [M, 2 n] float32, frames m0 .. m0 + n - 1: (re, im), each float32 [n, M]."""
    s = np.asarray(s, f32)
    W = np.asarray(W, f32).reshape(M // 2, 2)
    n = s.shape[1] // 2
    m = m0 + np.arange(n, dtype=np.int64)
    c = np.arange(M, dtype=np.int64)
    odd = ((m[:, None] & 1) & (c[None, :] & 1)).astype(bool)
    zr, zi = np.where(odd, -s[:, 0::2].T, s[:, 0::2].T), np.where(odd, -s[:, 1::2].T, s[:, 1::2].T)
    ar, ai = np.zeros((n, M), f32), np.zeros((n, M), f32)
    br = PC.bitrev(M)
    ar[:, br], ai[:, br] = zr, zi
    half = 1
    with np.errstate(all="ignore"):
        while half < M:
            w = W[np.arange(half) * (M // (2 * half))]
            wr, wi = w[:, 0][None, None, :], w[:, 1][None, None, :]
            ar4, ai4 = ar.reshape(n, M // (2 * half), 2, half), ai.reshape(n, M // (2 * half), 2, half)
            lor, loi, hir, hii = ar4[:, :, 0, :], ai4[:, :, 0, :], ar4[:, :, 1, :], ai4[:, :, 1, :]
            tr = wr * hir - wi * hii
            ti = wr * hii + wi * hir
            nr, ni = np.empty_like(ar4), np.empty_like(ai4)
            nr[:, :, 1, :], ni[:, :, 1, :] = lor - tr, loi - ti
            nr[:, :, 0, :], ni[:, :, 0, :] = lor + tr, loi + ti
            ar, ai = nr.reshape(n, M), ni.reshape(n, M)
            half *= 2
    assert ar.dtype == f32 and ai.dtype == f32
    return ar, ai


def sfb_reference(s, M, K, g, W, scale_out=1.0):
    """Everything a band emits for rows s [M, 2 n] float32 (frames 0 .. n - 1;
    what lies before them contributes +0): float32 [2 n D], the interleaved
    samples of the wideband row, each times scale_out (None: acc itself, what
    the quantiser of an integer format takes)."""
    g = np.asarray(g, f32)
    D, H, n = M // 2, 2 * K - 1, np.asarray(s).shape[1] // 2
    ur, ui = transforms(s, M, W)
    ur, ui = np.concatenate([np.zeros((H, M), f32), ur]), np.concatenate([np.zeros((H, M), f32), ui])
    r = np.arange(D)
    accr, acci = np.zeros((n, D), f32), np.zeros((n, D), f32)
    with np.errstate(all="ignore"):
        for j in range(2 * K):
            col = r + (j & 1) * D                          # (r + j D) mod M
            gj = g[j * D + r][None, :]
            accr = accr + gj * ur[H - j: H - j + n][:, col]
            acci = acci + gj * ui[H - j: H - j + n][:, col]
        if scale_out is not None:
            accr, acci = accr * f32(scale_out), acci * f32(scale_out)
    assert accr.dtype == f32 and acci.dtype == f32
    out = np.zeros(2 * n * D, f32)
    out[0::2], out[1::2] = accr.reshape(-1), acci.reshape(-1)
    return out


def sfb_exact(s, M, K, g, idx):
    """Output samples idx (an int array) from the filter-bank sum itself,
    sum_c sum_m s_c[m] g[i - m D] e^{+j 2 pi c i / M}, in complex128 on the same
    float inputs: ([len(idx)] complex128, and sum_c sum_m |g[i - m D]| |s_c[m]|
    per sample, the scale of its rounding error)."""
    s = np.asarray(s, f32)
    g64 = np.asarray(g, f32).astype(f64)
    D, L, n = M // 2, M * K, s.shape[1] // 2
    z = s[:, 0::2].astype(f64) + 1j * s[:, 1::2].astype(f64)
    c = np.arange(M, dtype=np.int64)
    out, scale = np.zeros(len(idx), np.complex128), np.zeros(len(idx), f64)
    for k, i in enumerate(idx):
        i = int(i)
        m = np.arange(max(0, -(-(i - L + 1) // D)), min(i // D, n - 1) + 1)
        gi = g64[i - m * D]
        ph = np.exp(2j * np.pi * ((c * i) % M) / M)
        out[k] = ph @ (z[:, m] @ gi)
        scale[k] = np.sum(np.abs(z[:, m]) @ np.abs(gi))
    return out, scale


class PySfb:
    """One band's state record over calls, and the record as the library lays it out."""

    def __init__(self, M, K):
        self.M, self.K, self.H = M, K, 2 * K - 1
        self.in_pos = self.out_pos = 0
        self.hist = np.zeros((self.H, M, 2), f32)

    def call(self, s):
        """Takes rows s [M, 2 len] float32 (widened); returns the samples the call emits."""
        s = np.asarray(s, f32).reshape(self.M, -1, 2)
        n = s.shape[1]
        self.hist = np.concatenate([self.hist, s.transpose(1, 0, 2)])[-self.H:]
        self.in_pos += n
        self.out_pos += n * (self.M // 2)
        return n * (self.M // 2)

    def record(self, dtype):
        rec = np.zeros(1, dtype)
        rec["in_pos"], rec["out_pos"] = self.in_pos, self.out_pos
        rec["hist"][0] = self.hist
        return rec


@functools.lru_cache(maxsize=None)
def random_rows(B, M, n, seed=0):
    """[B M, 2 n] float32 with +-0 and denormals up front."""
    return PC.random_rows(B * M, n, seed)


def call_cuts(K):
    """Call lengths in frames around the history's 2K - 1."""
    return [0, 1, 2, 2 * K - 2, 2 * K - 1, 2 * K, 6 * K + 1]


def quantised(acc, out_fmt, scale_out):
    """The yardstick's sums as the modulator's fixed-scale quantiser stores
    them: the restatement the modulator's tests use."""
    from test_quantise_abi import quantise_ref
    return quantise_ref(np.asarray(acc, f32), out_fmt, "fixed", scale_out)[0]


# ---------------------------------------------------------------------------
# the chain: modulator -> synthesis bank -> channeliser -> demodulator -> framer
# ---------------------------------------------------------------------------
START, STOP = b"MESSAGE_START", b"MESSAGE_STOP"
E2E = dict(M=16, K=8, rounds=3, span=8, tail=64)
# the wideband hop: its format, the bank's scale_out as a multiple of D, the channeliser's scale_in
HOPS = {"cf32": (1.0, None), "cs16": (2000.0, 1.0 / 2000), "cs8": (12.0, 1.0 / 12)}


def payload(c, k):
    import common as K
    return (f"carrier {c} round {k}: " + K.PAYLOAD * 3)[:48].encode("utf-8")


@functools.lru_cache(maxsize=None)
def wideband_case(fmt):
    """Per channel and round what the CPU chain returns: oracle.modulate_bytes at
    4 samples a symbol (one 48-byte frame a carrier and round, `tail` zero
    samples behind it) -> sfb_reference (and the quantiser) -> pfb_reference ->
    OracleDemod.DeModulateBytes, cut as the calls cut it.  Returns (the frames a
    round takes, the largest wideband element, the frames [M][rounds])."""
    import common as K
    import gpu_harness as H
    import oracle as O
    import qpsk_amd
    M, K_, rounds, span, tail = (E2E[k] for k in ("M", "K", "rounds", "span", "tail"))
    D = M // 2
    fs_ch, rs = K.FS // D, K.FS // (2 * M)
    mult, scale_in = HOPS[fmt]
    blocks = []
    for k in range(rounds):
        sigs = [O.modulate_bytes(fs_ch, rs, payload(c, k), START, STOP, rrc_alpha=K.ALPHA, rrc_span=span, tsc=K.TSC)
                for c in range(M)]
        assert len({s.size for s in sigs}) == 1
        blk = np.zeros((M, sigs[0].size + 2 * tail), f32)
        blk[:, : sigs[0].size] = np.stack(sigs)
        blocks.append(blk)
    n = blocks[0].shape[1] // 2
    g = qpsk_amd.pfb_design(qpsk_amd.pfb_params(channels=M, taps_per_branch=K_))
    W = qpsk_amd.pfb_twiddles(M)
    acc = sfb_reference(np.concatenate(blocks, axis=1), M, K_, g, W, scale_out=None)
    wide = quantised(acc, fmt, mult * D)
    peak = float(np.abs(wide.astype(f64)).max())
    if fmt != "cf32":
        wide = H.widened(wide, fmt, scale_in)
    y = PC.pfb_reference(wide, M, K_, g, W)
    assert y.shape[1] // 2 == rounds * n
    want = []
    for c in range(M):
        dm = O.OracleDemod(fs_ch, rs, K.ALPHA, span, tsc=K.TSC)
        want.append([dm.DeModulateBytes(y[c, 2 * k * n: 2 * (k + 1) * n], START, STOP) for k in range(rounds)])
    return n, peak, want
