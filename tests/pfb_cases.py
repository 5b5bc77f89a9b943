"""What the channeliser tests share (tests/test_pfb_abi.py, tests/test_gpu_pfb.py):
the yardstick of the polyphase channeliser (include/qpsk_demod.h, "The polyphase
channeliser on the device").  Needs no GPU; the taps and the twiddles come from
the library as data (tests/test_pfb_abi.py holds them to their formulas).

pfb_reference     the definition as numpy array operations on np.float32: numpy
                  fuses nothing, so every operation rounds once, in the order
                  the definition writes them.
pfb_exact         the same frames from the filter-bank sum itself, in complex128.
py_count          the emit count by a loop over frames.
PyPfb             one band's state over a call sequence, pure Python.
"""
import functools

import numpy as np

f32, f64 = np.float32, np.float64
CHANNELS = [8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096]
BRANCH_TAPS = [1, 2, 3, 8, 16]          # at M = 16
TILE_ELEMS = 4096                       # frames x channels one workgroup holds


def tile_frames(M):
    return TILE_ELEMS // M


def design_formula(M, K):
    """The prototype by its formula in numpy float64, as float32 [L]."""
    L = M * K
    n = np.arange(1, L, dtype=f64)
    t = (n - L / 2) / M
    safe = np.where(t == 0, 1.0, t)
    sinc = np.where(t == 0, 1.0, np.sin(np.pi * safe) / (np.pi * safe))
    g = sinc * (0.54 - 0.46 * np.cos(2.0 * np.pi * (n - 1) / (L - 2)))
    return np.concatenate([[0.0], g / g.sum()]).astype(f32)


def twiddle_formula(M):
    q = np.arange(M // 2, dtype=f64)
    a = 2.0 * np.pi * q / M
    w = np.stack([np.cos(a), np.sin(a)], axis=1).astype(f32)
    w[0] = [1.0, 0.0]
    w[M // 4] = [0.0, 1.0]
    return w


def bitrev(M):
    bits = M.bit_length() - 1
    p = np.arange(M)
    r = np.zeros(M, np.int64)
    for b in range(bits):
        r |= ((p >> b) & 1) << (bits - 1 - b)
    return r


def py_emitted(M, in_end):
    """How many frames m >= 0 have m * D <= in_end - 1, by a loop over frames."""
    D, m = M // 2, 0
    while m * D <= in_end - 1:
        m += 1
    return m


def py_count(M, out_pos, in_end):
    return max(0, py_emitted(M, in_end) - out_pos)


def py_out_bound(M, n_in):
    return n_in // (M // 2) + 1


def pfb_reference(x, M, K, h, W, gain=1.0):
    """Every frame a band can emit from inputs x [2 n] float32 (absolute indices
    0 .. n - 1; what lies before them is +0): float32 [M, 2 frames], row c the
    interleaved samples of channel c."""
    x = np.asarray(x, f32)
    h = np.asarray(h, f32)
    W = np.asarray(W, f32).reshape(M // 2, 2)
    D, L, n = M // 2, M * K, x.size // 2
    m = np.arange((n + D - 1) // D, dtype=np.int64)      # the frames emitted once n inputs are in
    Fr = m.size
    xr = np.concatenate([np.zeros(L, f32), x[0::2]])
    xi = np.concatenate([np.zeros(L, f32), x[1::2]])
    p = np.arange(M, dtype=np.int64)
    idx = m[:, None] * D - p[None, :] + L                # x[m D - p] in the padded rows
    vr, vi = np.zeros((Fr, M), f32), np.zeros((Fr, M), f32)
    with np.errstate(all="ignore"):
        for k in range(K):
            at = idx - k * M
            ok = at >= 0
            at = np.maximum(at, 0)
            hk = h[p + k * M][None, :]
            vr = vr + hk * np.where(ok, xr[at], f32(0))
            vi = vi + hk * np.where(ok, xi[at], f32(0))
        ar, ai = np.zeros_like(vr), np.zeros_like(vi)
        br = bitrev(M)
        ar[:, br], ai[:, br] = vr, vi
        half = 1
        while half < M:
            w = W[np.arange(half) * (M // (2 * half))]
            wr, wi = w[:, 0][None, None, :], w[:, 1][None, None, :]
            ar4, ai4 = ar.reshape(Fr, M // (2 * half), 2, half), ai.reshape(Fr, M // (2 * half), 2, half)
            lor, loi, hir, hii = ar4[:, :, 0, :], ai4[:, :, 0, :], ar4[:, :, 1, :], ai4[:, :, 1, :]
            tr = wr * hir - wi * hii
            ti = wr * hii + wi * hir
            nr, ni = np.empty_like(ar4), np.empty_like(ai4)
            nr[:, :, 1, :], ni[:, :, 1, :] = lor - tr, loi - ti
            nr[:, :, 0, :], ni[:, :, 0, :] = lor + tr, loi + ti
            ar, ai = nr.reshape(Fr, M), ni.reshape(Fr, M)
            half *= 2
        odd = ((m[:, None] & 1) & (p[None, :] & 1)).astype(bool)
        ar, ai = np.where(odd, -ar, ar), np.where(odd, -ai, ai)
        g = f32(gain)
        ar, ai = ar * g, ai * g
    assert ar.dtype == f32 and ai.dtype == f32
    out = np.zeros((M, 2 * Fr), f32)
    out[:, 0::2], out[:, 1::2] = ar.T, ai.T
    return out


def pfb_exact(x, M, K, h, m, c=None):
    """Frames m (an int array) of channels c (default: all) from the filter-bank sum itself,
    sum_n h[n] x[m D - n] e^{-j 2 pi c (m D - n) / M}, in complex128 on the same
    float inputs (x from absolute index 0): ([len(c), frames] complex128, and
    sum_n |h[n]| |x[m D - n]| per frame, the scale of its rounding error)."""
    x = np.asarray(x, f32)
    h64 = np.asarray(h, f32).astype(f64)
    D, L = M // 2, M * K
    z = np.concatenate([np.zeros(L, np.complex128), x[0::2].astype(f64) + 1j * x[1::2].astype(f64)])
    n = np.arange(L, dtype=np.int64)
    c = np.arange(M, dtype=np.int64) if c is None else np.asarray(c, np.int64)
    out = np.zeros((c.size, len(m)), np.complex128)
    scale = np.zeros(len(m), f64)
    for k, mm in enumerate(m):
        i = int(mm) * D - n                                # absolute indices
        seg = h64 * z[i + L]
        ph = np.exp(-2j * np.pi * ((c[:, None] * i[None, :]) % M) / M)
        out[:, k] = ph @ seg
        scale[k] = np.sum(np.abs(seg))
    return out, scale


class PyPfb:
    """One band's state record over calls, and the record as the library lays it out."""

    def __init__(self, M, K):
        self.M, self.K, self.L = M, K, M * K
        self.in_pos = self.out_pos = 0
        self.hist = np.zeros((self.L, 2), f32)

    def call(self, x):
        """Takes x [2 len] float32; returns the number of frames the call emits."""
        x = np.asarray(x, f32).reshape(-1, 2)
        cnt = py_count(self.M, self.out_pos, self.in_pos + x.shape[0])
        self.hist = np.concatenate([self.hist, x])[-self.L:]
        self.in_pos += x.shape[0]
        self.out_pos += cnt
        return cnt

    def record(self, dtype):
        rec = np.zeros(1, dtype)
        rec["in_pos"], rec["out_pos"] = self.in_pos, self.out_pos
        rec["hist"][0] = self.hist
        return rec


@functools.lru_cache(maxsize=None)
def random_rows(B, n, seed=0):
    """[B, 2 n] float32 with +-0 and denormals up front."""
    x = np.random.default_rng(seed).standard_normal((B, 2 * max(n, 4))).astype(f32)
    head = np.array([0.0, -0.0, 1e-45, -1e-40, 1.0, -1.0, -0.0, 3e-39], f32)
    x[:, : head.size] = head
    x[1::2, : head.size] = head[::-1]
    x = x[:, : 2 * n]
    x.setflags(write=False)
    return x


def ragged_cuts(M, K):
    """Call lengths that cross frame parity and the history mid-call."""
    D, L = M // 2, M * K
    return [0, 1, D - 1, D, D + 1, L - 2, L, 3 * L + 5]
