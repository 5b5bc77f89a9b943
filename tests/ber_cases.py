"""What the bit-error counter's tests share (tests/test_ber_abi.py on the host,
tests/test_gpu_ber.py on the device): the seeded cases, a restatement of the
definition that also serves reference rows whose bit count is no multiple of
8, the yardstick (bench.ber_after_lock, one stream at a time), and rows laid
out with strides, base offsets and 0xFF behind every valid bit.

A case is (name, params, rx bits, ref bits, hand-worked counts or None), the
bits as uint8 arrays of 0 / 1.  Cases are grouped by their parameters: one
call of the library has one parameter set, so a batch holds cases of one group.
"""
import collections
import functools

import numpy as np

import bench
import qpsk_amd as Q

Case = collections.namedtuple("Case", "name params rx ref hand")

P100 = dict(skip_bits=100, window=100, key_bits=16, search=32)      # the issue's small shape
P100_D0 = dict(P100, search=0)
P_K1 = dict(skip_bits=0, window=64, key_bits=1, search=0)       # the key is one bit: found at bit 0
P_K13 = dict(skip_bits=7, window=129, key_bits=13, search=5)
P_K64_W64 = dict(skip_bits=33, window=64, key_bits=64, search=3)
P_DEFAULT = dict(skip_bits=8000, window=2048, key_bits=64, search=512)
# a 16-bit key with no border (no proper prefix equals a suffix) that starts and ends in 1
KEY16 = np.array([1, 0, 1, 0, 0, 1, 1, 1, 0, 1, 1, 0, 0, 1, 0, 1], np.uint8)


def rand(n, seed):
    return np.random.default_rng(seed).integers(0, 2, n, dtype=np.uint8)


def flipped(bits, positions):
    out = bits.copy()
    out[np.asarray(positions, np.int64)] ^= 1
    return out


def flips(bits, k, seed, lo=0):
    """k distinct seeded flips at positions >= lo."""
    return flipped(bits, lo + np.random.default_rng(seed).choice(bits.size - lo, k, replace=False))


def _step_edge(pos):
    """The first window's key occurs first at ref position pos (lo = 0, so the
    kernel's step edges are 63 | 64) and again 200 bits later, inside the range."""
    data = rand(3000, 40 + pos)
    data[:16] = KEY16
    data[200:216] = KEY16
    ref = np.zeros(4000, np.uint8)
    ref[pos: pos + 3000] = data
    rx = np.concatenate([rand(100, 41), data])
    return rx, ref


def _key_at_range_end(at, n_ref):
    """One window (w = 100, R = 200) whose key lies in ref only at position `at`."""
    rx = np.concatenate([rand(100, 50), KEY16, rand(84, 51)])
    ref = np.zeros(max(n_ref, at + 16), np.uint8)
    ref[at: at + 16] = KEY16
    return rx, ref[:n_ref]


@functools.lru_cache(maxsize=None)
def cases():
    """Every case, in a fixed order."""
    out = []
    add = lambda name, params, rx, ref, hand=None: out.append(Case(name, params, rx, ref, hand))
    ref = rand(4000, 1)
    rx = ref[2:]                                   # the differential decoder's dropped dibit
    # hand-worked: 38 windows from bit 100 on, all found at offset 2
    add("clean", P100, rx, ref, dict(bit_errors=0, bits=3800, lost_windows=0, slips=0, windows=38, last_offset=2,
                                     located=1))
    add("flips30", P100, flips(rx, 30, 2), ref)
    slipped = flips(rx, 30, 3)
    slipped = np.concatenate([slipped[:1500], slipped[1502:2600], rand(2, 4), slipped[2600:]])
    add("flips_deletion_insertion", P100, slipped, ref)
    per = np.tile(rand(24, 5), 167)[:4000]
    add("period24", P100, per[2:], per)            # first match, not nearest: slips on clean data
    add("negative_offset", P100, np.concatenate([rand(50, 6), ref]), ref)
    for R in (0, 199, 200, 201):                   # w0 + W = 200
        add(f"R{R}", P100, rx[:R], ref)
    add("N_below_K", P100, rx, ref[:10])
    add("N_zero", P100, rx, ref[:0])
    add("ref_ends_in_window", P100, np.concatenate([ref[2:2960], rand(1000, 7)]), ref[:2960])
    add("ref_ends_in_window_odd", P100, np.concatenate([ref[2:2957], rand(1000, 7)]), ref[:2957])
    # window [300, 400): m / 8 = 12 errors clear of the key and of the last 16 bits are counted, 13 lose it
    add("errors_at_limit", P100, flipped(rx, range(320, 332)), ref,
        dict(bit_errors=12, bits=3800, lost_windows=0, slips=0, windows=38, last_offset=2, located=1))
    add("errors_past_limit", P100, flipped(rx, range(320, 333)), ref,
        dict(bit_errors=0, bits=3700, lost_windows=1, slips=0, windows=38, last_offset=2, located=1))
    add("flip_in_key", P100, flipped(rx, [305]), ref,
        dict(bit_errors=0, bits=3700, lost_windows=1, slips=0, windows=38, last_offset=2, located=1))
    add("flip_in_tail", P100, flipped(rx, [390]), ref,
        dict(bit_errors=0, bits=3700, lost_windows=1, slips=0, windows=38, last_offset=2, located=1))
    for pos in (63, 64, 65):
        srx, sref = _step_edge(pos)
        add(f"step_edge_{pos}", P100, srx, sref,
            dict(bit_errors=0, bits=3000, lost_windows=0, slips=0, windows=30, last_offset=pos - 100, located=1))
    # hi = min(N, w + 4 W): the key must lie wholly below it
    add("key_ends_at_N", P100, *_key_at_range_end(288, 304),
        hand=dict(bit_errors=0, bits=16, lost_windows=0, slips=0, windows=1, last_offset=188, located=1))
    add("key_ends_past_N", P100, *_key_at_range_end(288, 303),
        hand=dict(bit_errors=0, bits=0, lost_windows=1, slips=0, windows=1, last_offset=0, located=0))
    add("key_ends_at_hi", P100, *_key_at_range_end(484, 600),
        hand=dict(bit_errors=0, bits=0, lost_windows=1, slips=0, windows=1, last_offset=384, located=1))
    add("key_ends_past_hi", P100, *_key_at_range_end(485, 600),
        hand=dict(bit_errors=0, bits=0, lost_windows=1, slips=0, windows=1, last_offset=0, located=0))
    add("noise", P100, rand(4000, 8), ref)         # never locates: every window scans its whole range

    add("d0_clean", P100_D0, rx, ref)
    add("d0_deletion", P100_D0, np.concatenate([rx[:1500], rx[1502:]]), ref)
    add("k1", P_K1, flips(ref, 60, 9, lo=1), ref)
    add("k1_same", P_K1, ref, ref)
    ref13 = rand(4003 + 2, 10)
    rx13 = flips(ref13[2:], 25, 11)
    add("k13_w129", P_K13, np.concatenate([rx13[:2000], rx13[2002:]]), ref13[:4000])
    add("k13_w129_odd_ref", P_K13, np.concatenate([rx13[:2000], rx13[2002:]]), ref13)
    add("k64_w64", P_K64_W64, flips(rx, 6, 12), ref)
    big = rand(40000, 13)
    brx = flips(big[2:], 200, 14)
    add("defaults_40000", P_DEFAULT, np.concatenate([brx[:21000], brx[21001:]]), big)
    add("defaults_short", P_DEFAULT, big[2:10047], big)        # R = w0 + W - 3: no window
    add("defaults_noise", P_DEFAULT, rand(20000, 15), big[:16000])
    return tuple(out)


def groups():
    """Cases by parameter set, in first-seen order: [(params, [case, ...])]."""
    by = collections.OrderedDict()
    for c in cases():
        by.setdefault(tuple(sorted(c.params.items())), []).append(c)
    return [(dict(k), v) for k, v in by.items()]


FIELDS = ("bit_errors", "bits", "lost_windows", "slips", "windows", "last_offset", "located")


def model(rx, ref, skip_bits, window, key_bits, search):
    """The definition of include/qpsk_demod.h on 0 / 1 arrays, as a dict of the
    row's fields: ber_after_lock's loop (bytes.find is first-match with the
    match wholly inside the slice), also for reference rows of any bit count."""
    rxb, refb = rx.tobytes(), ref.tobytes()
    r = dict.fromkeys(FIELDS, 0)
    off = 0
    w = skip_bits
    while w + window <= rx.size:
        r["windows"] += 1
        key = rxb[w: w + key_bits]
        if r["located"]:
            lo, hi = max(0, w + off - search), min(ref.size, w + off + search + key_bits)
        else:
            lo, hi = 0, min(ref.size, w + 4 * window)
        i = refb.find(key, lo, hi) if hi - lo >= key_bits else -1
        if i < 0:
            r["lost_windows"] += 1
            w += window
            continue
        if r["located"] and i - w != off:
            r["slips"] += 1
        r["located"], off = 1, i - w
        m = min(window, ref.size - i)
        e = int(np.count_nonzero(rx[w: w + m] != ref[i: i + m]))
        if rxb[w + m - key_bits: w + m] != refb[i + m - key_bits: i + m] or e > m // 8:
            r["lost_windows"] += 1
        else:
            r["bit_errors"] += e
            r["bits"] += m
        w += window
    r["last_offset"] = off
    return r


def yardstick(case):
    """bench.ber_after_lock on the case alone: (errs, bits, lost, slips).  It
    takes the reference row whole, so only cases with 8 | N have one."""
    assert case.ref.size % 8 == 0 and case.ref.size > 0
    rx = np.packbits(case.rx) if case.rx.size else np.zeros(1, np.uint8)
    return bench.ber_after_lock(rx[None, :], np.array([case.rx.size], np.int64), np.packbits(case.ref)[None, :], 1,
                                **case.params)


def row_dict(row):
    assert all(int(v) == 0 for v in row["reserved"])
    return {f: int(row[f]) for f in FIELDS}


def laid_out(bit_rows, pad=0, base=0):
    """[S, width] uint8 rows holding the packed bit_rows, as a view into a
    buffer of 0xFF: `base` bytes in front, stride = width + pad, every bit that
    is not one of a row's own set (the rest of its last byte, the bytes behind
    it, the bytes between rows).  Returns (view, bit counts, the buffer)."""
    S = len(bit_rows)
    width = max([1] + [(b.size + 7) // 8 for b in bit_rows])
    buf = np.full(base + S * (width + pad) + 8, 0xFF, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[base:], shape=(S, width), strides=(width + pad, 1))
    for s, b in enumerate(bit_rows):
        full = np.ones(8 * ((b.size + 7) // 8), np.uint8)
        full[: b.size] = b
        view[s, : full.size // 8] = np.packbits(full)
    return view, np.array([b.size for b in bit_rows], np.int64), buf


def host_rows(cs, pad=0, base=0, **params):
    """Q.ber_count over cases cs (one parameter set) in the given layout."""
    rx, n_rx, _ = laid_out([c.rx for c in cs], pad, base)
    ref, n_ref, _ = laid_out([c.ref for c in cs], pad, base)
    return Q.ber_count(rx, n_rx, ref, n_ref, **(params or cs[0].params))
