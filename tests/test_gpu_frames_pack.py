"""qpsk_frames_pack_device against its packing rule computed in numpy
(frame_cases.pack_rule): all of offsets, head and packed[0:total] byte for
byte, the padding zeros included.

The payload rows are filled with 0xAA past each frame's bytes, so a tail word
copied without its mask shows; packed, offsets and head are pre-filled with a
sentinel, so a word written past the total, or a refused call that wrote,
shows as well.  S crosses the wave (64) and scan-block (1024) edges.
"""
import numpy as np
import pytest

import qpsk_amd as Q
from frame_cases import pack_rule, packed_bytes
from gpu_harness import dev  # noqa: F401

SENTINEL = 0x5C
STREAMS = [1, 63, 64, 65, 300, 1025]


def lengths_for(S, P, kind, seed):
    """n_payload of one case.  "mixed": drawn from the edge lengths, with runs
    of zeros; "single": one frame, the rest empty; "full": every stream holds
    a frame."""
    rng = np.random.default_rng(seed)
    edge = np.array([0, 1, 15, 16, 17, P - 1, P, P + 1, 5 * P], np.int64)
    if kind == "single":
        L = np.zeros(S, np.int64)
        L[S // 2] = P - 1
        return L
    if kind == "full":
        return edge[rng.integers(1, edge.size, S)]
    L = edge[rng.integers(0, edge.size, S)]
    for _ in range(max(S // 20, 1)):                  # runs of empty streams
        a = int(rng.integers(0, S))
        L[a: a + int(rng.integers(1, min(40, S // 4 + 2)))] = 0
    return L


def run_pack(torch, L, P, C, cap_alloc=None):
    """One call on a stream of its own; (rows, offsets, head, packed) as numpy."""
    S = L.size
    rng = np.random.default_rng(1000 + S + P)
    rows = rng.integers(0, 256, (S, P), dtype=np.uint8)
    k = np.minimum(L, P)
    rows[np.arange(P)[None, :] >= k[:, None]] = 0xAA   # stale bytes past the frame
    alloc = max(C if cap_alloc is None else cap_alloc, 16)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        pay = torch.from_numpy(rows).cuda()
        npay = torch.from_numpy(L).cuda()
        packed = torch.full((alloc + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        offs = torch.full((S,), -7, dtype=torch.int64, device="cuda")
        head = torch.full((2,), -7, dtype=torch.int64, device="cuda")
        Q.frames_pack_device(pay, npay, packed, offs, head, st.cuda_stream, packed_cap=C)
        out = offs.cpu().numpy(), head.cpu().numpy(), packed.cpu().numpy()
    return (rows,) + out


def check(torch, L, P, C):
    rows, offs, head, packed = run_pack(torch, L, P, C)
    k, a, want_off, total, flags = pack_rule(L, P, C)
    assert np.array_equal(offs, want_off), (L.size, P, C)
    assert (int(head[0]), int(head[1])) == (total, flags), (L.size, P, C)
    assert np.array_equal(packed[:total], packed_bytes(rows, L, P, C)), (L.size, P, C)
    assert (packed[total:] == SENTINEL).all(), "a word written past the total"
    return total, flags


@pytest.mark.gpu
@pytest.mark.parametrize("P", [16, 48])
@pytest.mark.parametrize("S", STREAMS)
def test_pack_matches_the_rule(dev, S, P):
    """Mixed lengths at the four capacities: unlimited, exactly the total, one
    word short of it, and none."""
    L = lengths_for(S, P, "mixed", 10 * S + P)
    if not L.any():
        L[0] = 17
    unlimited = S * P
    total, flags = check(dev, L, P, unlimited)
    assert total > 0 and not flags & 2
    assert flags & 1 or S < 20, "a truncated frame among the lengths"
    assert check(dev, L, P, total) == (total, flags)
    t2, f2 = check(dev, L, P, total - 16)
    assert t2 < total and f2 & 2
    assert check(dev, L, P, 0) == (0, flags | 2)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["single", "full"])
@pytest.mark.parametrize("S", STREAMS)
def test_pack_single_frame_and_every_stream(dev, S, kind):
    P = 48
    L = lengths_for(S, P, kind, 77 + S)
    total, flags = check(dev, L, P, S * P)
    if kind == "single":
        assert (total, flags) == (48, 0)
    else:
        assert total >= 16 * S
        check(dev, L, P, (total // 2) // 16 * 16)   # the capacity runs out half way


@pytest.mark.gpu
def test_pack_of_no_frames(dev):
    for S in (1, 65, 1025):
        assert check(dev, np.zeros(S, np.int64), 16, 16 * S) == (0, 0)


@pytest.mark.gpu
def test_bad_arguments_are_refused_and_write_nothing(dev):
    torch = dev
    S, P = 8, 32
    pay = torch.full((S, P), 1, dtype=torch.uint8, device="cuda")
    npay = torch.full((S,), 5, dtype=torch.int64, device="cuda")
    packed = torch.full((S * P + 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    # views one int32 in: 4 mod 8
    offs = torch.full((2 * S + 2,), -7, dtype=torch.int32, device="cuda")
    head = torch.full((6,), -7, dtype=torch.int32, device="cuda")
    ok_offs, ok_head = offs[: 2 * S].view(torch.int64), head[:4].view(torch.int64)
    torch.cuda.synchronize()
    L = Q.lib()
    call = lambda **kw: L.qpsk_frames_pack_device(  # noqa: E731
        pay.data_ptr(), kw.get("P", P), npay.data_ptr(), kw.get("S", S), kw.get("packed", packed.data_ptr()),
        kw.get("C", S * P), kw.get("offs", ok_offs.data_ptr()), kw.get("head", ok_head.data_ptr()), None)
    assert packed.data_ptr() % 16 == 0 and ok_offs.data_ptr() % 8 == 0
    for kw in (dict(P=0), dict(P=-32), dict(P=24), dict(C=-16), dict(C=40), dict(packed=packed.data_ptr() + 8),
               dict(packed=packed.data_ptr() + 1), dict(offs=offs.data_ptr() + 4), dict(head=head.data_ptr() + 4),
               dict(S=0), dict(S=-1)):
        assert call(**kw) == Q.QPSK_ERR_ARGUMENT, kw
    torch.cuda.synchronize()
    assert (packed == SENTINEL).all() and (offs == -7).all() and (head == -7).all(), "a refused call wrote"
    assert call() == Q.QPSK_OK
    torch.cuda.synchronize()
    assert ok_head.cpu().tolist() == [16 * S, 0] and ok_offs.cpu().tolist() == [16 * s for s in range(S)]
