"""Geometry of the symbol-loop shapes (qpsk_demod_loop_shape), no device.

The two-slot sample ring (loop_variant 5, csrc/qpsk_loop.hip) keeps a stream's
backlog in the kPre samples loaded in front of each round, so its bounds are
inequalities between the shape's constants; the LDS figures decide how many
matched-filter workgroups of the next pipelined call share the CU.
"""
import math

import pytest

import qpsk_amd as Q

CU_LDS = 160 * 1024
CUS = 256


def alloc(nbytes, granule):
    return -(-nbytes // granule) * granule


def fir_lds(taps):
    """fir_tile_kernel's LDS tile: 2048 outputs + taps - 1 inputs, 8 pad slots per 64, float2."""
    nin = 2048 + taps - 1
    return 8 * (nin + (nin >> 6) * 8 + 8)


# the floor of each sps class a two-slot instantiation serves: its CAP must hold there
@pytest.mark.parametrize("sps,sps_floor", [(4.0, 4.0), (4.3478, 4.0), (7.99, 4.0), (8.0, 8.0), (30.0, 8.0)])
@pytest.mark.parametrize("want_syms", [False, True])
def test_two_slot_ring_inequalities(sps, sps_floor, want_syms):
    g = Q.loop_shape(5, 4096, sps, CUS, 0, want_syms)
    assert g["slots"] == 2 and g["prefix"] == 16
    assert g["lanes"] == g["streams"] <= 64
    kb, pre, cap = g["round"], g["prefix"], g["cap"]
    # every tap b - 1 .. b + 2 of a symbol of round r lies in [KB r - P, KB (r + 1))
    assert 0 < g["lag_max"] <= pre - 4
    lag = Q.loop_shape(5, 4096, sps_floor, CUS, 0, want_syms)["lag_max"]
    assert lag == pre - 4, "the CAP of the class holds the whole prefix at the class's smallest sps"
    # a round holds at most (KB + 4 + lag_max) / (sps - 0.1) + 1 symbols
    assert (cap - 1) * (sps_floor - 0.1) >= kb + 4 + lag
    assert (cap - 1) * (sps - 0.1) >= kb + 4 + g["lag_max"]
    assert (cap + 1) % 2 == 1, "odd symbol row stride"
    # one loader instruction moves 64 lanes x 16 B: the slot is whole 16-B pairs
    assert (kb + pre) % 2 == 0
    assert alloc(g["lds_bytes"], g["lds_granule"]) <= CU_LDS


@pytest.mark.parametrize("sps,taps,beside", [(4.0, 129, 1), (8.0, 65, 2)])
def test_two_slot_lds_leaves_room_for_the_matched_filter(sps, taps, beside):
    """64 x 64: one T = 129 FIR workgroup beside the sps >= 4 workgroup, two
    T = 65 beside the sps >= 8 one (bits only, portable trig)."""
    g = Q.loop_shape(5, 4096, sps, CUS, 0, False)
    assert (g["streams"], g["round"]) == (64, 64)
    assert g["fir_taps"] == taps and g["fir_beside"] == beside
    assert g["fir_lds_bytes"] == fir_lds(taps)
    gr = g["lds_granule"]
    assert alloc(g["lds_bytes"], gr) + beside * alloc(fir_lds(taps), gr) <= CU_LDS
    # with symbols no claim is made, but the workgroup itself fits
    gs = Q.loop_shape(5, 4096, sps, CUS, 0, True)
    assert gs["fir_beside"] == 0 and gs["lds_bytes"] > g["lds_bytes"]
    assert alloc(gs["lds_bytes"], gr) <= CU_LDS


def test_two_slot_lds_bytes():
    """tab 16 KB + float symbol slots + 2-byte decisions + counts + 64 rows of
    2 x (16 + 64) + 2 samples."""
    for sps, cap in ((4.0, 22), (8.0, 12)):
        g = Q.loop_shape(5, 4096, sps, CUS, 0, False)
        want = 16384 + 8 * 2 * 64 * (cap + 1) + 2 * 2 * 64 * (cap + 1) + 4 * (4 * 64 + 4) + 64 * 8 * 162
        assert g["cap"] == cap and g["lds_bytes"] == want


@pytest.mark.parametrize("variant,S,sps,trig,want", [
    # (streams, lanes, round, slots, prefix, cap): what the shapes use today
    (0, 256, 1.5, 0, (16, 16, 64, 4, 0, 80)),
    (5, 256, 1.5, 0, (16, 16, 64, 4, 0, 80)),
    (1, 256, 4.0, 0, (16, 16, 64, 4, 0, 40)),
    (2, 4096, 4.0, 0, (32, 32, 64, 4, 0, 28)),
    (2, 4096, 8.0, 0, (32, 32, 64, 4, 0, 14)),
    (2, 256, 2.0, 0, (32, 32, 64, 4, 0, 40)),
    (3, 256, 4.0, 0, (16, 16, 128, 4, 0, 72)),
    (4, 256, 8.0, 0, (24, 24, 128, 4, 0, 26)),
    (6, 256, 8.0, 0, (12, 32, 256, 4, 0, 51)),
    (7, 256, 8.0, 0, (6, 32, 512, 4, 0, 100)),
    (0, 256, 8.0, 0, (6, 32, 512, 4, 0, 100)),       # C2: qpsk_demod_pick_loop_variant -> 7
    (0, 2048, 8.0, 0, (12, 32, 256, 4, 0, 51)),
    (0, 256, 4.0, 0, (32, 32, 64, 4, 0, 28)),        # a small sps-4 batch keeps 32 x 64
    (0, 256, 2.0, 0, (32, 32, 64, 4, 0, 40)),
    (5, 256, 2.0, 0, (32, 32, 64, 4, 0, 40)),        # below sps 4 variant 5 runs as auto
    (5, 4096, 4.0, 1, (32, 32, 64, 4, 0, 28)),       # glibc trig pairs lanes: 32 streams
    (0, 4096, 4.0, 1, (32, 32, 64, 4, 0, 28)),
    (4, 256, 4.0, 0, (32, 32, 64, 4, 0, 28)),        # an sps >= 8 shape below sps 8 runs as auto
    (5, 70, 4.0, 0, (64, 64, 64, 2, 16, 22)),
    (5, 70, 8.0, 0, (64, 64, 64, 2, 16, 12)),
])
def test_shape_table(variant, S, sps, trig, want):
    g = Q.loop_shape(variant, S, sps, CUS, trig, False)
    assert (g["streams"], g["lanes"], g["round"], g["slots"], g["prefix"], g["cap"]) == want
    if g["slots"] == 4:
        assert g["lag_max"] == min(0.5 * g["round"], (g["cap"] - 1) * (sps - 0.1) - g["round"] - 4.0)


@pytest.mark.parametrize("S,sps,taps,cus,trig,two", [
    (4096, 4.0, 129, 256, 0, True),     # C3: the matched filter sets the step
    (8192, 4.0, 129, 256, 0, True),
    (4095, 4.0, 129, 256, 0, False),
    (3072, 4.0, 129, 256, 0, False),    # measured: the loop sets the step, 32 x 64 stays
    (256, 4.0, 129, 256, 0, False),
    (4096, 4.0, 33, 256, 0, False),     # a short filter: the loop sets the step
    (8192, 4.0, 65, 256, 0, True),
    (4096, 7.99, 129, 256, 0, True),
    (4096, 8.0, 65, 256, 0, False),     # C4: measured slower
    (8192, 8.0, 65, 256, 0, False),     # C5
    (4096, 3.99, 129, 256, 0, False),
    (4096, 4.0, 129, 256, 1, False),    # c3_glibc
    (4096, 4.0, 129, 0, 0, False),      # unknown CU count
    (4096, 4.0, 129, 1024, 0, False),   # a larger chip
    (16384, 4.0, 129, 1024, 0, True),
])
def test_automatic_shape_rule(S, sps, taps, cus, trig, two):
    """loop_variant 0: 64 x 64 on the two-slot ring at 4 <= sps < 8 where
    streams x taps >= 16 x 129 per CU, else what it was."""
    g = Q.loop_shape(0, S, sps, cus, trig, False, rrc_taps=taps)
    assert (g["slots"], g["streams"]) == ((2, 64) if two else (4, 32))
    # loop_variant 2 pins 32 x 64 whatever the rule says
    assert Q.loop_shape(2, S, sps, cus, trig, False, rrc_taps=taps)["slots"] == 4


def test_old_shapes_lds_bytes():
    """The C3 workgroup of DESIGN 3.2 (32 x 64, sps >= 4): float symbol slots,
    2-byte decisions, rows of 4 + 256 samples; two T = 129 FIR workgroups fit."""
    g = Q.loop_shape(2, 4096, 4.0, CUS, 0, False)
    assert g["lds_bytes"] == 16384 + 8 * 2 * 32 * 29 + 2 * 2 * 32 * 29 + 4 * (4 * 32 + 4) + 32 * 8 * 260
    assert g["fir_beside"] == 2 and g["fir_taps"] == 129
    assert alloc(g["lds_bytes"], g["lds_granule"]) + 2 * alloc(fir_lds(129), g["lds_granule"]) <= CU_LDS


def test_rejects_bad_arguments():
    with pytest.raises(ValueError):
        Q.loop_shape(8, 256, 4.0, CUS)
    with pytest.raises(ValueError):
        Q.loop_shape(0, 0, 4.0, CUS)
    with pytest.raises(ValueError):
        Q.loop_shape(0, 256, 4.0, CUS, costas_trig=2)
