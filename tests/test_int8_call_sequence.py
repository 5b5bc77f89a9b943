"""The 8-bit call sequence of tests/gpu_format_cases.py is what its cases need (no GPU):
with 8-sample loads every residue of a row's length mod 8 must end a row past
the first tile."""
from gpu_harness import SPECIALISED, TILE, calls_for


def test_call_sequence_ends_rows_at_every_residue_mod_8():
    for sps, span in SPECIALISED:
        calls = calls_for(sps * span + 1)
        total = sum(c[0] for c in calls)
        for s in range(6):
            assert sum(c[s] for c in calls) == total
            assert {c[s] % 8 for c in calls if c[s] >= TILE - 1} == set(range(8))
