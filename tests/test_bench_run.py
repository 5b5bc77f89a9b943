"""bench.py's plain run and --dump-outputs.

CPU: which rows the dump keeps (shape only, seeded, first and last stream
always, under 64 MB at the headline shape) and what it writes (float arrays,
nothing past a row's n_bits).  GPU: one plain run of a small C2-shaped batch in
a child process: the line carries the timed steps only, and the dumped rows
are the oracle's bits after the same warmup + timed calls.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle as O
import qpsk_amd as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_argv, sys.argv = sys.argv, sys.argv[:1]
import bench  # noqa: E402
sys.argv = _argv


def test_dump_rows_is_a_fixed_bounded_sample():
    assert bench.dump_rows(256, 32832) == list(range(256))          # C2: every row fits
    assert bench.dump_rows(1, 64) == [0] and bench.dump_rows(2, 1 << 26) == [0, 1]
    S, B = 4096, 65664                                               # C3's bit rows: 269 MB as bytes
    idx = bench.dump_rows(S, B)
    assert idx == bench.dump_rows(S, B)
    assert idx[0] == 0 and idx[-1] == S - 1 and idx == sorted(set(idx))
    assert 100 < len(idx) < S
    assert 4 * B * len(idx) + 8 * len(idx) + 8 * S + 3 * 128 <= 64_000_000


def test_dump_outputs_writes_float_arrays_of_the_valid_bits(tmp_path):
    rng = np.random.default_rng(3)
    raw = rng.integers(0, 256, (5, 24), dtype=np.uint8)
    nb = np.array([0, 1, 64, 101, 192], np.int64)
    out = tmp_path / "sub" / "dir"
    bench.dump_outputs(str(out), torch.from_numpy(raw), torch.from_numpy(nb))
    assert sorted(os.listdir(out)) == ["bits.npy", "bits_rows.npy", "n_bits.npy"]
    bits, rows, n_bits = (np.load(out / f) for f in ("bits.npy", "bits_rows.npy", "n_bits.npy"))
    assert bits.dtype == np.float32 and rows.dtype == np.float64 and n_bits.dtype == np.float64
    assert rows.tolist() == [0, 1, 2, 3, 4] and n_bits.tolist() == nb.tolist()
    for s in range(5):
        want = np.unpackbits(raw[s])
        want[nb[s]:] = 0
        assert np.array_equal(np.unpackbits(bits[s].astype(np.uint8)), want), s


STREAMS, SAMPLES, STEPS, WARMUP = 24, 1 << 16, 2, 1


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_call(tmp_path):
    cfg = bench.CONFIGS["c2"]
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c2",
           "--streams", str(STREAMS), "--samples", str(SAMPLES), "--steps", str(STEPS),
           "--warmup", str(WARMUP), "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["ms_per_step"] > 0
    assert line["unit"] == "MSa/s" and line["higher_is_better"] is True and line["dtype"] == "f32/f64"
    assert line["value"] == pytest.approx(STREAMS * SAMPLES / (line["ms_per_step"] * 1e-3) / 1e6, rel=1e-3)
    # nothing but the timed steps ran, and no side file was written
    assert "sub_records" not in line and line["parity"] == "not checked" and line["cpu_baseline"] is None
    assert line["detail"] is None
    assert sorted(os.listdir(tmp_path)) == ["bits.npy", "bits_rows.npy", "n_bits.npy"]

    bits, rows, n_bits = (np.load(tmp_path / f) for f in ("bits.npy", "bits_rows.npy", "n_bits.npy"))
    assert bits.dtype == np.float32 and n_bits.dtype == np.float64
    assert rows.tolist() == list(range(STREAMS)) and n_bits.shape == (STREAMS,)
    rs = bench.FS // cfg["sps"]
    iq, _ = Q.synth_generate(STREAMS, SAMPLES, bench.FS, rs, rrc_alpha=bench.ALPHA, rrc_span=cfg["span"],
                             seed=0x5159534B, lo_ppm=1.0, device=0)
    host = iq.cpu().numpy()
    for s in (0, 1, STREAMS // 2, STREAMS - 1):
        d = O.OracleDemod(bench.FS, rs, bench.ALPHA, cfg["span"], trig=O.TRIG_LIBM, ring_capacity=4096)
        for _ in range(WARMUP + STEPS):
            ref, _, _ = d.demodulate_ex(host[s])
        assert int(n_bits[s]) == len(ref) > 0, s
        assert Q.unpack_bits(bits[s].astype(np.uint8), len(ref)) == ref, s
        assert not bits[s, (len(ref) + 7) // 8:].any(), s
