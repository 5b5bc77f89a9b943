#!/usr/bin/env python3
"""What the format-tagged modulator costs on one MI355X, against the parent
commit's modulator.

    python tools/mod_bench.py --parent-lib <second build dir>/libqpsk_demod.so
    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- \\
        python tools/mod_bench.py --parent-lib ... --trace-plan DIR/plan.json
    python tools/mod_bench.py --merge-trace DIR

Writes one JSON file (--out, default profiles/mod_fmt_bench.json).  Two shapes:

  drop_in  S = 1, one 12 KB text frame (TSC, 0x02, text, 0x03) at sps 2, span 8,
           alpha 0.1: what one ModulateTextUtf8 of the reference program makes
  batch    S = 4096 rows of 2^16 dibits at sps 4, span 32 (the receive
           headline's filter)

Legs, alternated --rounds times in one run, every call on the modulator's own
stream bound to a torch stream:

  parent_cf32        the parent library's qpsk_mod_modulate, device rows: the yardstick
  cf32 cs16 cs8      this tree's qpsk_mod_modulate_fmt (FIXED, full scale), device rows
  peak_cs16          QPSK_MOD_NORM_PEAK, device rows
  host_*             the same four through host rows (pageable memory), fewer calls

All legs read the same device bit rows.  A call is timed twice: "device_ms"
between two events recorded on the stream in front of and behind the call
(its copies of counts and lengths included), "call_ms" on the host clock around
the call, which ends in the library's own synchronise.  The CF32 rows of the
two libraries are compared bit for bit before anything is timed.

Per kernel: the second command runs every device leg a few times under
rocprofv3 --kernel-trace and writes the order of the calls (--trace-plan); the
third folds the traced kernel times into the JSON (--merge-trace), matching
dispatches to calls by that order.
"""
from __future__ import annotations

import argparse
import csv
import ctypes as C
import glob
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qpsk-modulator-demodulator_amd"))

FS = 10_000_000
TSC = "11001010011101100100100110101100" + "01110100111001011010001101101001"
FMT = {"cf32": (0, "float32", 1.0), "cs16": (1, "int16", 32767.0), "cs8": (2, "int8", 127.0)}
SHAPES = {"drop_in": dict(streams=1, sps=2, span=8, alpha=0.1, what="one 12 KB text frame"),
          "batch": dict(streams=4096, sps=4, span=32, alpha=0.4000000059604645, what="2^16 dibits a row")}
DEVICE_LEGS = ["parent_cf32", "cf32", "cs16", "cs8", "peak_cs16"]
HOST_LEGS = ["host_cf32", "host_cs16", "host_cs8", "host_peak_cs16"]
KERNELS = re.compile(r"mod_(symbols|samples)_kernel")


class ModParams(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("symbol_rate", C.c_int32), ("rrc_alpha", C.c_double),
                ("rrc_span", C.c_int32), ("differential", C.c_int32), ("device", C.c_int32),
                ("reserved", C.c_int32 * 7)]


class Library:
    """One libqpsk_demod.so and a modulator handle of it on a torch stream."""

    def __init__(self, path, new):
        self.L = C.CDLL(path)
        self.new = new
        L = self.L
        L.qpsk_last_error.restype = C.c_char_p
        L.qpsk_mod_params_init.argtypes = [C.POINTER(ModParams), C.c_int32, C.c_int32]
        L.qpsk_mod_create.argtypes = [C.POINTER(ModParams), C.c_char_p, C.POINTER(C.c_void_p)]
        L.qpsk_mod_destroy.argtypes = [C.c_void_p]
        L.qpsk_mod_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.qpsk_mod_output_floats.argtypes = [C.c_void_p, C.c_int64, C.c_int32]
        L.qpsk_mod_output_floats.restype = C.c_int64
        call = [C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
        L.qpsk_mod_modulate.argtypes = [C.c_void_p] + call
        if new:
            L.qpsk_mod_modulate_fmt.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_float] + call + [C.c_void_p]

    def handle(self, shape, stream):
        p = ModParams()
        self.L.qpsk_mod_params_init(C.byref(p), FS, FS // shape["sps"])
        p.rrc_alpha, p.rrc_span = shape["alpha"], shape["span"]
        h = C.c_void_p()
        self.check(self.L.qpsk_mod_create(C.byref(p), TSC.encode(), C.byref(h)))
        self.check(self.L.qpsk_mod_set_stream(h, C.c_void_p(stream.cuda_stream)))
        return h

    def check(self, rc):
        if rc != 0:
            raise RuntimeError(f"status {rc}: {self.L.qpsk_last_error().decode(errors='replace')}")


def inputs(name, shape):
    """Packed bit rows [S, B] and their counts: the same for every leg."""
    rng = np.random.default_rng(7)
    if name == "drop_in":
        text = bytes(rng.integers(0x20, 0x7F, 12 * 1024, dtype=np.uint8))
        rows = np.frombuffer(b"\x02" + text + b"\x03", np.uint8)[None, :].copy()
    else:
        rows = rng.integers(0, 256, (shape["streams"], 2 * (1 << 16) // 8), dtype=np.uint8)
    return rows, np.full(rows.shape[0], 8 * rows.shape[1], np.int64)


class Bench:
    def __init__(self, torch, name, shape, this_lib, parent_lib):
        self.torch, self.name, self.shape = torch, name, shape
        self.stream = torch.cuda.Stream()
        self.libs = {"this": this_lib, "parent": parent_lib}
        self.h = {k: lib.handle(shape, self.stream) for k, lib in self.libs.items()}
        rows, nb = inputs(name, shape)
        self.S = rows.shape[0]
        self.rows_host, self.nb_host = rows, nb
        self.rows, self.nb = torch.from_numpy(rows).cuda(), torch.from_numpy(nb).cuda()
        self.n_out = torch.zeros(self.S, dtype=torch.int64, device="cuda")
        self.peak = torch.zeros(self.S, dtype=torch.float32, device="cuda")
        self.width = int(this_lib.L.qpsk_mod_output_floats(self.h["this"], int(nb[0]), 1))
        self.pitch = (self.width + 15) // 16 * 16       # 16-byte rows in every format
        self.out = {}
        self.host_out = {}
        torch.cuda.synchronize()

    def close(self):
        for k, lib in self.libs.items():
            lib.L.qpsk_mod_destroy(self.h[k])

    def device_out(self, leg):
        fmt = leg.split("_")[-1]
        key = "parent" if leg.startswith("parent") else fmt
        if key not in self.out:
            self.out[key] = self.torch.zeros((self.S, self.pitch), dtype=getattr(self.torch, FMT[fmt][1]), device="cuda")
            self.torch.cuda.synchronize()
        return self.out[key]

    def call(self, leg):
        """One call of a leg; returns its status."""
        host = leg.startswith("host_")
        fmt = leg.split("_")[-1]
        tag, dtype, full = FMT[fmt]
        norm = 1 if "peak" in leg else 0
        if host:
            if fmt not in self.host_out:
                self.host_out[fmt] = np.zeros((self.S, self.width), dtype=dtype)
            out = self.host_out[fmt]
            n_out, peak = np.zeros(self.S, np.int64), np.zeros(self.S, np.float32)
            return self.libs["this"].L.qpsk_mod_modulate_fmt(
                self.h["this"], tag, norm, full, self.S, self.rows_host.ctypes.data, self.rows_host.shape[1],
                self.nb_host.ctypes.data, 1, 0, out.ctypes.data, out.shape[1], n_out.ctypes.data, peak.ctypes.data)
        out = self.device_out(leg)
        tail = (self.S, self.rows.data_ptr(), self.rows.stride(0), self.nb.data_ptr(), 1, 1, out.data_ptr(), out.stride(0),
                self.n_out.data_ptr())
        if leg.startswith("parent"):
            return self.libs["parent"].L.qpsk_mod_modulate(self.h["parent"], *tail)
        return self.libs["this"].L.qpsk_mod_modulate_fmt(self.h["this"], tag, norm, full, *tail, self.peak.data_ptr())

    def timed(self, leg, calls):
        torch = self.torch
        dev_ms, call_ms = [], []
        for _ in range(calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(self.stream)
            t0 = time.perf_counter()
            rc = self.call(leg)
            call_ms.append((time.perf_counter() - t0) * 1e3)
            b.record(self.stream)
            b.synchronize()
            if rc != 0:
                raise RuntimeError(f"{leg}: status {rc}")
            dev_ms.append(a.elapsed_time(b))
        return dev_ms, call_ms

    def same_as_parent(self):
        for leg in ("parent_cf32", "cf32"):
            if self.call(leg) != 0:
                raise RuntimeError(leg)
        self.torch.cuda.synchronize()
        return bool(self.torch.equal(self.out["parent"].view(self.torch.int32), self.out["cf32"].view(self.torch.int32)))


def med(v):
    return round(statistics.median(v), 4)


def run(a, torch, this_lib, parent_lib):
    res = {"what": "qpsk_mod_modulate_fmt of this tree against qpsk_mod_modulate of the parent commit's library, one "
                   "MI355X, identical device bit rows, legs alternated, times in ms a call",
           "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "shapes": {}}
    for name, shape in SHAPES.items():
        b = Bench(torch, name, shape, this_lib, parent_lib)
        calls = a.calls_small if name == "drop_in" else a.calls_batch
        host_calls = a.calls_small if name == "drop_in" else a.calls_host
        r = {"shape": dict(shape), "bits_a_row": int(b.nb_host[0]), "complex_samples_a_row": b.width // 2,
             "cf32_rows_equal_the_parents_bit_for_bit": b.same_as_parent(), "calls_a_round": calls,
             "host_calls_a_round": host_calls, "legs": {}}
        for leg in DEVICE_LEGS + HOST_LEGS:          # every shape warmed before anything is timed
            b.timed(leg, 2 if not leg.startswith("host_") or name == "drop_in" else 1)
        rounds = {leg: [] for leg in DEVICE_LEGS + HOST_LEGS}
        for _ in range(a.rounds):
            for leg in DEVICE_LEGS + HOST_LEGS:
                dev_ms, call_ms = b.timed(leg, host_calls if leg.startswith("host_") else calls)
                rounds[leg].append({"device_ms": med(dev_ms), "call_ms": med(call_ms), "device_ms_min": round(min(dev_ms), 4),
                                    "device_ms_max": round(max(dev_ms), 4)})
        for leg, rr in rounds.items():
            r["legs"][leg] = {"rounds": rr, "device_ms": med([x["device_ms"] for x in rr]),
                              "call_ms": med([x["call_ms"] for x in rr])}
        L = r["legs"]
        ratio = lambda x, y, k="device_ms": round(L[x][k] / L[y][k], 3)
        spread = [x["device_ms"] for x in L["parent_cf32"]["rounds"]]
        r["summary"] = {
            "parent_cf32_over_this_cf32_device": ratio("parent_cf32", "cf32"),
            "parent_cf32_over_this_cf32_call": ratio("parent_cf32", "cf32", "call_ms"),
            "parents_own_rounds_apart_percent": round(100 * (max(spread) - min(spread)) / min(spread), 2),
            "cf32_over_cs16_device": ratio("cf32", "cs16"), "cf32_over_cs8_device": ratio("cf32", "cs8"),
            "peak_cs16_over_cs16_device": ratio("peak_cs16", "cs16"),
            "host_cf32_over_host_cs16_call": ratio("host_cf32", "host_cs16", "call_ms"),
            "host_cf32_over_host_cs8_call": ratio("host_cf32", "host_cs8", "call_ms"),
            "host_peak_cs16_over_host_cs16_call": ratio("host_peak_cs16", "host_cs16", "call_ms"),
            "host_cf32_over_device_cf32_call": ratio("host_cf32", "cf32", "call_ms")}
        res["shapes"][name] = r
        b.close()
        del b
        torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v["summary"] for k, v in res["shapes"].items()}, indent=1))


def trace_plan(a, torch, this_lib, parent_lib):
    """Every device leg a few times, under the profiler; the order goes to a file."""
    plan = []
    for name, shape in SHAPES.items():
        b = Bench(torch, name, shape, this_lib, parent_lib)
        for leg in DEVICE_LEGS:
            b.timed(leg, a.trace_calls)
            plan.append({"shape": name, "leg": leg, "calls": a.trace_calls, "kernels_a_call": 3 if "peak" in leg else 2})
        b.close()
        del b
        torch.cuda.empty_cache()
    with open(a.trace_plan, "w") as f:
        json.dump(plan, f, indent=1)


def merge_trace(a):
    plan = json.load(open(os.path.join(a.merge_trace, "plan.json")))
    rows = []
    for fn in glob.glob(os.path.join(a.merge_trace, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(fn, newline="")):
            m = KERNELS.search(row.get("Kernel_Name", ""))
            if m:
                rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), "mod_%s_kernel" % m.group(1)))
    rows.sort()
    want = sum(p["calls"] * p["kernels_a_call"] for p in plan)
    if len(rows) != want:
        raise SystemExit(f"{len(rows)} modulator dispatches in the trace, the plan has {want}")
    res = json.load(open(a.out))
    at = 0
    for p in plan:
        per = [[] for _ in range(p["kernels_a_call"])]
        for _ in range(p["calls"]):
            for k in range(p["kernels_a_call"]):
                s, e, kname = rows[at]
                per[k].append((kname, (e - s) / 1e6))
                at += 1
        names = ["symbols", "samples"] if p["kernels_a_call"] == 2 else ["symbols", "samples_max_pass", "samples"]
        out = {}
        for k, label in enumerate(names):
            assert all(kn == ("mod_symbols_kernel" if k == 0 else "mod_samples_kernel") for kn, _ in per[k]), (p, label)
            v = [t for _, t in per[k][1:]] or [t for _, t in per[k]]     # the first call of a leg is left out
            out[label + "_ms"] = round(statistics.median(v), 4)
        res["shapes"][p["shape"]]["legs"][p["leg"]]["kernels"] = out
    res["kernels_from"] = "rocprofv3 --kernel-trace, a run of its own: medians over %d calls a leg, the first left out" % (
        plan[0]["calls"])
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({n: {leg: v.get("kernels") for leg, v in s["legs"].items() if "kernels" in v}
                      for n, s in res["shapes"].items()}, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libqpsk_demod.so of the parent commit, from a second build directory")
    ap.add_argument("--this-lib", default=os.path.join(ROOT, "qpsk-modulator-demodulator_amd", "_build", "libqpsk_demod.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mod_fmt_bench.json"))
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--calls-small", type=int, default=200)
    ap.add_argument("--calls-batch", type=int, default=8)
    ap.add_argument("--calls-host", type=int, default=2)
    ap.add_argument("--trace-plan", help="run the device legs for a kernel trace and write their order here")
    ap.add_argument("--trace-calls", type=int, default=4)
    ap.add_argument("--merge-trace", help="directory of the trace and its plan.json: fold kernel times into --out")
    a = ap.parse_args()
    if a.merge_trace:
        return merge_trace(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("--parent-lib: build the parent commit's library in a second directory first")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mod_bench needs an MI355X: there is nothing to measure without one")
    torch.cuda.init()   # torch's HIP runtime first, then the libraries
    this_lib, parent_lib = Library(a.this_lib, True), Library(a.parent_lib, False)
    if a.trace_plan:
        return trace_plan(a, torch, this_lib, parent_lib)
    run(a, torch, this_lib, parent_lib)


if __name__ == "__main__":
    main()
