#!/usr/bin/env python3
"""Frame loss against noise and against LO instability from thousands of
independent streams on one MI355X, with no sample leaving the device: the
reference's end-to-end test (testAtDataLevel.cs:24-46, with
testFullDemodChain.cs:73's noise) at batch size.

Per point a fresh channel, demodulator state and framer; then --frames rounds
in which every one of the C3 batch's 4096 streams (sps 4, 129 taps) sends one
frame of its own random payload:

    qpsk_mod_modulate_bytes_fmt   TSC | MESSAGE_START | payload | MESSAGE_STOP, device rows
    qpsk_channel_apply_fmt        the LO pair (and the noise), in place
    qpsk_demod_process_fmt        all loop state carried from frame to frame
    qpsk_tsc_find_device, qpsk_framer_dev_push   DeModulateBytes' framer

A frame counts as received when the framer returns exactly the payload sent in
that round.  The comparison runs on the device; one count a round comes back.
The first --skip rounds (acquisition) are reported apart.

Two sweeps: frame loss against noise_rms at 1 ppm, and against ppm (both LOs)
with no noise.  Writes one JSON file (--out, default profiles/fer_curve.json).
The values are recorded as measured; nothing here asserts them.

--clock-ppm adds a third axis (off by default, the two sweeps above are then as
they were): the propagation path (qpsk_path_apply_fmt) goes between the
modulator and the channel with every stream's sample clock off by that many
ppm (tau0 = 0.5, one unit tap, no noise), once beside LOs at 1 ppm and once
beside LOs off by the same |ppm| as the clock, as one oscillator would have
them.  A round then hands the demodulator what the path emitted in it.
profiles/fer_curve_clock.json: --noise-rms "" --ppm "" --clock-ppm -100,...,100.

--wideband M (off by default, everything above is then as it was) runs the same
two sweeps at wideband: the streams are the carriers of --streams / M bands, so
the M carriers of a band share one LO pair and one sample clock, as they do
behind a real radio.  A round is

    qpsk_mod_modulate_bytes_fmt   one frame a carrier at rate 2 fs / M, sps 4
    qpsk_sfb_apply_fmt            M rows into one wideband row at fs (K = 8, scale_out = M / 2)
    qpsk_path_apply_fmt           the band's sample clock, off by the point's ppm (tau0 = --tau0, default 0.5)
    qpsk_channel_apply_fmt        the band's LO pair at the same ppm, and the noise, in place
    qpsk_pfb_apply_fmt            the wideband row back into M rows
    qpsk_demod_process_fmt, qpsk_tsc_find_device, qpsk_framer_dev_push

with 64 zero samples behind every carrier's frame, so that the 2K samples a row
is late through bank and channeliser stay inside the round.  noise_rms is the
noise of the wideband row, on which a carrier keeps its modulator amplitude.
CF32 rows only.  Default --out: profiles/fer_curve_wideband.json.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "qpsk-modulator-demodulator_amd"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FS = 10_000_000
ALPHA = 0.4000000059604645
C3 = dict(streams=4096, sps=4, span=32)
TSC = "11001010011101100100100110101100" + "01110100111001011010001101101001"
START, STOP = b"MESSAGE_START", b"MESSAGE_STOP"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="default: profiles/fer_curve.json (fer_curve_wideband.json with --wideband)")
    ap.add_argument("--streams", type=int, default=C3["streams"])
    ap.add_argument("--payload-bytes", type=int, default=48)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--skip", type=int, default=4)
    ap.add_argument("--noise-rms", default="0,0.05,0.1,0.15,0.2,0.25,0.3,0.4,0.5")
    ap.add_argument("--ppm", default="0,1,2,5,10,20,50,100")
    ap.add_argument("--fmt", default="cf32", choices=["cf32", "cs16", "cs8"])
    ap.add_argument("--clock-ppm", default="", help="sample-clock offsets, ppm (default: no clock sweep)")
    ap.add_argument("--wideband", type=int, default=0, metavar="M",
                    help="carriers a band: the sweeps through synthesis bank, path, channel and channeliser (default: off)")
    ap.add_argument("--tau0", type=float, default=0.5, help="with --wideband: where the band's sample clock starts")
    args = ap.parse_args()
    clocks = [float(v) for v in args.clock_ppm.split(",") if v]
    args.out = args.out or os.path.join(ROOT, "profiles", "fer_curve_wideband.json" if args.wideband else "fer_curve.json")

    import torch
    import qpsk_amd as Q
    torch.cuda.init()
    dev = torch.device("cuda", 0)
    if args.wideband:
        return wideband(args, torch, Q, dev)
    S, P, sps, span = args.streams, args.payload_bytes, C3["sps"], C3["span"]
    rs = FS // sps
    full = {"cf32": 1.0, "cs16": 32767.0, "cs8": 127.0}[args.fmt]
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    m = Q.QPSKModulator(FS, rs, ALPHA, span, tsc=TSC, device=dev.index)
    n = m.output_floats(8 * (len(START) + P + len(STOP))) // 2
    pitch = (n + 7) // 8 * 8
    if clocks:   # what the path can emit in a round
        pitch = (Q.path_out_bound(Q.path_params(clock_ppm=max(abs(c) for c in clocks)), n) + 7) // 8 * 8
    d = Q.BatchDemodulator(S, Q.params(FS, rs, ALPHA, span, device=dev.index, max_samples_per_call=pitch))
    fr = Q.DeviceFramer(S, START, STOP, ring_capacity=1 << 16, device=dev.index)
    for h in (m, d, fr):
        h.set_stream(stream.cuda_stream)
    fresh = d.get_state()
    rows = torch.zeros((S, 2 * pitch), dtype=Q._torch_dtype(args.fmt), device=dev)
    prop = torch.zeros_like(rows) if clocks else None
    n_out = torch.zeros(S, dtype=torch.int64, device=dev)
    plen = torch.full((S,), P, dtype=torch.int64, device=dev)
    ms = d.max_symbols(pitch)
    bits = torch.zeros((S, (2 * ms + 7) // 8 + 8), dtype=torch.uint8, device=dev)
    nbits = torch.zeros(S, dtype=torch.int64, device=dev)
    offs = torch.zeros(S, dtype=torch.int64, device=dev)
    pay = torch.zeros((S, 256), dtype=torch.uint8, device=dev)
    npay = torch.zeros(S, dtype=torch.int64, device=dev)
    gen = torch.Generator(device=dev)
    rec = {"device": torch.cuda.get_device_name(dev), "streams": S, "sps": sps, "taps": sps * span + 1, "fmt": args.fmt,
           "payload_bytes": P, "samples_per_frame": n, "frames": args.frames, "skip": args.skip, "lo_hz": 100e6,
           "noise_sweep": [], "ppm_sweep": []}

    def point(ppm, rms, clock=None):
        d.set_state(fresh)
        fr.reset_streams(range(S))
        ch = Q.Channel(S, sample_rate=float(FS), tx_ppm=ppm, rx_ppm=ppm, noise_rms=rms, noise_seed=11, device=dev.index)
        ch.set_stream(stream.cuda_stream)
        pa = None
        if clock is not None:
            pa = Q.Path(S, clock_ppm=clock, tau0=0.5, device=dev.index)
            pa.set_stream(stream.cuda_stream)
        gen.manual_seed(1234)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        good = []
        for _ in range(args.frames):
            sent = torch.randint(0, 256, (S, P), dtype=torch.uint8, device=dev, generator=gen)
            m.modulate_bytes_device(sent, plen, START, STOP, rows, n_out, fmt=args.fmt, scale=full)
            x, k = rows, n
            if pa is not None:   # one clock for all streams: they emit alike
                x, k = prop, int(pa.apply_device(rows, n, prop, fmt=args.fmt, scale_out=full)[0])
            ch.apply_device(x, k, fmt=args.fmt)
            d.process_device_fmt(x, k, bits, nbits, args.fmt)
            Q.tsc_find_device(bits, nbits, TSC, offs, stream.cuda_stream)
            fr.push(bits, nbits, pay, npay, offs)
            good.append(((npay == P) & (pay[:, :P] == sent).all(dim=1)).sum())
        e1.record(stream)
        e1.synchronize()
        good = [int(g) for g in good]
        ch.close()
        if pa is not None:
            pa.close()
        after = good[args.skip:]
        return dict(**({} if clock is None else {"clock_ppm": clock}), ppm=ppm, noise_rms=rms, frames_received_per_round=good, frames_sent_after_skip=S * len(after),
                    frames_lost_after_skip=S * len(after) - sum(after),
                    frame_loss_after_skip=round(1.0 - sum(after) / (S * len(after)), 6),
                    ms=round(e0.elapsed_time(e1), 1))

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")

    for rms in (float(v) for v in args.noise_rms.split(",") if v):
        rec["noise_sweep"].append(point(1.0, rms))
        print(json.dumps(rec["noise_sweep"][-1]), flush=True)
        save()
    for ppm in (float(v) for v in args.ppm.split(",") if v):
        rec["ppm_sweep"].append(point(ppm, 0.0))
        print(json.dumps(rec["ppm_sweep"][-1]), flush=True)
        save()
    if clocks:
        rec["clock_sweep"] = []
    for clock in clocks:
        for ppm in (1.0, abs(clock)):
            rec["clock_sweep"].append(point(ppm, 0.0, clock))
            print(json.dumps(rec["clock_sweep"][-1]), flush=True)
            save()
    m.close()
    d.close()


def wideband(args, torch, Q, dev):
    """The two sweeps with the streams as the carriers of --streams / M bands."""
    M, K, tail = args.wideband, 8, 64
    D = M // 2
    if args.fmt != "cf32" or args.clock_ppm or args.streams % M:
        raise SystemExit("--wideband takes CF32 rows, no --clock-ppm, and --streams a multiple of M")
    S, B, P, sps, span = args.streams, args.streams // M, args.payload_bytes, C3["sps"], C3["span"]
    fs_ch, rs = 2 * FS // M, FS // (2 * M)
    max_ppm = max([1.0] + [float(v) for v in args.ppm.split(",") if v])
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    m = Q.QPSKModulator(fs_ch, rs, ALPHA, span, tsc=TSC, device=dev.index)
    n = m.output_floats(8 * (len(START) + P + len(STOP))) // 2 + tail      # frames of the bank a round
    sf = Q.SynthesisBank(B, channels=M, taps_per_branch=K, device=dev.index)
    pf = Q.Channeliser(B, channels=M, taps_per_branch=K, gain=1.0, device=dev.index)
    wide_cap = Q.path_out_bound(Q.path_params(clock_ppm=max_ppm), n * D)
    cap = (pf.out_bound(wide_cap) + 7) // 8 * 8
    d = Q.BatchDemodulator(S, Q.params(fs_ch, rs, ALPHA, span, device=dev.index, max_samples_per_call=cap))
    fr = Q.DeviceFramer(S, START, STOP, ring_capacity=1 << 16, device=dev.index)
    for h in (m, sf, pf, d, fr):
        h.set_stream(stream.cuda_stream)
    fresh = d.get_state()
    rows = torch.zeros((S, 2 * n), dtype=torch.float32, device=dev)         # the tail stays zero
    wide = torch.zeros((B, 2 * n * D), dtype=torch.float32, device=dev)
    prop = torch.zeros((B, 2 * wide_cap), dtype=torch.float32, device=dev)
    chans = torch.zeros((S, 2 * cap), dtype=torch.float32, device=dev)
    n_out = torch.zeros(S, dtype=torch.int64, device=dev)
    plen = torch.full((S,), P, dtype=torch.int64, device=dev)
    ms = d.max_symbols(cap)
    bits = torch.zeros((S, (2 * ms + 7) // 8 + 8), dtype=torch.uint8, device=dev)
    nbits = torch.zeros(S, dtype=torch.int64, device=dev)
    offs = torch.zeros(S, dtype=torch.int64, device=dev)
    pay = torch.zeros((S, 256), dtype=torch.uint8, device=dev)
    npay = torch.zeros(S, dtype=torch.int64, device=dev)
    gen = torch.Generator(device=dev)
    rec = {"device": torch.cuda.get_device_name(dev), "streams": S, "bands": B, "channels": M, "taps_per_branch": K,
           "sps": sps, "taps": sps * span + 1, "fmt": "cf32", "payload_bytes": P, "frames_per_round": n, "tail": tail,
           "wideband_samples_per_round": n * D, "tau0": args.tau0, "frames": args.frames, "skip": args.skip, "lo_hz": 100e6,
           "noise_sweep": [], "ppm_sweep": []}

    def point(ppm, rms):
        d.set_state(fresh)
        fr.reset_streams(range(S))
        sf.reset_bands(range(B))
        pf.reset_bands(range(B))
        ch = Q.Channel(B, sample_rate=float(FS), tx_ppm=ppm, rx_ppm=ppm, noise_rms=rms, noise_seed=11, device=dev.index)
        pa = Q.Path(B, clock_ppm=ppm, tau0=args.tau0, device=dev.index)
        for h in (ch, pa):
            h.set_stream(stream.cuda_stream)
        gen.manual_seed(1234)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        good = []
        for _ in range(args.frames):
            sent = torch.randint(0, 256, (S, P), dtype=torch.uint8, device=dev, generator=gen)
            m.modulate_bytes_device(sent, plen, START, STOP, rows, n_out)
            sf.apply_device(rows, n, wide, scale_out=float(D))
            k = int(pa.apply_device(wide, n * D, prop)[0])                   # one clock for all bands: they emit alike
            ch.apply_device(prop, k)
            f = int(pf.apply_device(prop, k, chans, out_cap=cap)[0])
            d.process_device_fmt(chans, f, bits, nbits, "cf32")
            Q.tsc_find_device(bits, nbits, TSC, offs, stream.cuda_stream)
            fr.push(bits, nbits, pay, npay, offs)
            good.append(((npay == P) & (pay[:, :P] == sent).all(dim=1)).sum())
        e1.record(stream)
        e1.synchronize()
        good = [int(g) for g in good]
        ch.close()
        pa.close()
        after = good[args.skip:]
        return dict(ppm=ppm, noise_rms=rms, frames_received_per_round=good, frames_sent_after_skip=S * len(after),
                    frames_lost_after_skip=S * len(after) - sum(after),
                    frame_loss_after_skip=round(1.0 - sum(after) / (S * len(after)), 6), ms=round(e0.elapsed_time(e1), 1))

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")

    for rms in (float(v) for v in args.noise_rms.split(",") if v):
        rec["noise_sweep"].append(point(1.0, rms))
        print(json.dumps(rec["noise_sweep"][-1]), flush=True)
        save()
    for ppm in (float(v) for v in args.ppm.split(",") if v):
        rec["ppm_sweep"].append(point(ppm, 0.0))
        print(json.dumps(rec["ppm_sweep"][-1]), flush=True)
        save()
    for h in (m, sf, pf, d):
        h.close()


if __name__ == "__main__":
    main()
