"""A handle destroyed with pipelined calls still queued.

qpsk_demod_destroy is the one caller that hands the queued work to the
handle's destructor: it has to issue a deferred back stage, wait for both
library streams and only then release the buffers, events and streams those
calls use (the streams are declared in front of every buffer and event of the
handle, so they go last).  Three process_device_async calls of 2048, 1000 and
2048 samples are queued into three separate sets of device rows, the handle is
closed with no pipeline_wait, and after torch.cuda.synchronize() every call's
bits and counts (and symbols, where asked for) equal the oracle's bit for bit.
A second handle made right after runs one call and matches the oracle too.

Five streams at sps 8, span 8 (65 taps), max_samples_per_call 2048, in two
configurations: without the FLL, with symbol rows, timing, FIR phases and link
statistics all enabled first (every optional buffer of the handle is in use);
and with the FLL and the IQ balancer, bits only, where the newest call's back
stage is still deferred when the handle goes.
"""
import functools

import pytest

import common as K
import gpu_harness as H
from gpu_harness import dev

gpu = pytest.mark.gpu

S, SPS, SPAN, N_MAX = 5, 8, 8, 2048
CALLS = [[2048] * S, [1000] * S, [2048] * S]


def every_probe(b):
    b.enable_timing()
    b.enable_fir_phases()
    b.enable_link_stats()


# name -> (handle knobs, oracle knobs, prepare, symbol rows)
CFGS = {
    "probes-and-symbols": ({}, {}, every_probe, True),
    "fll-deferred": (dict(enable_fll=True, cfo_loop_bandwidth=1e-3, iq_balance=True),
                     dict(enable_fll=True, cfo_loop_bw=1e-3, iq_balance=True), None, False),
}


@functools.lru_cache(maxsize=None)
def signal():
    iq = K.batch_signals(S, seed0=11, sps=SPS, span=SPAN, n_bits=1400, snr_db=18)
    assert iq.shape[1] // 2 >= sum(c[0] for c in CALLS)
    iq.setflags(write=False)
    return iq


@functools.lru_cache(maxsize=None)
def oracle(cfg):
    return H.oracle_run(signal(), CALLS, K.FS // SPS, SPAN, **CFGS[cfg][1])


@gpu
@pytest.mark.parametrize("cfg", list(CFGS))
def test_close_with_pipelined_calls_queued(dev, cfg):
    knobs, _, prepare, want_syms = CFGS[cfg]
    want = oracle(cfg)
    got, depth = H.async_run(signal(), CALLS, SPS, SPAN, prepare=prepare, want_syms=want_syms, max_samples=N_MAX,
                             close_unwaited=True, **knobs)
    assert depth == 2
    H.assert_same(got, want, what=f"{cfg}, closed unwaited:")
    again = H.gpu_run(signal(), CALLS[:1], K.FS // SPS, SPAN, want_syms=want_syms, max_samples=N_MAX, **knobs)
    H.assert_same(again, want[:1], what=f"{cfg}, the next handle:")
