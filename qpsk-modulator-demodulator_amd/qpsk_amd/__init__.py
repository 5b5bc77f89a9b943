"""Python binding of libqpsk_demod.so (the C ABI in include/qpsk_demod.h).

Mirrors the reference C# API so the parity tests read like the reference's own
usage (testAtDataLevel.cs, ModDemodOverSDR.cs):

    QPSKDeModulator(SampleRate, SymbolRate, RrcAlpha=0.9, rrcSpan=6, ...)
        .DeModulate(samples) -> str            (QPSKDeModulator.cs:339-425)
        .deModulateConstellation(samples)      (:427-455)
        .DeModulateBytes(samples, start, end)  (:169-259)
        .DeModulateTextUtf8(samples, ...)      (:262-277)

and exposes the batched handle (`BatchDemodulator`) that one MI355X runs over
thousands of streams.  There is no CPU fallback: if the HIP library is missing
or no GPU is present, every compute call raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_PKG = os.path.dirname(_HERE)
# QPSK_DEMOD_LIB points at another in-tree build of the same library (A/B
# timing of kernel variants); it must be a libqpsk_demod.so, never a fallback
LIB_PATH = os.environ.get("QPSK_DEMOD_LIB") or os.path.join(_PKG, "_build", "libqpsk_demod.so")

QPSK_OK = 0
QPSK_ERR_ARGUMENT = -1
QPSK_ERR_ARGUMENT_NULL = -2
QPSK_ERR_OUT_OF_RANGE = -3
QPSK_ERR_DEVICE = -4
QPSK_ERR_CAPACITY = -5
QPSK_ERR_STATE = -6
# head[1] of qpsk_frames_pack_device, and the flags HostRing.collect_frames returns
FRAMES_TRUNCATED = 1          # a frame longer than the payload row (max_frame_bytes)
FRAMES_DROPPED = 2            # a frame not stored for lack of capacity (chunk_frame_bytes)
STATUS_CARRY_OVERFLOW = 1
STATUS_OUTPUT_TRUNCATED = 2
STATUS_NONFINITE_TIMING = 4
MEM_HOST = 0
MEM_DEVICE = 1
MODE_DEMODULATE = 0
MODE_CONSTELLATION = 1
# qpsk_demod_params.costas_trig: the Costas NCO's Math.Sin/Cos (CostasLoopQpsk.cs:69-70)
COSTAS_TRIG_PORTABLE = 0      # table sincos, within 1 ulp of glibc (default, faster)
COSTAS_TRIG_GLIBC = 1         # glibc's own sin/cos: symbols bit-identical to the libm oracle

# sample formats of the *_fmt entry points (QPSK_FMT_*)
FMT_CF32 = 0
FMT_CS16 = 1
FMT_CS8 = 2
FMT_CU8 = 3
# name -> (QPSK_FMT_*, numpy dtype of a row's elements, ctypes type): the one
# table of per-format facts (_torch_dtype derives a tensor's dtype from it)
_FORMATS = {"cf32": (FMT_CF32, np.float32, C.c_float), "cs16": (FMT_CS16, np.int16, C.c_int16),
            "cs8": (FMT_CS8, np.int8, C.c_int8), "cu8": (FMT_CU8, np.uint8, C.c_uint8)}


# qpsk_mod_modulate_fmt's norm (QPSK_MOD_NORM_*), and the row lengths at which its
# kernels change blocks (QPSK_MOD_TILE_SAMPLES, QPSK_MOD_SCAN_DIBITS)
NORM_FIXED = 0
NORM_PEAK = 1
_NORMS = {"fixed": NORM_FIXED, "peak": NORM_PEAK}
MOD_TILE_SAMPLES = 512
MOD_SCAN_DIBITS = 1024


def _format(fmt):
    """(QPSK_FMT_*, numpy dtype, ctypes type) of a format name or tag."""
    for name, rec in _FORMATS.items():
        if fmt == name or (not isinstance(fmt, str) and fmt == rec[0]):
            return rec
    raise ValueError("fmt must be 'cf32', 'cs16', 'cs8' or 'cu8'")


def _torch_dtype(fmt):
    """The torch dtype of a format's elements: the numpy dtype's namesake
    (torch is imported here, on first use, not with the module)."""
    import torch
    return getattr(torch, np.dtype(_format(fmt)[1]).name)


def _host_call(fn, handle, n_streams, max_syms, iq, mode, lengths, want_syms):
    """One host call of a process entry point fn (a handle's or a group's) on
    checked [S, 2n] rows: allocates the output rows for up to max_syms symbols
    a stream and returns (bits, n_bits, syms or None, n_syms)."""
    ms = max(int(max_syms), 1)
    bstride = (2 * ms + 7) // 8 + 8
    bits = np.zeros((n_streams, bstride), dtype=np.uint8)
    n_bits = np.zeros(n_streams, dtype=np.int64)
    n_syms = np.zeros(n_streams, dtype=np.int64)
    syms = np.zeros((n_streams, 2 * ms), dtype=np.float32) if (want_syms or mode == MODE_CONSTELLATION) else None
    _check(fn(
        handle, int(mode), iq.ctypes.data if iq.size else None, iq.shape[1], iq.shape[1] // 2,
        lengths.ctypes.data_as(_i64p) if lengths is not None else None, MEM_HOST,
        bits.ctypes.data if mode == MODE_DEMODULATE else None, bstride,
        n_bits.ctypes.data if mode == MODE_DEMODULATE else None,
        syms.ctypes.data if syms is not None else None, 2 * ms, n_syms.ctypes.data))
    return bits, n_bits, syms, n_syms


def fmt_sample_bytes(fmt: int) -> int:
    """Bytes of one complex sample of QPSK_FMT_* fmt, negative if unknown (needs no device)."""
    return int(lib().qpsk_fmt_sample_bytes(int(fmt)))


_i64p = C.POINTER(C.c_int64)
_u8p = C.POINTER(C.c_uint8)
_f32p = C.POINTER(C.c_float)
_f64p = C.POINTER(C.c_double)


class DemodParams(C.Structure):
    _fields_ = [
        ("sample_rate", C.c_int32),
        ("symbol_rate", C.c_int32),
        ("rrc_alpha", C.c_float),
        ("rrc_span", C.c_int32),
        ("symbol_sync_bandwidth", C.c_double),
        ("costas_loop_bandwidth", C.c_double),
        ("cfo_loop_bandwidth", C.c_double),
        ("differential", C.c_int32),
        ("enable_fll", C.c_int32),
        ("vector_lanes", C.c_int32),
        ("device", C.c_int32),
        ("max_samples_per_call", C.c_int64),
        ("loop_variant", C.c_int32),
        ("iq_balance", C.c_int32),
        ("costas_trig", C.c_int32),
        ("reserved", C.c_int32 * 5),
    ]


class SynthParams(C.Structure):
    _fields_ = [
        ("sample_rate", C.c_int32),
        ("symbol_rate", C.c_int32),
        ("rrc_alpha", C.c_double),
        ("rrc_span", C.c_int32),
        ("differential", C.c_int32),
        ("seed", C.c_uint64),
        ("lo_ppm", C.c_double),
        ("cfo_hz", C.c_double),
        ("multipath", C.c_int32),
        ("esn0_db", C.c_double),
        ("first_stream", C.c_int64),
        ("reserved", C.c_int32 * 6),
    ]


class ModParams(C.Structure):
    _fields_ = [
        ("sample_rate", C.c_int32),
        ("symbol_rate", C.c_int32),
        ("rrc_alpha", C.c_double),
        ("rrc_span", C.c_int32),
        ("differential", C.c_int32),
        ("device", C.c_int32),
        ("reserved", C.c_int32 * 7),
    ]


class BerParams(C.Structure):
    """qpsk_ber_params: skip_bits, window, key_bits and search of the bit-error counter."""
    _fields_ = [("skip_bits", C.c_int64), ("window", C.c_int32), ("key_bits", C.c_int32), ("search", C.c_int32),
                ("reserved", C.c_int32 * 3)]


class ChannelParams(C.Structure):
    """qpsk_channel_params: the LO pair and the noise of the test bench's channel."""
    _fields_ = [("sample_rate", C.c_double), ("lo_hz", C.c_double), ("tx_ppm", C.c_double), ("rx_ppm", C.c_double),
                ("tx_phase0", C.c_double), ("rx_phase0", C.c_double), ("tx_seed", C.c_uint64), ("rx_seed", C.c_uint64),
                ("noise_rms", C.c_double), ("noise_seed", C.c_uint64), ("first_stream", C.c_int64),
                ("device", C.c_int32), ("reserved", C.c_int32 * 7)]


class PathParams(C.Structure):
    """qpsk_path_params: the sample-clock offset and the default taps of the propagation path."""
    _fields_ = [("clock_ppm", C.c_double), ("clock_spread", C.c_double), ("clock_seed", C.c_uint64),
                ("tau0", C.c_double), ("tau_random", C.c_int32), ("multipath", C.c_int32), ("first_stream", C.c_int64),
                ("device", C.c_int32), ("reserved", C.c_int32 * 7)]


class PfbParams(C.Structure):
    """qpsk_pfb_params: the channels, the prototype's length and the gain of the polyphase channeliser."""
    _fields_ = [("channels", C.c_int32), ("taps_per_branch", C.c_int32), ("gain", C.c_float), ("device", C.c_int32),
                ("reserved", C.c_int32 * 12)]


class SfbParams(C.Structure):
    """qpsk_sfb_params: the channels and the prototype's length of the polyphase synthesis bank."""
    _fields_ = [("channels", C.c_int32), ("taps_per_branch", C.c_int32), ("device", C.c_int32),
                ("reserved", C.c_int32 * 12)]


class TunerParams(C.Structure):
    """qpsk_tuner_params: the default tuning, the rate, the prototype's length and cutoff of the tuner."""
    _fields_ = [("freq", C.c_double), ("rate", C.c_double), ("tau0", C.c_double), ("cutoff", C.c_double),
                ("taps_per_phase", C.c_int32), ("device", C.c_int32), ("first_stream", C.c_int64),
                ("reserved", C.c_int32 * 6)]


class LoopShape(C.Structure):
    """qpsk_loop_shape (include/qpsk_demod.h)"""
    _fields_ = [(n, C.c_int32) for n in (
        "streams", "lanes", "round", "slots", "prefix", "cap", "lds_bytes", "fir_beside", "fir_taps",
        "fir_lds_bytes", "lds_granule", "reserved")] + [("lag_max", C.c_double)]


def loop_shape(requested, n_streams, sps, cus, costas_trig=0, want_syms=False, rrc_taps=129):
    """The loop shape a handle would run (qpsk_demod_loop_shape), as a dict; needs no device."""
    o = LoopShape()
    _check(lib().qpsk_demod_loop_shape(int(requested), int(n_streams), float(sps), int(cus), int(rrc_taps),
                                       int(costas_trig), 1 if want_syms else 0, C.byref(o)))
    return {n: getattr(o, n) for n, _ in LoopShape._fields_ if n != "reserved"}


class QPSKError(RuntimeError):
    pass


_lib = None


class _Missing:
    """Signature sink for an entry point an older A/B build does not export."""

    def __setattr__(self, name, value):
        pass


class _Lenient:
    def __init__(self, real):
        object.__setattr__(self, "_real", real)

    def __getattr__(self, name):
        try:
            return getattr(self._real, name)
        except AttributeError:
            return _Missing()


def lib():
    """Load the HIP library; raise loudly if it was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise QPSKError(f"{LIB_PATH} missing: run `make -C qpsk-modulator-demodulator_amd` "
                        "(there is no CPU fallback)")
    real = C.CDLL(LIB_PATH)
    # an A/B build of an older revision (QPSK_DEMOD_LIB) may lack newer entry
    # points: their signatures are then skipped instead of failing the load
    L = _Lenient(real) if os.environ.get("QPSK_DEMOD_LIB") else real
    L.qpsk_abi_version.restype = C.c_int
    L.qpsk_last_error.restype = C.c_char_p
    L.qpsk_demod_params_init.argtypes = [C.POINTER(DemodParams), C.c_int32, C.c_int32]
    L.qpsk_demod_create.argtypes = [C.POINTER(DemodParams), C.c_int32, C.POINTER(C.c_void_p)]
    L.qpsk_demod_destroy.argtypes = [C.c_void_p]
    L.qpsk_demod_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    L.qpsk_demod_process.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int64,
                                     _i64p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                     C.c_void_p, C.c_int64, C.c_void_p]
    L.qpsk_demod_process_async.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int64,
                                           _i64p, C.c_void_p, C.c_int64, C.c_void_p,
                                           C.c_void_p, C.c_int64, C.c_void_p]
    # CS16 (int16 I,Q) input: the float entry points' arguments, int16 rows
    L.qpsk_demod_process_cs16.argtypes = L.qpsk_demod_process.argtypes
    L.qpsk_demod_process_async_cs16.argtypes = L.qpsk_demod_process_async.argtypes
    L.qpsk_demod_set_cs16_scale.argtypes = [C.c_void_p, C.c_float]
    L.qpsk_demod_get_cs16_scale.argtypes = [C.c_void_p, _f32p]
    # format-tagged entry points: fmt in front of the float ones' arguments
    L.qpsk_fmt_sample_bytes.argtypes = [C.c_int32]
    L.qpsk_demod_process_fmt.argtypes = [C.c_void_p, C.c_int32] + L.qpsk_demod_process.argtypes[1:]
    L.qpsk_demod_process_async_fmt.argtypes = [C.c_void_p, C.c_int32] + L.qpsk_demod_process_async.argtypes[1:]
    L.qpsk_demod_set_input_scale.argtypes = [C.c_void_p, C.c_int32, C.c_float]
    L.qpsk_demod_get_input_scale.argtypes = [C.c_void_p, C.c_int32, _f32p]
    L.qpsk_demod_pipeline_wait.argtypes = [C.c_void_p, C.c_void_p]
    L.qpsk_demod_status.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    L.qpsk_demod_last_mf.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32]
    L.qpsk_mod_params_init.argtypes = [C.POINTER(ModParams), C.c_int32, C.c_int32]
    L.qpsk_mod_create.argtypes = [C.POINTER(ModParams), C.c_char_p, C.POINTER(C.c_void_p)]
    L.qpsk_mod_destroy.argtypes = [C.c_void_p]
    L.qpsk_mod_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    L.qpsk_mod_output_floats.argtypes = [C.c_void_p, C.c_int64, C.c_int32]
    L.qpsk_mod_output_floats.restype = C.c_int64
    L.qpsk_mod_modulate.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32,
                                    C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
    L.qpsk_mod_modulate_bytes.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                          C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                          C.c_void_p, C.c_int64, C.c_void_p]
    # format-tagged modulator: fmt, norm, scale in front, void rows, peak behind
    L.qpsk_mod_modulate_fmt.argtypes = ([C.c_void_p, C.c_int32, C.c_int32, C.c_float] +
                                        L.qpsk_mod_modulate.argtypes[1:] + [C.c_void_p])
    L.qpsk_mod_modulate_bytes_fmt.argtypes = ([C.c_void_p, C.c_int32, C.c_int32, C.c_float] +
                                              L.qpsk_mod_modulate_bytes.argtypes[1:10] + [C.c_int32] +
                                              L.qpsk_mod_modulate_bytes.argtypes[10:] + [C.c_void_p])
    L.qpsk_quantise_iq.argtypes = [C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.qpsk_demod_pipeline_depth.argtypes = [C.c_void_p]
    L.qpsk_demod_max_symbols.argtypes = [C.c_void_p, C.c_int64]
    L.qpsk_demod_max_symbols.restype = C.c_int64
    L.qpsk_tsc_find.argtypes = [_u8p, C.c_int64, C.c_char_p]
    L.qpsk_tsc_find.restype = C.c_int64
    L.qpsk_demod_enable_timing.argtypes = [C.c_void_p, C.c_int32]
    L.qpsk_demod_stage_times.argtypes = [C.c_void_p, _f32p, C.c_int32]
    L.qpsk_demod_launch_times.argtypes = [C.c_void_p, _f32p, C.c_int32]
    L.qpsk_demod_kernel_clocks.argtypes = [C.c_void_p, _f32p, C.c_int32]
    L.qpsk_demod_rrc_taps.argtypes = [C.c_void_p, _f32p, C.c_int32]
    L.qpsk_demod_gains.argtypes = [C.c_void_p] + [_f64p] * 5
    L.qpsk_demod_fll_taps.argtypes = [C.c_void_p, _f32p, _f32p, C.c_int32]
    L.qpsk_demod_state_bytes.argtypes = [C.c_void_p]
    L.qpsk_demod_state_bytes.restype = C.c_int64
    L.qpsk_demod_get_state.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.qpsk_demod_set_state.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.qpsk_state_blob_check.argtypes = [C.POINTER(DemodParams), C.c_int32, C.c_void_p, C.c_int64]
    L.qpsk_pipeline_gate_enabled.restype = C.c_int
    L.qpsk_demod_gate_timeouts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.qpsk_demod_pick_loop_variant.argtypes = [C.c_int32, C.c_int32, C.c_double, C.c_int32]
    L.qpsk_demod_pick_loop_variant.restype = C.c_int32
    L.qpsk_demod_loop_shape.argtypes = [C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_int32, C.POINTER(LoopShape)]
    L.qpsk_demod_enable_fir_phases.argtypes = [C.c_void_p, C.c_int32]
    L.qpsk_demod_fir_phases.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    L.qpsk_framer_create.argtypes = [C.c_int32, _u8p, C.c_int32, _u8p, C.c_int32, C.c_int64,
                                     C.POINTER(C.c_void_p)]
    L.qpsk_framer_destroy.argtypes = [C.c_void_p]
    L.qpsk_framer_set_markers.argtypes = [C.c_void_p, _u8p, C.c_int32, _u8p, C.c_int32]
    L.qpsk_demod_design.argtypes = [C.POINTER(DemodParams), _f32p, C.c_int32, _f64p, _f32p, _f32p]
    L.qpsk_framer_push.argtypes = [C.c_void_p, _u8p, C.c_int64, _i64p, _i64p, _u8p, C.c_int64,
                                   _i64p]
    L.qpsk_framer_dev_create.argtypes = [C.c_int32, _u8p, C.c_int32, _u8p, C.c_int32, C.c_int64,
                                         C.c_int32, C.POINTER(C.c_void_p)]
    L.qpsk_framer_dev_destroy.argtypes = [C.c_void_p]
    L.qpsk_framer_dev_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    L.qpsk_framer_dev_set_markers.argtypes = [C.c_void_p, _u8p, C.c_int32, _u8p, C.c_int32]
    L.qpsk_framer_dev_push.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_int64, C.c_void_p]
    L.qpsk_framer_dev_status.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.qpsk_tsc_find_device.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_char_p,
                                       C.c_void_p, C.c_void_p]
    L.qpsk_framer_dev_reset_streams.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int32]
    L.qpsk_frames_pack_device.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64,
                                          C.c_void_p, C.c_void_p, C.c_void_p]
    L.qpsk_synth_params_init.argtypes = [C.POINTER(SynthParams), C.c_int32, C.c_int32]
    L.qpsk_synth_generate.argtypes = [C.POINTER(SynthParams), C.c_int32, C.c_void_p, C.c_int32,
                                      C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
    L.qpsk_rx_create.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    L.qpsk_rx_destroy.argtypes = [C.c_void_p]
    L.qpsk_rx_next_slot.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    L.qpsk_rx_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, _i64p,
                                 C.POINTER(C.c_int64)]
    L.qpsk_rx_collect.argtypes = [C.c_void_p, _u8p, C.c_int64, _i64p, C.POINTER(C.c_int64)]
    L.qpsk_rx_create_cs16.argtypes = L.qpsk_rx_create.argtypes
    L.qpsk_rx_next_slot_cs16.argtypes = L.qpsk_rx_next_slot.argtypes
    L.qpsk_rx_submit_cs16.argtypes = L.qpsk_rx_submit.argtypes
    L.qpsk_rx_create_fmt.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    L.qpsk_rx_next_slot_fmt.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    L.qpsk_rx_submit_fmt.argtypes = [C.c_void_p, C.c_int32] + L.qpsk_rx_submit.argtypes[1:]
    # a framed ring: the chunk's completed frames instead of its bits
    L.qpsk_rx_attach_framer.argtypes = [C.c_void_p, _u8p, C.c_int32, _u8p, C.c_int32, C.c_char_p, C.c_int64,
                                        C.c_int64, C.c_int64, C.c_int32]
    L.qpsk_rx_set_markers.argtypes = [C.c_void_p, _u8p, C.c_int32, _u8p, C.c_int32]
    L.qpsk_rx_frames_bytes.argtypes = [C.c_void_p]
    L.qpsk_rx_frames_bytes.restype = C.c_int64
    L.qpsk_rx_collect_frames.argtypes = [C.c_void_p, _u8p, C.c_int64, _i64p, _i64p, _u8p, C.c_int64, _i64p,
                                         C.POINTER(C.c_int64)]
    L.qpsk_rx_reset_streams.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int32]
    L.qpsk_shard_streams.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32),
                                     C.POINTER(C.c_int32)]
    L.qpsk_demod_group_create.argtypes = [C.POINTER(DemodParams), C.POINTER(C.c_int32), C.c_int32, C.c_int32,
                                          C.POINTER(C.c_void_p)]
    L.qpsk_demod_group_destroy.argtypes = [C.c_void_p]
    L.qpsk_demod_group_size.argtypes = [C.c_void_p]
    L.qpsk_demod_group_shard.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                         C.POINTER(C.c_int32), C.POINTER(C.c_void_p)]
    L.qpsk_demod_group_process.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int64,
                                           _i64p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                           C.c_void_p, C.c_int64, C.c_void_p]
    L.qpsk_demod_group_process_fmt.argtypes = [C.c_void_p, C.c_int32] + L.qpsk_demod_group_process.argtypes[1:]
    L.qpsk_demod_group_state_bytes.argtypes = [C.c_void_p, C.c_int32]
    L.qpsk_demod_group_state_bytes.restype = C.c_int64
    L.qpsk_demod_group_get_state.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]
    L.qpsk_demod_group_set_state.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]
    L.qpsk_link_stats_size.restype = C.c_int
    L.qpsk_demod_enable_link_stats.argtypes = [C.c_void_p, C.c_int32]
    L.qpsk_demod_link_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
    L.qpsk_demod_group_enable_link_stats.argtypes = [C.c_void_p, C.c_int32]
    L.qpsk_demod_group_link_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    _i32p = C.POINTER(C.c_int32)
    L.qpsk_stream_list_check.argtypes = [C.c_int32, _i32p, C.c_int32]
    rows = [C.POINTER(DemodParams), C.c_int32, C.c_void_p, C.c_int64, _i32p, C.c_int32, C.c_void_p, C.c_int64]
    L.qpsk_state_blob_select.argtypes = rows
    L.qpsk_state_blob_merge.argtypes = rows
    for owner in ("qpsk_demod", "qpsk_demod_group"):
        getattr(L, owner + "_reset_streams").argtypes = [C.c_void_p, _i32p, C.c_int32]
        getattr(L, owner + "_streams_state_bytes").argtypes = [C.c_void_p, C.c_int32]
        getattr(L, owner + "_streams_state_bytes").restype = C.c_int64
        getattr(L, owner + "_get_streams_state").argtypes = [C.c_void_p, _i32p, C.c_int32, C.c_void_p, C.c_int64]
        getattr(L, owner + "_set_streams_state").argtypes = [C.c_void_p, _i32p, C.c_int32, C.c_void_p, C.c_int64]
    # bit errors where the bits are: params, rx rows, ref rows, S, out (, stream)
    ber = [C.POINTER(BerParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32,
           C.c_void_p]
    L.qpsk_ber_params_init.argtypes = [C.POINTER(BerParams)]
    L.qpsk_ber_params_init.restype = None
    L.qpsk_ber_row_size.restype = C.c_int
    L.qpsk_ber_count.argtypes = ber
    L.qpsk_ber_count_device.argtypes = ber + [C.c_void_p]
    # the test bench's channel: LO pair and noise on rows of any format
    L.qpsk_channel_params_init.argtypes = [C.POINTER(ChannelParams), C.c_double]
    L.qpsk_channel_params_init.restype = None
    L.qpsk_channel_create.argtypes = [C.POINTER(ChannelParams), C.c_int32, C.POINTER(C.c_void_p)]
    L.qpsk_channel_destroy.argtypes = [C.c_void_p]
    L.qpsk_channel_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    L.qpsk_channel_apply_fmt.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_float, C.c_int32, C.c_int32,
                                         C.c_void_p, C.c_int64, C.c_float, C.c_int64, _i64p, C.c_int32]
    L.qpsk_channel_state_size.restype = C.c_int
    L.qpsk_channel_get_state.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.qpsk_channel_set_state.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.qpsk_channel_reset_streams.argtypes = [C.c_void_p, _i32p, C.c_int32]
    L.qpsk_channel_state_check.argtypes = [C.POINTER(ChannelParams), C.c_int32, C.c_void_p, C.c_int64]
    # the propagation path: multipath taps and a sample-clock offset
    L.qpsk_path_params_init.argtypes = [C.POINTER(PathParams)]
    L.qpsk_path_params_init.restype = None
    L.qpsk_path_create.argtypes = [C.POINTER(PathParams), C.c_int32, C.POINTER(C.c_void_p)]
    L.qpsk_path_destroy.argtypes = [C.c_void_p]
    L.qpsk_path_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    L.qpsk_path_set_taps.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
    L.qpsk_path_apply_fmt.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_float, C.c_int32, C.c_int32,
                                      C.c_void_p, C.c_int64, C.c_int64, C.c_float, C.c_int64, _i64p, _i64p, C.c_int32]
    L.qpsk_path_out_bound.argtypes = [C.POINTER(PathParams), C.c_int64]
    L.qpsk_path_out_bound.restype = C.c_int64
    L.qpsk_path_count.argtypes = [C.c_double, C.c_double, C.c_int64, C.c_int64]
    L.qpsk_path_count.restype = C.c_int64
    L.qpsk_path_state_size.restype = C.c_int
    L.qpsk_path_state_init.argtypes = [C.POINTER(PathParams), C.c_int32, C.c_void_p, C.c_int64]
    L.qpsk_path_get_state.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.qpsk_path_set_state.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.qpsk_path_reset_streams.argtypes = [C.c_void_p, _i32p, C.c_int32]
    L.qpsk_path_state_check.argtypes = [C.c_int32, C.c_void_p, C.c_int64]
    L.qpsk_path_apply_host.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                       C.c_int64, C.c_int64, _i64p, _i64p]
    # the polyphase channeliser: one wideband row into M streams
    L.qpsk_pfb_params_init.argtypes = [C.POINTER(PfbParams)]
    L.qpsk_pfb_params_init.restype = None
    L.qpsk_pfb_create.argtypes = [C.POINTER(PfbParams), C.c_int32, C.POINTER(C.c_void_p)]
    L.qpsk_pfb_destroy.argtypes = [C.c_void_p]
    L.qpsk_pfb_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    L.qpsk_pfb_design.argtypes = [C.POINTER(PfbParams), C.c_void_p, C.c_int64]
    L.qpsk_pfb_twiddles.argtypes = [C.c_int32, C.c_void_p, C.c_int64]
    L.qpsk_pfb_set_taps.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.qpsk_pfb_count.argtypes = [C.c_int32, C.c_int64, C.c_int64]
    L.qpsk_pfb_count.restype = C.c_int64
    L.qpsk_pfb_out_bound.argtypes = [C.c_int32, C.c_int64]
    L.qpsk_pfb_out_bound.restype = C.c_int64
    L.qpsk_pfb_tile_frames.argtypes = [C.c_int32]
    L.qpsk_pfb_apply_fmt.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_int64,
                                     C.c_int64, C.c_int64, _i64p, _i64p, C.c_int32]
    L.qpsk_pfb_state_size.argtypes = [C.POINTER(PfbParams)]
    L.qpsk_pfb_state_size.restype = C.c_int64
    L.qpsk_pfb_state_init.argtypes = [C.POINTER(PfbParams), C.c_int32, C.c_void_p, C.c_int64]
    L.qpsk_pfb_get_state.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.qpsk_pfb_set_state.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.qpsk_pfb_reset_bands.argtypes = [C.c_void_p, _i32p, C.c_int32]
    L.qpsk_pfb_state_check.argtypes = [C.POINTER(PfbParams), C.c_int32, C.c_void_p, C.c_int64]
    L.qpsk_pfb_apply_host.argtypes = [C.POINTER(PfbParams), C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                      C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, _i64p, _i64p]
    L.qpsk_sfb_params_init.argtypes = [C.POINTER(SfbParams)]
    L.qpsk_sfb_params_init.restype = None
    L.qpsk_sfb_create.argtypes = [C.POINTER(SfbParams), C.c_int32, C.POINTER(C.c_void_p)]
    L.qpsk_sfb_destroy.argtypes = [C.c_void_p]
    L.qpsk_sfb_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    L.qpsk_sfb_set_taps.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.qpsk_sfb_tile_frames.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    L.qpsk_sfb_apply_fmt.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_float, C.c_int32, C.c_int32,
                                     C.c_void_p, C.c_int64, C.c_float, C.c_int64, _i64p, C.c_int32]
    L.qpsk_sfb_state_size.argtypes = [C.POINTER(SfbParams)]
    L.qpsk_sfb_state_size.restype = C.c_int64
    L.qpsk_sfb_state_init.argtypes = [C.POINTER(SfbParams), C.c_int32, C.c_void_p, C.c_int64]
    L.qpsk_sfb_get_state.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.qpsk_sfb_set_state.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.qpsk_sfb_reset_bands.argtypes = [C.c_void_p, _i32p, C.c_int32]
    L.qpsk_sfb_state_check.argtypes = [C.POINTER(SfbParams), C.c_int32, C.c_void_p, C.c_int64]
    L.qpsk_sfb_apply_host.argtypes = [C.POINTER(SfbParams), C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                      C.c_int64, C.c_void_p, C.c_int64, C.c_float, C.c_int64, _i64p]
    # the tuner: per-stream frequency shift and any-rate resampler
    L.qpsk_tuner_params_init.argtypes = [C.POINTER(TunerParams)]
    L.qpsk_tuner_params_init.restype = None
    L.qpsk_tuner_create.argtypes = [C.POINTER(TunerParams), C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    L.qpsk_tuner_destroy.argtypes = [C.c_void_p]
    L.qpsk_tuner_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    L.qpsk_tuner_design.argtypes = [C.c_int32, C.c_double, C.c_void_p, C.c_int64]
    L.qpsk_tuner_tables.argtypes = [C.c_void_p, C.c_void_p]
    L.qpsk_tuner_osc.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.qpsk_tuner_set_taps.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.qpsk_tuner_set_freq.argtypes = [C.c_void_p, _i32p, C.c_int32, C.c_void_p]
    L.qpsk_tuner_apply_fmt.argtypes = L.qpsk_path_apply_fmt.argtypes
    L.qpsk_tuner_out_bound.argtypes = [C.POINTER(TunerParams), C.c_void_p, C.c_int32, C.c_int64]
    L.qpsk_tuner_out_bound.restype = C.c_int64
    L.qpsk_tuner_count.argtypes = [C.c_double, C.c_double, C.c_int32, C.c_int64, C.c_int64]
    L.qpsk_tuner_count.restype = C.c_int64
    L.qpsk_tuner_state_size.restype = C.c_int
    L.qpsk_tuner_state_init.argtypes = [C.POINTER(TunerParams), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    L.qpsk_tuner_get_state.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.qpsk_tuner_set_state.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.qpsk_tuner_reset_streams.argtypes = [C.c_void_p, _i32p, C.c_int32]
    L.qpsk_tuner_state_check.argtypes = [C.POINTER(TunerParams), C.c_int32, C.c_void_p, C.c_int64]
    L.qpsk_tuner_apply_host.argtypes = [C.POINTER(TunerParams), C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                        C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, _i64p, _i64p]
    _lib = real
    return real


EXPORTED_SYMBOLS = [
    "qpsk_abi_version", "qpsk_last_error", "qpsk_demod_params_init", "qpsk_demod_create",
    "qpsk_demod_destroy", "qpsk_demod_set_stream", "qpsk_demod_process", "qpsk_demod_max_symbols",
    "qpsk_tsc_find", "qpsk_demod_enable_timing", "qpsk_demod_stage_times", "qpsk_demod_launch_times",
    "qpsk_demod_kernel_clocks",
    "qpsk_demod_rrc_taps",
    "qpsk_demod_gains", "qpsk_demod_fll_taps", "qpsk_demod_state_bytes", "qpsk_demod_get_state",
    "qpsk_demod_set_state", "qpsk_pipeline_gate_enabled", "qpsk_demod_gate_timeouts",
    "qpsk_demod_pick_loop_variant", "qpsk_demod_loop_shape",
    "qpsk_demod_enable_fir_phases",
    "qpsk_demod_fir_phases", "qpsk_demod_design", "qpsk_framer_create", "qpsk_framer_destroy",
    "qpsk_framer_set_markers", "qpsk_framer_push", "qpsk_framer_dev_create",
    "qpsk_framer_dev_destroy", "qpsk_framer_dev_set_stream", "qpsk_framer_dev_set_markers",
    "qpsk_framer_dev_push", "qpsk_framer_dev_status", "qpsk_tsc_find_device",
    "qpsk_synth_params_init", "qpsk_synth_generate", "qpsk_demod_process_async",
    "qpsk_demod_pipeline_wait", "qpsk_demod_pipeline_depth", "qpsk_rx_create", "qpsk_rx_destroy",
    "qpsk_rx_next_slot", "qpsk_rx_submit", "qpsk_rx_collect", "qpsk_demod_status", "qpsk_demod_last_mf",
    "qpsk_mod_params_init", "qpsk_mod_create", "qpsk_mod_destroy", "qpsk_mod_set_stream",
    "qpsk_mod_output_floats", "qpsk_mod_modulate", "qpsk_mod_modulate_bytes",
    "qpsk_shard_streams", "qpsk_demod_group_create", "qpsk_demod_group_destroy", "qpsk_demod_group_size",
    "qpsk_demod_group_shard", "qpsk_demod_group_process", "qpsk_demod_group_state_bytes",
    "qpsk_demod_group_get_state", "qpsk_demod_group_set_state",
    "qpsk_demod_set_cs16_scale", "qpsk_demod_get_cs16_scale", "qpsk_demod_process_cs16",
    "qpsk_demod_process_async_cs16", "qpsk_rx_create_cs16", "qpsk_rx_next_slot_cs16", "qpsk_rx_submit_cs16",
    "qpsk_fmt_sample_bytes", "qpsk_demod_process_fmt", "qpsk_demod_process_async_fmt",
    "qpsk_demod_set_input_scale", "qpsk_demod_get_input_scale", "qpsk_rx_create_fmt", "qpsk_rx_next_slot_fmt",
    "qpsk_rx_submit_fmt", "qpsk_demod_group_process_fmt",
    "qpsk_state_blob_check",
    "qpsk_link_stats_size", "qpsk_demod_enable_link_stats", "qpsk_demod_link_stats",
    "qpsk_demod_group_enable_link_stats", "qpsk_demod_group_link_stats",
    "qpsk_stream_list_check", "qpsk_state_blob_select", "qpsk_state_blob_merge",
    "qpsk_demod_reset_streams", "qpsk_demod_streams_state_bytes", "qpsk_demod_get_streams_state",
    "qpsk_demod_set_streams_state", "qpsk_demod_group_reset_streams", "qpsk_demod_group_streams_state_bytes",
    "qpsk_demod_group_get_streams_state", "qpsk_demod_group_set_streams_state",
    "qpsk_framer_dev_reset_streams", "qpsk_frames_pack_device", "qpsk_rx_attach_framer", "qpsk_rx_set_markers",
    "qpsk_rx_frames_bytes", "qpsk_rx_collect_frames", "qpsk_rx_reset_streams",
    "qpsk_quantise_iq", "qpsk_mod_modulate_fmt", "qpsk_mod_modulate_bytes_fmt",
    "qpsk_ber_params_init", "qpsk_ber_row_size", "qpsk_ber_count", "qpsk_ber_count_device",
    "qpsk_channel_params_init", "qpsk_channel_create", "qpsk_channel_destroy", "qpsk_channel_set_stream",
    "qpsk_channel_apply_fmt", "qpsk_channel_state_size", "qpsk_channel_get_state", "qpsk_channel_set_state",
    "qpsk_channel_reset_streams", "qpsk_channel_state_check",
    "qpsk_path_params_init", "qpsk_path_create", "qpsk_path_destroy", "qpsk_path_set_stream", "qpsk_path_set_taps",
    "qpsk_path_apply_fmt", "qpsk_path_out_bound", "qpsk_path_count", "qpsk_path_state_size", "qpsk_path_state_init",
    "qpsk_path_get_state", "qpsk_path_set_state", "qpsk_path_reset_streams", "qpsk_path_state_check",
    "qpsk_path_apply_host",
    "qpsk_pfb_params_init", "qpsk_pfb_create", "qpsk_pfb_destroy", "qpsk_pfb_set_stream", "qpsk_pfb_design",
    "qpsk_pfb_twiddles", "qpsk_pfb_set_taps", "qpsk_pfb_count", "qpsk_pfb_out_bound", "qpsk_pfb_tile_frames",
    "qpsk_pfb_apply_fmt", "qpsk_pfb_state_size", "qpsk_pfb_state_init", "qpsk_pfb_get_state", "qpsk_pfb_set_state",
    "qpsk_pfb_reset_bands", "qpsk_pfb_state_check", "qpsk_pfb_apply_host",
    "qpsk_sfb_params_init", "qpsk_sfb_create", "qpsk_sfb_destroy", "qpsk_sfb_set_stream", "qpsk_sfb_set_taps",
    "qpsk_sfb_tile_frames", "qpsk_sfb_apply_fmt", "qpsk_sfb_state_size", "qpsk_sfb_state_init", "qpsk_sfb_get_state",
    "qpsk_sfb_set_state", "qpsk_sfb_reset_bands", "qpsk_sfb_state_check", "qpsk_sfb_apply_host",
    "qpsk_tuner_params_init", "qpsk_tuner_create", "qpsk_tuner_destroy", "qpsk_tuner_set_stream", "qpsk_tuner_design",
    "qpsk_tuner_tables", "qpsk_tuner_osc", "qpsk_tuner_set_taps", "qpsk_tuner_set_freq", "qpsk_tuner_apply_fmt",
    "qpsk_tuner_out_bound", "qpsk_tuner_count", "qpsk_tuner_state_size", "qpsk_tuner_state_init",
    "qpsk_tuner_get_state", "qpsk_tuner_set_state", "qpsk_tuner_reset_streams", "qpsk_tuner_state_check",
    "qpsk_tuner_apply_host",
]

_EXC = {
    QPSK_ERR_ARGUMENT: ValueError,
    QPSK_ERR_ARGUMENT_NULL: ValueError,
    QPSK_ERR_OUT_OF_RANGE: ValueError,
    QPSK_ERR_CAPACITY: ValueError,
}


def _check(rc):
    if rc < 0:
        msg = lib().qpsk_last_error().decode(errors="replace")
        raise _EXC.get(rc, QPSKError)(f"qpsk error {rc}: {msg}")
    return rc


def params(sample_rate, symbol_rate, rrc_alpha=0.9, rrc_span=6, symbol_sync_bandwidth=0.0001,
           costas_loop_bandwidth=120.0, cfo_loop_bandwidth=None, differential=True,
           enable_fll=False, vector_lanes=8, device=0, max_samples_per_call=1 << 20,
           loop_variant=0, iq_balance=False, costas_trig=0):
    """qpsk_demod_params (include/qpsk_demod.h); costas_trig = 1 runs the
    Costas NCO with glibc's own sin / cos (bit-identical symbols vs the
    libm oracle), 0 the faster portable table sincos."""
    p = DemodParams()
    lib().qpsk_demod_params_init(C.byref(p), int(sample_rate), int(symbol_rate))
    p.rrc_alpha = float(np.float32(rrc_alpha))
    p.rrc_span = int(rrc_span)
    p.symbol_sync_bandwidth = float(symbol_sync_bandwidth)
    p.costas_loop_bandwidth = float(costas_loop_bandwidth)
    if cfo_loop_bandwidth is not None:
        p.cfo_loop_bandwidth = float(cfo_loop_bandwidth)
    p.differential = 1 if differential else 0
    p.enable_fll = 1 if enable_fll else 0
    p.vector_lanes = int(vector_lanes)
    p.device = int(device)
    p.max_samples_per_call = int(max_samples_per_call)
    p.loop_variant = int(loop_variant)
    p.iq_balance = 1 if iq_balance else 0
    p.costas_trig = int(costas_trig)
    return p


def unpack_bits(row: np.ndarray, n_bits: int) -> str:
    """Packed MSB-first bits -> '0'/'1' string (the reference's bit strings)."""
    if n_bits <= 0:
        return ""
    b = np.unpackbits(np.asarray(row, dtype=np.uint8)[: (n_bits + 7) // 8])[:n_bits]
    return (b + ord("0")).astype(np.uint8).tobytes().decode()


def pack_bits(bits: str) -> np.ndarray:
    a = np.frombuffer(bits.encode(), dtype=np.uint8) - ord("0")
    return np.packbits(a)


# a qpsk_demod_get_state blob: a 32-byte header (magic "QPSK", format 2,
# streams, taps, carry, FLL taps, record size), then StreamState[S]
# (csrc/qpsk_state.h), carries, FIR histories, FLL delay lines
STATE_HEADER_BYTES = 32
# StreamState (csrc/qpsk_state.h)
STREAM_STATE_DTYPE = np.dtype([("mu", "f8"), ("integ", "f8"), ("theta", "f8"), ("freq", "f8"),
                               ("base", "i4"), ("has_prev", "i4"), ("psi", "f4"), ("psq", "f4"),
                               ("pdi", "f4"), ("pdq", "f4"), ("carry_n", "i4"), ("diff_have", "i4"),
                               ("diff_pi", "f4"), ("diff_pq", "f4"), ("fll_phase", "f4"),
                               ("fll_freq", "f4"), ("fll_pos", "i4"), ("error", "i4"), ("tofs", "i8"),
                               ("iqb_re", "f4"), ("iqb_im", "f4"), ("_pad", "V8")])   # alignas(16): 112 B
STATE_CARRY_MAX = 256   # kCarryMax
STATE_FLL_TAPS = 40     # kFllTaps


# qpsk_link_stats (include/qpsk_demod.h): one 64-byte row per stream
LINK_STATS_DTYPE = np.dtype([("n_symbols", "i8"), ("sum_dist2", "f8"), ("sum_power", "f8"),
                             ("costas_freq", "f8"), ("costas_theta", "f8"), ("mm_mu", "f8"),
                             ("mm_rate", "f8"), ("fll_freq", "f4"), ("error", "i4")])


class LinkStats(C.Structure):
    """qpsk_link_stats as a ctypes structure (LINK_STATS_DTYPE is the same layout)."""
    _fields_ = [("n_symbols", C.c_int64), ("sum_dist2", C.c_double), ("sum_power", C.c_double),
                ("costas_freq", C.c_double), ("costas_theta", C.c_double), ("mm_mu", C.c_double),
                ("mm_rate", C.c_double), ("fll_freq", C.c_float), ("error", C.c_int32)]


def link_stats_size() -> int:
    """sizeof(qpsk_link_stats) as the library was built (needs no device)."""
    return int(lib().qpsk_link_stats_size())


# qpsk_ber_row (include/qpsk_demod.h): one 64-byte row per stream
BER_ROW_DTYPE = np.dtype([("bit_errors", "i8"), ("bits", "i8"), ("lost_windows", "i8"), ("slips", "i8"),
                          ("windows", "i8"), ("last_offset", "i8"), ("located", "i4"), ("reserved", "i4", (3,))])


class BerRow(C.Structure):
    """qpsk_ber_row as a ctypes structure (BER_ROW_DTYPE is the same layout)."""
    _fields_ = [("bit_errors", C.c_int64), ("bits", C.c_int64), ("lost_windows", C.c_int64), ("slips", C.c_int64),
                ("windows", C.c_int64), ("last_offset", C.c_int64), ("located", C.c_int32),
                ("reserved", C.c_int32 * 3)]


def ber_row_size() -> int:
    """sizeof(qpsk_ber_row) as the library was built (needs no device)."""
    return int(lib().qpsk_ber_row_size())


def ber_params(skip_bits=None, window=None, key_bits=None, search=None) -> BerParams:
    """qpsk_ber_params_init's values (8000, 2048, 64, 512: bench.py's), then the ones given."""
    p = BerParams()
    lib().qpsk_ber_params_init(C.byref(p))
    for name, v in (("skip_bits", skip_bits), ("window", window), ("key_bits", key_bits), ("search", search)):
        if v is not None:
            setattr(p, name, int(v))
    return p


def ber_count(rx, n_rx, ref, n_ref=None, **params) -> np.ndarray:
    """qpsk_ber_count on host rows (needs no device): rx [S, B] and ref [S, B']
    uint8, packed MSB-first, rows of any stride; n_rx [S] bit counts; n_ref
    None = the whole row, 8 * ref.shape[1], as bench.py's ber_after_lock takes
    it.  params: skip_bits, window, key_bits, search.  Returns [S] rows of
    BER_ROW_DTYPE."""
    rx, ref = np.asarray(rx), np.asarray(ref)
    if rx.dtype != np.uint8 or ref.dtype != np.uint8 or rx.ndim != 2 or ref.ndim != 2:
        raise ValueError("rx and ref are [S, bytes] uint8 rows")
    S = rx.shape[0]
    if ref.shape[0] != S:
        raise ValueError("rx and ref hold different numbers of rows")
    if S == 0:
        return np.zeros(0, BER_ROW_DTYPE)
    if (rx.shape[1] > 1 and rx.strides[1] != 1) or (ref.shape[1] > 1 and ref.strides[1] != 1):
        raise ValueError("the bytes of a row must be contiguous")
    n_rx = np.ascontiguousarray(n_rx, dtype=np.int64).reshape(-1)
    n_ref = (np.full(S, 8 * ref.shape[1], np.int64) if n_ref is None
             else np.ascontiguousarray(n_ref, dtype=np.int64).reshape(-1))
    if n_rx.size != S or n_ref.size != S:
        raise ValueError("one bit count per row")
    out = np.zeros(S, BER_ROW_DTYPE)
    # the caller's own strides; numpy gives a new axis stride 0, and then a lone row's width serves
    rx_stride = rx.strides[0] if rx.strides[0] > 0 or S > 1 else rx.shape[1]
    ref_stride = ref.strides[0] if ref.strides[0] > 0 or S > 1 else ref.shape[1]
    _check(lib().qpsk_ber_count(C.byref(ber_params(**params)), rx.ctypes.data, rx_stride, n_rx.ctypes.data,
                                ref.ctypes.data, ref_stride, n_ref.ctypes.data, S, out.ctypes.data))
    return out


def ber_count_device(rx_dev, n_rx_dev, ref_dev, n_ref_dev, out_dev=None, hip_stream=None, **params):
    """qpsk_ber_count_device on torch CUDA tensors, nothing copied: rx_dev [S, B]
    and ref_dev [S, B'] uint8 rows (any stride and alignment), n_rx_dev and
    n_ref_dev [S] int64 on the device, out_dev [S, 64] uint8 (8-byte aligned;
    made here if None).  The kernel is ordered on hip_stream, or on torch's
    current stream if None, and the call does not wait for it.  Returns out_dev;
    out_dev.cpu().numpy().view(BER_ROW_DTYPE).reshape(-1) are its rows."""
    import torch
    for t, what in ((rx_dev, "rx_dev"), (ref_dev, "ref_dev")):
        if t.dtype != torch.uint8 or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
            raise ValueError(f"{what} must be a contiguous-row uint8 [n_streams, bytes] tensor")
    S = int(rx_dev.shape[0])
    for t, what in ((n_rx_dev, "n_rx_dev"), (n_ref_dev, "n_ref_dev")):
        if t.dtype != torch.int64 or t.numel() != S or not t.is_contiguous():
            raise ValueError(f"{what} must be a contiguous int64 [n_streams] tensor")
    if ref_dev.shape[0] != S:
        raise ValueError("rx_dev and ref_dev hold different numbers of rows")
    if out_dev is not None and (out_dev.dtype != torch.uint8 or not out_dev.is_contiguous()
                                or out_dev.numel() != S * BER_ROW_DTYPE.itemsize):
        raise ValueError("out_dev must be a contiguous uint8 tensor of 64 bytes a stream")
    if out_dev is None:
        out_dev = torch.empty((S, BER_ROW_DTYPE.itemsize), dtype=torch.uint8, device=rx_dev.device)
    if S == 0:
        return out_dev
    if hip_stream is None:
        hip_stream = torch.cuda.current_stream(rx_dev.device).cuda_stream
    # the caller's own strides; a lone row of stride 0 (an expanded view) takes its width, as in ber_count
    rx_stride = rx_dev.stride(0) if rx_dev.stride(0) > 0 or S > 1 else rx_dev.shape[1]
    ref_stride = ref_dev.stride(0) if ref_dev.stride(0) > 0 or S > 1 else ref_dev.shape[1]
    _check(lib().qpsk_ber_count_device(
        C.byref(ber_params(**params)), rx_dev.data_ptr(), rx_stride, n_rx_dev.data_ptr(), ref_dev.data_ptr(),
        ref_stride, n_ref_dev.data_ptr(), S, out_dev.data_ptr(), C.c_void_p(hip_stream or 0)))
    return out_dev


def ber_summary(rows) -> dict:
    """The figures bench.py reports under "ber_after_lock", summed over rows of BER_ROW_DTYPE."""
    rows = np.asarray(rows)
    if rows.dtype != BER_ROW_DTYPE:                     # [S, 64] uint8, as ber_count_device returns them
        rows = np.ascontiguousarray(rows).view(BER_ROW_DTYPE)
    rows = rows.reshape(-1)
    errs, bits = int(rows["bit_errors"].sum()), int(rows["bits"].sum())
    return {"bit_errors": errs, "bits": bits, "ber": (errs / bits) if bits else None,
            "lost_windows": int(rows["lost_windows"].sum()), "symbol_slips": int(rows["slips"].sum()),
            "streams": int(rows.size)}


def state_blob_check(p: DemodParams, n_streams: int, blob: bytes):
    """qpsk_state_blob_check: what set_state checks of a blob for a handle of
    n_streams streams and params p, on the host (needs no device).  Raises
    ValueError naming the stream, the field, its value and the allowed range."""
    buf = C.create_string_buffer(bytes(blob), max(len(blob), 1))
    _check(lib().qpsk_state_blob_check(C.byref(p), int(n_streams), buf, len(blob)))


def state_blob_parts(blob: bytes, n_streams: int, taps: int):
    """The sections of a blob as arrays (copies): records [S] (STREAM_STATE_DTYPE),
    carries [S, 256, 2], FIR histories [S, taps - 1, 2] (oldest sample first),
    FLL delay lines [S, 80, 2] (the reference's doubled line: entry q and
    q + 40 hold the sample last written at position q)."""
    S, H = int(n_streams), int(taps) - 1
    o = STATE_HEADER_BYTES
    rec = np.frombuffer(blob, dtype=STREAM_STATE_DTYPE, count=S, offset=o).copy()
    o += S * STREAM_STATE_DTYPE.itemsize
    carry = np.frombuffer(blob, dtype=np.float32, count=S * STATE_CARRY_MAX * 2, offset=o)
    o += carry.nbytes
    hist = np.frombuffer(blob, dtype=np.float32, count=S * H * 2, offset=o)
    o += hist.nbytes
    dl = np.frombuffer(blob, dtype=np.float32, count=S * 2 * STATE_FLL_TAPS * 2, offset=o)
    assert o + dl.nbytes == len(blob)
    return (rec, carry.reshape(S, STATE_CARRY_MAX, 2).copy(), hist.reshape(S, H, 2).copy(),
            dl.reshape(S, 2 * STATE_FLL_TAPS, 2).copy())


def _stream_list(streams):
    """A stream list as (ctypes int32 array, n); indices are passed on as they
    are, for the library to check."""
    ids = [int(v) for v in streams]
    return (C.c_int32 * max(len(ids), 1))(*ids), len(ids)


def stream_list_check(n_streams: int, streams):
    """qpsk_stream_list_check: 1 <= len(streams) <= n_streams, every index in
    [0, n_streams), none twice (needs no device).  Raises ValueError naming
    the position and the value."""
    ids, n = _stream_list(streams)
    _check(lib().qpsk_stream_list_check(int(n_streams), ids, n))


def state_blob_select(p: DemodParams, n_streams: int, blob: bytes, streams) -> bytes:
    """qpsk_state_blob_select: the rows `streams` of an n_streams blob, in
    list order, as a blob of len(streams) streams (needs no device)."""
    ids, n = _stream_list(streams)
    taps = design(p)[0].size
    src = C.create_string_buffer(bytes(blob), max(len(blob), 1))
    sub = C.create_string_buffer(state_blob_bytes(max(n, 1), taps))
    _check(lib().qpsk_state_blob_select(C.byref(p), int(n_streams), src, len(blob), ids, n, sub, len(sub)))
    return sub.raw


def state_blob_merge(p: DemodParams, n_streams: int, blob: bytes, streams, sub: bytes) -> bytes:
    """qpsk_state_blob_merge: a copy of blob whose rows `streams` are the rows
    of sub, a blob of len(streams) streams (needs no device)."""
    ids, n = _stream_list(streams)
    dst = C.create_string_buffer(bytes(blob), max(len(blob), 1))
    src = C.create_string_buffer(bytes(sub), max(len(sub), 1))
    _check(lib().qpsk_state_blob_merge(C.byref(p), int(n_streams), dst, len(blob), ids, n, src, len(sub)))
    return dst.raw[:len(blob)]


def state_blob_bytes(n_streams: int, taps: int) -> int:
    """Bytes of a state blob of n_streams streams of a taps-tap matched filter."""
    return STATE_HEADER_BYTES + int(n_streams) * (STREAM_STATE_DTYPE.itemsize + 8 * STATE_CARRY_MAX +
                                                  8 * (int(taps) - 1) + 8 * 2 * STATE_FLL_TAPS)


class _StreamRows:
    """reset_streams / get_streams_state / set_streams_state over a handle or a
    group: _rows_owner() gives the entry points' prefix and the C object."""

    def reset_streams(self, streams):
        """`new QPSKDeModulator(...)` on the listed rows: loops, filter history,
        FLL and IQ-balancer state, differential decoder, sticky error and the
        rows' link sums go back to construction.  Waits for every queued call.
        An empty list does nothing."""
        prefix, obj = self._rows_owner()
        ids, n = _stream_list(streams)
        _check(getattr(lib(), prefix + "_reset_streams")(obj, ids, n))

    def get_streams_state(self, streams) -> bytes:
        """The listed rows, in list order, as a state blob of len(streams)
        streams (what state_blob_select cuts from get_state()).  Waits for
        every queued call."""
        prefix, obj = self._rows_owner()
        ids, n = _stream_list(streams)
        size = getattr(lib(), prefix + "_streams_state_bytes")(obj, n)
        buf = C.create_string_buffer(max(size, 1))
        _check(getattr(lib(), prefix + "_get_streams_state")(obj, ids, n, buf, size))
        return buf.raw[:size]

    def set_streams_state(self, streams, sub: bytes):
        """Overwrite the listed rows with the rows of sub, a blob of
        len(streams) streams.  A bad list or a sub-blob that fails
        state_blob_check raises ValueError and changes nothing.  The link
        sums stay as they are."""
        prefix, obj = self._rows_owner()
        ids, n = _stream_list(streams)
        buf = C.create_string_buffer(bytes(sub), max(len(sub), 1))
        _check(getattr(lib(), prefix + "_set_streams_state")(obj, ids, n, buf, len(sub)))


class BatchDemodulator(_StreamRows):
    """A batch of S independent reference demodulators on one MI355X."""

    def _rows_owner(self):
        return "qpsk_demod", self._h

    def __init__(self, n_streams: int, p: DemodParams):
        self.S = int(n_streams)
        self.p = p
        h = C.c_void_p()
        _check(lib().qpsk_demod_create(C.byref(p), self.S, C.byref(h)))
        self._h = h
        self._bound = False   # set_stream(torch's stream) orders device calls on it

    def close(self):
        if getattr(self, "_h", None):
            lib().qpsk_demod_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream_ptr: int | None):
        _check(lib().qpsk_demod_set_stream(self._h, C.c_void_p(hip_stream_ptr or 0)))
        self._bound = bool(hip_stream_ptr)

    def _after_torch(self, t):
        """The handle's own stream (no set_stream) does not order against torch's:
        wait for torch's queued work on the tensors (their zero-fills, copies)
        before the library's kernels read or write them.  Round 6: with an
        experimental faster matched filter, test_rows_past_4gib_bit_exact saw
        its symbol rows' first entries zeroed after the loop kernel wrote them,
        by the torch.zeros still queued on torch's stream
        (profiles/r06_red_stream_race_gputest.log)."""
        if not self._bound:
            import torch
            torch.cuda.current_stream(t.device).synchronize()

    def max_symbols(self, n: int) -> int:
        return int(lib().qpsk_demod_max_symbols(self._h, int(n)))

    def enable_timing(self, on=True):
        _check(lib().qpsk_demod_enable_timing(self._h, 1 if on else 0))

    def enable_fir_phases(self, on=True):
        _check(lib().qpsk_demod_enable_fir_phases(self._h, 1 if on else 0))

    def fir_phases(self) -> dict:
        """Mean shader cycles per sampled FIR workgroup and phase, on CUs a
        loop workgroup held ("shared") and on the others ("free"); the sums
        are cleared (qpsk_demod_fir_phases)."""
        out = np.zeros(16, dtype=np.uint64)
        _check(lib().qpsk_demod_fir_phases(self._h, out.ctypes.data, 16))
        res = {}
        for name, k in (("free", 0), ("shared", 1)):
            cnt = int(out[8 * k + 3])
            res[name] = {"workgroups": cnt, **{ph: (round(int(out[8 * k + i]) / cnt, 1) if cnt else None)
                                               for i, ph in enumerate(("stage", "compute", "store"))}}
        return res

    def stage_times(self):
        """Average kernel launch times (ms) of the calls since enable_timing:
        the kernels' own first-workgroup-start to last-workgroup-end spans."""
        ms = (C.c_float * 4)()
        _check(lib().qpsk_demod_stage_times(self._h, ms, 4))
        return {"fll": ms[0], "fir": ms[1], "loop": ms[2], "total": ms[3]}

    def launch_times(self, max_calls=4096) -> np.ndarray:
        """[calls, 4] float32: FLL, FIR, loop kernel and the call's kernel span
        (ms) per call since enable_timing; 0 = the kernel did not run."""
        out = np.zeros((max_calls, 4), dtype=np.float32)
        k = _check(lib().qpsk_demod_launch_times(self._h, out.ctypes.data_as(_f32p), max_calls))
        return out[:k].copy()

    def kernel_clocks(self, max_calls=4096) -> np.ndarray:
        """[calls, 3] float32: the shader clock (GHz) the FLL, FIR and loop
        kernel of each recorded call ran at (qpsk_demod_kernel_clocks; 0 = the
        kernel did not run)."""
        out = np.zeros((max_calls, 3), dtype=np.float32)
        k = _check(lib().qpsk_demod_kernel_clocks(self._h, out.ctypes.data_as(_f32p), max_calls))
        return out[:k].copy()

    def rrc_taps(self):
        out = np.zeros(4096, dtype=np.float32)
        n = _check(lib().qpsk_demod_rrc_taps(self._h, out.ctypes.data_as(_f32p), 4096))
        return out[:n].copy()

    def gains(self):
        v = [C.c_double() for _ in range(5)]
        _check(lib().qpsk_demod_gains(self._h, *[C.byref(x) for x in v]))
        return dict(zip(["mm_sps", "kp", "ki", "costas_alpha", "costas_beta"], [x.value for x in v]))

    def fll_taps(self):
        lo = np.zeros(80, dtype=np.float32)
        up = np.zeros(80, dtype=np.float32)
        _check(lib().qpsk_demod_fll_taps(self._h, lo.ctypes.data_as(_f32p), up.ctypes.data_as(_f32p), 80))
        return lo, up

    def status(self) -> int:
        """OR of the STATUS_* flags raised since the last status() call (waits
        for every queued call; qpsk_demod_status)."""
        f = C.c_uint32()
        _check(lib().qpsk_demod_status(self._h, C.byref(f)))
        return int(f.value)

    def enable_link_stats(self, on=True):
        """Per-stream link statistics on or off (qpsk_demod_enable_link_stats):
        waits for every queued call; turning them on zeroes every stream's sums."""
        _check(lib().qpsk_demod_enable_link_stats(self._h, 1 if on else 0))

    def link_stats(self, reset=False) -> np.ndarray:
        """[S] LINK_STATS_DTYPE: every stream's symbol count, sums of dist2 and
        power since the last reset, and its loop state now (waits for every
        queued call; qpsk_demod_link_stats).  reset zeroes the sums behind the
        read.  QPSKError (QPSK_ERR_STATE) while statistics are not enabled."""
        out = np.zeros(self.S, dtype=LINK_STATS_DTYPE)
        _check(lib().qpsk_demod_link_stats(self._h, out.ctypes.data, MEM_HOST, 1 if reset else 0))
        return out

    def link_stats_device(self, out_tensor, reset=False):
        """link_stats() into device memory: out_tensor holds at least 64 * S
        contiguous bytes on the handle's device, 8-byte aligned; the rows are
        written in order on the handle's stream.  Returns out_tensor."""
        if not out_tensor.is_cuda or not out_tensor.is_contiguous():
            raise ValueError("out_tensor must be a contiguous device tensor")
        if out_tensor.numel() * out_tensor.element_size() < self.S * LINK_STATS_DTYPE.itemsize:
            raise ValueError("out_tensor holds fewer than 64 bytes a stream")
        self._after_torch(out_tensor)
        _check(lib().qpsk_demod_link_stats(self._h, out_tensor.data_ptr(), MEM_DEVICE, 1 if reset else 0))
        return out_tensor

    def last_mf(self, n: int) -> np.ndarray:
        """[S, 2n] float32: the matched-filter output of the last synchronous call."""
        out = np.zeros((self.S, max(2 * int(n), 2)), dtype=np.float32)
        _check(lib().qpsk_demod_last_mf(self._h, out.ctypes.data, out.shape[1], int(n), MEM_HOST))
        return out[:, : 2 * int(n)]

    def get_state(self) -> bytes:
        n = lib().qpsk_demod_state_bytes(self._h)
        buf = C.create_string_buffer(n)
        _check(lib().qpsk_demod_get_state(self._h, buf, n))
        return buf.raw

    def stream_states(self, blob: bytes | None = None) -> np.ndarray:
        """The per-stream loop state records (StreamState, csrc/qpsk_state.h)
        at the head of a get_state() blob, as a structured array [S]."""
        blob = self.get_state() if blob is None else blob
        return np.frombuffer(blob[STATE_HEADER_BYTES: STATE_HEADER_BYTES + self.S * STREAM_STATE_DTYPE.itemsize],
                             dtype=STREAM_STATE_DTYPE)

    def set_state(self, blob: bytes):
        """Restore a get_state() blob of a handle of the same shape (streams,
        taps); any other blob, and one whose records fail state_blob_check,
        raises (QPSK_ERR_ARGUMENT) and leaves the handle as it was."""
        buf = C.create_string_buffer(bytes(blob), len(blob))
        _check(lib().qpsk_demod_set_state(self._h, buf, len(blob)))

    # ---- CS16 (interleaved int16 I,Q) input -------------------------------
    def set_cs16_scale(self, scale: float):
        """A CS16 sample's value is float32(x) * scale (default 1 / 32768); applies
        to calls issued from now on.  Finite and > 0, else ValueError."""
        _check(lib().qpsk_demod_set_cs16_scale(self._h, C.c_float(float(np.float32(scale)))))

    def cs16_scale(self) -> float:
        v = C.c_float()
        _check(lib().qpsk_demod_get_cs16_scale(self._h, C.byref(v)))
        return float(v.value)

    def process_cs16(self, iq: np.ndarray, mode=MODE_DEMODULATE, lengths=None, want_syms=False):
        """process() on an [S, 2n] int16 host array (qpsk_demod_process_cs16); any
        other dtype raises: nothing is converted on the way."""
        if np.asarray(iq).dtype != np.int16:
            raise ValueError("process_cs16 takes int16 samples")
        return self._process_host(lib().qpsk_demod_process_cs16, np.ascontiguousarray(iq), mode, lengths,
                                  want_syms)

    def process_device_cs16(self, iq_dev, n, bits_dev, n_bits_dev, mode=MODE_DEMODULATE,
                            syms_dev=None, n_syms_dev=None, lengths=None):
        """process_device() on an int16 [S, >= 2n] torch CUDA tensor; lengths:
        optional host int64 array of per-stream sample counts."""
        self._device_call(lib().qpsk_demod_process_cs16, FMT_CS16, iq_dev, n, bits_dev, n_bits_dev, mode, syms_dev,
                          n_syms_dev, lengths, False)

    def process_device_async_cs16(self, iq_dev, n, bits_dev, n_bits_dev, mode=MODE_DEMODULATE,
                                  syms_dev=None, n_syms_dev=None, lengths=None):
        """process_device_async() on an int16 [S, >= 2n] torch CUDA tensor."""
        self._device_call(lib().qpsk_demod_process_async_cs16, FMT_CS16, iq_dev, n, bits_dev, n_bits_dev, mode,
                          syms_dev, n_syms_dev, lengths, True)

    # ---- any format (CF32, CS16, CS8, CU8) through the *_fmt entry points --
    def set_input_scale(self, fmt, scale: float):
        """The scale of an integer format ("cs16": the one set_cs16_scale sets;
        "cs8" / "cu8": default 1 / 128); applies to calls issued from now on.
        Finite and > 0, else ValueError; "cf32" has none (ValueError)."""
        _check(lib().qpsk_demod_set_input_scale(self._h, _format(fmt)[0], C.c_float(float(np.float32(scale)))))

    def input_scale(self, fmt) -> float:
        v = C.c_float()
        _check(lib().qpsk_demod_get_input_scale(self._h, _format(fmt)[0], C.byref(v)))
        return float(v.value)

    def process_fmt(self, iq: np.ndarray, fmt, mode=MODE_DEMODULATE, lengths=None, want_syms=False):
        """process() on an [S, 2n] host array of the format's element type
        (float32, int16, int8 for "cs8", uint8 for "cu8"); any other dtype
        raises: nothing is converted on the way."""
        tag, dtype, _ = _format(fmt)
        if np.asarray(iq).dtype != dtype:
            raise ValueError(f"process_fmt({fmt!r}) takes {np.dtype(dtype).name} samples")
        fn = lib().qpsk_demod_process_fmt
        return self._process_host(lambda h, *a: fn(h, tag, *a), np.ascontiguousarray(iq), mode, lengths, want_syms)

    def process_device_fmt(self, iq_dev, n, bits_dev, n_bits_dev, fmt, mode=MODE_DEMODULATE,
                           syms_dev=None, n_syms_dev=None, lengths=None):
        """process_device() on an [S, >= 2n] torch CUDA tensor of the format's
        element type; lengths: optional host int64 array of per-stream counts."""
        tag = _format(fmt)[0]
        fn = lib().qpsk_demod_process_fmt
        self._device_call(lambda h, *a: fn(h, tag, *a), tag, iq_dev, n, bits_dev, n_bits_dev, mode, syms_dev,
                          n_syms_dev, lengths, False)

    def process_device_async_fmt(self, iq_dev, n, bits_dev, n_bits_dev, fmt, mode=MODE_DEMODULATE,
                                 syms_dev=None, n_syms_dev=None, lengths=None):
        """process_device_async() on a tensor of the format's element type."""
        tag = _format(fmt)[0]
        fn = lib().qpsk_demod_process_async_fmt
        self._device_call(lambda h, *a: fn(h, tag, *a), tag, iq_dev, n, bits_dev, n_bits_dev, mode, syms_dev,
                          n_syms_dev, lengths, True)

    def _device_call(self, fn, fmt, iq_dev, n, bits_dev, n_bits_dev, mode, syms_dev, n_syms_dev, lengths,
                     is_async):
        self._check_device_args(iq_dev, n, bits_dev, n_bits_dev, syms_dev, n_syms_dev, fmt=int(fmt))
        self._after_torch(iq_dev)
        bstride = bits_dev.stride(0) * bits_dev.element_size() if bits_dev is not None else 0
        sstride = syms_dev.stride(0) if syms_dev is not None else 0
        if lengths is not None:
            lengths = np.ascontiguousarray(lengths, dtype=np.int64)
        head = (self._h, int(mode), iq_dev.data_ptr(), iq_dev.stride(0), int(n),
                lengths.ctypes.data_as(_i64p) if lengths is not None else None)
        tail = (bits_dev.data_ptr() if bits_dev is not None else None, bstride,
                n_bits_dev.data_ptr() if n_bits_dev is not None else None,
                syms_dev.data_ptr() if syms_dev is not None else None, sstride,
                n_syms_dev.data_ptr() if n_syms_dev is not None else None)
        _check(fn(*head, *tail) if is_async else fn(*head, MEM_DEVICE, *tail))

    # ---- host path --------------------------------------------------------
    def process(self, iq: np.ndarray, mode=MODE_DEMODULATE, lengths=None, want_syms=False):
        """iq: [S, 2n] float32 host array.  Returns (bits [S, B] uint8, n_bits [S],
        syms [S, 2M] float32 or None, n_syms [S])."""
        iq = np.ascontiguousarray(iq, dtype=np.float32)
        return self._process_host(lib().qpsk_demod_process, iq, mode, lengths, want_syms)

    def _process_host(self, fn, iq, mode, lengths, want_syms):
        if iq.ndim != 2 or iq.shape[0] != self.S:
            raise ValueError("iq must be [n_streams, 2*n]")
        if iq.shape[1] & 1:
            raise ValueError("Samples must be interleaved IQ with even length.")
        n = iq.shape[1] // 2
        if lengths is not None:
            lengths = np.ascontiguousarray(lengths, dtype=np.int64)
            if lengths.shape != (self.S,):
                raise ValueError("lengths must hold one count per stream")
            nmax = int(lengths.max()) if lengths.size else 0
            if nmax > n:
                raise ValueError("a length exceeds the row (iq.shape[1] // 2 samples)")
        else:
            nmax = n
        return _host_call(fn, self._h, self.S, self.max_symbols(nmax), iq, mode, lengths, want_syms)

    # ---- device path (torch tensors resident in HBM) ---------------------
    def _check_device_args(self, iq_dev, n, bits_dev, n_bits_dev, syms_dev, n_syms_dev, fmt=FMT_CF32):
        import torch
        want = _torch_dtype(fmt)
        if iq_dev.dtype != want or iq_dev.dim() != 2 or iq_dev.shape[0] != self.S:
            raise ValueError(f"iq_dev must be a {want} [n_streams, >= 2n] tensor")
        if iq_dev.stride(1) != 1 or iq_dev.shape[1] < 2 * int(n):
            raise ValueError("iq_dev rows must be contiguous and hold 2n elements")
        for t, dt, what in ((bits_dev, torch.uint8, "bits_dev"), (syms_dev, torch.float32, "syms_dev")):
            if t is not None and (t.dtype != dt or t.dim() != 2 or t.shape[0] != self.S or t.stride(1) != 1):
                raise ValueError(f"{what} must be a contiguous-row {dt} [n_streams, k] tensor")
        for t, what in ((n_bits_dev, "n_bits_dev"), (n_syms_dev, "n_syms_dev")):
            if t is not None and (t.dtype != torch.int64 or t.numel() != self.S or not t.is_contiguous()):
                raise ValueError(f"{what} must be a contiguous int64 [n_streams] tensor")

    def process_device(self, iq_dev, n, bits_dev, n_bits_dev, mode=MODE_DEMODULATE,
                       syms_dev=None, n_syms_dev=None):
        """All arguments are torch CUDA tensors; stream-ordered on the handle's
        stream (bind torch's stream with set_stream first; without it the call
        first waits for torch's current stream)."""
        self._device_call(lib().qpsk_demod_process, FMT_CF32, iq_dev, n, bits_dev, n_bits_dev, mode, syms_dev,
                          n_syms_dev, None, False)

    def process_device_async(self, iq_dev, n, bits_dev, n_bits_dev, mode=MODE_DEMODULATE,
                             syms_dev=None, n_syms_dev=None, lengths=None):
        """Pipelined call (qpsk_demod_process_async): returns once queued; the
        outputs are complete after pipeline_wait().  lengths: optional host
        int64 array of per-stream sample counts."""
        self._device_call(lib().qpsk_demod_process_async, FMT_CF32, iq_dev, n, bits_dev, n_bits_dev, mode,
                          syms_dev, n_syms_dev, lengths, True)

    def pipeline_wait(self, hip_stream_ptr: int | None = None):
        """hip_stream_ptr waits for every pipelined call (None: block the host)."""
        _check(lib().qpsk_demod_pipeline_wait(self._h, C.c_void_p(hip_stream_ptr or 0)))

    def pipeline_depth(self) -> int:
        return _check(lib().qpsk_demod_pipeline_depth(self._h))

    def gate_timeouts(self) -> int:
        """Residency-gate waits that ran out (QPSK_GATE_TIMEOUT_MS) so far."""
        v = C.c_uint64()
        _check(lib().qpsk_demod_gate_timeouts(self._h, C.byref(v)))
        return v.value


def shard_streams(n_streams: int, n_parts: int, k: int):
    """(first, count) of contiguous shard k of n_parts (qpsk_shard_streams;
    needs no device)."""
    f, c = C.c_int32(), C.c_int32()
    _check(lib().qpsk_shard_streams(int(n_streams), int(n_parts), int(k), C.byref(f), C.byref(c)))
    return f.value, c.value


class DemodGroup(_StreamRows):
    """One batch of streams over several GPUs (qpsk_demod_group_*): shard k =
    contiguous streams on devices[k], one handle each, fanned out per call on
    worker threads and joined.  process() takes the same host rows as
    BatchDemodulator.process over all n_streams and returns the same arrays.
    reset_streams / get_streams_state / set_streams_state take global ids."""

    def _rows_owner(self):
        return "qpsk_demod_group", self._g

    def __init__(self, n_streams: int, p: DemodParams, devices):
        self.S = int(n_streams)
        self.p = p
        devs = (C.c_int32 * len(devices))(*[int(d) for d in devices])
        g = C.c_void_p()
        _check(lib().qpsk_demod_group_create(C.byref(p), devs, len(devices), self.S, C.byref(g)))
        self._g = g
        # for max_symbols (every shard has the same params)
        self._h0 = self.shard(0)[3]

    def close(self):
        if getattr(self, "_g", None):
            lib().qpsk_demod_group_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self) -> int:
        return _check(lib().qpsk_demod_group_size(self._g))

    def shard(self, k: int):
        """(first_stream, n_streams, device, raw handle) of shard k."""
        f, n, d, h = C.c_int32(), C.c_int32(), C.c_int32(), C.c_void_p()
        _check(lib().qpsk_demod_group_shard(self._g, int(k), C.byref(f), C.byref(n), C.byref(d), C.byref(h)))
        return f.value, n.value, d.value, h

    def max_symbols(self, n: int) -> int:
        return int(lib().qpsk_demod_max_symbols(self._h0, int(n)))

    def get_state(self, k: int) -> bytes:
        n = lib().qpsk_demod_group_state_bytes(self._g, int(k))
        buf = C.create_string_buffer(n)
        _check(lib().qpsk_demod_group_get_state(self._g, int(k), buf, n))
        return buf.raw

    def set_state(self, k: int, blob: bytes):
        buf = C.create_string_buffer(bytes(blob), len(blob))
        _check(lib().qpsk_demod_group_set_state(self._g, int(k), buf, len(blob)))

    def enable_link_stats(self, on=True):
        """BatchDemodulator.enable_link_stats on every shard."""
        _check(lib().qpsk_demod_group_enable_link_stats(self._g, 1 if on else 0))

    def link_stats(self, reset=False) -> np.ndarray:
        """[S] LINK_STATS_DTYPE over the whole batch in stream order
        (qpsk_demod_group_link_stats), as BatchDemodulator.link_stats."""
        out = np.zeros(self.S, dtype=LINK_STATS_DTYPE)
        _check(lib().qpsk_demod_group_link_stats(self._g, out.ctypes.data, 1 if reset else 0))
        return out

    def process(self, iq: np.ndarray, mode=MODE_DEMODULATE, lengths=None, want_syms=False):
        """iq: [S, 2n] float32 host rows of the whole batch; returns (bits,
        n_bits, syms or None, n_syms) exactly as BatchDemodulator.process."""
        return self._process_host(lib().qpsk_demod_group_process, np.ascontiguousarray(iq, dtype=np.float32), mode,
                                  lengths, want_syms)

    def process_fmt(self, iq: np.ndarray, fmt, mode=MODE_DEMODULATE, lengths=None, want_syms=False):
        """process() on host rows of any format (qpsk_demod_group_process_fmt):
        [S, 2n] of the format's element type, nothing converted on the way."""
        tag, dtype, _ = _format(fmt)
        if np.asarray(iq).dtype != dtype:
            raise ValueError(f"process_fmt({fmt!r}) takes {np.dtype(dtype).name} samples")
        fn = lib().qpsk_demod_group_process_fmt
        return self._process_host(lambda g, *a: fn(g, tag, *a), np.ascontiguousarray(iq), mode, lengths, want_syms)

    def _process_host(self, fn, iq, mode, lengths, want_syms):
        if iq.ndim != 2 or iq.shape[0] != self.S or iq.shape[1] & 1:
            raise ValueError("iq must be [n_streams, 2*n]")
        n = iq.shape[1] // 2
        if lengths is not None:
            lengths = np.ascontiguousarray(lengths, dtype=np.int64)
            nmax = int(lengths.max()) if lengths.size else 0
        else:
            nmax = n
        return _host_call(fn, self._g, self.S, self.max_symbols(nmax), iq, mode, lengths, want_syms)

    def process_device(self, iq_dev, n, bits_dev, n_bits_dev, mode=MODE_DEMODULATE, syms_dev=None,
                       n_syms_dev=None):
        """Device rows of the whole batch (every shard on one device): returns
        with the outputs written.  The shards run on their handles' own
        streams, so the call first waits for torch's current stream."""
        self._process_device(lib().qpsk_demod_group_process, iq_dev, n, bits_dev, n_bits_dev, mode, syms_dev,
                             n_syms_dev)

    def process_device_fmt(self, iq_dev, n, bits_dev, n_bits_dev, fmt, mode=MODE_DEMODULATE, syms_dev=None,
                           n_syms_dev=None):
        """process_device() on device rows of any format (a tensor of the
        format's element type)."""
        tag = _format(fmt)[0]
        want = _torch_dtype(tag)
        if iq_dev.dtype != want:
            raise ValueError(f"process_device_fmt({fmt!r}) takes a {want} tensor")
        fn = lib().qpsk_demod_group_process_fmt
        self._process_device(lambda g, *a: fn(g, tag, *a), iq_dev, n, bits_dev, n_bits_dev, mode, syms_dev,
                             n_syms_dev)

    def _process_device(self, fn, iq_dev, n, bits_dev, n_bits_dev, mode, syms_dev, n_syms_dev):
        import torch
        torch.cuda.current_stream(iq_dev.device).synchronize()
        bstride = bits_dev.stride(0) * bits_dev.element_size() if bits_dev is not None else 0
        sstride = syms_dev.stride(0) if syms_dev is not None else 0
        _check(fn(
            self._g, int(mode), iq_dev.data_ptr(), iq_dev.stride(0), int(n), None, MEM_DEVICE,
            bits_dev.data_ptr() if bits_dev is not None else None, bstride,
            n_bits_dev.data_ptr() if n_bits_dev is not None else None,
            syms_dev.data_ptr() if syms_dev is not None else None, sstride,
            n_syms_dev.data_ptr() if n_syms_dev is not None else None))


class HostRing:
    """Host-fed streaming front-end over one BatchDemodulator (qpsk_rx_*, the
    ModDemodOverSDR.cs:116-183 receive loop): submit() queues one DeModulate call
    on host samples, collect() returns the oldest outstanding call's bits.  The
    handle must not be used directly while the ring lives."""

    def __init__(self, demod: "BatchDemodulator", depth: int = 2, fmt: str = "cf32"):
        """fmt "cf32": float32 slots; "cs16": int16 slots, half the pinned memory
        and upload bytes, widened by the matched filter."""
        if fmt not in ("cf32", "cs16"):
            raise ValueError("fmt must be 'cf32' or 'cs16' (HostRing.create_fmt makes a ring of any format)")
        self._open(demod, depth, fmt)

    @classmethod
    def create_fmt(cls, demod: "BatchDemodulator", depth: int = 2, fmt: str = "cs8") -> "HostRing":
        """A ring of any one format: "cs8" (int8 slots) and "cu8" (uint8 slots)
        are a quarter of the float ring's pinned memory and upload bytes; "cf32"
        and "cs16" are the constructor's rings."""
        ring = cls.__new__(cls)
        ring._open(demod, depth, fmt)
        return ring

    def _open(self, demod, depth, fmt):
        """Every ring goes through qpsk_rx_create_fmt / _next_slot_fmt / _submit_fmt."""
        self._r = C.c_void_p()
        self._tag, self._dtype, self._ctype = _format(fmt)
        self.fmt = next(k for k, v in _FORMATS.items() if v[0] == self._tag)
        self._demod = demod
        self.S = demod.S
        _check(lib().qpsk_rx_create_fmt(demod._h, int(depth), self._tag, C.byref(self._r)))
        ms = demod.max_symbols(int(demod.p.max_samples_per_call))
        self.bits_stride = (2 * ms + 7) // 8

    def next_slot(self) -> np.ndarray:
        """The pinned slot the next submit reads, as a writable (S, stride) view
        of the ring's sample type (float32, or int16 for a CS16 ring)."""
        ptr, stride = C.c_void_p(), C.c_int64()
        _check(lib().qpsk_rx_next_slot_fmt(self._r, self._tag, C.byref(ptr), C.byref(stride)))
        buf = (self._ctype * (self.S * stride.value)).from_address(ptr.value)
        return np.ctypeslib.as_array(buf).reshape(self.S, stride.value)

    def submit(self, iq: np.ndarray | None = None, n: int | None = None, lengths=None) -> int:
        """iq None: the slot from next_slot() (filled in place); else (S, >= 2n)
        rows of the ring's sample type (a CS16 ring takes int16 only)."""
        if iq is None:
            slot = self.next_slot()
            ptr, stride = slot.ctypes.data, slot.shape[1]
        else:
            if self.fmt != "cf32" and np.asarray(iq).dtype != self._dtype:
                raise ValueError(f"a {self.fmt.upper()} ring takes {np.dtype(self._dtype).name} samples")
            iq = np.ascontiguousarray(iq, dtype=self._dtype)
            assert iq.shape[0] == self.S
            ptr, stride = iq.ctypes.data, iq.shape[1]
        if n is None:
            n = stride // 2
        lens = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.int64)
        t = C.c_int64()
        _check(lib().qpsk_rx_submit_fmt(self._r, self._tag, C.c_void_p(ptr), int(stride), int(n),
                                        lens.ctypes.data_as(_i64p) if lens is not None else None, C.byref(t)))
        return t.value

    def collect(self):
        """(bits (S, stride) uint8, n_bits (S,) int64, ticket) of the oldest outstanding call."""
        bits = np.zeros((self.S, self.bits_stride), dtype=np.uint8)
        nb = np.zeros(self.S, dtype=np.int64)
        t = C.c_int64()
        _check(lib().qpsk_rx_collect(self._r, bits.ctypes.data_as(_u8p), self.bits_stride,
                                     nb.ctypes.data_as(_i64p), C.byref(t)))
        return bits, nb, t.value

    def attach_framer(self, start: bytes, end: bytes, tsc: str | None = None, ring_capacity=1 << 16,
                      max_frame_bytes=256, chunk_frame_bytes=0, keep_bits=False):
        """Give the ring a device framer (qpsk_rx_attach_framer): from now on
        every chunk's bits go through the TSC strip, the DeModulateBytes state
        machine (markers start / end, ring_capacity bytes a stream) and the
        packing kernel on the device, and collect_frames() returns the frames
        the chunk completed.  max_frame_bytes: the bytes of a frame that come
        back (longer ones are truncated and flagged); chunk_frame_bytes: the
        bytes of frames one chunk returns (0: n_streams * max_frame_bytes).
        keep_bits=False queues no bit download at all.  ring_capacity must hold
        one chunk's bit bytes (entering a frame appends the rest of the chunk's
        bits; the default suits chunks of up to 2^20 samples at sps 4).  Once
        per ring, with nothing outstanding (QPSKError otherwise)."""
        s, e = _markers(start, end)
        _check(lib().qpsk_rx_attach_framer(self._r, s.ctypes.data_as(_u8p), s.size, e.ctypes.data_as(_u8p), e.size,
                                           tsc.encode() if tsc else None, int(ring_capacity), int(max_frame_bytes),
                                           int(chunk_frame_bytes), 1 if keep_bits else 0))
        self.max_frame_bytes = (int(max_frame_bytes) + 15) // 16 * 16
        self.keep_bits = bool(keep_bits)

    def frames_bytes(self) -> int:
        """The bytes of frames one chunk can return (0: no framer attached)."""
        return int(lib().qpsk_rx_frames_bytes(self._r))

    def set_markers(self, start: bytes, end: bytes):
        """The markers of later submits (DeModulateBytes takes them per call);
        waits for the framer work already queued."""
        s, e = _markers(start, end)
        _check(lib().qpsk_rx_set_markers(self._r, s.ctypes.data_as(_u8p), s.size, e.ctypes.data_as(_u8p), e.size))

    def collect_frames(self, want_bits=False, frames_cap=None):
        """The oldest outstanding chunk of a framed ring: (frames, lengths,
        flags, ticket).  frames[s] is the frame DeModulateBytes returned on
        stream s for this chunk (its first max_frame_bytes bytes), or None;
        lengths (S,) int64 the frames' full lengths (0 = none); flags the OR
        of FRAMES_TRUNCATED and FRAMES_DROPPED (a dropped frame has a length
        and None for its bytes).  want_bits (a keep_bits ring): the chunk's
        (bits, n_bits) as collect() returns them follow the ticket.
        frames_cap: the size of the buffer handed to the library (default
        frames_bytes(), which always suffices)."""
        cap = self.frames_bytes() if frames_cap is None else int(frames_cap)
        buf = np.zeros(max(cap, 1), dtype=np.uint8)
        off = np.zeros(self.S, dtype=np.int64)
        lens = np.zeros(self.S, dtype=np.int64)
        bits = np.zeros((self.S, self.bits_stride), dtype=np.uint8) if want_bits else None
        nb = np.zeros(self.S, dtype=np.int64) if want_bits else None
        t = C.c_int64()
        rc = lib().qpsk_rx_collect_frames(self._r, buf.ctypes.data_as(_u8p), cap, off.ctypes.data_as(_i64p),
                                          lens.ctypes.data_as(_i64p),
                                          bits.ctypes.data_as(_u8p) if want_bits else None, self.bits_stride,
                                          nb.ctypes.data_as(_i64p) if want_bits else None, C.byref(t))
        if rc != QPSK_ERR_CAPACITY:     # a flagged chunk is consumed and its outputs are written
            _check(rc)
        P = getattr(self, "max_frame_bytes", 0)
        frames = [bytes(buf[int(off[s]): int(off[s]) + min(int(lens[s]), P)]) if off[s] >= 0 else None
                  for s in range(self.S)]
        flags = (FRAMES_TRUNCATED if (lens > P).any() else 0) | \
                (FRAMES_DROPPED if ((lens > 0) & (off < 0)).any() else 0)
        assert (rc == QPSK_ERR_CAPACITY) == bool(flags)
        return (frames, lens, flags, t.value) + ((bits, nb) if want_bits else ())

    def reset_streams(self, streams):
        """`new QPSKDeModulator(...)` on the listed rows between submits: the
        handle's rows (BatchDemodulator.reset_streams) and the framer's.  Waits
        for the outstanding chunks' work.  An empty list does nothing."""
        ids, n = _stream_list(streams)
        _check(lib().qpsk_rx_reset_streams(self._r, ids, n))

    def close(self):
        if getattr(self, "_r", None):
            _check(lib().qpsk_rx_destroy(self._r))
            self._r = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def design(p: DemodParams):
    """Constructor math without a GPU: (rrc taps, gains dict, fll lower, fll upper)."""
    taps = np.zeros(4096, dtype=np.float32)
    g = (C.c_double * 5)()
    lo = np.zeros(80, dtype=np.float32)
    up = np.zeros(80, dtype=np.float32)
    n = _check(lib().qpsk_demod_design(C.byref(p), taps.ctypes.data_as(_f32p), 4096, g,
                                       lo.ctypes.data_as(_f32p), up.ctypes.data_as(_f32p)))
    gains = dict(zip(["mm_sps", "kp", "ki", "costas_alpha", "costas_beta"], list(g)))
    return taps[:n].copy(), gains, lo, up


def tsc_find(bits_row: np.ndarray, n_bits: int, tsc: str | None) -> int:
    row = np.ascontiguousarray(bits_row, dtype=np.uint8)
    return int(lib().qpsk_tsc_find(row.ctypes.data_as(_u8p), int(n_bits),
                                    tsc.encode() if tsc else None))


class Framer:
    """Batched DeModulateBytes framer (QPSKDeModulator.cs:169-259)."""

    def __init__(self, n_streams, start: bytes, end: bytes, ring_capacity=300_000_000):
        if len(start) == 0:
            raise ValueError("startMarker cannot be empty.")
        if len(end) == 0:
            raise ValueError("endMarker cannot be empty.")
        self.S = n_streams
        s = np.frombuffer(start, dtype=np.uint8).copy()
        e = np.frombuffer(end, dtype=np.uint8).copy()
        h = C.c_void_p()
        _check(lib().qpsk_framer_create(n_streams, s.ctypes.data_as(_u8p), s.size,
                                        e.ctypes.data_as(_u8p), e.size, int(ring_capacity),
                                        C.byref(h)))
        self._h = h

    def set_markers(self, start: bytes, end: bytes):
        if len(start) == 0:
            raise ValueError("startMarker cannot be empty.")
        if len(end) == 0:
            raise ValueError("endMarker cannot be empty.")
        s = np.frombuffer(start, dtype=np.uint8).copy()
        e = np.frombuffer(end, dtype=np.uint8).copy()
        _check(lib().qpsk_framer_set_markers(self._h, s.ctypes.data_as(_u8p), s.size,
                                             e.ctypes.data_as(_u8p), e.size))

    def push(self, bits: np.ndarray, n_bits, offsets=None, payload_cap=1 << 16):
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        n_bits = np.ascontiguousarray(n_bits, dtype=np.int64)
        off = np.ascontiguousarray(offsets if offsets is not None else np.zeros(self.S), dtype=np.int64)
        pay = np.zeros((self.S, payload_cap), dtype=np.uint8)
        npay = np.zeros(self.S, dtype=np.int64)
        _check(lib().qpsk_framer_push(self._h, bits.ctypes.data_as(_u8p), bits.shape[1],
                                      off.ctypes.data_as(_i64p), n_bits.ctypes.data_as(_i64p),
                                      pay.ctypes.data_as(_u8p), payload_cap,
                                      npay.ctypes.data_as(_i64p)))
        return [bytes(pay[s, : min(int(npay[s]), payload_cap)]) for s in range(self.S)]

    def __del__(self):
        if getattr(self, "_h", None):
            lib().qpsk_framer_destroy(self._h)
            self._h = None


def _markers(start: bytes, end: bytes):
    if len(start) == 0:
        raise ValueError("startMarker cannot be empty.")                          # :174
    if len(end) == 0:
        raise ValueError("endMarker cannot be empty.")                            # :175
    return (np.frombuffer(bytes(start), dtype=np.uint8).copy(),
            np.frombuffer(bytes(end), dtype=np.uint8).copy())


def tsc_find_device(bits_dev, n_bits_dev, tsc: str | None, offsets_dev, hip_stream=None):
    """qpsk_tsc_find on every row of a device bit batch (torch CUDA tensors);
    offsets_dev[s] = first payload bit after the TSC, -1 if absent."""
    _check(lib().qpsk_tsc_find_device(
        bits_dev.data_ptr(), bits_dev.stride(0) * bits_dev.element_size(), n_bits_dev.data_ptr(),
        int(bits_dev.shape[0]), tsc.encode() if tsc else None, offsets_dev.data_ptr(),
        hip_stream))


def frames_pack_device(payload_dev, n_payload_dev, packed_dev, offsets_dev, head_dev, hip_stream=None,
                       packed_cap=None):
    """qpsk_frames_pack_device on torch CUDA tensors: the frames DeviceFramer.push
    left in payload_dev [S][P] / n_payload_dev [S], packed densely at 16-byte
    offsets into packed_dev (uint8, packed_cap bytes of it, default all);
    offsets_dev [S] int64 receives each frame's offset or -1, head_dev [2]
    int64 the bytes used and the FRAMES_* flags.  Ordered on hip_stream."""
    cap = packed_dev.numel() if packed_cap is None else int(packed_cap)
    _check(lib().qpsk_frames_pack_device(payload_dev.data_ptr(), payload_dev.stride(0), n_payload_dev.data_ptr(),
                                         int(payload_dev.shape[0]), packed_dev.data_ptr(), cap,
                                         offsets_dev.data_ptr(), head_dev.data_ptr(), hip_stream))


class DeviceFramer:
    """The DeModulateBytes framer (QPSKDeModulator.cs:169-259) resident on the
    GPU: fed straight from BatchDemodulator.process_device's bit rows."""

    def __init__(self, n_streams, start: bytes, end: bytes, ring_capacity=300_000_000, device=0):
        s, e = _markers(start, end)
        self.S = n_streams
        h = C.c_void_p()
        _check(lib().qpsk_framer_dev_create(n_streams, s.ctypes.data_as(_u8p), s.size,
                                            e.ctypes.data_as(_u8p), e.size, int(ring_capacity),
                                            int(device), C.byref(h)))
        self._h = h

    def set_stream(self, hip_stream_ptr: int | None):
        _check(lib().qpsk_framer_dev_set_stream(self._h, hip_stream_ptr))

    def set_markers(self, start: bytes, end: bytes):
        s, e = _markers(start, end)
        _check(lib().qpsk_framer_dev_set_markers(self._h, s.ctypes.data_as(_u8p), s.size,
                                                 e.ctypes.data_as(_u8p), e.size))

    def push(self, bits_dev, n_bits_dev, payload_dev, n_payload_dev, offsets_dev=None):
        """Stream-ordered; every argument a torch CUDA tensor (payload_dev is
        [S][payload_stride] uint8, n_payload_dev [S] int64)."""
        _check(lib().qpsk_framer_dev_push(
            self._h, bits_dev.data_ptr(), bits_dev.stride(0) * bits_dev.element_size(),
            offsets_dev.data_ptr() if offsets_dev is not None else None, n_bits_dev.data_ptr(),
            payload_dev.data_ptr(), payload_dev.stride(0), n_payload_dev.data_ptr()))

    def reset_streams(self, streams):
        """The listed rows go back to construction (qpsk_framer_dev_reset_streams):
        not in a frame, empty ring, no carry.  An empty list does nothing."""
        ids, n = _stream_list(streams)
        _check(lib().qpsk_framer_dev_reset_streams(self._h, ids, n))

    def status(self):
        inf = np.zeros(self.S, np.int32)
        cnt = np.zeros(self.S, np.int64)
        car = np.zeros(self.S, np.int64)
        _check(lib().qpsk_framer_dev_status(self._h, inf.ctypes.data, cnt.ctypes.data,
                                            car.ctypes.data))
        return inf, cnt, car

    def __del__(self):
        if getattr(self, "_h", None):
            lib().qpsk_framer_dev_destroy(self._h)
            self._h = None


class QPSKDeModulator:
    """Single-stream mirror of the reference class (QPSKDeModulator.cs:11-457),
    backed by a 1-stream batch on the GPU."""

    def __init__(self, SampleRate, SymbolRate, RrcAlpha=0.9, rrcSpan=6, SymbolSyncBandwith=0.0001,
                 CostasLoopBandwith=120.0, CFOLoopBandwith=None, differentialEncoding=True,
                 tsc=None, enable_fll=False, vector_lanes=8, device=0,
                 max_samples_per_call=1 << 20, ring_capacity=300_000_000):
        p = params(SampleRate, SymbolRate, RrcAlpha, rrcSpan, SymbolSyncBandwith, CostasLoopBandwith,
                   CFOLoopBandwith, differentialEncoding, enable_fll, vector_lanes, device,
                   max_samples_per_call)
        self._b = BatchDemodulator(1, p)
        self._tsc = None if (tsc is None or tsc.strip() == "") else tsc   # :21
        self._framer = None
        self._framer_key = None
        self._ring_capacity = ring_capacity

    def _demod_packed(self, samples):
        x = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
        if x.size & 1:
            raise ValueError("Samples must be interleaved IQ with even length.")   # :347-348
        if x.size == 0:
            return np.zeros((1, 1), np.uint8), 0, 0                               # :350-351
        bits, nb, _, _ = self._b.process(x[None, :])
        n = int(nb[0])
        start = 0
        if self._tsc is not None:                                                 # :413-422
            start = tsc_find(bits[0], n, self._tsc)
            if start < 0:
                return bits, n, -1
        return bits, n, start

    def DeModulate(self, samples) -> str:
        if samples is None:
            raise ValueError("SamplesIQ")                                         # ArgumentNull :341
        bits, n, start = self._demod_packed(samples)
        if start < 0 or n == 0:
            return ""
        return unpack_bits(bits[0], n)[start:]

    def deModulateConstellation(self, samples) -> np.ndarray:
        if samples is None:
            raise ValueError("SamplesIQ")
        x = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
        if x.size & 1:
            raise ValueError("Samples must be interleaved IQ with even length.")   # :430
        _, _, syms, ns = self._b.process(x[None, :], mode=MODE_CONSTELLATION)
        return syms[0, : 2 * int(ns[0])].copy()

    def DeModulateBytes(self, samples, startMarker: bytes, endMarker: bytes) -> bytes:
        if len(startMarker) == 0:
            raise ValueError("startMarker cannot be empty.")                      # :174
        if len(endMarker) == 0:
            raise ValueError("endMarker cannot be empty.")                        # :175
        key = (bytes(startMarker), bytes(endMarker))
        if self._framer is None:
            self._framer = Framer(1, key[0], key[1], self._ring_capacity)
        elif self._framer_key != key:
            self._framer.set_markers(key[0], key[1])   # per-call markers, state kept
        self._framer_key = key
        bits, n, start = self._demod_packed(samples)
        if start < 0 or n - start <= 0:
            return b""
        out = self._framer.push(bits, np.array([n], np.int64), np.array([start], np.int64))
        return out[0]

    def DeModulateTextUtf8(self, samples, startMarker="\u0002", endMarker="\u0003") -> str:
        p = self.DeModulateBytes(samples, startMarker.encode("utf-8"), endMarker.encode("utf-8"))
        return p.decode("utf-8", errors="replace") if p else ""


class QPSKModulator:
    """The reference's QPSKModulator (QPSKModulator.cs:18-167) on the GPU:
    Modulate / ModulateBytes / ModulateTextUtf8 for one stream, and the
    batched form (modulate_batch) that one call runs over many bit strings."""

    def __init__(self, SampleRate, SymbolRate, RrcAlpha=0.9, rrcSpan=6, differentialEncoding=True,
                 tsc=None, device=0):
        p = ModParams()
        lib().qpsk_mod_params_init(C.byref(p), int(SampleRate), int(SymbolRate))
        p.rrc_alpha = float(RrcAlpha)
        p.rrc_span = int(rrcSpan)
        p.differential = 1 if differentialEncoding else 0
        p.device = int(device)
        h = C.c_void_p()
        _check(lib().qpsk_mod_create(C.byref(p), tsc.encode() if tsc else None, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().qpsk_mod_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def output_floats(self, n_bits, pulse_shaping=True) -> int:
        return int(lib().qpsk_mod_output_floats(self._h, int(n_bits), 1 if pulse_shaping else 0))

    def set_stream(self, hip_stream_ptr: int | None):
        """Order the handle's calls on a caller's stream (torch's); None goes
        back to the handle's own."""
        _check(lib().qpsk_mod_set_stream(self._h, C.c_void_p(hip_stream_ptr or 0)))
        self._bound = bool(hip_stream_ptr)

    # ---- host memory -------------------------------------------------------
    def _host_rows(self, call, S, n_max_bits, pulse_shaping, fmt, norm, scale, raw):
        """One host call: call(tag, norm, scale, out, width, n_out, peak) fills S
        rows of fmt wide enough for n_max_bits payload bits.  Returns the rows
        cut to their lengths, or with raw (out [S, width], n_out [S]) as the
        library left them; a PEAK call leaves its peaks in last_peaks."""
        tag, dtype, _ = _format(fmt)
        width = max(self.output_floats(n_max_bits, pulse_shaping), 2)
        out = np.zeros((S, width), dtype=dtype)
        nout = np.zeros(S, dtype=np.int64)
        peak = np.zeros(S, dtype=np.float32) if _norm(norm) == NORM_PEAK else None
        _check(call(tag, _norm(norm), C.c_float(float(np.float32(scale))), out.ctypes.data, width, nout.ctypes.data,
                    peak.ctypes.data if peak is not None else None))
        self.last_peaks = peak
        return (out, nout) if raw else [out[s, : int(nout[s])].copy() for s in range(S)]

    def modulate_batch(self, bit_rows, n_bits, pulse_shaping=True, fmt="cf32", norm="fixed", scale=1.0, raw=False):
        """bit_rows [S, B] uint8 packed MSB-first, n_bits [S] -> list of arrays of
        fmt's element type ("cf32" float32, "cs16" int16, "cs8" int8, "cu8"
        uint8; qpsk_mod_modulate_fmt).  norm "fixed": x * scale, clamped and
        truncated; "peak": each row scaled by its own peak (SaveAsCs16), the
        peaks in last_peaks."""
        rows = np.ascontiguousarray(bit_rows, dtype=np.uint8)
        nb = np.ascontiguousarray(n_bits, dtype=np.int64)
        S = nb.size
        if rows.ndim != 2 or rows.shape[0] != S:
            raise ValueError("bit_rows must be [S, B] with one n_bits per row")
        if S and int(nb.max()) > 8 * rows.shape[1]:
            raise ValueError("a bit count exceeds its row")
        fn = lib().qpsk_mod_modulate_fmt
        return self._host_rows(
            lambda tag, nrm, sc, out, width, nout, peak: fn(
                self._h, tag, nrm, sc, S, rows.ctypes.data if rows.size else None, rows.shape[1], nb.ctypes.data,
                1 if pulse_shaping else 0, MEM_HOST, out, width, nout, peak),
            S, int(nb.max()) if S else 0, pulse_shaping, fmt, norm, scale, raw)

    def modulate_bytes_batch(self, payload_rows, n_payload, startMarker: bytes, endMarker: bytes,
                             pulse_shaping=True, fmt="cf32", norm="fixed", scale=1.0, raw=False):
        """ModulateBytes on every row: payload_rows [S, P] uint8, n_payload [S]
        bytes each -> list of arrays of fmt (qpsk_mod_modulate_bytes_fmt)."""
        st, en = _markers(startMarker, endMarker)
        rows = np.ascontiguousarray(payload_rows, dtype=np.uint8)
        npay = np.ascontiguousarray(n_payload, dtype=np.int64)
        S = npay.size
        if rows.ndim != 2 or rows.shape[0] != S:
            raise ValueError("payload_rows must be [S, P] with one n_payload per row")
        if S and int(npay.max()) > rows.shape[1]:
            raise ValueError("a payload length exceeds its row")
        fn = lib().qpsk_mod_modulate_bytes_fmt
        return self._host_rows(
            lambda tag, nrm, sc, out, width, nout, peak: fn(
                self._h, tag, nrm, sc, S, rows.ctypes.data if rows.size else None, max(rows.shape[1], 1),
                npay.ctypes.data, st.ctypes.data, st.size, en.ctypes.data, en.size, 1 if pulse_shaping else 0, MEM_HOST,
                out, width, nout, peak),
            S, 8 * (len(startMarker) + (int(npay.max()) if S else 0) + len(endMarker)), pulse_shaping, fmt, norm,
            scale, raw)

    def Modulate(self, data: str, pulseShaping=True, fmt="cf32", norm="fixed", scale=1.0) -> np.ndarray:
        if data is None:
            raise ValueError("data")                                   # ArgumentNullException :107
        if any(c not in "01" for c in data):
            raise ValueError("data must be a '0'/'1' string")
        row = pack_bits(data) if data else np.zeros(1, np.uint8)
        return self.modulate_batch(row[None, :], [len(data)], pulseShaping, fmt, norm, scale)[0]

    def ModulateBytes(self, payload: bytes, startMarker: bytes, endMarker: bytes,
                      pulseShaping=True, fmt="cf32", norm="fixed", scale=1.0) -> np.ndarray:
        if len(startMarker) == 0:
            raise ValueError("startMarker cannot be empty.")              # :60
        if len(endMarker) == 0:
            raise ValueError("endMarker cannot be empty.")                # :61
        pay = np.frombuffer(bytes(payload), dtype=np.uint8)
        return self.modulate_bytes_batch(pay.reshape(1, -1), [pay.size], bytes(startMarker), bytes(endMarker),
                                         pulseShaping, fmt, norm, scale)[0]

    def ModulateTextUtf8(self, text: str, startMarker="\u0002", endMarker="\u0003",
                         pulseShaping=True, fmt="cf32", norm="fixed", scale=1.0) -> np.ndarray:
        if text is None:
            raise ValueError("text")                                   # :81
        return self.ModulateBytes(text.encode("utf-8"), startMarker.encode("utf-8"),
                                  endMarker.encode("utf-8"), pulseShaping, fmt, norm, scale)

    # ---- device memory (torch tensors resident in HBM) ----------------------
    def _device_rows(self, call, rows_dev, counts_dev, out_dev, n_out_dev, fmt, norm, peak_dev):
        """One device call: checks what the library cannot see of the tensors
        (device, dtypes, contiguous rows, one count a row) and leaves alignment
        and strides to it.  The call returns when the rows are complete."""
        import torch
        tag = _format(fmt)[0]
        S = counts_dev.numel()
        for t, dt, what in ((rows_dev, torch.uint8, "rows"), (out_dev, _torch_dtype(fmt), "out_dev")):
            if not t.is_cuda or t.dtype != dt or t.dim() != 2 or t.shape[0] != S or (t.shape[1] > 1 and t.stride(1) != 1):
                raise ValueError(f"{what} must be a contiguous-row {dt} [n_streams, k] device tensor")
        for t, what in ((counts_dev, "counts"), (n_out_dev, "n_out_dev")):
            if not t.is_cuda or t.dtype != torch.int64 or t.numel() != S or not t.is_contiguous():
                raise ValueError(f"{what} must be a contiguous int64 [n_streams] device tensor")
        if _norm(norm) == NORM_PEAK and (peak_dev is None or not peak_dev.is_cuda or peak_dev.dtype != torch.float32 or
                                         peak_dev.numel() != S or not peak_dev.is_contiguous()):
            raise ValueError("norm 'peak' needs peak_dev, a contiguous float32 [n_streams] device tensor")
        if not getattr(self, "_bound", False):   # the handle's own stream does not order against torch's
            torch.cuda.current_stream(out_dev.device).synchronize()
        _check(call(tag, rows_dev.data_ptr(), rows_dev.stride(0), counts_dev.data_ptr(), out_dev.data_ptr(),
                    out_dev.stride(0), n_out_dev.data_ptr(), peak_dev.data_ptr() if peak_dev is not None else None))

    def modulate_device(self, bits_dev, n_bits_dev, out_dev, n_out_dev, pulse_shaping=True, fmt="cf32",
                        norm="fixed", scale=1.0, peak_dev=None):
        """modulate_batch on device tensors: bits_dev uint8 [S, B], n_bits_dev
        int64 [S], out_dev [S, >= longest row] of fmt's element type, n_out_dev
        int64 [S] (elements written a row), peak_dev float32 [S] for norm
        "peak".  Rows aligned to 16 bytes with a pitch of a multiple of 16
        bytes are written 16 bytes a store and go into process_device_fmt as
        they are; elements past a row's length are not written."""
        fn = lib().qpsk_mod_modulate_fmt
        sc = C.c_float(float(np.float32(scale)))
        self._device_rows(lambda tag, rows, rstride, cnt, out, ostride, nout, peak: fn(
            self._h, tag, _norm(norm), sc, n_bits_dev.numel(), rows, rstride, cnt, 1 if pulse_shaping else 0,
            MEM_DEVICE, out, ostride, nout, peak), bits_dev, n_bits_dev, out_dev, n_out_dev, fmt, norm, peak_dev)

    def modulate_bytes_device(self, payload_dev, n_payload_dev, startMarker: bytes, endMarker: bytes, out_dev,
                              n_out_dev, pulse_shaping=True, fmt="cf32", norm="fixed", scale=1.0, peak_dev=None):
        """modulate_bytes_batch on device tensors: the payload rows (uint8
        [S, P], n_payload_dev int64 [S]) stay where they are, the markers are
        host bytes."""
        st, en = _markers(startMarker, endMarker)
        fn = lib().qpsk_mod_modulate_bytes_fmt
        sc = C.c_float(float(np.float32(scale)))
        self._device_rows(lambda tag, rows, rstride, cnt, out, ostride, nout, peak: fn(
            self._h, tag, _norm(norm), sc, n_payload_dev.numel(), rows, rstride, cnt, st.ctypes.data, st.size,
            en.ctypes.data, en.size, 1 if pulse_shaping else 0, MEM_DEVICE, out, ostride, nout, peak),
            payload_dev, n_payload_dev, out_dev, n_out_dev, fmt, norm, peak_dev)


# one oscillator of a channel stream's state, and the 128-byte record
_CHANNEL_NCO = [("static_ppm", "f8"), ("drift_ppm", "f8"), ("total_ppm", "f8"), ("cur_hz", "f8"), ("phase", "f8"),
                ("counter", "i8"), ("rng", "u8")]
CHANNEL_STATE_DTYPE = np.dtype([("tx", _CHANNEL_NCO), ("rx", _CHANNEL_NCO), ("pos", "i8"), ("reserved", "i8")])
CHANNEL_TILE_STREAMS = 16     # QPSK_CHANNEL_TILE_STREAMS
CHANNEL_BLOCK_SAMPLES = 64    # QPSK_CHANNEL_BLOCK_SAMPLES
# the default scale of a format's samples, in and out (full scale 1.0)
_CHANNEL_SCALE_IN = {FMT_CF32: 1.0, FMT_CS16: 1.0 / 32768, FMT_CS8: 1.0 / 128, FMT_CU8: 1.0 / 128}
_CHANNEL_SCALE_OUT = {FMT_CF32: 1.0, FMT_CS16: 32767.0, FMT_CS8: 127.0, FMT_CU8: 127.0}


def channel_state_size() -> int:
    """qpsk_channel_state_size(): 128 (needs no device)."""
    return int(lib().qpsk_channel_state_size())


def channel_params(sample_rate, lo_hz=None, tx_ppm=None, rx_ppm=None, tx_phase0=None, rx_phase0=None, tx_seed=None,
                   rx_seed=None, noise_rms=None, noise_seed=None, first_stream=None, device=None) -> ChannelParams:
    """qpsk_channel_params_init's defaults (100 MHz, 1 ppm and 1 ppm, no noise)
    with the given fields replaced."""
    p = ChannelParams()
    lib().qpsk_channel_params_init(C.byref(p), float(sample_rate))
    for name, v in (("lo_hz", lo_hz), ("tx_ppm", tx_ppm), ("rx_ppm", rx_ppm), ("tx_phase0", tx_phase0),
                    ("rx_phase0", rx_phase0), ("noise_rms", noise_rms)):
        if v is not None:
            setattr(p, name, float(v))
    for name, v in (("tx_seed", tx_seed), ("rx_seed", rx_seed), ("noise_seed", noise_seed)):
        if v is not None:
            setattr(p, name, int(v) & (2 ** 64 - 1))
    for name, v in (("first_stream", first_stream), ("device", device)):
        if v is not None:
            setattr(p, name, int(v))
    return p


def channel_state_check(p: ChannelParams, n_streams: int, blob):
    """qpsk_channel_state_check: raises ValueError naming stream, oscillator and
    field when blob is no state of a handle (p, n_streams).  Needs no device."""
    b = bytes(blob)
    _check(lib().qpsk_channel_state_check(C.byref(p), int(n_streams), b, len(b)))


def _scales(tag_in, tag_out, scale_in, scale_out):
    si = _CHANNEL_SCALE_IN[tag_in] if scale_in is None else scale_in
    so = _CHANNEL_SCALE_OUT[tag_out] if scale_out is None else scale_out
    return C.c_float(float(np.float32(si))), C.c_float(float(np.float32(so)))


def _lengths(lengths, S):
    if lengths is None:
        return None, None
    ln = np.ascontiguousarray(lengths, dtype=np.int64)
    if ln.shape != (S,):
        raise ValueError("lengths must hold one count a stream")
    return ln, ln.ctypes.data_as(_i64p)


def _check_host_rows(a, n_rows, dtype, must):
    """What a host-memory call asks of an array: [n_rows, k] of dtype, a row's
    elements side by side.  must: the text up to " with contiguous rows"."""
    if a.dtype != dtype or a.ndim != 2 or a.shape[0] != n_rows or (a.shape[1] > 1 and a.strides[1] != a.itemsize):
        raise ValueError(f"{must} with contiguous rows")


def _check_device_rows(t, n_rows, need, fmt, what, rows_word="n_streams"):
    """What a device-memory call asks of a tensor: [n_rows, >= need] of fmt's
    element type on the device, a row's elements side by side."""
    if (not t.is_cuda or t.dtype != _torch_dtype(fmt) or t.dim() != 2 or t.shape[0] != n_rows or
            (t.shape[1] > 1 and t.stride(1) != 1) or t.shape[1] < need):
        raise ValueError(f"{what} must be a contiguous-row [{rows_word}, >= 2 n] device tensor of its format")


class _RowStage:
    """What Channel, Path, Channeliser, SynthesisBank and Tuner share: the handle's life, its stream,
    its state and the order of a device-memory call.  A subclass names the
    prefix of its qpsk_* functions, creates its handle with _create, and says
    how many bytes its state takes (_state_bytes)."""

    _PREFIX = ""
    _h = None
    _bound = False

    def _fn(self, name):
        return getattr(lib(), f"qpsk_{self._PREFIX}_{name}")

    def _create(self, n_rows):
        h = C.c_void_p()
        _check(self._fn("create")(C.byref(self.p), n_rows, C.byref(h)))
        self._h = h

    def close(self):
        if self._h:
            self._fn("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream_ptr: int | None):
        """Order the handle's calls on a caller's stream (torch's); None goes
        back to the handle's own."""
        _check(self._fn("set_stream")(self._h, C.c_void_p(hip_stream_ptr or 0)))
        self._bound = bool(hip_stream_ptr)

    def sync(self):
        """Wait for the calls queued on the handle (reads its state)."""
        self.get_state()

    def get_state(self) -> bytes:
        buf = C.create_string_buffer(self._state_bytes())
        _check(self._fn("get_state")(self._h, buf, len(buf)))
        return buf.raw

    def set_state(self, blob):
        b = bytes(blob)
        _check(self._fn("set_state")(self._h, b, len(b)))

    def _reset(self, what, rows):
        a, n = _stream_list(rows)
        _check(self._fn("reset_" + what)(self._h, a, n))

    def _device_call(self, out_dev, call):
        """call() on device tensors: the handle's own stream does not order
        against torch's, so unless a stream is bound torch's is drained first
        and the call is waited for."""
        import torch
        if not self._bound:
            torch.cuda.current_stream(out_dev.device).synchronize()
        _check(call())
        if not self._bound:
            self.sync()


class Channel(_RowStage):
    """The reference test bench's channel on S streams (qpsk_channel_*): every
    sample times txNCO.NextSample() * conj(rxNCO.NextSample())
    (testAtDataLevel.cs:39-42), optionally with GenerateIqNoise's samples
    added first (testFullDemodChain.cs:73).  Rows of any format in, rows of
    any format out, host or device memory; the state carries over calls."""

    _PREFIX = "channel"

    def __init__(self, n_streams: int, p: ChannelParams | None = None, **fields):
        self.p = p if p is not None else channel_params(**fields)
        self.n_streams = int(n_streams)
        self._create(self.n_streams)

    def _state_bytes(self):
        return channel_state_size() * self.n_streams

    def apply(self, rows: np.ndarray, fmt="cf32", out_fmt=None, lengths=None, scale_in=None, scale_out=None,
              norm="fixed", out: np.ndarray | None = None, n: int | None = None) -> np.ndarray:
        """One host-memory call on rows [S, 2 n] of fmt; returns rows of out_fmt
        (default fmt), written into out where given (out may be rows itself
        for one format).  Default scales: full scale 1.0 both ways."""
        tag_in, dt_in, _ = _format(fmt)
        tag_out, dt_out, _ = _format(fmt if out_fmt is None else out_fmt)
        _check_host_rows(rows, self.n_streams, dt_in, f"rows must be [n_streams, 2 n] of {np.dtype(dt_in).name}")
        n = rows.shape[1] // 2 if n is None else int(n)
        if out is None:
            out = np.zeros((self.n_streams, max(2 * n, 2)), dtype=dt_out)
        _check_host_rows(out, self.n_streams, dt_out, f"out must be [n_streams, 2 n] of {np.dtype(dt_out).name}")
        keep, lp = _lengths(lengths, self.n_streams)
        si, so = _scales(tag_in, tag_out, scale_in, scale_out)
        _check(lib().qpsk_channel_apply_fmt(self._h, tag_in, rows.ctypes.data, rows.strides[0] // rows.itemsize, si,
                                            tag_out, _norm(norm), out.ctypes.data, out.strides[0] // out.itemsize, so,
                                            n, lp, MEM_HOST))
        return out

    def apply_device(self, in_dev, n: int, out_dev=None, fmt="cf32", out_fmt=None, lengths=None, scale_in=None,
                     scale_out=None, norm="fixed"):
        """One device-memory call: in_dev [S, >= 2 n] of fmt, out_dev likewise
        of out_fmt (default: in place).  lengths is a host array.  Ordered on
        the handle's stream; without set_stream the caller's torch stream is
        drained first and the call is waited for."""
        fo = fmt if out_fmt is None else out_fmt
        tag_in, tag_out = _format(fmt)[0], _format(fo)[0]
        out_dev = in_dev if out_dev is None else out_dev
        _check_device_rows(in_dev, self.n_streams, 2 * n, fmt, "in_dev")
        _check_device_rows(out_dev, self.n_streams, 2 * n, fo, "out_dev")
        keep, lp = _lengths(lengths, self.n_streams)
        si, so = _scales(tag_in, tag_out, scale_in, scale_out)
        self._device_call(out_dev, lambda: lib().qpsk_channel_apply_fmt(
            self._h, tag_in, in_dev.data_ptr(), in_dev.stride(0), si, tag_out, _norm(norm), out_dev.data_ptr(),
            out_dev.stride(0), so, int(n), lp, MEM_DEVICE))
        return out_dev

    def states(self, blob: bytes | None = None) -> np.ndarray:
        """The state as a CHANNEL_STATE_DTYPE array, one record a stream."""
        return np.frombuffer(self.get_state() if blob is None else blob, dtype=CHANNEL_STATE_DTYPE).copy()

    def reset_streams(self, streams):
        self._reset("streams", streams)


# the 256-byte record of a path stream's state
PATH_STATE_DTYPE = np.dtype([("r", "f8"), ("tau", "f8"), ("in_pos", "i8"), ("out_pos", "i8"), ("n_taps", "i4"),
                             ("taps", "f4", (8, 2)), ("hist", "f4", (16, 2)), ("reserved", "u1", (28,))])
assert PATH_STATE_DTYPE.itemsize == 256
PATH_TILE_OUTPUTS = 1024      # QPSK_PATH_TILE_OUTPUTS
PATH_MAX_TAPS = 8             # QPSK_PATH_MAX_TAPS
PATH_HIST = 16                # QPSK_PATH_HIST


def path_state_size() -> int:
    """qpsk_path_state_size(): 256 (needs no device)."""
    return int(lib().qpsk_path_state_size())


def path_params(clock_ppm=None, clock_spread=None, clock_seed=None, tau0=None, tau_random=None, multipath=None,
                first_stream=None, device=None) -> PathParams:
    """qpsk_path_params_init's defaults (no offset, one unit tap) with the given fields replaced."""
    p = PathParams()
    lib().qpsk_path_params_init(C.byref(p))
    for name, v in (("clock_ppm", clock_ppm), ("clock_spread", clock_spread), ("tau0", tau0)):
        if v is not None:
            setattr(p, name, float(v))
    if clock_seed is not None:
        p.clock_seed = int(clock_seed) & (2 ** 64 - 1)
    for name, v in (("tau_random", tau_random), ("multipath", multipath), ("first_stream", first_stream),
                    ("device", device)):
        if v is not None:
            setattr(p, name, int(v))
    return p


def path_count(r: float, tau: float, out_pos: int, in_end: int) -> int:
    """qpsk_path_count: the outputs k >= out_pos with floor(tau + k r) <= in_end - 3 (needs no device)."""
    return int(_check(lib().qpsk_path_count(float(r), float(tau), int(out_pos), int(in_end))))


def path_out_bound(p: PathParams, n_in: int) -> int:
    """qpsk_path_out_bound: an output capacity that suffices for any call of n_in samples (needs no device)."""
    return int(_check(lib().qpsk_path_out_bound(C.byref(p), int(n_in))))


def path_state_init(p: PathParams, n_streams: int) -> bytes:
    """qpsk_path_state_init: the state qpsk_path_create leaves (needs no device)."""
    buf = C.create_string_buffer(path_state_size() * int(n_streams))
    _check(lib().qpsk_path_state_init(C.byref(p), int(n_streams), buf, len(buf)))
    return buf.raw


def path_state_check(n_streams: int, blob):
    """qpsk_path_state_check: raises ValueError naming stream and field when
    blob is no state of a path of n_streams.  Needs no device."""
    b = bytes(blob)
    _check(lib().qpsk_path_state_check(int(n_streams), b, len(b)))


def path_apply_host(state, rows: np.ndarray, lengths=None, out: np.ndarray | None = None, out_cap: int | None = None,
                    n: int | None = None):
    """qpsk_path_apply_host: one call on host float32 rows [S, 2 n] and a state
    blob, no device.  Returns (the new state, out rows, n_out); a refused call
    raises and leaves out as it was."""
    st = C.create_string_buffer(bytes(state), len(bytes(state)))
    S = len(st) // path_state_size()
    _check_host_rows(rows, S, np.float32, "rows must be [n_streams, 2 n] float32")
    n = rows.shape[1] // 2 if n is None else int(n)
    if out is None:
        cap = n + n // 512 + 4 if out_cap is None else int(out_cap)
        out = np.zeros((S, max(2 * cap, 2)), np.float32)
    cap = out.shape[1] // 2 if out_cap is None else int(out_cap)
    keep, lp = _lengths(lengths, S)
    n_out = np.zeros(S, np.int64)
    _check(lib().qpsk_path_apply_host(st, len(st), S, rows.ctypes.data, rows.strides[0] // 4, out.ctypes.data,
                                      out.strides[0] // 4, cap, n, lp, n_out.ctypes.data_as(_i64p)))
    return st.raw, out, n_out


class Path(_RowStage):
    """The propagation path on S streams (qpsk_path_*): each stream's multipath
    taps, then a resampler onto the receiver's sample clock
    (MuellerMuller.CubicLagrange4 at p_k = tau + k r).  Rows of any format in,
    rows of any format out, host or device memory; a call emits what its
    inputs make computable and returns the counts."""

    _PREFIX = "path"

    def __init__(self, n_streams: int, p: PathParams | None = None, **fields):
        self.p = p if p is not None else path_params(**fields)
        self.n_streams = int(n_streams)
        self._create(self.n_streams)

    def _state_bytes(self):
        return path_state_size() * self.n_streams

    def set_taps(self, taps, per_stream=False):
        """Complex taps [L] for all streams, or [S, L] with per_stream."""
        t = np.ascontiguousarray(np.asarray(taps, dtype=np.complex64))
        if t.ndim != (2 if per_stream else 1) or (per_stream and t.shape[0] != self.n_streams):
            raise ValueError("taps must be [L], or [n_streams, L] with per_stream")
        f = t.view(np.float32)
        _check(lib().qpsk_path_set_taps(self._h, f.ctypes.data, t.shape[-1], 1 if per_stream else 0))

    def out_bound(self, n_in: int) -> int:
        return path_out_bound(self.p, n_in)

    def apply(self, rows: np.ndarray, fmt="cf32", out_fmt=None, lengths=None, scale_in=None, scale_out=None,
              norm="fixed", out: np.ndarray | None = None, n: int | None = None, out_cap: int | None = None):
        """One host-memory call on rows [S, 2 n] of fmt; returns (rows of
        out_fmt (default fmt), n_out).  out: rows to write into, [S, >= 2
        out_cap]; what lies past a row's n_out stays as it was."""
        tag_in, dt_in, _ = _format(fmt)
        tag_out, dt_out, _ = _format(fmt if out_fmt is None else out_fmt)
        _check_host_rows(rows, self.n_streams, dt_in, f"rows must be [n_streams, 2 n] of {np.dtype(dt_in).name}")
        n = rows.shape[1] // 2 if n is None else int(n)
        if out is None:
            out = np.zeros((self.n_streams, max(2 * (self.out_bound(n) if out_cap is None else int(out_cap)), 2)),
                           dtype=dt_out)
        _check_host_rows(out, self.n_streams, dt_out, f"out must be [n_streams, 2 out_cap] of {np.dtype(dt_out).name}")
        cap = out.shape[1] // 2 if out_cap is None else int(out_cap)
        keep, lp = _lengths(lengths, self.n_streams)
        si, so = _scales(tag_in, tag_out, scale_in, scale_out)
        n_out = np.zeros(self.n_streams, np.int64)
        _check(lib().qpsk_path_apply_fmt(self._h, tag_in, rows.ctypes.data, rows.strides[0] // rows.itemsize, si,
                                         tag_out, _norm(norm), out.ctypes.data, out.strides[0] // out.itemsize, cap, so,
                                         n, lp, n_out.ctypes.data_as(_i64p), MEM_HOST))
        return out, n_out

    def apply_device(self, in_dev, n: int, out_dev, fmt="cf32", out_fmt=None, lengths=None, scale_in=None,
                     scale_out=None, norm="fixed", out_cap: int | None = None) -> np.ndarray:
        """One device-memory call: in_dev [S, >= 2 n] of fmt, out_dev [S, >= 2
        out_cap] of out_fmt (out_cap defaults to what out_dev holds).  Returns
        n_out, a host array, at once.  lengths is a host array.  Ordered on the
        handle's stream; without set_stream the caller's torch stream is
        drained first and the call is waited for."""
        fo = fmt if out_fmt is None else out_fmt
        tag_in, tag_out = _format(fmt)[0], _format(fo)[0]
        cap = out_dev.shape[1] // 2 if out_cap is None else int(out_cap)
        _check_device_rows(in_dev, self.n_streams, 2 * n, fmt, "in_dev")
        _check_device_rows(out_dev, self.n_streams, 2 * cap, fo, "out_dev")
        keep, lp = _lengths(lengths, self.n_streams)
        si, so = _scales(tag_in, tag_out, scale_in, scale_out)
        n_out = np.zeros(self.n_streams, np.int64)
        self._device_call(out_dev, lambda: lib().qpsk_path_apply_fmt(
            self._h, tag_in, in_dev.data_ptr(), in_dev.stride(0), si, tag_out, _norm(norm), out_dev.data_ptr(),
            out_dev.stride(0), cap, so, int(n), lp, n_out.ctypes.data_as(_i64p), MEM_DEVICE))
        return n_out

    def states(self, blob: bytes | None = None) -> np.ndarray:
        """The state as a PATH_STATE_DTYPE array, one record a stream."""
        return np.frombuffer(self.get_state() if blob is None else blob, dtype=PATH_STATE_DTYPE).copy()

    def reset_streams(self, streams):
        self._reset("streams", streams)


PFB_STATE_HEAD = 64           # QPSK_PFB_STATE_HEAD
PFB_MIN_CHANNELS, PFB_MAX_CHANNELS, PFB_MAX_BRANCH_TAPS, PFB_MAX_TAPS = 8, 4096, 16, 32768


def pfb_state_dtype(channels: int, taps_per_branch: int) -> np.dtype:
    """One band's state record: the 64-byte head, then hist[L][2]."""
    dt = np.dtype([("in_pos", "i8"), ("out_pos", "i8"), ("reserved", "u1", (48,)),
                   ("hist", "f4", (int(channels) * int(taps_per_branch), 2))])
    assert dt.itemsize == PFB_STATE_HEAD + 8 * int(channels) * int(taps_per_branch)
    return dt


def pfb_params(channels=None, taps_per_branch=None, gain=None, device=None) -> PfbParams:
    """qpsk_pfb_params_init's defaults (64 channels, 8 taps a branch, gain 1) with the given fields replaced."""
    p = PfbParams()
    lib().qpsk_pfb_params_init(C.byref(p))
    for name, v in (("channels", channels), ("taps_per_branch", taps_per_branch), ("device", device)):
        if v is not None:
            setattr(p, name, int(v))
    if gain is not None:
        p.gain = float(gain)
    return p


def pfb_design(p: PfbParams) -> np.ndarray:
    """qpsk_pfb_design: the prototype of p, float32 [M K] (needs no device)."""
    h = np.zeros(max(int(p.channels) * int(p.taps_per_branch), 1), np.float32)
    _check(lib().qpsk_pfb_design(C.byref(p), h.ctypes.data, int(p.channels) * int(p.taps_per_branch)))
    return h


def pfb_twiddles(channels: int) -> np.ndarray:
    """qpsk_pfb_twiddles: W of M channels, float32 [M / 2, 2] (needs no device)."""
    w = np.zeros((max(int(channels) // 2, 1), 2), np.float32)
    _check(lib().qpsk_pfb_twiddles(int(channels), w.ctypes.data, int(channels)))
    return w


def pfb_count(channels: int, out_pos: int, in_end: int) -> int:
    """qpsk_pfb_count: max(0, ceil(in_end / D) - out_pos) (needs no device)."""
    return int(_check(lib().qpsk_pfb_count(int(channels), int(out_pos), int(in_end))))


def pfb_out_bound(channels: int, n_in: int) -> int:
    """qpsk_pfb_out_bound: n_in / D + 1 (needs no device)."""
    return int(_check(lib().qpsk_pfb_out_bound(int(channels), int(n_in))))


def pfb_tile_frames(channels: int) -> int:
    """qpsk_pfb_tile_frames: the frames one workgroup of the kernel covers (needs no device)."""
    return int(_check(lib().qpsk_pfb_tile_frames(int(channels))))


def pfb_state_size(p: PfbParams) -> int:
    """qpsk_pfb_state_size: the bytes of one band's state, 64 + 8 M K (needs no device)."""
    return int(_check(lib().qpsk_pfb_state_size(C.byref(p))))


def pfb_state_init(p: PfbParams, n_bands: int) -> bytes:
    """qpsk_pfb_state_init: the state qpsk_pfb_create leaves (needs no device)."""
    buf = C.create_string_buffer(pfb_state_size(p) * int(n_bands))
    _check(lib().qpsk_pfb_state_init(C.byref(p), int(n_bands), buf, len(buf)))
    return buf.raw


def pfb_state_check(p: PfbParams, n_bands: int, blob):
    """qpsk_pfb_state_check: raises ValueError naming band and field when blob
    is no state of a channeliser of n_bands.  Needs no device."""
    b = bytes(blob)
    _check(lib().qpsk_pfb_state_check(C.byref(p), int(n_bands), b, len(b)))


def pfb_apply_host(p: PfbParams, state, rows: np.ndarray, lengths=None, out: np.ndarray | None = None,
                   out_cap: int | None = None, n: int | None = None, taps=None):
    """qpsk_pfb_apply_host: one call on host float32 rows [n_bands, 2 n] and a
    state blob, no device.  Returns (the new state, out rows [n_bands M, 2
    out_cap], n_out); a refused call raises and leaves out as it was."""
    st = C.create_string_buffer(bytes(state), len(bytes(state)))
    B = len(st) // max(pfb_state_size(p), 1)
    _check_host_rows(rows, B, np.float32, "rows must be [n_bands, 2 n] float32")
    n = rows.shape[1] // 2 if n is None else int(n)
    if out is None:
        cap = pfb_out_bound(p.channels, n) if out_cap is None else int(out_cap)
        out = np.zeros((B * p.channels, max(2 * cap, 2)), np.float32)
    cap = out.shape[1] // 2 if out_cap is None else int(out_cap)
    keep, lp = _lengths(lengths, B)
    t = None if taps is None else np.ascontiguousarray(taps, dtype=np.float32)
    n_out = np.zeros(B, np.int64)
    _check(lib().qpsk_pfb_apply_host(C.byref(p), None if t is None else t.ctypes.data, st, len(st), B, rows.ctypes.data,
                                     rows.strides[0] // 4, out.ctypes.data, out.strides[0] // 4, cap, n, lp,
                                     n_out.ctypes.data_as(_i64p)))
    return st.raw, out, n_out


class Channeliser(_RowStage):
    """The polyphase channeliser on n_bands wideband rows (qpsk_pfb_*): band b's
    M = channels output rows b M .. b M + M - 1 are the signals around c fs / M
    at rate 2 fs / M, CF32, ready for BatchDemodulator.  Rows of any format in,
    host or device memory; a call emits the frames its inputs make computable
    and returns the counts."""

    _PREFIX = "pfb"

    def __init__(self, n_bands: int, p: PfbParams | None = None, **fields):
        self.p = p if p is not None else pfb_params(**fields)
        self.n_bands = int(n_bands)
        self.channels = int(self.p.channels)
        self.n_rows = self.n_bands * self.channels
        self._create(self.n_bands)

    def _state_bytes(self):
        return pfb_state_size(self.p) * self.n_bands

    def set_taps(self, taps):
        """Replace the prototype: M K real taps."""
        t = np.ascontiguousarray(np.asarray(taps, dtype=np.float32).reshape(-1))
        _check(lib().qpsk_pfb_set_taps(self._h, t.ctypes.data if t.size else None, t.size))

    def out_bound(self, n_in: int) -> int:
        return pfb_out_bound(self.channels, n_in)

    def lengths_for_demod(self, n_out) -> np.ndarray:
        """A band's count repeated over its M rows: the lengths of the
        demodulator call that takes the output rows."""
        n_out = np.asarray(n_out, np.int64).reshape(-1)
        if n_out.size != self.n_bands:
            raise ValueError("n_out must hold one count a band")
        return np.repeat(n_out, self.channels)

    def apply(self, rows: np.ndarray, fmt="cf32", lengths=None, scale_in=None, out: np.ndarray | None = None,
              n: int | None = None, out_cap: int | None = None):
        """One host-memory call on rows [n_bands, 2 n] of fmt; returns (float32
        rows [n_bands M, 2 out_cap], n_out).  out: rows to write into; what
        lies past a row's n_out stays as it was."""
        tag_in, dt_in, _ = _format(fmt)
        _check_host_rows(rows, self.n_bands, dt_in, f"rows must be [n_bands, 2 n] of {np.dtype(dt_in).name}")
        n = rows.shape[1] // 2 if n is None else int(n)
        if out is None:
            out = np.zeros((self.n_rows, max(2 * (self.out_bound(n) if out_cap is None else int(out_cap)), 2)), np.float32)
        _check_host_rows(out, self.n_rows, np.float32, "out must be [n_bands M, 2 out_cap] float32")
        cap = out.shape[1] // 2 if out_cap is None else int(out_cap)
        keep, lp = _lengths(lengths, self.n_bands)
        si, _ = _scales(tag_in, FMT_CF32, scale_in, None)
        n_out = np.zeros(self.n_bands, np.int64)
        _check(lib().qpsk_pfb_apply_fmt(self._h, tag_in, rows.ctypes.data, rows.strides[0] // rows.itemsize, si,
                                        out.ctypes.data, out.strides[0] // 4, cap, n, lp, n_out.ctypes.data_as(_i64p),
                                        MEM_HOST))
        return out, n_out

    def apply_device(self, in_dev, n: int, out_dev, fmt="cf32", lengths=None, scale_in=None,
                     out_cap: int | None = None) -> np.ndarray:
        """One device-memory call: in_dev [n_bands, >= 2 n] of fmt, out_dev
        [n_bands M, >= 2 out_cap] float32 (out_cap defaults to what out_dev
        holds).  Returns n_out, a host array, at once.  lengths is a host
        array.  Ordered on the handle's stream; without set_stream the
        caller's torch stream is drained first and the call is waited for."""
        tag_in = _format(fmt)[0]
        cap = out_dev.shape[1] // 2 if out_cap is None else int(out_cap)
        _check_device_rows(in_dev, self.n_bands, 2 * n, fmt, "in_dev", "rows")
        _check_device_rows(out_dev, self.n_rows, 2 * cap, "cf32", "out_dev", "rows")
        keep, lp = _lengths(lengths, self.n_bands)
        si, _ = _scales(tag_in, FMT_CF32, scale_in, None)
        n_out = np.zeros(self.n_bands, np.int64)
        self._device_call(out_dev, lambda: lib().qpsk_pfb_apply_fmt(
            self._h, tag_in, in_dev.data_ptr(), in_dev.stride(0), si, out_dev.data_ptr(), out_dev.stride(0), cap, int(n),
            lp, n_out.ctypes.data_as(_i64p), MEM_DEVICE))
        return n_out

    def states(self, blob: bytes | None = None) -> np.ndarray:
        """The state as a pfb_state_dtype array, one record a band."""
        dt = pfb_state_dtype(self.channels, self.p.taps_per_branch)
        return np.frombuffer(self.get_state() if blob is None else blob, dtype=dt).copy()

    def reset_bands(self, bands):
        self._reset("bands", bands)


SFB_STATE_HEAD = 64           # QPSK_SFB_STATE_HEAD
SFB_TILE_TRANSFORM, SFB_TILE_SUM, SFB_TILE_SLAB = 0, 1, 2      # QPSK_SFB_TILE_*


def sfb_state_dtype(channels: int, taps_per_branch: int) -> np.dtype:
    """One band's state record: the 64-byte head, then hist[2K - 1][M][2]."""
    dt = np.dtype([("in_pos", "i8"), ("out_pos", "i8"), ("reserved", "u1", (48,)),
                   ("hist", "f4", (2 * int(taps_per_branch) - 1, int(channels), 2))])
    assert dt.itemsize == SFB_STATE_HEAD + 8 * int(channels) * (2 * int(taps_per_branch) - 1)
    return dt


def sfb_params(channels=None, taps_per_branch=None, device=None) -> SfbParams:
    """qpsk_sfb_params_init's defaults (64 channels, 8 taps a branch) with the given fields replaced."""
    p = SfbParams()
    lib().qpsk_sfb_params_init(C.byref(p))
    for name, v in (("channels", channels), ("taps_per_branch", taps_per_branch), ("device", device)):
        if v is not None:
            setattr(p, name, int(v))
    return p


def sfb_tile_frames(channels: int, taps_per_branch: int, which: int) -> int:
    """qpsk_sfb_tile_frames: the per-call frame counts at which the kernel
    SFB_TILE_* names takes another workgroup, or the call another pass (needs no device)."""
    return int(_check(lib().qpsk_sfb_tile_frames(int(channels), int(taps_per_branch), int(which))))


def sfb_state_size(p: SfbParams) -> int:
    """qpsk_sfb_state_size: the bytes of one band's state, 64 + 8 M (2K - 1) (needs no device)."""
    return int(_check(lib().qpsk_sfb_state_size(C.byref(p))))


def sfb_state_init(p: SfbParams, n_bands: int) -> bytes:
    """qpsk_sfb_state_init: the state qpsk_sfb_create leaves (needs no device)."""
    buf = C.create_string_buffer(sfb_state_size(p) * int(n_bands))
    _check(lib().qpsk_sfb_state_init(C.byref(p), int(n_bands), buf, len(buf)))
    return buf.raw


def sfb_state_check(p: SfbParams, n_bands: int, blob):
    """qpsk_sfb_state_check: raises ValueError naming band and field when blob
    is no state of a synthesis bank of n_bands.  Needs no device."""
    b = bytes(blob)
    _check(lib().qpsk_sfb_state_check(C.byref(p), int(n_bands), b, len(b)))


def sfb_apply_host(p: SfbParams, state, rows: np.ndarray, lengths=None, out: np.ndarray | None = None,
                   n: int | None = None, taps=None, scale_out=1.0):
    """qpsk_sfb_apply_host: one call on host float32 rows [n_bands M, 2 n] and a
    state blob, no device.  Returns (the new state, out rows [n_bands, 2 n D]);
    a refused call raises and leaves out as it was."""
    st = C.create_string_buffer(bytes(state), len(bytes(state)))
    B = len(st) // max(sfb_state_size(p), 1)
    D = int(p.channels) // 2
    _check_host_rows(rows, B * int(p.channels), np.float32, "rows must be [n_bands M, 2 n] float32")
    n = rows.shape[1] // 2 if n is None else int(n)
    if out is None:
        out = np.zeros((B, max(2 * n * D, 2)), np.float32)
    _check_host_rows(out, B, np.float32, "out must be [n_bands, 2 n D] float32")
    keep, lp = _lengths(lengths, B)
    t = None if taps is None else np.ascontiguousarray(taps, dtype=np.float32)
    _check(lib().qpsk_sfb_apply_host(C.byref(p), None if t is None else t.ctypes.data, st, len(st), B, rows.ctypes.data,
                                     rows.strides[0] // 4, out.ctypes.data, out.strides[0] // 4,
                                     C.c_float(float(np.float32(scale_out))), n, lp))
    return st.raw, out


class SynthesisBank(_RowStage):
    """The polyphase synthesis bank on n_bands bands (qpsk_sfb_*), the
    channeliser's dual: band b's M = channels input rows b M .. b M + M - 1 at
    rate 2 fs / M become the carriers around c fs / M of its wideband row b at
    rate fs.  Rows of any format in and out, host or device memory; a call of
    n frames emits n M / 2 samples a band."""

    _PREFIX = "sfb"

    def __init__(self, n_bands: int, p: SfbParams | None = None, **fields):
        self.p = p if p is not None else sfb_params(**fields)
        self.n_bands = int(n_bands)
        self.channels = int(self.p.channels)
        self.n_rows = self.n_bands * self.channels
        self._create(self.n_bands)

    def _state_bytes(self):
        return sfb_state_size(self.p) * self.n_bands

    def set_taps(self, taps):
        """Replace the prototype: M K real taps."""
        t = np.ascontiguousarray(np.asarray(taps, dtype=np.float32).reshape(-1))
        _check(lib().qpsk_sfb_set_taps(self._h, t.ctypes.data if t.size else None, t.size))

    def out_len(self, n_frames: int) -> int:
        """The samples a band emits for n_frames frames: n_frames M / 2."""
        return int(n_frames) * (self.channels // 2)

    def apply_host(self, rows: np.ndarray, fmt="cf32", out_fmt="cf32", lengths=None, scale_in=None, scale_out=None,
                   norm="fixed", out: np.ndarray | None = None, n: int | None = None) -> np.ndarray:
        """One host-memory call on rows [n_bands M, 2 n] of fmt; returns rows
        [n_bands, 2 n D] of out_fmt.  out: rows to write into; what lies past
        a band's samples stays as it was."""
        tag_in, dt_in, _ = _format(fmt)
        tag_out, dt_out, _ = _format(out_fmt)
        _check_host_rows(rows, self.n_rows, dt_in, f"rows must be [n_bands M, 2 n] of {np.dtype(dt_in).name}")
        n = rows.shape[1] // 2 if n is None else int(n)
        if out is None:
            out = np.zeros((self.n_bands, max(2 * self.out_len(n), 2)), dtype=dt_out)
        _check_host_rows(out, self.n_bands, dt_out, f"out must be [n_bands, 2 n D] of {np.dtype(dt_out).name}")
        keep, lp = _lengths(lengths, self.n_bands)
        si, so = _scales(tag_in, tag_out, scale_in, scale_out)
        _check(lib().qpsk_sfb_apply_fmt(self._h, tag_in, rows.ctypes.data, rows.strides[0] // rows.itemsize, si, tag_out,
                                        _norm(norm), out.ctypes.data, out.strides[0] // out.itemsize, so, n, lp, MEM_HOST))
        return out

    def apply_device(self, in_dev, n: int, out_dev, fmt="cf32", out_fmt="cf32", lengths=None, scale_in=None,
                     scale_out=None, norm="fixed"):
        """One device-memory call: in_dev [n_bands M, >= 2 n] of fmt, out_dev
        [n_bands, >= 2 n D] of out_fmt.  lengths is a host array.  Ordered on
        the handle's stream; without set_stream the caller's torch stream is
        drained first and the call is waited for."""
        tag_in, tag_out = _format(fmt)[0], _format(out_fmt)[0]
        _check_device_rows(in_dev, self.n_rows, 2 * n, fmt, "in_dev", "rows")
        _check_device_rows(out_dev, self.n_bands, 2 * self.out_len(n), out_fmt, "out_dev", "n_bands")
        keep, lp = _lengths(lengths, self.n_bands)
        si, so = _scales(tag_in, tag_out, scale_in, scale_out)
        self._device_call(out_dev, lambda: lib().qpsk_sfb_apply_fmt(
            self._h, tag_in, in_dev.data_ptr(), in_dev.stride(0), si, tag_out, _norm(norm), out_dev.data_ptr(),
            out_dev.stride(0), so, int(n), lp, MEM_DEVICE))
        return out_dev

    def states(self, blob: bytes | None = None) -> np.ndarray:
        """The state as an sfb_state_dtype array, one record a band."""
        dt = sfb_state_dtype(self.channels, self.p.taps_per_branch)
        return np.frombuffer(self.get_state() if blob is None else blob, dtype=dt).copy()

    def reset_bands(self, bands):
        self._reset("bands", bands)


# the 320-byte record of a tuner stream's state
TUNER_STATE_DTYPE = np.dtype([("r", "f8"), ("tau", "f8"), ("fw", "i8"), ("ph0", "u8"), ("in_pos", "i8"),
                              ("out_pos", "i8"), ("reserved", "u1", (16,)), ("hist", "f4", (32, 2))])
assert TUNER_STATE_DTYPE.itemsize == 320
TUNER_TILE_OUTPUTS = 1024     # QPSK_TUNER_TILE_OUTPUTS
TUNER_PHASES = 64             # QPSK_TUNER_PHASES
TUNER_HIST = 32               # QPSK_TUNER_HIST


def _f64_row(v, n, name):
    """An optional per-stream double array as the C ABI takes it: (keep-alive, pointer)."""
    if v is None:
        return None, None
    a = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
    if a.size != n:
        raise ValueError(f"{name} must hold one value a stream")
    return a, a.ctypes.data


def tuner_state_size() -> int:
    """qpsk_tuner_state_size(): 320 (needs no device)."""
    return int(lib().qpsk_tuner_state_size())


def tuner_params(freq=None, rate=None, tau0=None, cutoff=None, taps_per_phase=None, first_stream=None,
                 device=None) -> TunerParams:
    """qpsk_tuner_params_init's defaults (no shift, rate 1, 16 taps a phase) with the given fields replaced."""
    p = TunerParams()
    lib().qpsk_tuner_params_init(C.byref(p))
    for name, v in (("freq", freq), ("rate", rate), ("tau0", tau0), ("cutoff", cutoff)):
        if v is not None:
            setattr(p, name, float(v))
    for name, v in (("taps_per_phase", taps_per_phase), ("first_stream", first_stream), ("device", device)):
        if v is not None:
            setattr(p, name, int(v))
    return p


def tuner_cutoff(p: TunerParams) -> float:
    """The cutoff a handle of p designs for: cutoff, or 0.4 * min(1, 1 / rate) where it is 0."""
    return float(p.cutoff) if p.cutoff != 0.0 else 0.4 * (1.0 / p.rate if p.rate > 1.0 else 1.0)


def tuner_design(taps_per_phase: int, cutoff: float) -> np.ndarray:
    """qpsk_tuner_design: the prototype, float32 [64 T + 1] (needs no device)."""
    n = TUNER_PHASES * int(taps_per_phase) + 1
    h = np.zeros(max(n, 1), np.float32)
    _check(lib().qpsk_tuner_design(int(taps_per_phase), float(cutoff), h.ctypes.data, n))
    return h


def tuner_tables():
    """qpsk_tuner_tables: the oscillator's coarse and fine tables, float32 [1024, 2] each (needs no device)."""
    c, f = np.zeros((1024, 2), np.float32), np.zeros((1024, 2), np.float32)
    _check(lib().qpsk_tuner_tables(c.ctypes.data, f.ctypes.data))
    return c, f


def tuner_osc(ph) -> np.ndarray:
    """qpsk_tuner_osc: w of each uint64 phase, float32 [n, 2] (needs no device)."""
    a = np.ascontiguousarray(ph, dtype=np.uint64).reshape(-1)
    w = np.zeros((max(a.size, 1), 2), np.float32)
    _check(lib().qpsk_tuner_osc(a.ctypes.data, a.size, w.ctypes.data))
    return w[: a.size]


def tuner_count(r: float, tau: float, taps_per_phase: int, out_pos: int, in_end: int) -> int:
    """qpsk_tuner_count: the outputs k >= out_pos with floor(tau + k r) <= in_end - 1 - T/2 (needs no device)."""
    return int(_check(lib().qpsk_tuner_count(float(r), float(tau), int(taps_per_phase), int(out_pos), int(in_end))))


def tuner_out_bound(p: TunerParams, n_in: int, rates=None) -> int:
    """qpsk_tuner_out_bound: an output capacity that suffices for any call of n_in samples (needs no device)."""
    n = 1 if rates is None else np.asarray(rates).size
    keep, rp = _f64_row(rates, n, "rates")
    return int(_check(lib().qpsk_tuner_out_bound(C.byref(p), rp, n, int(n_in))))


def tuner_state_init(p: TunerParams, n_streams: int, freq=None, rate=None) -> bytes:
    """qpsk_tuner_state_init: the state qpsk_tuner_create leaves (needs no device)."""
    buf = C.create_string_buffer(tuner_state_size() * int(n_streams))
    kf, fp = _f64_row(freq, int(n_streams), "freq")
    kr, rp = _f64_row(rate, int(n_streams), "rate")
    _check(lib().qpsk_tuner_state_init(C.byref(p), int(n_streams), fp, rp, buf, len(buf)))
    return buf.raw


def tuner_state_check(p: TunerParams, n_streams: int, blob):
    """qpsk_tuner_state_check: raises ValueError naming stream and field when
    blob is no state of a tuner of n_streams.  Needs no device."""
    b = bytes(blob)
    _check(lib().qpsk_tuner_state_check(C.byref(p), int(n_streams), b, len(b)))


def tuner_apply_host(p: TunerParams, state, rows: np.ndarray, lengths=None, out: np.ndarray | None = None,
                     out_cap: int | None = None, n: int | None = None, taps=None):
    """qpsk_tuner_apply_host: one call on host float32 rows [S, 2 n] and a state
    blob, no device.  Returns (the new state, out rows, n_out); a refused call
    raises and leaves out as it was."""
    st = C.create_string_buffer(bytes(state), len(bytes(state)))
    S = len(st) // tuner_state_size()
    _check_host_rows(rows, S, np.float32, "rows must be [n_streams, 2 n] float32")
    n = rows.shape[1] // 2 if n is None else int(n)
    if out is None:
        cap = 4 * n + 4 if out_cap is None else int(out_cap)
        out = np.zeros((S, max(2 * cap, 2)), np.float32)
    cap = out.shape[1] // 2 if out_cap is None else int(out_cap)
    keep, lp = _lengths(lengths, S)
    t = None if taps is None else np.ascontiguousarray(taps, dtype=np.float32)
    if t is not None and t.size != TUNER_PHASES * int(p.taps_per_phase) + 1:
        raise ValueError("taps must hold 64 T + 1 floats")
    n_out = np.zeros(S, np.int64)
    _check(lib().qpsk_tuner_apply_host(C.byref(p), None if t is None else t.ctypes.data, st, len(st), S,
                                       rows.ctypes.data, rows.strides[0] // 4, out.ctypes.data, out.strides[0] // 4, cap,
                                       n, lp, n_out.ctypes.data_as(_i64p)))
    return st.raw, out, n_out


class Tuner(_RowStage):
    """The tuner on S streams (qpsk_tuner_*): each stream's oscillator brings a
    carrier at +freq to DC, then a 64-phase polyphase lowpass resamples by r
    input samples an output.  Rows of any format in, rows of any format out,
    host or device memory; a call emits what its inputs make computable and
    returns the counts."""

    _PREFIX = "tuner"

    def __init__(self, n_streams: int, p: TunerParams | None = None, freq=None, rate=None, **fields):
        """freq, rate: one value for every stream (the params' field) or one a stream."""
        if freq is not None and np.ndim(freq) == 0:
            fields["freq"], freq = freq, None
        if rate is not None and np.ndim(rate) == 0:
            fields["rate"], rate = rate, None
        self.p = p if p is not None else tuner_params(**fields)
        self.n_streams = int(n_streams)
        kf, fp = _f64_row(freq, self.n_streams, "freq")
        kr, rp = _f64_row(rate, self.n_streams, "rate")
        self.rates = kr.copy() if kr is not None else np.full(self.n_streams, float(self.p.rate))
        h = C.c_void_p()
        _check(lib().qpsk_tuner_create(C.byref(self.p), self.n_streams, fp, rp, C.byref(h)))
        self._h = h

    def _state_bytes(self):
        return tuner_state_size() * self.n_streams

    def set_taps(self, taps):
        """Replace the prototype: 64 T + 1 real points."""
        t = np.ascontiguousarray(np.asarray(taps, dtype=np.float32).reshape(-1))
        _check(lib().qpsk_tuner_set_taps(self._h, t.ctypes.data if t.size else None, t.size))

    def set_freq(self, streams, freqs):
        """Retune the listed streams behind the calls queued so far; the phase stays continuous."""
        a, n = _stream_list(streams)
        keep, fp = _f64_row(freqs, n, "freqs")
        _check(lib().qpsk_tuner_set_freq(self._h, a, n, fp))

    def out_bound(self, n_in: int) -> int:
        return tuner_out_bound(self.p, n_in, self.rates)

    def lengths_for_demod(self, n_out) -> np.ndarray:
        """The counts of a call as the lengths of the demodulator call that takes the output rows."""
        n_out = np.asarray(n_out, np.int64).reshape(-1)
        if n_out.size != self.n_streams:
            raise ValueError("n_out must hold one count a stream")
        return n_out.copy()

    def apply_host(self, rows: np.ndarray, fmt="cf32", out_fmt=None, lengths=None, scale_in=None, scale_out=None,
                   norm="fixed", out: np.ndarray | None = None, n: int | None = None, out_cap: int | None = None):
        """One host-memory call on rows [S, 2 n] of fmt; returns (rows of
        out_fmt (default fmt), n_out).  out: rows to write into, [S, >= 2
        out_cap]; what lies past a row's n_out stays as it was."""
        tag_in, dt_in, _ = _format(fmt)
        tag_out, dt_out, _ = _format(fmt if out_fmt is None else out_fmt)
        _check_host_rows(rows, self.n_streams, dt_in, f"rows must be [n_streams, 2 n] of {np.dtype(dt_in).name}")
        n = rows.shape[1] // 2 if n is None else int(n)
        if out is None:
            out = np.zeros((self.n_streams, max(2 * (self.out_bound(n) if out_cap is None else int(out_cap)), 2)),
                           dtype=dt_out)
        _check_host_rows(out, self.n_streams, dt_out, f"out must be [n_streams, 2 out_cap] of {np.dtype(dt_out).name}")
        cap = out.shape[1] // 2 if out_cap is None else int(out_cap)
        keep, lp = _lengths(lengths, self.n_streams)
        si, so = _scales(tag_in, tag_out, scale_in, scale_out)
        n_out = np.zeros(self.n_streams, np.int64)
        _check(lib().qpsk_tuner_apply_fmt(self._h, tag_in, rows.ctypes.data, rows.strides[0] // rows.itemsize, si,
                                          tag_out, _norm(norm), out.ctypes.data, out.strides[0] // out.itemsize, cap, so,
                                          n, lp, n_out.ctypes.data_as(_i64p), MEM_HOST))
        return out, n_out

    def apply_device(self, in_dev, n: int, out_dev, fmt="cf32", out_fmt=None, lengths=None, scale_in=None,
                     scale_out=None, norm="fixed", out_cap: int | None = None) -> np.ndarray:
        """One device-memory call: in_dev [S, >= 2 n] of fmt, out_dev [S, >= 2
        out_cap] of out_fmt (out_cap defaults to what out_dev holds).  Returns
        n_out, a host array, at once.  lengths is a host array.  Ordered on the
        handle's stream; without set_stream the caller's torch stream is
        drained first and the call is waited for."""
        fo = fmt if out_fmt is None else out_fmt
        tag_in, tag_out = _format(fmt)[0], _format(fo)[0]
        cap = out_dev.shape[1] // 2 if out_cap is None else int(out_cap)
        _check_device_rows(in_dev, self.n_streams, 2 * n, fmt, "in_dev")
        _check_device_rows(out_dev, self.n_streams, 2 * cap, fo, "out_dev")
        keep, lp = _lengths(lengths, self.n_streams)
        si, so = _scales(tag_in, tag_out, scale_in, scale_out)
        n_out = np.zeros(self.n_streams, np.int64)
        self._device_call(out_dev, lambda: lib().qpsk_tuner_apply_fmt(
            self._h, tag_in, in_dev.data_ptr(), in_dev.stride(0), si, tag_out, _norm(norm), out_dev.data_ptr(),
            out_dev.stride(0), cap, so, int(n), lp, n_out.ctypes.data_as(_i64p), MEM_DEVICE))
        return n_out

    def state(self) -> bytes:
        """The state blob behind the calls queued so far."""
        return self.get_state()

    def states(self, blob: bytes | None = None) -> np.ndarray:
        """The state as a TUNER_STATE_DTYPE array, one record a stream."""
        return np.frombuffer(self.get_state() if blob is None else blob, dtype=TUNER_STATE_DTYPE).copy()

    def reset_streams(self, streams):
        self._reset("streams", streams)


def _norm(norm):
    """QPSK_MOD_NORM_* of "fixed" / "peak" or a tag (passed on for the library to check)."""
    return _NORMS[norm] if isinstance(norm, str) else int(norm)


def quantise_iq(iq, fmt, norm="fixed", scale=1.0):
    """qpsk_quantise_iq: one row of host float32 I,Q to fmt by the modulator's
    own rules (needs no device).  Returns (row of fmt's element type, the
    row's peak as np.float32 for norm "peak", else None)."""
    tag, dtype, _ = _format(fmt)
    x = np.ascontiguousarray(iq, dtype=np.float32).reshape(-1)
    out = np.zeros(x.size, dtype=dtype)
    peak = np.zeros(1, dtype=np.float32)
    is_peak = _norm(norm) == NORM_PEAK
    _check(lib().qpsk_quantise_iq(tag, _norm(norm), C.c_float(float(np.float32(scale))),
                                  x.ctypes.data if x.size else None, x.size, out.ctypes.data if x.size else None,
                                  peak.ctypes.data if is_peak else None))
    return out, (peak[0] if is_peak else None)


def synth_generate(n_streams, n_samples, sample_rate, symbol_rate, rrc_alpha=float(np.float32(0.4)),
                   rrc_span=8, seed=0x5159534B, lo_ppm=1.0, cfo_hz=0.0, multipath=False,
                   esn0_db=None, differential=True, device=0, stream=None, out=None, tx_bits=None,
                   first_stream=0):
    """Batched synthetic baseband straight into HBM (torch tensors)."""
    import torch
    p = SynthParams()
    lib().qpsk_synth_params_init(C.byref(p), int(sample_rate), int(symbol_rate))
    p.rrc_alpha = float(rrc_alpha)
    p.rrc_span = int(rrc_span)
    p.seed = int(seed)
    p.lo_ppm = float(lo_ppm)
    p.cfo_hz = float(cfo_hz)
    p.multipath = 1 if multipath else 0
    p.esn0_db = 1000.0 if esn0_db is None else float(esn0_db)
    p.differential = 1 if differential else 0
    p.first_stream = int(first_stream)
    dev = torch.device("cuda", device)
    if out is None:
        out = torch.empty((n_streams, 2 * n_samples), dtype=torch.float32, device=dev)
    sps = sample_rate // symbol_rate
    nsym = (n_samples + 4096) // sps + 2
    if tx_bits is None:
        tx_bits = torch.zeros((n_streams, (2 * nsym + 7) // 8 + 8), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    _check(lib().qpsk_synth_generate(C.byref(p), int(device), C.c_void_p(stream or 0), n_streams,
                                     int(n_samples), out.data_ptr(), out.stride(0),
                                     tx_bits.data_ptr(), tx_bits.stride(0)))
    return out, tx_bits
