/*
 * qpsk_demod.h -- C ABI of the MI355X-native batched QPSK demodulation chain.
 *
 * This is the drop-in boundary for the reference's QPSKDeModulator C# class
 * (NustyFrozen/QPSK-Modulator-Demodulator, Modulation-Simulation/QPSKDeModulator.cs).
 * The reference has no FFI layer; its boundary *is* that public class.  A C#
 * host binds these entry points with [DllImport("qpsk_demod")] (see
 * INTEGRATION.md); one handle serves a batch of S independent streams, each of
 * which behaves exactly like one QPSKDeModulator instance.
 *
 * Conventions (QPSKDeModulator.cs:339-425):
 *  - input is interleaved float32 I,Q; every call continues the previous call's
 *    FIR / FLL / Mueller-Muller / Costas / differential-decode state;
 *  - an odd float count is QPSK_ERR_ARGUMENT (ArgumentException, :347-348);
 *  - a zero-length call returns no bits and leaves the state untouched (:350-351);
 *  - the caller owns every I/O buffer, the library owns device buffers and the
 *    per-stream state; a handle is not thread-safe (one caller thread per
 *    handle), distinct handles are independent.
 * Every function returns an int status: 0 = ok, < 0 = error, message in
 * qpsk_last_error().
 */
#ifndef QPSK_DEMOD_H
#define QPSK_DEMOD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3: multi-GPU group (qpsk_shard_streams, qpsk_demod_group_*); no change to
 *    existing entry points or the state blob.
 * 2: versioned state blob (header + length checked by set_state; 256-sample
 *    M&M carry), get_state / set_state take the buffer length and a non-const
 *    handle (they flush pipelined work), qpsk_pipeline_gate_enabled.
 * 1: rounds 1-3. */
#define QPSK_ABI_VERSION 3

/* status codes -> the C# exception each one replaces */
#define QPSK_OK 0
#define QPSK_ERR_ARGUMENT (-1)        /* ArgumentException (odd length, empty marker) */
#define QPSK_ERR_ARGUMENT_NULL (-2)   /* ArgumentNullException (QPSKDeModulator.cs:341,429) */
#define QPSK_ERR_OUT_OF_RANGE (-3)    /* ArgumentOutOfRangeException (Band-Edge Filter.cs:42-45) */
#define QPSK_ERR_DEVICE (-4)          /* HIP runtime failure */
#define QPSK_ERR_CAPACITY (-5)        /* an output row would have been truncated */
#define QPSK_ERR_STATE (-6)           /* loop state left the reference's defined behaviour
                                         (QPSK_STATUS_CARRY_OVERFLOW / _NONFINITE_TIMING), or a
                                         host ring used out of order */

/* status flags (qpsk_demod_status; a host-memory process() call returns the
 * matching error code when its own call raised one) */
#define QPSK_STATUS_CARRY_OVERFLOW 1u    /* symbol-sync queue kept > 256 samples: the queue
                                            holds <= 3 samples between calls at any sps, more
                                            only when the M&M stops on output capacity (sps
                                            below ~1); the reference keeps them all
                                            (MuellerMuller.cs:123-133) */
#define QPSK_STATUS_OUTPUT_TRUNCATED 2u  /* a bit / symbol row hit its capacity */
#define QPSK_STATUS_NONFINITE_TIMING 4u  /* a NaN/Inf sample reached the M&M timing loop: the
                                            reference's (int)Math.Floor(NaN) = 0 pins baseIndex
                                            at 0 (MuellerMuller.cs:113-115) and its outputs are
                                            no longer tracked */

/* where a pointer lives */
#define QPSK_MEM_HOST 0
#define QPSK_MEM_DEVICE 1

/* what one call produces */
#define QPSK_MODE_DEMODULATE 0        /* DeModulate: bits (+ optional symbols) */
#define QPSK_MODE_CONSTELLATION 1     /* deModulateConstellation: symbols only, diff state untouched */

/* Mirrors the QPSKDeModulator primary constructor 1:1 (QPSKDeModulator.cs:11-18)
 * plus the batch / device knobs. */
typedef struct qpsk_demod_params {
    int32_t sample_rate;            /* int SampleRate                                   */
    int32_t symbol_rate;            /* int SymbolRate                                   */
    float rrc_alpha;                /* float RrcAlpha = 0.9f                            */
    int32_t rrc_span;               /* int rrcSpan = 6                                  */
    double symbol_sync_bandwidth;   /* double SymbolSyncBandwith = 0.0001               */
    double costas_loop_bandwidth;   /* double CostasLoopBandwith = 120                  */
    double cfo_loop_bandwidth;      /* double CFOLoopBandwith = 0.0001f                 */
    int32_t differential;           /* bool differentialEncoding = true                 */
    int32_t enable_fll;             /* 0 = reference DeModulate (fll.Process disabled, :359) */
    int32_t vector_lanes;           /* Vector<float>.Count whose summation order the FIR
                                       reproduces: 8 (x64 AVX2, default), 4 (ARM64), 1 (no SIMD) */
    int32_t device;                 /* HIP device ordinal                               */
    int64_t max_samples_per_call;   /* complex samples per stream per internal chunk (device
                                       buffers), 1 .. 2^30; longer calls run as consecutive
                                       chunks with identical results */
    int32_t loop_variant;           /* symbol-loop kernel shape: 0 = auto,
                                       1 = 16 streams x 64-sample rounds, 2 = 32 x 64,
                                       3 = 16 x 128 (sps >= 2 only), 4 = 24 x 128 (sps >= 8
                                       only, else auto), 5 = 64 x 64 on the two-slot
                                       sample ring (sps >= 4 and costas_trig 0 only,
                                       else auto), 6 = 12 x 256,
                                       7 = 6 x 512 (both sps >= 8 only, else auto;
                                       32 busy lanes); results are
                                       identical */
    int32_t iq_balance;             /* 1 = IQ_Balancer.Process (IQ Balancer.cs:15-25) on every
                                       sample before the FLL / matched filter; 0 (default) =
                                       the reference DeModulate, which constructs the balancer
                                       (QPSKDeModulator.cs:38) but never calls it */
    int32_t costas_trig;            /* the Costas NCO's Math.Cos / Math.Sin (CostasLoopQpsk.cs:69-70):
                                       0 (default) = a portable table sincos within 1 ulp of
                                       glibc (bit-identical on ~98.7 % of arguments); 1 = glibc's
                                       own sin / cos restated exactly (what .NET calls on Linux
                                       x86-64; symbols bit-identical by construction, slower) */
    int32_t reserved[5];
} qpsk_demod_params;

typedef struct qpsk_demod qpsk_demod;

/* Fill defaults exactly as the C# optional parameters. */
void qpsk_demod_params_init(qpsk_demod_params *p, int32_t sample_rate, int32_t symbol_rate);

/* new QPSKDeModulator(...) x n_streams  (QPSKDeModulator.cs:11-56) */
int qpsk_demod_create(const qpsk_demod_params *p, int32_t n_streams, qpsk_demod **out);
int qpsk_demod_destroy(qpsk_demod *h);

/* Bind the handle to a caller-owned hipStream_t (NULL = library-owned stream). */
int qpsk_demod_set_stream(qpsk_demod *h, void *hip_stream);

/*
 * One DeModulate (mode 0) or deModulateConstellation (mode 1) call on every
 * stream of the batch  (QPSKDeModulator.cs:345-425 / :427-455).
 *
 * iq        [n_streams][stride_floats] float32, stream s holds
 *           2*len(s) floats, len(s) = lengths ? lengths[s] : n_samples
 * bits      [n_streams][bits_stride_bytes] raw demodulated bits of this call,
 *           packed MSB-first (BitPacker order, HelperFunctions.cs:14-29), before
 *           any TSC strip; may be NULL in mode 1
 * n_bits    [n_streams] bit counts (2 per symbol; the very first symbol of a
 *           differential stream yields none, :390-395)
 * syms      [n_streams][syms_stride_floats] rotated Costas output symbols
 *           (interleaved I,Q) or NULL
 * n_syms    [n_streams] symbol counts or NULL
 * mem       QPSK_MEM_HOST or QPSK_MEM_DEVICE for every pointer above
 * The call is synchronous for host pointers and stream-ordered for device ones.
 * Any length is accepted (QPSKDeModulator.cs:345-360 takes any span): a call
 * longer than max_samples_per_call runs as consecutive internal chunks whose
 * rows are concatenated, bit for bit what one call returns.  Host-memory calls
 * return QPSK_ERR_STATE / QPSK_ERR_CAPACITY when they raised a QPSK_STATUS_*
 * flag (outputs are still written); device-memory calls report them through
 * qpsk_demod_status.
 * Bytes of a bit row past the last bit (and floats of a symbol row past the
 * last symbol) are unspecified.  Device rows that are 4-byte aligned with
 * bits_stride_bytes % 4 == 0 (8-byte aligned, even syms_stride_floats for
 * symbols) are written in place by the loop kernel, whole 32-bit words up to
 * the row's last bit; other rows are filled from an internal buffer by a copy.
 */
int qpsk_demod_process(qpsk_demod *h, int32_t mode, const float *iq, int64_t stride_floats,
                       int64_t n_samples, const int64_t *lengths, int32_t mem, uint8_t *bits,
                       int64_t bits_stride_bytes, int64_t *n_bits, float *syms,
                       int64_t syms_stride_floats, int64_t *n_syms);

/*
 * Pipelined DeModulate calls (device memory only).  Same arguments, checks and
 * results as qpsk_demod_process(mem = QPSK_MEM_DEVICE); calls still apply to
 * every stream in order and carry the state exactly as synchronous calls do.
 * The difference is scheduling: each call is split into a front stage (FLL on:
 * the FLL; FLL off: the matched filter) and a back stage (the rest) on two
 * library streams, so call k+1's front stage runs while call k's symbol loop
 * runs.  A C# host feeding consecutive SDR buffers keeps the GPU busy this
 * way instead of waiting for each DeModulate to return.
 *  - iq is read after the work already queued on the handle's stream; it must
 *    stay unchanged until qpsk_demod_pipeline_wait has been called for it.
 *  - bits / n_bits / syms / n_syms are complete after qpsk_demod_pipeline_wait.
 *  - synchronous process(), get/set_state, set_stream and destroy first wait
 *    for every pipelined call.
 *  - Residency gate: call k+1's matched filter waits ON THE DEVICE (a
 *    one-wave kernel ahead of it on the front stream) until call k's
 *    symbol-loop workgroups hold their CUs, so the two always overlap in the
 *    same order.  The wait is bounded: after QPSK_GATE_TIMEOUT_MS (default
 *    2000 ms, read at create) the filter goes ahead and the timeout is counted
 *    (qpsk_demod_gate_timeouts); results never depend on the gate.  Under
 *    serialised dispatch the loop kernel could only start after the waiting
 *    filter, so every wait would run out: the gate is off when
 *    qpsk_pipeline_gate_enabled() says so:
 *    QPSK_PIPELINE_GATE=0, AMD_SERIALIZE_KERNEL or AMD_SERIALIZE_COPY != 0,
 *    HIP_LAUNCH_BLOCKING or CUDA_LAUNCH_BLOCKING != 0, rocprofv3 counter
 *    collection (ROCPROF_COUNTER_COLLECTION=1) or kernel serialisation
 *    (ROCPROFILER_KERNEL_SERIALIZATION), HSA_ENABLE_DEBUG.  A tool that
 *    serialises dispatch without any of these (e.g. a debugger attached after
 *    start-up) costs one timeout per call: set QPSK_PIPELINE_GATE=0 for such
 *    runs (results are identical with the gate off; only the overlap order may
 *    vary).
 *    QPSK_PIPELINE_GATE=1 forces it on.  Read once per handle, at create.
 */
int qpsk_demod_process_async(qpsk_demod *h, int32_t mode, const float *iq, int64_t stride_floats,
                             int64_t n_samples, const int64_t *lengths, uint8_t *bits,
                             int64_t bits_stride_bytes, int64_t *n_bits, float *syms,
                             int64_t syms_stride_floats, int64_t *n_syms);
/*
 * CS16 input: interleaved int16 I,Q, the format SDR hardware and SoapySDR
 * streams deliver natively (the reference asks its driver for CF32 only
 * because its FIR takes floats, ModDemodOverSDR.cs:116-183).  A sample's value
 * is (float)x * scale: one exact conversion, then one float multiply (no fma),
 * done inside the first kernel that reads the samples, so the chain computes
 * bit for bit what it computes from the widened floats and no float copy of
 * the input is written to device memory (FLL off, no IQ balancer; with either
 * of them one widening pass fills an internal row ahead of it).  All state
 * stays float: a handle may alternate float and CS16 calls freely.
 *
 * The scale is per handle, 1.0f / 32768 by default (SoapySDR's CS16 -> CF32
 * convention), and is captured when a call is issued: set waits for nothing
 * and affects later calls only; pipelined calls already queued keep theirs.
 * It must be finite and > 0, else QPSK_ERR_OUT_OF_RANGE.
 */
int qpsk_demod_set_cs16_scale(qpsk_demod *h, float scale);
int qpsk_demod_get_cs16_scale(const qpsk_demod *h, float *scale);
/* qpsk_demod_process / qpsk_demod_process_async with iq as
 * [n_streams][stride_i16] int16, stream s holding 2*len(s) int16; every other
 * argument, check, limit and result as there (calls longer than
 * max_samples_per_call chunk the same way; qpsk_demod_last_mf works after the
 * synchronous one).  Device rows must be 4-byte aligned with an even
 * stride_i16, else QPSK_ERR_ARGUMENT; rows that are 16-byte aligned with
 * stride_i16 % 8 == 0 are read with 16-byte loads (4 samples), others with
 * 4-byte loads. */
int qpsk_demod_process_cs16(qpsk_demod *h, int32_t mode, const int16_t *iq, int64_t stride_i16,
                            int64_t n_samples, const int64_t *lengths, int32_t mem, uint8_t *bits,
                            int64_t bits_stride_bytes, int64_t *n_bits, float *syms,
                            int64_t syms_stride_floats, int64_t *n_syms);
int qpsk_demod_process_async_cs16(qpsk_demod *h, int32_t mode, const int16_t *iq, int64_t stride_i16,
                                  int64_t n_samples, const int64_t *lengths, uint8_t *bits,
                                  int64_t bits_stride_bytes, int64_t *n_bits, float *syms,
                                  int64_t syms_stride_floats, int64_t *n_syms);
/* 1 if handles created now use the residency gate, 0 if the environment turns
 * it off (the list above); needs no device. */
int qpsk_pipeline_gate_enabled(void);
/* Residency-gate waits of this handle that ran out (QPSK_GATE_TIMEOUT_MS) since
 * it was created, after every queued call; 0 in normal operation.  Besides
 * serialised dispatch, contention can also run a wait out: at most one loop
 * workgroup fits a CU (its LDS), so another handle's or process's loop kernel
 * holding every CU for longer than the cap delays this one's workgroups past
 * it.  Nothing hangs and no result changes; only the overlap order of that
 * call may differ.  Raise QPSK_GATE_TIMEOUT_MS where handles share a GPU with
 * long calls.  (QPSK_GATE_NO_PUBLISH=1 is a test hook that suppresses the
 * count so every wait runs out; it is honoured only together with
 * QPSK_PIPELINE_GATE=1.) */
int qpsk_demod_gate_timeouts(qpsk_demod *h, uint64_t *count);
/* The symbol-loop shape qpsk_demod_create picks for loop_variant = 0 (auto):
 * at sps >= 8, 7 (6 streams x 512-sample rounds) while ceil(S/6) <= cus, else
 * 6 (12 x 256) while ceil(S/12) <= cus, else 0 (the launcher's default for the
 * sps: 32 x 64 at sps >= 2).  (24 x 128, variant 4, needed ceil(S/24) <= cus/2,
 * which no batch past the 12 x 256 bound meets; it is only picked on request.)
 * A requested variant != 0 is returned unchanged.  Needs no device. */
int32_t qpsk_demod_pick_loop_variant(int32_t requested, int32_t n_streams, double sps, int32_t cus);
/* The geometry of the symbol-loop shape a handle of n_streams streams runs for
 * a requested loop_variant (through qpsk_demod_pick_loop_variant and the
 * launcher's own rule for what that leaves at 0), on a device of cus CUs
 * (0 = unknown) with a matched filter of rrc_taps taps (rrc_span * sps + 1),
 * for costas_trig 0 / 1 and with (1) or without (0) symbol output (a handle
 * with link statistics enabled runs the with-symbols form in every call).  The
 * launcher's rule: at 4 <= sps < 8 and costas_trig 0, 64 streams x 64-sample
 * rounds on the two-slot ring where n_streams * rrc_taps >= cus * 16 * 129
 * (the matched filter of the next pipelined call sets the step: C3), else
 * 32 x 64.  Needs no device. */
typedef struct qpsk_loop_shape {
    int32_t streams;        /* streams (LDS rows) per workgroup                          */
    int32_t lanes;          /* busy lanes of the stage waves (>= streams: shadow lanes)   */
    int32_t round;          /* samples per round                                          */
    int32_t slots;          /* rounds the sample ring holds: 4, or 2 (two-slot ring)      */
    int32_t prefix;         /* two-slot ring: samples loaded in front of a round, else 0  */
    int32_t cap;            /* symbol slots per stream and round (row stride cap + 1)     */
    int32_t lds_bytes;      /* LDS of the workgroup                                       */
    int32_t fir_beside;     /* matched-filter workgroups of the next pipelined call that  */
    int32_t fir_taps;       /*   fit the CU beside it, of this many taps, each of         */
    int32_t fir_lds_bytes;  /*   this much LDS (0: no claim made, e.g. with symbols)      */
    int32_t lds_granule;    /* LDS allocation granule of a CU, bytes                      */
    int32_t reserved;
    double lag_max;         /* largest backlog (samples) a stream carries into a round    */
} qpsk_loop_shape;
int qpsk_demod_loop_shape(int32_t requested, int32_t n_streams, double sps, int32_t cus, int32_t rrc_taps,
                          int32_t costas_trig, int32_t want_syms, qpsk_loop_shape *out);
/* OR of the QPSK_STATUS_* flags raised since the last qpsk_demod_status call
 * (waits for every queued call), then cleared.  0 = every call so far stayed
 * inside the reference's defined behaviour. */
int qpsk_demod_status(qpsk_demod *h, uint32_t *flags);

/* The matched-filter output (ComplexFIRFilter.Filter, FIRFilter.cs:80-91) of
 * the last synchronous qpsk_demod_process call of at most max_samples_per_call
 * samples: n_samples per stream into out [S][stride_floats] (host or device
 * memory).  For inspection and FIR parity checks; pipelined and chunked calls
 * leave other buffers behind. */
int qpsk_demod_last_mf(qpsk_demod *h, float *out, int64_t stride_floats, int64_t n_samples, int32_t mem);

/* Make hip_stream wait for every pipelined call issued so far (NULL: block the
 * calling host thread until they are done). */
int qpsk_demod_pipeline_wait(qpsk_demod *h, void *hip_stream);
/* 2 = the stage boundary is double-buffered (front and back stages overlap),
 * 1 = no device memory was left for the second buffer (stages serialise),
 * 0 = no pipelined call yet. */
int qpsk_demod_pipeline_depth(const qpsk_demod *h);

/* Upper bounds a caller sizes outputs with, for a call of n_samples per stream. */
int64_t qpsk_demod_max_symbols(const qpsk_demod *h, int64_t n_samples);

/* First ordinal occurrence of tsc (a '0'/'1' string) in a packed bit row, i.e.
 * rx.IndexOf(_tsc, StringComparison.Ordinal) (QPSKDeModulator.cs:413-422).
 * Returns the bit index just past the TSC, or -1. */
int64_t qpsk_tsc_find(const uint8_t *bits, int64_t n_bits, const char *tsc);

/* Kernel launch times of the calls issued since timing was enabled (the first
 * 4096 of them), recorded by the kernels themselves: first workgroup start to
 * last workgroup end on the device's 100 MHz wall clock, so a launch's time is
 * its own span whichever stream or neighbour it ran beside (pipelined calls
 * included).  enable_timing(on) restarts the record.
 * stage_times: averages over the recorded calls of ms[0] = FLL, ms[1] =
 * matched-filter FIR, ms[2] = symbol-sync + Costas + decode kernel, ms[3] =
 * the call's kernel span (earliest start to latest end); a kernel that did not
 * run counts as absent.  Returns the number of entries written (<= 4).
 * launch_times: the same four values per call, ms[4*k .. 4*k+3] for call k
 * (0 = did not run); returns the number of calls written (<= max_calls).
 * kernel_clocks: per recorded call, the shader clock (GHz) the FLL, the FIR
 * and the loop kernel ran at, ghz[3*k .. 3*k+2]: shader-clock ticks
 * (s_memtime) over wall ticks of a sample of their waves' lifetimes (FIR:
 * every 64th workgroup; FLL: every workgroup; loop: every M&M wave; 0 = did
 * not run); returns the calls written. */
int qpsk_demod_enable_timing(qpsk_demod *h, int32_t on);
int qpsk_demod_stage_times(qpsk_demod *h, float *ms, int32_t n);
int qpsk_demod_launch_times(qpsk_demod *h, float *ms, int32_t max_calls);
int qpsk_demod_kernel_clocks(qpsk_demod *h, float *ghz, int32_t max_calls);

/* FIR phase sample (diagnostic): while on, every 64th matched-filter
 * workgroup adds the shader cycles of its three phases -- stage (HBM -> LDS),
 * products and sums, stores -- to one of two sums, chosen by whether a
 * symbol-loop workgroup of this handle held its CU when it started (each loop
 * workgroup marks its CU, read from the hardware HW_ID / XCC_ID registers).
 * fir_phases: out[8 * shared + k], k = 0 stage, 1 compute, 2 store cycles, 3
 * workgroups, shared = 0 free CU / 1 loop-shared CU (n >= 16); the sums are
 * then cleared.  Returns 16. */
int qpsk_demod_enable_fir_phases(qpsk_demod *h, int32_t on);
int qpsk_demod_fir_phases(qpsk_demod *h, uint64_t *out, int32_t n);

/* Design products, for parity checks against the reference constructor. */
int qpsk_demod_rrc_taps(const qpsk_demod *h, float *taps, int32_t cap);
int qpsk_demod_gains(const qpsk_demod *h, double *mm_sps, double *kp, double *ki,
                     double *costas_alpha, double *costas_beta);
int qpsk_demod_fll_taps(const qpsk_demod *h, float *lower_iq, float *upper_iq, int32_t cap_floats);

/* Constructor math without a device: RRC taps (float, as widened by
 * ToInterleavedIQRealTaps, QPSKDeModulator.cs:278-288), gains[5] = {M&M sps,
 * kp, ki, Costas alpha, Costas beta}, FLL band-edge taps (interleaved, 80
 * floats each).  Returns the tap count or an error (same validation as create). */
int qpsk_demod_design(const qpsk_demod_params *p, float *rrc_taps, int32_t cap, double *gains,
                      float *fll_lower_iq, float *fll_upper_iq);

/* Loop state snapshot (checkpoint / migration): a 32-byte header (magic
 * "QPSK", format 2, streams, RRC taps, carry length, FLL taps, record size)
 * then one record per stream, the M&M carries, FIR histories and FLL delay
 * lines.  get_state needs buf_bytes >= state_bytes; set_state needs exactly
 * state_bytes and a header matching this handle, else QPSK_ERR_ARGUMENT (a
 * blob of another handle shape or library version is never misread).  Both
 * first wait for (and flush) pipelined calls. */
int64_t qpsk_demod_state_bytes(const qpsk_demod *h);
int qpsk_demod_get_state(qpsk_demod *h, void *host_buf, int64_t buf_bytes);
int qpsk_demod_set_state(qpsk_demod *h, const void *host_buf, int64_t buf_bytes);

/* A blob is external input (a file, another host): the kernels use a record's
 * integers and its timing phase as addresses, so every blob is checked on the
 * host before a byte of it reaches the device.  Needs no device and no handle:
 * the tap count and the M&M samples per symbol come from p as in
 * qpsk_demod_design.  Checks the length, the header against (p, n_streams),
 * then every record: carry_n in [0, 256], fll_pos in [0, 40), tofs == 0,
 * has_prev and diff_have 0 or 1, error in [0, 3], base in [0, 1 + ceil(sps +
 * 0.1)], mu in [+0, 1) (DESIGN.md "State blob" derives each range).  Every
 * other float is data and is taken as it is, NaN and Inf included.  Returns
 * QPSK_OK or QPSK_ERR_ARGUMENT; qpsk_last_error names the stream, the field,
 * its value and the allowed range.  set_state runs it with the handle's own
 * params first; a rejected blob leaves the handle untouched.  (Added within
 * ABI version 3: no existing entry point or the blob layout changed.) */
int qpsk_state_blob_check(const qpsk_demod_params *p, int32_t n_streams, const void *buf, int64_t buf_bytes);

/* ---------------------------------------------------------------------------
 * Per-stream link statistics: which of the batch's receivers are locked, in 64
 * bytes a stream, without symbol rows and without the state blob.  (Added
 * within ABI version 3: no existing entry point or the blob layout changed.)
 *
 * The reference computes each symbol's squared distance to its decision and
 * drops it (QPSKDeModulator.cs:381-384), and offers the Costas NCO state
 * through CostasLoopQpsk.GetState() (CostasLoopQpsk.cs:127-130).  While
 * statistics are enabled, every symbol the Costas loop produces adds to three
 * running sums of its stream.  Per symbol, in float, one rounding per
 * operation (no fused multiply-add):
 *     dec  = rot >= 0 ? 1 : -1          (GetSign, so a NaN gives -1), I and Q
 *     e    = rot - dec
 *     dist2 = eI*eI + eQ*eQ
 *     pw    = rotI*rotI + rotQ*rotQ
 * then sum_dist2 += (double)dist2 and sum_power += (double)pw, in symbol order
 * from the running value.  The sums therefore do not depend on how the
 * samples were cut into calls or internal chunks.  They run across calls
 * (synchronous, chunked, pipelined, through a qpsk_rx ring or a group) until a
 * read resets them; a host that wants per-call figures reads with reset = 1
 * after each call.  Both modes count, and a symbol counts even where a symbol
 * row hit its capacity.  A stream with no samples in a call is untouched.
 * qpsk_demod_set_state leaves the sums alone.  No thresholds are applied: the
 * host judges mean dist2 against mean power and |costas_freq|.
 */
typedef struct qpsk_link_stats {      /* 64 bytes, no padding */
    int64_t n_symbols;    /* symbols the Costas loop produced since the last reset           */
    double  sum_dist2;    /* sum of (double)dist2, dist2 in float as QPSKDeModulator.cs:381-384 */
    double  sum_power;    /* sum of (double)(rotI*rotI + rotQ*rotQ), the products and the add in float */
    double  costas_freq;  /* CostasLoopQpsk.GetState().freq  (rad/symbol) after the last call */
    double  costas_theta; /* ... .theta                                                       */
    double  mm_mu;        /* MuellerMuller.mu                                                 */
    double  mm_rate;      /* MuellerMuller.ncoIntegral                                        */
    float   fll_freq;     /* Band-Edge FLL freq (0 with the FLL off)                          */
    int32_t error;        /* the stream record's sticky `error`, as get_state returns it      */
} qpsk_link_stats;
/* sizeof(qpsk_link_stats) = 64; needs no device. */
int qpsk_link_stats_size(void);
/* Waits for every queued call (as qpsk_demod_set_stream does), then turns the
 * statistics on or off.  Turning them on, also when they are on already,
 * zeroes the three sums of every stream.  While they are off (the default)
 * every launch is exactly what it is without this feature.  While they are on,
 * the symbol loop runs its symbol-carrying form whether or not a call asks for
 * symbol rows (results are identical; DESIGN.md 3.11 has the cost). */
int qpsk_demod_enable_link_stats(qpsk_demod *h, int32_t on);
/* Waits for every queued call (as qpsk_demod_status does), then writes one row
 * per stream to out: host memory (mem = QPSK_MEM_HOST) or device memory
 * (QPSK_MEM_DEVICE; 8-byte aligned, else QPSK_ERR_ARGUMENT; written in order
 * on the handle's stream).  reset != 0 then zeroes the three sums; the loop
 * state fields are a copy of the state and are never reset.  QPSK_ERR_STATE
 * while statistics are not enabled.  Like qpsk_demod_status it may be called
 * on a handle that feeds a qpsk_rx ring. */
int qpsk_demod_link_stats(qpsk_demod *h, qpsk_link_stats *out, int32_t mem, int32_t reset);

/* ---------------------------------------------------------------------------
 * Selected streams: reset, read and write the state of the rows a caller
 * names, and of no other.  (Added within ABI version 3: no existing entry
 * point or the blob layout changed.)
 *
 * The reference constructs and drops each receiver on its own
 * (QPSKDeModulator.cs:11-56); a handle makes all of its rows at once, and
 * qpsk_demod_get_state / set_state move all of them.  These calls give one row
 * the lifetime of one instance: a new receiver on row s (a stream in a Costas
 * false lock, a client that reconnects), and a stream moved to another handle
 * or another GPU, at the cost of the rows moved.
 *
 * A stream list is n indices into the batch: 1 <= n <= n_streams, every index
 * in [0, n_streams), none twice, in any order; else QPSK_ERR_ARGUMENT, and
 * qpsk_last_error names the position and the value.
 *
 * The rows of n listed streams, laid out as header (streams = n), records,
 * carries, histories and delay lines in list order, are themselves a state
 * blob of an n-stream handle with the same tap count: a "sub-blob" is no new
 * format.  qpsk_state_blob_check(p, n, sub, bytes) and qpsk_demod_set_state of
 * an n-stream handle take it as it is.
 */
/* The three below need no device and no handle (p as in qpsk_state_blob_check). */
int qpsk_stream_list_check(int32_t n_streams, const int32_t *streams, int32_t n);
/* sub <- the sub-blob of rows streams[0..n) of blob, in list order.  First
 * qpsk_state_blob_check on blob for (p, n_streams); blob_bytes and sub_bytes
 * are exact.  A rejected call writes nothing. */
int qpsk_state_blob_select(const qpsk_demod_params *p, int32_t n_streams, const void *blob, int64_t blob_bytes,
                           const int32_t *streams, int32_t n, void *sub, int64_t sub_bytes);
/* Row streams[i] of blob <- row i of sub, and no other byte of blob.  First
 * qpsk_state_blob_check on sub for (p, n) and on blob for (p, n_streams).  A
 * rejected call changes nothing. */
int qpsk_state_blob_merge(const qpsk_demod_params *p, int32_t n_streams, void *blob, int64_t blob_bytes,
                          const int32_t *streams, int32_t n, const void *sub, int64_t sub_bytes);
/* On a handle.  Each call checks its arguments on the host first (a rejected
 * call neither waits nor changes anything), then waits for every queued call,
 * pipelined ones included, as qpsk_demod_set_state and qpsk_demod_link_stats
 * do: a stream's record holds fields of both pipeline stages, so no row is
 * written between queued calls (DESIGN.md 3.12 has the cost).  It then runs on
 * the handle's stream and returns when done.  Like qpsk_demod_link_stats they
 * may be called on a handle that feeds a qpsk_rx ring, between submits.
 * Handle-wide things stay as they are: status flags, input scales, timing
 * records.
 *
 * reset_streams is `new QPSKDeModulator(...)` on those rows: the symbol-sync
 * and Costas loops, the matched filter's history, the FLL and IQ-balancer
 * state, the differential decoder (the fields of QPSKDeModulator.cs:20-73) and
 * the sticky `error` go back to construction, and the rows' three link sums
 * are zeroed (a new receiver has seen no symbol).  n = 0 is QPSK_OK and does
 * nothing.
 *
 * streams_state_bytes: the bytes of a blob of n streams; 0 for a null handle
 * or n outside [1, n_streams].  get_streams_state writes the sub-blob of the
 * listed rows as they are (buf_bytes exactly streams_state_bytes; a row with a
 * carry-overflow record is returned, and a later set refuses it).
 * set_streams_state runs qpsk_state_blob_check on the sub-blob for n streams,
 * then overwrites the listed rows; it leaves the link sums alone, as
 * qpsk_demod_set_state does.  For both n = 0 is QPSK_ERR_ARGUMENT: there is no
 * blob of zero streams. */
int qpsk_demod_reset_streams(qpsk_demod *h, const int32_t *streams, int32_t n);
int64_t qpsk_demod_streams_state_bytes(const qpsk_demod *h, int32_t n);
int qpsk_demod_get_streams_state(qpsk_demod *h, const int32_t *streams, int32_t n, void *host_buf, int64_t buf_bytes);
int qpsk_demod_set_streams_state(qpsk_demod *h, const int32_t *streams, int32_t n, const void *host_buf,
                                 int64_t buf_bytes);

/* ---------------------------------------------------------------------------
 * Multi-GPU group: one batch of n_streams over several GPUs,
 * for a host (the C# shim, a C++ driver) that wants the whole node behind one
 * object.  Every reference instance owns its loop state (QPSKDeModulator.cs:20-73),
 * so the batch splits into contiguous shards with no exchange: shard k =
 * streams [n*k/n_dev, n*(k+1)/n_dev) on devices[k], one ordinary handle each
 * (the split bench.py's ranks use).  A group call slices the caller's rows by
 * row offset (shard k reads iq + first_k*stride_floats, lengths + first_k and
 * writes bits + first_k*bits_stride_bytes, n_bits + first_k, syms + ..., n_syms
 * + ...), runs every shard at once on its own worker thread, and returns when
 * all are done.  Results equal one handle's over the whole batch, stream for
 * stream.  One caller thread per group, as for a handle.
 */
typedef struct qpsk_demod_group qpsk_demod_group;
/* Contiguous shard k of n_parts over n_streams: *first = n_streams*k/n_parts,
 * *count = n_streams*(k+1)/n_parts - *first.  Needs no device. */
int qpsk_shard_streams(int32_t n_streams, int32_t n_parts, int32_t k, int32_t *first, int32_t *count);
/* n_dev handles with params p (p->device ignored: shard k lives on devices[k];
 * a device may repeat, e.g. two shards on device 0).  n_streams >= n_dev. */
int qpsk_demod_group_create(const qpsk_demod_params *p, const int32_t *devices, int32_t n_dev,
                            int32_t n_streams, qpsk_demod_group **out);
/* Waits for every shard's work, destroys the handles, stops the workers. */
int qpsk_demod_group_destroy(qpsk_demod_group *g);
/* Number of shards (n_dev). */
int qpsk_demod_group_size(const qpsk_demod_group *g);
/* Shard k's first stream, stream count, device and handle (any may be NULL).
 * The handle belongs to the group; use it for device-resident batches on a
 * multi-GPU group (pointers on that shard's device), streams, timing. */
int qpsk_demod_group_shard(const qpsk_demod_group *g, int32_t k, int32_t *first_stream, int32_t *n_streams,
                           int32_t *device, qpsk_demod **handle);
/* qpsk_demod_process on every shard, fanned out and joined; arguments as for
 * one handle over all n_streams rows.  mem = QPSK_MEM_HOST (the C# spans) on
 * any group; QPSK_MEM_DEVICE only when every shard is on one device (else
 * QPSK_ERR_ARGUMENT: call the shard handles), and the call then returns with
 * the outputs written (each shard's stream is joined).  Arguments are checked
 * on the whole batch before any shard runs; a shard that fails later returns
 * its status with "shard k (device d): ..." in qpsk_last_error, the other
 * shards' calls having run (as independent C# instances would). */
int qpsk_demod_group_process(qpsk_demod_group *g, int32_t mode, const float *iq, int64_t stride_floats,
                             int64_t n_samples, const int64_t *lengths, int32_t mem, uint8_t *bits,
                             int64_t bits_stride_bytes, int64_t *n_bits, float *syms, int64_t syms_stride_floats,
                             int64_t *n_syms);
/* Per-shard checkpoint / migration: qpsk_demod_state_bytes / get_state /
 * set_state of shard k's handle (0 bytes for a bad k). */
int64_t qpsk_demod_group_state_bytes(const qpsk_demod_group *g, int32_t k);
int qpsk_demod_group_get_state(qpsk_demod_group *g, int32_t k, void *host_buf, int64_t buf_bytes);
int qpsk_demod_group_set_state(qpsk_demod_group *g, int32_t k, const void *host_buf, int64_t buf_bytes);
/* qpsk_demod_enable_link_stats / qpsk_demod_link_stats on every shard: the
 * rows of all n_streams streams in stream order, in host memory. */
int qpsk_demod_group_enable_link_stats(qpsk_demod_group *g, int32_t on);
int qpsk_demod_group_link_stats(qpsk_demod_group *g, qpsk_link_stats *out_host, int32_t reset);
/* Selected streams of the group by global stream id (0 .. n_streams - 1 over
 * the whole batch).  The list, and for set the whole sub-blob, is checked
 * before any shard runs; each shard then works on its own rows on its worker.
 * A stream moves between GPUs in two calls: get on one id, set on another. */
int qpsk_demod_group_reset_streams(qpsk_demod_group *g, const int32_t *streams, int32_t n);
int64_t qpsk_demod_group_streams_state_bytes(const qpsk_demod_group *g, int32_t n);
int qpsk_demod_group_get_streams_state(qpsk_demod_group *g, const int32_t *streams, int32_t n, void *host_buf,
                                       int64_t buf_bytes);
int qpsk_demod_group_set_streams_state(qpsk_demod_group *g, const int32_t *streams, int32_t n,
                                       const void *host_buf, int64_t buf_bytes);

/* ---------------------------------------------------------------------------
 * Host-fed streaming front-end: the deployment shape of
 * ModDemodOverSDR.cs:116-183, where the SDR thread hands CF32 buffers to
 * DeModulate one after another.  A ring of `depth` pinned host slots feeds one
 * handle: submit k uploads slot k on the DMA engine and queues a pipelined
 * DeModulate of it (qpsk_demod_process_async), so chunk k+1's upload overlaps
 * chunk k's matched filter and symbol loop, and chunk k's bits come back while
 * chunk k+1 computes.  collect returns the oldest outstanding chunk's bits.
 * Results equal consecutive qpsk_demod_process calls on the same chunks.  One
 * caller thread per ring, as for the handle (QPSKDeModulator is not
 * thread-safe either).
 */
typedef struct qpsk_rx qpsk_rx;
/* depth: 2..8 slots of n_streams x max_samples_per_call complex samples.  The
 * ring binds the handle to its own upload stream (as qpsk_demod_set_stream);
 * do not call the handle directly while the ring lives. */
int qpsk_rx_create(qpsk_demod *h, int32_t depth, qpsk_rx **out);
/* Waits for every outstanding chunk, then frees the ring (the handle keeps its
 * state and returns to a library-owned stream). */
int qpsk_rx_destroy(qpsk_rx *r);
/* The pinned host slot the next submit reads, [n_streams][*stride_floats]
 * interleaved I,Q: fill it in place (e.g. as an SDR driver's receive buffer)
 * and pass it to submit to skip the host copy.  QPSK_ERR_STATE while that slot
 * still holds an uncollected chunk. */
int qpsk_rx_next_slot(qpsk_rx *r, float **iq, int64_t *stride_floats);
/* Queue one DeModulate call on every stream.  iq: host rows, copied into the
 * slot unless iq is the slot itself; n_samples / lengths as in
 * qpsk_demod_process.  *ticket = the call's sequence number (may be NULL).
 * QPSK_ERR_STATE when all depth slots hold uncollected chunks. */
int qpsk_rx_submit(qpsk_rx *r, const float *iq, int64_t stride_floats, int64_t n_samples,
                   const int64_t *lengths, int64_t *ticket);
/* Wait for the oldest uncollected chunk and copy its bits (packed MSB-first,
 * as qpsk_demod_process) and bit counts to host memory.  QPSK_ERR_STATE when
 * nothing is outstanding. */
int qpsk_rx_collect(qpsk_rx *r, uint8_t *bits, int64_t bits_stride_bytes, int64_t *n_bits,
                    int64_t *ticket);
/* The same ring for CS16 buffers (a SoapySDR CS16 stream read straight into a
 * slot): qpsk_rx_create / qpsk_rx_next_slot / qpsk_rx_submit with pinned slots
 * of [n_streams][2 * max_samples_per_call] int16, half the pinned memory and
 * half the upload bytes, queued as qpsk_demod_process_async_cs16 with the
 * handle's scale at submit.  collect and destroy are the float ring's.  The
 * float next_slot / submit on a CS16 ring, and these on a float ring, return
 * QPSK_ERR_STATE. */
int qpsk_rx_create_cs16(qpsk_demod *h, int32_t depth, qpsk_rx **out);
int qpsk_rx_next_slot_cs16(qpsk_rx *r, int16_t **iq, int64_t *stride_i16);
int qpsk_rx_submit_cs16(qpsk_rx *r, const int16_t *iq, int64_t stride_i16, int64_t n_samples,
                        const int64_t *lengths, int64_t *ticket);

/* ---------------------------------------------------------------------------
 * Format-tagged entry points, and 8-bit input (CS8, CU8).
 *
 * The reference asks its driver for ComplexFloat32 (ModDemodOverSDR.cs:63-64)
 * and hands those buffers to DeModulate (the receive loop, :116-183).  HackRF
 * and RTL-SDR hardware, whose SoapySDR modules the reference ships, deliver
 * 8-bit samples natively: SoapySDR "CS8" (interleaved int8 I,Q) and the raw
 * "CU8" (interleaved uint8 I,Q, offset 128) of rtl-sdr and most capture files.
 * One family of entry points takes the sample format as an argument, so a
 * format adds no functions; the float and _cs16 entry points above are these
 * with their format fixed.
 *
 * A sample's value (SoapySDR's S8toF32 / U8toS8, full scale 128):
 *   QPSK_FMT_CS8   (float)(int8)x * scale
 *   QPSK_FMT_CU8   (float)((int)x - 128) * scale
 * The integer is exact in float and the multiply is the one rounding (no fma),
 * done inside the first kernel that reads the samples, as for CS16 input: the
 * chain computes bit for bit what it computes from the widened floats, and
 * all state stays float, so a handle may alternate all four formats call by
 * call (the state blob and QPSK_ABI_VERSION are unchanged).
 */
#define QPSK_FMT_CF32 0   /* interleaved float32 I,Q: qpsk_demod_process           */
#define QPSK_FMT_CS16 1   /* interleaved int16 I,Q:   qpsk_demod_process_cs16      */
#define QPSK_FMT_CS8 2    /* interleaved int8 I,Q                                  */
#define QPSK_FMT_CU8 3    /* interleaved uint8 I,Q, zero at 128                    */
/* Bytes of one complex sample: 8 / 4 / 2 / 2; negative (QPSK_ERR_ARGUMENT) for
 * an unknown format.  A row's stride_elems counts elements of half that size
 * (floats, int16 or bytes).  Needs no device.  Every entry point below returns
 * QPSK_ERR_ARGUMENT for an unknown fmt. */
int qpsk_fmt_sample_bytes(int32_t fmt);
/* The scale of an integer format, per handle and per format: 1.0f / 32768 for
 * CS16 (the variable qpsk_demod_set_cs16_scale sets), 1.0f / 128 for CS8 and
 * CU8.  Captured when a call is issued, as the CS16 scale is; finite and > 0,
 * else QPSK_ERR_OUT_OF_RANGE (the scale is then unchanged).  CF32 has no
 * scale: QPSK_ERR_ARGUMENT. */
int qpsk_demod_set_input_scale(qpsk_demod *h, int32_t fmt, float scale);
int qpsk_demod_get_input_scale(const qpsk_demod *h, int32_t fmt, float *scale);
/* qpsk_demod_process / qpsk_demod_process_async with iq as
 * [n_streams][stride_elems] elements of fmt, stream s holding 2*len(s) of
 * them; every other argument, check, limit and result as there (longer calls
 * chunk the same way; qpsk_demod_last_mf works after the synchronous one).
 * Device rows of CF32 and CS16 follow the rules of their own entry points.
 * Device rows of an 8-bit format must be 2-byte aligned with an even
 * stride_elems, else QPSK_ERR_ARGUMENT; rows that are 16-byte aligned with
 * stride_elems % 16 == 0 are read with 16-byte loads (8 samples; 8-byte loads
 * of 4 samples, from 8-byte alignment and stride_elems % 8 == 0 on, for the 13-
 * and 21-tap filters), others with 2-byte loads.  Host-memory calls are staged
 * in rows pitched to 8 samples and always take the wide loads.  A device call
 * longer than max_samples_per_call reads chunk k at iq + 2 * k *
 * max_samples_per_call elements, so its chunks after the first keep the wide
 * loads only when max_samples_per_call is a multiple of 8 (the same holds for
 * CS16 rows and a multiple of 4); the results do not depend on it. */
int qpsk_demod_process_fmt(qpsk_demod *h, int32_t fmt, int32_t mode, const void *iq, int64_t stride_elems,
                           int64_t n_samples, const int64_t *lengths, int32_t mem, uint8_t *bits,
                           int64_t bits_stride_bytes, int64_t *n_bits, float *syms,
                           int64_t syms_stride_floats, int64_t *n_syms);
int qpsk_demod_process_async_fmt(qpsk_demod *h, int32_t fmt, int32_t mode, const void *iq, int64_t stride_elems,
                                 int64_t n_samples, const int64_t *lengths, uint8_t *bits,
                                 int64_t bits_stride_bytes, int64_t *n_bits, float *syms,
                                 int64_t syms_stride_floats, int64_t *n_syms);
/* qpsk_rx_create / qpsk_rx_next_slot / qpsk_rx_submit for a ring of any one
 * format: pinned slots of [n_streams][2 * max_samples_per_call] elements (an
 * 8-bit ring: bytes, a quarter of the float ring's pinned memory and upload),
 * queued as qpsk_demod_process_async_fmt with the handle's scale at submit.
 * A ring has one format: next_slot / submit with another one (these or the
 * float and _cs16 ones) return QPSK_ERR_STATE.  collect and destroy are the
 * float ring's. */
int qpsk_rx_create_fmt(qpsk_demod *h, int32_t depth, int32_t fmt, qpsk_rx **out);
int qpsk_rx_next_slot_fmt(qpsk_rx *r, int32_t fmt, void **iq, int64_t *stride_elems);
int qpsk_rx_submit_fmt(qpsk_rx *r, int32_t fmt, const void *iq, int64_t stride_elems, int64_t n_samples,
                       const int64_t *lengths, int64_t *ticket);
/* qpsk_demod_group_process for rows of any format (the group's only CS16 and
 * 8-bit entry): shard k reads iq + first_k * stride_elems * element size.  The
 * whole-batch argument check comes first, as there. */
int qpsk_demod_group_process_fmt(qpsk_demod_group *g, int32_t fmt, int32_t mode, const void *iq,
                                 int64_t stride_elems, int64_t n_samples, const int64_t *lengths, int32_t mem,
                                 uint8_t *bits, int64_t bits_stride_bytes, int64_t *n_bits, float *syms,
                                 int64_t syms_stride_floats, int64_t *n_syms);

/* ---------------------------------------------------------------------------
 * Byte framer (DeModulateBytes, QPSKDeModulator.cs:169-259), batched: one
 * framer per stream fed with the packed bits of each process() call.
 */
typedef struct qpsk_framer qpsk_framer;
int qpsk_framer_create(int32_t n_streams, const uint8_t *start_marker, int32_t n_start,
                       const uint8_t *end_marker, int32_t n_end, int64_t ring_capacity,
                       qpsk_framer **out);
int qpsk_framer_destroy(qpsk_framer *f);
/* DeModulateBytes takes its markers per call; change them without touching
 * the framer state. */
int qpsk_framer_set_markers(qpsk_framer *f, const uint8_t *start_marker, int32_t n_start,
                            const uint8_t *end_marker, int32_t n_end);
/* Feed one call's (post-TSC) bits for every stream (host memory); payload[s]
 * receives the completed frame of this call if any (length in n_payload[s],
 * 0 = none), exactly like one DeModulateBytes return value. */
int qpsk_framer_push(qpsk_framer *f, const uint8_t *bits, int64_t bits_stride_bytes,
                     const int64_t *bit_offset, const int64_t *n_bits, uint8_t *payload,
                     int64_t payload_stride, int64_t *n_payload);

/* ---------------------------------------------------------------------------
 * Device-resident framer and TSC search: the same
 * DeModulateBytes state machine (QPSKDeModulator.cs:169-259) and TSC strip
 * (:413-422), one workgroup per stream, fed straight from process()'s device
 * bit rows with no host round trip.  Every pointer below is device memory and
 * every call is ordered on the framer's stream.  The ring is a per-stream
 * linear buffer of ring_capacity bytes (RingClear resets head to 0 and nothing
 * consumes from the tail, so the reference ring never wraps inside a frame);
 * overflow drops the frame and resyncs exactly like RingTryWriteByte (:95-103).
 */
typedef struct qpsk_framer_dev qpsk_framer_dev;
/* ring_capacity <= 0 selects the reference's 300_000_000 bytes per stream (:58). */
int qpsk_framer_dev_create(int32_t n_streams, const uint8_t *start_marker, int32_t n_start,
                           const uint8_t *end_marker, int32_t n_end, int64_t ring_capacity,
                           int32_t device, qpsk_framer_dev **out);
int qpsk_framer_dev_destroy(qpsk_framer_dev *f);
/* Bind to a caller-owned hipStream_t (NULL = library-owned stream). */
int qpsk_framer_dev_set_stream(qpsk_framer_dev *f, void *hip_stream);
/* Per-call markers (DeModulateBytes takes them per call); state is kept. */
int qpsk_framer_dev_set_markers(qpsk_framer_dev *f, const uint8_t *start_marker, int32_t n_start,
                                const uint8_t *end_marker, int32_t n_end);
/* One DeModulateBytes step on every stream: bits rows as qpsk_demod_process
 * wrote them, bit_offset[s] (NULL = 0) = first payload bit after the TSC, or
 * < 0 when this call's TSC search failed (DeModulate returned ""); payload[s]
 * receives the frame completed by this call (first payload_stride bytes) and
 * n_payload[s] its full length (0 = none). */
int qpsk_framer_dev_push(qpsk_framer_dev *f, const uint8_t *bits, int64_t bits_stride_bytes,
                         const int64_t *bit_offset, const int64_t *n_bits, uint8_t *payload,
                         int64_t payload_stride, int64_t *n_payload);
/* Host copy of every stream's framer status (arrays of n_streams, any may be
 * NULL; synchronises the framer's stream): in-frame flag, ring bytes held,
 * start-hunt carry bits. */
int qpsk_framer_dev_status(const qpsk_framer_dev *f, int32_t *in_frame, int64_t *ring_count,
                           int64_t *carry_bits);
/* qpsk_tsc_find for every stream of a device bit batch: offsets[s] = bit index
 * just past the first TSC occurrence in row s, -1 if absent, 0 for a NULL or
 * blank tsc.  Ordered on hip_stream (NULL = the null stream). */
int qpsk_tsc_find_device(const uint8_t *bits, int64_t bits_stride_bytes, const int64_t *n_bits,
                         int32_t n_streams, const char *tsc, int64_t *offsets, void *hip_stream);

/* ---------------------------------------------------------------------------
 * Frames on the device (additive within ABI version 3): the receive loop of
 * the reference calls DeModulateTextUtf8 on each buffer and looks only at the
 * frame that comes back (ModDemodOverSDR.cs:136; DeModulateBytes,
 * QPSKDeModulator.cs:169-259, behind the TSC strip, :412-422).  The three
 * pieces below put that chain behind a qpsk_rx ring, so that a chunk returns
 * the frames it completed and nothing else.
 *
 * qpsk_framer_dev_reset_streams: the framer half of `new QPSKDeModulator(...)`
 * on the listed rows.  One launch writes the construction-time framer state
 * (not in a frame, no lock offset, empty packer, empty ring, no carry bits)
 * into them.  The list is checked first by qpsk_stream_list_check (a bad list
 * changes nothing); the call is ordered on the framer's stream and returns
 * when done.  n = 0 is QPSK_OK and does nothing.
 */
int qpsk_framer_dev_reset_streams(qpsk_framer_dev *f, const int32_t *streams, int32_t n);

/* qpsk_frames_pack_device: the frames of one qpsk_framer_dev_push, packed
 * densely.  Every pointer is device memory; the call is ordered on hip_stream
 * (NULL = the null stream).  payload [n_streams][payload_stride] and n_payload
 * are what qpsk_framer_dev_push wrote; P = payload_stride must be a multiple of
 * 16 and > 0, C = packed_cap a multiple of 16 and >= 0, packed 16-byte
 * aligned (NULL only with C = 0), offsets and head 8-byte aligned; anything
 * else is QPSK_ERR_ARGUMENT and nothing is written.
 *
 * The packing rule, with L_s = n_payload[s]: k_s = min(L_s, P), a_s = k_s
 * rounded up to 16, E_s = the sum of a_t over t < s (int64).  Stream s is
 * stored iff k_s > 0 and E_s + a_s <= C.  offsets[s] = E_s if stored, else -1.
 * A stored frame occupies packed[E_s .. E_s + a_s): its k_s bytes, then zeros.
 * head[0] = the largest E_s + a_s over the stored streams, 0 if none: E_s
 * counts the earlier frames whether stored or not, so once one frame does not
 * fit no later one does, and packed[0 .. head[0]) is dense and fully written.
 * head[1] = QPSK_FRAMES_TRUNCATED if some L_s > P, | QPSK_FRAMES_DROPPED if
 * some frame with k_s > 0 was not stored for lack of capacity.
 */
#define QPSK_FRAMES_TRUNCATED 1
#define QPSK_FRAMES_DROPPED 2
int qpsk_frames_pack_device(const uint8_t *payload, int64_t payload_stride, const int64_t *n_payload,
                            int32_t n_streams, uint8_t *packed, int64_t packed_cap, int64_t *offsets,
                            int64_t *head, void *hip_stream);

/* A framed ring.  qpsk_rx_attach_framer gives the ring a device framer of its
 * own (qpsk_framer_dev_create's markers and ring_capacity, bound to the ring's
 * download stream); allowed once per ring and only with no chunk outstanding,
 * else QPSK_ERR_STATE.  tsc as in qpsk_tsc_find_device (NULL or blank = none).
 * Entering a frame appends the rest of the chunk's bits to the framer's ring
 * (QPSKDeModulator.cs:203-220), so a ring_capacity below one chunk's bit bytes
 * drops every frame, as the reference does at that FrameBuffer size.
 * max_frame_bytes (> 0, rounded up to 16) is the bytes of a frame the ring
 * returns; chunk_frame_bytes (rounded up to 16; 0 = n_streams *
 * max_frame_bytes) the bytes of frames one chunk can return, as
 * qpsk_rx_frames_bytes reports it (0 for a ring without a framer).  From then
 * on every submit queues, behind the chunk's DeModulate and on the download
 * stream: qpsk_tsc_find_device, qpsk_framer_dev_push, qpsk_frames_pack_device,
 * the download of the index (lengths, offsets, head) and, only with keep_bits
 * != 0, the download of the bits.  Chunk k + 1's framer step follows chunk
 * k's, the order DeModulateBytes needs.  A ring without a framer is what it
 * was.
 *
 * qpsk_rx_collect_frames waits for the oldest outstanding chunk, fetches
 * exactly head[0] packed bytes (on a stream of its own, which never waits for
 * a later chunk) and fills: frame_len[s] = the length of the array
 * DeModulateBytes returned for this buffer on stream s (0 = none, as in
 * qpsk_framer_dev_push); frame_offset[s] = the offset in `frames` of its first
 * byte, a multiple of 16, or -1 (no frame, or dropped); min(frame_len[s],
 * max_frame_bytes) bytes are present.  A buffer of qpsk_rx_frames_bytes bytes
 * always suffices; frames_cap smaller than head[0] is QPSK_ERR_ARGUMENT and
 * the chunk stays outstanding.  bits / n_bits (as in qpsk_rx_collect) may both
 * be NULL; non-NULL on a keep_bits = 0 ring is QPSK_ERR_STATE.  When head[1]
 * != 0 (a frame truncated or dropped) it returns QPSK_ERR_CAPACITY with the
 * outputs written and the chunk consumed, as the host process calls do.  A
 * rejected call neither waits nor fetches (frames_cap alone is known only
 * after the wait).  QPSK_ERR_STATE on a ring without a framer.
 *
 * qpsk_rx_collect on a framed ring: with keep_bits it works as before (the
 * chunk's frames are dropped; the framer state has advanced); with keep_bits
 * = 0 it returns QPSK_ERR_STATE.
 *
 * qpsk_rx_set_markers: markers are per-call arguments of DeModulateBytes; the
 * new pair applies to later submits.  It waits for the framer work already
 * queued.  qpsk_rx_reset_streams: `new QPSKDeModulator(...)` on the listed
 * rows of the ring, between submits: it waits for the outstanding chunks'
 * framer work, then qpsk_demod_reset_streams on the handle and
 * qpsk_framer_dev_reset_streams on the framer (the handle alone on a ring
 * without a framer).  A bad list changes neither; n = 0 does nothing.
 * qpsk_rx_destroy also destroys the framer.
 */
int qpsk_rx_attach_framer(qpsk_rx *r, const uint8_t *start, int32_t n_start, const uint8_t *end, int32_t n_end,
                          const char *tsc, int64_t ring_capacity, int64_t max_frame_bytes,
                          int64_t chunk_frame_bytes, int32_t keep_bits);
int qpsk_rx_set_markers(qpsk_rx *r, const uint8_t *start, int32_t n_start, const uint8_t *end, int32_t n_end);
int64_t qpsk_rx_frames_bytes(const qpsk_rx *r);
int qpsk_rx_collect_frames(qpsk_rx *r, uint8_t *frames, int64_t frames_cap, int64_t *frame_offset,
                           int64_t *frame_len, uint8_t *bits, int64_t bits_stride_bytes, int64_t *n_bits,
                           int64_t *ticket);
int qpsk_rx_reset_streams(qpsk_rx *r, const int32_t *streams, int32_t n);

/* ---------------------------------------------------------------------------
 * Synthetic batched input (QPSKModulator.Modulate + the test bench channel),
 * generated in device memory.  Stream s draws its payload from
 * splitmix64(seed ^ s); tx_bits receives the payload bits (packed MSB-first).
 * cfo_hz: per-stream carrier offset drawn U[-cfo_hz, +cfo_hz] (0 = clean
 * ±ppm LO pair), multipath: 4-tap channel [1, .25e^{j.7}, .1e^{-j1.9}, .05],
 * esn0_db: AWGN Es/N0 (>= 200 = none).  lo_ppm = cfo_hz = 0: no carrier at
 * all, i.e. QPSKModulator.Modulate's own baseband (QPSKModulator.cs:104-167).
 */
typedef struct qpsk_synth_params {
    int32_t sample_rate, symbol_rate;
    double rrc_alpha;
    int32_t rrc_span;
    int32_t differential;
    uint64_t seed;
    double lo_ppm;
    double cfo_hz;
    int32_t multipath;
    double esn0_db;
    int64_t first_stream;       /* global id of row 0: a rank's shard draws the same
                                   streams whatever the sharding */
    int32_t reserved[6];
} qpsk_synth_params;
void qpsk_synth_params_init(qpsk_synth_params *p, int32_t sample_rate, int32_t symbol_rate);
int qpsk_synth_generate(const qpsk_synth_params *p, int32_t device, void *hip_stream,
                        int32_t n_streams, int64_t n_samples, float *iq_dev,
                        int64_t stride_floats, uint8_t *tx_bits_dev, int64_t bits_stride_bytes);

/* ---------------------------------------------------------------------------
 * QPSKModulator (QPSKModulator.cs:18-167) behind the same ABI, batched: one
 * handle = one constructor (RRC taps, TSC, differential flag), one call =
 * Modulate (or ModulateBytes) on S independent bit strings, computed on the
 * GPU.  The impulse train (symbol d at delay + d*sps, delay = (T-1)/2) is
 * filtered by the float RRC taps in double and rounded to float, i.e.
 * fftFilter's output (FIRFilter.cs:96-141) restated as direct convolution;
 * output length = delay + nDibits*sps (+ delay when pulse shaping).
 * ModulateTextUtf8 (:74-89) is ModulateBytes on Encoding.GetBytes results and
 * stays in the C# shim.
 */
typedef struct qpsk_mod_params {
    int32_t sample_rate;        /* int SampleRate                 */
    int32_t symbol_rate;        /* int SymbolRate                 */
    double rrc_alpha;           /* double RrcAlpha = 0.9          */
    int32_t rrc_span;           /* int rrcSpan = 6                */
    int32_t differential;       /* bool differentialEncoding = true */
    int32_t device;             /* HIP device ordinal             */
    int32_t reserved[7];
} qpsk_mod_params;
typedef struct qpsk_mod qpsk_mod;
void qpsk_mod_params_init(qpsk_mod_params *p, int32_t sample_rate, int32_t symbol_rate);
/* new QPSKModulator(..., tsc): tsc is a '0'/'1' string prepended to every
 * Modulate call's data (NULL or blank = none, string.IsNullOrWhiteSpace). */
int qpsk_mod_create(const qpsk_mod_params *p, const char *tsc, qpsk_mod **out);
int qpsk_mod_destroy(qpsk_mod *m);
int qpsk_mod_set_stream(qpsk_mod *m, void *hip_stream);
/* floats one row of Modulate output holds for n_bits payload bits */
int64_t qpsk_mod_output_floats(const qpsk_mod *m, int64_t n_bits, int32_t pulse_shaping);
/* Modulate(string data, bool pulseShaping) on every stream: bits [S][stride]
 * packed MSB-first (bit i of the string = bit 7 - i%8 of byte i/8), n_bits[s]
 * bits each (an odd count drops the last bit, :113); out [S][out_stride]
 * interleaved float, n_out_floats[s] = its length (0 for < 2 bits in all).
 * mem applies to bits, n_bits, out and n_out_floats. */
int qpsk_mod_modulate(qpsk_mod *m, int32_t n_streams, const uint8_t *bits, int64_t bits_stride_bytes,
                      const int64_t *n_bits, int32_t pulse_shaping, int32_t mem, float *out,
                      int64_t out_stride_floats, int64_t *n_out_floats);
/* ModulateBytes(payload, startMarker, endMarker, pulseShaping) (:54-72) on every
 * stream, host memory: payload [S][payload_stride] bytes, n_payload[s] each.
 * Empty markers are QPSK_ERR_ARGUMENT (ArgumentException, :60-61). */
int qpsk_mod_modulate_bytes(qpsk_mod *m, int32_t n_streams, const uint8_t *payload, int64_t payload_stride,
                            const int64_t *n_payload, const uint8_t *start_marker, int32_t n_start,
                            const uint8_t *end_marker, int32_t n_end, int32_t pulse_shaping, float *out,
                            int64_t out_stride_floats, int64_t *n_out_floats);

/* ---------------------------------------------------------------------------
 * The modulator's output in a radio's own sample format.  The transmit half of
 * the reference program (ModDemodOverSDR.cs:87-111: ModulateTextUtf8, then
 * txStream.Write) hands the driver floats; a device that takes CS16 or CS8
 * wants integers, and the reference's own integer writer is SaveAsCs16
 * (HelperFunctions.cs:75-106).  x is a float component of the modulator's
 * output; full = 32767 (CS16) or 127 (CS8, CU8); [lo, hi] = [-32768, 32767]
 * or [-128, 127].
 *
 *   QPSK_MOD_NORM_FIXED  v = x * scale, one float multiply rounded once;
 *       clamp v to [lo, hi] (+-inf saturate); truncate toward zero: the
 *       reference's (short)Math.Max(short.MinValue, Math.Min(short.MaxValue,
 *       ...)) (HelperFunctions.cs:97-101).  CU8 stores the CS8 value + 128.
 *       CF32 stores v itself, so scale 1.0f gives the bits of
 *       qpsk_mod_modulate.  scale must be finite and > 0, else
 *       QPSK_ERR_OUT_OF_RANGE.  peak may be NULL and is not written.
 *   QPSK_MOD_NORM_PEAK   SaveAsCs16 per row, in double as there:
 *       (double)x / maxVal * (double)full, a division and then a
 *       multiplication (:97-98), clamped and truncated as above.  maxVal is
 *       the largest |component| of the row's whole output (:82-86), replaced
 *       by 1.0 when < 1e-12 (:88), so the peak sample stores exactly +-full.
 *       scale is ignored.  peak[s] (required) receives the row's largest
 *       |component| as found, a float: 0 for an empty row.  With
 *       QPSK_FMT_CF32 it is QPSK_ERR_ARGUMENT.
 *
 * qpsk_quantise_iq applies the rules to one row of n_floats host floats (needs
 * no device); the modulator's kernels share its arithmetic
 * (csrc/qpsk_quantise.h) and equal it element for element.  A rejected call
 * writes nothing.
 */
#define QPSK_MOD_NORM_FIXED 0
#define QPSK_MOD_NORM_PEAK 1
int qpsk_quantise_iq(int32_t fmt, int32_t norm, float scale, const float *iq, int64_t n_floats, void *out,
                     float *peak);
/* Output samples one workgroup of the sample kernel covers, and dibits one
 * pass of the symbol kernel's scan covers: the row lengths at which the
 * kernels change blocks (tests/test_gpu_mod_fmt.py spans them). */
#define QPSK_MOD_TILE_SAMPLES 512
#define QPSK_MOD_SCAN_DIBITS 1024
/* qpsk_mod_modulate / qpsk_mod_modulate_bytes with the output in fmt
 * (QPSK_FMT_*; unknown: QPSK_ERR_ARGUMENT): out is [n_streams][out_stride_elems]
 * floats, int16 or bytes, n_out_elems[s] = 2 x the row's complex samples (what
 * qpsk_mod_output_floats returns, the same in every format).  mem covers bits /
 * payload, their counts, out, n_out_elems and peak; markers are always host
 * memory.  With QPSK_MEM_DEVICE the payload rows of _bytes_fmt stay where they
 * are: the symbol kernel reads TSC, START, payload and END by index
 * (QPSKModulator.cs:54-72, :112-126), no framed copy is built.
 * Device output rows: out aligned to one complex sample (8 / 4 / 2 / 2 bytes),
 * out_stride_elems even and >= the longest row, else QPSK_ERR_ARGUMENT before
 * anything is launched.  Rows 16-byte aligned with a stride of a multiple of 16
 * bytes are written 16 bytes a store (the wide-load condition of
 * qpsk_demod_process_fmt, which can take them as they are), other rows one
 * sample a store; the values are the same.  Elements past n_out_elems[s] of a
 * device row are not written; what lies there in a host row is unspecified.
 * n_streams above 65535 (the grid dimension the streams run on) is
 * QPSK_ERR_ARGUMENT. */
int qpsk_mod_modulate_fmt(qpsk_mod *m, int32_t fmt, int32_t norm, float scale, int32_t n_streams,
                          const uint8_t *bits, int64_t bits_stride_bytes, const int64_t *n_bits,
                          int32_t pulse_shaping, int32_t mem, void *out, int64_t out_stride_elems,
                          int64_t *n_out_elems, float *peak);
int qpsk_mod_modulate_bytes_fmt(qpsk_mod *m, int32_t fmt, int32_t norm, float scale, int32_t n_streams,
                                const uint8_t *payload, int64_t payload_stride, const int64_t *n_payload,
                                const uint8_t *start_marker, int32_t n_start,
                                const uint8_t *end_marker, int32_t n_end, int32_t pulse_shaping,
                                int32_t mem, void *out, int64_t out_stride_elems,
                                int64_t *n_out_elems, float *peak);

/* ---------------------------------------------------------------------------
 * Bit errors, counted where the bits are.  (Added within ABI version 3: no
 * existing entry point, kernel or layout changed.)
 *
 * The reference's test bench compares what it received with what it sent
 * (testAtDataLevel.cs:44-46) around a modulator, an impaired channel and a
 * demodulator driven in a loop (testFullDemodChain.cs).  For packed bit rows
 * the comparison has to find where in the sent bits a received stretch lies:
 * the differential decoder drops the first dibit and a symbol slip of the
 * timing loop moves the offset by 2 bits.  The definition below is the one the
 * project reports as "BER after lock" (bench.py, ber_after_lock), restated for
 * one stream s.
 *
 * rx(j) and ref(j) are bit j of the stream's rx_bits and ref_bits rows, packed
 * MSB-first (bit 7 - j % 8 of byte j / 8) like every bit row of this ABI.
 * R = n_rx_bits[s], N = n_ref_bits[s]; w0 = skip_bits, W = window, K =
 * key_bits, D = search.  find(w, lo, hi) is the smallest i with lo <= i,
 * i + K <= hi and ref(i + t) == rx(w + t) for all t < K, or -1 if there is
 * none (an empty or inverted range gives -1).
 *
 *     located = 0; errs = bits = lost = slips = windows = 0
 *     for (w = w0; w + W <= R; w += W):
 *         windows += 1
 *         i = located ? find(w, max(0, w + off - D), min(N, w + off + D + K))
 *                     : find(w, 0,                   min(N, w + 4 * W))
 *         if i < 0: lost += 1; continue               (off and located stay)
 *         if located and i - w != off: slips += 1
 *         located = 1; off = i - w
 *         m = min(W, N - i)                           (>= K: the key lies inside ref)
 *         e = #{ t < m : rx(w + t) != ref(i + t) }
 *         tail_ok = rx[w + m - K, w + m) == ref[i + m - K, i + m)
 *         if !tail_ok or e > m / 8 (integer division): lost += 1
 *         else: errs += e; bits += m
 *
 * All positions are int64 and off may be negative.  A row with R < w0 + W
 * yields a row of zeros, for every w0 up to INT64_MAX (the loop condition is
 * evaluated as w <= R - W).  The first match is part of the definition: on
 * low-entropy data the key occurs before the place a human would pick, and the
 * counts say so.  A window that cannot be located (an error or a slip inside
 * its key) or whose last K bits no longer line up (a slip inside it) or that
 * holds more than one error in 8 bits is a lost window, not bit errors.
 *
 * Known cost, by the definition: a row that never locates scans up to
 * min(N, w + 4 W) positions in every window.
 */
typedef struct qpsk_ber_params {
    int64_t skip_bits;      /* w0: bits of every rx row left out (acquisition), >= 0        */
    int32_t window;         /* W: bits per window, key_bits .. 2^20                         */
    int32_t key_bits;       /* K: leading bits of a window located in ref, 1 .. 64          */
    int32_t search;         /* D: positions searched either side of the last offset, 0 .. 2^20 */
    int32_t reserved[3];
} qpsk_ber_params;
/* 8000, 2048, 64, 512: the values bench.py reports with; reserved = 0. */
void qpsk_ber_params_init(qpsk_ber_params *p);
typedef struct qpsk_ber_row {         /* 64 bytes, no padding */
    int64_t bit_errors;     /* errs                                                         */
    int64_t bits;           /* bits compared in the windows that count                      */
    int64_t lost_windows;   /* lost                                                         */
    int64_t slips;          /* windows located at another offset than the one before        */
    int64_t windows;        /* windows looked at: max(0, (R - w0) / W)                      */
    int64_t last_offset;    /* off after the last window; 0 while located == 0              */
    int32_t located;        /* 1 once a window has been located                             */
    int32_t reserved[3];    /* written as 0                                                 */
} qpsk_ber_row;
/* sizeof(qpsk_ber_row) = 64, as qpsk_link_stats_size; needs no device. */
int qpsk_ber_row_size(void);
/*
 * qpsk_ber_count: every pointer is host memory, no device is needed; out[s]
 * receives stream s's row.  qpsk_ber_count_device: every pointer but p is
 * device memory, the counting kernel is ordered on hip_stream (NULL = the null
 * stream) and the call returns without waiting for it; out_dev[s] is complete
 * once hip_stream has run it.  The rows the device form writes equal the host
 * form's byte for byte.
 *
 * Checked on the host before anything is launched or written, for every
 * n_streams: a null pointer is QPSK_ERR_ARGUMENT_NULL; n_streams < 0, a
 * negative stride or (device form) out_dev not 8-byte aligned is
 * QPSK_ERR_ARGUMENT; skip_bits < 0, key_bits outside [1, 64], window outside
 * [key_bits, 2^20] or search outside [0, 2^20] is QPSK_ERR_OUT_OF_RANGE.
 * n_streams == 0 is then QPSK_OK and does nothing.  The host form also
 * refuses a count n_rx_bits[s] or n_ref_bits[s] that is negative, larger
 * than 8 * its stride or not below 2^61 with QPSK_ERR_ARGUMENT, and writes
 * nothing.  The device
 * form cannot see the counts: its kernel treats such a row as R = 0 or N = 0
 * respectively (a row of zeros, or one whose windows are all lost).
 *
 * Bit rows may have any byte alignment and any stride (row s starts at
 * s * stride bytes).  Bits at or past n_*_bits[s] are never interpreted, the
 * rest of the last byte included, and no byte at or past ceil(n / 8) of a row
 * is read.
 */
int qpsk_ber_count(const qpsk_ber_params *p, const uint8_t *rx_bits, int64_t rx_stride_bytes,
                   const int64_t *n_rx_bits, const uint8_t *ref_bits, int64_t ref_stride_bytes,
                   const int64_t *n_ref_bits, int32_t n_streams, qpsk_ber_row *out);
int qpsk_ber_count_device(const qpsk_ber_params *p, const uint8_t *rx_bits, int64_t rx_stride_bytes,
                          const int64_t *n_rx_bits, const uint8_t *ref_bits, int64_t ref_stride_bytes,
                          const int64_t *n_ref_bits, int32_t n_streams, qpsk_ber_row *out_dev,
                          void *hip_stream);

/* ---------------------------------------------------------------------------
 * The test bench's channel on the device: the LO pair and the noise, batched.
 * (Added within ABI version 3: no existing entry point, kernel or layout
 * changed.)
 *
 * The reference's end-to-end test (testAtDataLevel.cs:24-46) multiplies every
 * sample of ModulateTextUtf8's output by
 * txNCO.NextSample() * rxNCO.NextSample().Conjugate() before DeModulateTextUtf8;
 * testFullDemodChain.cs:59-73 adds NoiseGenerator.GenerateIqNoise's samples
 * ahead of the same LO pair.  One handle is that channel for S independent
 * streams; one call takes rows where the modulator leaves them and leaves
 * rows the demodulator takes.
 *
 * LO pair.  Each stream has two oscillators, each LocalOscilator.cs:5-194:
 *   construction (:20-60)   max = |ppm|; static = max > 0 ? (u * 2 - 1) * max : 0
 *                           (one draw); drift = 0; total = static;
 *                           cur_hz = lo_hz * (1 + total * 1e-6); phase = wrap(phase0);
 *                           interval = max(1, (int)(sample_rate * 1e-3)); counter = 0
 *   NextSample (:150-194)   max > 0: every interval-th call draws
 *                           step = (u * 2 - 1) * (max * 0.001); drift += step;
 *                           total = static + drift, clamped to +-max (drift =
 *                           total - static then); cur_hz as above.
 *                           phase = wrap(phase + 2 pi cur_hz / sample_rate);
 *                           the sample is (cos phase, sin phase), glibc's double
 *                           cos and sin.  max = 0: cur_hz = lo_hz, no draws.
 *   wrap(x)                 fmod(x, 2 pi), + 2 pi if that is negative
 *   u                       splitmix64: (z >> 11) * 2^-53
 * Stream g = first_stream + row seeds its transmit oscillator with tx_seed + g
 * and its receive oscillator with rx_seed + g.  With a = tx sample, b =
 * conj(rx sample), x the input sample, all double, System.Numerics.Complex's
 * product and no contraction (testAtDataLevel.cs:39-42):
 *   l = (a.re b.re - a.im b.im, a.im b.re + a.re b.im)
 *   y = (x.re l.re - x.im l.im, x.im l.re + x.re l.im), each rounded to float once.
 *
 * Noise (noise_rms > 0; HelperModels.cs:17-45 with linearRms = noise_rms).  For
 * the sample at the stream's absolute position pos (samples the stream has
 * taken since its construction or reset, kept in its state):
 *   h = noise_seed ^ (g << 40) ^ pos ^ 0xA5A5A5A5; u1 = 1 - u(h); u2 = 1 - u(h)
 *   mag = sqrt(-2 log(u1)) * noise_rms; ph = 2 pi u2
 *   n = ((float)(mag cos ph), (float)(mag sin ph)), each clamped to [-1, 1]
 *   x = (x.re + (double)n.re, x.im + (double)n.im) ahead of the product above
 *   (testFullDemodChain.cs:73)
 * cos and sin are glibc's, sqrt is correctly rounded, log is the device
 * library's (the one operation of the channel that is not pinned bit for bit).
 * The draw depends on pos alone, so the noise does not depend on how calls cut
 * a stream.
 *
 * Formats.  An input sample's value is what qpsk_demod_process_fmt reads:
 * CF32 as it stands (scale_in is ignored), (float)x * scale_in for CS16 and CS8,
 * (float)((int)x - 128) * scale_in for CU8.  The float result y goes through
 * QPSK_MOD_NORM_FIXED of qpsk_quantise_iq with scale_out: CF32 stores
 * y * scale_out (1.0f: y itself), an integer row equals qpsk_quantise_iq of the
 * CF32 row.  Per-row peak normalisation needs a second pass over the row and
 * is not offered: norm_out other than QPSK_MOD_NORM_FIXED is
 * QPSK_ERR_ARGUMENT.  Not modelled: multipath, a sample-clock offset.
 */
typedef struct qpsk_channel_params {
    double sample_rate;         /* NCO sampleRate (LocalOscilator.cs:20), > 0             */
    double lo_hz;               /* NCO frequencyHz of both LOs: 100e6 (testAtDataLevel.cs:27-28) */
    double tx_ppm, rx_ppm;      /* NCO ppmError: 1 and 1 (:27-28); the sign is dropped (:30) */
    double tx_phase0, rx_phase0;/* NCO initialPhase: 0                                    */
    uint64_t tx_seed, rx_seed;  /* stream g draws from tx_seed + g and rx_seed + g        */
    double noise_rms;           /* linearRms of GenerateIqNoise; 0 = no noise             */
    uint64_t noise_seed;
    int64_t first_stream;       /* global id of row 0: a shard equals rows first_stream.. of the batch */
    int32_t device;             /* HIP device ordinal                                     */
    int32_t reserved[7];
} qpsk_channel_params;
typedef struct qpsk_channel qpsk_channel;
/* lo_hz = 100e6, tx_ppm = rx_ppm = 1, phases 0, tx_seed = 1000, rx_seed = 2000,
 * noise_rms = 0, noise_seed = 0, first_stream = 0, device = 0, reserved = 0. */
void qpsk_channel_params_init(qpsk_channel_params *p, double sample_rate);
/* new NCO(lo_hz, sample_rate, ppm, phase0) twice per stream, pos = 0.
 * sample_rate not finite or <= 0, a non-finite lo_hz, ppm or phase0, noise_rms
 * not finite or < 0, or first_stream < 0: QPSK_ERR_OUT_OF_RANGE; n_streams <
 * 1: QPSK_ERR_ARGUMENT; all before a device is touched. */
int qpsk_channel_create(const qpsk_channel_params *p, int32_t n_streams, qpsk_channel **out);
int qpsk_channel_destroy(qpsk_channel *ch);
/* Calls are ordered on the handle's stream: its own, or the caller's
 * (NULL = back to an own one), as qpsk_mod_set_stream. */
int qpsk_channel_set_stream(qpsk_channel *ch, void *hip_stream);
/* One call: stream s takes lengths[s] samples (lengths == NULL: n_samples for
 * all; lengths is host memory, each 0 .. n_samples) from row s of in,
 * [n_streams][stride_in] elements of fmt_in, and writes as many to row s of
 * out, [n_streams][stride_out] elements of fmt_out; strides count elements
 * (two per sample) and must hold 2 * n_samples.  Elements past a row's length
 * are not written.  mem covers in and out.  out == in is allowed when fmt_out
 * == fmt_in and the strides are equal (the reference works in place); rows
 * that overlap in any other way are undefined.  Device rows follow the rules
 * of qpsk_demod_process_fmt: an even stride, CS16 rows 4-byte and 8-bit rows
 * 2-byte aligned, CF32 rows 4-byte aligned (rows not 8-byte aligned are read
 * and written one float at a time), else QPSK_ERR_ARGUMENT.  scale_out, and
 * scale_in of an integer format, must be finite and > 0, else
 * QPSK_ERR_OUT_OF_RANGE.  A rejected call changes neither the state nor out.
 * A device call without lengths is queued on the handle's stream and returns;
 * a call with lengths or with host rows returns when it has run.  The
 * caller's current device is the same on return. */
int qpsk_channel_apply_fmt(qpsk_channel *ch, int32_t fmt_in, const void *in, int64_t stride_in, float scale_in,
                           int32_t fmt_out, int32_t norm_out, void *out, int64_t stride_out, float scale_out,
                           int64_t n_samples, const int64_t *lengths, int32_t mem);
/* State: per stream 128 bytes, no header,
 *   two oscillators (tx, rx) of 56 bytes: double static_ppm, drift_ppm,
 *   total_ppm, cur_hz, phase; int64 counter; uint64 rng
 *   int64 pos; 8 reserved bytes (0)
 * qpsk_channel_state_size() = 128, needs no device.  get_state / set_state move
 * all n_streams records (buf_bytes = 128 * n_streams, host memory) behind the
 * calls queued so far.  set_state runs qpsk_channel_state_check first and
 * changes nothing when it fails. */
int qpsk_channel_state_size(void);
int qpsk_channel_get_state(qpsk_channel *ch, void *host_buf, int64_t buf_bytes);
int qpsk_channel_set_state(qpsk_channel *ch, const void *host_buf, int64_t buf_bytes);
/* new NCO(...) twice and pos = 0 for the listed rows (a list as
 * qpsk_stream_list_check accepts it); the other rows are untouched. */
int qpsk_channel_reset_streams(qpsk_channel *ch, const int32_t *streams, int32_t n);
/* What a state must satisfy for handle parameters p (host only, no device):
 * buf_bytes = 128 * n_streams; per oscillator every double finite, |static_ppm|
 * and |total_ppm| <= |ppm|, total_ppm = static_ppm + drift_ppm to within the
 * two roundings the clamp leaves (2^-50 |ppm|), cur_hz = lo_hz * (1 + total_ppm
 * * 1e-6) exactly, phase in [0, 2 pi] (-0 included: fmod's remainder of a negative
 * multiple of 2 pi; wrap's "+ 2 pi" rounds a tiny negative remainder to 2 pi
 * itself), counter in [0, interval); pos >= 0; reserved = 0.
 * A failure is QPSK_ERR_ARGUMENT and names stream, oscillator and field in
 * qpsk_last_error. */
int qpsk_channel_state_check(const qpsk_channel_params *p, int32_t n_streams, const void *buf, int64_t buf_bytes);
/* Streams one workgroup of the channel kernel holds and samples one block of
 * its phase scan covers: the batch sizes and call lengths at which the kernel
 * changes tiles (tests/test_gpu_channel.py spans them). */
#define QPSK_CHANNEL_TILE_STREAMS 16
#define QPSK_CHANNEL_BLOCK_SAMPLES 64

/* ---------------------------------------------------------------------------
 * The propagation path on the device: multipath taps and a sample-clock
 * offset, batched.  (Added within ABI version 3: no existing entry point,
 * kernel or layout changed.)
 *
 * What the channel above leaves out.  The test bench chain is modulator ->
 * path -> channel -> demodulator, every hop on rows of any QPSK_FMT_*.  One
 * call takes n_in samples a stream, passes them through the stream's
 * multipath taps, resamples the result onto the receiver's sample clock and
 * writes the samples that are now computable; it reports how many that was
 * for each stream.  Nothing contracts to an FMA.
 *
 * Clock.  Stream g = first_stream + row draws u1, u2, the first and second
 * draws of splitmix64 seeded with clock_seed + g, u = (z >> 11) * 2^-53 (as
 * the channel's oscillators draw):
 *   ppm = clock_ppm + (clock_spread > 0 ? (u1 * 2 - 1) * clock_spread : 0)
 *   r   = 1.0 + ppm * 1e-6        input samples per output sample; ppm > 0 is
 *                                 a slow receiver clock.  Constant: no drift.
 *   tau = tau_random ? u2 : tau0  the position of output 0, in [0, 1)
 *
 * Multipath.  A stream has L complex float taps h[0..L-1], 1 <= L <= 8.  With
 * x[i] the widened input sample at the stream's absolute index i and x[i] = +0
 * for i < 0, all float, one rounding an operation:
 *   z[i].re = acc, acc = +0.0f, then for j = 0 .. L-1 in order
 *             acc = acc + (h[j].re * x[i-j].re - h[j].im * x[i-j].im)
 *   z[i].im   likewise with (h[j].re * x[i-j].im + h[j].im * x[i-j].re)
 * multipath = 0: L = 1, h = [(1, 0)].  multipath = 1: the project's four taps
 * [1, .25 e^{j.7}, .1 e^{-j1.9}, .05] (qpsk_synth_generate's), formed in double
 * and rounded to float once.
 *
 * Resampler.  Output k, the stream's absolute output index from 0, sits at
 *   p_k = tau + (double)k * r     (two double roundings, closed form: the
 *                                 result does not depend on how calls cut the
 *                                 stream)
 *   n = floor(p_k) as int64, mu = p_k - (double)n, t = (float)mu
 * and its value is MuellerMuller.CubicLagrange4 (MuellerMuller.cs:160-190) on
 * z[n-1], z[n], z[n+1], z[n+2], in float, I and Q separately:
 *   tm1 = t - 1, tm2 = t - 2, tp1 = t + 1
 *   c_m1 = -(t * tm1 * tm2) * (1f / 6f)     c_0 = (tp1 * tm1 * tm2) * (1f / 2f)
 *   c_1 = -(tp1 * t * tm2) * (1f / 2f)      c_2 = (tp1 * t * tm1) * (1f / 6f)
 *   y = c_m1 * z[n-1] + c_0 * z[n] + c_1 * z[n+1] + c_2 * z[n+2], left to right
 * The position is double at every k: at k = 2^40 the ulp of p_k is 2^-12
 * sample, which is the resolution of mu there.  Input positions are held to
 * 2^50 (output positions then stay below 2^51).
 *
 * What a call emits.  After a call the stream has taken inputs 0 .. in_end-1;
 * the call emits every not yet emitted k with floor(p_k) <= in_end - 3 (the
 * interpolator looks two samples ahead: the first call of N samples at r = 1,
 * tau = 0 emits N - 2).  There is no flush: append zeros for the tail.
 * With L = 1, h = (1, 0), r = 1, tau = 0 a finite row comes back bit for bit,
 * two samples short, except that -0 becomes +0.
 *
 * Formats as the channel's: input values as qpsk_demod_process_fmt reads them
 * (scale_in; CU8 zero at 128), the float result through QPSK_MOD_NORM_FIXED of
 * qpsk_quantise_iq with scale_out; QPSK_MOD_NORM_PEAK is QPSK_ERR_ARGUMENT.
 * Not modelled: a time-varying r (clock drift), fractional-delay taps. */
typedef struct qpsk_path_params {
    double clock_ppm;           /* sample-clock offset of every stream, ppm: 0            */
    double clock_spread;        /* + uniform(-spread, spread) per stream, ppm, >= 0: 0    */
    uint64_t clock_seed;        /* stream g draws from clock_seed + g: 3000               */
    double tau0;                /* position of output 0 when tau_random = 0, [0, 1): 0    */
    int32_t tau_random;         /* 1: tau = the stream's second draw                      */
    int32_t multipath;          /* 0: one unit tap; 1: the project's four taps            */
    int64_t first_stream;       /* global id of row 0                                     */
    int32_t device;             /* HIP device ordinal                                     */
    int32_t reserved[7];
} qpsk_path_params;
typedef struct qpsk_path qpsk_path;
#define QPSK_PATH_MAX_TAPS 8
#define QPSK_PATH_HIST 16
#define QPSK_PATH_MAX_PPM 1000.0
/* The outputs one workgroup of the path kernel covers: the per-call output
 * counts at which the kernel changes tiles (tests/test_gpu_path.py spans them). */
#define QPSK_PATH_TILE_OUTPUTS 1024
/* All 0 but clock_seed = 3000. */
void qpsk_path_params_init(qpsk_path_params *p);
/* |clock_ppm| + clock_spread > 1000, clock_spread < 0, tau0 outside [0, 1), any
 * of them not finite, or first_stream < 0: QPSK_ERR_OUT_OF_RANGE; n_streams < 1:
 * QPSK_ERR_ARGUMENT; all before a device is touched. */
int qpsk_path_create(const qpsk_path_params *p, int32_t n_streams, qpsk_path **out);
int qpsk_path_destroy(qpsk_path *pa);
/* As qpsk_channel_set_stream. */
int qpsk_path_set_stream(qpsk_path *pa, void *hip_stream);
/* Replaces the taps: taps_iq is host memory, [2 * n_taps] floats (re, im) for
 * all streams or [n_streams][2 * n_taps] when per_stream != 0; n_taps in 1..8,
 * else QPSK_ERR_ARGUMENT; a non-finite tap is QPSK_ERR_OUT_OF_RANGE.  Takes
 * effect behind the calls queued so far; the history is kept. */
int qpsk_path_set_taps(qpsk_path *pa, const float *taps_iq, int32_t n_taps, int32_t per_stream);
/* One call: stream s takes lengths[s] samples (lengths == NULL: n_samples for
 * all; host memory, each 0 .. n_samples) from row s of in, [n_streams][stride_in]
 * elements of fmt_in, and writes n_out[s] samples to row s of out,
 * [n_streams][stride_out] elements of fmt_out, stride_out >= 2 * out_cap.
 * n_out is host memory, [n_streams], and is filled before the call returns even
 * when the device work is only queued: the counts are a function of the call
 * lengths and each stream's (r, tau) alone, and the handle keeps every stream's
 * positions on the host.  A stream that would emit more than out_cap samples
 * makes the call QPSK_ERR_ARGUMENT (qpsk_path_out_bound gives a capacity that
 * always suffices).  out must not overlap in (the lengths differ: there is no
 * in-place form; the test is on the two buffers' whole extents, first row to
 * last), else QPSK_ERR_ARGUMENT.  Device rows, scales, norm_out, mem,
 * queueing and the return follow qpsk_channel_apply_fmt: a device call without
 * lengths is queued on the handle's stream and returns; rows 16-byte aligned
 * with a pitch that is a multiple of 16 bytes are read with 16-byte loads.
 * Elements past a row's n_out are not written.  A rejected call changes neither
 * the state nor out.  The caller's current device is the same on return. */
int qpsk_path_apply_fmt(qpsk_path *pa, int32_t fmt_in, const void *in, int64_t stride_in, float scale_in,
                        int32_t fmt_out, int32_t norm_out, void *out, int64_t stride_out, int64_t out_cap,
                        float scale_out, int64_t n_samples, const int64_t *lengths, int64_t *n_out, int32_t mem);
/* Host only, no device.  The capacity that is enough for any call of n_in
 * samples on a handle made from p: ceil(n_in / (1 - (|clock_ppm| +
 * clock_spread) * 1e-6)) + 2; negative (an error code) for bad arguments. */
int64_t qpsk_path_out_bound(const qpsk_path_params *p, int64_t n_in);
/* Host only.  How many outputs a stream at (r, tau) that has emitted out_pos
 * emits once it has taken in_end inputs: the k >= out_pos with floor(p_k) <=
 * in_end - 3, from a division and a correction by that predicate (no loop over
 * samples).  Negative (an error code) when r is not within 1000 ppm of 1, tau
 * not in [0, 1), in_end outside [0, 2^50] or out_pos outside [0, 2^51]. */
int64_t qpsk_path_count(double r, double tau, int64_t out_pos, int64_t in_end);
/* State: per stream 256 bytes, no header,
 *   double r, tau; int64 in_pos, out_pos; int32 n_taps; float taps[8][2];
 *   float hist[16][2]; 28 reserved bytes (0)
 * hist holds the widened inputs at indices in_pos-16 .. in_pos-1 (the last
 * L - 1 + 3 <= 10 samples the next call can still need, rounded up); entries
 * at negative indices are +0.  qpsk_path_state_size() = 256 and
 * qpsk_path_state_init (the state qpsk_path_create leaves, buf_bytes = 256 *
 * n_streams) need no device.  get_state / set_state / reset_streams as the
 * channel's; set_state runs qpsk_path_state_check first and changes nothing
 * when it fails; reset_streams gives the listed rows their created (r, tau),
 * positions 0 and an empty history and keeps their taps. */
int qpsk_path_state_size(void);
int qpsk_path_state_init(const qpsk_path_params *p, int32_t n_streams, void *buf, int64_t buf_bytes);
int qpsk_path_get_state(qpsk_path *pa, void *host_buf, int64_t buf_bytes);
int qpsk_path_set_state(qpsk_path *pa, const void *host_buf, int64_t buf_bytes);
int qpsk_path_reset_streams(qpsk_path *pa, const int32_t *streams, int32_t n);
/* What a state must satisfy (host only): buf_bytes = 256 * n_streams; r finite
 * and within [1 - 1000e-6, 1 + 1000e-6]; tau in [0, 1); in_pos in [0, 2^50],
 * out_pos >= 0; out_pos == qpsk_path_count(r, tau, 0, in_pos) (the stream has
 * emitted everything it could); n_taps in 1..8, taps finite, unused taps +0;
 * hist entries at negative indices +0 (the others may hold any bits: inputs may
 * be NaN); reserved bytes 0.  A failure is QPSK_ERR_ARGUMENT and names stream
 * and field in qpsk_last_error. */
int qpsk_path_state_check(int32_t n_streams, const void *buf, int64_t buf_bytes);
/* The same call on host CF32 rows and a state blob, single-threaded, no
 * device: state is [n_streams] records (checked first, advanced by the call),
 * in and out float rows with strides in floats, the rest as
 * qpsk_path_apply_fmt with both formats CF32 and both scales 1. */
int qpsk_path_apply_host(void *state, int64_t state_bytes, int32_t n_streams, const float *in, int64_t stride_in,
                         float *out, int64_t stride_out, int64_t out_cap, int64_t n_samples,
                         const int64_t *lengths, int64_t *n_out);

/* ---------------------------------------------------------------------------
 * The polyphase channeliser on the device: one wideband row into M streams.
 * (Added within ABI version 3: no existing entry point, kernel or layout
 * changed.)
 *
 * What stands in front of the demodulator when a radio delivers one wideband
 * capture and not S baseband rows.  A handle holds n_bands wideband inputs at
 * rate fs, rows of any QPSK_FMT_*.  Band b yields M = channels output rows:
 * row b * M + c is the signal around c * fs / M at rate 2 * fs / M (an M-channel
 * polyphase filter bank oversampled by 2), CF32, ready for
 * qpsk_demod_process_fmt; channels c >= M / 2 are the negative frequencies.  A
 * carrier of symbol rate fs / (2 M) comes out at 4 samples a symbol.  Every
 * operation is float with one rounding; nothing contracts to an FMA.
 * Let D = M / 2, K = taps_per_branch, L = M * K.
 *
 * Prototype taps h[0 .. L-1], real floats.  qpsk_pfb_create designs them on the
 * host in double with glibc sin / cos (pi = 3.14159265358979323846):
 *   h[0] = 0
 *   for n = 1 .. L/2:   t = (double)(n - L/2) / (double)M
 *                       sinc = t == 0 ? 1 : sin(pi * t) / (pi * t)
 *                       g[n] = sinc * (0.54 - 0.46 * cos(2.0 * pi * (double)(n - 1) / (double)(L - 2)))
 *   for n = L/2+1 .. L-1:  g[n] = g[L - n]        (the window is symmetric about
 *                          L/2: g[n] of this formula at n and L - n, made equal
 *                          bit for bit)
 *   sum = g[1] + g[2] + .. + g[L-1], left to right;  h[n] = (float)(g[n] / sum)
 * L - 1 taps symmetric about n = L/2: the delay is exactly K output samples
 * (output m carries the band at input time (m - K) * D), the DC gain is 1.
 * qpsk_pfb_set_taps replaces them.
 *
 * Twiddles W[q], q in [0, M/2):  W[q] = ((float)cos(a), (float)sin(a)) with
 * a = 2.0 * pi * (double)q / (double)M in double; W[0] = (1, +0) and
 * W[M/4] = (+0, 1) are set explicitly.
 *
 * Frame m, the band's absolute frame index from 0.  With x[i] the widened input
 * at the band's absolute index i and x[i] = +0 for i < 0:
 *   1. Polyphase sum.  v[p], p in [0, M): acc = (+0, +0); for k = 0 .. K-1 in
 *      order  acc = acc + h[p + k*M] * x[m*D - p - k*M]  (the taps are real: re
 *      and im apart, a product rounded, then the sum).
 *   2. Transform, radix-2 decimation in time.  a[bitrev(p)] = v[p] (bitrev over
 *      log2 M bits); stages half = 1, 2, .., M/2; in a stage every butterfly at
 *      j0 (a multiple of 2*half) and j < half takes w = W[j * (M / (2*half))],
 *      b = a[j0+j+half],
 *        t = (w.re*b.re - w.im*b.im, w.re*b.im + w.im*b.re)
 *        a[j0+j+half] = a[j0+j] - t;  a[j0+j] = a[j0+j] + t
 *      The full multiply is done at every butterfly, also where w is 1 or j:
 *      that fixes the sign of a zero.
 *   3. Output.  y_c[m] = a[c], both parts negated when c * m is odd; then each
 *      part times gain.
 * This equals the mixer e^{-j 2 pi c i / M} on the absolute input index i, the
 * lowpass h and a decimation by D; no constant phase is left over.
 *
 * What a call emits.  After a call the band has taken inputs 0 .. in_end-1; the
 * call emits every not yet emitted frame m <= (in_end - 1) / D, so ceil(in_end
 * / D) frames are out in all.  There is no flush: append zeros for the tail.
 *
 * Not built: a subset of the channels, an oversampling other than 2, output
 * formats other than CF32, a channeliser behind the host-fed ring, a group
 * form.  (The dual, M rows into one wideband row, is the synthesis bank
 * below.) */
typedef struct qpsk_pfb_params {
    int32_t channels;           /* M, a power of two in 8 .. 4096: 64                     */
    int32_t taps_per_branch;    /* K in 1 .. 16, M * K <= 32768: 8                        */
    float gain;                 /* finite: 1                                              */
    int32_t device;             /* HIP device ordinal                                     */
    int32_t reserved[12];
} qpsk_pfb_params;
typedef struct qpsk_pfb qpsk_pfb;
#define QPSK_PFB_MIN_CHANNELS 8
#define QPSK_PFB_MAX_CHANNELS 4096
#define QPSK_PFB_MAX_BRANCH_TAPS 16
#define QPSK_PFB_MAX_TAPS 32768
#define QPSK_PFB_STATE_HEAD 64
/* channels = 64, taps_per_branch = 8, gain = 1, the rest 0. */
void qpsk_pfb_params_init(qpsk_pfb_params *p);
/* channels, taps_per_branch or their product outside the limits above, or a
 * gain that is not finite: QPSK_ERR_OUT_OF_RANGE; n_bands outside 1 .. 65535:
 * QPSK_ERR_ARGUMENT; all before a device is touched. */
int qpsk_pfb_create(const qpsk_pfb_params *p, int32_t n_bands, qpsk_pfb **out);
int qpsk_pfb_destroy(qpsk_pfb *pf);
/* As qpsk_path_set_stream. */
int qpsk_pfb_set_stream(qpsk_pfb *pf, void *hip_stream);
/* Host only.  The prototype of p into taps[n_taps], n_taps = M * K (else
 * QPSK_ERR_ARGUMENT). */
int qpsk_pfb_design(const qpsk_pfb_params *p, float *taps, int64_t n_taps);
/* Host only.  W of M channels into w[n_floats], n_floats = M (re, im of M / 2
 * twiddles; else QPSK_ERR_ARGUMENT); a bad M is QPSK_ERR_OUT_OF_RANGE. */
int qpsk_pfb_twiddles(int32_t channels, float *w, int64_t n_floats);
/* Replaces the prototype: taps is host memory, n_taps = M * K floats (else
 * QPSK_ERR_ARGUMENT), all finite (else QPSK_ERR_OUT_OF_RANGE).  Takes effect
 * behind the calls queued so far; the history is kept. */
int qpsk_pfb_set_taps(qpsk_pfb *pf, const float *taps, int64_t n_taps);
/* Host only.  max(0, ceil(in_end / D) - out_pos): what a band that has emitted
 * out_pos frames emits once it has taken in_end inputs.  Negative (an error
 * code) for a bad M, in_end outside [0, 2^50] or out_pos < 0. */
int64_t qpsk_pfb_count(int32_t channels, int64_t out_pos, int64_t in_end);
/* Host only.  n_in / D + 1, a capacity that suffices for any call of n_in
 * samples; negative (an error code) for a bad M or n_in outside [0, 2^50]. */
int64_t qpsk_pfb_out_bound(int32_t channels, int64_t n_in);
/* Host only.  The frames one workgroup of the kernel covers, 4096 / M: the
 * per-call frame counts at which the kernel changes tiles
 * (tests/test_gpu_pfb.py spans them).  A bad M is QPSK_ERR_OUT_OF_RANGE. */
int qpsk_pfb_tile_frames(int32_t channels);
/* One call: band b takes lengths[b] samples (lengths == NULL: n_samples for
 * all; host memory, each 0 .. n_samples) from row b of in, [n_bands][stride_in]
 * elements of fmt_in read as qpsk_demod_process_fmt reads them (scale_in; CU8
 * zero at 128), and writes n_out[b] samples to each of its M rows of out,
 * [n_bands * M][stride_out] floats, stride_out >= 2 * out_cap.  n_out is host
 * memory, [n_bands], and is filled before the call returns even when the
 * device work is only queued: the counts are a function of the call lengths
 * and the positions, which the handle keeps on the host.  A band that would
 * emit more than out_cap frames makes the call QPSK_ERR_ARGUMENT
 * (qpsk_pfb_out_bound gives a capacity that always suffices).  out must not
 * overlap in (the test is on the two buffers' whole extents), else
 * QPSK_ERR_ARGUMENT.  Device rows, scale_in, mem, queueing and the return
 * follow qpsk_path_apply_fmt: a device call without lengths is queued on the
 * handle's stream and returns; input rows 16-byte aligned with a pitch that is
 * a multiple of 16 bytes are read with 16-byte loads; output rows 8-byte
 * aligned are written a sample a store.  Elements past a row's n_out are not
 * written.  A rejected call changes neither the state nor out.  The caller's
 * current device is the same on return. */
int qpsk_pfb_apply_fmt(qpsk_pfb *pf, int32_t fmt_in, const void *in, int64_t stride_in, float scale_in, float *out,
                       int64_t stride_out, int64_t out_cap, int64_t n_samples, const int64_t *lengths, int64_t *n_out,
                       int32_t mem);
/* State: per band QPSK_PFB_STATE_HEAD = 64 bytes
 *   int64 in_pos, out_pos; 48 reserved bytes (0)
 * followed by float hist[L][2], the widened inputs at indices in_pos-L ..
 * in_pos-1 (entries at negative indices are +0); no header in front of the
 * bands.  The taps are not part of it.  qpsk_pfb_state_size(p) = 64 + 8 L
 * (negative, an error code, for bad parameters) and qpsk_pfb_state_init (the
 * state qpsk_pfb_create leaves: all zero; buf_bytes = n_bands * state_size)
 * need no device.  get_state / set_state as the path's; set_state runs
 * qpsk_pfb_state_check first and changes nothing when it fails; reset_bands
 * gives the listed bands (a list as qpsk_stream_list_check accepts) positions
 * 0 and an empty history. */
int64_t qpsk_pfb_state_size(const qpsk_pfb_params *p);
int qpsk_pfb_state_init(const qpsk_pfb_params *p, int32_t n_bands, void *buf, int64_t buf_bytes);
int qpsk_pfb_get_state(qpsk_pfb *pf, void *host_buf, int64_t buf_bytes);
int qpsk_pfb_set_state(qpsk_pfb *pf, const void *host_buf, int64_t buf_bytes);
int qpsk_pfb_reset_bands(qpsk_pfb *pf, const int32_t *bands, int32_t n);
/* What a state must satisfy (host only): buf_bytes = n_bands * state_size;
 * in_pos in [0, 2^50]; out_pos == ceil(in_pos / D) (the band has emitted
 * everything it could); hist entries at negative indices +0 (the others may
 * hold any bits: inputs may be NaN); reserved bytes 0.  A failure is
 * QPSK_ERR_ARGUMENT and names band and field in qpsk_last_error. */
int qpsk_pfb_state_check(const qpsk_pfb_params *p, int32_t n_bands, const void *buf, int64_t buf_bytes);
/* The same call on host CF32 rows and a state blob, single-threaded, no
 * device: taps is the prototype, M * K floats (NULL: the design of p); state
 * is [n_bands] records (checked first, advanced by the call), in and out float
 * rows with strides in floats, the rest as qpsk_pfb_apply_fmt with CF32 input. */
int qpsk_pfb_apply_host(const qpsk_pfb_params *p, const float *taps, void *state, int64_t state_bytes, int32_t n_bands,
                        const float *in, int64_t stride_in, float *out, int64_t stride_out, int64_t out_cap,
                        int64_t n_samples, const int64_t *lengths, int64_t *n_out);

/* ---------------------------------------------------------------------------
 * The polyphase synthesis bank on the device: M streams into one wideband row.
 * (Added within ABI version 3: no existing entry point, kernel or layout
 * changed.)
 *
 * The channeliser's dual, what stands behind the modulator when a radio takes
 * one wideband row and not S baseband rows.  A handle holds n_bands bands.
 * Band b takes M = channels input rows b * M + c at rate 2 * fs / M, rows of any
 * QPSK_FMT_* widened as qpsk_demod_process_fmt reads them, and writes one
 * wideband row b at rate fs, of any QPSK_FMT_*.  Row c lands around c * fs / M;
 * rows c >= M / 2 are the negative frequencies.  A modulator row at 4 samples a
 * symbol becomes a carrier of symbol rate fs / (2 M), which is what qpsk_pfb
 * returns at 4 samples a symbol.  Every operation is float with one rounding;
 * nothing contracts to an FMA.  Let D = M / 2, K = taps_per_branch, L = M * K.
 * The limits on M, K, L and n_bands are the channeliser's (QPSK_PFB_*).
 *
 * The prototype g[0 .. L-1] and the twiddles W[q] are the channeliser's own
 * (qpsk_pfb_design, qpsk_pfb_twiddles, defined above); qpsk_sfb_set_taps
 * replaces the prototype.
 *
 * Frame m, the band's absolute frame index from 0, is one sample s_c[m] of each
 * of the M rows.  The band's output sample i = f * D + r, r in [0, D):
 *   1. Sign.  z_c[m] = s_c[m], both parts negated when c * m is odd.
 *   2. Transform, the channeliser's step 2 verbatim.  a[bitrev(c)] = z_c[m];
 *      stages half = 1, 2, .., M/2, every butterfly with w = W[j * (M / (2*half))]
 *      and the full multiply everywhere; u_m[q] = a[q].
 *   3. Polyphase sum.  acc = (+0, +0); for j = 0 .. 2K-1 in order
 *        acc = acc + g[j*D + r] * u_{f-j}[(r + j*D) mod M]
 *      (the taps are real: re and im apart, a product rounded, then the sum).
 *      Frames m < 0 contribute +0; acc starts at +0 and is never -0, so the
 *      sign of such a zero cannot show.  The sample is acc stored as the
 *      modulator's fixed-scale quantiser stores it (qpsk_quantise_iq with
 *      QPSK_MOD_NORM_FIXED): one multiply by scale_out, then, for the integer
 *      formats, clamp and truncate.  There is no separate gain: scale_out = D
 *      gives a carrier its input amplitude.
 * This equals x[i] = sum_c sum_m s_c[m] * g[i - m*D] * e^{+j 2 pi c i / M}: an
 * upsampling by D, the lowpass g and the mixer on the absolute output index i.
 *
 * What a call emits.  A band that has taken n frames has emitted exactly n * D
 * samples, and a call of len frames emits len * D: no ragged count, no flush.
 * The delay is L / 2 wideband samples, so bank and channeliser together delay
 * a row by 2 K of its samples.
 *
 * Bank and channeliser are no perfect-reconstruction pair.  On the CPU, with
 * M = 16, K = 8, one carrier at 4 samples a symbol, alpha = 0.4, the designed
 * prototype and scale_out = D, the carrier comes back within 0.17 of its peak
 * on its own channel, 0.013 leaks into each neighbour and <= 5e-4 appears
 * elsewhere: the prototype's transition band lies over the RRC's edge.
 *
 * Not built: a subset of the channels, an oversampling other than 2, a bank
 * behind the host-fed ring, a group form, a kernel that fuses transform and
 * sum, a prototype designed for reconstruction. */
typedef struct qpsk_sfb_params {
    int32_t channels;           /* M, a power of two in 8 .. 4096: 64                     */
    int32_t taps_per_branch;    /* K in 1 .. 16, M * K <= 32768: 8                        */
    int32_t device;             /* HIP device ordinal                                     */
    int32_t reserved[12];
} qpsk_sfb_params;
typedef struct qpsk_sfb qpsk_sfb;
#define QPSK_SFB_STATE_HEAD 64
#define QPSK_SFB_TILE_TRANSFORM 0
#define QPSK_SFB_TILE_SUM 1
#define QPSK_SFB_TILE_SLAB 2
/* channels = 64, taps_per_branch = 8, the rest 0. */
void qpsk_sfb_params_init(qpsk_sfb_params *p);
/* channels, taps_per_branch or their product outside the channeliser's limits:
 * QPSK_ERR_OUT_OF_RANGE; n_bands outside 1 .. 65535: QPSK_ERR_ARGUMENT; all
 * before a device is touched. */
int qpsk_sfb_create(const qpsk_sfb_params *p, int32_t n_bands, qpsk_sfb **out);
int qpsk_sfb_destroy(qpsk_sfb *sf);
/* As qpsk_path_set_stream. */
int qpsk_sfb_set_stream(qpsk_sfb *sf, void *hip_stream);
/* As qpsk_pfb_set_taps. */
int qpsk_sfb_set_taps(qpsk_sfb *sf, const float *taps, int64_t n_taps);
/* Host only.  The per-call frame counts at which a kernel takes another
 * workgroup or the call another pass (tests/test_gpu_sfb.py spans them):
 *   QPSK_SFB_TILE_TRANSFORM  the smallest n >= 1 for which n + 2K - 1 is a
 *                            multiple of 4096 / M: the transform kernel's
 *                            tiles of 4096 / M frames count from the 2K - 1
 *                            frames of history in front of a call;
 *   QPSK_SFB_TILE_SUM        128, the run of frames a lane of the sum kernel
 *                            walks;
 *   QPSK_SFB_TILE_SLAB       max(64, 2^22 / M), the frames a one-band handle
 *                            transforms and sums in one pass; a handle of
 *                            n_bands bands takes max(64, 2^22 / M / n_bands).
 * A bad M or K is QPSK_ERR_OUT_OF_RANGE, a bad `which` QPSK_ERR_ARGUMENT. */
int qpsk_sfb_tile_frames(int32_t channels, int32_t taps_per_branch, int32_t which);
/* One call: band b takes lengths[b] frames (lengths == NULL: n_frames for all;
 * host memory, each 0 .. n_frames), one sample of each of its M rows of in,
 * [n_bands * M][stride_in] elements of fmt_in (scale_in; CU8 zero at 128),
 * stride_in >= 2 * n_frames, and writes lengths[b] * D samples to row b of out,
 * [n_bands][stride_out] elements of fmt_out, stride_out >= 2 * n_frames * D.
 * norm_out must be QPSK_MOD_NORM_FIXED (QPSK_MOD_NORM_PEAK would need a second
 * pass: QPSK_ERR_ARGUMENT).  out must not overlap in (the test is on the two
 * buffers' whole extents), else QPSK_ERR_ARGUMENT.  Device rows, scales, mem,
 * queueing and the return follow qpsk_path_apply_fmt: a device call without
 * lengths is queued on the handle's stream and returns; rows 8-byte aligned
 * (CF32) are read and written a sample an access.  Elements past a row's
 * lengths[b] * D samples are not written.  The handle owns a scratch buffer of
 * at most 2^22 + (2K - 1) * M * n_bands transform elements of 8 bytes (more
 * where n_bands * M * 64 exceeds 2^22); when it cannot be allocated the call is
 * QPSK_ERR_DEVICE.  A rejected call changes neither the state nor out.  The
 * caller's current device is the same on return. */
int qpsk_sfb_apply_fmt(qpsk_sfb *sf, int32_t fmt_in, const void *in, int64_t stride_in, float scale_in,
                       int32_t fmt_out, int32_t norm_out, void *out, int64_t stride_out, float scale_out,
                       int64_t n_frames, const int64_t *lengths, int32_t mem);
/* State: per band QPSK_SFB_STATE_HEAD = 64 bytes
 *   int64 in_pos (frames), out_pos (== in_pos * D); 48 reserved bytes (0)
 * followed by float hist[2K-1][M][2], the widened inputs of frames
 * in_pos-(2K-1) .. in_pos-1 before the sign, frame-major (frames at negative
 * indices are +0); no header in front of the bands.  The taps are not part of
 * it.  qpsk_sfb_state_size(p) = 64 + 8 M (2K - 1) (negative, an error code, for
 * bad parameters) and qpsk_sfb_state_init (the state qpsk_sfb_create leaves:
 * all zero; buf_bytes = n_bands * state_size) need no device.  get_state /
 * set_state / reset_bands as the channeliser's. */
int64_t qpsk_sfb_state_size(const qpsk_sfb_params *p);
int qpsk_sfb_state_init(const qpsk_sfb_params *p, int32_t n_bands, void *buf, int64_t buf_bytes);
int qpsk_sfb_get_state(qpsk_sfb *sf, void *host_buf, int64_t buf_bytes);
int qpsk_sfb_set_state(qpsk_sfb *sf, const void *host_buf, int64_t buf_bytes);
int qpsk_sfb_reset_bands(qpsk_sfb *sf, const int32_t *bands, int32_t n);
/* What a state must satisfy (host only): buf_bytes = n_bands * state_size;
 * in_pos in [0, 2^50 / D]; out_pos == in_pos * D; hist frames at negative
 * indices +0 (the others may hold any bits: inputs may be NaN); reserved bytes
 * 0.  A failure is QPSK_ERR_ARGUMENT and names band and field in
 * qpsk_last_error. */
int qpsk_sfb_state_check(const qpsk_sfb_params *p, int32_t n_bands, const void *buf, int64_t buf_bytes);
/* The same call on host CF32 rows and a state blob, single-threaded, no
 * device: taps is the prototype, M * K floats (NULL: the design); state is
 * [n_bands] records (checked first, advanced by the call), in and out float
 * rows with strides in floats, CF32 out at scale_out, the rest as
 * qpsk_sfb_apply_fmt with CF32 input. */
int qpsk_sfb_apply_host(const qpsk_sfb_params *p, const float *taps, void *state, int64_t state_bytes, int32_t n_bands,
                        const float *in, int64_t stride_in, float *out, int64_t stride_out, float scale_out,
                        int64_t n_frames, const int64_t *lengths);

/* ---------------------------------------------------------------------------
 * The tuner on the device: per-stream frequency shift and any-rate resampler.
 * (Added within ABI version 3: no existing entry point, kernel or layout
 * changed.)
 *
 * The digital down-converter that stands behind the channeliser, or in front
 * of the demodulator on its own: a carrier that is off the bank's grid, or a
 * baseband row from a radio, is moved to DC and brought to the sample rate the
 * demodulator wants.  Per stream: a numerically controlled oscillator, a
 * lowpass and a resampler by an arbitrary ratio, rows of any QPSK_FMT_* in and
 * out.  Used in reverse (resample first, then shift in a second handle) two
 * tuners make off-grid test carriers.  Every operation is float (double or
 * integer where stated) with one rounding; nothing contracts to an FMA; no
 * result depends on how calls cut a stream.  T = taps_per_phase.
 *
 * Oscillator.  fw = (int64) rint(freq * 2^64), freq in cycles per input sample
 * (the scaling is exact).  The phase of the stream's absolute input index i is
 *   ph(i) = ph0 + fw * i          wrapping uint64 arithmetic: exact, whatever
 *                                 i's size and however calls cut the stream
 *   a = ph >> 54 (10 bits),  b = (ph >> 44) & 1023;  the low 44 bits are dropped
 * Two tables of 1024 complex floats, formed on the host in double with glibc
 * cos / sin (pi = 3.14159265358979323846) and rounded once:
 *   C[a] = ((float)cos(t), (float)sin(t)),  t = 2.0 * pi * (double)a / 1024.0
 *   F[b] likewise with                      t = 2.0 * pi * (double)b / 1048576.0
 * C[0] = F[0] = (1, +0) are set explicitly.  Then
 *   w    = (C.re*F.re - C.im*F.im, C.re*F.im + C.im*F.re)
 *   z[i] = x[i] * conj(w) = (x.re*w.re + x.im*w.im, x.im*w.re - x.re*w.im)
 * so a positive freq brings a carrier at +freq to DC.  x[i] is the widened
 * input as qpsk_demod_process_fmt reads it (scale_in; CU8 zero at 128), and +0
 * for i < 0 (z[i] is still formed by the two lines above).
 * |w - e^{j 2 pi ph / 2^64}| <= 2 pi 2^-20 + 2^-21: the dropped bits, then the
 * float roundings.
 *
 * Prototype h[0 .. 64 T]: 64 phases of T taps and one end point, real floats.
 * qpsk_tuner_create designs them on the host in double with glibc sin / cos,
 * N = 64 T, fc = cutoff (cycles per input sample), g = 2.0 * fc:
 *   for m = 0 .. N/2:  t = (double)(m - N/2) / 64.0;  x = g * t
 *                      sinc = x == 0 ? 1 : sin(pi * x) / (pi * x)
 *                      G[m] = g * sinc * (0.54 - 0.46 * cos(2.0 * pi * (double)m / (double)N))
 *                             (the products left to right)
 *   for m = N/2+1 .. N:  G[m] = G[N - m]      (symmetric about N/2 bit for bit)
 *   sum = G[0] + G[1] + .. + G[N], left to right;  h[m] = (float)(G[m] * 64.0 / sum)
 *   d[m] = h[m+1] - h[m], m = 0 .. N-1: one float subtraction, precomputed
 * Every phase's T taps sum to about 1: the DC gain is 1.  The filter is centred
 * on the output's own position p_k below: the stage adds no delay to a row.
 * qpsk_tuner_set_taps replaces h; the library derives d again.  cutoff = 0
 * stands for 0.4 * min(1, 1 / rate) with the params' rate.
 *
 * Resampler.  Output k, the stream's absolute output index from 0, sits at the
 * path's closed form  p_k = tau + (double)k * r  (r input samples per output
 * sample), all in double:
 *   n = floor(p_k), mu = p_k - n;  u = mu * 64 (exact);  q = (int)floor(u);
 *   f = (float)(u - q)
 *   acc = (+0, +0); for j = 0 .. T-1 in order
 *     m = 64 * (T - 1 - j) + q
 *     c = h[m] + f * d[m]                    (the product rounded, then the sum)
 *     acc = acc + c * z[n - T/2 + 1 + j]     (re and im apart, each product
 *                                            rounded, then the sum)
 * The result goes through QPSK_MOD_NORM_FIXED of qpsk_quantise_iq with
 * scale_out, as the path stores; QPSK_MOD_NORM_PEAK is QPSK_ERR_ARGUMENT.
 *
 * What a call emits.  After a call the stream has taken inputs 0 .. in_end-1;
 * the call emits every not yet emitted k with floor(p_k) <= in_end - 1 - T/2.
 * There is no flush: append zeros for the tail.  Input positions are held to
 * 2^50 (output positions then stay below 2^52 + 2).
 *
 * Not built: finding carriers, a time-varying r or a change of r on a live
 * stream (reset the stream, or set a state), r outside [0.25, 4] (use another
 * channeliser M), per-stream prototypes (use one handle a filter), a group
 * form, the host-fed ring, peak normalisation. */
typedef struct qpsk_tuner_params {
    double freq;                /* cycles per input sample, [-0.5, 0.5): 0                */
    double rate;                /* r, input samples per output sample, [0.25, 4]: 1       */
    double tau0;                /* position of output 0, [0, 1): 0                        */
    double cutoff;              /* fc in (0, 0.5]; 0: 0.4 * min(1, 1 / rate)              */
    int32_t taps_per_phase;     /* T, even, 4 .. 32: 16                                   */
    int32_t device;             /* HIP device ordinal                                     */
    int64_t first_stream;       /* global id of row 0, >= 0 (carried, not interpreted)    */
    int32_t reserved[6];
} qpsk_tuner_params;
typedef struct qpsk_tuner qpsk_tuner;
#define QPSK_TUNER_PHASES 64
#define QPSK_TUNER_MIN_TAPS 4
#define QPSK_TUNER_MAX_TAPS 32
#define QPSK_TUNER_HIST 32
#define QPSK_TUNER_MIN_RATE 0.25
#define QPSK_TUNER_MAX_RATE 4.0
/* The outputs one workgroup of the tuner kernel covers: the per-call output
 * counts at which the kernel changes tiles (tests/test_gpu_tuner.py spans them). */
#define QPSK_TUNER_TILE_OUTPUTS 1024
/* rate = 1, taps_per_phase = 16, the rest 0. */
void qpsk_tuner_params_init(qpsk_tuner_params *p);
/* freq and rate, both host memory, [n_streams], give per-stream values where
 * not NULL (else the params' freq and rate hold for every stream).  One
 * prototype, designed from T and cutoff, serves the whole handle.  A freq, rate,
 * tau0, cutoff or T outside its range (or not finite) or first_stream < 0:
 * QPSK_ERR_OUT_OF_RANGE; n_streams < 1: QPSK_ERR_ARGUMENT; all before a device
 * is touched. */
int qpsk_tuner_create(const qpsk_tuner_params *p, int32_t n_streams, const double *freq, const double *rate,
                      qpsk_tuner **out);
int qpsk_tuner_destroy(qpsk_tuner *tu);
/* As qpsk_path_set_stream. */
int qpsk_tuner_set_stream(qpsk_tuner *tu, void *hip_stream);
/* Host only.  The prototype of (T, cutoff) into h[n_points], n_points = 64 T + 1
 * (else QPSK_ERR_ARGUMENT); cutoff in (0, 0.5] and T as above, else
 * QPSK_ERR_OUT_OF_RANGE. */
int qpsk_tuner_design(int32_t taps_per_phase, double cutoff, float *h, int64_t n_points);
/* Host only.  The oscillator's tables, [1024][2] floats each. */
int qpsk_tuner_tables(float *coarse, float *fine);
/* Host only.  w of each of n phases, [n][2] floats. */
int qpsk_tuner_osc(const uint64_t *ph, int64_t n, float *w);
/* Replaces the prototype: h is host memory, n_points = 64 T + 1 floats (else
 * QPSK_ERR_ARGUMENT), all finite (else QPSK_ERR_OUT_OF_RANGE).  Takes effect
 * behind the calls queued so far; the history is kept. */
int qpsk_tuner_set_taps(qpsk_tuner *tu, const float *h, int64_t n_points);
/* Retunes the n listed streams (a list as qpsk_stream_list_check accepts) to
 * freqs[n], host memory, behind the calls queued so far.  The phase stays
 * continuous: ph0' = ph0 + (fw_old - fw_new) * in_pos (wrapping), so ph(in_pos)
 * is what it was.  A freq outside [-0.5, 0.5) is QPSK_ERR_OUT_OF_RANGE and
 * changes nothing.  (The Costas freq of qpsk_demod_link_stats, in cycles per
 * output sample, divided by r is what a caller adds to follow a carrier.) */
int qpsk_tuner_set_freq(qpsk_tuner *tu, const int32_t *streams, int32_t n, const double *freqs);
/* One call, with the argument list and every rule of qpsk_path_apply_fmt:
 * host or device memory, per-stream lengths, n_out filled before the call
 * returns, out_cap (qpsk_tuner_out_bound gives one that always suffices), no
 * overlap of in and out, 16-byte rows read with 16-byte loads, a rejected call
 * changes neither the state nor out, a device call without lengths is only
 * queued. */
int qpsk_tuner_apply_fmt(qpsk_tuner *tu, int32_t fmt_in, const void *in, int64_t stride_in, float scale_in,
                         int32_t fmt_out, int32_t norm_out, void *out, int64_t stride_out, int64_t out_cap,
                         float scale_out, int64_t n_samples, const int64_t *lengths, int64_t *n_out, int32_t mem);
/* Host only.  A capacity that is enough for any call of n_in samples on a
 * stream of the smallest of rates[n_streams] (rates == NULL: the params' rate):
 * ceil(n_in / r_min) + 4; negative (an error code) for bad arguments. */
int64_t qpsk_tuner_out_bound(const qpsk_tuner_params *p, const double *rates, int32_t n_streams, int64_t n_in);
/* Host only.  How many outputs a stream at (r, tau) with T taps a phase that
 * has emitted out_pos emits once it has taken in_end inputs: the k >= out_pos
 * with floor(p_k) <= in_end - 1 - T/2, from the path's division and a
 * correction by that predicate.  Negative (an error code) for r, tau or T
 * outside their ranges, in_end outside [0, 2^50] or out_pos outside [0, 2^52 + 2]. */
int64_t qpsk_tuner_count(double r, double tau, int32_t taps_per_phase, int64_t out_pos, int64_t in_end);
/* State: per stream 320 bytes, no header,
 *   double r, tau; int64 fw; uint64 ph0; int64 in_pos, out_pos; 16 reserved
 *   bytes (0); float hist[32][2]
 * hist holds the widened, unmixed inputs at indices in_pos-32 .. in_pos-1 (the
 * next call can need T - 1 <= 31 of them); entries at negative indices are +0.
 * The mixer is redone from the absolute index: no oscillator history exists.
 * The prototype is not part of it.  qpsk_tuner_state_size() = 320 and
 * qpsk_tuner_state_init (the state qpsk_tuner_create leaves for the same
 * arguments, buf_bytes = 320 * n_streams) need no device.  get_state /
 * set_state / reset_streams as the path's; set_state runs
 * qpsk_tuner_state_check first and changes nothing when it fails;
 * reset_streams gives the listed rows their created (r, tau), ph0 = 0,
 * positions 0 and an empty history and keeps their fw as set_freq left it. */
int qpsk_tuner_state_size(void);
int qpsk_tuner_state_init(const qpsk_tuner_params *p, int32_t n_streams, const double *freq, const double *rate,
                          void *buf, int64_t buf_bytes);
int qpsk_tuner_get_state(qpsk_tuner *tu, void *host_buf, int64_t buf_bytes);
int qpsk_tuner_set_state(qpsk_tuner *tu, const void *host_buf, int64_t buf_bytes);
int qpsk_tuner_reset_streams(qpsk_tuner *tu, const int32_t *streams, int32_t n);
/* What a state must satisfy (host only; p gives T): buf_bytes = 320 *
 * n_streams; r in [0.25, 4]; tau in [0, 1); in_pos in [0, 2^50]; out_pos ==
 * qpsk_tuner_count(r, tau, T, 0, in_pos) (the stream has emitted everything it
 * could); hist entries at negative indices +0 (the others may hold any bits);
 * reserved bytes 0; fw and ph0 may hold any value.  A failure is
 * QPSK_ERR_ARGUMENT and names stream and field in qpsk_last_error. */
int qpsk_tuner_state_check(const qpsk_tuner_params *p, int32_t n_streams, const void *buf, int64_t buf_bytes);
/* The same call on host CF32 rows and a state blob, single-threaded, no
 * device: h is the prototype, 64 T + 1 floats (NULL: the design of p); state is
 * [n_streams] records (checked first, advanced by the call), in and out float
 * rows with strides in floats, the rest as qpsk_tuner_apply_fmt with both
 * formats CF32 and both scales 1. */
int qpsk_tuner_apply_host(const qpsk_tuner_params *p, const float *h, void *state, int64_t state_bytes,
                          int32_t n_streams, const float *in, int64_t stride_in, float *out, int64_t stride_out,
                          int64_t out_cap, int64_t n_samples, const int64_t *lengths, int64_t *n_out);

const char *qpsk_last_error(void);
int qpsk_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
