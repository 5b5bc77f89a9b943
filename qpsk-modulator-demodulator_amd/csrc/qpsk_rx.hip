// qpsk_rx.hip -- host-fed streaming front-end.
//
// The reference's deployment loop (ModDemodOverSDR.cs:116-183) reads CF32
// buffers from the SDR and calls DeModulate on each in turn, one host thread,
// state carried from call to call.  Here a ring of `depth` pinned host slots
// feeds one batched handle:
//
//   submit k:  [host copy into pinned slot k%D unless the caller filled it]
//              upload stream U : wait(slot free) -> H2D slot -> (handle's stream)
//              qpsk_demod_process_async: front (FIR / FLL) then back (loop)
//              front stream    : record in_free[slot]   (input consumed)
//              download stream : wait(back stage) -> D2H bits, counts -> out_done[slot]
//   collect:   wait out_done of the oldest chunk, copy its rows to the caller
//
// U is the handle's own stream, so process_async's front stage is ordered
// after the upload; the next upload (slot k+1) only waits for the stage that
// last read ITS slot, so it runs on the copy engine while chunk k computes.
// Everything the chain computes is done by the same kernels in the same call
// order as synchronous qpsk_demod_process calls, hence identical bits.
//
// A CS16 ring (qpsk_rx_create_cs16) is the same ring with int16 slots: an SDR
// driver's native CS16 buffers go up as they are, 4 bytes a sample, and the
// matched filter widens them (qpsk_demod_process_async_cs16).  A CS8 or CU8
// ring (qpsk_rx_create_fmt) has byte slots, 2 bytes a sample; its device
// slots' rows are pitched to 8 samples so the matched filter reads them with
// 16-byte loads whatever max_samples_per_call is.
//
// A framed ring (qpsk_rx_attach_framer) owns a device framer and returns what
// the reference's loop looks at, DeModulateBytes' frames (ModDemodOverSDR.cs:136):
//
//   submit k:  download stream : wait(back stage) -> TSC search -> framer step
//              -> pack the completed frames -> D2H index [-> D2H bits] -> out_done[slot]
//   collect_frames: wait out_done, D2H exactly head[0] packed bytes on the
//              fetch stream (the download stream may hold chunk k+1 already)
//
// The framer's state passes from chunk to chunk in submit order because every
// chunk's framer step is queued on the one download stream.
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "qpsk_handle.h"

namespace {
using qpsk::fail;

struct Slot {
    qpsk::PinnedBuf<char> h_in;      // [S][in_stride] elements of the ring's format
    qpsk::DevBuf<char> d_in;         // [S][dev_stride]
    qpsk::DevBuf<uint8_t> d_bits;    // [S][bits_stride]
    qpsk::DevBuf<int64_t> d_nb;      // [S]
    qpsk::PinnedBuf<uint8_t> h_bits;
    qpsk::PinnedBuf<int64_t> h_nb;
    qpsk::Event in_free, out_done;
    int64_t row_bytes = 0;      // bit bytes per row this chunk can hold
    // a framed ring (qpsk_rx_attach_framer)
    qpsk::DevBuf<uint8_t> d_packed;     // [chunk_frame_bytes] the chunk's frames, packed
    qpsk::PinnedBuf<uint8_t> h_packed;
    qpsk::PinnedBuf<int64_t> h_index;   // frame_len[S], offsets[S], head[2]
};

// The device framer behind a framed ring.  The payload rows, the TSC offsets
// and the index are shared by the slots: a framer's chunks are serial on the
// download stream, and each chunk's index is copied to its slot's pinned
// memory before the next chunk's framer step runs.
struct Framed {
    qpsk_framer_dev *fr = nullptr;
    std::string tsc;
    int64_t P = 0;                      // max_frame_bytes, a multiple of 16
    int64_t C = 0;                      // chunk_frame_bytes, a multiple of 16
    bool keep_bits = false;
    qpsk::Stream fetch;                 // collect_frames' D2H: no chunk's work is ever queued on it
    qpsk::DevBuf<uint8_t> rows;         // [S][P]
    qpsk::DevBuf<int64_t> tsc_off;      // [S]
    qpsk::DevBuf<int64_t> index;        // frame_len[S], offsets[S], head[2]
    ~Framed() {
        if (fr) qpsk_framer_dev_destroy(fr);
    }
};
}  // namespace

struct qpsk_rx {
    qpsk_demod *h = nullptr;
    int depth = 0;
    int S = 0;
    int64_t n_max = 0;
    int64_t in_stride = 0;      // elements (floats, int16 or bytes): 2 * n_max
    int64_t dev_stride = 0;     // elements of a device slot's row (8-bit: n_max rounded up to 8 samples)
    int32_t fmt = QPSK_FMT_CF32;
    size_t elem = sizeof(float);   // bytes per element of a slot
    int64_t bits_stride = 0;    // bytes
    int device = 0;
    qpsk::Stream up, down;      // in front of the slots, which go first
    std::vector<Slot> slots;
    int64_t submitted = 0, collected = 0;
    std::unique_ptr<Framed> fr;     // behind the streams and the slots: it goes first
};

namespace {
int setup(qpsk_rx *r) {
    QPSK_HIP_TRY(hipSetDevice(r->device));
    QPSK_HIP_TRY(r->up.create(hipStreamNonBlocking));
    QPSK_HIP_TRY(r->down.create(hipStreamNonBlocking));
    const size_t S = static_cast<size_t>(r->S);
    const size_t in_bytes = S * static_cast<size_t>(r->in_stride) * r->elem;
    const size_t dev_bytes = S * static_cast<size_t>(r->dev_stride) * r->elem;
    const size_t bit_bytes = S * static_cast<size_t>(r->bits_stride);
    r->slots.resize(r->depth);
    for (auto &s : r->slots) {
        QPSK_HIP_TRY(s.h_in.alloc(in_bytes));
        QPSK_HIP_TRY(s.h_bits.alloc(bit_bytes));
        QPSK_HIP_TRY(s.h_nb.alloc(S));
        QPSK_HIP_TRY(s.d_in.alloc(dev_bytes));
        QPSK_HIP_TRY(s.d_bits.alloc(bit_bytes));
        QPSK_HIP_TRY(s.d_nb.alloc(S));
        QPSK_HIP_TRY(s.in_free.ensure());
        QPSK_HIP_TRY(s.out_done.ensure());
    }
    return QPSK_OK;
}

const char *kUnknownFormat = "unknown sample format";
const char *kNoFramer = "the ring has no framer (qpsk_rx_attach_framer)";
const char *kNoBits = "the ring's framer keeps no bits (keep_bits = 0)";

// the collected chunk's bit rows and counts, from the slot's pinned memory
void copy_bits(const qpsk_rx *r, const Slot &sl, uint8_t *bits, int64_t bits_stride_bytes, int64_t *n_bits) {
    for (int s = 0; s < r->S; ++s) {
        const int64_t nb = sl.h_nb[s];
        n_bits[s] = nb;
        std::memcpy(bits + static_cast<int64_t>(s) * bits_stride_bytes, sl.h_bits + static_cast<int64_t>(s) * r->bits_stride,
                    static_cast<size_t>((nb + 7) / 8));
    }
}

int create(qpsk_demod *h, int32_t depth, int32_t fmt, qpsk_rx **out) {
    if (!h || !out) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    *out = nullptr;
    if (!qpsk::fmt_known(fmt)) return fail(QPSK_ERR_ARGUMENT, kUnknownFormat);
    if (depth < 2 || depth > 8) return fail(QPSK_ERR_ARGUMENT, "depth must be 2..8");
    qpsk_rx *r = new qpsk_rx;
    r->h = h;
    r->depth = depth;
    r->S = h->S;
    r->n_max = h->n_max;
    r->device = h->p.device;
    r->in_stride = 2 * r->n_max;
    r->fmt = fmt;
    r->elem = static_cast<size_t>(qpsk::fmt_elem_bytes(fmt));
    r->dev_stride = r->elem == 1 ? 2 * ((r->n_max + 7) / 8 * 8) : r->in_stride;
    r->bits_stride = ((2 * qpsk_demod_max_symbols(h, r->n_max) + 7) / 8 + 15) / 16 * 16;
    int rc = setup(r);
    if (rc == QPSK_OK) rc = qpsk_demod_set_stream(h, r->up);
    if (rc != QPSK_OK) {
        delete r;
        return rc;
    }
    *out = r;
    return QPSK_OK;
}

// a ring has one format; between the two formats of the untagged entry points
// the text names them
int wrong_format(int32_t ring_fmt, int32_t fmt) {
    const bool pair = ring_fmt <= QPSK_FMT_CS16 && fmt <= QPSK_FMT_CS16;
    return fail(QPSK_ERR_STATE, pair ? "the ring was created for the other sample format (CF32 / CS16)"
                                     : "the ring was created for another sample format");
}

int next_slot(qpsk_rx *r, int32_t fmt, void **iq, int64_t *stride_floats) {
    if (!r || !iq) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    if (!qpsk::fmt_known(fmt)) return fail(QPSK_ERR_ARGUMENT, kUnknownFormat);
    if (r->fmt != fmt) return wrong_format(r->fmt, fmt);
    if (r->submitted - r->collected >= r->depth)
        return fail(QPSK_ERR_STATE, "every ring slot holds an uncollected chunk");
    Slot &sl = r->slots[r->submitted % r->depth];
    // the caller writes the slot next: its previous chunk must have been read
    QPSK_HIP_TRY(sl.in_free.sync());
    *iq = sl.h_in;
    if (stride_floats) *stride_floats = r->in_stride;
    return QPSK_OK;
}

int submit(qpsk_rx *r, int32_t fmt, const void *iq, int64_t stride_floats, int64_t n_samples,
           const int64_t *lengths, int64_t *ticket) {
    if (!r) return fail(QPSK_ERR_ARGUMENT_NULL, "null ring");
    if (!qpsk::fmt_known(fmt)) return fail(QPSK_ERR_ARGUMENT, kUnknownFormat);
    if (r->fmt != fmt) return wrong_format(r->fmt, fmt);
    if (r->submitted - r->collected >= r->depth)
        return fail(QPSK_ERR_STATE, "every ring slot holds an uncollected chunk");
    const int S = r->S;
    Slot &sl = r->slots[r->submitted % r->depth];
    int rc;
    int64_t n_call = 0;
    // a slot is shorter than the longest call a handle takes, so the ring's own
    // limit answers before the shared check's
    if ((rc = qpsk::call_length(S, n_samples, lengths, &n_call))) return rc;
    if (n_call > r->n_max) return fail(QPSK_ERR_ARGUMENT, "chunk longer than the ring slots (max_samples_per_call)");
    // the call as the handle will see it, but on the caller's host rows (which
    // no rule asks the sample format of)
    qpsk::CallArgs c{QPSK_MODE_DEMODULATE, iq, stride_floats, n_samples, lengths, QPSK_MEM_HOST,
                     sl.d_bits, r->bits_stride, sl.d_nb, nullptr, 0, nullptr, fmt};
    if ((rc = qpsk::check_call(r->h, S, c))) return rc;
    QPSK_HIP_TRY(hipSetDevice(r->device));
    // the slot's previous chunk: its input was consumed (front stage) and its
    // bits were downloaded before this chunk overwrites either (the back stage
    // of this chunk follows the upload through the handle's stream)
    QPSK_HIP_TRY(sl.in_free.sync());
    if (n_call > 0 && iq != sl.h_in.get()) {
        for (int s = 0; s < S; ++s) {
            const int64_t len = lengths ? lengths[s] : n_call;
            std::memcpy(sl.h_in + static_cast<int64_t>(s) * r->in_stride * r->elem,
                        static_cast<const char *>(iq) + static_cast<int64_t>(s) * stride_floats * r->elem,
                        static_cast<size_t>(2 * len) * r->elem);
        }
    } else if (n_call > 0 && stride_floats != r->in_stride) {
        return fail(QPSK_ERR_ARGUMENT, "a ring slot has a stride of 2 * max_samples_per_call elements");
    }
    QPSK_HIP_TRY(sl.out_done.wait(r->up));
    if (n_call > 0)
        QPSK_HIP_TRY(hipMemcpy2DAsync(sl.d_in, r->dev_stride * r->elem, sl.h_in, r->in_stride * r->elem,
                                      2 * n_call * r->elem, S, hipMemcpyHostToDevice, r->up));
    rc = qpsk_demod_process_async_fmt(r->h, fmt, QPSK_MODE_DEMODULATE, sl.d_in, r->dev_stride, n_samples, lengths,
                                      sl.d_bits, r->bits_stride, sl.d_nb, nullptr, 0, nullptr);
    if (rc != QPSK_OK) return rc;
    QPSK_HIP_TRY(sl.in_free.record(r->h->s_front));   // "input consumed": behind the front stage
    if ((rc = qpsk_demod_pipeline_wait(r->h, r->down)) != QPSK_OK) return rc;
    sl.row_bytes = (2 * qpsk_demod_max_symbols(r->h, n_call) + 7) / 8;
    if (Framed *f = r->fr.get()) {
        // one DeModulateBytes step behind the chunk's bits, on the download
        // stream: chunk k + 1's step follows chunk k's, the order the framer's
        // state needs.  The frames stay on the device until collect_frames.
        int64_t *len = f->index, *offsets = f->index + S, *head = f->index + 2 * S;
        if ((rc = qpsk_tsc_find_device(sl.d_bits, r->bits_stride, sl.d_nb, S, f->tsc.empty() ? nullptr : f->tsc.c_str(),
                                       f->tsc_off, r->down)) ||
            (rc = qpsk_framer_dev_push(f->fr, sl.d_bits, r->bits_stride, f->tsc_off, sl.d_nb, f->rows, f->P, len)) ||
            (rc = qpsk_frames_pack_device(f->rows, f->P, len, S, sl.d_packed, f->C, offsets, head, r->down)))
            return rc;
        QPSK_HIP_TRY(hipMemcpyAsync(sl.h_index, f->index, (2 * S + 2) * sizeof(int64_t), hipMemcpyDeviceToHost, r->down));
    }
    if (!r->fr || r->fr->keep_bits) {
        QPSK_HIP_TRY(hipMemcpyAsync(sl.h_nb, sl.d_nb, S * sizeof(int64_t), hipMemcpyDeviceToHost, r->down));
        if (sl.row_bytes > 0)
            QPSK_HIP_TRY(hipMemcpy2DAsync(sl.h_bits, r->bits_stride, sl.d_bits, r->bits_stride, sl.row_bytes, S,
                                          hipMemcpyDeviceToHost, r->down));
    }
    QPSK_HIP_TRY(sl.out_done.record(r->down));
    if (ticket) *ticket = r->submitted;
    ++r->submitted;
    return QPSK_OK;
}

}  // namespace

extern "C" {

int qpsk_rx_create(qpsk_demod *h, int32_t depth, qpsk_rx **out) { return create(h, depth, QPSK_FMT_CF32, out); }
int qpsk_rx_create_cs16(qpsk_demod *h, int32_t depth, qpsk_rx **out) { return create(h, depth, QPSK_FMT_CS16, out); }
int qpsk_rx_create_fmt(qpsk_demod *h, int32_t depth, int32_t fmt, qpsk_rx **out) { return create(h, depth, fmt, out); }

int qpsk_rx_next_slot(qpsk_rx *r, float **iq, int64_t *stride_floats) {
    return next_slot(r, QPSK_FMT_CF32, reinterpret_cast<void **>(iq), stride_floats);
}
int qpsk_rx_next_slot_cs16(qpsk_rx *r, int16_t **iq, int64_t *stride_i16) {
    return next_slot(r, QPSK_FMT_CS16, reinterpret_cast<void **>(iq), stride_i16);
}
int qpsk_rx_next_slot_fmt(qpsk_rx *r, int32_t fmt, void **iq, int64_t *stride_elems) {
    return next_slot(r, fmt, iq, stride_elems);
}

int qpsk_rx_submit(qpsk_rx *r, const float *iq, int64_t stride_floats, int64_t n_samples,
                   const int64_t *lengths, int64_t *ticket) {
    return submit(r, QPSK_FMT_CF32, iq, stride_floats, n_samples, lengths, ticket);
}
int qpsk_rx_submit_cs16(qpsk_rx *r, const int16_t *iq, int64_t stride_i16, int64_t n_samples,
                        const int64_t *lengths, int64_t *ticket) {
    return submit(r, QPSK_FMT_CS16, iq, stride_i16, n_samples, lengths, ticket);
}
int qpsk_rx_submit_fmt(qpsk_rx *r, int32_t fmt, const void *iq, int64_t stride_elems, int64_t n_samples,
                       const int64_t *lengths, int64_t *ticket) {
    return submit(r, fmt, iq, stride_elems, n_samples, lengths, ticket);
}

int qpsk_rx_destroy(qpsk_rx *r) {
    if (!r) return fail(QPSK_ERR_ARGUMENT_NULL, "null ring");
    hipSetDevice(r->device);
    qpsk_demod_pipeline_wait(r->h, nullptr);
    hipStreamSynchronize(r->up);
    hipStreamSynchronize(r->down);
    const int rc = qpsk_demod_set_stream(r->h, nullptr);
    delete r;
    return rc;
}

int qpsk_rx_collect(qpsk_rx *r, uint8_t *bits, int64_t bits_stride_bytes, int64_t *n_bits,
                    int64_t *ticket) {
    if (!r || !bits || !n_bits) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    if (r->fr && !r->fr->keep_bits) return fail(QPSK_ERR_STATE, kNoBits);
    if (r->collected == r->submitted) return fail(QPSK_ERR_STATE, "no chunk outstanding");
    Slot &sl = r->slots[r->collected % r->depth];
    if (bits_stride_bytes < sl.row_bytes)
        return fail(QPSK_ERR_ARGUMENT, "bits_stride_bytes smaller than 2*max_symbols/8");
    QPSK_HIP_TRY(hipSetDevice(r->device));
    QPSK_HIP_TRY(sl.out_done.sync());
    copy_bits(r, sl, bits, bits_stride_bytes, n_bits);
    if (ticket) *ticket = r->collected;
    ++r->collected;
    return QPSK_OK;
}

int qpsk_rx_attach_framer(qpsk_rx *r, const uint8_t *start, int32_t n_start, const uint8_t *end, int32_t n_end,
                          const char *tsc, int64_t ring_capacity, int64_t max_frame_bytes,
                          int64_t chunk_frame_bytes, int32_t keep_bits) {
    if (!r || !start || !end) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    if (max_frame_bytes <= 0) return fail(QPSK_ERR_ARGUMENT, "max_frame_bytes must be positive");
    if (chunk_frame_bytes < 0) return fail(QPSK_ERR_ARGUMENT, "chunk_frame_bytes must not be negative");
    if (r->fr) return fail(QPSK_ERR_STATE, "the ring has a framer already");
    if (r->collected != r->submitted) return fail(QPSK_ERR_STATE, "attach a framer with no chunk outstanding");
    const size_t S = static_cast<size_t>(r->S);
    std::unique_ptr<Framed> f(new Framed);
    f->P = (max_frame_bytes + 15) / 16 * 16;
    f->C = chunk_frame_bytes ? (chunk_frame_bytes + 15) / 16 * 16 : static_cast<int64_t>(S) * f->P;
    f->keep_bits = keep_bits != 0;
    if (tsc) f->tsc = tsc;
    int rc = qpsk_framer_dev_create(r->S, start, n_start, end, n_end, ring_capacity, r->device, &f->fr);
    if (rc == QPSK_OK) rc = qpsk_framer_dev_set_stream(f->fr, r->down);
    if (rc != QPSK_OK) return rc;
    QPSK_HIP_TRY(hipSetDevice(r->device));
    QPSK_HIP_TRY(f->fetch.create(hipStreamNonBlocking));
    QPSK_HIP_TRY(f->rows.alloc(S * static_cast<size_t>(f->P)));
    QPSK_HIP_TRY(f->tsc_off.alloc(S));
    QPSK_HIP_TRY(f->index.alloc(2 * S + 2));
    // packed buffers of their own, so that a failed attach leaves the slots as they were
    std::vector<qpsk::DevBuf<uint8_t>> d_packed(r->depth);
    std::vector<qpsk::PinnedBuf<uint8_t>> h_packed(r->depth);
    std::vector<qpsk::PinnedBuf<int64_t>> h_index(r->depth);
    for (int k = 0; k < r->depth; ++k) {
        QPSK_HIP_TRY(d_packed[k].alloc(static_cast<size_t>(f->C)));
        QPSK_HIP_TRY(h_packed[k].alloc(static_cast<size_t>(f->C)));
        QPSK_HIP_TRY(h_index[k].alloc(2 * S + 2));
    }
    for (int k = 0; k < r->depth; ++k) {
        r->slots[k].d_packed.swap(d_packed[k]);
        r->slots[k].h_packed.swap(h_packed[k]);
        r->slots[k].h_index.swap(h_index[k]);
    }
    r->fr = std::move(f);
    return QPSK_OK;
}

int qpsk_rx_set_markers(qpsk_rx *r, const uint8_t *start, int32_t n_start, const uint8_t *end, int32_t n_end) {
    if (!r || !start || !end) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    if (!r->fr) return fail(QPSK_ERR_STATE, kNoFramer);
    return qpsk_framer_dev_set_markers(r->fr->fr, start, n_start, end, n_end);
}

int64_t qpsk_rx_frames_bytes(const qpsk_rx *r) { return r && r->fr ? r->fr->C : 0; }

int qpsk_rx_collect_frames(qpsk_rx *r, uint8_t *frames, int64_t frames_cap, int64_t *frame_offset,
                           int64_t *frame_len, uint8_t *bits, int64_t bits_stride_bytes, int64_t *n_bits,
                           int64_t *ticket) {
    if (!r || !frames || !frame_offset || !frame_len) return fail(QPSK_ERR_ARGUMENT_NULL, "null argument");
    if (!r->fr) return fail(QPSK_ERR_STATE, kNoFramer);
    if ((bits || n_bits) && !r->fr->keep_bits) return fail(QPSK_ERR_STATE, kNoBits);
    if (!bits != !n_bits) return fail(QPSK_ERR_ARGUMENT_NULL, "bits and n_bits go together");
    if (r->collected == r->submitted) return fail(QPSK_ERR_STATE, "no chunk outstanding");
    Slot &sl = r->slots[r->collected % r->depth];
    if (bits && bits_stride_bytes < sl.row_bytes)
        return fail(QPSK_ERR_ARGUMENT, "bits_stride_bytes smaller than 2*max_symbols/8");
    QPSK_HIP_TRY(hipSetDevice(r->device));
    QPSK_HIP_TRY(sl.out_done.sync());
    const int S = r->S;
    const int64_t total = sl.h_index[2 * S], flags = sl.h_index[2 * S + 1];
    if (frames_cap < total)
        return fail(QPSK_ERR_ARGUMENT, "frames_cap smaller than the chunk's frames (" + std::to_string(total) + " bytes)");
    if (total > 0) {
        // exactly the frames' bytes, on a stream of their own: the download
        // stream may hold the next chunks' work already
        QPSK_HIP_TRY(hipMemcpyAsync(sl.h_packed, sl.d_packed, static_cast<size_t>(total), hipMemcpyDeviceToHost,
                                    r->fr->fetch));
        QPSK_HIP_TRY(hipStreamSynchronize(r->fr->fetch));
        std::memcpy(frames, sl.h_packed, static_cast<size_t>(total));
    }
    std::memcpy(frame_len, sl.h_index, S * sizeof(int64_t));
    std::memcpy(frame_offset, sl.h_index + S, S * sizeof(int64_t));
    if (bits) copy_bits(r, sl, bits, bits_stride_bytes, n_bits);
    if (ticket) *ticket = r->collected;
    ++r->collected;
    if (flags)
        return fail(QPSK_ERR_CAPACITY, (flags & QPSK_FRAMES_TRUNCATED)
                                           ? "a frame is longer than max_frame_bytes (truncated)"
                                           : "the chunk's frames exceed chunk_frame_bytes (dropped)");
    return QPSK_OK;
}

int qpsk_rx_reset_streams(qpsk_rx *r, const int32_t *streams, int32_t n) {
    if (!r) return fail(QPSK_ERR_ARGUMENT_NULL, "null ring");
    if (n == 0) return QPSK_OK;
    int rc;
    if ((rc = qpsk_stream_list_check(r->S, streams, n))) return rc;
    QPSK_HIP_TRY(hipSetDevice(r->device));
    // the outstanding chunks' framer steps have run before a row is rewritten
    // (the handle's reset waits for its own queued calls)
    QPSK_HIP_TRY(hipStreamSynchronize(r->down));
    if ((rc = qpsk_demod_reset_streams(r->h, streams, n))) return rc;
    return r->fr ? qpsk_framer_dev_reset_streams(r->fr->fr, streams, n) : QPSK_OK;
}

}  // extern "C"
