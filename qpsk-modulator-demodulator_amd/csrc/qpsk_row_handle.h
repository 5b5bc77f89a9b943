// qpsk_row_handle.h -- what the handles of the test-bench stages that take rows
// of samples (qpsk_channel, qpsk_path, qpsk_pfb) have in common: the device,
// the stream, the buffer of a call's checked lengths and the two staging
// buffers of a host-memory call, with the steps every such handle takes in the
// same way.  A stage derives its handle from RowHandle, adds its state, and
// composes the steps in its own entry points, which keep the checks, the order
// and the kernels that are its own ("The test-bench stages' shared
// pieces").  Also the argument checks the three apply calls share.  Private,
// HIP host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "qpsk_demod.h"
#include "qpsk_device.h"
#include "qpsk_internal.h"
#include "qpsk_quantise.h"

namespace qpsk {

// A base's members outlive a derived handle's: the stream, declared in front
// of the buffers here, is destroyed after every buffer, a stage's own included.
struct RowHandle {
    int device = 0;
    Stream stream;
    DevBuf<int64_t> d_len;         // [rows]: a call's checked lengths
    DevBuf<uint8_t> d_in, d_out;   // host calls: 16-byte-pitched rows

    // the first links of a create's chain: the device current, an own stream, d_len
    hipError_t open(int dev, int rows) {
        device = dev;
        hipError_t e = hipSetDevice(dev);
        if (e == hipSuccess) e = stream.create(hipStreamNonBlocking);
        return e == hipSuccess ? d_len.alloc(rows) : e;
    }

    int set_stream(void *hip_stream) {
        DeviceGuard guard;
        QPSK_HIP_TRY(hipSetDevice(device));
        QPSK_HIP_TRY(hipStreamSynchronize(stream));
        QPSK_HIP_TRY(stream.rebind(hip_stream));
        return QPSK_OK;
    }

    // bytes between the state on the device and a host blob, behind the calls
    // queued on the stream; complete on return
    int state_out(void *host_buf, const void *d_state, int64_t bytes) { return state_copy(host_buf, d_state, bytes, hipMemcpyDeviceToHost); }
    int state_in(void *d_state, const void *host_buf, int64_t bytes) { return state_copy(d_state, host_buf, bytes, hipMemcpyHostToDevice); }

    // the kernels read the lengths the host checked: *dev is d_len behind the
    // upload, or stays nullptr without lengths
    int upload_lengths(const int64_t *lengths, int rows, const int64_t **dev) {
        if (!lengths) return QPSK_OK;
        QPSK_HIP_TRY(hipMemcpyAsync(d_len, lengths, rows * sizeof(int64_t), hipMemcpyHostToDevice, stream));
        *dev = d_len;
        return QPSK_OK;
    }

    // The staging steps of a host-memory call: `rows` rows of n samples of
    // elem_bytes elements, pitched to 16 bytes.  stage_out only makes room, and
    // what a stage uploads of `out` first is its own rule; stage_in uploads the
    // caller's rows.  A call takes stage_out first: no copy from the caller's
    // memory is queued while an allocation can still refuse the call.  *dev and
    // *stride (elements) are what the kernel takes.  label: what alloc_status
    // names when the buffer cannot grow.
    int stage_in(const char *label, const void *in, int64_t stride_in, int64_t elem_bytes, int64_t n, int64_t rows,
                 const void **dev, int64_t *stride) {
        const int64_t pitch = row_pitch(n, elem_bytes);
        int rc;
        if ((rc = alloc_status(d_in.grow(static_cast<size_t>(rows) * pitch), label))) return rc;
        QPSK_HIP_TRY(hipMemcpy2DAsync(d_in, pitch, in, stride_in * elem_bytes, 2 * n * elem_bytes, rows, hipMemcpyHostToDevice,
                                      stream));
        *dev = d_in;
        *stride = pitch / elem_bytes;
        return QPSK_OK;
    }
    template <typename T>
    int stage_out(const char *label, int64_t elem_bytes, int64_t n, int64_t rows, T **dev, int64_t *stride) {
        const int64_t pitch = row_pitch(n, elem_bytes);
        int rc;
        if ((rc = alloc_status(d_out.grow(static_cast<size_t>(rows) * pitch), label))) return rc;
        *dev = reinterpret_cast<T *>(d_out.get());
        *stride = pitch / elem_bytes;
        return QPSK_OK;
    }

  private:
    static int64_t row_pitch(int64_t n, int64_t elem_bytes) { return (2 * n * elem_bytes + 15) / 16 * 16; }
    int state_copy(void *dst, const void *src, int64_t bytes, hipMemcpyKind kind) {
        DeviceGuard guard;
        QPSK_HIP_TRY(hipSetDevice(device));
        QPSK_HIP_TRY(hipMemcpyAsync(dst, src, bytes, kind, stream));
        QPSK_HIP_TRY(hipStreamSynchronize(stream));
        return QPSK_OK;
    }
};

// every *_destroy: waits for what is queued, then releases the handle on its device
template <typename H>
int row_handle_destroy(H *h) {
    if (!h) return QPSK_OK;
    DeviceGuard guard;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    delete h;
    return QPSK_OK;
}

// The argument checks the apply calls share, in their one order: known formats,
// a fixed norm, a known mem, scale_in where the input is not CF32, scale_out.
// stage: the noun of the text ("the path does not normalise ...").
inline int check_row_formats(const char *stage, int fmt_in, float scale_in, int fmt_out, int norm_out, float scale_out,
                             int mem) {
    if (!fmt_known(fmt_in) || !fmt_known(fmt_out)) return fail(QPSK_ERR_ARGUMENT, "unknown sample format");
    if (norm_out != QPSK_MOD_NORM_FIXED)
        return fail(QPSK_ERR_ARGUMENT, norm_out == QPSK_MOD_NORM_PEAK
                                           ? std::string("the ") + stage + " does not normalise rows to their peak (a "
                                             "second pass): QPSK_MOD_NORM_FIXED only"
                                           : "unknown norm");
    if (mem != QPSK_MEM_HOST && mem != QPSK_MEM_DEVICE) return fail(QPSK_ERR_ARGUMENT, "unknown mem");
    if (fmt_in != QPSK_FMT_CF32 && !quant_scale_ok(scale_in))
        return fail(QPSK_ERR_OUT_OF_RANGE, "scale_in must be finite and > 0");
    if (!quant_scale_ok(scale_out)) return fail(QPSK_ERR_OUT_OF_RANGE, "scale_out must be finite and > 0");
    return QPSK_OK;
}

}  // namespace qpsk
