// qpsk_device.h -- the four owners of GPU resources behind the host code: device
// memory, pinned host memory, an event and a stream.  A handle holds them as
// members, so its destructor releases them (in reverse order of declaration,
// on the device its body made current) and a set-up that fails half way leaks
// nothing.  Move-only.  And DeviceGuard, which keeps an entry point from
// changing its caller's current device.  Every call that can fail returns the hipError_t; the
// file that makes the call gives it that file's error text.  Private, host-only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace qpsk {

// Memory from hipMalloc (DevBuf) or hipHostMalloc (PinnedBuf).  Reads as the T*
// it holds: kernel arguments, copies and pointer arithmetic take it as it is.
template <typename T, bool Pinned>
class Buf {
  public:
    Buf() = default;
    Buf(Buf &&o) noexcept { swap(o); }
    Buf &operator=(Buf &&o) noexcept {
        if (this != &o) reset(), swap(o);
        return *this;
    }
    ~Buf() { reset(); }

    operator T *() const { return p_; }
    T *get() const { return p_; }
    size_t bytes() const { return bytes_; }
    void swap(Buf &o) noexcept {
        std::swap(p_, o.p_);
        std::swap(bytes_, o.bytes_);
    }
    void reset() { adopt(nullptr, 0); }
    // frees what it holds and takes over p, memory that the same free call
    // releases (signal memory from hipExtMallocWithFlags)
    void adopt(T *p, size_t bytes) {
        if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = p;
        bytes_ = bytes;
    }
    // count elements, unless it holds memory already (a set-up that runs again
    // keeps what it made); none for count 0
    hipError_t alloc(size_t count) { return p_ || count == 0 ? hipSuccess : raw(count * sizeof(T)); }
    // at least `bytes` bytes afterwards.  A buffer too small is freed first and
    // then allocated anew (the two never exist together): what it held is
    // dropped, and nothing queued may still use it
    hipError_t grow(size_t bytes) {
        if (bytes <= bytes_) return hipSuccess;
        reset();
        return raw(bytes);
    }

  private:
    hipError_t raw(size_t bytes) {   // empty on entry
        void *q = nullptr;
        const hipError_t e = Pinned ? hipHostMalloc(&q, bytes) : hipMalloc(&q, bytes);
        if (e == hipSuccess) p_ = static_cast<T *>(q), bytes_ = bytes;
        return e;
    }
    T *p_ = nullptr;
    size_t bytes_ = 0;
};
template <typename T>
using DevBuf = Buf<T, false>;
template <typename T>
using PinnedBuf = Buf<T, true>;

// An event without timing that knows whether it has been recorded: waiting
// for one that never was is no HIP call at all.
class Event {
  public:
    Event() = default;
    Event(Event &&o) noexcept : e_(std::exchange(o.e_, nullptr)), recorded_(std::exchange(o.recorded_, false)) {}
    ~Event() {
        if (e_) (void)hipEventDestroy(e_);
    }
    // made once
    hipError_t ensure() { return e_ ? hipSuccess : hipEventCreateWithFlags(&e_, hipEventDisableTiming); }
    hipError_t record(hipStream_t s) {
        const hipError_t e = hipEventRecord(e_, s);
        recorded_ = recorded_ || e == hipSuccess;
        return e;
    }
    bool recorded() const { return recorded_; }
    hipError_t wait(hipStream_t s) const { return recorded_ ? hipStreamWaitEvent(s, e_, 0) : hipSuccess; }
    hipError_t sync() const { return recorded_ ? hipEventSynchronize(e_) : hipSuccess; }

  private:
    hipEvent_t e_ = nullptr;
    bool recorded_ = false;
};

// A stream the handle made (and destroys) or one its caller lent it (never
// destroyed here).  Reads as the hipStream_t.
class Stream {
  public:
    Stream() = default;
    Stream(Stream &&o) noexcept : s_(std::exchange(o.s_, nullptr)), own_(std::exchange(o.own_, false)) {}
    ~Stream() {
        if (own_ && s_) (void)hipStreamDestroy(s_);
    }
    operator hipStream_t() const { return s_; }
    // an own stream, unless it holds one already
    hipError_t create(unsigned flags) { return s_ ? hipSuccess : made(hipStreamCreateWithFlags(&s_, flags)); }
    hipError_t create(unsigned flags, int priority) {
        return s_ ? hipSuccess : made(hipStreamCreateWithPriority(&s_, flags, priority));
    }
    // every set_stream entry point, behind its own synchronisation: the
    // caller's stream replaces (and ends) an own one; nullptr goes back from a
    // borrowed stream to an own one
    hipError_t rebind(void *hip_stream) {
        if (!hip_stream) return own_ ? hipSuccess : made(hipStreamCreateWithFlags(&s_, hipStreamNonBlocking));
        if (own_) (void)hipStreamDestroy(s_);
        s_ = static_cast<hipStream_t>(hip_stream);
        own_ = false;
        return hipSuccess;
    }

  private:
    hipError_t made(hipError_t e) {
        own_ = e == hipSuccess;
        return e;
    }
    hipStream_t s_ = nullptr;
    bool own_ = false;
};

// the caller's current device, put back when a call returns
struct DeviceGuard {
    int prev = -1;
    DeviceGuard() {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

}  // namespace qpsk
