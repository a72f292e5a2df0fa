// Host-side plumbing shared by the stateful handle objects of include/tokenhmr_hip.h: thmr_cropper (crop.hip), thmr_renderer (render.hip),
// thmr_jpeg (jpeg.hip), thmr_jpeg_encoder (jpegenc.hip) and thmr_png (png.hip).  Host only: no kernel includes this.  The rules every
// such object keeps:
//   * an entry point checks its arguments before it touches the device, so a refusal costs no HIP call;
//   * a grow-only buffer is re-allocated only behind a synchronisation of the caller's stream (grow_synced): earlier launches may
//     still read the old allocation;
//   * the last error is kept per handle (thmr_X_last_error(h)) and per thread (thmr_X_last_error(NULL)).
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>
#include <string>

#include "../../include/tokenhmr_hip.h"

int fail(int code, const std::string& msg);      // engine.hip: writes the string behind thmr_last_error(NULL)

// The error strings of one handle family, declared `thread_local ErrorSink<thmr_X>` by its file.  The handle type H keeps its own copy
// in `std::string err`; `h` may be null (create, and the entries that check their arguments before the handle), then only the thread's
// string is written.
template <typename H>
struct ErrorSink {
    bool also_global = false;     // the JPEG family: its stateless entries report through thmr_last_error(NULL) as well
    std::string last;

    int fail(H* h, int code, const std::string& m) {
        if (h) h->err = m;
        last = m;
        return also_global ? ::fail(code, m) : code;
    }
    int invalid(H* h, const std::string& m) { return fail(h, THMR_ERR_INVALID, m); }
    int hip(H* h, const char* what, hipError_t e) { return fail(h, THMR_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }
    const char* read(const H* h) const { return h ? h->err.c_str() : last.c_str(); }
};

inline bool check_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && device >= 0 && device < ndev) return true;
    (void)hipGetLastError();
    return false;
}

// thmr_X_create / _destroy of a family whose handle starts empty (`int device` and grow-only buffers): the cropper, the JPEG decoder
// and the two image writers.  no_device_text: what the refusal says where `device` is no HIP device.
template <typename H>
int handle_create(int32_t device, H** out, ErrorSink<H>& sink, const char* no_device_text) {
    if (!out) return sink.invalid(nullptr, "null out");
    *out = nullptr;
    if (!check_device(device)) return sink.fail(nullptr, THMR_ERR_HIP, no_device_text);
    H* h = new H();
    h->device = device;
    *out = h;
    return 0;
}
template <typename H>
void handle_destroy(H* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    delete h;          // the buffers free themselves
}

// What a batch entry does once its arguments and the handle are checked: selects the handle's device and asks whether `st` is being
// captured.  0, or the status of the HIP failure, reported through the sink.  What a capture means is the caller's business.
template <typename H>
int enter_stream(H* h, hipStream_t st, ErrorSink<H>& sink, bool* capturing) {
    hipError_t e;
    if ((e = hipSetDevice(h->device)) != hipSuccess) return sink.hip(h, "hipSetDevice", e);
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if ((e = hipStreamIsCapturing(st, &cap)) != hipSuccess) return sink.hip(h, "hipStreamIsCapturing", e);
    *capturing = cap != hipStreamCaptureStatusNone;
    return 0;
}

// One grow-only HIP allocation, untyped: device memory, or (pinned) page-locked host memory.  Freed by release() or the destructor; the
// owner selects the device first (thmr_X_destroy: hipSetDevice, then delete).  Handles hold the typed forms below.
struct HipBuf {
    void* mem = nullptr;
    size_t bytes = 0;
    const bool pinned;

    explicit HipBuf(bool pinned_) : pinned(pinned_) {}
    HipBuf(const HipBuf&) = delete;
    HipBuf& operator=(const HipBuf&) = delete;
    ~HipBuf() { release(); }
    void release() {
        if (mem) (void)(pinned ? hipHostFree(mem) : hipFree(mem));
        mem = nullptr; bytes = 0;
    }
    // frees and re-allocates only when `need` exceeds the capacity; a failure leaves the buffer empty
    hipError_t reserve_bytes(size_t need, size_t bytes_when_grown) {
        if (need <= bytes) return hipSuccess;
        release();
        const hipError_t e = pinned ? hipHostMalloc(&mem, bytes_when_grown, hipHostMallocDefault) : hipMalloc(&mem, bytes_when_grown);
        if (e == hipSuccess) bytes = bytes_when_grown; else mem = nullptr;
        return e;
    }
};

// One request of grow_synced: `buf` must hold `need` bytes and, where it has to grow for that, gets `bytes_when_grown` (the call site's
// growth policy); `what` names the allocation in the error message.
struct Grow {
    HipBuf& buf;
    size_t need, bytes_when_grown;
    const char* what;
};

// The typed buffers: DevBuf<T> in device memory, PinnedBuf<T> in page-locked host memory.  Sizes are in elements.
template <typename T, bool Pinned>
struct TypedBuf : HipBuf {
    TypedBuf() : HipBuf(Pinned) {}
    T* ptr() const { return static_cast<T*>(mem); }
    operator T*() const { return ptr(); }      // a kernel or copy argument
    hipError_t reserve(size_t n, size_t capacity_when_grown) { return reserve_bytes(sizeof(T) * n, sizeof(T) * capacity_when_grown); }
    Grow want(size_t n, size_t capacity_when_grown, const char* what) { return {*this, sizeof(T) * n, sizeof(T) * capacity_when_grown, what}; }
};
template <typename T> using DevBuf = TypedBuf<T, false>;
template <typename T> using PinnedBuf = TypedBuf<T, true>;

inline bool must_grow(std::initializer_list<Grow> reqs) {
    for (const Grow& g : reqs)
        if (g.need > g.buf.bytes) return true;
    return false;
}

// The one way a handle's buffers grow during a call: nothing happens when every request fits; otherwise the stream is synchronised
// once (earlier launches may still use the old allocations) and the requests are served in order.  `what` names the HIP call that
// failed, and is null on success.
inline hipError_t grow_synced(hipStream_t st, std::initializer_list<Grow> reqs, const char*& what) {
    what = nullptr;
    if (!must_grow(reqs)) return hipSuccess;
    what = "hipStreamSynchronize";
    if (hipError_t e = hipStreamSynchronize(st)) return e;
    for (const Grow& g : reqs) {
        what = g.what;
        if (hipError_t e = g.buf.reserve_bytes(g.need, g.bytes_when_grown)) return e;
    }
    return hipSuccess;
}
