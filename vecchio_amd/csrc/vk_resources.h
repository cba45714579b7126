// vk_resources.h — the device resources a handle of the C ABI owns: device buffers, pinned host buffers, events and streams as
// move-only members, so that deleting a handle releases everything in it and a resource added to a handle cannot be forgotten in a
// hand-kept free list.
//
// Part of vk_api.hip's translation unit (included behind its fail() and HIP_TRY).  Every object remembers the device it was made on: its
// destructor makes that device current, releases the resource and clears HIP's sticky error.  Nothing here waits: a handle whose work
// may still be in flight synchronises before it lets go (destroy_one, progress_free, temporal_free).
#ifndef VK_RESOURCES_H
#define VK_RESOURCES_H

#ifdef VK_DEBUG_LIB
#include <atomic>
#endif

namespace vkr {

enum { LIVE_DEVICE_BUFFER = 0, LIVE_PINNED_BUFFER = 1, LIVE_EVENT = 2, LIVE_STREAM = 3 };
#ifdef VK_DEBUG_LIB
// the debug library counts the live objects of each kind (vk_debug_live_objects: the leak check of tests/test_gpu_lifecycle.py)
inline std::atomic<uint64_t> g_live[4];
inline void live(int kind, int d) { g_live[kind] += (uint64_t)(int64_t)d; }
#else
inline void live(int, int) {}
#endif

// One HIP handle H, released by FREE on the device that was current when it was adopted.
template <class H, int KIND, hipError_t (*FREE)(H)>
class Owned {
public:
    Owned() = default;
    Owned(Owned &&o) noexcept : h_(o.h_), device_(o.device_) { o.h_ = nullptr; }
    Owned &operator=(Owned &&o) noexcept {
        if (this != &o) { reset(); h_ = o.h_; device_ = o.device_; o.h_ = nullptr; }
        return *this;
    }
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    ~Owned() { reset(); }
    void reset() {
        if (!h_) return;
        (void)hipSetDevice(device_);
        (void)FREE(h_);
        (void)hipGetLastError();
        h_ = nullptr;
        live(KIND, -1);
    }
    int device() const { return device_; }

protected:
    void adopt(H h) { h_ = h; (void)hipGetDevice(&device_); live(KIND, +1); }
    H h_ = nullptr;
    int device_ = 0;
};

// Device memory of the device that is current at its allocation.
template <class T = uint8_t>
class DeviceBuffer : public Owned<void *, LIVE_DEVICE_BUFFER, hipFree> {
public:
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer &&o) noexcept : Owned(std::move(o)), bytes_(o.bytes_) { o.bytes_ = 0; }
    DeviceBuffer &operator=(DeviceBuffer &&o) noexcept {
        Owned::operator=(std::move(o)); bytes_ = o.bytes_; o.bytes_ = 0;
        return *this;
    }
    T *get() const { return static_cast<T *>(h_); }
    operator T *() const { return get(); }
    size_t bytes() const { return bytes_; }
    // an empty buffer's first allocation (16 bytes at least), HIP's own verdict: for the callers that map it to a code of their own
    hipError_t alloc(size_t bytes) {
        void *p = nullptr;
        hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
        if (e == hipSuccess) { adopt(p); bytes_ = bytes; }
        return e;
    }
    // grows the buffer (never shrinks; the contents are NOT kept: freed, then allocated); its device must be current
    int ensure(size_t need) {
        if (need <= bytes_ && h_) return VK_OK;
        if (h_) {
            HIP_TRY(hipFree(h_));
            h_ = nullptr; bytes_ = 0; live(LIVE_DEVICE_BUFFER, -1);
        }
        HIP_TRY(alloc(need));
        return VK_OK;
    }

private:
    size_t bytes_ = 0;
};

// Pinned host memory (hipHostMalloc), zeroed.
template <class T>
class PinnedBuffer : public Owned<void *, LIVE_PINNED_BUFFER, hipHostFree> {
public:
    T *get() const { return static_cast<T *>(h_); }
    operator T *() const { return get(); }
    hipError_t alloc(size_t bytes) {
        void *p = nullptr;
        hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
        if (e == hipSuccess) { memset(p, 0, bytes); adopt(p); }
        return e;
    }
};

// An event, made on first use: timed (the default) or with hipEventDisableTiming, as its site asks.
class Event : public Owned<hipEvent_t, LIVE_EVENT, hipEventDestroy> {
public:
    operator hipEvent_t() const { return h_; }
    int create(unsigned flags = hipEventDefault) {
        if (h_) return VK_OK;
        hipEvent_t e = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&e, flags));
        adopt(e);
        return VK_OK;
    }
};

// A non-blocking stream.
class Stream : public Owned<hipStream_t, LIVE_STREAM, hipStreamDestroy> {
public:
    operator hipStream_t() const { return h_; }
    int create() {
        hipStream_t s = nullptr;
        HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        adopt(s);
        return VK_OK;
    }
};

}  // namespace vkr
#endif
