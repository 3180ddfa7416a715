// aq_host_mem.h -- what the host side owns on the HIP runtime: device buffers, pinned host buffers, events and
// streams, each freed by its destructor. Move-only; a buffer knows its element count, and a device buffer may
// add its bytes to a counter (aq_ctx::dev_bytes, what aq_ctx_device_bytes reports). The only hipFree /
// hipHostFree of the library are here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <utility>

namespace aq {

template <typename T>
class DevBuf {
public:
    explicit DevBuf(unsigned long long* counter = nullptr) : counter_(counter) {}
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_), counter_(o.counter_) { o.p_ = nullptr, o.n_ = 0; }
    DevBuf& operator=(DevBuf&&) = delete;
    ~DevBuf() { reset(); }
    // count elements (what was held is freed first), zeroed if asked
    hipError_t alloc(size_t count, bool zero) {
        reset();
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&p_), count * sizeof(T));
        if (e != hipSuccess) {
            p_ = nullptr;
            return e;
        }
        n_ = count;
        if (counter_) *counter_ += count * sizeof(T);
        return zero ? hipMemset(p_, 0, count * sizeof(T)) : hipSuccess;
    }
    // at least count elements; the contents are not kept. A failure leaves the buffer empty.
    hipError_t grow(size_t count) { return n_ >= count ? hipSuccess : alloc(count, false); }
    void reset() {
        if (!p_) return;
        (void)hipFree(p_);
        if (counter_) *counter_ -= n_ * sizeof(T);
        p_ = nullptr, n_ = 0;
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t count() const { return n_; }

private:
    T* p_ = nullptr;
    size_t n_ = 0;
    unsigned long long* counter_;
};

template <typename T>
class PinBuf {
public:
    PinBuf() = default;
    PinBuf(PinBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
    PinBuf& operator=(PinBuf&&) = delete;
    ~PinBuf() { reset(); }
    hipError_t alloc(size_t count, bool zero, unsigned flags = hipHostMallocDefault) {
        reset();
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p_), count * sizeof(T), flags);
        if (e != hipSuccess) {
            p_ = nullptr;
            return e;
        }
        n_ = count;
        if (zero) memset(p_, 0, count * sizeof(T));
        return hipSuccess;
    }
    hipError_t grow(size_t count) { return n_ >= count ? hipSuccess : alloc(count, false); }
    void reset() {
        if (p_) (void)hipHostFree(p_);
        p_ = nullptr, n_ = 0;
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    T* operator->() const { return p_; }
    size_t count() const { return n_; }

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
    Event& operator=(Event&& o) noexcept { std::swap(e, o.e); return *this; }
    ~Event() { if (e) (void)hipEventDestroy(e); }
    hipError_t create(unsigned flags = hipEventDefault) { return hipEventCreateWithFlags(&e, flags); }
    operator hipEvent_t() const { return e; }
};

struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    operator hipStream_t() const { return s; }
};

}  // namespace aq
