// rtgo_owners.h -- host-side owners of the context's HIP allocations (rtgo_capi.hip).  One alloc is one hipMalloc (or hipHostMalloc), freed
// by the next alloc, reset, move-assignment or the destructor: no pooling, no caching, no sharing.  Whoever drops an owner has made the
// device current and finished the work that still reads it, as for any hipFree.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace rtgo {

template <class T, bool kPinned>
class HipArray {
public:
    HipArray() = default;
    HipArray(const HipArray&) = delete;
    HipArray& operator=(const HipArray&) = delete;
    HipArray(HipArray&& o) noexcept : p_(o.p_), n_(o.n_)
    {
        o.p_ = nullptr;
        o.n_ = 0;
    }
    HipArray& operator=(HipArray&& o) noexcept
    {
        if (this != &o) {
            reset();
            p_ = o.p_;
            n_ = o.n_;
            o.p_ = nullptr;
            o.n_ = 0;
        }
        return *this;
    }
    ~HipArray() { reset(); }

    // frees what it holds, then allocates n elements (uninitialised); holds nothing when that fails
    hipError_t alloc(size_t n)
    {
        reset();
        void* p = nullptr;
        const hipError_t e = kPinned ? hipHostMalloc(&p, n * sizeof(T), hipHostMallocDefault) : hipMalloc(&p, n * sizeof(T));
        if (e == hipSuccess) {
            p_ = static_cast<T*>(p);
            n_ = n;
        }
        return e;
    }
    // alloc(n), then an asynchronous copy of host[0, n) on `stream`
    hipError_t upload(const T* host, size_t n, hipStream_t stream)
    {
        hipError_t e = alloc(n);
        if (e == hipSuccess) e = hipMemcpyAsync(p_, host, n * sizeof(T), hipMemcpyHostToDevice, stream);
        return e;
    }
    void reset()
    {
        if (p_) (void)(kPinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        n_ = 0;
    }
    T* get() const { return p_; }
    size_t size() const { return n_; }

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

template <class T>
using DeviceArray = HipArray<T, false>;   // device memory
template <class T>
using PinnedArray = HipArray<T, true>;    // page-locked host memory

// an event created on first use and destroyed with its owner
class LazyEvent {
public:
    LazyEvent() = default;
    LazyEvent(const LazyEvent&) = delete;
    LazyEvent& operator=(const LazyEvent&) = delete;
    ~LazyEvent()
    {
        if (e_) (void)hipEventDestroy(e_);
    }
    hipEvent_t get() const { return e_; }
    hipError_t create(unsigned flags) { return hipEventCreateWithFlags(&e_, flags); }

private:
    hipEvent_t e_ = nullptr;
};

}  // namespace rtgo
