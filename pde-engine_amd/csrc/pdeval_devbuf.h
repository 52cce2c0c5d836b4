// pdeval_devbuf.h -- DevBuf<T>, the owning device buffer of the host side (the validator context
// in pdeval.hip, its batch scratch in pdeval_scratch.h, the foliation entry points).  Nothing but
// hipMalloc, hipFree, hipMemset and hipGetLastError; a host program that defines PD_HOST_SIM
// supplies those four, hipError_t and hipSuccess itself (tests/hostsim/guard_ctx_scratch.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#ifndef PD_HOST_SIM
#include <hip/hip_runtime_api.h>
#endif

namespace pd {

// An owning device buffer of `cap` elements; the destructor frees, on the device that is current
// then.  It copies nothing when it grows, in either of two ways: reserve() allocates the new
// block before it frees the old one and keeps the old one on failure (a registry stays usable);
// replace() frees first, for batch-sized scratch whose peak memory must not double while it
// grows, and is empty on failure.
template <class T>
struct DevBuf {
    T* p = nullptr;
    int64_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { (void)hipFree(p); }
    operator T*() const { return p; }
    // room for n elements; false (the old block and capacity untouched, no HIP error left
    // pending) when the allocation fails
    bool reserve(int64_t n) {
        if (n <= cap) return true;
        T* q = nullptr;
        if (hipMalloc((void**)&q, (size_t)n * sizeof(T)) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        (void)hipFree(p);
        p = q;
        cap = n;
        return true;
    }
    // Room for n elements, the old block freed before the new one is allocated.  `epoch` counts
    // the moves of every buffer a captured graph may hold (pdeval.hip buf_epoch): it advances
    // whenever p changes, here and in release(), so no caller has to remember to.  On failure
    // (of the allocation, or of the zeroing asked for) the buffer is empty and no HIP error is
    // left pending.
    hipError_t replace(int64_t n, uint64_t& epoch, bool zeroed = false) {
        if (n <= cap) return hipSuccess;
        ++epoch;
        drop();
        hipError_t e = hipMalloc((void**)&p, (size_t)n * sizeof(T));
        if (e == hipSuccess && zeroed) e = hipMemset(p, 0, (size_t)n * sizeof(T));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            drop();
            return e;
        }
        cap = n;
        return hipSuccess;
    }
    void release(uint64_t& epoch) {
        if (p) ++epoch;
        drop();
    }
    void drop() {
        (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    void swap(DevBuf& o) {
        std::swap(p, o.p);
        std::swap(cap, o.cap);
    }
};

}  // namespace pd
