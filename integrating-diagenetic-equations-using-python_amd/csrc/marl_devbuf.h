// A device allocation that frees itself (host side only).  Move-only.  Work that uses the buffer may still be in flight on `stream`
// when an error return drops it, so the destructor waits for the stream first (a no-op after the caller's own last synchronise).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

namespace marl {

struct DevBuf {
    void* p = nullptr;
    hipStream_t stream = nullptr;
    explicit DevBuf(hipStream_t s = nullptr) : stream(s) {}
    DevBuf(DevBuf&& o) noexcept : p(o.p), stream(o.stream) { o.p = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) { release(); p = o.p; stream = o.stream; o.p = nullptr; }
        return *this;
    }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    hipError_t alloc(size_t bytes) { release(); return hipMalloc(&p, bytes); }
    void release()
    {
        if (!p) return;
        (void)hipStreamSynchronize(stream);
        (void)hipFree(p);
        p = nullptr;
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

}  // namespace marl
