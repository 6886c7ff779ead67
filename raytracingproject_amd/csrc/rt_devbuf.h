// rt_devbuf.h -- DevBuf, the one owner of a device allocation: every buffer of the context
// (rt_ctx.h), of the mesh builder's scratch (rt_lbvh.h) and every device temporary is one, and
// no other file of csrc/ allocates or frees device memory.
// Includes the HIP runtime API and nothing of the project's: tests/cpp/devbuf_driver.cpp
// compiles it with g++ against counting fakes of the three HIP calls below.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>

namespace rtx {

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;   // the bytes last asked for (an empty request still holds 16)

    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            (void)reset();
            p = o.p, cap = o.cap;
            o.p = nullptr, o.cap = 0;
        }
        return *this;
    }
    ~DevBuf() { (void)reset(); }

    hipError_t reset() {
        const hipError_t e = p ? hipFree(p) : hipSuccess;
        p = nullptr, cap = 0;
        return e;
    }
    // At least `bytes`: an allocation that holds them is kept (contents and address), else it
    // is replaced (contents lost).  After an error the buffer is empty.
    hipError_t reserve(size_t bytes) {
        if (p && cap >= bytes) return hipSuccess;
        hipError_t e = reset();
        if (e == hipSuccess) e = hipMalloc(&p, bytes ? bytes : 16);
        if (e != hipSuccess) {
            p = nullptr;
            return e;
        }
        cap = bytes;
        return hipSuccess;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
};

}  // namespace rtx
