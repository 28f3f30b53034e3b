// Device buffer (grow-only): every device array the host side owns.
#pragma once
#include <algorithm>
#include <cstddef>
#include <hip/hip_runtime.h>

template <typename T>
struct DBuf {
    T* p = nullptr;
    size_t cap = 0;
    unsigned flags = 0;   // hipExtMallocWithFlags flags (0 = plain hipMalloc)
    DBuf() = default;
    DBuf(const DBuf&) = delete;
    DBuf& operator=(const DBuf&) = delete;
    ~DBuf() { reset(); }
    void reset() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }   // back to "never allocated": a null p is read as "no such table" (joints.hpp)
    hipError_t ensure(size_t n, bool keep = false, hipStream_t st = nullptr) {
        if (n <= cap) return hipSuccess;
        size_t ncap = std::max(n, cap + cap / 2);
        T* np = nullptr;
        hipError_t e = flags ? hipExtMallocWithFlags((void**)&np, ncap * sizeof(T), flags) : hipMalloc((void**)&np, ncap * sizeof(T));
        if (e != hipSuccess) return e;
        if (keep && p && cap) { e = hipMemcpyAsync(np, p, cap * sizeof(T), hipMemcpyDeviceToDevice, st); if (e != hipSuccess) return e; (void)hipStreamSynchronize(st); }
        if (p) (void)hipFree(p);
        p = np; cap = ncap;
        return hipSuccess;
    }
    void swap(DBuf& o) { std::swap(p, o.p); std::swap(cap, o.cap); std::swap(flags, o.flags); }
};
