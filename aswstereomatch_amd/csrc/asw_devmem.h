// Device memory of the host layer: the owning buffer and the cache entry of a parameter table.  Needs
// the declarations of the HIP runtime API only, so a host compiler builds it without a kernel in sight (tests/cpp/devmem_*.cpp).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>

#include "../../include/asw_mi355x.h"

#define ASW_HIP_TRY(expr)                                  \
    do {                                                   \
        hipError_t _e = (expr);                            \
        if (_e != hipSuccess) {                            \
            asw_note_hip_error(_e, #expr, __FILE__, __LINE__); \
            return ASW_ERR_HIP;                            \
        }                                                  \
    } while (0)

#define ASW_TRY(expr)                  \
    do {                               \
        int _rc = (expr);              \
        if (_rc != ASW_OK) return _rc; \
    } while (0)

void asw_note_hip_error(hipError_t e, const char* what, const char* file, int line);

// Grow-only device buffer that owns its allocation: freed when the buffer (or whatever holds it) goes away, moved but never copied.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) {
            release();
            p = o.p; cap = o.cap;
            o.p = nullptr; o.cap = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    int ensure(size_t bytes)
    {
        if (bytes <= cap && p) return ASW_OK;
        release();
        size_t want = bytes < 256 ? 256 : bytes;
        if (hipMalloc(&p, want) != hipSuccess) {
            p = nullptr;
            return ASW_ERR_ALLOC;
        }
        cap = want;
        return ASW_OK;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

// What the device tables next to it hold.  The one way to fill them:
//     if (cache.hit(key)) return ASW_OK;         // a miss marks the entry invalid before a byte is overwritten
//     ... build on the host ...
//     ASW_TRY(cache.upload(buf, data, bytes));   // once per table; any early return leaves the entry invalid
//     return cache.commit(key);                  // waits while the host data is still in scope, then stores the key
// so the key never describes a buffer that holds something else, and no host table dies before its copy has run.
template <typename Key>
struct TableCache {
    Key key{};
    bool valid = false;
    hipStream_t stream = nullptr;  // of the miss in progress
    bool hit(const Key& k, hipStream_t s)
    {
        if (valid && key == k) return true;
        valid = false;
        stream = s;
        return false;
    }
    int upload(DevBuf& dst, const void* src, size_t bytes)
    {
        ASW_TRY(dst.ensure(bytes));
        ASW_HIP_TRY(hipMemcpyAsync(dst.p, src, bytes, hipMemcpyHostToDevice, stream));
        return ASW_OK;
    }
    int commit(const Key& k)
    {
        ASW_HIP_TRY(hipStreamSynchronize(stream));
        key = k;
        valid = true;
        return ASW_OK;
    }
};
