// The few HIP runtime calls csrc/asw_devmem.h and asw_ctx's destructor make, defined here so that a host program runs them without
// libamdhip64 and without a GPU (tests/test_devmem_cpu.py).  "Device" memory is host memory, which puts it under the sanitizers:
//   - allocations, streams and events are counted, and freeing / destroying / copying into one that was never handed out aborts;
//   - the n-th hipMalloc, hipMemcpyAsync or hipStreamSynchronize from now can be told to fail;
//   - hipMemcpyAsync only records the copy: it is carried out at the next hipStreamSynchronize of its stream, so host data that
//     died in between is read after its lifetime -- which AddressSanitizer reports.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <set>
#include <vector>

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            abort();                                                         \
        }                                                                    \
    } while (0)

struct FakeHip {
    std::map<char*, size_t> live;  // allocation -> bytes
    std::set<void*> streams, events;
    long mallocs = 0, frees = 0, copies = 0, copied_bytes = 0, syncs = 0, set_device = 0;
    int fail_malloc = 0, fail_copy = 0, fail_sync = 0;  // n > 0: the n-th call from now fails, once
    struct Copy { void* dst; const void* src; size_t bytes; hipStream_t stream; };
    std::vector<Copy> pending;
    bool due(int& n) { return n > 0 && --n == 0; }
    hipStream_t new_stream() { void* s = malloc(1); streams.insert(s); return (hipStream_t)s; }
    hipEvent_t new_event() { void* e = malloc(1); events.insert(e); return (hipEvent_t)e; }
    bool inside_live(const void* p, size_t bytes) const
    {
        for (auto& kv : live)
            if ((const char*)p >= kv.first && (const char*)p + bytes <= kv.first + kv.second) return true;
        return false;
    }
};
static FakeHip fake;

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes)
{
    if (fake.due(fake.fail_malloc)) return hipErrorOutOfMemory;
    char* m = (char*)malloc(bytes);
    fake.live[m] = bytes;
    fake.mallocs++;
    *p = m;
    return hipSuccess;
}
hipError_t hipFree(void* p)
{
    CHECK(fake.live.count((char*)p) == 1);  // handed out, and not freed yet
    fake.live.erase((char*)p);
    fake.frees++;
    free(p);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t stream)
{
    CHECK(kind == hipMemcpyHostToDevice && fake.inside_live(dst, bytes));
    if (fake.due(fake.fail_copy)) return hipErrorUnknown;
    fake.pending.push_back({dst, src, bytes, stream});
    fake.copies++;
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t stream)
{
    CHECK(fake.streams.count(stream) == 1);
    fake.syncs++;
    std::vector<FakeHip::Copy> rest;
    for (auto& c : fake.pending) {
        if (c.stream != stream) { rest.push_back(c); continue; }
        CHECK(fake.inside_live(c.dst, c.bytes));
        memcpy(c.dst, c.src, c.bytes);  // the host side is read only now
        fake.copied_bytes += (long)c.bytes;
    }
    fake.pending.swap(rest);
    if (fake.due(fake.fail_sync)) return hipErrorUnknown;
    return hipSuccess;
}
hipError_t hipSetDevice(int)
{
    fake.set_device++;
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s)
{
    CHECK(fake.streams.erase(s) == 1);
    free(s);
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e)
{
    CHECK(fake.events.erase(e) == 1);
    free(e);
    return hipSuccess;
}
}

void asw_note_hip_error(hipError_t, const char*, const char*, int) {}
