// The few HIP runtime calls csrc/asw_devmem.h, csrc/asw_streams.h and asw_ctx's destructor make, defined here so that a host program
// runs them without libamdhip64 and without a GPU (tests/test_devmem_cpu.py, tests/test_streams_cpu.py).  "Device" memory is host
// memory, which puts it under the sanitizers:
//   - allocations, streams and events are counted, and freeing / destroying / copying into one that was never handed out aborts;
//   - the n-th hipMalloc, hipMemcpyAsync, hipStreamSynchronize or event call from now can be told to fail;
//   - event records, waits and synchronisations are logged in order with their stream and event, which must be the fake's own;
//     hipEventElapsedTime gives what the program set for the pair;
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
    // the event calls of csrc/asw_streams.h ("record", "wait", "sync") and every hipStreamSynchronize ("stream-sync"), in the order
    // they were made; a failed event call is not logged
    struct EventCall {
        const char* call; hipStream_t stream; hipEvent_t event;
        bool operator==(const EventCall& o) const { return !strcmp(call, o.call) && stream == o.stream && event == o.event; }
    };
    std::vector<EventCall> log;
    int fail_event = 0;  // counts hipEventRecord, hipStreamWaitEvent and hipEventSynchronize together
    std::map<std::pair<hipEvent_t, hipEvent_t>, float> elapsed;  // what hipEventElapsedTime gives for (start, stop): set by the program
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
    fake.log.push_back({"stream-sync", stream, nullptr});
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
hipError_t hipEventRecord(hipEvent_t e, hipStream_t stream)
{
    CHECK(fake.events.count(e) == 1 && fake.streams.count(stream) == 1);
    if (fake.due(fake.fail_event)) return hipErrorUnknown;
    fake.log.push_back({"record", stream, e});
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t stream, hipEvent_t e, unsigned flags)
{
    CHECK(fake.events.count(e) == 1 && fake.streams.count(stream) == 1 && flags == 0);
    if (fake.due(fake.fail_event)) return hipErrorUnknown;
    fake.log.push_back({"wait", stream, e});
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e)
{
    CHECK(fake.events.count(e) == 1);
    if (fake.due(fake.fail_event)) return hipErrorUnknown;
    fake.log.push_back({"sync", nullptr, e});
    return hipSuccess;
}
hipError_t hipEventElapsedTime(float* ms, hipEvent_t start, hipEvent_t stop)
{
    CHECK(fake.events.count(start) == 1 && fake.events.count(stop) == 1 && fake.elapsed.count({start, stop}) == 1);
    *ms = fake.elapsed[{start, stop}];
    return hipSuccess;
}
}

void asw_note_hip_error(hipError_t, const char*, const char*, int) {}
