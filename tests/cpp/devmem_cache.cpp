// DevBuf's contract and the TableCache protocol of csrc/asw_devmem.h against the fake runtime of devmem_fake_hip.h
// (tests/test_devmem_cpu.py builds this with -fsanitize=address,undefined).  Prints one line per check group; aborts on a miss.
#include <tuple>
#include <type_traits>
#include <utility>

#include "devmem_fake_hip.h"

#include "asw_devmem.h"

static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_assignable<DevBuf>::value, "DevBuf is never copied");
static_assert(std::is_nothrow_move_constructible<DevBuf>::value && std::is_nothrow_move_assignable<DevBuf>::value,
              "DevBuf moves without throwing: std::vector<Frame> relocates by move");

static void ensure_contract()
{
    {
        DevBuf b;
        CHECK(b.ensure(1) == ASW_OK && b.p && b.cap == 256 && fake.mallocs == 1);  // the 256-byte minimum
        void* p = b.p;
        CHECK(b.ensure(256) == ASW_OK && b.p == p && fake.mallocs == 1);  // bytes <= cap: nothing new
        CHECK(b.ensure(0) == ASW_OK && b.p == p && fake.mallocs == 1);
        CHECK(b.ensure(257) == ASW_OK && b.cap == 257 && fake.mallocs == 2 && fake.frees == 1);  // grows, the old block freed
        CHECK(b.ensure(100) == ASW_OK && b.cap == 257 && fake.mallocs == 2);                     // and never shrinks
        fake.fail_malloc = 1;
        CHECK(b.ensure(1000) == ASW_ERR_ALLOC && b.p == nullptr && b.cap == 0);  // a failed allocation leaves an empty buffer
        CHECK(fake.live.empty() && fake.frees == 2);                            // and no leak
        CHECK(b.ensure(1000) == ASW_OK && b.cap == 1000);                       // which can be filled again
        b.release();
        CHECK(b.p == nullptr && b.cap == 0 && fake.live.empty());
        b.release();  // twice is once
        DevBuf c;
        CHECK(c.ensure(300) == ASW_OK && b.ensure(400) == ASW_OK);
        void* q = b.p;
        c = std::move(b);  // onto a non-empty buffer: its block is freed, the source is left empty
        CHECK(c.p == q && c.cap == 400 && b.p == nullptr && b.cap == 0 && fake.live.size() == 1);
        DevBuf d(std::move(c));
        CHECK(d.p == q && c.p == nullptr && fake.live.size() == 1);
    }
    CHECK(fake.live.empty() && fake.mallocs == fake.frees);  // the destructor frees
    printf("ensure contract ok: %ld allocations, %ld frees\n", fake.mallocs, fake.frees);
}

// a table site as the library writes them: the host data lives in this function, the cache synchronises before it returns
static int builds = 0;
static int ensure_table(TableCache<std::tuple<int, double>>& cache, DevBuf& buf, hipStream_t s, int n, double scale)
{
    const auto key = std::make_tuple(n, scale);
    if (cache.hit(key, s)) return ASW_OK;
    builds++;
    std::vector<double> tab(n);
    for (int i = 0; i < n; i++) tab[i] = scale * i;
    ASW_TRY(cache.upload(buf, tab.data(), tab.size() * sizeof(double)));
    return cache.commit(key);
}

static bool holds(const DevBuf& buf, int n, double scale)
{
    for (int i = 0; i < n; i++)
        if (buf.as<double>()[i] != scale * i) return false;
    return true;
}

static void cache_protocol()
{
    hipStream_t s = fake.new_stream();
    {
        TableCache<std::tuple<int, double>> cache;
        DevBuf buf;
        const long c0 = fake.copies, y0 = fake.syncs;
        CHECK(ensure_table(cache, buf, s, 100, 0.5) == ASW_OK && builds == 1 && cache.valid);  // miss: built once
        CHECK(fake.copies == c0 + 1 && fake.syncs == y0 + 1 && fake.pending.empty());         // one copy, one wait, inside
        CHECK(holds(buf, 100, 0.5));                                                           // the device bytes are the builder's
        CHECK(ensure_table(cache, buf, s, 100, 0.5) == ASW_OK && builds == 1);                 // hit: no builder
        CHECK(fake.copies == c0 + 1 && fake.syncs == y0 + 1);                                  // no copy, no wait
        CHECK(ensure_table(cache, buf, s, 100, 0.25) == ASW_OK && builds == 2 && holds(buf, 100, 0.25));  // key change: rebuilt
        CHECK(ensure_table(cache, buf, s, 50, 0.25) == ASW_OK && builds == 3 && holds(buf, 50, 0.25));
        // the stale-key case: a failed upload of another key, then the previous key again
        fake.fail_copy = 1;
        CHECK(ensure_table(cache, buf, s, 60, 2.0) == ASW_ERR_HIP && builds == 4 && !cache.valid);
        CHECK(ensure_table(cache, buf, s, 50, 0.25) == ASW_OK && builds == 5 && holds(buf, 50, 0.25));
        // the same for a failed wait (the copy may have landed: the buffer holds the new table under no key)
        fake.fail_sync = 1;
        CHECK(ensure_table(cache, buf, s, 60, 2.0) == ASW_ERR_HIP && builds == 6 && !cache.valid);
        CHECK(ensure_table(cache, buf, s, 50, 0.25) == ASW_OK && builds == 7 && holds(buf, 50, 0.25));
        // and for a failed allocation
        fake.fail_malloc = 1;
        CHECK(ensure_table(cache, buf, s, 4000, 1.0) == ASW_ERR_ALLOC && builds == 8 && !cache.valid && buf.p == nullptr);
        CHECK(ensure_table(cache, buf, s, 50, 0.25) == ASW_OK && builds == 9 && holds(buf, 50, 0.25));
    }
    CHECK(hipStreamDestroy(s) == hipSuccess);
    CHECK(fake.live.empty() && fake.mallocs == fake.frees && fake.pending.empty());
    printf("cache protocol ok: %d builds\n", builds);
}

// what the protocol rules out: the host table dies before the wait.  The fake reads it at the wait, so AddressSanitizer ends the
// program here -- the proof that the checks above would notice a cache that waited too late
static void dead_host_table()
{
    hipStream_t s = fake.new_stream();
    TableCache<int> cache;
    DevBuf buf;
    cache.hit(1, s);
    {
        std::vector<double> tab(100, 1.0);
        CHECK(cache.upload(buf, tab.data(), tab.size() * sizeof(double)) == ASW_OK);
    }
    (void)cache.commit(1);
    printf("dead host table went unnoticed\n");
}

int main(int argc, char** argv)
{
    if (argc > 1 && !strcmp(argv[1], "dead-host-table")) {
        dead_host_table();
        return 0;
    }
    ensure_contract();
    cache_protocol();
    return 0;
}
