// Who frees what an asw_ctx holds (csrc/asw_internal.h), against the fake runtime of devmem_fake_hip.h: a context on the stack gets an
// allocation in every member that can hold one, is put through the moves the library makes, and must leave nothing behind when it
// goes out of scope.  Prints "live <allocations> mallocs <n> frees <n> streams <n> events <n>"; tests/test_devmem_cpu.py reads it.
#include <utility>

#include "devmem_fake_hip.h"

#include "asw_internal.h"

static void fill(Frame& f, size_t bytes)
{
    for (DevBuf* b : {&f.L, &f.R, &f.disp, &f.vol}) CHECK(b->ensure(bytes) == ASW_OK);
}

static void exercise()
{
    asw_ctx ctx;
    ctx.stream = fake.new_stream();
    ctx.clock.stream = ctx.stream;
    for (auto& s : ctx.side.stream) s = fake.new_stream();
    for (hipEvent_t* e : {&ctx.clock.total_start, &ctx.clock.total_stop, &ctx.clock.agg_start, &ctx.clock.agg_stop, &ctx.side.fork,
                          &ctx.side.joined[0], &ctx.side.joined[1]})
        *e = fake.new_event();
    // every member that bears a buffer
    fill(ctx.host_frame, 1000);
    for (Frame& f : ctx.coarse) fill(f, 500);
    for (DevBuf* b : {&ctx.bil.taps, &ctx.bil.lut, &ctx.bil.cells, &ctx.bil.lut_xq, &ctx.refine.tc, &ctx.refine.ts, &ctx.twopass.t,
                      &ctx.perm.t, &ctx.census.t, &ctx.wm.lut2, &ctx.wm.wd, &ctx.prep.t})
        CHECK(b->ensure(300) == ASW_OK);
    // frame slots as frame_slot() grows them: 3, then 70 -- the vector reallocates and the frames move
    ctx.frames.resize(3);
    for (Frame& f : ctx.frames) fill(f, 2000);
    const void* disp1 = ctx.frames[1].disp.p;
    ctx.frames.resize(70);
    CHECK(ctx.frames[1].disp.p == disp1 && ctx.frames[1].disp.cap == 2000);
    fill(ctx.frames[69], 100);
    // named scratch
    for (const char* name : {"grayL", "grayR", "refine_mask"}) CHECK(ctx.buf(name).ensure(4000) == ASW_OK);
    // match_refined swaps a frame's map with a scratch buffer
    DevBuf& side = ctx.buf("refine_dl");
    CHECK(side.ensure(8000) == ASW_OK);
    const void* a = side.p;
    std::swap(ctx.frames[1].disp, side);
    CHECK(ctx.frames[1].disp.p == a && ctx.frames[1].disp.cap == 8000 && side.p == disp1 && side.cap == 2000);
    // a move-assignment onto a buffer that holds something
    const long frees = fake.frees;
    ctx.frames[0].vol = std::move(ctx.frames[2].vol);
    CHECK(fake.frees == frees + 1 && ctx.frames[2].vol.p == nullptr && ctx.frames[0].vol.p);
    const long live = (long)fake.live.size();
    CHECK(live == fake.mallocs - fake.frees && live > 40);
}

int main()
{
    exercise();
    printf("live %ld mallocs %ld frees %ld streams %ld events %ld\n", (long)fake.live.size(), fake.mallocs, fake.frees,
           (long)fake.streams.size(), (long)fake.events.size());
    fflush(stdout);  // LeakSanitizer ends a leaking program without flushing
    return 0;
}
