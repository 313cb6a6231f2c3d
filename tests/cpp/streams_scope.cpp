// The side-stream scope and the call clock of csrc/asw_streams.h against the fake runtime of devmem_fake_hip.h
// (tests/test_streams_cpu.py builds this with -fsanitize=address,undefined).  Every case asserts and prints the event calls it
// logged, one line per case: "<call> <event> <stream>", comma separated; aborts on a miss.
#include <string>

#include "devmem_fake_hip.h"

#include "asw_streams.h"

static std::map<const void*, const char*> names;
static hipStream_t S_main;
static SideSet set;
static CallClock clk;

static void setup()
{
    names[nullptr] = "-";
    names[S_main = fake.new_stream()] = "main";
    names[set.stream[0] = fake.new_stream()] = "side0";
    names[set.stream[1] = fake.new_stream()] = "side1";
    names[set.fork = fake.new_event()] = "fork";
    names[set.joined[0] = fake.new_event()] = "j0";
    names[set.joined[1] = fake.new_event()] = "j1";
    clk.stream = S_main;
    names[clk.total_start = fake.new_event()] = "total0";
    names[clk.total_stop = fake.new_event()] = "total1";
    names[clk.agg_start = fake.new_event()] = "agg0";
    names[clk.agg_stop = fake.new_event()] = "agg1";
    fake.elapsed[{clk.total_start, clk.total_stop}] = 10.0f;
    fake.elapsed[{clk.agg_start, clk.agg_stop}] = 4.0f;
}

static void teardown()
{
    for (hipStream_t s : {S_main, set.stream[0], set.stream[1]}) CHECK(hipStreamDestroy(s) == hipSuccess);
    for (hipEvent_t e : {set.fork, set.joined[0], set.joined[1], clk.total_start, clk.total_stop, clk.agg_start, clk.agg_stop})
        CHECK(hipEventDestroy(e) == hipSuccess);
    CHECK(fake.streams.empty() && fake.events.empty());
}

using Log = std::vector<FakeHip::EventCall>;

// the log since the last case must be `want`; printed under the case's name
static void expect(const char* name, const Log& want)
{
    std::string line;
    for (auto& c : fake.log) {
        CHECK(names.count(c.event) && names.count(c.stream));
        line += std::string(line.empty() ? "" : ", ") + c.call + " " + names[c.event] + " " + names[c.stream];
    }
    printf("%s: %s\n", name, line.empty() ? "nothing" : line.c_str());
    fflush(stdout);
    CHECK(fake.log == want);
    fake.log.clear();
}

static void scope_cases()
{
    hipStream_t s = nullptr;
    const Log join0 = {{"record", set.stream[0], set.joined[0]}, {"wait", S_main, set.joined[0]}};
    const Log join1 = {{"record", set.stream[1], set.joined[1]}, {"wait", S_main, set.joined[1]}};
    {  // 1
        SideStreams side(S_main, set);
        CHECK(side.use(0, &s) == ASW_OK && s == set.stream[0]);
        CHECK(side.join() == ASW_OK);
    }
    expect("one side", {{"record", S_main, set.fork}, {"wait", set.stream[0], set.fork}, join0[0], join0[1]});
    {  // 2: one fork record, one wait per stream in order of first use, joins in index order, nothing for the repeated use
        SideStreams side(S_main, set);
        CHECK(side.use(0, &s) == ASW_OK && s == set.stream[0]);
        CHECK(side.use(1, &s) == ASW_OK && s == set.stream[1]);
        CHECK(side.use(0, &s) == ASW_OK && s == set.stream[0]);
        CHECK(side.join() == ASW_OK);
    }
    expect("both sides", {{"record", S_main, set.fork}, {"wait", set.stream[0], set.fork}, {"wait", set.stream[1], set.fork}, join0[0],
                          join0[1], join1[0], join1[1]});
    {  // the same with side 1 first: the waits follow the uses, the joins the indices
        SideStreams side(S_main, set);
        CHECK(side.use(1, &s) == ASW_OK && side.use(0, &s) == ASW_OK);
        CHECK(side.join() == ASW_OK);
    }
    expect("side 1 first", {{"record", S_main, set.fork}, {"wait", set.stream[1], set.fork}, {"wait", set.stream[0], set.fork}, join0[0],
                            join0[1], join1[0], join1[1]});
    {  // 3
        SideStreams side(S_main, set);
        CHECK(side.join() == ASW_OK);
    }
    expect("never used", {});
    {  // 4: an early return between fork and join
        SideStreams side(S_main, set);
        CHECK(side.use(1, &s) == ASW_OK && s == set.stream[1]);
        fake.log.clear();
    }
    expect("left open", join1);
    {  // 5
        SideStreams side(S_main, set);
        CHECK(side.use(0, &s) == ASW_OK);
        fake.log.clear();
        CHECK(side.join() == ASW_OK && side.join() == ASW_OK);
    }
    expect("joined twice, then left", join0);
    {  // 6: a stream whose fork failed counts as not used
        SideStreams side(S_main, set);
        fake.fail_event = 1;
        CHECK(side.use(0, &s) == ASW_ERR_HIP && s == nullptr);
        CHECK(side.join() == ASW_OK);
    }
    expect("fork record fails", {});
    {  // the fork recorded, the stream's wait refused: not used either
        SideStreams side(S_main, set);
        fake.fail_event = 2;
        CHECK(side.use(0, &s) == ASW_ERR_HIP && s == nullptr);
        CHECK(side.join() == ASW_OK);
    }
    expect("fork wait fails", {{"record", S_main, set.fork}});
    {  // 7: the status of a failed join; the other stream is joined all the same, and nothing is left for the destructor
        SideStreams side(S_main, set);
        CHECK(side.use(0, &s) == ASW_OK && side.use(1, &s) == ASW_OK);
        fake.log.clear();
        fake.fail_event = 1;
        CHECK(side.join() == ASW_ERR_HIP);
    }
    expect("join record fails", join1);
}

static bool is(const asw_timing& t, float total, float agg, float cost, int launches)
{
    return t.total_ms == total && t.aggregate_ms == agg && t.cost_ms == cost && t.aggregate_launches == launches;
}

static void clock_cases()
{
    // 8
    CHECK(clk.begin_total() == ASW_OK && clk.begin_aggregate() == ASW_OK && clk.end_aggregate(3) == ASW_OK);
    CHECK(clk.finish(true) == ASW_OK && is(clk.timing, 10.0f, 4.0f, 6.0f, 3));
    expect("clock", {{"record", S_main, clk.total_start}, {"record", S_main, clk.agg_start}, {"record", S_main, clk.agg_stop},
                     {"record", S_main, clk.total_stop}, {"stream-sync", S_main, nullptr}});
    // 9
    fake.elapsed[{clk.total_start, clk.total_stop}] = 99.0f;
    CHECK(clk.finish(false) == ASW_OK && is(clk.timing, 10.0f, 4.0f, 6.0f, 3));
    expect("clock, no wait", {{"record", S_main, clk.total_stop}});
    // the marks of a launcher: both recorded through the clock with the launch count, nothing without a clock
    AggMarks none, marks{&clk, 7};
    CHECK(none.begin() == ASW_OK && none.end() == ASW_OK && clk.timing.aggregate_launches == 3);
    CHECK(marks.begin() == ASW_OK && marks.end() == ASW_OK && clk.timing.aggregate_launches == 7);
    expect("marks", {{"record", S_main, clk.agg_start}, {"record", S_main, clk.agg_stop}});
    // 10: waits on the step's stop event, not on the stream
    fake.elapsed[{clk.total_start, clk.total_stop}] = 2.5f;
    const asw_timing sum = {7.0f, 3.0f, 0.0f, 5};
    int steps = 0;
    CHECK(clk.timed_step(sum, [&] { steps++; return (int)ASW_OK; }) == ASW_OK && steps == 1);
    CHECK(is(clk.timing, 9.5f, 3.0f, 6.5f, 5));
    expect("added step", {{"record", S_main, clk.total_start}, {"record", S_main, clk.total_stop}, {"sync", nullptr, clk.total_stop}});
    // a step that fails: its status, no stop, the timing as it was
    CHECK(clk.timed_step({1.0f, 1.0f, 0.0f, 1}, [&] { return (int)ASW_ERR_ALLOC; }) == ASW_ERR_ALLOC && is(clk.timing, 9.5f, 3.0f, 6.5f, 5));
    expect("added step fails", {{"record", S_main, clk.total_start}});
}

int main()
{
    setup();
    scope_cases();
    clock_cases();
    teardown();
    printf("ok\n");
    return 0;
}
