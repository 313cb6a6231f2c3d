// Streams and events of a call: the fork / join of the two side streams and the clock behind asw_timing.
// Like asw_devmem.h it needs the declarations of the HIP runtime API only (tests/cpp/streams_scope.cpp).
#pragma once
#include <hip/hip_runtime_api.h>

#include "asw_devmem.h"

// What a context owns for the side work of a method: small launches that are independent of the method's main kernel (border tiles,
// a one-candidate tail, the normalisation plane of the permeability scans) overlap it instead of adding their latency to the frame.
struct SideSet {
    hipStream_t stream[2] = {nullptr, nullptr};  // hipStreamNonBlocking
    hipEvent_t fork = nullptr;                   // hipEventDisableTiming, like joined[]
    hipEvent_t joined[2] = {nullptr, nullptr};
};

// One fork / join of a runner.  A runner forks through the scope, never by hand:
//     SideStreams side(ctx->stream, ctx->side);
//     hipStream_t s0;
//     ASW_TRY(side.use(0, &s0));   // first use in the scope: the fork event on the main stream, once; then stream 0 waits on it
//     ... launches on s0, beside those on the main stream ...
//     ASW_TRY(side.join());        // every stream used, in index order: its event recorded on it, the main stream waits on it
// A scope that is left any other way -- an ASW_TRY return between the two -- joins in its destructor, so the main stream is
// ordered behind the side work whatever the runner returns, and the next call on the context cannot reuse scratch it still writes.
class SideStreams {
public:
    SideStreams(hipStream_t main, const SideSet& set) : main_(main), set_(set) {}
    SideStreams(const SideStreams&) = delete;
    SideStreams& operator=(const SideStreams&) = delete;
    ~SideStreams() { (void)join(); }
    // *s = side stream i, ordered behind everything the main stream held when the scope first used a side stream.  A stream whose
    // fork failed (ASW_ERR_HIP) counts as not used
    int use(int i, hipStream_t* s)
    {
        *s = nullptr;
        if (!used_[i]) {
            if (!forked_) ASW_HIP_TRY(hipEventRecord(set_.fork, main_));
            forked_ = true;
            ASW_HIP_TRY(hipStreamWaitEvent(set_.stream[i], set_.fork, 0));
            used_[i] = true;
        }
        *s = set_.stream[i];
        return ASW_OK;
    }
    // Idempotent; no HIP call when nothing was used.  A failure does not keep the other stream from being joined
    int join()
    {
        int rc = ASW_OK;
        for (int i = 0; i < 2; i++) {
            if (!used_[i]) continue;
            used_[i] = false;
            if (join_one(i) != ASW_OK) rc = ASW_ERR_HIP;
        }
        forked_ = false;
        return rc;
    }

private:
    int join_one(int i)
    {
        ASW_HIP_TRY(hipEventRecord(set_.joined[i], set_.stream[i]));
        ASW_HIP_TRY(hipStreamWaitEvent(main_, set_.joined[i], 0));
        return ASW_OK;
    }
    hipStream_t main_;
    const SideSet& set_;
    bool forked_ = false;
    bool used_[2] = {false, false};
};

// The four timing events of a call on the context's stream, and the asw_timing they produce (asw_get_timing returns `timing`):
// total_ms between begin_total and finish, aggregate_ms between begin_aggregate and end_aggregate, cost_ms = total - aggregate.
struct CallClock {
    hipStream_t stream = nullptr;  // the context's main stream (not owned)
    hipEvent_t total_start = nullptr, total_stop = nullptr, agg_start = nullptr, agg_stop = nullptr;  // timing enabled
    asw_timing timing = {0, 0, 0, 0};

    int begin_total()
    {
        ASW_HIP_TRY(hipEventRecord(total_start, stream));
        return ASW_OK;
    }
    int begin_aggregate()
    {
        ASW_HIP_TRY(hipEventRecord(agg_start, stream));
        return ASW_OK;
    }
    int end_aggregate(int launches)
    {
        ASW_HIP_TRY(hipEventRecord(agg_stop, stream));
        timing.aggregate_launches = launches;
        return ASW_OK;
    }
    // records the stop; sync: waits for the stream and fills the three times.  Without it the caller orders and waits on the stream
    // itself and `timing` keeps its times (the batch scheduler)
    int finish(bool sync)
    {
        ASW_HIP_TRY(hipEventRecord(total_stop, stream));
        if (!sync) return ASW_OK;
        ASW_HIP_TRY(hipStreamSynchronize(stream));
        float t = 0;
        ASW_HIP_TRY(hipEventElapsedTime(&t, total_start, total_stop));
        timing.total_ms = t;
        ASW_HIP_TRY(hipEventElapsedTime(&t, agg_start, agg_stop));
        timing.aggregate_ms = t;
        timing.cost_ms = timing.total_ms - timing.aggregate_ms;
        return ASW_OK;
    }
    // A further step on top of finished calls whose timing the caller accumulated in `sum`: step() (an asw_status) is bracketed by
    // the total pair and waited for on its stop event; `timing` = sum with the step's time added to total_ms and cost_ms recomputed.
    // On a failure `timing` stays what the last call left
    template <typename Step>
    int timed_step(asw_timing sum, Step&& step)
    {
        ASW_HIP_TRY(hipEventRecord(total_start, stream));
        ASW_TRY(step());
        ASW_HIP_TRY(hipEventRecord(total_stop, stream));
        ASW_HIP_TRY(hipEventSynchronize(total_stop));
        float t = 0;
        ASW_HIP_TRY(hipEventElapsedTime(&t, total_start, total_stop));
        sum.total_ms += t;
        sum.cost_ms = sum.total_ms - sum.aggregate_ms;
        timing = sum;
        return ASW_OK;
    }
};

// The clock's aggregate marks for a launcher that has work of its own on either side of them (launch_sgbm, launch_bm): begin() /
// end() around the aggregation kernels, back to back where there are none.  Without a clock both do nothing.
struct AggMarks {
    CallClock* clock = nullptr;
    int launches = 0;  // the aggregation launches between the marks (asw_timing::aggregate_launches)
    int begin() const { return clock ? clock->begin_aggregate() : ASW_OK; }
    int end() const { return clock ? clock->end_aggregate(launches) : ASW_OK; }
};
