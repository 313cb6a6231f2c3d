"""Per-call times (HIP events of the library, asw_get_timing) of AD-Census matching (asw_alg_adcensus) at
1920x1080x3, 128 candidates, for win 15 and 35, next to plain selector entry 12 (truncated AD under the same aggregation kernels) of
the same build in the same run.  Resident pair, best of N by total time; cost_ms holds the gray, census and cost kernels, so the
difference of the two cost_ms is the price of the census kernels.

    python tools/time_adcensus.py [--reps N]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import aswstereomatch_amd as asw  # noqa: E402
import cross_ref as cr  # noqa: E402

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
ctx = asw.Context(0)
H, W, D = 1080, 1920, 128
METHODS = (("cross (entry 12)", int(asw.StereoMatchingAlgorithms.ADAPTIVE_WEIGHT_CROSS)), ("adcensus", asw.adcensus_algorithm()))


def best_of(call):
    ts = []
    for i in range(reps + 1):  # the first call warms up
        call()
        ts.append(ctx.timing())
    return min(ts[1:], key=lambda t: t["total_ms"])


def line(label, t):
    print("1920x1080x3 D=128  %-36s: total %.3f ms  aggregate %.3f ms  cost %.3f ms  launches %d" % (
        label, t["total_ms"], t["aggregate_ms"], t["cost_ms"], t["aggregate_launches"]), flush=True)


L, R, _ = cr.region_pair(H, W, 64, 1, (25, 40), 0.12, block=48)
ctx.upload_pair(0, L, R)
for win in (15, 35):
    for dt, name in ((asw.DISPARITY_LEFT, "LEFT"), (asw.DISPARITY_RIGHT, "RIGHT")):
        cost = {}
        for label, alg in METHODS:
            t = best_of(lambda: ctx.match_resident(0, dt, alg, win, 0, D, keep_volume=False))
            line("%s win %d %s" % (label, win, name), t)
            cost[label] = t["cost_ms"]
            d0 = ctx.download_disparity(0, (H, W))
            t = best_of(lambda: ctx.match_resident(0, dt, alg, win, 0, D, keep_volume=True))
            line("%s win %d %s + volume" % (label, win, name), t)
            print("    map without the volume == map with it: %s" % np.array_equal(d0, ctx.download_disparity(0, (H, W))), flush=True)
        print("    cost_ms adcensus - cross: %.3f ms" % (cost["adcensus"] - cost["cross (entry 12)"]), flush=True)
ctx.close()
