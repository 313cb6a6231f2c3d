"""Per-call times (HIP events of the library, asw_get_timing) of the cross-based support-region method (selector entry 12, DESIGN.md
section 4.12) at 1920x1080x3, 128 candidates, for win 15 and 35, without and with the kept f32 volume, next to GuidedF_2 at win 15 on
the same frame.  Resident pair, best of N by total time; the map without the volume is compared with the map with it.

    python tools/time_cross.py [--reps N]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import aswstereomatch_amd as asw  # noqa: E402
import cross_ref as cr  # noqa: E402

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
ctx = asw.Context(0)
A = asw.StereoMatchingAlgorithms
H, W, D = 1080, 1920, 128


def best_of(call):
    ts = []
    for i in range(reps + 1):  # the first call warms up
        call()
        ts.append(ctx.timing())
    return min(ts[1:], key=lambda t: t["total_ms"])


def line(label, t):
    print("1920x1080x3 D=128  %-34s: total %.3f ms  aggregate %.3f ms  cost %.3f ms  launches %d" % (
        label, t["total_ms"], t["aggregate_ms"], t["cost_ms"], t["aggregate_launches"]), flush=True)


L, R, _ = cr.region_pair(H, W, 64, 1, (25, 40), 0.12, block=48)
ctx.upload_pair(0, L, R)
a = cr.arms(L, 20, 17)
print("arms of the frame at tau 20, win 35: 0 / between / 17 = %.3f %.3f %.3f" % cr.arm_shares(a, 17), flush=True)
for win in (15, 35):
    for dt, name in ((asw.DISPARITY_LEFT, "LEFT"), (asw.DISPARITY_RIGHT, "RIGHT")):
        t = best_of(lambda: ctx.match_resident(0, dt, A.ADAPTIVE_WEIGHT_CROSS, win, 0, D, keep_volume=False))
        line("cross win %d %s" % (win, name), t)
        d0 = ctx.download_disparity(0, (H, W))
        t = best_of(lambda: ctx.match_resident(0, dt, A.ADAPTIVE_WEIGHT_CROSS, win, 0, D, keep_volume=True))
        line("cross win %d %s + volume" % (win, name), t)
        print("    map without the volume == map with it: %s" % np.array_equal(d0, ctx.download_disparity(0, (H, W))), flush=True)
t = best_of(lambda: ctx.match_resident(0, asw.DISPARITY_LEFT, A.ADAPTIVE_WEIGHT_GUIDED_FILTER_2, 15, 0, D, keep_volume=False))
line("GuidedF_2 win 15 LEFT", t)
ctx.close()
