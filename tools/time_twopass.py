"""Per-call times (HIP events of the library, asw_get_timing) of the two-pass (separable) ASW (asw_alg_twopass, DESIGN.md section
4.16) at 1920x1080x3, numDisparity 128 (129 candidates), for win 15 and 35, both directions, with and without the kept volume, next
to plain selector entry 2 (the exact method it approximates) of the same build in the same run.  Resident pair, best of N by
aggregate time.  The last column is entry 2's aggregate_ms over the two-pass one for the same window, direction and volume choice.

    python tools/time_twopass.py [--reps N]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aswstereomatch_amd as asw  # noqa: E402
from aswstereomatch_amd.synth import make_pair  # noqa: E402

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
ctx = asw.Context(0)
H, W, D = 1080, 1920, 128
METHODS = (("entry 2 (exact)", int(asw.StereoMatchingAlgorithms.ADAPTIVE_WEIGHT)), ("twopass", asw.twopass_algorithm()))


def best_of(call):
    ts = []
    for i in range(reps + 1):  # the first call warms up
        call()
        ts.append(ctx.timing())
    return min(ts[1:], key=lambda t: t["aggregate_ms"])


def line(label, t, ratio=None):
    print("1920x1080x3 D=128  %-36s: total %.3f ms  aggregate %.3f ms  cost %.3f ms  launches %d%s" % (
        label, t["total_ms"], t["aggregate_ms"], t["cost_ms"], t["aggregate_launches"],
        "" if ratio is None else "  entry 2 / twopass = %.2f" % ratio), flush=True)


print("tools/time_twopass.py --reps %d: best of %d calls by aggregate_ms after one warm-up call" % (reps, reps), flush=True)
L, R, _ = make_pair(H, W, D, seed=1234, block=48)
ctx.upload_pair(0, L, R)
worst = None
for win in (15, 35):
    for dt, name in ((asw.DISPARITY_LEFT, "LEFT"), (asw.DISPARITY_RIGHT, "RIGHT")):
        for keep in (False, True):
            agg = {}
            for label, alg in METHODS:
                t = best_of(lambda: ctx.match_resident(0, dt, alg, win, 0, D, keep_volume=keep))
                agg[label] = t["aggregate_ms"]
                ratio = agg["entry 2 (exact)"] / t["aggregate_ms"] if label == "twopass" else None
                line("%s win %d %s%s" % (label, win, name, " + volume" if keep else ""), t, ratio)
                if ratio is not None:
                    worst = ratio if worst is None else min(worst, ratio)
            if keep:
                d1 = ctx.download_disparity(0, (H, W))
                ctx.match_resident(0, dt, asw.twopass_algorithm(), win, 0, D, keep_volume=False)
                print("    twopass map without the volume == map with it: %s" % np.array_equal(d1, ctx.download_disparity(0, (H, W))),
                      flush=True)
print("smallest entry 2 / twopass aggregate ratio: %.2f (the gate: above 1 everywhere)" % worst, flush=True)
ctx.close()
sys.exit(0 if worst > 1.0 else 1)
