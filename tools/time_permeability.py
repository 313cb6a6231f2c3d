"""Per-call times (HIP events of the library, asw_get_timing) of the recursive (permeability) aggregation (asw_alg_permeability,
DESIGN.md section 4.17) at 1920x1080x3, numDisparity 128, both directions, with and without the kept volume, next to the two-pass ASW
at win 15 and 35 and selector entry 12 (cross-based regions) at win 35 of the same build in the same run.  Resident pair, best of N
by aggregate time after one warm-up call.  The gate: the permeability aggregate_ms is below the two-pass win-35 one for the same
direction and volume choice; the ratio to the two-pass win-15 time is printed, not required.

    python tools/time_permeability.py [--reps N]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aswstereomatch_amd as asw  # noqa: E402
from aswstereomatch_amd.synth import make_pair  # noqa: E402

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
ctx = asw.Context(0)
H, W, D = 1080, 1920, 128
PERM = asw.permeability_algorithm()
METHODS = (("twopass win 15", asw.twopass_algorithm(), 15), ("twopass win 35", asw.twopass_algorithm(), 35),
           ("entry 12 (cross) win 35", int(asw.StereoMatchingAlgorithms.ADAPTIVE_WEIGHT_CROSS), 35), ("permeability", PERM, 0))


def best_of(call):
    ts = []
    for i in range(reps + 1):  # the first call warms up
        call()
        ts.append(ctx.timing())
    return min(ts[1:], key=lambda t: t["aggregate_ms"])


def line(label, t, note=""):
    print("1920x1080x3 D=128  %-36s: total %.3f ms  aggregate %.3f ms  cost %.3f ms  launches %d%s" % (
        label, t["total_ms"], t["aggregate_ms"], t["cost_ms"], t["aggregate_launches"], note), flush=True)


print("tools/time_permeability.py --reps %d: best of %d calls by aggregate_ms after one warm-up call" % (reps, reps), flush=True)
L, R, _ = make_pair(H, W, D, seed=1234, block=48)
ctx.upload_pair(0, L, R)
worst = None
for dt, name in ((asw.DISPARITY_LEFT, "LEFT"), (asw.DISPARITY_RIGHT, "RIGHT")):
    for keep in (False, True):
        agg = {}
        for label, alg, win in METHODS:
            t = best_of(lambda: ctx.match_resident(0, dt, alg, win, 0, D, keep_volume=keep))
            agg[label] = t["aggregate_ms"]
            note = ""
            if label == "permeability":
                r35, r15 = agg["twopass win 35"] / t["aggregate_ms"], agg["twopass win 15"] / t["aggregate_ms"]
                note = "  twopass 35 / permeability = %.2f  twopass 15 / permeability = %.2f" % (r35, r15)
                worst = r35 if worst is None else min(worst, r35)
            line("%s %s%s" % (label, name, " + volume" if keep else ""), t, note)
        if keep:
            d1 = ctx.download_disparity(0, (H, W))
            ctx.match_resident(0, dt, PERM, 0, 0, D, keep_volume=False)
            print("    permeability map without the volume == map with it: %s" % np.array_equal(d1, ctx.download_disparity(0, (H, W))),
                  flush=True)
print("smallest twopass win 35 / permeability aggregate ratio: %.2f (the gate: above 1 everywhere)" % worst, flush=True)
ctx.close()
sys.exit(0 if worst > 1.0 else 1)
