"""Per-call times (HIP events of the library, asw_get_timing) of the smoothed match (asw_match_smoothed_resident, T = 3, the wrappers'
default parameters; asw_mi355x.h "Smoothing") at 1920x1080x3, numDisparity 128, over selector entries 2 (window
15), 8 (window 15) and 12 (window 35), against the plain resident match that keeps its volume and against the left-right refinement
(asw_match_refined_resident, refine_win 15) where that is served (entry 8 has no DISPARITY_RIGHT branch).  The three calls alternate
in one run of one build; best of N each by total time after one warm-up round.  The smoothed call computes and writes the method's
volume like the plain one, then runs the confidence kernel and the smoothing's 2 T + 2 kernels: `extra` = the difference of the two
totals is what the confidence and the smoothing add to one match.  The per-kernel times (prep, row pass, column pass, final) come from
a run of their own, `rocprofv3 --kernel-trace --stats -- python tools/time_smooth.py --reps 1`.

    python tools/time_smooth.py [--reps N]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aswstereomatch_amd as asw  # noqa: E402
from aswstereomatch_amd.synth import make_pair  # noqa: E402

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
ctx = asw.Context(0)
H, W, D, T = 1080, 1920, 128, 3
A = asw.StereoMatchingAlgorithms
METHODS = (("entry 2 (classic) win 15", int(A.ADAPTIVE_WEIGHT), 15, True), ("entry 8 (GuidedF_2) win 15", int(A.ADAPTIVE_WEIGHT_GUIDED_FILTER_2), 15, False),
           ("entry 12 (cross) win 35", int(A.ADAPTIVE_WEIGHT_CROSS), 35, True))


def line(label, t, note=""):
    print("1920x1080x3 D=128  %-44s: total %8.3f ms  aggregate %8.3f ms  launches %d%s" % (
        label, t["total_ms"], t["aggregate_ms"], t["aggregate_launches"], note), flush=True)


print("tools/time_smooth.py --reps %d: best of %d calls by total_ms after one warm-up round, the calls alternating" % (reps, reps), flush=True)
L, R, _ = make_pair(H, W, D, seed=1234, block=48)
ctx.upload_pair(0, L, R)
for label, alg, win, refined in METHODS:
    plain, smooth, refine = [], [], []
    for i in range(reps + 1):  # the first round warms up
        ctx.match_resident(0, asw.DISPARITY_LEFT, alg, win, 0, D, keep_volume=True)
        plain.append(ctx.timing())
        ctx.match_smoothed_resident(0, alg, win, 0, D, iterations=T)
        smooth.append(ctx.timing())
        if refined:
            ctx.match_refined_resident(0, alg, win, 0, D, refineWin=15)
            refine.append(ctx.timing())
    t1 = min(plain[1:], key=lambda t: t["total_ms"])
    t2 = min(smooth[1:], key=lambda t: t["total_ms"])
    extra = t2["total_ms"] - t1["total_ms"]
    line("%s plain + volume" % label, t1)
    line("%s smoothed T=%d" % (label, T), t2, "  extra %8.3f ms = %.4f of the plain total" % (extra, extra / t1["total_ms"]))
    if refined:
        t3 = min(refine[1:], key=lambda t: t["total_ms"])
        line("%s refined win 15" % label, t3, "  extra %8.3f ms = %.4f of the plain total; smoothed / refined = %.3f" % (
            t3["total_ms"] - t1["total_ms"], (t3["total_ms"] - t1["total_ms"]) / t1["total_ms"], t2["total_ms"] / t3["total_ms"]))
    else:
        print("1920x1080x3 D=128  %-44s: not served (no DISPARITY_RIGHT branch)" % ("%s refined win 15" % label), flush=True)
ctx.close()
