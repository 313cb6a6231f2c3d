"""Per-call times (HIP events of the library, asw_get_timing) of cross-scale cost aggregation (asw_disparity_cross_scale, DESIGN.md
section 4.18) at 1920x1080x3, numDisparity 128, DISPARITY_LEFT, for S = 2, 3 and 5 scales (lambda code 19) over selector entries 2
(window 15), 8 (window 15) and 12 (window 35), with and without the kept volume, next to the plain match of the same build in the
same run.  Resident pair, best of N by total time after one warm-up call.  aggregate_ms of a flagged call is the finest scale's
alone (the event pair stays on it), so `extra` = total - plain total is what the coarse scales, the pyramid and the combine pass
add together; the predictions it is held against: coarse scales about 1/8 + 1/64 + .. of the plain aggregate time, the combine pass
well under a millisecond.

    python tools/time_cross_scale.py [--reps N]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aswstereomatch_amd as asw  # noqa: E402
from aswstereomatch_amd.synth import make_pair  # noqa: E402

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
ctx = asw.Context(0)
H, W, D = 1080, 1920, 128
A = asw.StereoMatchingAlgorithms
METHODS = (("entry 2 (classic) win 15", int(A.ADAPTIVE_WEIGHT), 15), ("entry 8 (GuidedF_2) win 15", int(A.ADAPTIVE_WEIGHT_GUIDED_FILTER_2), 15),
           ("entry 12 (cross) win 35", int(A.ADAPTIVE_WEIGHT_CROSS), 35))


def best_of(call):
    ts = []
    for i in range(reps + 1):  # the first call warms up
        call()
        ts.append(ctx.timing())
    return min(ts[1:], key=lambda t: t["total_ms"])


def line(label, t, note=""):
    print("1920x1080x3 D=128  %-44s: total %8.3f ms  aggregate %8.3f ms  launches %d%s" % (
        label, t["total_ms"], t["aggregate_ms"], t["aggregate_launches"], note), flush=True)


print("tools/time_cross_scale.py --reps %d: best of %d calls by total_ms after one warm-up call" % (reps, reps), flush=True)
L, R, _ = make_pair(H, W, D, seed=1234, block=48)
ctx.upload_pair(0, L, R)
for label, alg, win in METHODS:
    for keep in (False, True):
        vol = " + volume" if keep else ""
        plain = best_of(lambda: ctx.match_resident(0, asw.DISPARITY_LEFT, alg, win, 0, D, keep_volume=keep))
        line("%s plain%s" % (label, vol), plain)
        d0 = ctx.download_disparity(0, (H, W))
        for S in (2, 3, 5):
            t = best_of(lambda: ctx.match_resident(0, asw.DISPARITY_LEFT, alg, win, 0, D, keep_volume=keep, cross_scale=asw.cross_scale(S, 19)))
            extra = t["total_ms"] - plain["total_ms"]
            predicted = plain["aggregate_ms"] * sum(8.0 ** -s for s in range(1, S))
            moved = float((ctx.download_disparity(0, (H, W)) != d0).mean())
            line("%s S=%d%s" % (label, S, vol), t, "  extra %7.3f ms = %.3f of plain total (coarse scales predicted %.3f ms)  map moved %.3f" % (
                extra, extra / plain["total_ms"], predicted, moved))
ctx.close()
