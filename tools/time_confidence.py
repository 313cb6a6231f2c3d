"""Per-call times (HIP events of the library, asw_get_timing) of the confidence channel (a 2-channel disparity image; asw_mi355x.h
"Confidence") at 1920x1080x3, numDisparity 128, DISPARITY_LEFT, over selector entries 2 (window 15), 8 (window
15) and 12 (window 35).  Both calls of a pair compute and write the method's volume and neither downloads it: the 1-channel one is a
resident match that keeps its volume, the 2-channel one a host-image call without cost_volume_out; the two alternate in one run of one
build, best of N each by total time after one warm-up call, so `extra` = the difference of the totals is what k_confidence adds.  It
reads the n planes once and writes 8 bytes per pixel.  The yardstick is k_wta on the same volume (entry 8 launches it on its own
volume: `rocprofv3 --kernel-trace --stats -- python tools/time_confidence.py` lists both kernels), which moves the same bytes.

    python tools/time_confidence.py [--reps N]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aswstereomatch_amd as asw  # noqa: E402
from aswstereomatch_amd import _lib  # noqa: E402
from aswstereomatch_amd.synth import make_pair  # noqa: E402

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
ctx = asw.Context(0)
H, W, D = 1080, 1920, 128
A = asw.StereoMatchingAlgorithms
METHODS = (("entry 2 (classic) win 15", int(A.ADAPTIVE_WEIGHT), 15), ("entry 8 (GuidedF_2) win 15", int(A.ADAPTIVE_WEIGHT_GUIDED_FILTER_2), 15),
           ("entry 12 (cross) win 35", int(A.ADAPTIVE_WEIGHT_CROSS), 35))


def line(label, t, note=""):
    print("1920x1080x3 D=128  %-44s: total %8.3f ms  aggregate %8.3f ms  launches %d%s" % (
        label, t["total_ms"], t["aggregate_ms"], t["aggregate_launches"], note), flush=True)


print("tools/time_confidence.py --reps %d: best of %d calls by total_ms after one warm-up call, the two calls alternating" % (reps, reps),
      flush=True)
L, R, _ = make_pair(H, W, D, seed=1234, block=48)
ctx.upload_pair(0, L, R)
for label, alg, win in METHODS:
    n = _lib.lib().asw_volume_planes(alg, D)
    gb = (n * 4 + 4 + 8) * H * W / 1e9  # n planes and the map read, 8 bytes per pixel written
    one, two = [], []
    for i in range(reps + 1):  # the first pair of calls warms up
        ctx.match_resident(0, asw.DISPARITY_LEFT, alg, win, 0, D, keep_volume=True)
        one.append(ctx.timing())
        d2, c2 = ctx.stereoMatching(L, R, asw.DISPARITY_LEFT, alg, win, 0, D, return_confidence=True)
        two.append(ctx.timing())
    t1 = min(one[1:], key=lambda t: t["total_ms"])
    t2 = min(two[1:], key=lambda t: t["total_ms"])
    d1, c1 = ctx.download_disparity(0, (H, W), confidence=True)  # the slot's kept volume gives the same pair
    assert (d1 == d2).all() and (c1.view("u4") == c2.view("u4")).all()
    extra = t2["total_ms"] - t1["total_ms"]
    line("%s 1 channel + volume" % label, t1)
    line("%s 2 channels" % label, t2, "  extra %8.3f ms = %.4f of the 1-channel total (%d planes, %.3f GB per frame: %.0f GB/s)  confidence mean %.3f, zero share %.3f" % (
        extra, extra / t1["total_ms"], n, gb, gb / max(extra, 1e-9) * 1e3, float(c2.mean()), float((c2 == 0).mean())))
ctx.close()
