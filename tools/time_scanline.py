"""Per-call times (HIP events of the library, asw_get_timing) of scanline optimisation (asw_disparity_scanline)
at 1920x1080x3, numDisparity 128, DISPARITY_LEFT, default penalties, over selector entries 2 (window 15), 8 (window 15) and 12
(window 35), with and without the kept volume, next to the plain match of the same build in the same run.  Resident pair, best of N
by total time after one warm-up call.  The step runs behind the aggregation events, so aggregate_ms of a flagged call is the
method's alone and `extra` = total - plain total is what the three scanline kernels add -- plus, without the kept volume, what the
method saves when it may skip writing its volume, which a flagged call never may.  The prediction it is held against: 9 volumes of
traffic (the horizontal pass reads V twice and writes the sum, the two vertical passes read V and the sum and write one of them) and a
dependent chain of about 3 W + 2 H steps per wavefront.

    python tools/time_scanline.py [--reps N]"""
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


def best_of(call):
    ts = []
    for i in range(reps + 1):  # the first call warms up
        call()
        ts.append(ctx.timing())
    return min(ts[1:], key=lambda t: t["total_ms"])


def line(label, t, note=""):
    print("1920x1080x3 D=128  %-44s: total %8.3f ms  aggregate %8.3f ms  launches %d%s" % (
        label, t["total_ms"], t["aggregate_ms"], t["aggregate_launches"], note), flush=True)


print("tools/time_scanline.py --reps %d: best of %d calls by total_ms after one warm-up call" % (reps, reps), flush=True)
L, R, _ = make_pair(H, W, D, seed=1234, block=48)
ctx.upload_pair(0, L, R)
for label, alg, win in METHODS:
    n = _lib.lib().asw_volume_planes(alg, D)
    gb = 9.0 * n * H * W * 4 / 1e9
    for keep in (False, True):
        vol = " + volume" if keep else ""
        plain = best_of(lambda: ctx.match_resident(0, asw.DISPARITY_LEFT, alg, win, 0, D, keep_volume=keep))
        line("%s plain%s" % (label, vol), plain)
        d0 = ctx.download_disparity(0, (H, W))
        t = best_of(lambda: ctx.match_resident(0, asw.DISPARITY_LEFT, alg, win, 0, D, keep_volume=keep, scanline=asw.scanline()))
        extra = t["total_ms"] - plain["total_ms"]
        moved = float((ctx.download_disparity(0, (H, W)) != d0).mean())
        line("%s scanline%s" % (label, vol), t, "  extra %8.3f ms = %.3f of plain total (%d planes, 9 volumes = %.2f GB: %.0f GB/s)  map moved %.3f" % (
            extra, extra / plain["total_ms"], n, gb, gb / max(extra, 1e-9) * 1e3, moved))
ctx.close()
