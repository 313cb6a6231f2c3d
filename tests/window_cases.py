"""Every float ASW method at the top of its window range: the table of served windows, the windows on both sides of every switch
between kernel forms, and the cases that run them (tests/test_window_cases_cpu.py on the oracle alone, tests/test_gpu_large_windows.py
on the GPU).  Plain numpy: nothing here needs a GPU.  TEST INFRASTRUCTURE ONLY.

tests/asw_cases.py ends at window 35 and the fixed parity tests use 5 to 15; the largest LDS layouts the library launches (classic at
160160 of 163840 bytes, the run-time-layout bilateral form above its 64 KB opt-in, BLO1's chunk-width-1 instance) lie above that.
An error in an offset, a halo width or a reflection at these sizes shows on no smaller window.

Parts:

  `LIMITS`: per method (largest served window, first refused window, the status there, the source expression the numbers follow
  from).  The host entries refuse with the launcher's own limit before they build a table, a buffer or a launch
  (bilateral_max_window, ncc_max_window, walk_max_kernel, blo1_max_window in csrc/asw_internal.h);

  `FORM_WINDOWS`: the windows each method runs, on both sides of every switch;

  `FRAMES` and `cases(method, win, frame)`: cases built by asw_cases.build_case, so a printed tag rebuilds the case.  Not the full
  product: every window runs on (6, 90), the two extreme windows of a method run on the other two frames, and the pairs of a frame
  are fixed per direction (`PAIRS`), so that consecutive windows of a method see the same pair;

  `sad_d_views(case, k)`: the bordered view getCostSAD_d takes for plane k of a SAD-cost case.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import asw_cases as ac  # noqa: E402

LEFT, RIGHT = ac.LEFT, ac.RIGHT
ERR_EVEN_WINDOW, ERR_BAD_ARGUMENT = 2, 7      # include/asw_mi355x.h

# method -> (largest served window, first refused window, status at the first refused window, where the numbers come from).
# "sad" is the SAD cost (getCostSAD and getCostSAD_d), "geodist" is getGeodesicDist; the others are the names of asw_cases.METHODS.
LIMITS = {
    # k_bilateral.hip: Layout(win / 2, GT).total <= 160 * 1024; 160160 bytes at 63, 166912 at 65
    "classic": (63, 65, ERR_BAD_ARGUMENT, "bilateral_max_window()"),
    "direct8": (63, 65, ERR_BAD_ARGUMENT, "bilateral_max_window()"),
    # k_ncc.hip: (4 + 2h) * ((64 + 2h) + (64 + 2h + 15)) * 4 <= 64 * 1024; 64232 bytes at 59, 67328 at 61
    "ncc": (59, 61, ERR_BAD_ARGUMENT, "min(ncc_max_window(), walk_max_kernel())"),
    # k_guided.hip: k <= 64 * CPL / 2 with CPL = 2 columns per lane; GuidedF and the SAD cost take odd windows only
    "guided": (63, 65, ERR_BAD_ARGUMENT, "walk_max_kernel(), odd"),
    "guided2": (64, 65, ERR_BAD_ARGUMENT, "walk_max_kernel()"),     # the window is the box side as it stands, even ones too
    "guided3": (59, 61, ERR_BAD_ARGUMENT, "min(walk_max_kernel(), ncc_max_window())"),
    "sad": (63, 65, ERR_BAD_ARGUMENT, "walk_max_kernel(), odd"),
    # k_blo1.hip: (3 + win) * (63 + win) * 6 + 16 <= 160 * 1024 holds to 133; the SAD cost under it comes from the walk
    "blo1": (63, 65, ERR_BAD_ARGUMENT, "min(blo1_max_window(), walk_max_kernel()), odd"),
    "wmedian": (45, 47, ERR_BAD_ARGUMENT, "run_wmedian: 2048 slots of the per-pixel sort"),
    "geodesic": (35, 37, ERR_BAD_ARGUMENT, "run_geodesic: win <= 35"),
    "geodist": (35, 37, ERR_BAD_ARGUMENT, "asw_geodesic_dist: win_size <= 35"),
}


# ---------------------------------------------------------------- the launchers' expressions, restated
def _up(v, a):
    return (v + a - 1) // a * a


def bilateral_lds(win, G=4):
    """Layout::total of k_bilateral.hip: the cost tile (16 bytes per cell), the staged weights of G taps, both gray tiles"""
    h, TW, TH, DC = win // 2, 64, 4, 16
    cost = _up((TH + 2 * h) * (TW + 2 * h) * DC, 16)
    weights = _up(G * TH * (TW + DC - 1) * 4, 16) + G * TH * TW * 4
    return cost + weights + _up((TH + 2 * h) * _up(TW + 2 * h, 4), 16) + _up((TH + 2 * h) * _up(TW + 2 * h + DC - 1, 4), 16)


def ncc_lds(win):
    """launch_ncc: the reference tile and one chunk's tile of the other image, f32"""
    h = win // 2
    return (4 + 2 * h) * ((64 + 2 * h) + (64 + 2 * h + 15)) * 4


def blo1_lds(win, dc):
    """launch_blo1 at chunk width dc: dc costs (f32) and dc shifted samples per cell, one reference sample"""
    return (4 + win - 1) * (64 + win - 1) * (dc * 5 + 1) + 16


def blo1_chunk(win):
    """the chunk width launch_blo1 picks"""
    return 4 if blo1_lds(win, 4) <= 48 * 1024 else 2 if blo1_lds(win, 2) <= 64 * 1024 else 1


WALK_MAX_KERNEL = 64      # launch_walk_t: k - 1 halo columns must leave outputs in a strip of 64 * 2 columns
LDS_PER_WORKGROUP = 160 * 1024


def _last_odd(fits):
    win = 1
    while fits(win + 2):
        win += 2
    return win


def derived_limits():
    """method -> largest served window, from the expressions above alone"""
    bil = _last_odd(lambda w: bilateral_lds(w) <= LDS_PER_WORKGROUP)
    ncc = min(_last_odd(lambda w: ncc_lds(w) <= 64 * 1024), WALK_MAX_KERNEL)
    odd_walk = WALK_MAX_KERNEL - 1 + WALK_MAX_KERNEL % 2
    blo = min(_last_odd(lambda w: blo1_lds(w, 1) <= LDS_PER_WORKGROUP), odd_walk)
    return {"classic": bil, "direct8": bil, "ncc": ncc, "guided": odd_walk, "guided2": WALK_MAX_KERNEL, "guided3": min(ncc, odd_walk),
            "sad": odd_walk, "blo1": blo}


# the windows run per method: both sides of every switch between kernel forms, and the last served window
FORM_WINDOWS = {
    "classic": (29, 31, 37, 61, 63),     # 29 | 31: the dynamic-LDS opt-in above 64 KB (62656 / 67360 bytes); 37: past the <17> instance
    "direct8": (29, 31, 37, 61, 63),
    "ncc": (37, 57, 59),
    "guided": (37, 63),
    "guided2": (36, 37, 63, 64),         # even windows: GuidedF_2 alone
    "guided3": (37, 59),
    "sad": (37, 63),
    "blo1": (23, 25, 49, 51, 63),        # chunk width 4 | 2 at 23 | 25, 2 | 1 at 49 | 51
}
RUN_METHODS = tuple(FORM_WINDOWS)

# (H, W, row padding): two tile columns with the second partial and H no multiple of the tile height; a frame smaller than the
# window in both directions (borders reflect more than once); a third tile column, rows with padding
FRAMES = ((6, 90, 0), (3, 20, 0), (9, 130, 5))
# per frame and direction, the (kind, seed, numD, minD) of its two pairs: numD 18 crosses the 16-wide candidate chunk.  The periodic
# seeds give (period, shift) = (16, 3), (8, 2), (5, 5) (matcher_cases.make_input)
PAIRS = {
    (6, 90, 0): {LEFT: (("textured", 71, 18, 0), ("periodic", 23, 5, 3)), RIGHT: (("textured", 71, 5, 3), ("periodic", 23, 18, 0))},
    (3, 20, 0): {LEFT: (("textured", 72, 5, 3), ("periodic", 16, 18, 0)), RIGHT: (("textured", 72, 18, 0), ("periodic", 16, 5, 3))},
    (9, 130, 5): {LEFT: (("textured", 73, 18, 3), ("periodic", 33, 5, 0)), RIGHT: (("periodic", 33, 18, 3), ("textured", 73, 5, 0))},
}
SERVES_RIGHT = dict(ac.SERVES_RIGHT, sad=True)
TABLE_PARAMS = dict(ac.TABLE_PARAMS, sad=())


def directions(method):
    return (LEFT, RIGHT) if SERVES_RIGHT[method] else (LEFT,)


def frames(method, win):
    """the frames `win` runs on: all three for the method's two extreme windows, (6, 90) for the others"""
    w = FORM_WINDOWS[method]
    return FRAMES if win in (w[0], w[-1]) else FRAMES[:1]


def cases(method, win, frame):
    """the cases of (method, window, frame): both pairs of the frame in every direction the method serves"""
    H, W, pad = frame
    out = []
    for dt in directions(method):
        for kind, seed, numD, minD in PAIRS[frame][dt]:
            if method == "blo1":
                minD = 0          # the reference's absolute-offset indexing: only minDisparity == 0 is defined
            out.append(ac.build_case(method, (kind, H, W, win, minD, numD, dt, TABLE_PARAMS[method], pad, seed)))
    return out


def run_ids():
    """(method, window, frame) of every parametrised run"""
    return [(m, w, f) for m in RUN_METHODS for w in FORM_WINDOWS[m] for f in frames(m, w)]


def periodic_parameters(seed):
    """(period, shift) of the "periodic" pair of `seed`, as matcher_cases.make_input derives them"""
    return ac.mc._PERIODS[seed % len(ac.mc._PERIODS)], (seed // len(ac.mc._PERIODS)) % 8


def small_case(method, win=15):
    """a window-15 case of `method` that any context must still serve after a refusal"""
    minD = 0 if method == "blo1" else 2
    return ac.build_case(method, ("textured", 6, 40, win, minD, 5, LEFT, TABLE_PARAMS[method], 0, 74))


def reference(oracle, case):
    """asw_cases.reference; for the SAD cost {"vol": oracle.cost_sad}"""
    if case["method"] != "sad":
        return ac.reference(oracle, case)
    rc, vol = oracle.cost_sad(case["L"], case["R"], case["dt"], case["win"], case["minD"], case["numD"])
    assert rc == 0, case["tag"]
    return {"vol": vol}


def _reflect(p, n):
    """BORDER_REFLECT (fedcba|abcdefgh|hgfedcb), as often as it takes"""
    while p < 0 or p >= n:
        p = -p - 1 if p < 0 else 2 * n - 1 - p
    return p


def sad_d_views(case, k):
    """(left, right, disparity) for getCostSAD_d that give plane k of the case's getCostSAD: the view that is not the reference one
    bordered by max_offset REFLECT columns, on its left (LEFT) or on its right (RIGHT), as M.cpp:2877-2878 does it"""
    L, R, dt, minD, numD = (case[n] for n in ("L", "R", "dt", "minD", "numD"))
    W, max_off = L.shape[1], minD + numD - 1
    if dt == LEFT:
        cols = [_reflect(x - max_off, W) for x in range(W + max_off)]
        return L, np.ascontiguousarray(R[:, cols]), minD + k
    cols = [_reflect(x, W) for x in range(W + max_off)]
    return np.ascontiguousarray(L[:, cols]), R, minD + k
