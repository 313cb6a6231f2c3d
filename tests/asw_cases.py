"""Tie-dense pairs, a fixed tie table and a seeded case generator for the float ASW matchers (classic, direct8, geodesic, weighted
median, BLO1, NCC disparity, bilateral grid, the guided-filter family), in the manner of tests/matcher_cases.py, whose pair
generators and `tie_share` are reused.  Plain numpy: nothing here needs a GPU.  TEST INFRASTRUCTURE ONLY.

Every one of these methods resolves its winner by "strict `<` while d ascends", over many reduction stages (candidate chunks,
grid.z slices, wavefronts of an xq workgroup, tail slices, merge kernels).  A stage that keeps the later of two equal costs changes
the map only where two candidates have bit-identical costs, and textured pairs have none: `periodic` pairs have them at 0.65-0.95 of
the pixels (the table below; tests/test_asw_cases_cpu.py measures it on the oracle alone).

Parts:

  `periodic_same`: `periodic` with a shift of 0, an identical pair with period p (candidates 0, p, 2p, ... tie);

  the tie table `ONE_KERNEL_ROWS`, `XQ_ROWS`, `WMEDIAN_TILE_ROWS`, `ROW_CONSTANT_ROW` and `tie_cases(method)`;

  `random_case(rng, method, index)` / `build_case(method, tag)`: a case is rebuilt from its tag alone, so the tag an assertion prints
  is enough to run that case again;

  `reference(oracle, case)` and `gpu_result(ctx, case)`: {"disp", "vol"} of the oracle (oracle/asw_oracle.py) and of the library
  (`ctx` is an aswstereomatch_amd.Context), and `check(case, got, want)`, the comparison rules:

    bit-exact group: the volume and the map are equal bit for bit (NaN equal to NaN; BLO1 in its finite / NaN mask form);

    tolerance group (the guided-filter family, whose sliding sums differ from the oracle's direct sums): the volume within the
    method's bound (abs 1e-4 for guided and guided2, rtol 1e-4 for guided3), non-finite entries in the same places.  On `textured`
    and `flat_rects` pairs the maps are equal where all costs are finite.  On the tie-dense kinds the oracle itself has bit-equal
    minima that a different summation order may break legitimately, so there the GPU's winner d must be one of the oracle's
    minimisers within the bound: want_vol[d] <= want_vol.min(0) + tol(d) + tol(arg-min).  The two terms follow from the volume
    bound: the GPU's cost at its winner is within tol of the oracle's there, and so is its cost at the oracle's winner.  d must
    also lie in [minD, minD + planes).  On every kind the library's map must be the first strict minimum of the library's own
    returned volume, bit for bit: that holds k_wta to the tie rule where the oracle's volume cannot.

The bilateral grid stays out of the tie table: its grid coordinates depend on x, and blocky periodic pairs gave an oracle tie share
of at most 0.002.  The sweep covers it.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import matcher_cases as mc  # noqa: E402
from matcher_cases import constant, flat_rects, periodic, quantised, row_constant, textured, tie_share  # noqa: E402,F401

LEFT, RIGHT = 0, 1
BIT_EXACT = ("classic", "direct8", "geodesic", "wmedian", "blo1", "ncc", "bilgrid")
TOLERANCE = ("guided", "guided2", "guided3")
METHODS = BIT_EXACT + TOLERANCE
# DISPARITY_RIGHT served (matcher_cases.SUBPIXEL_METHODS and the ERR_UNSUPPORTED_LAYOUT tests of tests/test_gpu_parity.py); NCC
# disparity accepts RIGHT and writes nothing (the reference compares `cost > DBL_MAX`)
SERVES_RIGHT = {"classic": True, "direct8": False, "geodesic": True, "wmedian": False, "blo1": True, "ncc": True, "bilgrid": False,
                "guided": True, "guided2": False, "guided3": True}
# the method's own parameters in a tie-table case: the defaults of the parity tests
TABLE_PARAMS = {"classic": (30.0, 20.0), "direct8": (), "geodesic": (), "wmedian": (10.0, 10.0), "blo1": (0.015,), "ncc": (),
                "bilgrid": (10.0, 10.0), "guided": (1e-6,), "guided2": (1e-6,), "guided3": (1e-6,)}
KINDS = ("constant", "periodic", "periodic_same", "row_constant", "quantised", "flat_rects", "textured")
EXACT_MAP_KINDS = ("textured", "flat_rects")      # tolerance group: equal maps are claimed on these kinds only
WINDOWS = (1, 3, 5, 7, 9, 11, 15, 17, 21, 35)
SWEEP_SEEDS = (20265, 20266)
SWEEP_COUNT = 60          # cases per method and seed in tests/test_gpu_asw_sweep.py
FRESH_EVERY = 8           # the sweep creates a fresh context every so many cases


def directions(method):
    return (LEFT, RIGHT) if SERVES_RIGHT[method] else (LEFT,)


def planes(method, numD):
    """planes of the method's volume: the inclusive range numD + 1 for the bilateral family"""
    return numD + 1 if method in ("classic", "direct8", "geodesic", "bilgrid") else numD


def wta_planes(method, numD):
    """candidates the winner is taken over: NCC disparity never tests the last offset (M.cpp:864, `nwta` in k_ncc.hip)"""
    return numD - 1 if method == "ncc" else planes(method, numD)


# ---------------------------------------------------------------- pairs
def periodic_same(H, W, cn, p):
    """an identical pair of period p along x: candidates 0, p, 2p, ... match equally"""
    return periodic(H, W, cn, p, 0)


_SAME_PERIODS = (2, 3, 5, 8, 16, 64)


def make_input(kind, H, W, seed, D=16):
    """the 3-channel pair of `kind`: a name of KINDS, whose free parameters follow from `seed` as in matcher_cases.make_input, or
    ("periodic", p, shift) spelled out (the tie table)"""
    if isinstance(kind, tuple):
        return periodic(H, W, 3, kind[1], kind[2])
    if kind == "periodic_same":
        return periodic_same(H, W, 3, _SAME_PERIODS[seed % len(_SAME_PERIODS)])
    return mc.make_input(kind, H, W, 3, seed, D)


# ---------------------------------------------------------------- the tie table: (H, W, period, shift, win, minD, numD)
# A row's comment: what it ties across, then the oracle's tie share of the aggregated volume (`tie_share` over the candidates the
# winner is taken from), the range over the methods and directions that run the row.  tests/test_asw_cases_cpu.py measures the
# shares again and holds every (method, row, direction) to TIE_FLOOR and, where shift > 0, to MOVED_FLOOR: the share of the pixels
# whose winner is not minD (0.96-1.00 on every row here).  A row that misses a floor is replaced, never dropped.
TIE_FLOOR, MOVED_FLOOR = 0.3, 0.9
# classic, direct8 (LEFT), geodesic, BLO1 (the minD 0 rows), NCC disparity, weighted median
ONE_KERNEL_ROWS = [
    (9, 70, 16, 3, 7, 0, 40),      # chunks 16+16+8+1 and the grid.z slices (chunks16 = 3): 0.65-0.73
    (9, 70, 5, 2, 7, 0, 22),       # sub-chunks 16 / 4 / 2 / 1: 0.81-0.89
    (7, 90, 16, 3, 5, 2, 45),      # minD > 0: 0.72-0.80
    (1, 64, 4, 1, 3, 0, 9),        # one row: 0.87-0.96
]
# NCC keeps the SMALLEST correlation, so the pair's shift does not name its winner: on (9, 70, 5, 2, 7, 0, 22) the winner is minD at
# 0.23 of the pixels (moved share 0.77 < MOVED_FLOOR).  NCC runs this row in its place: tie share 0.87, moved share 1.00
NCC_REPLACED = {(9, 70, 5, 2, 7, 0, 22): (9, 70, 7, 1, 7, 0, 22)}
# the guided-filter family (launch_wta): periodic(8, 3), on which all three methods tie in both directions; the rows above gave
# guided2 and guided3 shares down to 0.00.  guided / guided2 / guided3, LEFT (RIGHT):
GUIDED_ROWS = [
    (9, 70, 8, 3, 7, 0, 40),       # 0.77 (0.78) / 0.62 / 0.44 (0.74)
    (7, 90, 8, 3, 5, 2, 45),       # minD > 0: 0.85 (0.83) / 0.70 / 0.76 (0.87)
    (12, 100, 8, 3, 9, 0, 40),     # 0.82 (0.78) / 0.68 / 0.76 (0.78)
]
# the xq forms of classic and geodesic (win 15), both directions; the two methods' shares agree to 0.002
XQ_ROWS = [
    (3, 257, 64, 0, 15, 0, 64),    # candidate 0 and the inclusive last candidate 64; 4-wave form, finished in the workgroup: 0.72
    (5, 400, 128, 0, 15, 0, 128),  # the same at 8 waves: candidates 0 and 128: 0.66 (0.33 at W = 200)
    (5, 200, 16, 3, 15, 0, 128),   # all eight wavefronts, interior and border columns: 0.87
    (5, 333, 64, 5, 15, 0, 130),   # candidates 5 and 69, tail of 3, full merge: 0.77
    (4, 400, 128, 7, 15, 0, 160),  # candidate 7 in the xq block and 135 in the tail slice: 0.64
    (9, 200, 8, 3, 15, 2, 70),     # 4-wave pass plus tail, minD > 0: 0.91
    (6, 300, 64, 5, 15, 0, 192),   # geodesic passes of 128 + 64 + `few`: 0.75
]
# the weighted median's tile forms (k_wmedian_tile.hip at 15 x 15, k_wmedian_tile_gen.hip at 17 x 17) against the per-pixel sort
WMEDIAN_TILE_ROWS = [
    (9, 70, 5, 2, 15, 0, 22),      # 0.89
    (9, 70, 16, 3, 17, 0, 20),     # 0.70
]
ROW_CONSTANT_ROW = (9, 200, 15, 0, 128)   # H, W, win, minD, numD: every candidate away from the borders ties (classic, geodesic): 1.00


def table_case(method, row, dt):
    H, W, p, shift, win, minD, numD = row
    return build_case(method, (("periodic", p, shift), H, W, win, minD, numD, dt, TABLE_PARAMS[method], 0, 0))


def tie_rows(method):
    """the rows of the tie table that `method` runs"""
    if method == "bilgrid":
        return []
    if method in TOLERANCE:
        return list(GUIDED_ROWS)
    rows = [r for r in ONE_KERNEL_ROWS if method != "blo1" or r[5] == 0]
    if method == "ncc":
        rows = [NCC_REPLACED.get(r, r) for r in rows]
    if method in ("classic", "geodesic"):
        rows += XQ_ROWS
    if method == "wmedian":
        rows += WMEDIAN_TILE_ROWS
    return rows


def tie_cases(method):
    return [table_case(method, row, dt) for row in tie_rows(method) for dt in directions(method)]


def row_constant_case(method, dt):
    H, W, win, minD, numD = ROW_CONSTANT_ROW
    return build_case(method, ("row_constant", H, W, win, minD, numD, dt, TABLE_PARAMS[method], 0, 5))


# ---------------------------------------------------------------- seeded cases
def _pick(rng, values):
    return values[int(rng.integers(0, len(values)))]


def random_case(rng, method, index=None):
    """One case of `method`, drawn from `rng`: only what the method serves.  With an `index` the input kind cycles over KINDS, the
    direction alternates from one round of kinds to the next, every eighth case of classic and geodesic is forced into the domain
    of the xq kernels and every twelfth case has a long candidate range; without one, all of these are drawn.

    tag = (kind, H, W, win, minD, numD, direction, the method's own parameters, row padding, seed)"""
    if index is None:
        index = int(rng.integers(0, 1 << 20))
    kind = KINDS[index % len(KINDS)]
    dt = index // len(KINDS) % 2 if SERVES_RIGHT[method] else LEFT
    H, W = int(rng.integers(1, 41)), int(rng.integers(1, 161))
    if rng.random() < 0.08:
        H = 1
    if rng.random() < 0.08:
        W = int(rng.integers(1, 5))
    win = _pick(rng, WINDOWS)
    minD = _pick(rng, (0, 0, 0, 1, 3, 17))
    numD = int(rng.integers(1, 48))
    long_range, xq = index % 12 == 5, index % 8 == 7 and method in ("classic", "geodesic")
    big = int(rng.integers(48, 151))
    if long_range:    # long candidate ranges cross the 16-wide chunk and z-split boundaries
        numD, H, W = big, min(H, 24), min(W, 96)
    xq_draws = (int(rng.integers(1, 10)), int(rng.integers(64, 301)), int(rng.integers(63, 201)),
                _pick(rng, (0, 0, 1, 5, 48, 49, 70) if method == "classic" else (0, 0, 2, 33, 130)))
    if xq:            # win 15, from 63 candidates up, widths with partial and border tiles
        H, W, numD, minD = xq_draws
        win = 15
    if method == "guided2" and rng.random() < 0.25:
        win += 1      # GuidedF_2 takes the window as the box radius argument and accepts even ones
    # keep the oracle's side in the millisecond range
    if win > 21:
        W, numD = min(W, 120), min(numD, 12)
    if method == "geodesic" and win > 15:     # (win + 2)^2 relaxations per pixel and pass
        H, W, numD = min(H, 20), min(W, 64), min(numD, 8)
    if method == "wmedian":                   # a multimap per pixel and candidate
        numD = min(numD, 20)
        if win > 11:
            H, W, numD = min(H, 24), min(W, 64), min(numD, 10)
    if method == "bilgrid":
        numD = min(numD, 12)
    if method == "blo1":
        minD = 0      # the reference's absolute-offset indexing: only minDisparity == 0 is defined
    params = draw_params(rng, method)
    pad = int(rng.integers(1, 9)) if rng.random() < 0.15 else 0     # rows with padding: the C-ABI reads them through asw_image.step
    seed = int(rng.integers(0, 1 << 30))
    return build_case(method, (kind, H, W, win, minD, numD, dt, params, pad, seed))


def draw_params(rng, method):
    """the method's own parameters: gamma_c and gamma_g, the sample rates, eps"""
    if method == "classic":
        return (_pick(rng, (30.0, 5.0, 0.5, 100.0)), _pick(rng, (20.0, 2.0, 7.5, 60.0)))
    if method == "wmedian":
        return _pick(rng, ((10.0, 10.0), (5.0, 20.0), (3.0, 3.0), (25.0, 2.5)))
    if method == "blo1":
        return (_pick(rng, (0.015, 0.05, 0.004, 0.2)),)
    if method == "bilgrid":
        return (_pick(rng, (2.5, 4.0, 6.0, 7.5, 10.0, 16.0)), _pick(rng, (3.0, 5.0, 10.0, 33.3, 40.0, 64.0, 128.0, 300.0)))
    if method in ("guided", "guided2"):
        return (_pick(rng, (1e-6, 1e-8, 1e-3)),)
    return (1e-6,) if method == "guided3" else ()


def cases(method, seed, count=SWEEP_COUNT):
    """the `count` cases of (method, seed)"""
    rng = np.random.default_rng([seed, METHODS.index(method)])
    return [random_case(rng, method, i) for i in range(count)]


def build_case(method, tag):
    """the case of `tag`: dict(method, tag, the pair and every parameter)"""
    kind, H, W, win, minD, numD, dt, params, pad, seed = tag
    L, R = make_input(kind, H, W, seed, numD)
    return {"method": method, "tag": tuple(tag), "kind": kind, "L": mc.padded_view(L, pad, 0), "R": mc.padded_view(R, pad, 255),
            "win": win, "minD": minD, "numD": numD, "dt": dt, "params": tuple(params)}


# ---------------------------------------------------------------- both sides of a case, in one layout
def reference(oracle, case):
    """the oracle's {"disp", "vol"}; NCC: the disparity overload's map and the un-normalised planes of the volume overload"""
    m, L, R, dt, win, minD, numD, p = (case[k] for k in ("method", "L", "R", "dt", "win", "minD", "numD", "params"))
    if m == "ncc":
        rc, disp = oracle.ncc_disparity(L, R, dt, win, minD, numD)
        rc2, vol = oracle.cost_ncc(L, R, dt, win, minD, numD, raw=True)
        assert rc == 0 and rc2 == 0, case["tag"]
        return {"disp": disp, "vol": vol}
    if m == "classic":
        rc, disp, vol = oracle.asw_classic(L, R, p[0], p[1], dt, win, minD, numD, want_vol=True)
    elif m == "direct8":
        rc, disp, vol = oracle.asw_direct8(L, R, dt, win, minD, numD, want_vol=True)
    elif m == "geodesic":
        rc, disp, vol = oracle.asw_geodesic(L, R, dt, win, minD, numD, want_vol=True)
    elif m == "wmedian":
        rc, disp, vol = oracle.asw_wmedian(L, R, dt, win, p[0], p[1], minD, numD, want_vol=True)
    elif m == "blo1":
        rc, disp, vol = oracle.asw_blo1(L, R, dt, p[0], win, minD, numD, want_vol=True)
    elif m == "bilgrid":
        rc, disp, vol = oracle.asw_bilgrid(L, R, dt, p[0], p[1], minD, numD, want_vol=True)
    elif m == "guided":
        rc, disp, vol = oracle.asw_guided(L, R, dt, p[0], win, minD, numD, want_vol=True)
    elif m == "guided2":
        rc, disp, vol = oracle.asw_guided2(L, R, dt, p[0], win, minD, numD, want_vol=True)
    elif m == "guided3":
        rc, disp, vol = oracle.asw_guided3(L, R, dt, p[0], win, minD, numD, want_vol=True)
    else:
        raise ValueError(m)
    assert rc == 0, case["tag"]
    return {"disp": disp, "vol": vol}


def gpu_result(ctx, case):
    """the library's {"disp", "vol"} through the method's own entry point with return_cost_volume=True"""
    m, L, R, dt, win, minD, numD, p = (case[k] for k in ("method", "L", "R", "dt", "win", "minD", "numD", "params"))
    if m == "ncc":
        return {"disp": ctx.computeNCC(L, R, dt, win, minD, numD),
                "vol": np.stack(ctx.computeNCC_costs(L, R, dt, win, minD, numD, normalized=False))}
    if m == "classic":
        disp, vol = ctx.computeAdaptiveWeight(L, R, p[0], p[1], dt, win, minD, numD, return_cost_volume=True)
    elif m == "direct8":
        disp, vol = ctx.computeAdaptiveWeight_direct8(L, R, dt, win, minD, numD, return_cost_volume=True)
    elif m == "geodesic":
        disp, vol = ctx.computeAdaptiveWeight_geodesic(L, R, dt, win, minD, numD, return_cost_volume=True)
    elif m == "wmedian":
        disp, vol = ctx.computeAdaptiveWeight_WeightedMedian(L, R, dt, win, p[0], p[1], minD, numD, return_cost_volume=True)
    elif m == "blo1":
        disp, vol = ctx.computeAdaptiveWeight_BLO1(L, R, dt, p[0], win, minD, numD, return_cost_volume=True)
    elif m == "bilgrid":
        disp, vol = ctx.computeAdaptiveWeight_bilateralGrid(L, R, dt, p[0], p[1], minD, numD, return_cost_volume=True)
    elif m == "guided":
        disp, vol = ctx.computeAdaptiveWeight_GuidedF(L, R, dt, p[0], win, minD, numD, return_cost_volume=True)
    elif m == "guided2":
        disp, vol = ctx.computeAdaptiveWeight_GuidedF_2(L, R, dt, p[0], win, minD, numD, return_cost_volume=True)
    elif m == "guided3":
        disp, vol = ctx.computeAdaptiveWeight_GuidedF_3(L, R, dt, p[0], win, minD, numD, return_cost_volume=True)
    else:
        raise ValueError(m)
    return {"disp": disp, "vol": vol}


def first_strict_minimum(vol, minD):
    """the winner rule on a volume [d][y][x]: the first strict minimum in ascending d, NaN never selected, 0 where nothing is
    selected (a cost must be below DBL_MAX: +inf never is)"""
    v = np.where(np.isnan(vol) | (vol == np.inf), np.inf, vol.astype(np.float64))
    sel = (v < np.inf).any(axis=0)
    return np.where(sel, minD + v.argmin(axis=0), 0).astype(np.float32)


def tolerance(method, want_vol):
    """the volume bound of a tolerance-group method, per entry"""
    if method == "guided3":
        return 1e-4 * np.abs(want_vol.astype(np.float64)) + 1e-30
    return np.full(want_vol.shape, 1e-4)


def check(case, got, want):
    """the comparison rules of this file's header; raises AssertionError naming the rebuild call"""
    m, kind, minD = case["method"], case["kind"], case["minD"]
    where = "asw_cases.build_case(%r, %r)" % (m, case["tag"])
    gv, wv, gd, wd = got["vol"], want["vol"], got["disp"], want["disp"]
    assert gv.shape == wv.shape and gd.shape == wd.shape, "shapes differ: " + where
    if m == "blo1":
        fin = np.isfinite(wv)
        assert np.array_equal(fin, np.isfinite(gv)) and np.array_equal(np.isnan(wv), np.isnan(gv)), "finite / NaN masks differ: " + where
        assert np.array_equal(gv[fin], wv[fin]), "vol differs: " + where
        assert np.array_equal(gd, wd), "disp differs: " + where
        return
    if m in BIT_EXACT:
        assert np.array_equal(gv, wv, equal_nan=True), "vol differs: " + where
        assert np.array_equal(gd, wd), "disp differs: " + where
        return
    fin = np.isfinite(wv)
    assert np.array_equal(fin, np.isfinite(gv)) and np.array_equal(gv[~fin], wv[~fin], equal_nan=True), "non-finite entries differ: " + where
    tol = tolerance(m, wv)
    err = np.abs(gv.astype(np.float64) - wv.astype(np.float64))
    if m == "guided3":
        assert (err[fin] <= tol[fin]).all(), "vol beyond rtol 1e-4: " + where
    else:
        assert (err[fin] < tol[fin]).all(), "vol beyond abs 1e-4 (max %g): %s" % (err[fin].max(), where)
    pix = fin.all(axis=0)
    # whatever the sums' order did to a tie, the library's map is the winner rule on the library's own volume, bit for bit
    assert np.array_equal(gd[pix], first_strict_minimum(gv, minD)[pix]), "disp is not the first strict minimum of the returned vol: " + where
    if kind in EXACT_MAP_KINDS:
        assert np.array_equal(gd[pix], wd[pix]), "disp differs: " + where
        return
    n = wv.shape[0]
    k = gd.astype(np.int64) - minD
    assert (gd[pix] == np.rint(gd[pix])).all() and ((k[pix] >= 0) & (k[pix] < n)).all(), "winner outside [minD, minD + planes): " + where
    k = np.clip(k, 0, n - 1)[None]
    kmin = np.where(fin, wv, np.inf).argmin(axis=0)[None]
    at = lambda a, i: np.take_along_axis(a, i, axis=0)[0]
    ok = at(wv, k).astype(np.float64) <= at(wv, kmin).astype(np.float64) + at(tol, k) + at(tol, kmin)
    assert ok[pix].all(), "winner is no minimiser of the oracle's volume within the bound: " + where
