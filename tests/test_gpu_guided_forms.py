"""The guided-filter family (GuidedF, GuidedF_2, GuidedF_3) runs one of many kernel forms per call, chosen by frame size,
window, NaN safety and the AswTuning switches.  The oracle holds the family only to 1e-4 relative on the volume, so the forms
are pinned to each other bit for bit here -- the fused a/b -> q walk against the two passes, every band / ring / workgroup
partition against the default one, shared 6-channel guide statistics against plain per-slice ones -- and every case is also
checked against the oracle (volume within 1e-4 relative, WTA map index-exact)."""
import numpy as np
import pytest

import aswstereomatch_amd as asw
from aswstereomatch_amd.synth import make_pair, shifted_pair

pytestmark = pytest.mark.gpu
LEFT, RIGHT = asw.DISPARITY_LEFT, asw.DISPARITY_RIGHT
EPS = 1e-6

_CTX = {}


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _CTX.values():
        c.close()
    _CTX.clear()


def ctx(**env):
    """One context per switch set (asw_create reads the switches once)."""
    key = tuple(sorted(env.items()))
    if key not in _CTX:
        _CTX[key] = asw.Context(0, env={"ASW_" + k: str(v) for k, v in env.items()})
    return _CTX[key]


def run(c, kind, L, R, dt, win, minD, D):
    fn = {1: c.computeAdaptiveWeight_GuidedF, 2: c.computeAdaptiveWeight_GuidedF_2, 3: c.computeAdaptiveWeight_GuidedF_3}[kind]
    return fn(L, R, dt, EPS, win, minD, D, return_cost_volume=True)


def same(a, b):
    """bit for bit: volume and WTA map (NaN where NaN)"""
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True)


def ulps(a, b):
    """largest distance in f32 ulps between the finite entries of two volumes (for the failure message)"""
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    fin = np.isfinite(a) & np.isfinite(b)
    return int(np.abs(ia - ib)[fin].max()) if fin.any() else 0


def check_oracle(oracle, kind, L, R, dt, win, minD, D, got):
    fn = {1: oracle.asw_guided, 2: oracle.asw_guided2, 3: oracle.asw_guided3}[kind]
    rc, dw, vw = fn(L, R, int(dt), EPS, win, minD, D, want_vol=True)
    d, v = got
    assert rc == 0
    assert np.array_equal(np.isnan(v), np.isnan(vw)), "NaN pattern differs from the oracle"
    fin = np.isfinite(vw)
    assert np.allclose(v[fin], vw[fin], rtol=1e-4, atol=1e-6), "volume differs from the oracle"
    ok = fin.all(axis=0)  # the WTA of a pixel with a NaN cost follows the '<' of NaN comparisons: compared where all are finite
    assert np.array_equal(d[ok], dw[ok]), "WTA map differs from the oracle"


def near_min_pair(H, W, d0, off, seed):
    """Flat 16 x 16 colour blocks; R = L shifted by d0 and `off` levels brighter, a few saturated left pixels.  Inside the blocks
    the TAD C+G cost is the same constant > 0 at every d, so the slice minimum is not 0 and is attained over large flat areas,
    where raw * scale + shift leaves residues of a few ulps of 1 (or exactly 0, depending on the scale: `off` is chosen per
    shape so that residues occur) next to values near 1 -- f64 window sums of such costs are inexact."""
    rng = np.random.default_rng(seed)
    blocks = rng.integers(40, 200, ((H + 15) // 16, (W + d0 + 15) // 16, 3))
    wide = np.repeat(np.repeat(blocks, 16, 0), 16, 1)[:H, :W + d0].astype(np.int32)
    L = np.ascontiguousarray(wide[:, :W]).astype(np.uint8)
    R = np.ascontiguousarray(np.clip(wide[:, d0:d0 + W] + off, 0, 255)).astype(np.uint8)
    for _ in range(max(2, H * W // 2000)):
        L[rng.integers(0, H), rng.integers(0, W)] = (255, 0, 255)
    return L, R


def normalised_similarity(oracle, L, R, minD, D):
    rc, vol = oracle.compute_similarity(L, R, 0.4, 10, 50, 0, minD, D)
    out = []
    for p in np.asarray(vol):
        mn, mx = float(p.min()), float(p.max())
        sc = 1.0 / (mx - mn) if mx - mn > 2.220446049250313e-16 else 0.0
        out.append((p * np.float32(sc)).astype(np.float32) + np.float32(0.0 - mn * sc))
    return np.stack(out)


# ---------------------------------------------------------------- 1. fused a/b -> q walk against the two passes (GuidedF_2, 15x15)

FUSED_SHAPES = [  # H, W, n: odd W; W at / next to the 100-column strip of the fused walk; H not a multiple of the band; H = 16;
    (16, 99, 5), (16, 100, 1), (17, 101, 2), (23, 57, 5),   # one strip; n = 1, 2, 5, > 64
    (33, 199, 5), (47, 201, 70), (61, 131, 9), (75, 231, 12),
]
# near-minimum inputs: (H, W, n, brightness offset)
NEAR_MIN = [(16, 99, 5, 3), (23, 57, 5, 3), (16, 101, 6, 4), (47, 201, 70, 16), (61, 131, 9, 16), (75, 231, 12, 20)]


@pytest.mark.parametrize("H,W,n,off", [(H, W, n, None) for H, W, n in FUSED_SHAPES] + NEAR_MIN)
def test_fused_walk_equals_two_pass(oracle, H, W, n, off):
    if off is None:
        L, R, _ = make_pair(H, W, n, seed=H * 7 + W)
    else:
        L, R = near_min_pair(H, W, 3, off, seed=H + W)
        p = normalised_similarity(oracle, L, R, 0, n)
        assert ((p != 0) & (np.abs(p) < 2.0 ** -20)).any(), "the input has no near-minimum normalised costs"
    two = run(ctx(GUIDED_FUSED=0), 2, L, R, LEFT, 15, 0, n)
    assert ctx(GUIDED_FUSED=0).timing()["aggregate_launches"] == 4
    bands = [0] + ([30, 31, H - 1, H] if H > 31 else [])
    for b in bands:
        c = ctx(GUIDED_FUSED=1, BAND_Q=b) if b else ctx(GUIDED_FUSED=1)
        fused = run(c, 2, L, R, LEFT, 15, 0, n)
        assert c.timing()["aggregate_launches"] == 3, "the fused walk did not run"
        assert same(fused, two), (b, ulps(fused[1], two[1]))
    check_oracle(oracle, 2, L, R, LEFT, 15, 0, n, two)


def test_fused_walk_guard_at_minimum_height(oracle):
    """ASW_GUIDED_FUSED=1 is honoured from H = 16 (the walk mirrors 14 rows at each border); H = 15 runs the two passes."""
    for H, launches in ((15, 4), (16, 3)):
        L, R, _ = make_pair(H, 101, 6, seed=H)
        c = ctx(GUIDED_FUSED=1)
        got = run(c, 2, L, R, LEFT, 15, 0, 6)
        assert c.timing()["aggregate_launches"] == launches, H
        assert same(got, run(ctx(GUIDED_FUSED=0), 2, L, R, LEFT, 15, 0, 6)), H
        check_oracle(oracle, 2, L, R, LEFT, 15, 0, 6, got)


@pytest.mark.parametrize("H,launches,other", [(1000, 3, "0"), (999, 4, "1")])
def test_fused_threshold_on_a_default_context(H, launches, other):
    """guided_uses_fused: ceil(W/100) * n * H >= 2e6 takes the fused walk on a default context (W = 2000, n = 100: from
    H = 1000).  The a/b scratch is sized by the same decision (launch_guided refuses a two-pass run with a smaller one).
    GPU against GPU: the oracle is too slow at this size.
    Not bit for bit here: the fused walk sums the same real window sums in another f64 order (mirrored border windows, its own
    band partition), and at H = 999 the normalised costs a few ulps above the slice minimum share windows with costs near 1, so
    some of those sums are inexact (291 of the 900 first-stage sums around the pixel that differs): one volume entry of 2e8
    lands 1 f32 ulp away, the WTA map is the same.  Bound: WTA equal, volume within 1 ulp."""
    W, n = 2000, 100
    L, R, _ = make_pair(H, W, 64, seed=H, block=64)
    d = ctx()
    got = run(d, 2, L, R, LEFT, 15, 0, n)
    assert d.timing()["aggregate_launches"] == launches
    c = ctx(GUIDED_FUSED=other)
    forced = run(c, 2, L, R, LEFT, 15, 0, n)
    assert c.timing()["aggregate_launches"] == 7 - launches
    assert np.array_equal(got[0], forced[0]) and np.array_equal(np.isnan(got[1]), np.isnan(forced[1]))
    assert ulps(got[1], forced[1]) <= 1
    # a small frame on the same contexts afterwards: the scratch the large call left behind does not change the decision
    L, R, _ = make_pair(20, 130, 5, seed=3)
    assert same(run(d, 2, L, R, LEFT, 15, 0, 5), run(ctx(GUIDED_FUSED=0), 2, L, R, LEFT, 15, 0, 5))
    assert d.timing()["aggregate_launches"] == 4


# ---------------------------------------------------------------- 2. partitions of the two-pass walks
# Small frames: launch_walk_t halves the band until the launch has ~4096 wavefronts, so a forced band shrinks too there (and
# a band below 2k is raised to 2k first); the (97, 233, 160) shape keeps bands of 15+ rows, the small ones bands of 1-4 rows.

G2_SHAPES = [(40, 131, 9), (37, 100, 5), (97, 233, 160)]


def _bands(H, values):
    return sorted({b for b in values + [H - 1] if b >= 2})


@pytest.mark.parametrize("H,W,n", G2_SHAPES)
def test_guided2_two_pass_partitions(oracle, H, W, n):
    L, R, _ = make_pair(H, W, min(n, 40), seed=H * 3 + W)
    base = run(ctx(GUIDED_FUSED=0), 2, L, R, LEFT, 15, 0, n)
    envs = [dict(BAND_AB=b) for b in _bands(H, [2, 7, 29, 31])] + [dict(BAND_Q=b) for b in _bands(H, [2, 7, 29, 31])]
    envs += [dict(RING_AB=0), dict(RING_Q=0), dict(Q_WG_STRIPS=0), dict(RING_AB=0, RING_Q=0, Q_WG_STRIPS=0)]
    for e in envs:
        got = run(ctx(GUIDED_FUSED=0, **e), 2, L, R, LEFT, 15, 0, n)
        assert same(got, base), (e, ulps(got[1], base[1]))
    check_oracle(oracle, 2, L, R, LEFT, 15, 0, n, base)
    # other windows: the run-time-k walks (no ring)
    for win in (7, 21):
        base = run(ctx(), 2, L, R, LEFT, win, 0, n)
        for e in (dict(BAND_AB=H - 1), dict(BAND_Q=H - 1), dict(Q_WG_STRIPS=0)):
            assert same(run(ctx(**e), 2, L, R, LEFT, win, 0, n), base), (win, e)
        check_oracle(oracle, 2, L, R, LEFT, win, 0, n, base)


@pytest.mark.parametrize("H,W,n,minD", [(40, 131, 9, 0), (53, 233, 12, 5), (31, 77, 6, 2)])
@pytest.mark.parametrize("dt", [LEFT, RIGHT])
def test_guided6_pair_kernel_bands(oracle, H, W, n, minD, dt):
    """GuidedF at 15x15: k_ab6_pair / k_q6_pair honour any band of 16 rows or more."""
    L, R, _ = make_pair(H, W, n + minD, seed=H + W + int(dt))
    base = run(ctx(), 1, L, R, dt, 15, minD, n)
    for b in sorted({16, 17, 31, H - 1}):
        for e in (dict(BAND_AB=b), dict(BAND_Q=b), dict(BAND_AB=b, BAND_Q=b)):
            got = run(ctx(**e), 1, L, R, dt, 15, minD, n)
            assert same(got, base), (e, ulps(got[1], base[1]))
    assert same(run(ctx(AB6_PAIR=0, Q6_PAIR=0), 1, L, R, dt, 15, minD, n), base)
    check_oracle(oracle, 1, L, R, dt, 15, minD, n, base)


def flat_patch_pair(H, W, D, seed):
    """flat patches: every window inside one is constant, so the NCC cost there is 0/0 (as in test_gpu_edges.py; 20 x 24 and
    larger, so that 15 x 15 windows fit)"""
    L, R, _ = make_pair(H, W, D, seed=seed, block=8)
    L[8:28, 50:74] = 77
    R[8:28, 36:64] = 91
    L[H - 8:H - 5, W - 30:W - 24] = 5
    return L, R


@pytest.mark.parametrize("H,W,n,minD", [(40, 200, 12, 0), (37, 131, 9, 3)])
@pytest.mark.parametrize("dt", [LEFT, RIGHT])
@pytest.mark.parametrize("win", [3, 15])
def test_guided3_nan_safe_forms(oracle, H, W, n, minD, dt, win):
    """GuidedF_3 (NCC costs with NaN): LEFT runs the 6-channel guide (NaN-safe k_ab6_pair / k_q6_pair at 15x15, NaN-safe
    k_box_walk otherwise), RIGHT the 3-channel one (NaN-safe re-fetching walks): every partition gives the same bits and the same
    NaN pattern."""
    L, R = flat_patch_pair(H, W, n + minD, seed=H + W)
    base = run(ctx(), 3, L, R, dt, win, minD, n)
    assert np.isnan(base[1]).any() and np.isfinite(base[1]).mean() > 0.5
    envs = [dict(BAND_AB=b) for b in (16, 17, 31, H - 1)] + [dict(BAND_Q=b) for b in (16, 17, 31, H - 1)]
    envs += [dict(Q_WG_STRIPS=0), dict(AB6_PAIR=0), dict(Q6_PAIR=0), dict(GUIDE_SHARE=0)]
    for e in envs:
        got = run(ctx(**e), 3, L, R, dt, win, minD, n)
        assert same(got, base), (e, ulps(got[1], base[1]))
    check_oracle(oracle, 3, L, R, dt, win, minD, n, base)


# ---------------------------------------------------------------- 3. shared 6-channel guide statistics under many scale groups

def _reflect(p, n):
    """BORDER_REFLECT (the shifted view of GuidedF, M.cpp:2907-2912 / 2925-2929)"""
    if n == 1:
        return np.zeros_like(p)
    p = p.copy()
    while True:
        lo, hi = p < 0, p >= n
        if not (lo.any() or hi.any()):
            return p
        p[lo] = -p[lo] - 1
        p[hi] = 2 * n - 1 - p[hi]


def guide_scale_groups(L, R, dt, minD, n):
    """numpy restatement of launch_guide_scales_lr: normalize(NORM_MINMAX) of the 6-channel guide [fixed image, other image
    shifted by d] per slice, min / max over the fixed image and the columns of the other image the shifted view shows.
    Returns the distinct (scale, shift) f32 pairs in slice order (k_scale_groups compares them bitwise)."""
    ref, oth = (L, R) if dt == LEFT else (R, L)
    W = L.shape[1]
    cmin, cmax = oth.min(axis=(0, 2)).astype(np.float64), oth.max(axis=(0, 2)).astype(np.float64)
    x = np.arange(W)
    pairs = []
    for k in range(n):
        d = minD + k
        cols = _reflect(x - d if dt == LEFT else x + d, W)
        mn, mx = min(float(ref.min()), cmin[cols].min()), max(float(ref.max()), cmax[cols].max())
        sc = 1.0 / (mx - mn) if mx - mn > 2.220446049250313e-16 else 0.0
        pair = (np.float32(sc).view(np.uint32), np.float32(0.0 - mn * sc).view(np.uint32))
        if pair not in pairs:
            pairs.append(pair)
    return pairs


def grouped_pair(H, W, minD, n, groups, dt, seed):
    """A LEFT pair (fixed image L, shifted image R read at x - d) with a chosen number of guide-scale groups; for RIGHT the
    shifted image is mirrored so that the same columns leave the view (L read at x + d):
      one:   natural images (the global extrema stay in view at every d);
      every: the fixed image keeps to [100, 140], the shifted one is a horizontal ramp whose maximum sits in the column that
             leaves the view as d grows -- a new maximum, hence a new scale, in every slice;
      few:   the shifted image keeps to [60, 90] but for a bright and a dark column that leave the view at d = minD + 6 and
             minD + 14 -- three groups."""
    rng = np.random.default_rng(seed)
    if groups == "one":
        L, R, _ = make_pair(H, W, minD + n, seed=seed)
        return L, R
    F = rng.integers(100, 141, (H, W, 3)).astype(np.uint8)
    if groups == "every":
        base = 20 + 2 * np.arange(W)
        assert base[-1] <= 255
        S = base[None, :, None] - rng.integers(0, 7, (H, W, 3))
        S[0] = base[:, None]  # every column reaches its ramp value
    else:
        S = rng.integers(60, 91, (H, W, 3))
        S[:, W - 1 - (minD + 5)] = 255
        S[:, W - 1 - (minD + 13)] = 0
    S = S.astype(np.uint8)
    if dt == LEFT:
        return F, S
    return np.ascontiguousarray(S[:, ::-1]), F


SHARE_CASES = [(kind, dt) for kind, dt in ((1, LEFT), (1, RIGHT), (3, LEFT))]


@pytest.mark.parametrize("kind,dt", SHARE_CASES)
@pytest.mark.parametrize("groups", ["one", "every", "few"])
@pytest.mark.parametrize("win", [15, 7, 35])
@pytest.mark.parametrize("minD", [0, 9])
def test_shared_guide_statistics(oracle, kind, dt, groups, win, minD):
    """GuidedF / GuidedF_3 (6-channel guide): statistics shared across the slices of a scale group (fixed word: the group
    representative's; shifted word: the unshifted image's at x + sgn*d away from the border strips) against plain per-slice
    statistics (ASW_GUIDE_SHARE=0), bit for bit.  Win 15 runs the pair kernels, 7 and 35 the k_box_walk a/b forms (one / two
    columns per lane)."""
    H, W, n = 30, 118, 24
    L, R = grouped_pair(H, W, minD, n, groups, dt, seed=win * 10 + minD + int(dt))
    want = {"one": 1, "every": n, "few": 3}[groups]
    assert len(guide_scale_groups(L, R, dt, minD, n)) == want
    shared = run(ctx(), kind, L, R, dt, win, minD, n)
    plain = run(ctx(GUIDE_SHARE=0), kind, L, R, dt, win, minD, n)
    assert same(shared, plain), ulps(shared[1], plain[1])
    check_oracle(oracle, kind, L, R, dt, win, minD, n, shared)
