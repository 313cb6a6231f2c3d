"""The widths at which the two "one workgroup per row" cost kernels change behaviour (k_cost_ad<C> of k_basic.hip, k_cost_census<C> of
k_census.hip), shared by tests/test_wide_rows_cpu.py (the table and the references alone) and tests/test_gpu_wide_rows.py (the kernels).

Both kernels stage whole rows in dynamic LDS and walk a row 1024 pixels a pass (256 threads x 4 pixels), so two things depend on the
frame width alone: which pass writes a pixel, and how much LDS a launch asks for.  The two budgets below restate the launchers'
formulas; tests/test_wide_rows_cpu.py holds every width of the table to the side of 64 KB and 160 KB its label names, so a launcher
whose budget changes moves the table with it or fails there.

    ad_lds(W, C), census_lds(W, C)   bytes of dynamic LDS of launch_cost_ad / launch_cost_census (C = 0: the Hamming-only form)
    PASSES                           (width, passes of the x4 loop, what the width is for): all well under 64 KB
    LINE_64K[form]                   (last width at or under 64 KB, first over it, next over it with W % 4 == 0)
    LINE_160K[form]                  (last width the launcher accepts, first it refuses with ERR_BAD_ARGUMENT)
    random_pair, region_pair         the inputs
    COST_CASES_LOW / _HIGH, LIMIT_CASES, ADCENSUS_MATCH_*, CROSS_MATCH_*   the cases of the GPU file, under 64 KB first"""
import numpy as np

import adcensus_ref as ac
import cross_ref as cr

LDS_64K = 64 * 1024     # above it five other launchers set hipFuncAttributeMaxDynamicSharedMemorySize first
LDS_LIMIT = 160 * 1024  # what both launchers refuse above
PASS_PIXELS = 1024      # 256 threads x 4 pixels


def ad_lds(W, C):
    return 2 * W * C


def census_lds(W, C):
    return 16 * W + (2 * W * C + 320 if C else 0)


def passes(W):
    return -(-W // PASS_PIXELS)


# form -> (budget, C of the budget, image channels of the cases that exercise it)
FORMS = {
    "adcensus3": (census_lds, 3, 3),
    "adcensus1": (census_lds, 1, 1),
    "hamming": (census_lds, 0, 3),
    "ad3": (ad_lds, 3, 3),
    "ad1": (ad_lds, 1, 1),
}
CENSUS_FORMS = ("adcensus3", "adcensus1", "hamming")
AD_FORMS = ("ad3", "ad1")


def form_lds(form, W):
    fn, C, _ = FORMS[form]
    return fn(W, C)


# width, passes, rows of the cost cases, what it is for
PASSES = [
    (1023, 1, 3, "one pass, the last group short of a pixel"),
    (1024, 1, 1, "one whole pass"),
    (1025, 2, 5, "byte stores, the second pass owns one pixel"),
    (1028, 2, 5, "dword rows, the second pass owns one group"),
    (1920, 2, 2, "the workload's width"),
    (2049, 3, 4, "a third pass"),
]

LINE_64K = {
    "adcensus3": (2964, 2965, 2968),
    "adcensus1": (3623, 3624, 3628),
    "hamming": (4096, 4097, 4100),  # 4096: exactly 64 KB
    "ad3": (10922, 10923, 10924),
    "ad1": (32768, 32769, 32772),
}

LINE_160K = {
    "adcensus3": (7432, 7433),
    "adcensus1": (9084, 9085),
    "hamming": (10240, 10241),
    "ad3": (27306, 27307),
    "ad1": (81920, 81921),
}

MIN_D, NUM_D = 3, 17  # two candidate slabs of 16, the second with one plane
TAD_THRESHOLD = 30
FLAT = 24             # columns of the flat patches of random_pair


def random_pair(H, W, cn, seed, pad=0):
    """Seeded random uint8 pair (Hamming distances up to about 60, AD-Census costs above 127, saturating channel sums).  The first and
    the last FLAT columns of row 0 hold one value in both images: an absolute difference of 0 in every plane there, so that the TAD
    mask holds a 0 past column 1024 even where one column lies there.  pad > 0: views of wider arrays, rows that carry padding."""
    rng = np.random.default_rng(seed)
    shp = (H, W + pad, 3) if cn == 3 else (H, W + pad)
    L = rng.integers(0, 256, shp).astype(np.uint8)
    R = rng.integers(0, 256, shp).astype(np.uint8)
    if W >= 2 * FLAT:
        for img in (L, R):
            img[0, :FLAT] = 77
            img[0, W - FLAT:W] = 77
    return L[:, :W], R[:, :W]


def cost_pair(H, W, cn, dt, pad=0):
    """the random pair of a cost-builder case"""
    return random_pair(H, W, cn, 16 * W + 4 * H + 2 * (cn == 3) + dt, pad)


def region_pair(H, W, cn, D, pad=0):
    """cross_ref.region_pair as tests/test_gpu_cross.py and tests/test_gpu_adcensus.py call it"""
    L, R, _ = cr.region_pair(H, W + pad, max(2, D), H * 1000 + W, (5, 7), 0.12, block=8)
    if cn == 1:
        L, R = np.ascontiguousarray(L[:, :, 1]), np.ascontiguousarray(R[:, :, 1])
    return L[:, :W], R[:, :W]


def _rows_at_line(i):
    return (2, 5, 3)[i]  # last at or under 64 KB, first over, next over with W % 4 == 0


def is_ad_kernel(kernel):
    return kernel in ("ad",) + AD_FORMS


def expected_costs(oracle, kernel, L, R, dt, minD, D):
    """name -> expected uint8 volume [D][H][W] of every cost builder a case of `kernel` runs: the CPU oracle for k_cost_ad's three
    forms, tests/adcensus_ref.py for k_cost_census's two"""
    if is_ad_kernel(kernel):
        out = {}
        for name, (rc, vol) in (("AD", oracle.compute_ad(L, R, dt, minD, D)), ("TAD", oracle.compute_tad(L, R, dt, TAD_THRESHOLD, minD, D)),
                                ("SD", oracle.compute_sd(L, R, dt, minD, D))):
            assert rc == 0
            out[name] = vol
        return out
    out = {"Census": ac.hamming(L, R, dt, minD, D)}
    if kernel != "hamming":
        out["ADCensus"] = ac.cost(L, R, dt, LAMBDA_AD, LAMBDA_CENSUS, minD, D)
    return out


def expected_cross(oracle, L, R, dt, win, minD, D):
    """S, N, E, disp of entry 12 over the ORACLE's AD volume: the wide cases do not lean on k_cost_ad"""
    rc, e = oracle.compute_ad(L, R, dt, minD, D)
    assert rc == 0
    return cr.aggregate(e, cr.arms(R if dt else L, TAU, win // 2), TRUNC, minD)


def expected_adcensus(L, R, dt, win, minD, D):
    return ac.match(L, R, dt, TAU, LAMBDA_AD, LAMBDA_CENSUS, win, minD, D)


# ---- the cost-builder cases: (kernel, H, W, channels, direction, minD, D); kernel "ad" runs computeAD / TAD / SD, "census" runs
# computeCensus and computeADCensus.  Every passes width in both directions and channel counts; the reflection case of each kernel
def _low_cases():
    out = []
    for kernel in ("ad", "census"):
        for W, _, H, _ in PASSES:
            for cn in (3, 1):
                for dt in (0, 1):
                    out.append((kernel, H, W, cn, dt, MIN_D, NUM_D))
        out.append((kernel, 3, 2049, 3, 0, 2049 - 5, NUM_D))  # min_d = W - 5: every partner column reflected, on a wide row
        out.append((kernel, 2, 1028, 1, 1, 1028 - 5, NUM_D))
    return out


# every width of the 64 KB line of the forms a kernel has, with the channel count of the form, in both directions.  "hamming" cases
# run computeCensus alone (computeADCensus at these widths is an adcensus3 launch of no special size)
def _high_cases():
    out = []
    for form in AD_FORMS + CENSUS_FORMS:
        for i, W in enumerate(LINE_64K[form]):
            for dt in (0, 1):
                out.append((form, _rows_at_line(i), W, FORMS[form][2], dt, MIN_D, NUM_D))
    return out


COST_CASES_LOW = _low_cases()
COST_CASES_HIGH = _high_cases()
PADDED_CASE = (3, 1025, 3, 0, MIN_D, NUM_D, 5)  # H, W, channels, direction, minD, D, pad

# accepted at the limit, refused one past it: (form, H, last accepted, first refused, direction), two candidates
LIMIT_MIN_D, LIMIT_NUM_D = 3, 2
LIMIT_CASES = [(form, 1 + i % 2, LINE_160K[form][0], LINE_160K[form][1], i % 2) for i, form in enumerate(AD_FORMS + CENSUS_FORMS)]

# ---- the matcher cases: H, W, channels, win, minD, D, direction
ADCENSUS_MATCH_LOW = [(34, 1920, 3, 15, 0, 17, 0), (34, 1920, 3, 15, 0, 17, 1)]
ADCENSUS_MATCH_HIGH = [(6, 2968, 3, 7, 0, 5, 0), (5, 3628, 1, 3, 0, 3, 1)]
CROSS_MATCH_LOW = [(34, 1920, 3, 15, 0, 17, 0), (34, 1920, 3, 15, 0, 17, 1)]
CROSS_MATCH_HIGH = [(3, 10924, 3, 7, 0, 3, 0)]
TAU, TRUNC, LAMBDA_AD, LAMBDA_CENSUS = 20, 20, 10, 30

# ---- winnerTakeAll: launch_wta takes k_wta<4> from 2^20 pixels up, and there its scalar branch when the plane is no multiple of 4
WTA_SWITCH = 1 << 20
WTA_N = 3
WTA_CASES = [(1023, 1025, "k_wta<1>"), (1024, 1024, "k_wta<4> vector"), (1025, 1025, "k_wta<4> scalar")]


def wta_volume(H, W, seed):
    """n = 3 planes; even rows quantised to sixteenths (ties everywhere: the lowest d wins), and the special columns of test_wta at
    the start of the first row, the start of the last row and the end of the plane (its last four pixels and the one before)."""
    rng = np.random.default_rng(seed)
    vol = rng.random((WTA_N, H, W), dtype=np.float32)
    vol[:, ::2] = np.floor(vol[:, ::2] * 16) / 16
    flat = vol.reshape(WTA_N, H * W)

    def special(i, kind):
        if kind == 0:
            flat[:, i] = np.nan         # all-NaN column -> 0
        elif kind == 1:
            flat[:, i] = 0.5            # ties -> lowest d
        elif kind == 2:
            flat[0, i] = np.inf         # a leading +inf loses to what follows
        elif kind == 3:
            flat[:, i] = np.inf         # (double)inf < DBL_MAX is false -> never selected -> 0
        else:
            flat[0, i] = 0.25
            flat[1:, i] = -np.inf       # -inf wins once, the tie after it does not
    for base in (0, (H - 1) * W):
        for kind in range(5):
            special(base + kind, kind)
    for i, kind in zip(range(H * W - 5, H * W), (2, 0, 1, 3, 4)):
        special(i, kind)
    return vol
