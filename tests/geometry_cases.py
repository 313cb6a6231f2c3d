"""The frames at which the host launchers change their launch geometry, shared by tests/test_geometry_cases_cpu.py (the table and the
references alone) and tests/test_gpu_launch_geometry.py (the kernels).

Several launchers size a chunk, a tile or a candidate slice from the number of workgroups a frame gives: the form changes loop trip
counts, LDS tile widths and which slices a merge kernel sees.  The decisions count workgroups, not pixels, so a tall narrow frame
takes the large-frame form with a few hundred thousand pixels.  Every formula below restates one launcher; the named constants are
read back from the source text by tests/test_geometry_cases_cpu.py, so a changed launcher fails there instead of leaving this table
stale.  A value is left out only where its smallest frame has more than MAX_PIXELS pixels: NOT_REACHED names each with that frame.
The sections follow the list below.

    sim_launch(H, W, numD)             launch_similarity (k_cost.hip): dch, z slices, the short last slice, column blocks
    split_launch(H, W, nD, target)     launch_t (k_bilateral.hip, target 2048) / launch_geo_t (k_geodesic.hip, 4096): nz, cand_per_z
    bm_launch(H, W, minD, D, w)        launch_match (k_bm.hip): TX, rows_per, strips
    census_launch(H, W, minD, D, w)    launch_hcost_census (k_sgbm.hip): spb, want, nseg, seglen, gy
    disp_u8_blocks / slice_scales_blocks / u8_scale_blocks   the capped grids of k_prep.hip and k_cost.hip
    perm_chunk(H, W, n) / wmedian_chunk(H, W, win, n)        the natural chunk sizes of asw_methods.hip, and the frames past them
    NOT_REACHED                                              what stays out, and the frame that would reach it
    band_pair, gray_band_pair          the inputs: row bands of known disparity, so that winners spread over the candidate range"""
import numpy as np

MAX_PIXELS = 1 << 21


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------- the inputs
def band_pair(H, W, dmax, seed, band=5):
    """3-channel pair of a smoothed random texture; rows [i * band, (i + 1) * band) of the right image are the left image shifted
    by d_i = floor(frac((i + seed) * 0.618...) * dmax) columns (L(x) = R(x - d_i) exactly), dmax <= W - 2: the winner of a row
    band is d_i wherever x >= d_i, and the golden-ratio sequence spreads a few bands over the whole range."""
    assert 1 <= dmax <= max(1, W - 2)
    rng = np.random.default_rng(seed)
    tex = rng.integers(0, 256, (H + 2, W + dmax + 2, 3)).astype(np.float32)
    acc = np.zeros((H, W + dmax, 3), np.float32)
    for dy in range(3):
        for dx in range(3):
            acc += tex[dy:dy + H, dx:dx + W + dmax]
    wide = np.clip((acc / 9.0 - 128.0) * 2.5 + 128.0, 0, 255).astype(np.uint8)
    L = np.ascontiguousarray(wide[:, :W])
    R = np.empty_like(L)
    for i, y in enumerate(range(0, H, band)):
        d = int((i + seed) * 0.6180339887498949 % 1.0 * dmax)
        R[y:y + band] = wide[y:y + band, d:d + W]
    return L, R


def gray_band_pair(H, W, dmax, seed, band=5):
    L, R = band_pair(H, W, dmax, seed, band)
    return np.ascontiguousarray(L[:, :, 1]), np.ascontiguousarray(R[:, :, 1])


def gray_noise_band_pair(H, W, dmax, seed, band=5):
    """band_pair's shifts on one channel of plain noise: a tenth of its time on the frames of a million pixels"""
    assert 1 <= dmax <= max(1, W - 2)
    rng = np.random.default_rng(seed)
    wide = rng.integers(0, 256, (H, W + dmax), dtype=np.uint8)
    nb = cdiv(H, band)
    d = ((np.arange(nb) + seed) * 0.6180339887498949 % 1.0 * dmax).astype(np.int64)
    cols = np.repeat(d, band)[:H, None] + np.arange(W)[None, :]
    return np.ascontiguousarray(wide[:, :W]), np.take_along_axis(wide, cols, axis=1)


def dmax_for(W, n):
    """the disparities a band pair of width W can hold among n candidates"""
    return max(1, min(n, W - 2))


# ---------------------------------------------------------------- launch_similarity, k_cost.hip
SIM_ROWS, SIM_COLS, SIM_DCH, SIM_DCH_MIN, SIM_WG_TARGET = 4, 256, 512, 8, 4096
SIM_DCH_VALUES = (8, 16, 32, 64, 128, 256, 512)


def sim_launch(H, W, numD):
    """launch_similarity: dch = SIM_DCH; while (dch > 8 && wg_xy * ceil(numD / dch) < sim_wg_target) dch /= 2"""
    gx, gy = cdiv(W, SIM_COLS), cdiv(H, SIM_ROWS)
    dch = SIM_DCH
    while dch > SIM_DCH_MIN and gx * gy * cdiv(numD, dch) < SIM_WG_TARGET:
        dch //= 2
    nz = cdiv(numD, dch)
    return {"dch": dch, "nz": nz, "last": numD - (nz - 1) * dch, "gx": gx, "gy": gy,
            "lds": SIM_ROWS * ((SIM_COLS + min(numD, dch)) & ~1) * 12 + 512 * 4}


# dch -> (H, W, minD, numD): the least H of a frame of this width and candidate count that takes dch (one row less gives dch / 2);
# numD > dch and numD % dch != 0 everywhere: more than one z slice, the last one short.  H is odd: the last row block holds one row
SIM_FIRST = {
    8: (9, 300, 1, 13),            # small frames stay at 8; two column blocks
    16: (8189, 11, 0, 24),
    32: (8189, 9, 3, 50),
    64: (8189, 7, 0, 100),
    128: (8189, 9, 2, 136),
    256: (8189, 9, 0, 264),
    512: (8189, 9, 1, 520),        # two z slices, the last of 8 candidates
}
# The reflected right image repeats every 2 W offsets.  No case has a width with dch % (2 W) == 0, so planes k and k + dch, which
# two different z slices write, hold different values: tests/test_geometry_cases_cpu.py asserts both.  Few candidates past dch: the
# oracle walks the reflection of a far offset step by step, and its time grows with numD^2 on a narrow frame.
# W > 256, W % 256 != 0 at a dch > 8: two column blocks, the second 3 columns wide, x 1024 row blocks x 2 slices
SIM_WIDE = (4093, 259, 2, 17, 16)  # H, W, minD, numD, dch
SIM_PAD_WIN = 5                    # winSize of the padded overload
SIM_PARAMS = (0.4, 10.0, 50.0)     # regularity, thresC, thresG of the reference's call sites


def sim_cases():
    """(H, W, minD, numD, dch) of every similarity case"""
    return [(H, W, minD, numD, dch) for dch, (H, W, minD, numD) in SIM_FIRST.items()] + [SIM_WIDE]


def sim_pair(H, W, numD, seed):
    return band_pair(H, W, dmax_for(W, numD), seed)


# one large-dch case each of GuidedF_2 and the weighted median: (H, W, win, minD, numD, dch)
GUIDED2_CASE = (8189, 7, 5, 0, 70, 64)
WMEDIAN_CASE = (8189, 7, 3, 0, 70, 64)

# section 5 of the issue: the parameter values at which the integer / float forms of the two double comparisons could differ
THRES_C = (0.0, 0.5, 9.999, 10.0, 254.6, 300.0)
THRES_G = (0.0, 49.5, float(np.nextafter(50.0, 0.0)), 50.0, 1e9)
REGULARITY = (0.0, 0.4, 1.0)
PARAM_FRAME = (11, 37, 2, 11)      # H, W, minD, numD


def param_pair():
    """the band pair with its gradients and colours spread: a quarter of the right image is replaced by noise, so that colour sums
    reach the top of the range and gradient sums cross every thresG of the list"""
    H, W, minD, numD = PARAM_FRAME
    L, R = band_pair(H, W, 9, 5)
    rng = np.random.default_rng(17)
    R = R.copy()
    R[:, W // 2:W // 2 + W // 4] = rng.integers(0, 256, R[:, W // 2:W // 2 + W // 4].shape)
    L = L.copy()
    L[:3] = (L[:3].astype(np.int32) // 64 * 85).astype(np.uint8)  # saturated steps: large Scharr responses
    return L, R


# ---------------------------------------------------------------- launch_t (k_bilateral.hip), launch_geo_t (k_geodesic.hip)
TILE_W, TILE_H = 64, 4
BIL_TARGET, GEO_TARGET = 2048, 4096
MAX_SLICES = 8
SPLIT_MAX_PLANE = 1 << 20  # run_bilateral / run_geodesic (asw_methods.hip) hand out slice scratch up to here only
XQ_MIN_W, XQ_MIN_CANDIDATES = 64, 64


def split_launch(H, W, nD, target):
    """launch_t / launch_geo_t for a whole frame from candidate 0: (nz, cand_per_z)"""
    tiles, chunks16 = cdiv(W, TILE_W) * cdiv(H, TILE_H), cdiv(nD, 16)
    nz = 1
    if H * W <= SPLIT_MAX_PLANE and tiles < target:
        nz = min(chunks16, MAX_SLICES, cdiv(target, tiles))
    per_z = cdiv(chunks16, nz)
    return cdiv(chunks16, per_z), per_z * 16


def takes_xq(W, win, nD):
    """run_bilateral / run_geodesic: the 15x15 problem goes to the xq kernels from 64 candidates and 64 columns up"""
    return win == 15 and W >= XQ_MIN_W and nD >= XQ_MIN_CANDIDATES


# kernel -> (method, window, target).  classic15 / classic35 / classic5: the three instantiations launch_bilateral chooses from
SPLIT_KERNELS = {
    "classic15": ("classic", 15, BIL_TARGET),
    "classic35": ("classic", 35, BIL_TARGET),
    "classic5": ("classic", 5, BIL_TARGET),
    "geodesic15": ("geodesic", 15, GEO_TARGET),
    "geodesic5": ("geodesic", 5, GEO_TARGET),
}


def _split_cases(kernel):
    """(H, W, win, minD, numD, nz, cand_per_z, what): numD + 1 candidates (the reference's inclusive range).  W < 64 throughout: one
    tile column, and the 15x15 cases stay with the one-kernel form.  The decision reads the tile and candidate counts alone, never
    the window: the frames of thousands of rows and tens of columns, which two slices by the tile count need, run at window 5, whose
    oracle a quick test can afford; the 4-column frame of one slice of 17 candidates and the frames of a few tiles run at every
    window"""
    _, win, target = SPLIT_KERNELS[kernel]
    rows = TILE_H * target            # tiles >= target from H = rows - 3 on
    geo = SPLIT_KERNELS[kernel][0] == "geodesic"
    out = []
    for nz in range(1, 9):            # few tiles: the candidate count decides
        out.append((21 + nz % 3, 63 - nz, win, nz % 2 * 2, 16 * nz - 1 - (nz > 1) * (nz % 4), nz, 16, "nz %d by the candidate count" % nz))
    out.append((22, 52, win, 0, 128, 5, 32, "129 candidates over 8 slices: 32 a slice, 5 slices"))
    # (a frame on which the winners of both directions reach the second slice: 14 rows do at 35x35, the dearest oracle)
    out.append((14 if win == 35 else 32, 52 if win == 35 else 60, win, 0, 256, 6, 48, "257 candidates over 8 slices: 48 a slice, 6 slices"))
    out.append((rows - 3, 4, win, 0, 16, 1, 32, "the first frame with tiles >= target: one slice of 17 candidates"))
    if win == 5:
        # half the target: two slices by the tile count, whatever the candidate count
        out.append((rows // 2 - 3, 35, win, 0, 32, 2, 32, "two slices of 32 by the tile count"))
        if not geo:
            out.append((rows // 2 - 3, 52, win, 1, 64, 2, 48, "two slices of 48 by the tile count"))
    return out


SPLIT_CASES = {k: _split_cases(k) for k in SPLIT_KERNELS}


def split_threshold_pairs(kernel):
    """[(last frame on one side, first frame on the other, nD, (nz, cand_per_z) of each)]: one row of tiles less changes the form"""
    _, _, target = SPLIT_KERNELS[kernel]
    rows = TILE_H * target
    return [((rows - 4, 9), (rows - 3, 9), 18, (2, 16), (1, 32)),
            ((rows // 2 - 4, 42), (rows // 2 - 3, 42), 40, (3, 16), (2, 32))]


def split_pair(H, W, numD, seed):
    return band_pair(H, W, dmax_for(W, numD + 1), seed)


# ---------------------------------------------------------------- launch_match, k_bm.hip
BM_WAVES_TARGET, BM_STRIP_ROWS, BM_TX_MIN, BM_ROWS_MIN = 4096, 16, 8, 8


def bm_npl(D):
    """dispatch_npl (asw_host.h)"""
    npl = cdiv(D, 64)
    return next(v for v in (1, 2, 4, 8, 16) if npl <= v)


def bm_launch(H, W, minD, D, w):
    h, lofs = w // 2, minD + D - 1
    Hv, Wx, npl = H - 2 * h, W - lofs, bm_npl(D)
    TX = min(64, 4096 // (npl * 64))
    while TX > BM_TX_MIN and cdiv(Wx, TX) * cdiv(Hv, BM_STRIP_ROWS) < BM_WAVES_TARGET:
        TX //= 2
    tiles = cdiv(Wx, TX)
    rows_per = max(cdiv(Hv, max(1, BM_WAVES_TARGET // tiles)), BM_ROWS_MIN)
    return {"TX": TX, "npl": npl, "tiles": tiles, "rows_per": rows_per, "strips": cdiv(Hv, rows_per)}


# TX -> (H, W, minD, D, w): the least H at this width, window 5, 16 candidates.  A frame needs W - (minD + D - 1) > 2 h valid
# columns; 16 valid rows make one row of wavefronts
BM_FIRST = {
    4: (20, 1100, 0, 1024, 5),      # 16 planes per lane: TX starts at 4 and is never halved
    8: (37, 131, 3, 32, 9),         # small frames end at 8
    16: (32757, 32, 0, 16, 5),      # 17 columns: 2 tiles of 16, 1 of 32; 2048 rows of wavefronts
    32: (32757, 48, 0, 16, 5),      # 33 columns: 2 tiles of 32, 1 of 64
    64: (65525, 24, 0, 16, 5),      # one tile of any width: 4096 rows of wavefronts
}
BM_SETTINGS = (31, 10, 15, 0, 0, -1)  # preFilterCap, textureThreshold, uniquenessRatio, speckleWindowSize, speckleRange, disp12MaxDiff


# ---------------------------------------------------------------- launch_hcost_census, k_sgbm.hip
CENSUS_WG_TARGET, CENSUS_SEG_MIN = 2048, 32


def census_launch(H, W, minD, D, w):
    h, Wv = w // 2, W - (minD + D)
    spb = 256 // min(D, 256)
    want = spb * cdiv(CENSUS_WG_TARGET, H)
    by_width = Wv // max(CENSUS_SEG_MIN, 2 * (2 * h + 1))
    nseg = max(1, min(want, by_width))
    seglen = cdiv(Wv, nseg)
    return {"spb": spb, "want": want, "by_width": by_width, "nseg": nseg, "seglen": seglen, "gy": cdiv(Wv, seglen * spb)}


# The frame decides through `want` (rows x candidates), the width through Wv / 32.  The kernel is handed seglen and a grid of H x gy
# alone: whether the rows or the width cut the segments does not reach it.  CENSUS_BY_ROWS are the frames on which the rows decide
# (what -> H, W, minD, D, w, nseg); the table test holds them to the formula.  Their restatement in Python takes a second or more at
# 2048 rows, so the GPU runs CENSUS_CASES: a few rows that give the kernel the same spb, the same segments a row and the same gy
CENSUS_BY_ROWS = {
    "one segment by the rows": (2048, 144 + 64, 0, 144, 3, 1),             # 64 valid columns would allow two
    "two segments by the rows": (1024, 144 + 96, 0, 144, 3, 2),            # 96 valid columns would allow three
}
CENSUS_LAST_UNDER = (2047, 144 + 64, 0, 144, 3, 2)  # one row less than "one segment by the rows": two segments again
CENSUS_CASES = {
    "one segment, one candidate a thread": (7, 144 + 63, 0, 144, 3, 1),    # the launch of "one segment by the rows" on 7 rows
    "two segments, one candidate a thread": (6, 144 + 95, 0, 144, 3, 2),   # the launch of "two segments by the rows" on 6 rows
    "many segments": (3, 2100, 5, 16, 5, 64),                              # what sgbm_census_ref.SHAPES[9] runs today
}
CENSUS_SAME_LAUNCH = {"one segment, one candidate a thread": "one segment by the rows",
                      "two segments, one candidate a thread": "two segments by the rows"}
CENSUS_SETTINGS = (72, 288, 1, 10, 0, 0)  # P1, P2, disp12MaxDiff, uniquenessRatio, speckleWindowSize, speckleRange
CENSUS_PATHS = 0x07


# ---------------------------------------------------------------- the capped grids
def disp_u8_blocks(n):
    """launch_disp_to_u8 (k_prep.hip): 256 threads x 8 elements a block, at most 1024 blocks"""
    return max(1, min(1024, cdiv(n, 256 * 8)))


def slice_scales_blocks(plane):
    """launch_slice_scales (k_cost.hip): 256 threads x 16 floats a block, at most 64 blocks a slice"""
    return max(1, min(64, cdiv(plane, 256 * 16)))


def u8_scale_blocks(nbytes):
    """launch_u8_scale (k_cost.hip): 256 threads x 64 bytes a block, at most 1024 blocks"""
    return max(1, min(1024, cdiv(nbytes, 256 * 64)))


DISP_U8_CAP, SLICE_SCALES_CAP, U8_SCALE_CAP = 1024 * 256 * 8, 64 * 256 * 16, 1024 * 256 * 64
# just past the cap of launch_disp_to_u8, which IS 2^21 elements: 32 rows of 64 columns more
DISP_U8_FRAME = (32800, 64)        # H, W: 2 099 200 pixels
DISP_U8_MATCH = (3, 2, 7)          # win, minD, numD of the classic matcher that fills the map: 8 taps x 8 candidates, the cheapest method
DISP_U8_MID, DISP_U8_TOP = 5, 9    # the disparity of the frame, and of its rows from DISP_U8_ROW on
DISP_U8_ROW = 32772                # four rows past the cap: the 3x3 windows of the rows under the cap see none of them


def disp_u8_pair():
    """the right image is the left one shifted by DISP_U8_MID, except the rows from DISP_U8_ROW on, shifted by DISP_U8_TOP = minD +
    numD: the map's maximum, which normalize needs, lies only in what the capped grid reads in its last round"""
    def run():
        H, W = DISP_U8_FRAME
        rng = np.random.default_rng(2047)
        wide = rng.integers(0, 256, (H, W + DISP_U8_TOP, 3)).astype(np.uint8)
        L = np.ascontiguousarray(wide[:, :W])
        R = np.ascontiguousarray(wide[:, DISP_U8_MID:DISP_U8_MID + W])
        R[DISP_U8_ROW:] = wide[DISP_U8_ROW:, DISP_U8_TOP:DISP_U8_TOP + W]
        return L, R
    return _once("disp_u8_pair", run)


def expected_disp_u8_map(oracle):
    def run():
        win, minD, numD = DISP_U8_MATCH
        rc, d = oracle.asw_classic(*disp_u8_pair(), 30, 20, 0, win, minD, numD)[:2]
        assert rc == 0
        return d
    return _once("disp_u8_map", run)


# past the cap of launch_slice_scales, plane % 4 == 0 (the float4 loop's second round) and plane % 4 != 0 (the scalar loop)
SLICE_SCALES_FRAMES = [(260, 1012), (263, 1001)]  # 263 120 and 263 263 pixels
SLICE_SCALES_NCC = (3, 1, 2)       # win, minD, numD of computeNCC_costs(normalized) there


def slice_scales_pair(H, W):
    """independent noise (NCC costs in the middle of their range) except for the last two rows from column 100 on, where the right
    image is the left one shifted by minD: the extreme of plane 0 lies past the cap, in what only a later round of the loop reads"""
    rng = np.random.default_rng(H + W)
    L = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    R = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    d = SLICE_SCALES_NCC[1]
    R[H - 2:, 100 - d:W - d] = L[H - 2:, 100:]
    return L, R


# ---------------------------------------------------------------- the natural chunk sizes, asw_methods.hip
PERM_SEG = 16
BUDGET = 2 << 30


def perm_chunk(H, W, n):
    """run_permeability: candidates per chunk with no ASW_PERM_CHUNK"""
    seg = lambda v: cdiv(v, PERM_SEG)
    pad = lambda v: seg(v) * PERM_SEG + PERM_SEG
    plane = H * W
    ck_per = max(H * seg(W), W * seg(H))
    fixed = (2 * plane + ck_per + H * pad(W) + 2 * W * pad(H)) * 8 + plane
    per_cand = (plane + ck_per) * 8
    fit = (BUDGET - fixed) // per_cand if BUDGET > fixed + per_cand else 1
    chunk = min(fit, min(n, 4096))
    if chunk < n and chunk >= 64:
        chunk = chunk // 64 * 64
    return chunk


def wmedian_chunk(H, W, win, n):
    """run_wmedian's tile forms: slices per list chunk with no ASW_WMEDIAN_TILE_CHUNK"""
    blocks = cdiv(W, 8) * cdiv(H, 8)
    nreg = (8 + win - 1) ** 2
    slots = 512 if win == 15 else (256 if nreg <= 256 else 512 if nreg <= 512 else 1024 if nreg <= 1024 else 2048)
    return min(n, max(8, BUDGET // 6 // (blocks * slots) // 8 * 8))


# one frame each past the natural chunk, no switch set
PERM_NATURAL = (512, 1024, 0, 477, 8, 20)  # H, W (one channel), minD, candidates, sigma, trunc: chunks of 448 and 29
PERM_PLANES = (0, 447, 448, 476)           # the planes held to the restatement: the ends of both chunks
WMEDIAN_NATURAL = (14568, 48, 35, 0, 9)    # H, W, win, minD, candidates: 699 264 pixels, list chunks of 8 and 1 slices
WMEDIAN_BAND, WMEDIAN_MARGIN = 40, 18      # the oracle runs on the first and the last 40 rows; a crop agrees with the frame from
                                           # 18 rows off its cut on (17 of the 35x35 window, 1 of the 3x3 gradient)


def perm_natural_pair():
    H, W, minD, n, _, _ = PERM_NATURAL
    return _once("perm_pair", lambda: gray_noise_band_pair(H, W, n, 512, band=2))


def wmedian_natural_pair():
    H, W, win, minD, n = WMEDIAN_NATURAL
    return _once("wmedian_pair", lambda: band_pair(H, W, n, 35, band=4))


def expected_wmedian_bands(oracle):
    """((rows of the frame, map, volume) of the top band, the same of the bottom band): the oracle on the first and last
    WMEDIAN_BAND rows, cut back to the rows that the cut does not reach"""
    def run():
        H, W, win, minD, n = WMEDIAN_NATURAL
        L, R = wmedian_natural_pair()
        B, m = WMEDIAN_BAND, WMEDIAN_MARGIN
        out = []
        for rows, keep in ((slice(0, B), slice(0, B - m)), (slice(H - B, H), slice(m, B))):
            rc, d, v = oracle.asw_wmedian(L[rows], R[rows], 0, win, 10, 10, minD, n, want_vol=True)
            assert rc == 0
            ys = np.arange(H)[rows][keep]
            out.append((slice(int(ys[0]), int(ys[-1]) + 1), np.ascontiguousarray(d[keep]), np.ascontiguousarray(v[:, keep])))
        return tuple(out)
    return _once("wmedian_bands", run)


NOT_REACHED = {
    "launch_u8_scale past its cap": "16 777 216 bytes of a 3-channel image are 5 592 406 pixels, e.g. 2048 x 2731 > 2^21",
    "the weighted median's natural list chunk at 15x15": "chunk < n needs more than 2^31 / 6 / 16 list slots a slice: 2 796 203 pixels",
}


# ---------------------------------------------------------------- the references, computed once a session and never written to
_REFS = {}


def _once(key, fn):
    if key not in _REFS:
        val = fn()
        for a in (val if isinstance(val, tuple) else (val,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _REFS[key] = val
    return _REFS[key]


def similarity_inputs(case):
    H, W, minD, numD, _ = case
    return _once(("sim_pair", case), lambda: sim_pair(H, W, numD, H + W + numD))


def expected_similarity(oracle, case, win=None):
    """the oracle's volume of a similarity case, unpadded (win None) or padded"""
    def run():
        L, R = similarity_inputs(case)
        rc, vol = oracle.compute_similarity(L, R, *SIM_PARAMS, 0, case[2], case[3], win=win)
        assert rc == 0
        return vol
    return _once(("sim", case, win), run)


def split_inputs(case):
    H, W, win, minD, numD = case[:5]
    return _once(("split_pair", case[:5]), lambda: split_pair(H, W, numD, H + win + numD))


def expected_split(oracle, kernel, case, dt):
    """(map, volume) of oracle.asw_classic (gamma_c 30, gamma_g 20) / oracle.asw_geodesic at a split case, direction dt"""
    method = SPLIT_KERNELS[kernel][0]
    H, W, win, minD, numD = case[:5]

    def run():
        L, R = split_inputs(case)
        if method == "classic":
            rc, d, v = oracle.asw_classic(L, R, 30, 20, dt, win, minD, numD, want_vol=True)
        else:
            rc, d, v = oracle.asw_geodesic(L, R, dt, win, minD, numD, want_vol=True)
        assert rc == 0
        return d, v
    return _once((method, case[:5], dt), run)


def bm_inputs(case):
    H, W, minD, D, w = case
    return _once(("bm_pair", case), lambda: gray_noise_band_pair(H, W, dmax_for(W, D), H + W, band=7))


def expected_bm(case):
    import stereobm_ref
    H, W, minD, D, w = case
    cap, tex, U, sw, sr, M = BM_SETTINGS
    return _once(("bm", case), lambda: stereobm_ref.stereo_bm(*bm_inputs(case), minD, D, w, cap, tex, U, sw, sr, M))


def census_inputs(case):
    H, W, minD, D, w = case[:5]
    return _once(("census_pair", case[:5]), lambda: gray_band_pair(H, W, dmax_for(W, D), H + W, band=9))


def expected_census(case):
    import sgbm_census_ref
    H, W, minD, D, w = case[:5]
    P1, P2, m12, U, sw, sr = CENSUS_SETTINGS
    return _once(("census", case[:5]),
                 lambda: sgbm_census_ref.sgbm_census(*census_inputs(case), minD, D, w, P1, P2, m12, U, sw, sr, CENSUS_PATHS))


def varies(plane):
    """more than one value in the plane, NaN left out"""
    p = np.asarray(plane)
    return bool(np.nanmin(p) != np.nanmax(p))


def distinct(plane):
    """distinct finite-or-infinite values of a plane, NaN left out"""
    p = np.asarray(plane).ravel()
    return np.unique(p[~np.isnan(p)]) if p.dtype.kind == "f" else np.unique(p)
