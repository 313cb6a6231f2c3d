"""aswstereomatch_amd -- MI355X-native adaptive-support-weight stereo matching.

Host-side mirror (Python) of the reference's interface for the hot path
(aswStereoMatch/methods/aswMethods.h, "M.h"): same function names, argument order, defaults
and enum values; numpy arrays stand where cv::Mat stands (as in OpenCV's own Python binding).
Everything is computed by hand-written HIP kernels behind the C-ABI of include/asw_mi355x.h;
there is no CPU fallback -- a missing libasw_mi355x.so raises ImportError at first use.

Error behaviour follows the reference: where the reference returns silently or
hands back an empty cv::Mat (size mismatch, even window) the mirror returns None / an empty
list and records the status in ``last_status()``; anything else raises AswError.
"""
import ctypes as C
import enum
import os
import threading

import numpy as np

from . import _lib
from ._lib import AswError, AswImage, AswTiming

__all__ = [
    "DisparityType", "StereoMatchingAlgorithms", "DISPARITY_LEFT", "DISPARITY_RIGHT", "Context",
    "stereoMatching", "computeAD", "computeTAD", "computeSimilarity", "getCostSAD", "getCostSAD_d", "computeAdaptiveWeight",
    "computeAdaptiveWeight_geodesic", "getGeodesicDist", "getGuidedFilter", "computeAdaptiveWeight_GuidedF",
    "computeAdaptiveWeight_GuidedF_2", "computeAdaptiveWeight_WeightedMedian", "winnerTakeAll", "last_status",
    "stereoMatchingBatch", "computeAdaptiveWeight_BLO1", "computeAdaptiveWeight_direct8", "computeNCC", "computeNCC_costs",
    "computeAdaptiveWeight_GuidedF_3", "getDisparity_SGBM", "sgbm", "sgbm_paths", "sgbm_census", "filterSpeckles", "getDisparity_BM", "stereoBM",
    "PREFILTER_NORMALIZED_RESPONSE", "PREFILTER_XSOBEL", "refineDisparity", "stereoMatchingRefined",
    "REFINE_GAMMA_C", "REFINE_GAMMA_S", "SUBPIXEL_PARABOLA", "SUBPIXEL_EQUIANGULAR",
    "REFINE_SMOOTH", "SMOOTH_SIGMA_C", "SMOOTH_LAMBDA", "SMOOTH_ITERATIONS", "smoothDisparity", "stereoMatchingSmoothed",
    "SGBM_PATH_LR", "SGBM_PATH_RL", "SGBM_PATH_TB", "SGBM_PATH_BT", "SGBM_PATH_TLBR", "SGBM_PATH_TRBL", "SGBM_PATH_BRTL",
    "SGBM_PATH_BLTR", "SGBM_PATHS_3WAY", "SGBM_PATHS_HH4", "SGBM_PATHS_SGBM", "SGBM_PATHS_HH",
    "cross_algorithm", "computeAdaptiveWeight_cross",
    "adcensus_algorithm", "computeCensus", "computeADCensus", "computeAdaptiveWeight_adcensus",
    "twopass_algorithm", "computeAdaptiveWeight_twopass",
    "permeability_algorithm", "computeAdaptiveWeight_permeability",
    "CROSS_SCALE", "cross_scale",
    "SCANLINE", "scanline", "scanline_penalties",
    "AswError",
]


class DisparityType(enum.IntEnum):  # parametersStereo.h:4-8
    DISPARITY_LEFT = 0
    DISPARITY_RIGHT = 1


class StereoMatchingAlgorithms(enum.IntEnum):  # parametersStereo.h:10-24
    BM = 0
    SGBM = 1
    ADAPTIVE_WEIGHT = 2
    ADAPTIVE_WEIGHT_8DIRECT = 3
    ADAPTIVE_WEIGHT_GEODESIC = 4
    ADAPTIVE_WEIGHT_BILATERAL_GRID = 5
    ADAPTIVE_WEIGHT_BLO1 = 6
    ADAPTIVE_WEIGHT_GUIDED_FILTER = 7
    ADAPTIVE_WEIGHT_GUIDED_FILTER_2 = 8
    ADAPTIVE_WEIGHT_GUIDED_FILTER_3 = 9
    ADAPTIVE_WEIGHT_MEDIAN = 10
    NCC = 11
    ADAPTIVE_WEIGHT_CROSS = 12  # not in the reference: cross-based support regions


_A = StereoMatchingAlgorithms
DISPARITY_LEFT = DisparityType.DISPARITY_LEFT
DISPARITY_RIGHT = DisparityType.DISPARITY_RIGHT
# Sub-pixel disparity (asw_mi355x.h: ASW_DISPARITY_SUBPIXEL_*): OR one of them into a disparity type,
# e.g. DISPARITY_LEFT | SUBPIXEL_PARABOLA, or pass it as subpixel= where that keyword exists
SUBPIXEL_PARABOLA, SUBPIXEL_EQUIANGULAR = 0x100, 0x200

OK, ERR_SIZE_MISMATCH, ERR_EVEN_WINDOW, ERR_UNSUPPORTED_METHOD, ERR_UNSUPPORTED_LAYOUT = 0, 1, 2, 3, 4
ERR_HIP, ERR_ALLOC, ERR_BAD_ARGUMENT, ERR_NO_FRAME = 5, 6, 7, 8
MODE_SGBM_3WAY = 2  # StereoSGBM::MODE_SGBM_3WAY, the one mode asw_sgbm serves
# path directions of asw_sgbm_paths (asw_mi355x.h: ASW_SGBM_PATH_* / ASW_SGBM_PATHS_*)
(SGBM_PATH_LR, SGBM_PATH_RL, SGBM_PATH_TB, SGBM_PATH_BT, SGBM_PATH_TLBR, SGBM_PATH_TRBL, SGBM_PATH_BRTL,
 SGBM_PATH_BLTR) = (1 << _i for _i in range(8))
SGBM_PATHS_3WAY, SGBM_PATHS_HH4, SGBM_PATHS_SGBM, SGBM_PATHS_HH = 0x07, 0x0F, 0x37, 0xFF
_SGBM_MODE_PATHS = 0x40000000  # ASW_SGBM_MODE_PATHS: asw_sgbm's mode carrying a path mask, as the header's inline asw_sgbm_paths forms it
_SGBM_MODE_CENSUS = 0x10000  # ASW_SGBM_MODE_CENSUS: beside _SGBM_MODE_PATHS, the census cost of the header's inline asw_sgbm_census
_ALG_CROSS_PARAMS, _ALG_ADCENSUS_PARAMS, _ALG_TWOPASS_PARAMS, _ALG_PERMEABILITY_PARAMS = 1 << 30, 1 << 29, 1 << 28, 1 << 27  # ASW_ALG_*_PARAMS
_COST_CENSUS_PARAMS = 0x40000000  # ASW_COST_CENSUS_PARAMS: asw_cost_tad's threshold carrying the census cost builders, as the header's inline asw_cost_census / asw_cost_adcensus form it
CROSS_SCALE, SCANLINE = 1 << 12, 1 << 24  # ASW_DISPARITY_CROSS_SCALE, ASW_DISPARITY_SCANLINE
# The parameter fields of the selector's two packed words, `algorithmType` and `disparityType`, as asw_mi355x.h lays them out
# (csrc/asw_selector.h holds the decoders' side): name -> (shift, width, lowest, highest admissible value)
_FIELDS = {
    "tau": (8, 8, 0, 255), "trunc": (16, 8, 1, 255), "lambda_census": (16, 8, 1, 255), "lambda_ad": (24, 5, 1, 31),
    "gamma_c": (8, 8, 1, 255), "gamma_g": (16, 8, 1, 255), "sigma": (8, 8, 1, 255),
    "scales": (13, 3, 2, 5), "lambda_q": (16, 8, 1, 255),
    "p1_code": (1, 7, 1, 127), "unit_code": (25, 3, 0, 7), "p2_ratio - 1": (28, 3, 0, 7),
}


def _pack(base, values, spoil=None, spoil_bits=0):
    """base with every value in its field.  A value outside its field's range makes the word one the library refuses, the way
    asw_mi355x.h's encoder of the word does: spoil=None leaves 0 in that field; otherwise spoil_bits are set, the fields named in
    spoil hold 0 and the others their value cut to the field's width."""
    values = {name: int(v) for name, v in values.items()}
    bad = [name for name, v in values.items() if not _FIELDS[name][2] <= v <= _FIELDS[name][3]]
    zeroed = bad if spoil is None else spoil if bad else ()
    word = base | (spoil_bits if bad and spoil is not None else 0)
    for name, v in values.items():
        shift, width = _FIELDS[name][:2]
        word |= ((0 if name in zeroed else v) & ((1 << width) - 1)) << shift
    return word


def _unpack(word, *names):
    """the fields `names` of a packed word"""
    return tuple((int(word) >> _FIELDS[n][0]) & ((1 << _FIELDS[n][1]) - 1) for n in names)


def cross_algorithm(tau=20, trunc=20):
    """asw_alg_cross of asw_mi355x.h: the value of `algorithmType` that runs ADAPTIVE_WEIGHT_CROSS with colour threshold tau (0..255)
    and cost truncation trunc (1..255) in every call that takes an algorithm; an argument out of range gives a value the library
    refuses with ERR_BAD_ARGUMENT (bit 24)."""
    return _pack(_ALG_CROSS_PARAMS | int(_A.ADAPTIVE_WEIGHT_CROSS), {"tau": tau, "trunc": trunc}, spoil=(), spoil_bits=1 << 24)


def adcensus_algorithm(tau=20, lambda_ad=10, lambda_census=30):
    """asw_alg_adcensus of asw_mi355x.h: the value of `algorithmType` that runs AD-Census matching -- entry
    12's cross-based aggregation over the census + AD cost -- with colour threshold tau (0..255) and the table constants lambda_ad
    (1..31) and lambda_census (1..255) in every call that takes an algorithm; an argument out of range gives a value the library
    refuses with ERR_BAD_ARGUMENT (lambda_ad field 0)."""
    return _pack(_ALG_ADCENSUS_PARAMS | int(_A.ADAPTIVE_WEIGHT_CROSS), {"tau": tau, "lambda_ad": lambda_ad, "lambda_census": lambda_census},
                 spoil=("lambda_ad",))


def twopass_algorithm(gamma_c=30, gamma_g=20):
    """asw_alg_twopass of asw_mi355x.h: the value of `algorithmType` that runs ADAPTIVE_WEIGHT as the two-pass (separable)
    approximation with the integer gammas gamma_c and gamma_g (1..255 each) in every call that takes an
    algorithm; an argument out of range gives a value the library refuses with ERR_BAD_ARGUMENT (that gamma's field 0)."""
    return _pack(_ALG_TWOPASS_PARAMS | int(_A.ADAPTIVE_WEIGHT), {"gamma_c": gamma_c, "gamma_g": gamma_g})


def permeability_algorithm(sigma=8, trunc=20):
    """asw_alg_permeability of asw_mi355x.h: the value of `algorithmType` that runs ADAPTIVE_WEIGHT_CROSS as the recursive
    (permeability) aggregation over the whole image with the integers sigma and trunc (1..255 each) in every
    call that takes an algorithm; an argument out of range gives a value the library refuses with ERR_BAD_ARGUMENT (that field 0)."""
    return _pack(_ALG_PERMEABILITY_PARAMS | int(_A.ADAPTIVE_WEIGHT_CROSS), {"sigma": sigma, "trunc": trunc})


def cross_scale(scales=3, lambda_q=19):
    """asw_disparity_cross_scale of asw_mi355x.h: the value to OR into a disparity type (or to pass as cross_scale= where that keyword
    exists) that runs the method on `scales` (2..5) levels of a 2x2-mean pyramid and takes the winner of the regularised finest-scale
    volume, lambda = lambda_q / 64 with lambda_q in 1..255; an argument out of range gives a value the
    library refuses with ERR_BAD_ARGUMENT (scales field 0)."""
    return _pack(CROSS_SCALE, {"scales": scales, "lambda_q": lambda_q}, spoil=("scales",))


def scanline(p1_code=8, unit_code=5, p2_ratio=4):
    """asw_disparity_scanline of asw_mi355x.h: the value to OR into a disparity type (or to pass as scanline= where that keyword
    exists) that regularises the method's aggregated volume along four scan paths and takes the winner of the result (DESIGN.md
    section 4.19): P1 = p1_code * 4 ** (unit_code - 5), P2 = p2_ratio * P1, p1_code in 1..127, unit_code in 0..7, p2_ratio in 1..8;
    an argument out of range gives the flag alone, which the library refuses with ERR_BAD_ARGUMENT."""
    return _pack(SCANLINE, {"p1_code": p1_code, "unit_code": unit_code, "p2_ratio - 1": int(p2_ratio) - 1},
                 spoil=("p1_code", "unit_code", "p2_ratio - 1"))


def scanline_penalties(value):
    """(P1, P2) of a scanline() value, as the f32 numbers the library adds"""
    a, u, r1 = _unpack(value, "p1_code", "unit_code", "p2_ratio - 1")
    unit = 4.0 ** (u - 5)
    return np.float32(a * unit), np.float32((r1 + 1) * a * unit)


def _disparity_type(disparityType, subpixel, cross_scale, scanline):
    """disparityType with the keywords' values OR-ed in; cross_scale= together with scanline= is refused as the library refuses it"""
    if cross_scale and scanline:
        _state.status = ERR_BAD_ARGUMENT
        raise AswError(ERR_BAD_ARGUMENT, "cross_scale= with scanline=")
    return int(disparityType) | int(subpixel or 0) | int(cross_scale or 0) | int(scanline or 0)


PREFILTER_NORMALIZED_RESPONSE, PREFILTER_XSOBEL = 0, 1  # StereoBM::PREFILTER_*; asw_stereo_bm serves XSOBEL
REFINE_GAMMA_C, REFINE_GAMMA_S = 60.0, 9.0  # default colour / distance gammas of the refinement's weighted median (asw_mi355x.h)
# Smoothing (asw_mi355x.h: ASW_REFINE_SMOOTH): the flag that turns the refinement family's window argument into
# a smoothing request, and the wrappers' defaults (the paper's demonstration values: sigma about 0.03 * 255, lambda = 30^2, T = 3)
REFINE_SMOOTH = 0x40000000
SMOOTH_SIGMA_C, SMOOTH_LAMBDA, SMOOTH_ITERATIONS = 8.0, 900.0, 3


def _smooth_word(iterations):
    """REFINE_SMOOTH | T as the header's inline functions form it: iterations outside 1..8 travel as the word the library refuses"""
    return REFINE_SMOOTH | (int(iterations) if 1 <= int(iterations) <= 8 else 0)


# statuses for which the reference returns silently / an empty Mat
_SILENT = (ERR_SIZE_MISMATCH, ERR_EVEN_WINDOW)

_state = threading.local()


def last_status():
    """Status of the last call made from this thread (0 = ok)."""
    return getattr(_state, "status", 0)


def _image(arr, depth=0):
    """numpy array -> asw_image (keeps `arr` alive through the returned tuple)."""
    a = np.asarray(arr)
    want = {0: np.uint8, 3: np.int16, 5: np.float32}[depth]
    if a.dtype != want:
        raise TypeError("expected %s image, got %s" % (np.dtype(want).name, a.dtype))
    if a.ndim == 2:
        ch = 1
    elif a.ndim == 3:
        ch = a.shape[2]
    else:
        raise ValueError("image must be HxW or HxWxC")
    if a.strides[-1] != a.itemsize or (a.ndim == 3 and a.strides[1] != ch * a.itemsize):
        a = np.ascontiguousarray(a)
    img = AswImage(a.ctypes.data, a.shape[0], a.shape[1], ch, depth, a.strides[0])
    return img, a


class Context:
    """One device context (asw_create / asw_destroy).  Not shared between threads."""

    def __init__(self, device_id=0, env=None):
        """env: measurement / test switches (ASW_BILATERAL_XQ, ASW_BAND_Q, ...) for THIS context: the library reads its
        switches once, inside asw_create, so they are set only around that call."""
        self._h = C.c_void_p()
        self._lib = _lib.lib()
        saved = {k: os.environ.get(k) for k in (env or {})}
        try:
            for k, v in (env or {}).items():
                os.environ[k] = str(v)
            rc = self._lib.asw_create(int(device_id), C.byref(self._h))
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        if rc != 0:
            raise AswError(rc, "asw_create(device %d)" % device_id)
        self.device_id = device_id

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.asw_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_gray_bits(self, bits):
        """cvtColor(BGR2GRAY) constant set: 14 (OpenCV 4.1.0, default) or 15 (later 4.x) -- asw_set_gray_bits."""
        rc = self._lib.asw_set_gray_bits(self._h, int(bits))
        if rc != 0:
            raise AswError(rc, "asw_set_gray_bits")

    # ---- helpers ----
    def _finish(self, rc, where):
        _state.status = rc
        if rc == 0:
            return True
        if rc in _SILENT:
            return False
        raise AswError(rc, where)

    @staticmethod
    def _candidates(algorithm, numDisparity):
        n = _lib.lib().asw_volume_planes(int(algorithm), int(numDisparity))  # the library knows which ranges are inclusive
        return n if n > 0 else int(numDisparity)

    # ---- whole-method entry point (M.h:91-92) ----
    def stereoMatching(self, srcLeft, srcRight, disparityType, algorithmType, winSize=15, minDisparity=0,
                       numDisparity=64, return_cost_volume=False, subpixel=None, cross_scale=None, scanline=None,
                       return_confidence=False):
        """subpixel: None, SUBPIXEL_PARABOLA or SUBPIXEL_EQUIANGULAR; cross_scale: None or a cross_scale() value; scanline: None or
        a scanline() value (not together with cross_scale); all are OR-ed into disparityType.  return_confidence: also the
        per-pixel confidence in [0, 1] of the volume the call returns (asw_mi355x.h), last in the tuple:
        (disp, conf) or (disp, vol, conf)."""
        disparityType = _disparity_type(disparityType, subpixel, cross_scale, scanline)

        def call(h, l, r, d, *args):
            return self._lib.asw_stereo_match(h, l, r, d, disparityType, int(algorithmType), winSize, minDisparity, numDisparity, *args)
        return self._aggregate("asw_stereo_match", int(algorithmType), numDisparity, srcLeft, srcRight, (), return_cost_volume, fn=call,
                               return_confidence=return_confidence)

    def _aggregate(self, name, algorithm, numDisparity, leftImg, rightImg, args, return_cost_volume, fn=None, return_confidence=False):
        """One per-method entry point `name` (or the call `fn` standing for it); the library says how many planes the volume of
        `algorithm` has (asw_volume_planes).  return_confidence: the call gets a 2-channel map, disparity and confidence
        interleaved, and the two come back as separate arrays, the confidence last."""
        fn = fn or getattr(self._lib, name)
        li, la = _image(leftImg)
        ri, ra = _image(rightImg)
        disp = np.zeros((la.shape[0], la.shape[1]) + ((2,) if return_confidence else ()), np.float32)
        di, _ = _image(disp, 5)
        vol, pv = None, None
        if return_cost_volume:
            vol = np.zeros((self._candidates(algorithm, numDisparity), la.shape[0], la.shape[1]), np.float32)
            pv = vol.ctypes.data_as(C.c_void_p)
        rc = fn(self._h, C.byref(li), C.byref(ri), C.byref(di), *args, pv, 0 if vol is None else vol.size)
        ok = self._finish(rc, name)
        out = ((disp[..., 0].copy(), disp[..., 1].copy()) if return_confidence else (disp,)) if ok else (None,) * (1 + bool(return_confidence))
        out = out[:1] + ((vol if ok else None,) if return_cost_volume else ()) + out[1:]
        return out if len(out) > 1 else out[0]

    # ---- per-method entry points (M.h:133-182) ----
    def computeAdaptiveWeight(self, leftImg, rightImg, gamma_c=30, gamma_g=2, dispType=DISPARITY_LEFT, winSize=7,
                              minDisparity=186, numDisparity=144, return_cost_volume=False, return_confidence=False):
        return self._aggregate("asw_aggregate_bilateral", _A.ADAPTIVE_WEIGHT, numDisparity, leftImg, rightImg,
                               (float(gamma_c), float(gamma_g), int(dispType), winSize, minDisparity, numDisparity),
                               return_cost_volume, return_confidence=return_confidence)

    def computeAdaptiveWeight_direct8(self, leftImg, rightImg, dispType=DISPARITY_LEFT, winSize=7, minDisparity=186,
                                      numDisparity=144, return_cost_volume=False, return_confidence=False):
        """M.h:135-136, M.cpp:1167-1319 (DISPARITY_LEFT only: the reference's RIGHT branch is undefined behaviour)."""
        return self._aggregate("asw_aggregate_direct8", _A.ADAPTIVE_WEIGHT_8DIRECT, numDisparity, leftImg, rightImg,
                               (int(dispType), winSize, minDisparity, numDisparity), return_cost_volume, return_confidence=return_confidence)

    def computeAdaptiveWeight_geodesic(self, leftImg, rightImg, dispType=DISPARITY_LEFT, winSize=7, minDisparity=186,
                                       numDisparity=144, return_cost_volume=False, return_confidence=False):
        return self._aggregate("asw_aggregate_geodesic", _A.ADAPTIVE_WEIGHT_GEODESIC, numDisparity, leftImg, rightImg,
                               (int(dispType), winSize, minDisparity, numDisparity), return_cost_volume, return_confidence=return_confidence)

    def computeAdaptiveWeight_GuidedF(self, leftImg, rightImg, dispType=DISPARITY_LEFT, eps=1e-8, winSize=35,
                                      minDisparity=186, numDisparity=144, return_cost_volume=False, return_confidence=False):
        return self._aggregate("asw_aggregate_guided", _A.ADAPTIVE_WEIGHT_GUIDED_FILTER, numDisparity, leftImg, rightImg,
                               (int(dispType), float(eps), winSize, minDisparity, numDisparity), return_cost_volume, return_confidence=return_confidence)

    def computeAdaptiveWeight_GuidedF_2(self, leftImg, rightImg, dispType=DISPARITY_LEFT, eps=1e-8, winSize=35,
                                        minDisparity=186, numDisparity=144, return_cost_volume=False, return_confidence=False):
        return self._aggregate("asw_aggregate_guided2", _A.ADAPTIVE_WEIGHT_GUIDED_FILTER_2, numDisparity, leftImg, rightImg,
                               (int(dispType), float(eps), winSize, minDisparity, numDisparity), return_cost_volume, return_confidence=return_confidence)

    def computeAdaptiveWeight_GuidedF_3(self, leftImg, rightImg, dispType=DISPARITY_LEFT, eps=1e-6, winSize=35,
                                        minDisparity=186, numDisparity=144, return_cost_volume=False, return_confidence=False):
        """M.h:174-176, M.cpp:3063-3137: NCC costs + guided filter."""
        return self._aggregate("asw_aggregate_guided3", _A.ADAPTIVE_WEIGHT_GUIDED_FILTER_3, numDisparity, leftImg, rightImg,
                               (int(dispType), float(eps), winSize, minDisparity, numDisparity), return_cost_volume, return_confidence=return_confidence)

    def computeNCC(self, leftImg, rightImg, dispType=DISPARITY_LEFT, winSize=7, minDisparity=0, numDisparity=30):
        """computeNCC -> disparity (M.h:122-123, M.cpp:812-913)."""
        li, la = _image(leftImg)
        ri, ra = _image(rightImg)
        disp = np.zeros((la.shape[0], la.shape[1]), np.float32)
        di, _ = _image(disp, 5)
        rc = self._lib.asw_ncc_disparity(self._h, C.byref(li), C.byref(ri), C.byref(di), int(dispType), winSize, minDisparity,
                                         numDisparity)
        return disp if self._finish(rc, "asw_ncc_disparity") else None

    def computeNCC_costs(self, leftImg, rightImg, dispType=DISPARITY_LEFT, winSize=7, minDisparity=0, numDisparity=30,
                         normalized=True):
        """computeNCC -> cost_ds (M.h:124-126, M.cpp:924-1013); normalized=False returns the planes before normalize()."""
        a = np.asarray(leftImg)
        return self._cost(self._lib.asw_cost_ncc, "asw_cost_ncc", leftImg, rightImg, np.float32, a.shape[:2], numDisparity,
                          (int(dispType), winSize, minDisparity, numDisparity, int(bool(normalized))))

    def computeAdaptiveWeight_BLO1(self, leftImg, rightImg, dispType=DISPARITY_LEFT, sampleRateR=10, winSize=35,
                                   minDisparity=186, numDisparity=144, return_cost_volume=False, return_confidence=False):
        return self._aggregate("asw_aggregate_blo1", _A.ADAPTIVE_WEIGHT_BLO1, numDisparity, leftImg, rightImg,
                               (int(dispType), float(sampleRateR), winSize, minDisparity, numDisparity), return_cost_volume, return_confidence=return_confidence)

    def computeAdaptiveWeight_bilateralGrid(self, leftImg, rightImg, dispType=DISPARITY_LEFT, sampleRateS=10, sampleRateR=10,
                                            minDisparity=186, numDisparity=144, return_cost_volume=False, return_confidence=False):
        """M.h:155-157, M.cpp:2253-2430 (DISPARITY_LEFT only: the reference's RIGHT branch reads past the image row)."""
        return self._aggregate("asw_aggregate_bilgrid", _A.ADAPTIVE_WEIGHT_BILATERAL_GRID, numDisparity, leftImg, rightImg,
                               (int(dispType), float(sampleRateS), float(sampleRateR), minDisparity, numDisparity),
                               return_cost_volume, return_confidence=return_confidence)

    def computeAdaptiveWeight_WeightedMedian(self, leftImg, rightImg, dispType=DISPARITY_LEFT, winSize=35,
                                             sampleRateS=10, sampleRateR=10, minDisparity=186, numDisparity=144,
                                             return_cost_volume=False, return_confidence=False):
        return self._aggregate("asw_aggregate_wmedian", _A.ADAPTIVE_WEIGHT_MEDIAN, numDisparity, leftImg, rightImg,
                               (int(dispType), winSize, float(sampleRateS), float(sampleRateR), minDisparity, numDisparity),
                               return_cost_volume, return_confidence=return_confidence)

    def computeAdaptiveWeight_cross(self, leftImg, rightImg, dispType=DISPARITY_LEFT, tau=20, trunc=20, winSize=15, minDisparity=0,
                                    numDisparity=64, return_cost_volume=False, return_confidence=False):
        """Cross-based support-region aggregation (asw_aggregate_cross; not in the reference): the truncated
        AD cost summed over every pixel's cross-shaped region, exact integers and one f32 division; 1- or 3-channel pairs."""
        def call(h, l, r, d, *args):
            return self._lib.asw_stereo_match(h, l, r, d, int(dispType), cross_algorithm(tau, trunc), winSize, minDisparity,
                                              numDisparity, *args)
        return self._aggregate("asw_aggregate_cross", _A.ADAPTIVE_WEIGHT_CROSS, numDisparity, leftImg, rightImg, (), return_cost_volume,
                               fn=call, return_confidence=return_confidence)

    def computeAdaptiveWeight_adcensus(self, leftImg, rightImg, dispType=DISPARITY_LEFT, tau=20, lambda_ad=10, lambda_census=30,
                                       winSize=15, minDisparity=0, numDisparity=64, return_cost_volume=False, return_confidence=False):
        """AD-Census matching (asw_aggregate_adcensus; not in the reference): the census + AD cost of
        computeADCensus summed over every pixel's cross-shaped region, exact integers and one f32 division; 1- or 3-channel pairs."""
        alg = adcensus_algorithm(tau, lambda_ad, lambda_census)

        def call(h, l, r, d, *args):
            return self._lib.asw_stereo_match(h, l, r, d, int(dispType), alg, winSize, minDisparity, numDisparity, *args)
        return self._aggregate("asw_aggregate_adcensus", _A.ADAPTIVE_WEIGHT_CROSS, numDisparity, leftImg, rightImg, (),
                               return_cost_volume, fn=call, return_confidence=return_confidence)

    def computeAdaptiveWeight_twopass(self, leftImg, rightImg, gamma_c=30, gamma_g=20, dispType=DISPARITY_LEFT, winSize=15,
                                      minDisparity=0, numDisparity=64, return_cost_volume=False, return_confidence=False):
        """Two-pass (separable) adaptive-support-weight aggregation (asw_aggregate_twopass; not in the
        reference): a vertical, then a horizontal 1-D weighted pass, 2 * winSize taps in place of winSize^2 - 1; integer gammas
        1..255; candidates minDisparity .. minDisparity + numDisparity inclusive; 1- or 3-channel pairs."""
        alg = twopass_algorithm(gamma_c, gamma_g)

        def call(h, l, r, d, *args):
            return self._lib.asw_stereo_match(h, l, r, d, int(dispType), alg, winSize, minDisparity, numDisparity, *args)
        return self._aggregate("asw_aggregate_twopass", _A.ADAPTIVE_WEIGHT, numDisparity, leftImg, rightImg, (), return_cost_volume,
                               fn=call, return_confidence=return_confidence)

    def computeAdaptiveWeight_permeability(self, leftImg, rightImg, dispType=DISPARITY_LEFT, sigma=8, trunc=20, minDisparity=0,
                                           numDisparity=64, return_cost_volume=False, return_confidence=False):
        """Recursive (permeability) aggregation over the whole image (asw_aggregate_permeability; not in the
        reference): the truncated AD cost carried along rows and columns, damped by exp(-colour step / sigma), f64; no window;
        integers sigma and trunc 1..255; 1- or 3-channel pairs."""
        alg = permeability_algorithm(sigma, trunc)

        def call(h, l, r, d, *args):
            return self._lib.asw_stereo_match(h, l, r, d, int(dispType), alg, 0, minDisparity, numDisparity, *args)
        return self._aggregate("asw_aggregate_permeability", _A.ADAPTIVE_WEIGHT_CROSS, numDisparity, leftImg, rightImg, (),
                               return_cost_volume, fn=call, return_confidence=return_confidence)

    # ---- semi-global block matching ----
    def getDisparity_SGBM(self, srcLeft, srcRight, winSize=15, minDisparity=0, numDisparity=64):
        """getDisparity_SGBM (M.h:94, aswMethods.cpp:158-194): StereoSGBM with the reference's settings -> uint8 map
        (convertTo(CV_8U, 1/16)).  Where the reference raises CV_Error (numDisparity % 16 != 0, even winSize) AswError is raised
        with status ERR_UNSUPPORTED_METHOD."""
        d = self.stereoMatching(srcLeft, srcRight, DISPARITY_LEFT, StereoMatchingAlgorithms.SGBM, winSize, minDisparity,
                                numDisparity)
        return None if d is None else d.astype(np.uint8)

    def sgbm(self, left, right, minDisparity, numDisparities, blockSize, P1=0, P2=0, disp12MaxDiff=0, preFilterCap=0,
             uniquenessRatio=0, speckleWindowSize=0, speckleRange=0, mode=MODE_SGBM_3WAY, return_cost_volume=False):
        """StereoSGBM::create(...) + compute(): int16 disparity x 16 (invalid: 16 * (minDisparity - 1)); with return_cost_volume
        also the aggregated cost S, float32 [numDisparities][H][W] (asw_sgbm)."""
        return self._sgbm_call("asw_sgbm", left, right, minDisparity, numDisparities, blockSize, P1, P2, disp12MaxDiff, preFilterCap,
                               uniquenessRatio, speckleWindowSize, speckleRange, int(mode), return_cost_volume)

    def sgbm_paths(self, left, right, minDisparity, numDisparities, blockSize, P1=0, P2=0, disp12MaxDiff=0, preFilterCap=0,
                   uniquenessRatio=0, speckleWindowSize=0, speckleRange=0, paths=SGBM_PATHS_HH, return_cost_volume=False):
        """sgbm with the aggregated cost summed over the path directions of `paths` (an OR of SGBM_PATH_*, a superset of
        SGBM_PATHS_3WAY) instead of the three of MODE_SGBM_3WAY; SGBM_PATHS_3WAY gives sgbm's result
        (asw_sgbm_paths of asw_mi355x.h: asw_sgbm with the mask packed into its mode)."""
        mask = 0x100 if int(paths) & ~SGBM_PATHS_HH else int(paths)  # an invalid mask travels as the invalid mask 0x100
        return self._sgbm_call("asw_sgbm_paths", left, right, minDisparity, numDisparities, blockSize, P1, P2, disp12MaxDiff,
                               preFilterCap, uniquenessRatio, speckleWindowSize, speckleRange, _SGBM_MODE_PATHS | mask,
                               return_cost_volume)

    def sgbm_census(self, left, right, minDisparity, numDisparities, blockSize, P1=0, P2=0, disp12MaxDiff=0, uniquenessRatio=0,
                    speckleWindowSize=0, speckleRange=0, paths=SGBM_PATHS_HH, return_cost_volume=False):
        """sgbm_paths with a census cost in place of the prefilter and the Birchfield-Tomasi cost: the
        block sum of the Hamming distance of the 62-bit census codes of the gray pair, unchanged by a gain or offset between the
        two cameras.  No preFilterCap; numpy columns <= 10240 (asw_sgbm_census of asw_mi355x.h: asw_sgbm with the request packed
        into its mode)."""
        mask = 0x100 if int(paths) & ~SGBM_PATHS_HH else int(paths)  # an invalid mask travels as the invalid mask 0x100
        return self._sgbm_call("asw_sgbm_census", left, right, minDisparity, numDisparities, blockSize, P1, P2, disp12MaxDiff, 0,
                               uniquenessRatio, speckleWindowSize, speckleRange, _SGBM_MODE_PATHS | _SGBM_MODE_CENSUS | mask,
                               return_cost_volume)

    def _sgbm_call(self, where, left, right, minDisparity, numDisparities, blockSize, P1, P2, disp12MaxDiff, preFilterCap,
                   uniquenessRatio, speckleWindowSize, speckleRange, mode, return_cost_volume):
        li, la = _image(left)
        ri, ra = _image(right)
        disp = np.zeros(la.shape[:2], np.int16)
        di, _ = _image(disp, 3)
        vol, pv = None, None
        if return_cost_volume:
            vol = np.zeros((numDisparities,) + la.shape[:2], np.float32)
            pv = vol.ctypes.data_as(C.c_void_p)
        rc = self._lib.asw_sgbm(self._h, C.byref(li), C.byref(ri), C.byref(di), minDisparity, numDisparities, blockSize, P1, P2,
                                disp12MaxDiff, preFilterCap, uniquenessRatio, speckleWindowSize, speckleRange, mode, pv,
                                0 if vol is None else vol.size)
        self._strict(rc, where)
        return (disp, vol) if return_cost_volume else disp

    # ---- block matching ----
    def getDisparity_BM(self, srcLeft, srcRight, winSize=15, minDisparity=0, numDisparity=64):
        """getDisparity_BM (M.h:93, aswMethods.cpp:100-146): StereoBM with the reference's settings -> uint8 map
        (convertTo(CV_8U, 1/16)); 3-channel input is converted to gray first.  Where the reference raises CV_Error
        (numDisparity % 16 != 0, even winSize, an empty image, a block size outside 5..min(H, W, 255)) AswError is raised with
        status ERR_UNSUPPORTED_METHOD."""
        li, la = _image(srcLeft)
        ri, ra = _image(srcRight)
        out = np.zeros(la.shape[:2], np.uint8)
        oi, _ = _image(out)
        rc = self._lib.asw_get_disparity_bm(self._h, C.byref(li), C.byref(ri), C.byref(oi), winSize, minDisparity, numDisparity)
        self._strict(rc, "asw_get_disparity_bm")
        return out

    def stereoBM(self, left, right, minDisparity, numDisparities, blockSize, preFilterType=PREFILTER_XSOBEL, preFilterSize=9,
                 preFilterCap=31, textureThreshold=10, uniquenessRatio=15, speckleWindowSize=0, speckleRange=0, disp12MaxDiff=-1,
                 return_cost_volume=False):
        """StereoBM::create + setters + compute() on 8-bit gray images: int16 disparity x 16 (FILTERED: 16 * (minDisparity - 1));
        with return_cost_volume also the block SAD, float32 [numDisparities][H][W] (plane k <-> disparity minDisparity + k, NaN
        where nothing is computed) (asw_stereo_bm)."""
        li, la = _image(left)
        ri, ra = _image(right)
        disp = np.zeros(la.shape[:2], np.int16)
        di, _ = _image(disp, 3)
        vol, pv = None, None
        if return_cost_volume:
            vol = np.zeros((numDisparities,) + la.shape[:2], np.float32)
            pv = vol.ctypes.data_as(C.c_void_p)
        rc = self._lib.asw_stereo_bm(self._h, C.byref(li), C.byref(ri), C.byref(di), minDisparity, numDisparities, blockSize,
                                     int(preFilterType), preFilterSize, preFilterCap, textureThreshold, uniquenessRatio,
                                     speckleWindowSize, speckleRange, disp12MaxDiff, pv, 0 if vol is None else vol.size)
        self._strict(rc, "asw_stereo_bm")
        return (disp, vol) if return_cost_volume else disp

    def filterSpeckles(self, img, newVal, maxSpeckleSize, maxDiff):
        """cv::filterSpeckles on an int16 map (asw_filter_speckles): the filtered copy."""
        a = np.array(img, copy=True)
        if a.dtype != np.int16 or a.ndim != 2:
            raise TypeError("filterSpeckles: a 2-D int16 map expected (CV_16SC1), got %s %s" % (a.dtype, a.shape))
        ii, a = _image(a, 3)
        self._strict(self._lib.asw_filter_speckles(self._h, C.byref(ii), int(newVal), int(maxSpeckleSize), int(maxDiff)),
                     "asw_filter_speckles")
        return a

    # ---- cost builders (M.h:101-113): return a list of planes like std::vector<cv::Mat> ----
    def _cost(self, fn, name, leftImg, rightImg, dtype, plane_shape, numDisparity, args):
        li, la = _image(leftImg)
        ri, ra = _image(rightImg)
        out = np.zeros((numDisparity,) + plane_shape, dtype)
        rc = fn(self._h, C.byref(li), C.byref(ri), out.ctypes.data_as(C.c_void_p), *args)
        if not self._finish(rc, name):
            return []  # cost_ds left empty / untouched by the reference
        return list(out)

    def computeAD(self, leftImg, rightImg, dispType=DISPARITY_LEFT, minDisparity=0, numDisparity=30):
        a = np.asarray(leftImg)
        return self._cost(self._lib.asw_cost_ad, "asw_cost_ad", leftImg, rightImg, np.uint8, a.shape[:2], numDisparity,
                          (int(dispType), minDisparity, numDisparity))

    def computeCensus(self, leftImg, rightImg, dispType=DISPARITY_LEFT, minDisparity=0, numDisparity=30):
        """asw_cost_census: the Hamming distance (0..62) of the 9 x 7 census codes of the gray pair, uint8 planes like computeAD's."""
        a = np.asarray(leftImg)
        return self._cost(self._lib.asw_cost_tad, "asw_cost_census", leftImg, rightImg, np.uint8, a.shape[:2], numDisparity,
                          (int(dispType), _COST_CENSUS_PARAMS, minDisparity, numDisparity))

    def computeADCensus(self, leftImg, rightImg, dispType=DISPARITY_LEFT, lambda_ad=10, lambda_census=30, minDisparity=0,
                        numDisparity=30):
        """asw_cost_adcensus: TA[AD] + TC[Hamming] (0..254), the raw cost of AD-Census matching; both lambdas in 1..255."""
        a = np.asarray(leftImg)
        la, lc = int(lambda_ad), int(lambda_census)
        bad = 0x10000 if (la < 1 or la > 255 or lc < 1 or lc > 255) else 0
        return self._cost(self._lib.asw_cost_tad, "asw_cost_adcensus", leftImg, rightImg, np.uint8, a.shape[:2], numDisparity,
                          (int(dispType), _COST_CENSUS_PARAMS | bad | ((la & 0xFF) << 8) | (lc & 0xFF), minDisparity, numDisparity))

    def computeTAD(self, leftImg, rightImg, dispType=DISPARITY_LEFT, threshold_T=30, minDisparity=0, numDisparity=30):
        a = np.asarray(leftImg)
        return self._cost(self._lib.asw_cost_tad, "asw_cost_tad", leftImg, rightImg, np.uint8, a.shape[:2], numDisparity,
                          (int(dispType), threshold_T, minDisparity, numDisparity))

    def computeSD(self, leftImg, rightImg, dispType=DISPARITY_LEFT, minDisparity=0, numDisparity=30):
        """Squared differences (M.cpp:670-759): the AD plane multiplied by itself in u8, saturating at 255."""
        a = np.asarray(leftImg)
        return self._cost(self._lib.asw_cost_sd, "asw_cost_sd", leftImg, rightImg, np.uint8, a.shape[:2], numDisparity,
                          (int(dispType), minDisparity, numDisparity))

    def computeSimilarity(self, leftImg, rightImg, regularity, thresC, thresG, dispType, minDisparity, numDisparity,
                          winSize=None):
        """Both overloads of computeSimilarity (M.cpp:415, 651); winSize selects the padded one."""
        a = np.asarray(leftImg)
        h = 0 if winSize is None else winSize // 2
        shape = (a.shape[0] + 2 * h, a.shape[1] + 2 * h)
        return self._cost(self._lib.asw_cost_similarity, "asw_cost_similarity", leftImg, rightImg, np.float32, shape,
                          numDisparity, (float(regularity), float(thresC), float(thresG), int(dispType),
                                         0 if winSize is None else winSize, minDisparity, numDisparity))

    def getCostSAD(self, leftImg, rightImg, dispType=DISPARITY_LEFT, winSize=35, minDisparity=0, numDisparity=30):
        """getCostSAD_d (M.cpp:2442) for every disparity, as M.cpp:2884-2889 calls it."""
        a = np.asarray(leftImg)
        return self._cost(self._lib.asw_cost_sad, "asw_cost_sad", leftImg, rightImg, np.float32, a.shape[:2], numDisparity,
                          (int(dispType), winSize, minDisparity, numDisparity))

    def getCostSAD_d(self, leftImg, rightImg, disparity, dispType=DISPARITY_LEFT, winSize=35):
        """getCostSAD_d as declared (M.h:156, M.cpp:2442-2503): one disparity, the non-reference view already bordered by
        the caller (M.cpp:2877-2878).  None where the reference returns Mat()."""
        li, la = _image(leftImg)
        ri, ra = _image(rightImg)
        ref = la if int(dispType) == 0 else ra
        out = np.zeros(ref.shape[:2], np.float32)
        rc = self._lib.asw_cost_sad_d(self._h, C.byref(li), C.byref(ri), out.ctypes.data_as(C.c_void_p), int(disparity),
                                      int(dispType), winSize)
        return out if self._finish(rc, "asw_cost_sad_d") else None

    # ---- public building blocks ----
    def getGuidedFilter(self, guidedImg, inputP, r, eps):
        gi, ga = _image(guidedImg)
        p = np.ascontiguousarray(inputP, dtype=np.float32)
        if p.shape != ga.shape[:2]:
            _state.status = ERR_SIZE_MISMATCH
            return None  # M.cpp:2768-2769
        q = np.zeros_like(p)
        rc = self._lib.asw_guided_filter(self._h, C.byref(gi), p.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p),
                                         r, float(eps))
        return q if self._finish(rc, "asw_guided_filter") else None

    def getGeodesicDist(self, originImg, winSize=15, iterTime=3):
        ii, ia = _image(originImg)
        out = np.zeros((ia.shape[0], ia.shape[1], winSize, winSize), np.float32)
        rc = self._lib.asw_geodesic_dist(self._h, C.byref(ii), out.ctypes.data_as(C.c_void_p), winSize, iterTime)
        return out if self._finish(rc, "asw_geodesic_dist") else None

    def winnerTakeAll(self, costVolume, minDisparity=0):
        v = np.ascontiguousarray(costVolume, dtype=np.float32)
        disp = np.zeros(v.shape[1:], np.float32)
        rc = self._lib.asw_wta(self._h, v.ctypes.data_as(C.c_void_p), v.shape[0], v.shape[1], v.shape[2], minDisparity,
                               disp.ctypes.data_as(C.c_void_p))
        self._finish(rc, "asw_wta")
        return disp

    def leftRightCheck(self, dispLeft, dispRight, maxDiff=1.0, invalid=-1.0):
        """asw_lr_check: (checked left disparity, number of rejected pixels)."""
        a = np.ascontiguousarray(dispLeft, dtype=np.float32)
        b = np.ascontiguousarray(dispRight, dtype=np.float32)
        if a.ndim != 2 or a.shape != b.shape:
            raise ValueError("leftRightCheck: two float32 maps of equal (H, W) shape expected")
        out = np.zeros(a.shape, np.float32)
        n = C.c_int(0)
        rc = self._lib.asw_lr_check(self._h, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), a.shape[0], a.shape[1],
                                    float(maxDiff), float(invalid), out.ctypes.data_as(C.c_void_p), C.byref(n))
        self._finish(rc, "asw_lr_check")
        return out, n.value

    def refineDisparity(self, guide, dispLeft, dispRight, minDisparity, numValues, maxDiff=1.0, winSize=15,
                        gamma_c=REFINE_GAMMA_C, gamma_s=REFINE_GAMMA_S, return_mask=False):
        """asw_refine_disparity: cross-check, scan-line fill of the rejected pixels, weighted median over the filled ones ->
        (refined map, rejected pixels, unfillable pixels[, mask: 0 valid / 1 filled / 2 unfillable]).  numValues: number of
        admissible disparities from minDisparity on (asw_volume_planes(algorithm, numDisparity) for a selector method)."""
        gi, ga = _image(guide)
        a = np.ascontiguousarray(dispLeft, dtype=np.float32)
        b = np.ascontiguousarray(dispRight, dtype=np.float32)
        if a.ndim != 2 or a.shape != b.shape or a.shape != ga.shape[:2]:
            raise ValueError("refineDisparity: a guide and two float32 maps of equal (H, W) shape expected")
        out = np.zeros(a.shape, np.float32)
        mask = np.zeros(a.shape, np.uint8) if return_mask else None
        nr, nu = C.c_int(0), C.c_int(0)
        rc = self._lib.asw_refine_disparity(self._h, C.byref(gi), a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p),
                                            int(minDisparity), int(numValues), float(maxDiff), int(winSize), float(gamma_c),
                                            float(gamma_s), out.ctypes.data_as(C.c_void_p),
                                            mask.ctypes.data_as(C.c_void_p) if return_mask else None, C.byref(nr), C.byref(nu))
        self._strict(rc, "asw_refine_disparity")
        return (out, nr.value, nu.value, mask) if return_mask else (out, nr.value, nu.value)

    def stereoMatchingRefined(self, srcLeft, srcRight, algorithmType, winSize=15, minDisparity=0, numDisparity=64, maxDiff=1.0,
                              refineWin=15, gamma_c=REFINE_GAMMA_C, gamma_s=REFINE_GAMMA_S):
        """asw_stereo_match_refined: both directions of the method + refineDisparity with srcLeft as guide ->
        (refined left-view map, rejected pixels, unfillable pixels).  Not a reference function, so there is no silent return to
        mimic: like the resident calls, every non-zero status raises AswError (size mismatch and even window included)."""
        li, la = _image(srcLeft)
        ri, ra = _image(srcRight)
        disp = np.zeros(la.shape[:2], np.float32)
        di, _ = _image(disp, 5)
        nr, nu = C.c_int(0), C.c_int(0)
        rc = self._lib.asw_stereo_match_refined(self._h, C.byref(li), C.byref(ri), C.byref(di), int(algorithmType), winSize,
                                                minDisparity, numDisparity, float(maxDiff), int(refineWin), float(gamma_c),
                                                float(gamma_s), C.byref(nr), C.byref(nu))
        self._strict(rc, "asw_stereo_match_refined")
        return disp, nr.value, nu.value

    # ---- confidence-weighted edge-aware smoothing (asw_mi355x.h "Smoothing").  The three calls are the
    # header's inline functions: the request travels in the refinement family's window argument as REFINE_SMOOTH | iterations ----
    def smoothDisparity(self, guide, disp, conf, sigma_c=SMOOTH_SIGMA_C, lam=SMOOTH_LAMBDA, iterations=SMOOTH_ITERATIONS):
        """asw_smooth_disparity: the fast global smoother over disp * conf and conf, guided by the 8-bit image `guide` (1 or 3
        channels) -> the dense fractional map.  conf: any float32 trust value per pixel, e.g. the confidence a return_confidence=True
        call gives, or a 0/1 validity mask; non-finite map values and confidences <= 0 are holes.  The defaults are the paper's
        demonstration values (lambda = 30^2, sigma about 0.03 * 255, 3 iterations): a starting point, not a tuned choice."""
        gi, ga = _image(guide)
        a = np.ascontiguousarray(disp, dtype=np.float32)
        b = np.ascontiguousarray(conf, dtype=np.float32)
        if a.ndim != 2 or a.shape != b.shape or a.shape != ga.shape[:2]:
            raise ValueError("smoothDisparity: a guide, a float32 map and a float32 confidence of equal (H, W) shape expected")
        out = np.zeros(a.shape, np.float32)
        rc = self._lib.asw_refine_disparity(self._h, C.byref(gi), a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), 0, 1, 0.0,
                                            _smooth_word(iterations), float(sigma_c), float(lam), out.ctypes.data_as(C.c_void_p),
                                            None, None, None)
        self._strict(rc, "asw_smooth_disparity")
        return out

    def stereoMatchingSmoothed(self, srcLeft, srcRight, algorithmType, winSize=15, minDisparity=0, numDisparity=64,
                               sigma_c=SMOOTH_SIGMA_C, lam=SMOOTH_LAMBDA, iterations=SMOOTH_ITERATIONS):
        """asw_stereo_match_smoothed: ONE DISPARITY_LEFT match of the method with its confidence + smoothDisparity with srcLeft
        as guide -> the smoothed left-view map.  Every non-zero status raises AswError, as for stereoMatchingRefined."""
        li, la = _image(srcLeft)
        ri, ra = _image(srcRight)
        disp = np.zeros(la.shape[:2], np.float32)
        di, _ = _image(disp, 5)
        rc = self._lib.asw_stereo_match_refined(self._h, C.byref(li), C.byref(ri), C.byref(di), int(algorithmType), winSize,
                                                minDisparity, numDisparity, 0.0, _smooth_word(iterations), float(sigma_c), float(lam),
                                                None, None)
        self._strict(rc, "asw_stereo_match_smoothed")
        return disp

    def bgr2gray(self, img):
        ii, ia = _image(img)
        out = np.zeros(ia.shape[:2], np.uint8)
        rc = self._lib.asw_bgr2gray(self._h, C.byref(ii), out.ctypes.data_as(C.c_void_p))
        self._finish(rc, "asw_bgr2gray")
        return out

    # ---- resident (HBM) API used by bench.py.  The reference has no equivalent whose silent returns could be mimicked:
    # every non-zero status raises AswError (a rejected upload or a failed match also empties the slot's results, so a
    # later download cannot hand back another frame's disparity) ----
    def _strict(self, rc, where):
        _state.status = rc
        if rc != 0:
            raise AswError(rc, where)

    def upload_pair(self, slot, left, right):
        li, la = _image(left)
        ri, ra = _image(right)
        self._strict(self._lib.asw_upload_pair(self._h, slot, C.byref(li), C.byref(ri)), "asw_upload_pair")

    def match_resident(self, slot, disparityType, algorithmType, winSize, minDisparity, numDisparity, keep_volume=False,
                       subpixel=None, cross_scale=None, scanline=None):
        rc = self._lib.asw_match_resident(self._h, slot, _disparity_type(disparityType, subpixel, cross_scale, scanline), int(algorithmType), winSize,
                                          minDisparity, numDisparity, 1 if keep_volume else 0)
        self._strict(rc, "asw_match_resident")

    def match_refined_resident(self, slot, algorithmType, winSize, minDisparity, numDisparity, maxDiff=1.0, refineWin=15,
                               gamma_c=REFINE_GAMMA_C, gamma_s=REFINE_GAMMA_S):
        """asw_match_refined_resident: both directions on the slot's pair, the refined map becomes the slot's disparity ->
        (rejected pixels, unfillable pixels)."""
        nr, nu = C.c_int(0), C.c_int(0)
        rc = self._lib.asw_match_refined_resident(self._h, slot, int(algorithmType), winSize, minDisparity, numDisparity,
                                                  float(maxDiff), int(refineWin), float(gamma_c), float(gamma_s), C.byref(nr),
                                                  C.byref(nu))
        self._strict(rc, "asw_match_refined_resident")
        return nr.value, nu.value

    def match_smoothed_resident(self, slot, algorithmType, winSize, minDisparity, numDisparity, sigma_c=SMOOTH_SIGMA_C,
                                lam=SMOOTH_LAMBDA, iterations=SMOOTH_ITERATIONS):
        """asw_match_smoothed_resident: one DISPARITY_LEFT match on the slot's pair with its confidence, smoothed with the resident
        left image as guide; the smoothed map becomes the slot's disparity (no volume is kept)."""
        rc = self._lib.asw_match_refined_resident(self._h, slot, int(algorithmType), winSize, minDisparity, numDisparity, 0.0,
                                                  _smooth_word(iterations), float(sigma_c), float(lam), None, None)
        self._strict(rc, "asw_match_smoothed_resident")

    def download_disparity(self, slot, shape, confidence=False):
        """confidence: (disp, conf), the confidence computed from the volume the slot kept (match_resident with keep_volume);
        ERR_NO_FRAME without one."""
        disp = np.zeros(tuple(shape) + ((2,) if confidence else ()), np.float32)
        di, _ = _image(disp, 5)
        self._strict(self._lib.asw_download_disparity(self._h, slot, C.byref(di)), "asw_download_disparity")
        return (disp[..., 0].copy(), disp[..., 1].copy()) if confidence else disp

    def download_volume(self, slot, shape):
        vol = np.zeros(shape, np.float32)
        self._strict(self._lib.asw_download_volume(self._h, slot, vol.ctypes.data_as(C.c_void_p), vol.size), "asw_download_volume")
        return vol

    # ---- driver-side pre/post-processing on the device (aswStereoMatch.cpp:30-31, 67-89, 97-98) ----
    def preprocess_pair(self, slot, left_full, right_full, dsize=(640, 360), detail_boost=True):
        """resize(img, Size(w, h)) + the HSV-V bilateral detail boost of the reference's main(); the result becomes the
        resident pair of `slot`."""
        li, la = _image(left_full)
        ri, ra = _image(right_full)
        rc = self._lib.asw_preprocess_pair(self._h, slot, C.byref(li), C.byref(ri), int(dsize[0]), int(dsize[1]),
                                           1 if detail_boost else 0)
        self._strict(rc, "asw_preprocess_pair")
        return True

    def download_pair(self, slot, shape):
        """The resident 8U pair of `slot` (e.g. after preprocess_pair); shape = (rows, cols, channels)."""
        left = np.zeros(shape, np.uint8)
        right = np.zeros(shape, np.uint8)
        li, _ = _image(left)
        ri, _ = _image(right)
        self._strict(self._lib.asw_download_pair(self._h, slot, C.byref(li), C.byref(ri)), "asw_download_pair")
        return left, right

    def download_disparity_u8(self, slot, shape, normalize=True):
        """disparityMap.convertTo(CV_8UC1) [+ normalize(0, 255, NORM_MINMAX)] of the last match of `slot` (main.cpp:97-98)."""
        out = np.zeros(shape, np.uint8)
        oi, _ = _image(out)
        self._strict(self._lib.asw_download_disparity_u8(self._h, slot, C.byref(oi), 1 if normalize else 0),
                     "asw_download_disparity_u8")
        return out

    def timing(self):
        t = AswTiming()
        self._lib.asw_get_timing(self._h, C.byref(t))
        return {"total_ms": t.total_ms, "aggregate_ms": t.aggregate_ms, "cost_ms": t.cost_ms,
                "aggregate_launches": t.aggregate_launches}


def stereoMatchingBatch(lefts, rights, disparityType, algorithmType, winSize=15, minDisparity=0, numDisparity=64,
                        device_ids=None, out=None, subpixel=None, cross_scale=None, scanline=None):
    """asw_stereo_match_batch: frame i -> device device_ids[i % len(device_ids)], one host thread per device.
    subpixel: None, SUBPIXEL_PARABOLA or SUBPIXEL_EQUIANGULAR; cross_scale: None or a cross_scale() value; scanline: None or a
    scanline() value (not together with cross_scale); all are OR-ed into disparityType.

    out: optional list of C-contiguous float32 (H, W) arrays to receive the disparities (a frame loop that reuses its
    output buffers avoids first-touch page faults on 8 MB per 1080p frame)."""
    lib = _lib.lib()
    disparityType = _disparity_type(disparityType, subpixel, cross_scale, scanline)
    n = len(lefts)
    if device_ids is None:
        device_ids = list(range(max(1, lib.asw_device_count())))
    keep = []
    L = (AswImage * n)()
    R = (AswImage * n)()
    D = (AswImage * n)()
    outs = []
    for i in range(n):
        li, la = _image(lefts[i])
        ri, ra = _image(rights[i])
        if out is not None:
            o = out[i]
            if not (isinstance(o, np.ndarray) and o.dtype == np.float32 and o.flags.c_contiguous and o.shape == la.shape[:2]):
                raise ValueError("out[%d] must be a C-contiguous float32 array of shape %s" % (i, (la.shape[:2],)))
        else:
            o = np.zeros((la.shape[0], la.shape[1]), np.float32)
        di, _ = _image(o, 5)
        L[i], R[i], D[i] = li, ri, di
        keep.append((la, ra))
        outs.append(o)
    devs = (C.c_int * len(device_ids))(*device_ids)
    rc = lib.asw_stereo_match_batch(n, L, R, D, disparityType, int(algorithmType), winSize, minDisparity, numDisparity,
                                    len(device_ids), devs)
    _state.status = rc
    if rc in _SILENT:
        return None
    if rc != 0:
        raise AswError(rc, "asw_stereo_match_batch")
    return outs


# ---- module-level functions with the reference's names, bound to a lazily created default context ----
_default = {}
_default_lock = threading.Lock()


def default_context(device_id=None):
    if device_id is None:
        device_id = int(os.environ.get("ASW_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    with _default_lock:
        if device_id not in _default:
            _default[device_id] = Context(device_id)
        return _default[device_id]


def _bind(name):
    def f(*args, **kwargs):
        return getattr(default_context(), name)(*args, **kwargs)
    f.__name__ = name
    f.__doc__ = getattr(Context, name).__doc__
    return f


stereoMatching = _bind("stereoMatching")
computeAD = _bind("computeAD")
computeTAD = _bind("computeTAD")
computeSimilarity = _bind("computeSimilarity")
getCostSAD = _bind("getCostSAD")
getCostSAD_d = _bind("getCostSAD_d")
computeAdaptiveWeight = _bind("computeAdaptiveWeight")
computeAdaptiveWeight_direct8 = _bind("computeAdaptiveWeight_direct8")
computeAdaptiveWeight_GuidedF_3 = _bind("computeAdaptiveWeight_GuidedF_3")
computeNCC = _bind("computeNCC")
computeNCC_costs = _bind("computeNCC_costs")
computeAdaptiveWeight_geodesic = _bind("computeAdaptiveWeight_geodesic")
getGeodesicDist = _bind("getGeodesicDist")
getGuidedFilter = _bind("getGuidedFilter")
computeAdaptiveWeight_GuidedF = _bind("computeAdaptiveWeight_GuidedF")
computeAdaptiveWeight_GuidedF_2 = _bind("computeAdaptiveWeight_GuidedF_2")
computeAdaptiveWeight_WeightedMedian = _bind("computeAdaptiveWeight_WeightedMedian")
computeAdaptiveWeight_BLO1 = _bind("computeAdaptiveWeight_BLO1")
computeAdaptiveWeight_cross = _bind("computeAdaptiveWeight_cross")
computeCensus = _bind("computeCensus")
computeADCensus = _bind("computeADCensus")
computeAdaptiveWeight_adcensus = _bind("computeAdaptiveWeight_adcensus")
computeAdaptiveWeight_twopass = _bind("computeAdaptiveWeight_twopass")
computeAdaptiveWeight_permeability = _bind("computeAdaptiveWeight_permeability")
winnerTakeAll = _bind("winnerTakeAll")
getDisparity_SGBM = _bind("getDisparity_SGBM")
sgbm = _bind("sgbm")
sgbm_paths = _bind("sgbm_paths")
sgbm_census = _bind("sgbm_census")
filterSpeckles = _bind("filterSpeckles")
getDisparity_BM = _bind("getDisparity_BM")
stereoBM = _bind("stereoBM")
refineDisparity = _bind("refineDisparity")
stereoMatchingRefined = _bind("stereoMatchingRefined")
smoothDisparity = _bind("smoothDisparity")
stereoMatchingSmoothed = _bind("stereoMatchingSmoothed")
