// aswMethods_mi355x.hpp -- C++ surface of the reference (aswStereoMatch/methods/aswMethods.h, "M.h") on
// top of the C-ABI of asw_mi355x.h.  Header-only.
//
//  * With OpenCV available (#include <opencv2/core.hpp> found, or ASW_WITH_OPENCV defined) the functions
//    take and return cv::Mat with EXACTLY the reference signatures, so a maintainer of the reference
//    replaces `#include "methods/aswMethods.h"` by this header and links libasw_mi355x.so
//    (INTEGRATION.md).
//  * Without OpenCV the same functions are available on asw::Mat, a minimal stand-in for the part of
//    cv::Mat the path uses (rows, cols, type, step, data, empty()).
//
// Error behaviour mirrors the reference: where it returns silently or an empty Mat (size mismatch, even
// window) so does the shim; statuses with no reference equivalent (HIP error, unsupported method) throw
// std::runtime_error -- the reference throws cv::Exception in comparable situations (M.cpp:103-116).
#pragma once
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "asw_mi355x.h"

#if !defined(ASW_WITH_OPENCV) && defined(__has_include)
#if __has_include(<opencv2/core.hpp>)
#define ASW_WITH_OPENCV 1
#endif
#endif
#ifdef ASW_WITH_OPENCV
#include <opencv2/core.hpp>
#endif

// parametersStereo.h:4-24 -- same names and values (skip when the reference header is also included)
#ifndef ASW_REFERENCE_ENUMS_DEFINED
#define ASW_REFERENCE_ENUMS_DEFINED
enum DisparityType { DISPARITY_LEFT = 0, DISPARITY_RIGHT = 1 };
enum StereoMatchingAlgorithms {
    BM = 0, SGBM = 1, ADAPTIVE_WEIGHT = 2, ADAPTIVE_WEIGHT_8DIRECT = 3, ADAPTIVE_WEIGHT_GEODESIC = 4,
    ADAPTIVE_WEIGHT_BILATERAL_GRID = 5, ADAPTIVE_WEIGHT_BLO1 = 6, ADAPTIVE_WEIGHT_GUIDED_FILTER = 7,
    ADAPTIVE_WEIGHT_GUIDED_FILTER_2 = 8, ADAPTIVE_WEIGHT_GUIDED_FILTER_3 = 9, ADAPTIVE_WEIGHT_MEDIAN = 10, NCC = 11,
    ADAPTIVE_WEIGHT_CROSS = 12  // not in the reference: cross-based support regions (asw_mi355x.h)
};
#endif
// Not in the reference: the sub-pixel rules of asw_mi355x.h (ASW_DISPARITY_SUBPIXEL_*), for stereoMatchingSubpixel below
enum SubpixelMethod { SUBPIXEL_PARABOLA = ASW_DISPARITY_SUBPIXEL_PARABOLA, SUBPIXEL_EQUIANGULAR = ASW_DISPARITY_SUBPIXEL_EQUIANGULAR };

namespace asw {

// ---- minimal Mat used when OpenCV is absent --------------------------------------------------------
struct Mat {
    int rows = 0, cols = 0, channels_ = 0, depth_ = ASW_8U;
    size_t step = 0;
    std::shared_ptr<std::vector<uint8_t>> buf;
    uint8_t* data = nullptr;
    Mat() {}
    Mat(int r, int c, int depth, int ch) { create(r, c, depth, ch); }
    void create(int r, int c, int depth, int ch)
    {
        rows = r; cols = c; depth_ = depth; channels_ = ch;
        step = (size_t)c * ch * (depth == ASW_32F ? 4 : 1);
        buf = std::make_shared<std::vector<uint8_t>>(step * r);
        data = buf->data();
    }
    bool empty() const { return data == nullptr || rows == 0 || cols == 0; }
    int channels() const { return channels_; }
    int depth() const { return depth_; }
};

// cv::Point where OpenCV is absent (key of getGeodesicDist's map, M.h:141)
struct Point {
    int x = 0, y = 0;
    Point() {}
    Point(int x_, int y_) : x(x_), y(y_) {}
};

namespace detail {

inline asw_ctx* context()
{
    // one lazily created context per host thread (contexts are not shared between threads)
    struct Holder {
        asw_ctx* c = nullptr;
        ~Holder() { if (c) asw_destroy(c); }
    };
    static thread_local Holder h;
    if (!h.c) {
        int rc = asw_create(0, &h.c);
        if (rc != ASW_OK) throw std::runtime_error(std::string("asw_create: ") + asw_status_string(rc));
    }
    return h.c;
}

inline bool silent(int rc) { return rc == ASW_ERR_SIZE_MISMATCH || rc == ASW_ERR_EVEN_WINDOW; }
inline void raise_unless_ok(int rc, const char* what)
{
    if (rc != ASW_OK && !silent(rc)) throw std::runtime_error(std::string(what) + ": " + asw_status_string(rc));
}

#ifdef ASW_WITH_OPENCV
typedef cv::Mat MatT;
inline asw_image view(const cv::Mat& m)
{
    asw_image v{m.data, m.rows, m.cols, m.channels(), m.depth() == CV_32F ? ASW_32F : (m.depth() == CV_8U ? ASW_8U : -1), m.step[0]};
    return v;
}
inline cv::Mat make(int r, int c, int depth, int ch) { return cv::Mat(r, c, CV_MAKETYPE(depth == ASW_32F ? CV_32F : CV_8U, ch)); }
#else
typedef asw::Mat MatT;
inline asw_image view(const asw::Mat& m) { return asw_image{m.data, m.rows, m.cols, m.channels_, m.depth_, m.step}; }
inline asw::Mat make(int r, int c, int depth, int ch) { return asw::Mat(r, c, depth, ch); }
#endif

template <typename Fn>
inline MatT aggregate(const MatT& l, const MatT& r, Fn fn, const char* what)
{
    if (l.empty() || r.empty()) return MatT();
    MatT disp = make(l.rows, l.cols, ASW_32F, 1);
    asw_image li = view(l), ri = view(r), di = view(disp);
    int rc = fn(context(), &li, &ri, &di);
    raise_unless_ok(rc, what);
    return rc == ASW_OK ? disp : MatT();  // empty Mat where the reference returns Mat()
}

template <typename T, typename Fn>
inline void cost_volume(const MatT& l, const MatT& r, std::vector<MatT>& out, int n, int depth, int pad, Fn fn, const char* what)
{
    if (!out.empty()) out.clear();  // M.cpp:222-225
    if (l.empty() || r.empty() || n <= 0) return;
    const int H = l.rows + 2 * pad, W = l.cols + 2 * pad;
    std::vector<T> vol((size_t)n * H * W);
    asw_image li = view(l), ri = view(r);
    int rc = fn(context(), &li, &ri, vol.data());
    raise_unless_ok(rc, what);
    if (rc != ASW_OK) return;  // silent return of the reference: cost_ds stays empty
    for (int k = 0; k < n; k++) {
        MatT m = make(H, W, depth, 1);
        asw_image mi = view(m);
        for (int y = 0; y < H; y++)
            std::memcpy((uint8_t*)mi.data + (size_t)y * mi.step, vol.data() + ((size_t)k * H + y) * W, (size_t)W * sizeof(T));
        out.push_back(m);
    }
}

// the selector's SGBM result (whole numbers 0..255 in a CV_32F map) as the CV_8U Mat convertTo(CV_8U, 1/16) gives the reference
inline MatT f32_to_u8(const MatT& f)
{
    if (f.empty()) return MatT();
    MatT u = make(f.rows, f.cols, ASW_8U, 1);
    asw_image fi = view(f), ui = view(u);
    for (int y = 0; y < f.rows; y++) {
        const float* src = (const float*)((const uint8_t*)fi.data + (size_t)y * fi.step);
        uint8_t* dst = (uint8_t*)ui.data + (size_t)y * ui.step;
        for (int x = 0; x < f.cols; x++) dst[x] = (uint8_t)src[x];
    }
    return u;
}

}  // namespace detail
}  // namespace asw

// ---------------------------------------------------------------------------------------------------
// The reference's functions (M.h:91-182), global namespace like the reference
// ---------------------------------------------------------------------------------------------------
typedef asw::detail::MatT AswMat;

// M.h:94 / aswMethods.cpp:158-194: StereoSGBM (MODE_SGBM_3WAY) with the reference's settings, CV_8U result.  The CV_Error cases
// (numDisparity % 16 != 0, even winSize, an empty image) throw.
inline void getDisparity_SGBM(AswMat srcLeft, AswMat srcRight, AswMat& disparityMap, int winSize = 15, int minDisparity = 0,
                              int numDisparity = 64)
{
    if (srcLeft.empty() || srcRight.empty()) throw std::runtime_error("getDisparity_SGBM: one of the input images is empty");
    AswMat d = asw::detail::aggregate(srcLeft, srcRight, [&](asw_ctx* c, asw_image* l, asw_image* r, asw_image* o) {
        return asw_stereo_match(c, l, r, o, (int)DISPARITY_LEFT, (int)SGBM, winSize, minDisparity, numDisparity, nullptr, 0);
    }, "getDisparity_SGBM");
    disparityMap = asw::detail::f32_to_u8(d);
}

namespace asw {
namespace detail {
// getDisparity_SGBM_paths / getDisparity_SGBM_census: getDisparity_SGBM's argument rules around call(left, right, disp16, w), an
// asw_sgbm_paths or asw_sgbm_census call, and the CV_8U map of its int16 result (convertTo(CV_8U, 1/16): round half to even, saturate)
template <typename Call>
inline void sgbm_u8(const MatT& srcLeft, const MatT& srcRight, MatT& disparityMap, int winSize, int numDisparity, const char* where,
                    Call call)
{
    const int w = winSize > 0 ? winSize : 3;
    int rc = numDisparity % 16 != 0 || winSize % 2 == 0 ? ASW_ERR_UNSUPPORTED_METHOD : w > 4096 ? ASW_ERR_BAD_ARGUMENT : ASW_OK;
    const int H = srcLeft.rows, W = srcLeft.cols;
    std::vector<short> d16((size_t)H * W);
    if (rc == ASW_OK) {
        asw_image li = view(srcLeft), ri = view(srcRight);
        asw_image di{d16.data(), H, W, 1, ASW_16S, (size_t)W * sizeof(short)};
        rc = call(&li, &ri, &di, w);
    }
    raise_unless_ok(rc, where);
    if (rc != ASW_OK) {
        disparityMap = MatT();
        return;
    }
    MatT u = make(H, W, ASW_8U, 1);
    asw_image ui = view(u);
    for (int y = 0; y < H; y++) {
        uint8_t* dst = (uint8_t*)ui.data + (size_t)y * ui.step;
        for (int x = 0; x < W; x++) {
            const int v = d16[(size_t)y * W + x], q = v >> 4, r = v & 15;  // v / 16 = q + r / 16, q = floor
            const int n = q + (r > 8 || (r == 8 && (q & 1)));
            dst[x] = (uint8_t)(n < 0 ? 0 : n > 255 ? 255 : n);
        }
    }
    disparityMap = u;
}
}  // namespace detail
}  // namespace asw

// Not in the reference: getDisparity_SGBM with the aggregated cost summed over the path directions of `paths` (an OR of
// ASW_SGBM_PATH_*, asw_sgbm_paths) instead of the three of MODE_SGBM_3WAY.  The same StereoSGBM settings,
// the same CV_8U result (convertTo(CV_8U, 1/16) of the int16 map: round half to even, saturate) and the same throwing behaviour.
inline void getDisparity_SGBM_paths(AswMat srcLeft, AswMat srcRight, AswMat& disparityMap, int winSize = 15, int minDisparity = 0,
                                    int numDisparity = 64, int paths = ASW_SGBM_PATHS_HH)
{
    if (srcLeft.empty() || srcRight.empty()) throw std::runtime_error("getDisparity_SGBM_paths: one of the input images is empty");
    asw::detail::sgbm_u8(srcLeft, srcRight, disparityMap, winSize, numDisparity, "getDisparity_SGBM_paths",
                         [&](asw_image* li, asw_image* ri, asw_image* di, int w) {
                             const int cn = li->channels;
                             return asw_sgbm_paths(asw::detail::context(), li, ri, di, minDisparity, numDisparity, w, 8 * cn * w * w,
                                                   32 * cn * w * w, 200, 10, 10, 175, 32, paths, nullptr, 0);
                         });
}

// Not in the reference: getDisparity_SGBM_paths with the census cost of asw_sgbm_census in place of the
// prefilter and the Birchfield-Tomasi cost.  getDisparity_SGBM's settings with the penalties of one plane, P1 = 8 w^2 and P2 = 32 w^2
// whatever the channel count (the cost comes from one gray plane), uniqueness 10, speckles 175 / 32, disp12MaxDiff 200.  The
// penalties are a stated choice, carried over from the Birchfield-Tomasi cost, not a tuned one: a census pixel cost ranges over
// 0..62.  The same CV_8U result and the same throwing behaviour.
inline void getDisparity_SGBM_census(AswMat srcLeft, AswMat srcRight, AswMat& disparityMap, int winSize = 15, int minDisparity = 0,
                                     int numDisparity = 64, int paths = ASW_SGBM_PATHS_HH)
{
    if (srcLeft.empty() || srcRight.empty()) throw std::runtime_error("getDisparity_SGBM_census: one of the input images is empty");
    asw::detail::sgbm_u8(srcLeft, srcRight, disparityMap, winSize, numDisparity, "getDisparity_SGBM_census",
                         [&](asw_image* li, asw_image* ri, asw_image* di, int w) {
                             return asw_sgbm_census(asw::detail::context(), li, ri, di, minDisparity, numDisparity, w, 8 * w * w,
                                                    32 * w * w, 200, 10, 175, 32, paths, nullptr, 0);
                         });
}

// M.h:93 / aswMethods.cpp:100-146: StereoBM (PREFILTER_XSOBEL) with the reference's settings, CV_8U result; a 3-channel image is
// converted to gray first.  The CV_Error cases (numDisparity % 16 != 0, even winSize, an empty image, a block size outside
// 5..min(rows, cols, 255)) throw, and so does every other failure.  stereoMatching(..., BM, ...) is not routed here.
inline void getDisparity_BM(AswMat srcLeft, AswMat srcRight, AswMat& disparityMap, int winSize = 15, int minDisparity = 0,
                            int numDisparity = 64)
{
    if (srcLeft.empty() || srcRight.empty()) throw std::runtime_error("getDisparity_BM: one of the input images is empty");
    AswMat d = asw::detail::make(srcLeft.rows, srcLeft.cols, ASW_8U, 1);
    asw_image li = asw::detail::view(srcLeft), ri = asw::detail::view(srcRight), di = asw::detail::view(d);
    const int rc = asw_get_disparity_bm(asw::detail::context(), &li, &ri, &di, winSize, minDisparity, numDisparity);
    if (rc != ASW_OK) throw std::runtime_error(std::string("getDisparity_BM: ") + asw_status_string(rc));
    disparityMap = d;
}

// M.h:91-92 / M.cpp:46-88 (SGBM: the CV_8U map of getDisparity_SGBM, as M.cpp:54-55; every other method CV_32F)
inline void stereoMatching(AswMat srcLeft, AswMat srcRight, AswMat& disparityMap, DisparityType disparityType,
                           StereoMatchingAlgorithms algorithmType, int winSize = 15, int minDisparity = 0, int numDisparity = 64)
{
    if (algorithmType == SGBM) {
        getDisparity_SGBM(srcLeft, srcRight, disparityMap, winSize, minDisparity, numDisparity);
        return;
    }
    AswMat d = asw::detail::aggregate(srcLeft, srcRight, [&](asw_ctx* c, asw_image* l, asw_image* r, asw_image* o) {
        return asw_stereo_match(c, l, r, o, (int)disparityType, (int)algorithmType, winSize, minDisparity, numDisparity, nullptr, 0);
    }, "stereoMatching");
    disparityMap = d;  // `disparityMap = computeAdaptiveWeight...(...)`, M.cpp:58-82 (empty Mat on silent errors)
}

// Not in the reference: stereoMatching with a sub-pixel disparity map -- the method's winner-take-all
// map, every pixel moved by at most half a disparity along the parabola / the equiangular V through the three aggregated costs
// around its winner.  Silent errors leave an empty Mat like stereoMatching; SGBM (its CV_8U map has no fraction), BM and NCC throw.
inline void stereoMatchingSubpixel(AswMat srcLeft, AswMat srcRight, AswMat& disparityMap, DisparityType disparityType,
                                   StereoMatchingAlgorithms algorithmType, int winSize = 15, int minDisparity = 0, int numDisparity = 64,
                                   SubpixelMethod method = SUBPIXEL_PARABOLA)
{
    if (algorithmType == SGBM) throw std::runtime_error("stereoMatchingSubpixel: SGBM has no sub-pixel form here");
    AswMat d = asw::detail::aggregate(srcLeft, srcRight, [&](asw_ctx* c, asw_image* l, asw_image* r, asw_image* o) {
        return asw_stereo_match(c, l, r, o, (int)disparityType | (int)method, (int)algorithmType, winSize, minDisparity, numDisparity,
                                nullptr, 0);
    }, "stereoMatchingSubpixel");
    disparityMap = d;
}

// Not in the reference: stereoMatching with cross-scale cost aggregation (Zhang et al. 2014) -- the method runs
// on `scales` (2..5) levels of a 2x2-mean pyramid of the pair, and the map is the winner of the regularised finest-scale volume,
// lambda = lambdaQ / 64 (lambdaQ 1..255).  subpixel: 0, SUBPIXEL_PARABOLA or SUBPIXEL_EQUIANGULAR, applied to that volume.  Silent
// errors leave an empty Mat like stereoMatching; arguments out of range, a candidate range too short for the scales, SGBM (it has no
// selector volume), BM and NCC throw.
inline void stereoMatchingCrossScale(AswMat srcLeft, AswMat srcRight, AswMat& disparityMap, DisparityType disparityType,
                                     StereoMatchingAlgorithms algorithmType, int winSize = 15, int minDisparity = 0, int numDisparity = 64,
                                     int scales = 3, int lambdaQ = 19, int subpixel = 0)
{
    if (algorithmType == SGBM) throw std::runtime_error("stereoMatchingCrossScale: SGBM has no cost volume to combine");
    AswMat d = asw::detail::aggregate(srcLeft, srcRight, [&](asw_ctx* c, asw_image* l, asw_image* r, asw_image* o) {
        return asw_stereo_match(c, l, r, o, (int)disparityType | subpixel | asw_disparity_cross_scale(scales, lambdaQ), (int)algorithmType,
                                winSize, minDisparity, numDisparity, nullptr, 0);
    }, "stereoMatchingCrossScale");
    disparityMap = d;
}

// Not in the reference: stereoMatching with scanline optimisation of the aggregated volume (Mei et al. 2011) --
// the method's volume is regularised along four scan paths with P1 = p1Code * 4^(unitCode - 5) and P2 = p2Ratio * P1 (p1Code 1..127,
// unitCode 0..7, p2Ratio 1..8), and the map is the winner of the result.  subpixel: 0, SUBPIXEL_PARABOLA or SUBPIXEL_EQUIANGULAR,
// applied to that volume.  Silent errors leave an empty Mat like stereoMatching; arguments out of range, SGBM (it has no selector
// volume), BM and NCC throw.
inline void stereoMatchingScanline(AswMat srcLeft, AswMat srcRight, AswMat& disparityMap, DisparityType disparityType,
                                   StereoMatchingAlgorithms algorithmType, int winSize = 15, int minDisparity = 0, int numDisparity = 64,
                                   int p1Code = 8, int unitCode = 5, int p2Ratio = 4, int subpixel = 0)
{
    if (algorithmType == SGBM) throw std::runtime_error("stereoMatchingScanline: SGBM has no cost volume to optimise");
    AswMat d = asw::detail::aggregate(srcLeft, srcRight, [&](asw_ctx* c, asw_image* l, asw_image* r, asw_image* o) {
        return asw_stereo_match(c, l, r, o, (int)disparityType | subpixel | asw_disparity_scanline(p1Code, unitCode, p2Ratio),
                                (int)algorithmType, winSize, minDisparity, numDisparity, nullptr, 0);
    }, "stereoMatchingScanline");
    disparityMap = d;
}

// Not in the reference: stereoMatching with a per-pixel confidence beside the map (asw_mi355x.h "Confidence") --
// the winner's margin over the best candidate that is not its neighbour, in units of the cost range of the pixel, in [0, 1], read off
// the volume the call works on.  disparityType: DISPARITY_LEFT / DISPARITY_RIGHT, optionally with the sub-pixel, cross-scale or
// scanline flags of asw_mi355x.h OR-ed in.  Both maps are CV_32F, one channel.  Silent errors leave two empty Mats like
// stereoMatching; SGBM (it has no selector volume), BM and NCC throw.
inline void stereoMatchingConfidence(AswMat srcLeft, AswMat srcRight, AswMat& disparityMap, AswMat& confidenceMap, int disparityType,
                                     StereoMatchingAlgorithms algorithmType, int winSize = 15, int minDisparity = 0, int numDisparity = 64)
{
    using namespace asw::detail;
    disparityMap = AswMat();
    confidenceMap = AswMat();
    if (srcLeft.empty() || srcRight.empty()) return;
    AswMat both = make(srcLeft.rows, srcLeft.cols, ASW_32F, 2);  // {disparity, confidence} interleaved
    asw_image li = view(srcLeft), ri = view(srcRight), bi = view(both);
    const int rc = asw_stereo_match(context(), &li, &ri, &bi, disparityType, (int)algorithmType, winSize, minDisparity, numDisparity, nullptr, 0);
    raise_unless_ok(rc, "stereoMatchingConfidence");
    if (rc != ASW_OK) return;
    AswMat d = make(both.rows, both.cols, ASW_32F, 1), c = make(both.rows, both.cols, ASW_32F, 1);
    asw_image di = view(d), ci = view(c);
    for (int y = 0; y < both.rows; y++) {
        const float* src = (const float*)((const uint8_t*)bi.data + (size_t)y * bi.step);
        float* dd = (float*)((uint8_t*)di.data + (size_t)y * di.step);
        float* cc = (float*)((uint8_t*)ci.data + (size_t)y * ci.step);
        for (int x = 0; x < both.cols; x++) { dd[x] = src[2 * x]; cc[x] = src[2 * x + 1]; }
    }
    disparityMap = d;
    confidenceMap = c;
}

// M.h:101-102
inline void computeAD(AswMat leftImg, AswMat rightImg, std::vector<AswMat>& cost_ds, DisparityType dispType = DISPARITY_LEFT,
                      int minDisparity = 0, int numDisparity = 30)
{
    asw::detail::cost_volume<uint8_t>(leftImg, rightImg, cost_ds, numDisparity, ASW_8U, 0, [&](asw_ctx* c, asw_image* l, asw_image* r, uint8_t* v) {
        return asw_cost_ad(c, l, r, v, (int)dispType, minDisparity, numDisparity);
    }, "computeAD");
}

// M.h:105-106
inline void computeTAD(AswMat leftImg, AswMat rightImg, std::vector<AswMat>& cost_ds, DisparityType dispType = DISPARITY_LEFT,
                       int threshold_T = 30, int minDisparity = 0, int numDisparity = 30)
{
    asw::detail::cost_volume<uint8_t>(leftImg, rightImg, cost_ds, numDisparity, ASW_8U, 0, [&](asw_ctx* c, asw_image* l, asw_image* r, uint8_t* v) {
        return asw_cost_tad(c, l, r, v, (int)dispType, threshold_T, minDisparity, numDisparity);
    }, "computeTAD");
}

// M.h:117-118
inline void computeSD(AswMat leftImg, AswMat rightImg, std::vector<AswMat>& cost_ds, DisparityType dispType = DISPARITY_LEFT,
                      int minDisparity = 0, int numDisparity = 30)
{
    asw::detail::cost_volume<uint8_t>(leftImg, rightImg, cost_ds, numDisparity, ASW_8U, 0, [&](asw_ctx* c, asw_image* l, asw_image* r, uint8_t* v) {
        return asw_cost_sd(c, l, r, v, (int)dispType, minDisparity, numDisparity);
    }, "computeSD");
}

// M.h:109-111
inline void computeSimilarity(AswMat leftImg, AswMat rightImg, std::vector<AswMat>& cost_d_imgs, double regularity, double thresC,
                              double thresG, DisparityType dispType, int minDisparity, int numDisparity)
{
    asw::detail::cost_volume<float>(leftImg, rightImg, cost_d_imgs, numDisparity, ASW_32F, 0, [&](asw_ctx* c, asw_image* l, asw_image* r, float* v) {
        return asw_cost_similarity(c, l, r, v, regularity, thresC, thresG, (int)dispType, 0, minDisparity, numDisparity);
    }, "computeSimilarity");
}

// M.h:112-114 (padded overload)
inline void computeSimilarity(AswMat leftImg, AswMat rightImg, std::vector<AswMat>& cost_d_imgs, double regularity, double thresC,
                              double thresG, DisparityType dispType, int winSize, int minDisparity, int numDisparity)
{
    if (winSize % 2 == 0) return;  // M.cpp:654-657: returns before touching cost_d_imgs
    asw::detail::cost_volume<float>(leftImg, rightImg, cost_d_imgs, numDisparity, ASW_32F, winSize / 2, [&](asw_ctx* c, asw_image* l, asw_image* r, float* v) {
        return asw_cost_similarity(c, l, r, v, regularity, thresC, thresG, (int)dispType, winSize, minDisparity, numDisparity);
    }, "computeSimilarity(padded)");
}

// M.h:122-123: computeNCC -> disparity
inline AswMat computeNCC(AswMat leftImg, AswMat rightImg, DisparityType dispType = DISPARITY_LEFT, int winSize = 7,
                         int minDisparity = 0, int numDisparity = 30)
{
    return asw::detail::aggregate(leftImg, rightImg, [&](asw_ctx* c, asw_image* l, asw_image* r, asw_image* o) {
        return asw_ncc_disparity(c, l, r, o, (int)dispType, winSize, minDisparity, numDisparity);
    }, "computeNCC");
}

// M.h:124-126: computeNCC -> min-max normalised cost planes
inline void computeNCC(AswMat leftImg, AswMat rightImg, std::vector<AswMat>& cost_ds, DisparityType dispType = DISPARITY_LEFT,
                       int winSize = 7, int minDisparity = 0, int numDisparity = 30)
{
    asw::detail::cost_volume<float>(leftImg, rightImg, cost_ds, numDisparity, ASW_32F, 0, [&](asw_ctx* c, asw_image* l, asw_image* r, float* v) {
        return asw_cost_ncc(c, l, r, v, (int)dispType, winSize, minDisparity, numDisparity, 1);
    }, "computeNCC(costs)");
}

// M.h:133-134
inline AswMat computeAdaptiveWeight(AswMat leftImg, AswMat rightImg, double gamma_c = 30, double gamma_g = 2,
                                    DisparityType dispType = DISPARITY_LEFT, int winSize = 7, int minDisparity = 186,
                                    int numDisparity = 144)
{
    return asw::detail::aggregate(leftImg, rightImg, [&](asw_ctx* c, asw_image* l, asw_image* r, asw_image* o) {
        return asw_aggregate_bilateral(c, l, r, o, gamma_c, gamma_g, (int)dispType, winSize, minDisparity, numDisparity, nullptr, 0);
    }, "computeAdaptiveWeight");
}

// M.h:135-136 (DISPARITY_RIGHT: undefined behaviour in the reference, M.cpp:1291-1295 -> empty Mat here)
inline AswMat computeAdaptiveWeight_direct8(AswMat leftImg, AswMat rightImg, DisparityType dispType = DISPARITY_LEFT, int winSize = 7,
                                            int minDisparity = 186, int numDisparity = 144)
{
    return asw::detail::aggregate(leftImg, rightImg, [&](asw_ctx* c, asw_image* l, asw_image* r, asw_image* o) {
        return asw_aggregate_direct8(c, l, r, o, (int)dispType, winSize, minDisparity, numDisparity, nullptr, 0);
    }, "computeAdaptiveWeight_direct8");
}

// M.h:142-143
inline AswMat computeAdaptiveWeight_geodesic(AswMat leftImg, AswMat rightImg, DisparityType dispType = DISPARITY_LEFT, int winSize = 7,
                                             int minDisparity = 186, int numDisparity = 144)
{
    return asw::detail::aggregate(leftImg, rightImg, [&](asw_ctx* c, asw_image* l, asw_image* r, asw_image* o) {
        return asw_aggregate_geodesic(c, l, r, o, (int)dispType, winSize, minDisparity, numDisparity, nullptr, 0);
    }, "computeAdaptiveWeight_geodesic");
}

// M.h:174-176
inline AswMat computeAdaptiveWeight_GuidedF_3(AswMat leftImg, AswMat rightImg, DisparityType dispType = DISPARITY_LEFT, double eps = 1e-6,
                                              int winSize = 35, int minDisparity = 186, int numDisparity = 144)
{
    return asw::detail::aggregate(leftImg, rightImg, [&](asw_ctx* c, asw_image* l, asw_image* r, asw_image* o) {
        return asw_aggregate_guided3(c, l, r, o, (int)dispType, eps, winSize, minDisparity, numDisparity, nullptr, 0);
    }, "computeAdaptiveWeight_GuidedF_3");
}

// M.h:155-157
inline AswMat computeAdaptiveWeight_bilateralGrid(AswMat leftImg, AswMat rightImg, DisparityType dispType = DISPARITY_LEFT,
                                                  double sampleRateS = 10, double sampleRateR = 10, int minDisparity = 186,
                                                  int numDisparity = 144)
{
    return asw::detail::aggregate(leftImg, rightImg, [&](asw_ctx* c, asw_image* l, asw_image* r, asw_image* o) {
        return asw_aggregate_bilgrid(c, l, r, o, (int)dispType, sampleRateS, sampleRateR, minDisparity, numDisparity, nullptr, 0);
    }, "computeAdaptiveWeight_bilateralGrid");
}

// M.h:157-159
inline AswMat computeAdaptiveWeight_BLO1(AswMat leftImg, AswMat rightImg, DisparityType dispType = DISPARITY_LEFT, double sampleRateR = 10,
                                         int winSize = 35, int minDisparity = 186, int numDisparity = 144)
{
    return asw::detail::aggregate(leftImg, rightImg, [&](asw_ctx* c, asw_image* l, asw_image* r, asw_image* o) {
        return asw_aggregate_blo1(c, l, r, o, (int)dispType, sampleRateR, winSize, minDisparity, numDisparity, nullptr, 0);
    }, "computeAdaptiveWeight_BLO1");
}

// Not in the reference: cross-based support-region aggregation (asw_aggregate_cross) -> the f32 map; empty Mat
// for an even window
inline AswMat computeAdaptiveWeight_cross(AswMat leftImg, AswMat rightImg, DisparityType dispType = DISPARITY_LEFT, int tau = 20,
                                          int trunc = 20, int winSize = 15, int minDisparity = 0, int numDisparity = 64)
{
    return asw::detail::aggregate(leftImg, rightImg, [&](asw_ctx* c, asw_image* l, asw_image* r, asw_image* o) {
        return asw_aggregate_cross(c, l, r, o, (int)dispType, tau, trunc, winSize, minDisparity, numDisparity, nullptr, 0);
    }, "computeAdaptiveWeight_cross");
}

// Not in the reference: AD-Census matching (asw_aggregate_adcensus) -- the census + AD cost under the cross-based
// aggregation -> the f32 map; empty Mat for an even window
inline AswMat computeAdaptiveWeight_adcensus(AswMat leftImg, AswMat rightImg, DisparityType dispType = DISPARITY_LEFT, int tau = 20,
                                             int lambda_ad = 10, int lambda_census = 30, int winSize = 15, int minDisparity = 0,
                                             int numDisparity = 64)
{
    return asw::detail::aggregate(leftImg, rightImg, [&](asw_ctx* c, asw_image* l, asw_image* r, asw_image* o) {
        return asw_aggregate_adcensus(c, l, r, o, (int)dispType, tau, lambda_ad, lambda_census, winSize, minDisparity, numDisparity, nullptr,
                                      0);
    }, "computeAdaptiveWeight_adcensus");
}

// Not in the reference: two-pass (separable) adaptive-support-weight aggregation (asw_aggregate_twopass) -- a
// vertical, then a horizontal 1-D weighted pass, integer gammas 1..255 -> the f32 map; empty Mat for an even window
inline AswMat computeAdaptiveWeight_twopass(AswMat leftImg, AswMat rightImg, int gamma_c = 30, int gamma_g = 20,
                                            DisparityType dispType = DISPARITY_LEFT, int winSize = 15, int minDisparity = 0,
                                            int numDisparity = 64)
{
    return asw::detail::aggregate(leftImg, rightImg, [&](asw_ctx* c, asw_image* l, asw_image* r, asw_image* o) {
        return asw_aggregate_twopass(c, l, r, o, gamma_c, gamma_g, (int)dispType, winSize, minDisparity, numDisparity, nullptr, 0);
    }, "computeAdaptiveWeight_twopass");
}

// Not in the reference: recursive (permeability) aggregation over the whole image (asw_aggregate_permeability) --
// no window, integers sigma and trunc 1..255 -> the f32 map
inline AswMat computeAdaptiveWeight_permeability(AswMat leftImg, AswMat rightImg, DisparityType dispType = DISPARITY_LEFT, int sigma = 8,
                                                 int trunc = 20, int minDisparity = 0, int numDisparity = 64)
{
    return asw::detail::aggregate(leftImg, rightImg, [&](asw_ctx* c, asw_image* l, asw_image* r, asw_image* o) {
        return asw_aggregate_permeability(c, l, r, o, (int)dispType, sigma, trunc, minDisparity, numDisparity, nullptr, 0);
    }, "computeAdaptiveWeight_permeability");
}

// Not in the reference: the cross-check that consumes a DISPARITY_LEFT and a DISPARITY_RIGHT map (asw_lr_check)
inline AswMat leftRightCheck(AswMat dispLeft, AswMat dispRight, float maxDiff = 1.0f, float invalidValue = -1.0f, int* nInvalid = nullptr)
{
    if (dispLeft.rows != dispRight.rows || dispLeft.cols != dispRight.cols) return AswMat();
    AswMat out = asw::detail::make(dispLeft.rows, dispLeft.cols, ASW_32F, 1);
    asw_image a = asw::detail::view(dispLeft), b = asw::detail::view(dispRight), o = asw::detail::view(out);
    if (a.depth != ASW_32F || b.depth != ASW_32F || a.step != (size_t)a.cols * 4 || b.step != (size_t)b.cols * 4 || o.step != (size_t)o.cols * 4)
        throw std::runtime_error("leftRightCheck: continuous CV_32FC1 maps expected");
    int rc = asw_lr_check(asw::detail::context(), (const float*)a.data, (const float*)b.data, a.rows, a.cols, maxDiff, invalidValue,
                          (float*)o.data, nInvalid);
    asw::detail::raise_unless_ok(rc, "leftRightCheck");
    return rc == ASW_OK ? out : AswMat();
}

// Not in the reference: left-right refinement (asw_refine_disparity) -- cross-check, scan-line fill of the rejected pixels, weighted
// median over the filled ones; numValues = number of admissible disparities from minDisparity on.  Throws like leftRightCheck.
inline AswMat refineDisparity(AswMat guide, AswMat dispLeft, AswMat dispRight, int minDisparity, int numValues, float maxDiff = 1.0f,
                              int winSize = 15, double gamma_c = 60, double gamma_s = 9, int* nRejected = nullptr,
                              int* nUnfillable = nullptr)
{
    if (dispLeft.rows != dispRight.rows || dispLeft.cols != dispRight.cols || guide.rows != dispLeft.rows || guide.cols != dispLeft.cols)
        return AswMat();
    AswMat out = asw::detail::make(dispLeft.rows, dispLeft.cols, ASW_32F, 1);
    asw_image g = asw::detail::view(guide), a = asw::detail::view(dispLeft), b = asw::detail::view(dispRight), o = asw::detail::view(out);
    if (a.depth != ASW_32F || b.depth != ASW_32F || a.step != (size_t)a.cols * 4 || b.step != (size_t)b.cols * 4 || o.step != (size_t)o.cols * 4)
        throw std::runtime_error("refineDisparity: continuous CV_32FC1 maps expected");
    int rc = asw_refine_disparity(asw::detail::context(), &g, (const float*)a.data, (const float*)b.data, minDisparity, numValues, maxDiff,
                                  winSize, gamma_c, gamma_s, (float*)o.data, nullptr, nRejected, nUnfillable);
    asw::detail::raise_unless_ok(rc, "refineDisparity");
    return rc == ASW_OK ? out : AswMat();
}

// Not in the reference: stereoMatching in both directions + refineDisparity with srcLeft as guide (asw_stereo_match_refined)
inline AswMat stereoMatchingRefined(AswMat srcLeft, AswMat srcRight, StereoMatchingAlgorithms algorithmType, int winSize = 15,
                                    int minDisparity = 0, int numDisparity = 64, float maxDiff = 1.0f, int refineWin = 15,
                                    double gamma_c = 60, double gamma_s = 9, int* nRejected = nullptr, int* nUnfillable = nullptr)
{
    return asw::detail::aggregate(srcLeft, srcRight, [&](asw_ctx* c, asw_image* l, asw_image* r, asw_image* o) {
        return asw_stereo_match_refined(c, l, r, o, (int)algorithmType, winSize, minDisparity, numDisparity, maxDiff, refineWin, gamma_c,
                                        gamma_s, nRejected, nUnfillable);
    }, "stereoMatchingRefined");
}

// Not in the reference: confidence-weighted edge-aware smoothing (asw_smooth_disparity; asw_mi355x.h "Smoothing", DESIGN.md section
// 4.25) of a CV_32FC1 map with a CV_32FC1 trust value per pixel (e.g. the two maps of stereoMatchingConfidence, or a 0/1 validity mask),
// guided by an 8-bit image of 1 or 3 channels -> the dense fractional map.  The defaults are the paper's demonstration values.  Throws
// like refineDisparity.
inline AswMat smoothDisparity(AswMat guide, AswMat disparityMap, AswMat confidenceMap, double sigma_c = 8.0, double lambda = 900.0,
                              int iterations = 3)
{
    if (disparityMap.rows != confidenceMap.rows || disparityMap.cols != confidenceMap.cols || guide.rows != disparityMap.rows ||
        guide.cols != disparityMap.cols)
        return AswMat();
    AswMat out = asw::detail::make(disparityMap.rows, disparityMap.cols, ASW_32F, 1);
    asw_image g = asw::detail::view(guide), a = asw::detail::view(disparityMap), b = asw::detail::view(confidenceMap), o = asw::detail::view(out);
    if (a.depth != ASW_32F || b.depth != ASW_32F || a.channels != 1 || b.channels != 1 || a.step != (size_t)a.cols * 4 ||
        b.step != (size_t)b.cols * 4 || o.step != (size_t)o.cols * 4)
        throw std::runtime_error("smoothDisparity: continuous CV_32FC1 maps expected");
    int rc = asw_smooth_disparity(asw::detail::context(), &g, (const float*)a.data, (const float*)b.data, sigma_c, lambda, iterations,
                                  (float*)o.data);
    asw::detail::raise_unless_ok(rc, "smoothDisparity");
    return rc == ASW_OK ? out : AswMat();
}

// Not in the reference: ONE DISPARITY_LEFT stereoMatching with its confidence + smoothDisparity with srcLeft as guide
// (asw_stereo_match_smoothed); serves the methods stereoMatchingRefined refuses for their missing DISPARITY_RIGHT branch
inline AswMat stereoMatchingSmoothed(AswMat srcLeft, AswMat srcRight, StereoMatchingAlgorithms algorithmType, int winSize = 15,
                                     int minDisparity = 0, int numDisparity = 64, double sigma_c = 8.0, double lambda = 900.0,
                                     int iterations = 3)
{
    return asw::detail::aggregate(srcLeft, srcRight, [&](asw_ctx* c, asw_image* l, asw_image* r, asw_image* o) {
        return asw_stereo_match_smoothed(c, l, r, o, (int)algorithmType, winSize, minDisparity, numDisparity, sigma_c, lambda, iterations);
    }, "stereoMatchingSmoothed");
}

// M.h:156 / M.cpp:2442-2503: ONE disparity; the view that is not the reference view arrives bordered by the caller
// (copyMakeBorder by max_offset, M.cpp:2877-2878).  Empty Mat for an even window or a bordered view that is not wider.
inline AswMat getCostSAD_d(AswMat leftImg, AswMat rightImg, int disparity, DisparityType dispType = DISPARITY_LEFT, int winSize = 35)
{
    if (leftImg.empty() || rightImg.empty()) return AswMat();
    const AswMat& ref = dispType == DISPARITY_LEFT ? leftImg : rightImg;
    AswMat cost = asw::detail::make(ref.rows, ref.cols, ASW_32F, 1);
    asw_image li = asw::detail::view(leftImg), ri = asw::detail::view(rightImg), ci = asw::detail::view(cost);
    if (ci.step != (size_t)ci.cols * 4) throw std::runtime_error("getCostSAD_d: continuous output expected");
    int rc = asw_cost_sad_d(asw::detail::context(), &li, &ri, (float*)ci.data, disparity, (int)dispType, winSize);
    asw::detail::raise_unless_ok(rc, "getCostSAD_d");
    return rc == ASW_OK ? cost : AswMat();
}

// M.h:5-19: strict weak order of the map below (x first, then y)
#ifndef ASW_REFERENCE_COMPARATORS_DEFINED
#define ASW_REFERENCE_COMPARATORS_DEFINED
#ifdef ASW_WITH_OPENCV
typedef cv::Point AswPoint;
#else
typedef asw::Point AswPoint;
#endif
struct MY_COMP_Point2i {
    bool operator()(const AswPoint& left, const AswPoint& right) const
    {
        if (left.x < right.x) return true;
        if (left.x == right.x && left.y < right.y) return true;
        return false;
    }
};
#endif

// M.h:141 / M.cpp:1392-1424: weightGeoDist[Point(x, y)] = winSize x winSize CV_32FC1 window of geodesic distances of pixel
// (x, y); the map is cleared first; an even window returns without touching it (M.cpp:1394-1397).
inline void getGeodesicDist(AswMat originImg, std::map<AswPoint, AswMat, MY_COMP_Point2i>& weightGeoDist, int winSize = 15,
                            int iterTime = 3)
{
    if (winSize % 2 == 0 || originImg.empty()) return;
    const int H = originImg.rows, W = originImg.cols;
    const size_t cells = (size_t)winSize * winSize;
    std::vector<float> dense((size_t)H * W * cells);  // [y][x][win][win], asw_geodesic_dist's layout
    asw_image ii = asw::detail::view(originImg);
    int rc = asw_geodesic_dist(asw::detail::context(), &ii, dense.data(), winSize, iterTime);
    asw::detail::raise_unless_ok(rc, "getGeodesicDist");
    if (rc != ASW_OK) return;
    if (!weightGeoDist.empty()) weightGeoDist.clear();  // M.cpp:1406-1409
    for (int x = 0; x < W; x++)                         // insertion order of the reference: x outer, y inner (M.cpp:1410-1412)
        for (int y = 0; y < H; y++) {
            AswMat w = asw::detail::make(winSize, winSize, ASW_32F, 1);
            asw_image wi = asw::detail::view(w);
            for (int r = 0; r < winSize; r++)
                std::memcpy((uint8_t*)wi.data + (size_t)r * wi.step, dense.data() + ((size_t)y * W + x) * cells + (size_t)r * winSize,
                            (size_t)winSize * 4);
            weightGeoDist[AswPoint(x, y)] = w;
        }
}

// M.h:165
inline AswMat getGuidedFilter(AswMat guidedImg, AswMat inputP, int r, double eps)
{
    if (guidedImg.rows != inputP.rows || guidedImg.cols != inputP.cols) return AswMat();  // M.cpp:2768-2769
    AswMat q = asw::detail::make(inputP.rows, inputP.cols, ASW_32F, 1);
    asw_image gi = asw::detail::view(guidedImg), pi = asw::detail::view(inputP), qi = asw::detail::view(q);
    if (pi.depth != ASW_32F || pi.step != (size_t)pi.cols * 4 || qi.step != (size_t)qi.cols * 4)
        throw std::runtime_error("getGuidedFilter: inputP must be a continuous CV_32FC1 Mat");
    int rc = asw_guided_filter(asw::detail::context(), &gi, (const float*)pi.data, (float*)qi.data, r, eps);
    asw::detail::raise_unless_ok(rc, "getGuidedFilter");
    return rc == ASW_OK ? q : AswMat();
}

// M.h:166-168
inline AswMat computeAdaptiveWeight_GuidedF(AswMat leftImg, AswMat rightImg, DisparityType dispType = DISPARITY_LEFT, double eps = 1e-8,
                                            int winSize = 35, int minDisparity = 186, int numDisparity = 144)
{
    return asw::detail::aggregate(leftImg, rightImg, [&](asw_ctx* c, asw_image* l, asw_image* r, asw_image* o) {
        return asw_aggregate_guided(c, l, r, o, (int)dispType, eps, winSize, minDisparity, numDisparity, nullptr, 0);
    }, "computeAdaptiveWeight_GuidedF");
}

// M.h:169-171
inline AswMat computeAdaptiveWeight_GuidedF_2(AswMat leftImg, AswMat rightImg, DisparityType dispType = DISPARITY_LEFT, double eps = 1e-8,
                                              int winSize = 35, int minDisparity = 186, int numDisparity = 144)
{
    return asw::detail::aggregate(leftImg, rightImg, [&](asw_ctx* c, asw_image* l, asw_image* r, asw_image* o) {
        return asw_aggregate_guided2(c, l, r, o, (int)dispType, eps, winSize, minDisparity, numDisparity, nullptr, 0);
    }, "computeAdaptiveWeight_GuidedF_2");
}

// M.h:179-182
inline AswMat computeAdaptiveWeight_WeightedMedian(AswMat leftImg, AswMat rightImg, DisparityType dispType = DISPARITY_LEFT,
                                                   int winSize = 35, double sampleRateS = 10, double sampleRateR = 10,
                                                   int minDisparity = 186, int numDisparity = 144)
{
    return asw::detail::aggregate(leftImg, rightImg, [&](asw_ctx* c, asw_image* l, asw_image* r, asw_image* o) {
        return asw_aggregate_wmedian(c, l, r, o, (int)dispType, winSize, sampleRateS, sampleRateR, minDisparity, numDisparity, nullptr, 0);
    }, "computeAdaptiveWeight_WeightedMedian");
}
