/*
 * asw_mi355x.h -- C-ABI of the MI355X (gfx950) adaptive-support-weight stereo matcher.
 *
 * Drop-in boundary for the hot path of ZhangYY12345/aswStereoMatch: every entry point below
 * replaces one function of aswStereoMatch/methods/aswMethods.{h,cpp} ("M.h"/"M.cpp"); the
 * reference interface it stands in for is cited next to it.  Plain pointers and sizes only;
 * no C++ / torch / OpenCV types cross this boundary.  INTEGRATION.md shows the cv::Mat shim a
 * maintainer of the reference would add on top (and the ctypes binding the tests use).
 *
 * Conventions
 *  - images are what cv::Mat holds: row-major, interleaved channels, `step` bytes per row;
 *  - cost volumes are d-major [d][y][x] and dense, plane k <-> disparity min_d + k, the same
 *    order as the reference's std::vector<cv::Mat>;
 *  - enum values equal the reference's (parametersStereo.h:4-24);
 *  - all host pointers are caller-owned; device scratch lives in the context and is reused;
 *  - every call is synchronous on return and returns an asw_status (never throws).
 */
#ifndef ASW_MI355X_H
#define ASW_MI355X_H

#include <stddef.h>
#include <stdint.h>

/* the library is built with -fvisibility=hidden: only the entry points below are exported */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (the reference has none: it returns silently / an empty Mat / throws) ---- */
typedef enum asw_status {
    ASW_OK = 0,
    ASW_ERR_SIZE_MISMATCH = 1,      /* M.cpp:217-220, 313-316, 430-433: silent return          */
    ASW_ERR_EVEN_WINDOW = 2,        /* M.cpp:654-657, 1440-1443, 2458-2462, 3238-3241: Mat()  */
    ASW_ERR_UNSUPPORTED_METHOD = 3, /* enum value 0 (BM); the CV_Error cases of SGBM / BM; unserved modes / prefilters */
    ASW_ERR_UNSUPPORTED_LAYOUT = 4, /* where the reference throws cv::Exception (SURVEY B-7)  */
    ASW_ERR_HIP = 5,                /* a HIP runtime call or kernel launch failed             */
    ASW_ERR_ALLOC = 6,
    ASW_ERR_BAD_ARGUMENT = 7,       /* null pointer, non-positive size, bad depth             */
    ASW_ERR_NO_FRAME = 8            /* resident API used before asw_upload_pair               */
} asw_status;

/* parametersStereo.h:4-8 */
enum { ASW_DISPARITY_LEFT = 0, ASW_DISPARITY_RIGHT = 1 };

/* Sub-pixel disparity (not in the reference): one of these flags OR-ed into the disparity_type of
 * asw_stereo_match, asw_match_resident, every asw_aggregate_* and asw_stereo_match_batch.  The low bit keeps its meaning and all
 * its statuses.  After the method's own winner-take-all every pixel whose winner k = d - min_d has two neighbours in the
 * aggregated volume V (0 < k < asw_volume_planes() - 1), all three costs finite, cm = V[k-1] >= c0 = V[k] <= cp = V[k+1] and
 * den > 0 becomes (float)((double)d + clamp((cm - cp) / (2 * den), -0.5, 0.5)), all in f64, one IEEE operation each:
 *   PARABOLA     den = (cm - c0) + (cp - c0)
 *   EQUIANGULAR  den = max(cm, cp) - c0
 * Every other pixel keeps d.  The map becomes the call's / the slot's disparity (asw_download_disparity, asw_download_disparity_u8);
 * the volume a flagged call returns is the unflagged one, and without keep_volume / cost_volume_out none is kept.
 * Both flags, or a flag with any other bit beside bit 0: ASW_ERR_BAD_ARGUMENT, before the method's own checks (a value with
 * neither flag is refused by the method as before).  ASW_ALG_NCC (and asw_ncc_disparity) with a flag: ASW_ERR_UNSUPPORTED_METHOD;
 * ASW_ALG_BM: ASW_ERR_UNSUPPORTED_METHOD as without; ASW_ALG_SGBM ignores disparity_type altogether.  The cost builders, asw_wta
 * and the refined calls do not take the flags.  asw_get_timing: the extra kernel counts in total_ms and cost_ms. */
enum { ASW_DISPARITY_SUBPIXEL_PARABOLA = 0x100, ASW_DISPARITY_SUBPIXEL_EQUIANGULAR = 0x200 };

/* Confidence (not in the reference): a `disp` image with 2 channels (ASW_32F, step >= cols * 8; the cv::Mat
 * idiom CV_32FC2) passed to asw_stereo_match, to any asw_aggregate_* or to asw_download_disparity receives the disparity in channel
 * 0 and a confidence in channel 1, interleaved.  Channel 0 and the returned volume are those of the same call with a 1-channel
 * image.  The confidence is a function of the volume alone: for every pixel let V[k], k = 0 .. n - 1 (n = asw_volume_planes()), be
 * the volume the same call returns in cost_volume_out -- the combined volume under the cross-scale flag, the optimised volume under
 * the scanline flag, the unflagged volume under a sub-pixel flag, the method's volume otherwise.  Then
 *   F = { k : V[k] finite };  F empty: conf = 0;
 *   c1 = min over F, k1 = the smallest k with V[k] == c1 (strict '<' in ascending k), cmax = max over F;
 *   G = { k in F : |k - k1| >= 2 } -- the winner's two neighbours are left out: a true minimum between two samples makes them
 *     nearly equal;  G empty, cmax == c1 or c2 == c1: conf = 0;
 *   c2 = min over G;  conf = (float)(((double)c2 - (double)c1) / ((double)cmax - (double)c1)), one IEEE f64 operation each.
 * The winner's margin over the best candidate that is not its neighbour, in units of the column's range: it lies in [0, 1], is
 * never -0 and never NaN, and does not change when the volume is scaled by a power of two.  Thresholding is the caller's.
 * Statuses, after those of the two packed words and before any work: ASW_ALG_SGBM, ASW_ALG_BM, a value outside the selector,
 * ASW_ALG_NCC and asw_ncc_disparity give ASW_ERR_UNSUPPORTED_METHOD; everything a 1-channel call refuses is refused with the same
 * status.  asw_match_resident takes no such request: asw_download_disparity with a 2-channel image computes the confidence from
 * the volume the slot kept (keep_volume != 0) and returns ASW_ERR_NO_FRAME without one (keep_volume == 0, or after
 * asw_match_refined_resident), as asw_download_volume does.  asw_stereo_match_batch, the refined calls, asw_sgbm and the block
 * matchers refuse a 2-channel image as before (ASW_ERR_BAD_ARGUMENT / their own status).  asw_get_timing: the extra kernel of a
 * 2-channel asw_stereo_match / asw_aggregate_* call counts in total_ms and cost_ms.  A 1-channel call allocates and launches
 * nothing new. */

/* Cross-scale cost aggregation (Zhang et al., CVPR 2014; not in the reference): asw_disparity_cross_scale(S, q)
 * OR-ed into the disparity_type of asw_stereo_match, asw_match_resident, every asw_aggregate_* and asw_stereo_match_batch.  The method
 * (same window, same parameters) aggregates on S levels of a 2x2-mean pyramid of the pair; the regularised finest-scale volume is
 * the closed-form combination of the levels' volumes, and the map is its winner.  Bit 12 = the flag, bits 13-15 = S (2..5), bits
 * 16-23 = q (1..255, lambda = q / 64); bits 0, 8 and 9 keep their meaning; every other bit must be 0.  Defaults everywhere: S = 3,
 * q = 19.  All integer / IEEE, one operation each:
 *   pyramid: level s+1 has ceil(h/2) x ceil(w/2) pixels, per channel (a + b + c + d + 2) >> 2 of the level-s pixels at
 *     (min(2Y+j, h-1), min(2X+i, w-1)), i, j in {0, 1};
 *   range: n = asw_volume_planes() at level 0; level s runs min_d_s = min_d >> s and planes_s = ((min_d + n - 1) >> s) - min_d_s + 1
 *     planes, i.e. num_d_s = planes_s - (n - num_d); a level with num_d_s < 1 refuses the call;
 *   weights: A = tridiag(-lambda; 1+lambda, 1+2 lambda, .., 1+lambda; -lambda) (S x S), w = A^-1 e_0 by the Thomas algorithm in
 *     f64, each w_s rounded to f32;
 *   combine: acc = 0.0 (f64); s = 0..S-1 in order: acc += (double)w_s * (double)V_s[((min_d + k) >> s) - min_d_s][y >> s][x >> s];
 *     out[k][y][x] = (float)acc; map = winner of out, strict '<' in ascending k, NaN never wins, min_d + k.
 * The volume a flagged call returns is `out`; a sub-pixel flag in the same value refines the map on `out`.  With bit 12 set:
 * S outside 2..5, q = 0, any other bit, both sub-pixel flags or a level with num_d_s < 1 give ASW_ERR_BAD_ARGUMENT before any work;
 * ASW_ALG_NCC (and asw_ncc_disparity) ASW_ERR_UNSUPPORTED_METHOD; ASW_ALG_SGBM ignores the bits as it ignores disparity_type; what
 * the method's runner refuses at any level is the call's status.  With bit 12 clear nothing changes.  asw_get_timing: aggregate_ms /
 * aggregate_launches are those of the finest level, total_ms covers the whole call.  The refined calls do not take the flag. */
enum { ASW_DISPARITY_CROSS_SCALE = 0x1000 };
static inline int asw_disparity_cross_scale(int scales, int lambda_q)
{
    const int bad = scales < 2 || scales > 5 || lambda_q < 1 || lambda_q > 255;
    return ASW_DISPARITY_CROSS_SCALE | ((bad ? 0 : scales) << 13) | ((lambda_q & 0xFF) << 16);
}

/* Scanline optimisation of the aggregated volume (Mei et al., ICCV Workshops 2011; not in the reference):
 * asw_disparity_scanline(p1_code, unit_code, p2_ratio) OR-ed into the disparity_type of asw_stereo_match, asw_match_resident, every
 * asw_aggregate_* and asw_stereo_match_batch.  The method's volume V (n = asw_volume_planes() planes) is regularised along four paths
 * and the map is the winner of the result.  Bit 24 = the flag, bits 1-7 = a (P1 code, 1..127), bits 25-27 = u (unit = 4^(u - 5),
 * 1/1024 .. 16), bits 28-30 = p2_ratio - 1 (p2_ratio 1..8); bits 0, 8 and 9 keep their meaning; every other bit, bit 31 included,
 * must be 0.  P1 = (float)(a * unit), P2 = (float)(p2_ratio * a * unit), both exact.  Defaults everywhere: a = 8, u = 5, ratio 4
 * (P1 = 8, P2 = 32); an argument out of range gives the flag alone (a = 0), which the library refuses.  All f32, one IEEE operation each:
 *   c = V where V is finite, else +inf (NaN, +inf and -inf alike);
 *   paths r in this order: LR (predecessor q = x-1), RL (x+1), TB (y-1), BT (y+1); minq = min over k of L_r(q,k);
 *   q outside the frame or minq == +inf (q has no finite candidate): L_r(p,k) = c(p,k); otherwise
 *     t0 = L_r(q,k); t1 = L_r(q,k-1) + P1 (absent for k = 0); t2 = L_r(q,k+1) + P1 (absent for k = n-1); t3 = minq + P2;
 *     m = min(t0, t1, t2, t3); L_r(p,k) = c(p,k) + (m - minq);
 *   S = ((L_LR + L_RL) + L_TB) + L_BT; out = V finite ? S : V; map = winner of out, strict '<' in ascending k, NaN and +inf never
 *   win, a pixel without a winner is 0, else min_d + k.
 * The volume a flagged call returns is `out`; a sub-pixel flag in the same value refines the map on `out`.  With bit 24 set, in
 * this order and before any work: bit 12 (cross-scale) as well ASW_ERR_BAD_ARGUMENT; any other bit, a = 0 or both sub-pixel flags
 * ASW_ERR_BAD_ARGUMENT; ASW_ALG_NCC (and asw_ncc_disparity), ASW_ALG_BM and values outside the selector ASW_ERR_UNSUPPORTED_METHOD;
 * more than 1025 planes ASW_ERR_BAD_ARGUMENT.  ASW_ALG_SGBM ignores the bits as it ignores disparity_type; what the method's runner
 * refuses is the call's status.  With bit 24 clear nothing changes.  asw_get_timing: the step counts in total_ms and cost_ms, like
 * the sub-pixel step.  The refined calls do not take the flag. */
enum { ASW_DISPARITY_SCANLINE = 0x01000000 };
static inline int asw_disparity_scanline(int p1_code, int unit_code, int p2_ratio)
{
    const int bad = p1_code < 1 || p1_code > 127 || unit_code < 0 || unit_code > 7 || p2_ratio < 1 || p2_ratio > 8;
    return bad ? ASW_DISPARITY_SCANLINE : ASW_DISPARITY_SCANLINE | (p1_code << 1) | (unit_code << 25) | ((p2_ratio - 1) << 28);
}

/* parametersStereo.h:10-24 (StereoMatchingAlgorithms) */
enum {
    ASW_ALG_BM = 0,
    ASW_ALG_SGBM = 1,
    ASW_ALG_ADAPTIVE_WEIGHT = 2,
    ASW_ALG_ADAPTIVE_WEIGHT_8DIRECT = 3,
    ASW_ALG_ADAPTIVE_WEIGHT_GEODESIC = 4,
    ASW_ALG_ADAPTIVE_WEIGHT_BILATERAL_GRID = 5,
    ASW_ALG_ADAPTIVE_WEIGHT_BLO1 = 6,
    ASW_ALG_ADAPTIVE_WEIGHT_GUIDED_FILTER = 7,
    ASW_ALG_ADAPTIVE_WEIGHT_GUIDED_FILTER_2 = 8,
    ASW_ALG_ADAPTIVE_WEIGHT_GUIDED_FILTER_3 = 9,
    ASW_ALG_ADAPTIVE_WEIGHT_MEDIAN = 10,
    ASW_ALG_NCC = 11,
    ASW_ALG_ADAPTIVE_WEIGHT_CROSS = 12 /* not in the reference: cross-based support regions, below */
};

/* ---- cross-based support-region aggregation (Zhang, Lu, Lafruit 2009; not in the reference) ----
 * Selector entry 12 of every call that takes `algorithm` (asw_stereo_match, asw_match_resident, asw_stereo_match_batch,
 * asw_match_refined_resident, asw_stereo_match_refined); both directions, 1- or 3-channel 8U pairs, the sub-pixel flags as for the
 * other methods.  I = the view image (left for DISPARITY_LEFT, right for DISPARITY_RIGHT), L = win_size / 2, all integer:
 *   e(x,y,d) = min(trunc, AD(x,y,d)), AD the u8 value asw_cost_ad returns for the same direction (borders included);
 *   arm a_u(p), u = left / right / up / down: the largest r in [0, L] with p + k u inside the image and
 *     max_c |I_c(p + k u) - I_c(p)| <= tau for every k = 1..r (against the anchor p);
 *   S(p,d) = sum over y' = y - up(p) .. y + down(p) of sum over x' = x - left(x,y') .. x + right(x,y') of e(x',y',d), N(p) the same
 *     sum of 1 (<= 35 * 35; S < 2^24);
 *   volume E = (float)S / (float)N, one correctly rounded division, [num_d][rows][cols]; map: strict '<' in ascending d, min_d + index.
 * win_size odd in 1..35 (even: ASW_ERR_EVEN_WINDOW, above 35: ASW_ERR_BAD_ARGUMENT); rows * cols < 2^31 and rows <= 262140 (the sums the kernels keep are
 * local to a tile and cannot leave int32).  The plain value 12 runs tau = 20, trunc = 20; asw_alg_cross(tau, trunc) forms a value of
 * `algorithm` that carries other parameters: bits 0-7 = 12, bits 8-15 = tau (0..255), bits 16-23 = trunc (1..255), bit 30 set
 * (ASW_ALG_CROSS_PARAMS), bits 24-29 and 31 clear.  With bit 30 set a low byte other than 12 gives ASW_ERR_UNSUPPORTED_METHOD, and
 * trunc = 0 or any of bits 24-29 / 31 gives ASW_ERR_BAD_ARGUMENT (asw_alg_cross sets bit 24 for an argument out of range);
 * asw_volume_planes is num_disparity for 12 and every valid encoded value, 0 for the invalid ones.  asw_get_timing: aggregate_ms /
 * aggregate_launches cover the arm, region-size and aggregation kernels, cost_ms the rest.  asw_aggregate_cross (an inline function,
 * after asw_stereo_match below) is the per-method form; neither is a symbol of the library. */
enum { ASW_ALG_CROSS_PARAMS = 0x40000000 };
static inline int asw_alg_cross(int tau, int trunc)
{
    const int bad = (tau < 0 || tau > 255 || trunc < 1 || trunc > 255) ? 0x01000000 : 0;
    return ASW_ALG_CROSS_PARAMS | bad | ((trunc & 0xFF) << 16) | ((tau & 0xFF) << 8) | ASW_ALG_ADAPTIVE_WEIGHT_CROSS;
}

/* ---- AD-Census matching (Mei et al. 2011; census of Zabih & Woodfill 1994; not in the reference) ----
 * Selector entry 12 with another raw cost: everything said above holds with e replaced by the AD-Census cost and trunc = 255
 * (a no-op on it).  A = the view image, B = the other one, s = -1 (LEFT) / +1 (RIGHT), off = min_d + plane index, all integer:
 *   gray: a 3-channel image through the context's cvtColor(BGR2GRAY) (asw_set_gray_bits), a 1-channel image as it is;
 *   census code of a gray pixel G(y,x): 62 bits, one per (dy, dx), dy in -3..3, dx in -4..4, (0,0) excluded, set exactly when
 *     G(clamp(y+dy), clamp(x+dx)) < G(y,x) (clamped at the image border; a flat neighbourhood gives 0);
 *   ham(y,x,off) = popcount(codeA(y,x) ^ codeB(y, reflect(x + s off))), 0..62, reflect the BORDER_REFLECT rule of asw_cost_ad;
 *   ad(y,x,off) = the u8 value asw_cost_ad gives for the same pair, direction and plane;
 *   e = TA[ad] + TC[ham] (0..254), TA[v] = floor(127 (1 - exp(-v / lambda_ad)) + 0.5), TC[h] the same with lambda_census (double).
 * asw_alg_adcensus(tau, lambda_ad, lambda_census) forms the value of `algorithm`: bits 0-7 = 12, bits 8-15 = tau (0..255), bits 16-23 =
 * lambda_census (1..255), bits 24-28 = lambda_ad (1..31), bit 29 set (ASW_ALG_ADCENSUS_PARAMS), bits 30 and 31 clear; an argument out of
 * range gives lambda_ad field 0.  A value with bit 30 set is an asw_alg_cross() value whatever bit 29 holds; otherwise, with bit 29
 * set, a low byte other than 12 gives ASW_ERR_UNSUPPORTED_METHOD and bit 31, lambda_ad field 0 or lambda_census field 0
 * ASW_ERR_BAD_ARGUMENT.  asw_volume_planes is num_disparity for every valid value and 0 for the invalid ones.  Defaults everywhere:
 * tau 20, lambda_ad 10, lambda_census 30.  The cost kernel stages a row pair in LDS: cols <= 7432 (3 channels) / 9084 (1 channel),
 * else ASW_ERR_BAD_ARGUMENT.  asw_get_timing: the gray, census and cost kernels count in cost_ms; aggregate_ms / aggregate_launches are
 * those of entry 12.  asw_aggregate_adcensus (inline, after asw_stereo_match below) is the per-method form. */
enum { ASW_ALG_ADCENSUS_PARAMS = 0x20000000 };
static inline int asw_alg_adcensus(int tau, int lambda_ad, int lambda_census)
{
    const int bad = tau < 0 || tau > 255 || lambda_ad < 1 || lambda_ad > 31 || lambda_census < 1 || lambda_census > 255;
    return ASW_ALG_ADCENSUS_PARAMS | ((bad ? 0 : lambda_ad) << 24) | ((lambda_census & 0xFF) << 16) | ((tau & 0xFF) << 8) |
           ASW_ALG_ADAPTIVE_WEIGHT_CROSS;
}

/* ---- two-pass (separable) adaptive-support-weight aggregation (Wang et al. 2006; not in the reference) ----
 * Selector entry 2 with the support weight w(p, q) replaced by w(p, p') w(p', q), p' the pixel in p's row and q's column: a vertical
 * 1-D weighted pass, then a horizontal one over its sums -- 2 win taps per (pixel, candidate) instead of win^2 - 1.  Every call that
 * takes `algorithm` serves it; both directions, 1- or 3-channel 8U pairs (3 channels through the context's cvtColor(BGR2GRAY),
 * asw_set_gray_bits; 1 channel as it is), the sub-pixel flags as for the other methods; candidates min_d .. min_d + num_d inclusive
 * (asw_volume_planes = num_d + 1, as for the plain value 2).  gL / gR the gray pair, h = win_size / 2, clamp to the image:
 *   T[r][dc] = (float)exp(-((double)dc / gamma_c + (double)r / gamma_g)), r = 0..h, dc = 0..255 (libm, double); the centre tap counts;
 *   DISPARITY_LEFT, xr = max(0, x - d):
 *   vertical, j = -h..h ascending, yy = clamp(y + j): ab = T[|j|][|gL(yy,x) - gL(y,x)|] * T[|j|][|gR(yy,xr) - gR(y,xr)|] (f32);
 *     vn += (double)ab * |gL(yy,x) - gR(yy,xr)|, vd += (double)ab (f64);
 *   horizontal, i = -h..h ascending, xx = clamp(x + i), xri = clamp(xr + i):
 *     ab = T[|i|][|gL(y,xx) - gL(y,x)|] * T[|i|][|gR(y,xri) - gR(y,xr)|] (f32);
 *     num = num + (double)ab * vn(xx,y,d), den = den + (double)ab * vd(xx,y,d) (f64, each product rounded before it is added);
 *   E = num / den (f64); volume plane (float)E; map: strict '<' of E in ascending d, min_d + index.
 *   DISPARITY_RIGHT: DISPARITY_LEFT of the x-mirrored, swapped pair, mirrored back.
 * asw_alg_twopass(gamma_c, gamma_g) forms the value of `algorithm`: bits 0-7 = 2, bits 8-15 = gamma_c (1..255), bits 16-23 = gamma_g
 * (1..255), bit 28 set (ASW_ALG_TWOPASS_PARAMS), bits 24-27 and 29-31 clear; an argument out of range gives that gamma's field 0.  A
 * value with bit 29 or 30 set is read as above (bit 28 belongs to lambda_ad there); otherwise, with bit 28 set, a low byte other than
 * 2 gives ASW_ERR_UNSUPPORTED_METHOD and a gamma field 0 or any of bits 24-27 / 31 ASW_ERR_BAD_ARGUMENT (asw_volume_planes: 0).
 * win_size odd (even: ASW_ERR_EVEN_WINDOW) in 1..95 (above: ASW_ERR_BAD_ARGUMENT, before anything is allocated); rows * cols < 2^31
 * and rows <= 262140.  asw_get_timing: aggregate_ms covers the one kernel (aggregate_launches = 1), cost_ms the gray conversion.
 * asw_aggregate_twopass (inline, after asw_stereo_match below) is the per-method form; neither is a symbol of the library. */
enum { ASW_ALG_TWOPASS_PARAMS = 0x10000000 };
static inline int asw_alg_twopass(int gamma_c, int gamma_g)
{
    const int c = (gamma_c < 1 || gamma_c > 255) ? 0 : gamma_c, g = (gamma_g < 1 || gamma_g > 255) ? 0 : gamma_g;
    return ASW_ALG_TWOPASS_PARAMS | (g << 16) | (c << 8) | ASW_ALG_ADAPTIVE_WEIGHT;
}

/* ---- recursive (information-permeability) aggregation over the whole image (Cigla & Alatan 2013; not in the reference; DESIGN.md
 * section 4.17) ----
 * Selector entry 12 with the cross-shaped region replaced by a support that is the whole image: a cost travels from pixel to
 * neighbouring pixel, damped by exp(-colour step / sigma); two horizontal and two vertical scans, about four multiply-adds per
 * (pixel, candidate) whatever the object size.  Every call that takes `algorithm` serves it; both directions, 1- or 3-channel 8U
 * pairs, the sub-pixel flags as for the other methods; planes d = min_d .. min_d + num_d - 1 (asw_volume_planes = num_d, as for 12).
 * I = the view image (left for DISPARITY_LEFT, right for DISPARITY_RIGHT):
 *   e(x,y,d) = min(trunc, AD(x,y,d)), AD the u8 value asw_cost_ad returns for the same pair, direction and plane (borders included);
 *   P[k] = (double)(float)exp(-(double)k / sigma), k = 0..255 (libm, built on the host, handed to the device as doubles); entries with
 *     k > 103.28 sigma are exactly 0 and act as hard barriers;
 *   ph(x,y) = P[max_c |I_c(x,y) - I_c(x-1,y)|] for x >= 1, pv(x,y) = P[max_c |I_c(x,y) - I_c(x,y-1)|] for y >= 1;
 *   horizontal pass, per row and plane, f64, every product rounded before it is added (no contraction):
 *     LR(0) = e(0), LR(x) = e(x) + ph(x) LR(x-1), ascending x;  RL(W-1) = e(W-1), RL(x) = e(x) + ph(x+1) RL(x+1), descending x;
 *     Hs(x) = (LR(x) + RL(x)) - e(x), in that order;
 *   vertical pass: the same three statements down and up every column, with Hs in place of e and pv in place of ph -> S(x,y,d);
 *   N(x,y) = the same two passes over e == 1 (independent of d, >= 1: no plane holds a NaN); E = S / N (f64, correctly rounded);
 *   volume plane (float)E; map: min_d + index of the strict-'<' running minimum of the f64 E over ascending d.
 * The scans are sequential by definition: a parallel-prefix form rounds differently and is not this method.
 * asw_alg_permeability(sigma, trunc) forms the value of `algorithm`: bits 0-7 = 12, bits 8-15 = sigma (1..255), bits 16-23 = trunc
 * (1..255), bit 27 set (ASW_ALG_PERMEABILITY_PARAMS), bits 24-26 and 28-31 clear; an argument out of range leaves 0 in its field.  Bit
 * 27 is read only when bits 28, 29 and 30 are clear (it belongs to lambda_ad under bit 29 and is a refused bit under bits 28 and 30);
 * then a low byte other than 12 gives ASW_ERR_UNSUPPORTED_METHOD and a zero field or any of bits 24-26 / 31 ASW_ERR_BAD_ARGUMENT
 * (asw_volume_planes: 0).  The method has no window: win_size is not read, every value of it -- even, zero or negative -- gives the
 * same result and status.  rows * cols < 2^31 and the column limits of asw_cost_ad, as for 12; the scan kernels have no limit of their
 * own on rows or columns.  Candidates go through the device in chunks that keep the method's scratch within 2 GiB beside the u8 cost
 * volume; the result does not depend on the chunking.  asw_get_timing: the AD cost build counts in cost_ms; aggregate_ms /
 * aggregate_launches cover the two permeability planes, N's two scans and two scans per chunk: aggregate_launches = 4 + 2 * chunks.
 * asw_aggregate_permeability (inline, after asw_stereo_match below) is the per-method form; neither is a symbol of the library. */
enum { ASW_ALG_PERMEABILITY_PARAMS = 0x08000000 };
static inline int asw_alg_permeability(int sigma, int trunc)
{
    const int s = (sigma < 1 || sigma > 255) ? 0 : sigma, t = (trunc < 1 || trunc > 255) ? 0 : trunc;
    return ASW_ALG_PERMEABILITY_PARAMS | (t << 16) | (s << 8) | ASW_ALG_ADAPTIVE_WEIGHT_CROSS;
}

/* cv::Mat depth codes */
enum { ASW_8U = 0, ASW_16S = 3, ASW_32F = 5 };

/* The part of a cv::Mat header the path needs (M.h:91: cv::Mat srcLeft, srcRight, disparityMap) */
typedef struct asw_image {
    void* data;   /* host pointer                               */
    int rows;     /* cv::Mat::rows                              */
    int cols;     /* cv::Mat::cols                              */
    int channels; /* cv::Mat::channels()                        */
    int depth;    /* ASW_8U, ASW_16S or ASW_32F                 */
    size_t step;  /* bytes per row (cv::Mat::step), >= cols*channels*elemsize */
} asw_image;

typedef struct asw_ctx asw_ctx; /* one per device; not shared between threads */

/* Per-call timing of the kernels of the last asw_match_resident / asw_stereo_match call,
 * measured with HIP events on the context's stream. */
typedef struct asw_timing {
    float total_ms;      /* all kernels of the call                                  */
    float aggregate_ms;  /* the dominant aggregation kernel(s) (ASW / guided / median) */
    float cost_ms;       /* cost-build kernels (gray, Scharr, min/max, ...)           */
    int aggregate_launches;
} asw_timing;

/* ---- context ---- */
int asw_create(int device_id, asw_ctx** out);
void asw_destroy(asw_ctx* ctx);
const char* asw_status_string(int status);
int asw_device_count(void);
/* cvtColor(COLOR_BGR2GRAY) on 8U is fixed-point in OpenCV and its constants changed between releases: 14 bits
 * {B 1868, G 9617, R 4899} in 4.1.0 -- the version the reference pins (aswStereoMatch.vcxproj:67,71), the default here --
 * and 15 bits {3735, 19235, 9798} in later 4.x releases; the two differ by +-1 on a few percent of the pixels.  A maintainer
 * who links the reference against a newer OpenCV selects 15 to keep bit-identical gray planes (classic, direct8, SAD, BLO1,
 * bilateral grid, NCC all start from them; M.cpp:1031-1033, 2448-2454, 835-840).  bits: 14 or 15. */
int asw_set_gray_bits(asw_ctx* ctx, int bits);

/* ---- whole-method entry point: stereoMatching(), M.h:91-92, M.cpp:46-88 ----
 * disp: ASW_32F, 1 channel, rows x cols, caller-allocated; receives ABSOLUTE disparity
 * (min_d + index), like the reference's CV_32FC1 result; with 2 channels also the confidence ("Confidence" above).  Per-method literals are the
 * selector's (gamma_c=30, gamma_g=20; eps=1e-6; rateS=rateR=10).
 * cost_volume_out (optional, may be NULL): aggregated cost volume, [n][rows][cols] f32 with
 * n = asw_volume_planes(algorithm, num_d): num_d, or num_d + 1 for ADAPTIVE_WEIGHT, 8DIRECT, GEODESIC and BILATERAL_GRID, whose
 * candidate range is inclusive (M.cpp:1021,1074; 1171; 1447,1467; 2256,2280).
 * cost_volume_floats: capacity of cost_volume_out in floats (ignored when it is NULL); a buffer shorter than
 * n * rows * cols is refused with ASW_ERR_BAD_ARGUMENT before anything is computed or written.  The same pair of
 * arguments ends every asw_aggregate_* entry point below.
 * These host-buffer entry points work on a private frame of the context: they never disturb the resident slots of
 * asw_upload_pair / asw_match_resident. */
int asw_stereo_match(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp,
                     int disparity_type, int algorithm, int win_size, int min_disparity, int num_disparity,
                     float* cost_volume_out, size_t cost_volume_floats);

/* Cross-based support regions with explicit parameters (above): asw_stereo_match with algorithm = asw_alg_cross(tau, trunc). */
static inline int asw_aggregate_cross(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp, int disparity_type,
                                      int tau, int trunc, int win_size, int min_disparity, int num_disparity, float* cost_volume_out,
                                      size_t cost_volume_floats)
{
    return asw_stereo_match(ctx, left, right, disp, disparity_type, asw_alg_cross(tau, trunc), win_size, min_disparity, num_disparity,
                            cost_volume_out, cost_volume_floats);
}

/* AD-Census matching with explicit parameters (above): asw_stereo_match with algorithm = asw_alg_adcensus(tau, lambda_ad, lambda_census). */
static inline int asw_aggregate_adcensus(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp, int disparity_type,
                                         int tau, int lambda_ad, int lambda_census, int win_size, int min_disparity, int num_disparity,
                                         float* cost_volume_out, size_t cost_volume_floats)
{
    return asw_stereo_match(ctx, left, right, disp, disparity_type, asw_alg_adcensus(tau, lambda_ad, lambda_census), win_size,
                            min_disparity, num_disparity, cost_volume_out, cost_volume_floats);
}

/* Two-pass ASW with explicit parameters (above): asw_stereo_match with algorithm = asw_alg_twopass(gamma_c, gamma_g). */
static inline int asw_aggregate_twopass(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp, int gamma_c,
                                        int gamma_g, int disparity_type, int win_size, int min_disparity, int num_disparity,
                                        float* cost_volume_out, size_t cost_volume_floats)
{
    return asw_stereo_match(ctx, left, right, disp, disparity_type, asw_alg_twopass(gamma_c, gamma_g), win_size, min_disparity,
                            num_disparity, cost_volume_out, cost_volume_floats);
}

/* Permeability aggregation with explicit parameters (above): asw_stereo_match with algorithm = asw_alg_permeability(sigma, trunc); the
 * method has no window, win_size is passed as 0. */
static inline int asw_aggregate_permeability(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp,
                                             int disparity_type, int sigma, int trunc, int min_disparity, int num_disparity,
                                             float* cost_volume_out, size_t cost_volume_floats)
{
    return asw_stereo_match(ctx, left, right, disp, disparity_type, asw_alg_permeability(sigma, trunc), 0, min_disparity, num_disparity,
                            cost_volume_out, cost_volume_floats);
}

/* Planes of the cost volume `algorithm` produces for num_disparity candidates (what cost_volume_out must hold);
 * 0 for an algorithm without a selector volume: BM (not served) and SGBM (a non-NULL cost_volume_out is refused with
 * ASW_ERR_BAD_ARGUMENT; asw_sgbm returns its aggregated cost). */
int asw_volume_planes(int algorithm, int num_disparity);

/* ---- the same, split so that inputs can stay resident in HBM (bench / pipelines) ----
 * Slots are caller-numbered (0..4095).  asw_upload_pair / asw_preprocess_pair replace a slot's pair and drop its previous
 * disparity and volume; asw_download_* return ASW_ERR_NO_FRAME until asw_match_resident has succeeded on the CURRENT
 * pair of the slot (a failed match drops the results too). */
int asw_upload_pair(asw_ctx* ctx, int slot, const asw_image* left, const asw_image* right);
int asw_match_resident(asw_ctx* ctx, int slot, int disparity_type, int algorithm, int win_size,
                       int min_disparity, int num_disparity, int keep_volume);
int asw_download_disparity(asw_ctx* ctx, int slot, asw_image* disp);
int asw_download_volume(asw_ctx* ctx, int slot, float* cost_volume_out, size_t n_floats);
int asw_synchronize(asw_ctx* ctx);
int asw_get_timing(asw_ctx* ctx, asw_timing* out);

/* ---- driver-side pre/post-processing on the device (aswStereoMatch.cpp, "main.cpp") ----
 * asw_preprocess_pair: main.cpp:30-31 resize(img, Size(out_width, out_height)) (INTER_LINEAR) and, if detail_boost != 0,
 * main.cpp:67-89 (BGR2HSV, V += 2*(V - bilateralFilter(V, 7, 10, 3, BORDER_REFLECT)), HSV2BGR) for both 8UC3 images; the
 * result becomes the resident pair of `slot` (as after asw_upload_pair).  asw_download_pair fetches it.
 * asw_download_disparity_u8: main.cpp:97-98 disparityMap.convertTo(CV_8UC1) and, if normalize != 0,
 * normalize(.., 0, 255, NORM_MINMAX) of the last asw_match_resident result of `slot`; disp_u8: ASW_8U, 1 channel. */
int asw_preprocess_pair(asw_ctx* ctx, int slot, const asw_image* left_full, const asw_image* right_full, int out_width,
                        int out_height, int detail_boost);
int asw_download_pair(asw_ctx* ctx, int slot, asw_image* left, asw_image* right);
int asw_download_disparity_u8(asw_ctx* ctx, int slot, asw_image* disp_u8, int normalize);

/* ---- served windows ----
 * win_size from 1 up to the value below, odd unless stated; the same range holds through asw_stereo_match, asw_match_resident,
 * asw_stereo_match_batch and the refined entry points.  Order of the checks: an even window gives ASW_ERR_EVEN_WINDOW (the
 * reference's empty Mat) whatever its size, an odd window past the range gives ASW_ERR_BAD_ARGUMENT before anything is allocated
 * or launched, and the context serves the next call as if the refused one had not been made.  Each limit is the limit of the kernel
 * launcher itself (what fits a workgroup's LDS, or a walk's strip); tests/test_gpu_large_windows.py runs every entry at its last
 * window and at the first refused one.
 *   asw_aggregate_bilateral, asw_aggregate_direct8 (enum 2, 3)   63   the tile's LDS layout: 160160 of 163840 bytes
 *   asw_ncc_disparity (enum 11), asw_cost_ncc                    59   two f32 tiles in 64 KB of LDS
 *   asw_aggregate_guided (enum 7)                                63   box side of the sliding walk <= 64
 *   asw_aggregate_guided2 (enum 8)                               64   the same; the window is the box side as it stands, even or odd
 *   asw_aggregate_guided3 (enum 9)                               59   the smaller of the walk's limit and NCC's
 *   asw_guided_filter                                         r <= 64   even or odd
 *   asw_cost_sad, asw_cost_sad_d                                 63   box side of the walk
 *   asw_aggregate_blo1 (enum 6)                                  63   its SAD cost comes from the walk (the kernel's own LDS: 133)
 *   asw_aggregate_wmedian (enum 10)                              45   2048 slots of the per-pixel sort
 *   asw_aggregate_geodesic (enum 4), asw_geodesic_dist           35   instantiated window sizes
 *   cross-based aggregation, AD-Census (enum 12), refinement     35   see above and below
 * asw_aggregate_bilgrid takes no window. */

/* ---- per-method entry points with explicit parameters (M.h:133-184) ---- */
/* computeAdaptiveWeight, M.h:133-134, M.cpp:1016-1156 */
int asw_aggregate_bilateral(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp,
                            double gamma_c, double gamma_g, int disparity_type, int win_size,
                            int min_disparity, int num_disparity, float* cost_volume_out, size_t cost_volume_floats);
/* computeAdaptiveWeight_direct8, M.h:135-136, M.cpp:1167-1319: the classic scheme on row + column + main diagonal of the
 * window, gamma_c = 30, gamma_g = win*2/3 (integer division).  DISPARITY_LEFT only: the reference's RIGHT branch indexes
 * its weight vectors with a negative tap coordinate (M.cpp:1291-1295) -> ASW_ERR_UNSUPPORTED_LAYOUT. */
int asw_aggregate_direct8(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp,
                          int disparity_type, int win_size, int min_disparity, int num_disparity,
                          float* cost_volume_out, size_t cost_volume_floats);
/* computeAdaptiveWeight_geodesic, M.h:142-143, M.cpp:1436-1534 */
int asw_aggregate_geodesic(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp,
                           int disparity_type, int win_size, int min_disparity, int num_disparity,
                           float* cost_volume_out, size_t cost_volume_floats);
/* computeAdaptiveWeight_GuidedF, M.h:166-168, M.cpp:2867-2963 */
int asw_aggregate_guided(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp,
                         int disparity_type, double eps, int win_size, int min_disparity, int num_disparity,
                         float* cost_volume_out, size_t cost_volume_floats);
/* computeAdaptiveWeight_GuidedF_2, M.h:169-171, M.cpp:2976-3050 */
int asw_aggregate_guided2(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp,
                          int disparity_type, double eps, int win_size, int min_disparity, int num_disparity,
                          float* cost_volume_out, size_t cost_volume_floats);
/* computeAdaptiveWeight_GuidedF_3, M.h:172-174, M.cpp:3063-3137: normalised NCC planes (computeNCC, M.cpp:924-1013) filtered
 * with the 6-channel guide [L, R shifted by d] (LEFT) or with the plain right image (RIGHT, M.cpp:3110) */
int asw_aggregate_guided3(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp,
                          int disparity_type, double eps, int win_size, int min_disparity, int num_disparity,
                          float* cost_volume_out, size_t cost_volume_floats);
/* computeAdaptiveWeight_BLO1, M.h:157-159, M.cpp:2505-2725 (min_disparity must be 0: the reference indexes its
 * per-key slices with the absolute offset) */
int asw_aggregate_blo1(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp,
                       int disparity_type, double sample_rate_r, int win_size, int min_disparity, int num_disparity,
                       float* cost_volume_out, size_t cost_volume_floats);
/* computeAdaptiveWeight_bilateralGrid, M.h:155-157, M.cpp:2253-2430 (grid: createBilGrid M.cpp:1831-2185, enum 5 calls it with
 * rates 10, 10): offsets min_d .. min_d+num_d inclusive, cost volume num_d+1 planes (NaN / inf where the interpolated count is 0).
 * DISPARITY_LEFT only -- the reference's RIGHT branch reads one column past the row (M.cpp:1929, 2356).
 * sample_rate_r >= 2.55 (at most 101 bins per range axis). */
int asw_aggregate_bilgrid(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp,
                          int disparity_type, double sample_rate_s, double sample_rate_r, int min_disparity,
                          int num_disparity, float* cost_volume_out, size_t cost_volume_floats);
/* computeAdaptiveWeight_WeightedMedian, M.h:179-182, M.cpp:3228-3383 */
int asw_aggregate_wmedian(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp,
                          int disparity_type, int win_size, double rate_s, double rate_r, int min_disparity,
                          int num_disparity, float* cost_volume_out, size_t cost_volume_floats);

/* ---- cost builders (M.h:101-113, 156) : outputs are dense d-major volumes ---- */
/* computeAD, M.cpp:208-292: cost u8 [num_d][rows][cols]; 1- or 3-channel 8U input.  asw_cost_ad, asw_cost_tad and asw_cost_sd stage a
 * row pair in LDS (2 * cols * channels bytes of 160 KB): cols <= 27306 (3 channels) / 81920 (1 channel), else ASW_ERR_BAD_ARGUMENT;
 * the same holds for selector entry 12, whose raw cost this is. */
int asw_cost_ad(asw_ctx* ctx, const asw_image* left, const asw_image* right, uint8_t* cost,
                int disparity_type, int min_disparity, int num_disparity);
/* computeTAD, M.cpp:304-401: 0/255 mask of AD > threshold_T */
int asw_cost_tad(asw_ctx* ctx, const asw_image* left, const asw_image* right, uint8_t* cost,
                 int disparity_type, int threshold_t, int min_disparity, int num_disparity);
/* Census cost and AD-Census cost (not in the reference; "AD-Census matching" above), inline over asw_cost_tad so that the library's
 * exported set does not grow: a threshold_t from ASW_COST_CENSUS_PARAMS (bit 30) up, which as a TAD threshold could only give an
 * all-zero mask, selects them: bits 8-15 = lambda_ad, bits 0-7 = lambda_census, both 0 (Hamming alone) or both 1..255, bits 16-29
 * clear, else ASW_ERR_BAD_ARGUMENT.  Arguments and statuses otherwise as asw_cost_ad; cost u8 [num_d][rows][cols].
 * asw_cost_census: the Hamming distance ham (0..62) of the census codes of the gray pair; cols <= 10240.
 * asw_cost_adcensus: e = TA[ad] + TC[ham] (0..254); both lambdas in 1..255; cols <= 7432 (3 channels) / 9084 (1 channel). */
enum { ASW_COST_CENSUS_PARAMS = 0x40000000 };
static inline int asw_cost_census(asw_ctx* ctx, const asw_image* left, const asw_image* right, uint8_t* cost, int disparity_type,
                                  int min_disparity, int num_disparity)
{
    return asw_cost_tad(ctx, left, right, cost, disparity_type, ASW_COST_CENSUS_PARAMS, min_disparity, num_disparity);
}
static inline int asw_cost_adcensus(asw_ctx* ctx, const asw_image* left, const asw_image* right, uint8_t* cost, int disparity_type,
                                    int lambda_ad, int lambda_census, int min_disparity, int num_disparity)
{
    const int bad = (lambda_ad < 1 || lambda_ad > 255 || lambda_census < 1 || lambda_census > 255) ? 0x10000 : 0;
    return asw_cost_tad(ctx, left, right, cost, disparity_type,
                        ASW_COST_CENSUS_PARAMS | bad | ((lambda_ad & 0xFF) << 8) | (lambda_census & 0xFF), min_disparity, num_disparity);
}
/* computeSD, M.h:117-118, M.cpp:670-759: the AD value squared by a u8 Mat::mul, i.e. min(255, ad*ad) */
int asw_cost_sd(asw_ctx* ctx, const asw_image* left, const asw_image* right, uint8_t* cost,
                int disparity_type, int min_disparity, int num_disparity);
/* computeSimilarity (TAD C+G), M.cpp:415-636; win_size = 0 selects the unpadded overload,
 * win_size > 0 the padded one (M.cpp:651-668): planes are (rows+2h) x (cols+2h). */
int asw_cost_similarity(asw_ctx* ctx, const asw_image* left, const asw_image* right, float* cost,
                        double regularity, double thres_c, double thres_g, int disparity_type,
                        int win_size, int min_disparity, int num_disparity);
/* getCostSAD_d for every d as called from M.cpp:2884-2898: box mean of gray abs-diff */
int asw_cost_sad(asw_ctx* ctx, const asw_image* left, const asw_image* right, float* cost,
                 int disparity_type, int win_size, int min_disparity, int num_disparity);

/* getCostSAD_d itself, M.h:156, M.cpp:2442-2503: ONE disparity, and the image that is not the reference view arrives
 * already bordered by the caller (wider by the caller's max_offset; M.cpp:2877-2878, 2884-2898): DISPARITY_LEFT reads
 * right(Rect(right.cols - left.cols - disparity, 0, left.cols, rows)), DISPARITY_RIGHT reads left(Rect(disparity, 0,
 * right.cols, rows)).  1- or 3-channel 8U inputs (3: BGR2GRAY first).  cost: f32 rows x cols of the reference view.
 * ASW_ERR_SIZE_MISMATCH where the reference returns Mat() (bordered image not wider, M.cpp:2473-2476, 2488-2491),
 * ASW_ERR_BAD_ARGUMENT for a ROI outside the bordered image (cv::Exception in the reference). */
int asw_cost_sad_d(asw_ctx* ctx, const asw_image* left, const asw_image* right, float* cost, int disparity,
                   int disparity_type, int win_size);

/* computeNCC, volume overload, M.h:121-122, M.cpp:924-1013: cost = sum(l*r) / (sum(l*l)*sum(r*r)) on mean-removed windows of
 * the RGB2GRAY images; normalized != 0: every plane min-max normalised as the reference stores it, 0: the raw planes.
 * 1- or 3-channel 8U input. */
int asw_cost_ncc(asw_ctx* ctx, const asw_image* left, const asw_image* right, float* cost, int disparity_type,
                 int win_size, int min_disparity, int num_disparity, int normalized);
/* computeNCC, disparity overload, M.h:119-120, M.cpp:812-913 (enum NCC = 11): offsets min_d .. min_d+num_d-2, smallest cost
 * wins (LEFT); DISPARITY_RIGHT never writes a pixel in the reference -> all zeros here. */
int asw_ncc_disparity(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp, int disparity_type,
                      int win_size, int min_disparity, int num_disparity);

/* ---- building blocks that are public in the reference header ---- */
/* getGuidedFilter, M.h:165, M.cpp:2766-2854: guide 8U with 3 or 6 channels, p/q f32 rows x cols */
int asw_guided_filter(asw_ctx* ctx, const asw_image* guide, const float* p, float* q, int r, double eps);
/* getGeodesicDist, M.h:141, M.cpp:1392-1424: out f32 [rows][cols][win][win] */
int asw_geodesic_dist(asw_ctx* ctx, const asw_image* img, float* out, int win_size, int iter_time);
/* inline WTA of M.cpp:1144-1150 / 3032-3048 on a dense f32 volume [n][rows][cols] */
int asw_wta(asw_ctx* ctx, const float* cost_volume, int n, int rows, int cols, int min_disparity,
            float* disp);
/* Left-right consistency check, the consumer of the DISPARITY_RIGHT maps (M.cpp:1113-1142, 1498-1520, 2919-2935 produce them;
 * the reference itself never cross-checks, so the rule is this library's): out(y,x) = dl(y,x) if xr = x - (int)dl(y,x) lies in
 * [0, cols) and |dl(y,x) - dr(y,xr)| <= max_diff, else invalid_value.  n_invalid (optional) receives the number of rejected pixels. */
int asw_lr_check(asw_ctx* ctx, const float* disp_left, const float* disp_right, int rows, int cols, float max_diff,
                 float invalid_value, float* out, int* n_invalid);
/* ---- left-right refinement: cross-check, occlusion fill, weighted median (not in the reference) ----
 * The post-processing Hosni, Bleyer, Gelautz put behind every weight function: asw_lr_check's rule, then every rejected pixel takes
 * the lower of the nearest valid disparities to its left and right on its row (the one that exists at a border; a row without a
 * valid pixel is unfillable), then every FILLED pixel takes the weighted median of the filled map over a win_size x win_size window
 * (taps inside the image, unfillable taps cast no vote).  Weights are integers, w = Tc[sum over channels |G(p) - G(q)|] * Ts[|j|][|i|],
 * Tc[c] = floor(4096 * exp(-c / gamma_c) + 0.5), Ts[j][i] = floor(256 * exp(-sqrt(i*i + j*j) / gamma_s) + 0.5) (host, double, libm);
 * the median is the smallest v with 2 * (weight of the votes <= v) >= total weight.  All sums are exact in 32 bits.
 * asw_refine_disparity: guide ASW_8U with 1 or 3 channels (else ASW_ERR_UNSUPPORTED_LAYOUT), rows x cols (rows <= 262140, rows * cols
 * < 2^31); disp_left / disp_right / out: dense f32 rows x cols, absolute disparities.  Every disp_left value must be an integer in
 * [min_disparity, min_disparity + num_values) -- anything else, NaN and inf included, gives ASW_ERR_BAD_ARGUMENT with nothing
 * written to out / mask_out / the counts; disp_right may hold anything.  1 <= num_values <= 1025 (asw_volume_planes(algorithm,
 * num_disparity) for a selector method), |min_disparity| <= 2^20, max_diff >= 0, win_size odd in 1..35 (1: cross-check + fill only),
 * gamma_c > 0, gamma_s > 0; the Python / C++ wrappers default to gamma_c = 60, gamma_s = 9, win_size = 15.  out: disp_left where
 * valid, the median where filled, min_disparity - 1 where unfillable.  mask_out (optional): one byte per pixel, 0 valid, 1 filled,
 * 2 unfillable.  n_rejected (optional): pixels the cross-check rejected (= asw_lr_check's n_invalid); n_unfillable (optional).
 * asw_match_refined_resident: DISPARITY_LEFT and DISPARITY_RIGHT of `algorithm` on the resident pair of `slot`, both winner-take-all
 * maps kept in HBM, refined with the resident left image as guide (after asw_preprocess_pair: the processed one) and num_values =
 * asw_volume_planes(algorithm, num_disparity); the refined map becomes the slot's disparity (asw_download_disparity /
 * asw_download_disparity_u8 as after asw_match_resident; no volume is kept: asw_download_volume gives ASW_ERR_NO_FRAME).  A method
 * whose DISPARITY_RIGHT match is not served returns that match's status (ASW_ERR_UNSUPPORTED_LAYOUT for 8DIRECT, BILATERAL_GRID,
 * GUIDED_FILTER_2, MEDIAN) before anything is computed: the RIGHT match runs first.  num_disparity <= 0 or min_disparity < 0:
 * ASW_ERR_BAD_ARGUMENT, as for asw_match_resident; ASW_ALG_SGBM / ASW_ALG_BM: ASW_ERR_UNSUPPORTED_METHOD (they carry their own disp12MaxDiff).  A matcher's
 * map leaves the domain above only where the method writes a literal 0: ASW_ALG_NCC leaves unwritten pixels 0 and its DISPARITY_RIGHT
 * map is all zeros, so with min_disparity > 0 the refined NCC call returns ASW_ERR_BAD_ARGUMENT like the building block.  Any failure
 * drops the slot's results as a failed asw_match_resident does; the resident pair is never disturbed.
 * asw_get_timing afterwards: total_ms = the kernels of both matches + the refinement; aggregate_ms / aggregate_launches = the two
 * matches' aggregation kernels summed; cost_ms = total_ms - aggregate_ms (the cost builders of both matches + the refinement).
 * asw_stereo_match_refined: the same on host images, on the context's private frame like asw_stereo_match. */
int asw_refine_disparity(asw_ctx* ctx, const asw_image* guide, const float* disp_left, const float* disp_right,
                         int min_disparity, int num_values, float max_diff, int win_size, double gamma_c, double gamma_s,
                         float* out, uint8_t* mask_out, int* n_rejected, int* n_unfillable);
int asw_match_refined_resident(asw_ctx* ctx, int slot, int algorithm, int win_size, int min_disparity, int num_disparity,
                               float max_diff, int refine_win, double gamma_c, double gamma_s, int* n_rejected, int* n_unfillable);
int asw_stereo_match_refined(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp, int algorithm,
                             int win_size, int min_disparity, int num_disparity, float max_diff, int refine_win, double gamma_c,
                             double gamma_s, int* n_rejected, int* n_unfillable);
/* ---- Smoothing: confidence-weighted edge-aware smoothing of a disparity map (not in the reference) ----
 * The fast global smoother of Min, Choi, Lu, Ham, Sohn, Do ("Fast global image smoothing based on weighted least squares", TIP
 * 2014) applied the way OpenCV's DisparityWLSFilter applies it: the map times its confidence and the confidence itself are smoothed
 * along the guide's edges and divided, so unreliable pixels are pulled towards reliable neighbours of similar colour.  It takes ONE
 * match (the left-right refinement above takes two), serves every method that has a confidence, and returns a dense fractional map.
 * Inputs: guide G, ASW_8U, 1 or 3 channels, rows x cols, its step honoured; d: dense f32 map; c: dense f32 confidence (the second
 * channel of a 2-channel disparity image, or any trust value: a 0/1 validity mask is a legal confidence); sigma_c and lambda finite
 * and > 0; T iterations, 1..8.  All arithmetic is f64, one IEEE operation per written operation, in the written order, never
 * contracted; N and D stay f64 from step 2 to step 6:
 *   1. ce = (isfinite(d) && isfinite(c) && c > 0) ? (double)c : 0  (selects: a non-finite value never enters a product);
 *   2. N0 = ce > 0 ? ce * (double)d : 0,  D0 = ce: non-finite map values and non-positive confidences are holes;
 *   3. Wt[k] = floor(65536 * exp(-k / sigma_c) + 0.5) / 65536, k = 0 .. 255 * channels (host, double, libm; quantised like Tc above, so
 *      a last-bit difference between libms cannot move it);
 *   4. wh(y, x) = Wt[sum over channels |G(y,x) - G(y,x-1)|] for x >= 1, wv(y, x) the same with the pixel above for y >= 1;
 *   5. for t = 1..T: lam_t = (1.5 * lambda * (double)(1 << 2*(T-t))) / (double)((1 << 2*T) - 1); a pass over every row, then a pass
 *      over every column; a pass solves one tridiagonal system per line for the two right-hand sides N and D of the previous pass.
 *      For a line of length n with link weights w_1 .. w_{n-1} and right-hand side f:
 *        a_i = -(lam_t * w_i), a_0 = 0;  c_i = -(lam_t * w_{i+1}), c_{n-1} = 0;  b_i = (1.0 - a_i) - c_i;
 *        forward:  m_0 = b_0,  m_i = b_i - a_i * cp_{i-1};  r_i = 1.0 / m_i;  cp_i = c_i * r_i;
 *                  fp_0 = f_0 * r_0,  fp_i = (f_i - a_i * fp_{i-1}) * r_i   (one reciprocal per step, shared by N and D);
 *        backward: u_{n-1} = fp_{n-1},  u_i = fp_i - cp_i * u_{i+1};
 *      a line of length 1 returns its input;
 *   6. out = D_T > 0 ? (float)(N_T / D_T) : d, the input's bits unchanged (a frame, or a region cut off by zero weights, without a
 *      confident pixel).
 * The request travels in the refinement family's win_size / refine_win argument as a value no window can take, ASW_REFINE_SMOOTH | T;
 * under it gamma_c carries sigma_c, gamma_s carries lambda and disp_right the confidence plane; the library does not look at
 * min_disparity, num_values or max_diff, places no domain requirement on the map and writes neither count.  The three functions
 * below are inline functions of this header, not symbols of the library (the exported set stays as it is).  Every win_size /
 * refine_win without bit 30 behaves as described above.
 * asw_smooth_disparity: the checks, in this order: null pointers and the guide as an image, as asw_refine_disparity; rows <= 262140
 * and rows * cols < 2^31; the word (iterations outside 1..8 travel as the invalid word ASW_REFINE_SMOOTH | 0): ASW_ERR_BAD_ARGUMENT;
 * sigma_c / lambda not finite and > 0: ASW_ERR_BAD_ARGUMENT; guide channels not 1 or 3: ASW_ERR_UNSUPPORTED_LAYOUT.  (A caller of
 * asw_refine_disparity itself who passes a mask_out under the flag gets ASW_ERR_BAD_ARGUMENT in front of the channel check.)
 * Nothing of the caller's is written on a refusal.
 * asw_match_smoothed_resident: ONE DISPARITY_LEFT match of `algorithm` on the resident pair of `slot`, with its volume written and
 * the confidence of the 2-channel disparity image computed from it; then the integer winner-take-all map is smoothed with that
 * confidence and the resident left image as guide, and the result becomes the slot's disparity (no volume is kept, as after
 * asw_match_refined_resident).  The methods without a DISPARITY_RIGHT branch are served.  The smoothing's own checks (frame size,
 * word, sigma_c, lambda, channels, as above) come first, so that nothing is computed for a call they refuse; then the argument
 * checks of asw_match_resident apply, in their order; a method that cannot give a confidence (ASW_ALG_SGBM, ASW_ALG_BM,
 * ASW_ALG_NCC, a value outside the table) returns what a 2-channel asw_stereo_match returns for it.  A failure drops the slot's
 * results and leaves the pair alone.  asw_get_timing afterwards: aggregate_ms / aggregate_launches are the match's, total_ms = the
 * match + the confidence + the smoothing (its 2 T + 2 launches), cost_ms = total_ms - aggregate_ms.
 * asw_stereo_match_smoothed: the same on host images, on the context's private frame; disp: ASW_32F, 1 channel.
 * The carrier has no disparity_type: the matched forms are LEFT-view matches without sub-pixel, cross-scale or scanline flags.  A
 * caller who wants a flagged match makes a 2-channel call and hands its two channels to asw_smooth_disparity. */
enum { ASW_REFINE_SMOOTH = 0x40000000 }; /* win_size / refine_win = ASW_REFINE_SMOOTH | T, T in 1..8 */
static inline int asw_smooth_disparity(asw_ctx* ctx, const asw_image* guide, const float* disp, const float* conf, double sigma_c,
                                       double lambda, int iterations, float* out)
{
    return asw_refine_disparity(ctx, guide, disp, conf, 0, 1, 0.f, ASW_REFINE_SMOOTH | (iterations >= 1 && iterations <= 8 ? iterations : 0), sigma_c, lambda, out, NULL, NULL, NULL);
}
static inline int asw_match_smoothed_resident(asw_ctx* ctx, int slot, int algorithm, int win_size, int min_disparity, int num_disparity,
                                              double sigma_c, double lambda, int iterations)
{
    return asw_match_refined_resident(ctx, slot, algorithm, win_size, min_disparity, num_disparity, 0.f, ASW_REFINE_SMOOTH | (iterations >= 1 && iterations <= 8 ? iterations : 0),
                                      sigma_c, lambda, NULL, NULL);
}
static inline int asw_stereo_match_smoothed(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp, int algorithm,
                                            int win_size, int min_disparity, int num_disparity, double sigma_c, double lambda,
                                            int iterations)
{
    return asw_stereo_match_refined(ctx, left, right, disp, algorithm, win_size, min_disparity, num_disparity, 0.f,
                                    ASW_REFINE_SMOOTH | (iterations >= 1 && iterations <= 8 ? iterations : 0), sigma_c, lambda, NULL, NULL);
}
/* cvtColor(COLOR_BGR2GRAY) as used at M.cpp:1031-1033 */
int asw_bgr2gray(asw_ctx* ctx, const asw_image* bgr, uint8_t* gray);

/* ---- semi-global block matching: StereoSGBM (OpenCV 4.1.0 stereosgbm.cpp, MODE_SGBM_3WAY) as DESIGN.md section 4.8 states it ----
 * The selector's SGBM entry (getDisparity_SGBM, aswMethods.cpp:158-194) runs it with the reference's fixed settings: blockSize w =
 * win > 0 ? win : 3, preFilterCap 10, P1 = 8*cn*w*w, P2 = 32*cn*w*w, uniquenessRatio 10, speckleWindowSize 175, speckleRange 32,
 * disp12MaxDiff 200, and returns convertTo(CV_8U, 1/16) of the result as floats; numDisparity % 16 != 0 and an even win (CV_Error in
 * the reference) give ASW_ERR_UNSUPPORTED_METHOD; disparity_type is ignored (the left-view map); it has no cost volume.
 * asw_sgbm: StereoSGBM::create(min_disparity, num_disparities, block_size, p1, p2, disp12_max_diff, pre_filter_cap, uniqueness_ratio,
 * speckle_window_size, speckle_range, mode) + compute().  disp16: ASW_16S, 1 channel (else ASW_ERR_UNSUPPORTED_LAYOUT, as for
 * asw_filter_speckles), rows x cols: disparity x 16, invalid pixels 16 * (min_disparity - 1).  mode: 2 (MODE_SGBM_3WAY), or the value asw_sgbm_paths or asw_sgbm_census below forms; else ASW_ERR_UNSUPPORTED_METHOD.  num_disparities: a positive multiple of
 * 16, at most 1024; min_disparity >= 0; 16 * (min_disparity + num_disparities) <= 32767; 1 or 3 channels.  Parameters for which a sum
 * could leave int32 (3 * (C_max + P2) >= 2^31, C_max = cn * (2 * ftzero + 63) * w^2) are refused with ASW_ERR_BAD_ARGUMENT.
 * cost_volume_out (optional): the aggregated cost S of the three paths, f32 [num_disparities][rows][cols] (plane k <-> disparity
 * min_disparity + k), 0 in the columns x < min_disparity + num_disparities; refused (ASW_ERR_BAD_ARGUMENT) when S could exceed 2^24
 * (not exact in f32) or when cost_volume_floats is short. */
int asw_sgbm(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp16, int min_disparity,
             int num_disparities, int block_size, int p1, int p2, int disp12_max_diff, int pre_filter_cap,
             int uniqueness_ratio, int speckle_window_size, int speckle_range, int mode, float* cost_volume_out,
             size_t cost_volume_floats);
/* asw_sgbm_paths: asw_sgbm with the aggregated cost S summed over a chosen set of path directions instead of
 * the three of MODE_SGBM_3WAY; everything before and after the aggregation is asw_sgbm's, and every other argument behaves as
 * there, with the same statuses in the same order.  A direction is the step (dx, dy) from a pixel's predecessor to the pixel; a
 * path starts (previous L = 0) wherever the predecessor lies outside the valid columns x >= min_disparity + num_disparities or the
 * rows of the frame.  paths: an OR of ASW_SGBM_PATH_*; a bit outside ASW_SGBM_PATHS_HH: ASW_ERR_BAD_ARGUMENT; a mask without all
 * of ASW_SGBM_PATHS_3WAY: ASW_ERR_UNSUPPORTED_METHOD.  ASW_SGBM_PATHS_3WAY returns bit for bit what asw_sgbm returns.  The named
 * masks read OpenCV's modes as path sets (MODE_HH4: 4 paths, MODE_SGBM: 5, MODE_HH: 8); parity with OpenCV in those modes is not
 * pinned.  With n paths the int32 and f32 bounds become n * (C_max + P2) >= 2^31 and >= 2^24 (ASW_ERR_BAD_ARGUMENT).
 * It is an inline function of this header, not a symbol of the library (the exported set stays as it is): it hands the mask to
 * asw_sgbm in its mode argument, ASW_SGBM_MODE_PATHS | paths, a value no StereoSGBM mode takes; a mask with a bit outside
 * ASW_SGBM_PATHS_HH travels as the invalid mask 0x100, so that it is refused where asw_sgbm refuses a mode. */
enum {
    ASW_SGBM_PATH_LR = 0x01,   /* (1, 0)   left -> right */
    ASW_SGBM_PATH_RL = 0x02,   /* (-1, 0)  right -> left */
    ASW_SGBM_PATH_TB = 0x04,   /* (0, 1)   top -> bottom */
    ASW_SGBM_PATH_BT = 0x08,   /* (0, -1)  bottom -> top */
    ASW_SGBM_PATH_TLBR = 0x10, /* (1, 1)   top-left -> bottom-right */
    ASW_SGBM_PATH_TRBL = 0x20, /* (-1, 1)  top-right -> bottom-left */
    ASW_SGBM_PATH_BRTL = 0x40, /* (-1, -1) bottom-right -> top-left */
    ASW_SGBM_PATH_BLTR = 0x80, /* (1, -1)  bottom-left -> top-right */
    ASW_SGBM_PATHS_3WAY = 0x07,
    ASW_SGBM_PATHS_HH4 = 0x0F,
    ASW_SGBM_PATHS_SGBM = 0x37, /* the four paths from the top-left half plane + right -> left */
    ASW_SGBM_PATHS_HH = 0xFF,
    ASW_SGBM_MODE_PATHS = 0x40000000 /* asw_sgbm's mode: the low bits hold a path mask */
};
static inline int asw_sgbm_paths(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp16, int min_disparity,
                                 int num_disparities, int block_size, int p1, int p2, int disp12_max_diff, int pre_filter_cap,
                                 int uniqueness_ratio, int speckle_window_size, int speckle_range, int paths, float* cost_volume_out,
                                 size_t cost_volume_floats)
{
    const int mask = (paths & ~ASW_SGBM_PATHS_HH) ? 0x100 : paths;
    return asw_sgbm(ctx, left, right, disp16, min_disparity, num_disparities, block_size, p1, p2, disp12_max_diff, pre_filter_cap,
                    uniqueness_ratio, speckle_window_size, speckle_range, ASW_SGBM_MODE_PATHS | mask, cost_volume_out,
                    cost_volume_floats);
}
/* asw_sgbm_census: asw_sgbm_paths with a census cost in place of the prefilter and the Birchfield-Tomasi pixel cost (DESIGN.md section
 * 4.8c), for pairs whose cameras differ in gain or offset: the cost compares the order of intensities, not the intensities.  With
 * x0 = min_disparity + num_disparities, Wv = cols - x0, h = w / 2, w the effective block size:
 *   1. gray: a 3-channel image goes through cvtColor(BGR2GRAY) (asw_set_gray_bits applies), a 1-channel image is used as it is;
 *   2. codeL, codeR: the 62-bit census code of every pixel of the whole image (the code of asw_cost_census: a 9 x 7 window, clamped at
 *      the border, strict '<');
 *   3. pix(y, xi, d) = popcount(codeL[y][x0 + xi] ^ codeR[y][x0 + xi - (min_disparity + d)]), 0..62, on the valid columns;
 *   4. C(y, xi, d) = the sum of pix over |i|, |j| <= h, xi clamped to [0, Wv - 1] and y to [0, rows - 1], as asw_sgbm clamps;
 *   5. paths over the mask, winner, uniqueness, sub-pixel fit, left-right rule, median and speckles are asw_sgbm_paths'.
 * There is no pre_filter_cap.  C_max = 62 * k^2, k = 2 h + 1, whatever the channel count: n * (C_max + P2) >= 2^31, n paths, is
 * refused with ASW_ERR_BAD_ARGUMENT, and with a volume the same bound at 2^24.  cols > 10240 (both code rows of a frame row are
 * staged in 160 KB of LDS): ASW_ERR_BAD_ARGUMENT, after the other argument checks.  Every other argument and status is
 * asw_sgbm_paths', in the same order.  Like it an inline function of this header: the request travels in asw_sgbm's mode as
 * ASW_SGBM_MODE_PATHS | ASW_SGBM_MODE_CENSUS | paths, pre_filter_cap 0 (asw_sgbm ignores it under this mode), an out-of-range mask
 * as 0x100.  ASW_SGBM_MODE_CENSUS without ASW_SGBM_MODE_PATHS is no mode: ASW_ERR_UNSUPPORTED_METHOD. */
enum { ASW_SGBM_MODE_CENSUS = 0x10000 }; /* asw_sgbm's mode, beside ASW_SGBM_MODE_PATHS: the census cost */
static inline int asw_sgbm_census(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp16, int min_disparity,
                                  int num_disparities, int block_size, int p1, int p2, int disp12_max_diff, int uniqueness_ratio,
                                  int speckle_window_size, int speckle_range, int paths, float* cost_volume_out,
                                  size_t cost_volume_floats)
{
    const int mask = (paths & ~ASW_SGBM_PATHS_HH) ? 0x100 : paths;
    return asw_sgbm(ctx, left, right, disp16, min_disparity, num_disparities, block_size, p1, p2, disp12_max_diff, 0,
                    uniqueness_ratio, speckle_window_size, speckle_range, ASW_SGBM_MODE_PATHS | ASW_SGBM_MODE_CENSUS | mask,
                    cost_volume_out, cost_volume_floats);
}
/* cv::filterSpeckles, in place: 4-connected components of pixels != new_val whose neighbours differ by at most max_diff; every
 * component of at most max_speckle_size pixels becomes new_val.  img: ASW_16S, 1 channel (ASW_8U: ASW_ERR_UNSUPPORTED_LAYOUT). */
int asw_filter_speckles(asw_ctx* ctx, asw_image* img, int new_val, int max_speckle_size, int max_diff);

/* ---- block matching: StereoBM (OpenCV 4.1.0 stereobm.cpp, PREFILTER_XSOBEL) as DESIGN.md section 4.9 states it ----
 * asw_stereo_bm: StereoBM::create + setters + compute().  left / right: ASW_8U, 1 channel (else ASW_ERR_UNSUPPORTED_LAYOUT, as
 * StereoBM); disp16: ASW_16S, 1 channel, rows x cols: disparity x 16, FILTERED = 16 * (min_disparity - 1).  Every image's step
 * is honoured.  pre_filter_type: ASW_PREFILTER_XSOBEL only (ASW_PREFILTER_NORMALIZED_RESPONSE: ASW_ERR_UNSUPPORTED_METHOD).
 * StereoBM::compute's assertions give ASW_ERR_BAD_ARGUMENT: pre_filter_size odd in 5..255, pre_filter_cap in 1..63, block_size odd
 * in 5..255 and <= min(rows, cols), num_disparities a positive multiple of 16, texture_threshold >= 0, uniqueness_ratio >= 0; so do
 * what the library does not serve: min_disparity < 0, num_disparities > 1024, 16 * (min_disparity + num_disparities) > 32767.
 * disp12_max_diff < 0 skips validateDisparity; speckles are filtered when speckle_range >= 0 and speckle_window_size > 0 (range
 * in whole disparities, unscaled).  cost_volume_out (optional): the block SAD, f32 [num_disparities][rows][cols] (plane k <->
 * disparity min_disparity + k), with values on the rows [w/2, rows - w/2) at the columns [min_disparity + num_disparities - 1,
 * cols) and NaN elsewhere; a short buffer is refused (ASW_ERR_BAD_ARGUMENT) before anything is written.
 * asw_get_disparity_bm: the reference's getDisparity_BM (aswMethods.h:93, aswMethods.cpp:100-146): 1- or 3-channel input (BGR2GRAY
 * on the device, asw_set_gray_bits), blockSize win > 0 ? win : 9, preFilterCap 31, textureThreshold 10, uniquenessRatio 15,
 * disp12MaxDiff 1, speckleWindowSize 100, speckleRange 32; disp_u8: ASW_8U, 1 channel, convertTo(CV_8U, 1/16) of the result.
 * Its CV_Error cases give ASW_ERR_UNSUPPORTED_METHOD: num_disparities % 16 != 0 or <= 0, an even win, an empty image, a blockSize
 * outside 5..min(rows, cols, 255).  The selector's BM value (ASW_ALG_BM) is not routed here. */
enum { ASW_PREFILTER_NORMALIZED_RESPONSE = 0, ASW_PREFILTER_XSOBEL = 1 };
int asw_stereo_bm(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp16, int min_disparity,
                  int num_disparities, int block_size, int pre_filter_type, int pre_filter_size, int pre_filter_cap,
                  int texture_threshold, int uniqueness_ratio, int speckle_window_size, int speckle_range, int disp12_max_diff,
                  float* cost_volume_out, size_t cost_volume_floats);
int asw_get_disparity_bm(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp_u8, int win,
                         int min_disparity, int num_disparities);

/* ---- batch over frames and devices (frames are independent; no collective) ----
 * Frame i goes to device device_ids[i % n_devices]; one host thread + one context per device. */
int asw_stereo_match_batch(int n_frames, const asw_image* lefts, const asw_image* rights, asw_image* disps,
                           int disparity_type, int algorithm, int win_size, int min_disparity,
                           int num_disparity, int n_devices, const int* device_ids);

#ifdef __cplusplus
}
#endif

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#endif /* ASW_MI355X_H */
