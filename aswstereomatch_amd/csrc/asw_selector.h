// The selector's two packed arguments on the host: the fields of `algorithm` and `disparity_type` as
// include/asw_mi355x.h lays them out, one table each, and the two functions that turn a caller's word into MatchParams or into the
// status the header promises.  No HIP, no context and no runner in here: the file compiles alone with a plain C++17 compiler, and
// tests/cpp/selector_words.cpp holds both functions to a record of every rule (tests/test_selector_words_cpu.py).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/asw_mi355x.h"

struct MatchParams {
    int disparity_type, win, minD, numD;  // disparity_type as the caller passed it; decode_disparity_type leaves the direction bit
    int subpixel = 0;                   // 0 | ASW_DISPARITY_SUBPIXEL_PARABOLA | ASW_DISPARITY_SUBPIXEL_EQUIANGULAR
    int cross_scales = 0, cross_lambda_q = 0;  // asw_disparity_cross_scale() fields: 0 = one scale, else 2..5 and 1..255
    float scan_p1 = 0, scan_p2 = 0;     // asw_disparity_scanline() penalties: scan_p1 == 0 = no scanline optimisation
    double gamma_c = 30, gamma_g = 20;  // M.cpp:58
    int twopass = 0;                    // entry 2 as the two-pass approximation (asw_alg_twopass()): the gammas above are its integers
    double eps = 1e-6;                  // M.cpp:73,76
    double rate_s = 10, rate_r = 10;    // M.cpp:82
    double blo_rate_r = 0.015;          // M.cpp:70
    double grid_rate_s = 10, grid_rate_r = 10;  // M.cpp:67
    int cross_tau = 20, cross_trunc = 20;       // ASW_ALG_ADAPTIVE_WEIGHT_CROSS; an encoded selector value replaces them
    int cross_cost = 0;                         // the cost entry 12 aggregates: 0 = truncated AD, 1 = AD-Census (asw_alg_adcensus())
    int lambda_ad = 10, lambda_census = 30;     // AD-Census: the two table constants
    int permeability = 0;                       // entry 12 as the recursive (permeability) aggregation (asw_alg_permeability())
    int perm_sigma = 8, perm_trunc = 20;        // its two parameters, 1..255 each
};
inline MatchParams match_params(int disparity_type, int win, int minD, int numD)
{
    MatchParams mp;
    mp.disparity_type = disparity_type; mp.win = win; mp.minD = minD; mp.numD = numD;
    return mp;
}

// What the host layer knows about a selector value beyond its runner (asw_host.h: MethodInfo adds that; asw_methods.hip: k_methods)
struct MethodTraits {
    int extra_planes;             // candidates / volume planes = numD + extra_planes: 1 where the reference's range is inclusive (offset <= max_offset)
    bool no_volume;               // no selector volume (0 planes), hence no sub-pixel step and no refinement either
    bool ignores_disparity_type;  // whatever disparity_type holds, flags included, is not looked at
    bool no_subpixel;             // a flag of disparity_type is refused with ASW_ERR_UNSUPPORTED_METHOD
    bool packed_params;           // the selector value may carry the method's parameters (asw_alg_cross(), asw_alg_adcensus())
    int planes(int numD) const { return no_volume ? 0 : numD + extra_planes; }
};

// ---- the words: a field is `width` bits from bit `shift`, read as an unsigned number that must lie in lo..hi ----
struct WordField {
    int shift, width, lo, hi;
    constexpr int mask() const { return (int)(((1u << width) - 1u) << shift); }
    constexpr int get(int word) const { return (int)(((unsigned)word >> shift) & ((1u << width) - 1u)); }
    constexpr bool holds(int word) const { return get(word) >= lo && get(word) <= hi; }
};
template <typename... F> constexpr int mask_of(F... f) { return (0 | ... | f.mask()); }
template <typename... F> constexpr bool all_hold(int word, F... f) { return (... && f.holds(word)); }

// disparity_type: the view, the sub-pixel flags (1 = PARABOLA, 2 = EQUIANGULAR, both: refused), and one of two optional steps
// with its flag bit.  Bits 10, 11 and 31 belong to nobody.
constexpr WordField DT_VIEW = {0, 1, 0, 1}, DT_SUBPIXEL = {8, 2, 0, 2};
constexpr WordField DT_CROSS_FLAG = {12, 1, 1, 1}, DT_CROSS_SCALES = {13, 3, 2, 5}, DT_CROSS_LAMBDA_Q = {16, 8, 1, 255};
constexpr WordField DT_SCAN_FLAG = {24, 1, 1, 1}, DT_SCAN_P1 = {1, 7, 1, 127}, DT_SCAN_UNIT = {25, 3, 0, 7}, DT_SCAN_RATIO = {28, 3, 0, 7};
constexpr int DT_CROSS_BITS = mask_of(DT_CROSS_FLAG, DT_CROSS_SCALES, DT_CROSS_LAMBDA_Q);
constexpr int DT_SCAN_BITS = mask_of(DT_SCAN_FLAG, DT_SCAN_P1, DT_SCAN_UNIT, DT_SCAN_RATIO);
static_assert(DT_SUBPIXEL.mask() == (ASW_DISPARITY_SUBPIXEL_PARABOLA | ASW_DISPARITY_SUBPIXEL_EQUIANGULAR), "asw_mi355x.h");
static_assert(DT_CROSS_FLAG.mask() == ASW_DISPARITY_CROSS_SCALE && DT_SCAN_FLAG.mask() == ASW_DISPARITY_SCANLINE, "asw_mi355x.h");

// algorithm: the method in the low byte, two parameter bytes, and in the top byte the flag bit that says whose parameters they are.
// An encoding owns its flag, the three low bytes and, for AD-Census, lambda_ad; every other bit of the top byte must be clear.  The
// rows stand in the order of precedence: the first whose flag is set reads the word, so bit 30 wins over bit 29, bit 28 is
// lambda_ad's under bit 29, and bit 27 is read only when bits 28-30 are clear.
constexpr WordField ALG_METHOD = {0, 8, 0, 255}, ALG_LAMBDA_AD = {24, 5, 1, 31}, ALG_NO_FIELD = {24, 0, 0, 0};
struct AlgEncoding {
    int flag, method;        // method < 0: any method of the table with packed_params
    WordField p8, p16, top;  // bits 8-15, bits 16-23, and what the encoding keeps in the top byte beside its flag
};
constexpr AlgEncoding k_alg_encodings[] = {
    {ASW_ALG_CROSS_PARAMS, -1, {8, 8, 0, 255}, {16, 8, 1, 255}, ALG_NO_FIELD},      // asw_alg_cross(): tau, trunc
    {ASW_ALG_ADCENSUS_PARAMS, -1, {8, 8, 0, 255}, {16, 8, 1, 255}, ALG_LAMBDA_AD},  // asw_alg_adcensus(): tau, lambda_census, lambda_ad
    {ASW_ALG_TWOPASS_PARAMS, ASW_ALG_ADAPTIVE_WEIGHT, {8, 8, 1, 255}, {16, 8, 1, 255}, ALG_NO_FIELD},  // asw_alg_twopass(): gamma_c, gamma_g
    {ASW_ALG_PERMEABILITY_PARAMS, ASW_ALG_ADAPTIVE_WEIGHT_CROSS, {8, 8, 1, 255}, {16, 8, 1, 255}, ALG_NO_FIELD},  // asw_alg_permeability(): sigma, trunc
};

// The selector's `algorithm` as a caller passes it -> the plain enum value in *method and the encoding's parameters in mp (left
// alone for a plain value and for a refused one; mp may be null).  traits(method): the MethodTraits row of a plain value, null
// outside the table.  A low byte that is not the encoding's method is refused before a field out of range or a bit nobody owns.
template <typename Lookup>
int decode_algorithm(int algorithm, int* method, MatchParams* mp, Lookup&& traits)
{
    *method = algorithm;
    for (const AlgEncoding& e : k_alg_encodings) {
        if (!(algorithm & e.flag)) continue;
        const int low = ALG_METHOD.get(algorithm);
        const MethodTraits* m = traits(low);
        if (e.method < 0 ? !m || !m->packed_params : low != e.method) return ASW_ERR_UNSUPPORTED_METHOD;
        const int owned = mask_of(ALG_METHOD, e.p8, e.p16, e.top) | e.flag;
        if ((algorithm & ~owned) || !all_hold(algorithm, e.p8, e.p16, e.top)) return ASW_ERR_BAD_ARGUMENT;
        *method = low;
        if (!mp) return ASW_OK;
        const int p8 = e.p8.get(algorithm), p16 = e.p16.get(algorithm);
        switch (e.flag) {
        case ASW_ALG_CROSS_PARAMS: mp->cross_tau = p8; mp->cross_trunc = p16; break;
        case ASW_ALG_ADCENSUS_PARAMS:
            mp->cross_cost = 1; mp->cross_tau = p8; mp->cross_trunc = 255; mp->lambda_census = p16; mp->lambda_ad = e.top.get(algorithm); break;
        case ASW_ALG_TWOPASS_PARAMS: mp->twopass = 1; mp->gamma_c = p8; mp->gamma_g = p16; break;
        default: mp->permeability = 1; mp->perm_sigma = p8; mp->perm_trunc = p16; break;
        }
        return ASW_OK;
    }
    return ASW_OK;
}

// level s of a cross-scale call: candidates (minD >> s) .. ((minD + n - 1) >> s), n the finest level's plane count
inline void cross_scale_range(const MethodTraits* m, const MatchParams& mp, int s, int* minD, int* numD)
{
    const long long last = (long long)mp.minD + mp.numD + m->extra_planes - 1;  // minD + n - 1, n = m->planes(numD); no int overflow
    *minD = mp.minD >> s;
    *numD = (int)((last >> s) - *minD + 1 - m->extra_planes);
}

// A caller's mp.disparity_type -> mp.subpixel, mp.cross_scales / cross_lambda_q, mp.scan_p1 / scan_p2, and mp.disparity_type with the
// direction bit alone (written once, when the word is accepted): everything the flags refuse before any work is refused here.
// m: the method's row, null outside the table; served: it has a runner; scanline_max_planes: what k_scanline.hip takes.  A method
// that ignores disparity_type and a word with no flag bit (8, 9, 12, 24) pass through untouched, whatever the other bits hold: the
// runner refuses what it always refused.  Otherwise the checks below, in their order.
inline int decode_disparity_type(const MethodTraits* m, bool served, int scanline_max_planes, MatchParams& mp)
{
    const int dt = mp.disparity_type;
    mp.subpixel = mp.cross_scales = mp.cross_lambda_q = 0; mp.scan_p1 = mp.scan_p2 = 0;
    const bool scan = dt & DT_SCAN_FLAG.mask(), cross = dt & DT_CROSS_FLAG.mask();
    if ((m && m->ignores_disparity_type) || !(scan || cross || DT_SUBPIXEL.get(dt))) return ASW_OK;
    if (scan && cross) return ASW_ERR_BAD_ARGUMENT;  // the two together: not served
    const int in_use = mask_of(DT_VIEW, DT_SUBPIXEL) | (scan ? DT_SCAN_BITS : cross ? DT_CROSS_BITS : 0);
    if ((dt & ~in_use) || !DT_SUBPIXEL.holds(dt)) return ASW_ERR_BAD_ARGUMENT;
    if (scan && !all_hold(dt, DT_SCAN_P1, DT_SCAN_UNIT, DT_SCAN_RATIO)) return ASW_ERR_BAD_ARGUMENT;
    if (cross && !all_hold(dt, DT_CROSS_SCALES, DT_CROSS_LAMBDA_Q)) return ASW_ERR_BAD_ARGUMENT;
    if (m && m->no_subpixel) return ASW_ERR_UNSUPPORTED_METHOD;  // NCC: its candidate range is its own
    if ((scan || cross) && (!m || !served || m->no_volume)) return ASW_ERR_UNSUPPORTED_METHOD;
    if (scan && m->planes(mp.numD) > scanline_max_planes) return ASW_ERR_BAD_ARGUMENT;
    for (int s = 1; cross && s < DT_CROSS_SCALES.get(dt); s++) {  // every level keeps at least one candidate for the runner
        int minD_s, numD_s;
        cross_scale_range(m, mp, s, &minD_s, &numD_s);
        if (numD_s < 1) return ASW_ERR_BAD_ARGUMENT;
    }
    mp.disparity_type = DT_VIEW.get(dt);
    mp.subpixel = dt & DT_SUBPIXEL.mask();
    if (cross) { mp.cross_scales = DT_CROSS_SCALES.get(dt); mp.cross_lambda_q = DT_CROSS_LAMBDA_Q.get(dt); }
    if (scan) {
        const int a = DT_SCAN_P1.get(dt), ratio = DT_SCAN_RATIO.get(dt) + 1;
        const float unit = ldexpf(1.0f, 2 * (DT_SCAN_UNIT.get(dt) - 5));  // 4^(u - 5): a * unit and ratio * a * unit are exact
        mp.scan_p1 = (float)a * unit; mp.scan_p2 = (float)(ratio * a) * unit;
    }
    return ASW_OK;
}
