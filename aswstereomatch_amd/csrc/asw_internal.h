// Internal declarations shared by the HIP translation units of libasw_mi355x.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "asw_devmem.h"
#include "asw_streams.h"

// The one way a kernel is launched: ASW_LAUNCH(kernel, grid, block, dynamic LDS bytes, stream, arguments...) gives an asw_status.
//   - more than 160 KB of dynamic LDS (a workgroup's whole share on gfx950): ASW_ERR_BAD_ARGUMENT, nothing is launched;
//   - more than 64 KB: the kernel is opted in first, on every such launch -- the attribute is per device, a process may hold
//     contexts on several devices, and a function-local flag would leave every device after the first at the 64 KB default;
//   - then the launch, then hipGetLastError: a refused launch is reported at its own site and nothing is enqueued behind it.
// A kernel name with a comma in it goes in parentheses, as for any macro.
template <typename K, typename... Args>
int asw_launch_at(const char* what, const char* file, int line, K kern, dim3 grid, dim3 block, size_t lds, hipStream_t s,
                  const Args&... args)
{
    if (lds > 160 * 1024) return ASW_ERR_BAD_ARGUMENT;
    hipError_t e = hipSuccess;
    if (lds > 64 * 1024)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(kern, grid, block, lds, s, args...);
        e = hipGetLastError();
    }
    if (e == hipSuccess) return ASW_OK;
    asw_note_hip_error(e, what, file, line);
    return ASW_ERR_HIP;
}
#define ASW_LAUNCH(kern, ...) asw_launch_at(#kern, __FILE__, __LINE__, kern, __VA_ARGS__)

struct Frame {
    DevBuf L, R;  // dense interleaved 8U images as uploaded
    int rows = 0, cols = 0, channels = 0;
    DevBuf disp;  // f32 rows x cols
    DevBuf vol;   // f32 aggregated cost volume of the last match (if kept)
    size_t vol_floats = 0;
    DevBuf dconf; // float2 {disparity, confidence} rows x cols, packed: only a 2-channel disparity image asks for it (k_confidence.hip)
    bool has_conf = false;  // dconf belongs to the current disp / vol
    bool valid = false;
    // the disparity (and volume) in `disp` / `vol` belong to the CURRENT pair: set by a successful match, cleared by every
    // upload / pre-processing into the slot and by a failed match, so a download can never return another frame's result
    // or read a smaller, older allocation
    bool has_disp = false;
    int disp_rows = 0, disp_cols = 0;
    void invalidate_results() { has_disp = has_conf = false; disp_rows = disp_cols = 0; vol_floats = 0; }
};

struct BilateralTables {
    // (kind, win, gamma_c, gamma_g, mirror); kind 0: classic (all win*win-1 taps, transposed consume order), 1: direct8 (row +
    // column + diagonal)
    TableCache<std::tuple<int, int, double, double, int>> cache;
    int ntaps = 0, ncls = 0;
    DevBuf taps;  // int4 per tap
    DevBuf lut;   // float [ncls][256]
    DevBuf cells; // kind 0, win 15, not mirrored: int4 per window cell (kx = -3..17, ky = 0..14) for k_asw_bilateral_xq
    DevBuf lut_xq;        // kind 0, win 15: the LUT x 2^60 -- k_asw_bilateral_xq accumulates in its scaled domain
    bool xq_lut_ok = false;  // the LUT admits that domain (bilateral_xq_lut_ok); else the one-kernel form runs
};

// Measurement / test switches, read from the environment ONCE when a context is created (asw_create): a call never looks at
// the environment.  -1 / 0 = the library's own choice.  A switch stays only while a GPU test sets it
// (tests/test_tuning_switches_cpu.py): the form it selects is otherwise code nothing checks.
struct AswTuning {
    int bilateral_xq = -1;       // ASW_BILATERAL_XQ: 0 = one-kernel form only (k_asw_bilateral), 1 = xq form wherever it applies
    int geodesic_xq = -1;        // ASW_GEODESIC_XQ
    int wmedian_tile = -1;       // ASW_WMEDIAN_TILE: 0 = per-pixel sort (k_wmedian)
    int wmedian_tile_chunk = 0;  // ASW_WMEDIAN_TILE_CHUNK: slices per list chunk (tests: odd chunkings)
    int wmedian_gen_rows = 0;    // ASW_WMEDIAN_GEN_ROWS: block rows per workgroup of the general tile form (windows 17..37): 1 | 2 | 4 | 8
    int band_ab = 0, band_q = 0; // ASW_BAND_AB / ASW_BAND_Q: rows per band of the guided filter's passes
    int ring_ab = 1, ring_q = 1; // ASW_RING_AB / ASW_RING_Q: register-ring form of the two passes (k_guided.hip: launch_guided3), 0 = re-fetch
    int guided_fused = -1;       // ASW_GUIDED_FUSED: fused a/b -> q walk of GuidedF_2 at 15x15 (k_guided_pair3: no a/b volume, a third of the traffic): 1 always, 0 never, -1 = frames large enough for it (guided_uses_fused)
    int ab6_pair = -1;           // ASW_AB6_PAIR: 0 = the a/b pass of the 6-channel guide through k_box_walk instead of k_ab6_pair
    int q6_pair = -1;            // ASW_Q6_PAIR: 0 = the q pass of the 6-channel guide through k_box_walk (re-fetching form) instead of k_q6_pair
    int q_wg_strips = 1;         // ASW_Q_WG_STRIPS: workgroup of the q pass = 4 neighbouring strips (1) / 4 slices of a strip (0)
    int guide_share = 1;         // ASW_GUIDE_SHARE: 6-channel guide [fixed image, other image shifted by d] (GuidedF, GuidedF_3 LEFT / RIGHT):
                                 // 1 = statistics shared across slices (k_guided.hip: StatsSplit), 0 = plain statistics of every slice
    int perm_chunk = 0;          // ASW_PERM_CHUNK: candidates per chunk of the permeability aggregation (tests: odd chunkings; the result does not depend on it)
    void read_environment();
};
// the name of AswTuning::perm_chunk's switch
constexpr char ASW_PERM_CHUNK_NAME[] = "ASW_PERM_CHUNK";

struct RefineTables {  // integer weights of the refinement's median (k_refine.hip)
    TableCache<std::tuple<int, double, double, int>> cache;  // (win, gamma_c, gamma_s, channels)
    int ntc = 0;
    DevBuf tc;  // u32 [255 * channels + 1]: floor(4096 * exp(-c / gamma_c) + 0.5)
    DevBuf ts;  // u32 [win/2 + 1][win/2 + 1]: floor(256 * exp(-sqrt(i*i + j*j) / gamma_s) + 0.5)
};

struct TwoPassTable {  // the weight table of the two-pass method (k_twopass.hip)
    TableCache<std::tuple<int, int, int>> cache;  // (win, gamma_c, gamma_g)
    DevBuf t;  // float [win / 2 + 1][256]: (float)exp(-(dc / gamma_c + r / gamma_g))
};

struct PermTable {  // the permeability table of k_permeability.hip
    TableCache<int> cache;  // sigma
    DevBuf t;  // double [256]: (double)(float)exp(-(double)k / sigma)
};

struct SmoothTable {  // the link-weight table of k_smooth.hip
    TableCache<std::tuple<double, int>> cache;  // (sigma_c, channels)
    DevBuf t;  // double [255 * channels + 1]: floor(65536 * exp(-k / sigma_c) + 0.5) / 65536
};

struct CensusTables {  // the AD-Census cost tables (asw_methods.hip: ensure_census_tables)
    TableCache<std::tuple<int, int>> cache;  // (lambda_ad, lambda_census)
    DevBuf t;  // u8 TA[256] | TC[64]
};

struct WMedianTables {  // weighted-median tables, two independent entries
    TableCache<double> lut2_cache;  // rateR
    DevBuf lut2;  // exp() LUT of the colour weight
    TableCache<std::tuple<double, int>> wd_cache;  // (rateS, win)
    DevBuf wd;    // space kernel
};

struct PrepTables {  // tables of the pre-processing entry points (asw_context.hip: ensure_prep_tables): they have no parameter
    TableCache<int> cache;
    int ntaps = 0;  // taps of the bilateral filter
    DevBuf t;
};

constexpr int CROSS_SCALE_MAX = 5;  // most pyramid levels of a cross-scale call, the finest included

struct asw_ctx {
    int device = 0;
    AswTuning tune;
    int gray_bits = 14;  // cvtColor(BGR2GRAY) constant set (asw_set_gray_bits): 14 = OpenCV 4.1.0, 15 = later 4.x
    hipStream_t stream = nullptr;
    std::vector<Frame> frames;  // resident slots of asw_upload_pair / asw_match_resident (caller-numbered)
    Frame host_frame;           // private frame of the host-buffer entry points (asw_stereo_match, asw_aggregate_*): never a slot
    Frame coarse[CROSS_SCALE_MAX - 1];  // private pyramid levels 1.. of a cross-scale call (pair and volume of each level): never slots
    std::vector<unsigned char> host_pack;  // dense staging for host images whose rows carry padding (asw_context.hip: copy_rows)
    std::map<std::string, DevBuf> scratch;  // named grow-only scratch buffers
    BilateralTables bil;
    RefineTables refine;
    TwoPassTable twopass;
    PermTable perm;
    SmoothTable smooth;
    CensusTables census;
    WMedianTables wm;
    PrepTables prep;
    CallClock clock;  // the call's four timing events and the asw_timing they give (asw_streams.h)
    SideSet side;     // the two side streams and their fork / join events; a runner uses them through a SideStreams scope
    DevBuf& buf(const char* name) { return scratch[name]; }
    asw_ctx() = default;
    asw_ctx(const asw_ctx&) = delete;
    asw_ctx& operator=(const asw_ctx&) = delete;
    // waits for the work in flight and gives back the streams and events, however few asw_create got to; the buffers free themselves
    ~asw_ctx()
    {
        (void)hipSetDevice(device);
        for (hipStream_t s : {stream, side.stream[0], side.stream[1]})
            if (s) (void)hipStreamSynchronize(s);
        for (hipEvent_t e : {clock.total_start, clock.total_stop, clock.agg_start, clock.agg_stop})
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : {side.fork, side.joined[0], side.joined[1]})
            if (e) (void)hipEventDestroy(e);
        for (hipStream_t s : {stream, side.stream[0], side.stream[1]})
            if (s) (void)hipStreamDestroy(s);
    }
};

// ---- kernel launchers (each returns an asw_status; all work is enqueued on `s`) ----
// bits: fixed-point width of the BT.601 constants, 14 (OpenCV 4.1.0, the reference's pin) or 15 (later 4.x): SURVEY App. A-1
int launch_bgr2gray(hipStream_t s, const uint8_t* bgr, int H, int W, uint8_t* gray, int bits);
// cvtColor(COLOR_RGB2GRAY) applied to BGR data, as computeNCC does (M.cpp:835,840): the R and B coefficients swap
int launch_rgb2gray(hipStream_t s, const uint8_t* bgr, int H, int W, uint8_t* gray, int bits);
// cost u8 [numD][H][W].  The staged row pair (2 W C bytes) must fit 160 KB of LDS, else ASW_ERR_BAD_ARGUMENT: W <= 27306 (C = 3),
// 81920 (C = 1)
int launch_cost_ad(hipStream_t s, const uint8_t* L, const uint8_t* R, int H, int W, int C, int disp_type, int minD,
                   int numD, int do_thresh /* 0: AD, 1: TAD mask, 2: SD */, int threshold, uint8_t* cost);
int launch_wta(hipStream_t s, const float* vol, int n, int H, int W, int minD, float* disp);
// ---- sub-pixel disparity (k_subpixel.hip), DESIGN.md section 4.11 ----
// mode: ASW_DISPARITY_SUBPIXEL_PARABOLA | ASW_DISPARITY_SUBPIXEL_EQUIANGULAR; vol [n][H][W] (plane k <-> disparity minD + k);
// disp [H][W]: the integer winner-take-all map, refined in place
int launch_subpixel(hipStream_t s, int mode, const float* vol, int n, int H, int W, int minD, float* disp);
// ---- confidence (k_confidence.hip), DESIGN.md section 4.24 ----
// vol [n][H][W], disp [H][W]: the final map, copied; out [H][W]: {disparity, confidence} interleaved, 8 bytes per pixel
int launch_confidence(hipStream_t s, const float* vol, int n, int H, int W, const float* disp, float2* out);

// ---- cross-scale aggregation (k_cross_scale.hip), DESIGN.md section 4.18 ----
// one pyramid step: dst [ceil(H/2)][ceil(W/2)][C] from src [H][W][C], the rounded 2x2 mean with the last row / column repeated
int launch_pyramid_down(hipStream_t s, const uint8_t* src, int H, int W, int C, uint8_t* dst);
// w[0..S-1]: the first column of the inverse of the paper's tridiagonal matrix for lambda = q / 64, solved in f64, rounded to f32
void cross_scale_weights(int S, int q, float* w);
struct CrossScaleLaunch {
    float* vol;   // V_0 [n][H][W]: read, and overwritten with the combined volume when `store`
    float* disp;  // [H][W]
    int H, W, n, minD, S, store;
    float w[CROSS_SCALE_MAX];
    const float* cv[CROSS_SCALE_MAX - 1];  // V_s of level s = index + 1: [planes_s][Hs][Ws]
    int cH[CROSS_SCALE_MAX - 1], cW[CROSS_SCALE_MAX - 1], cminD[CROSS_SCALE_MAX - 1];
};
int launch_cross_scale_combine(hipStream_t s, const CrossScaleLaunch& a);

// ---- scanline optimisation of an aggregated volume (k_scanline.hip), DESIGN.md section 4.19 ----
struct ScanlineLaunch {
    float* vol;   // V [n][H][W]: read, and overwritten with the optimised volume
    float* sum;   // scratch, n * H * W floats: the paths' running sum, [y][x][k]
    float* ck;    // scratch, scanline_checkpoint_floats(H, W, n) floats
    float* disp;  // [H][W]: the optimised volume's winner
    int H, W, n, minD;
    float P1, P2;
};
int scanline_max_planes();  // 1025
size_t scanline_checkpoint_floats(int H, int W, int n);
int launch_scanline(hipStream_t s, const ScanlineLaunch& a);  // horizontal pass, TB, BT + winner: three kernels

struct BilateralLaunch {
    const uint8_t* gL;
    const uint8_t* gR;
    int H, W, win, minD, nD;  // nD = number of candidates (numD + 1 for the reference's inclusive range)
    const int4* taps;         // {sample cell offset dys*LW+dxs, weight dx, weight dy, class*256}
    const float* lut;         // [ncls][256]
    int ntaps;
    int flip;    // 1: mirrored problem (DISPARITY_RIGHT), taps must come from the mirrored table
    float* vol;  // optional [nD][H][W]
    float* disp; // [H][W]
    double* partE;  // optional scratch [max_slices][H][W]: per-slice winners when the d range is split over grid.z
    float* partD;
    int max_slices;
    int c_begin = 0;  // > 0: only candidates [c_begin, nD)
    int resume = 0;   // 1: the running minimum starts from partE / partD ([H][W]) instead of DBL_MAX
    int out_slice = -1;  // >= 0: write this launch's winners to slice out_slice of partE / partD (merged later) instead of disp
    int col_lo = 0, col_hi = -1;  // image columns [col_lo, col_hi) to compute (col_hi < 0: W): only the tiles that overlap them are
                                  // launched and nothing is stored outside them (not with the grid.z split of small frames)
};
// xq form of the classic kernel (k_bilateral_xq.hip): candidates [0, bilateral_xq_candidates()) of a DISPARITY_LEFT, win = 15
// problem with at least that many candidates; writes the running minimum to bestE / bestD for the tail launch, or -- when
// there is no tail (disp != nullptr) -- the disparity itself
int bilateral_xq_candidates(int nwave);  // nwave = 8 / 4 wavefronts per workgroup: 128 / 64 candidates
// The xq kernel takes the LUT scaled by 2^XQ_LUT_SCALE_LOG2; its sums are bit-identical to the reference's only when every
// nonzero weight product is >= 2^-68 and the scaled products stay finite: checked on the (unscaled) LUT.
constexpr int XQ_LUT_SCALE_LOG2 = 60;
bool bilateral_xq_lut_ok(const float* lut, size_t n);
int launch_bilateral_xq(hipStream_t s, hipStream_t s_border, int nwave, const uint8_t* gL, const uint8_t* gR, int H, int W, int minD,
                        const int4* cells, const float* lut, float* vol, double* bestE, float* bestD, float* disp, bool right = false,
                        bool last = false);
// image columns [*lo, *hi) that the interior tiles of the xq launch cover (empty: no interior tile)
void bilateral_xq_interior_columns(int W, bool right, int* lo, int* hi);
int launch_bilateral(hipStream_t s, const BilateralLaunch& a);
// winners of per-slice partial WTAs (candidate range split over grid.z for small frames) -> disparity, strict '<' in ascending d
int launch_merge_slices(hipStream_t s, const double* partE, const float* partD, int nz, size_t plane, float* disp);
// the same over the image columns [col_lo, col_hi) only
int launch_merge_slices_cols(hipStream_t s, const double* partE, const float* partD, int nz, int H, int W, int col_lo, int col_hi,
                             float* disp);
int bilateral_lds_row_stride(int win);  // LW of the kernel's sample tile (taps[].x is expressed in it)
// largest window launch_bilateral serves: the last odd one whose LDS layout fits a workgroup's 160 KB (63: 160160 bytes).  The host
// entries refuse a larger window before they build a table
int bilateral_max_window();

// ---- two-pass (separable) ASW (k_twopass.hip), DESIGN.md section 4.16 ----
struct TwoPassLaunch {
    const uint8_t* gL;   // reference gray image (RIGHT: the right image), read mirrored when flip
    const uint8_t* gR;
    int H, W, win, minD, nD;  // nD = number of candidates (numD + 1: the inclusive range of entry 2)
    const float* table;  // TwoPassTable: [win / 2 + 1][256]
    int flip;            // 1: mirrored problem (DISPARITY_RIGHT)
    float* vol;          // optional [nD][H][W]
    float* disp;         // [H][W]
};
int launch_twopass(hipStream_t s, const TwoPassLaunch& a);
// largest window launch_twopass serves: the last odd one whose LDS layout (sums of a chunk, table, two gray tiles) fits a
// workgroup's 160 KB (95: 162976 bytes).  The host entry refuses a larger window before it builds a table
int twopass_max_window();

// ---- recursive (permeability) aggregation (k_permeability.hip), DESIGN.md section 4.17 ----
// The kernels scan in segments of 16 positions: perm_segments(n) segments along an axis of n positions, and the permeability planes
// carry perm_padded(n) entries per row (zeros in front of position 1 and behind the last one).  No limit of their own on rows or
// columns: rows * cols < 2^31 is all they ask.
int perm_segments(int n);
int perm_padded(int n);
// ph [H][perm_padded(W)], pvT [W][perm_padded(H)] (transposed) from the view image (C = 1 or 3) and the table P[256]; two launches
int launch_perm_weights(hipStream_t s, const uint8_t* img, int H, int W, int C, const double* P, double* ph, double* pvT);
struct PermLaunch {
    const uint8_t* cost;  // u8 cost planes of the chunk, [nc][H][W]
    int H, W, nc, trunc;  // nc candidates in the chunk; e = min(trunc, cost)
    int cbeg, minD, first;  // vertical: the chunk's first plane in the volume, the map's offset, 1 = the first chunk of the frame
    const double* ph;
    const double* pvT;
    double* ck;           // checkpoints: nc * max(H * perm_segments(W), W * perm_segments(H)) doubles, shared by the two passes
    double* hs;           // horizontal sums [H][W][nc]: written by the horizontal, read by the vertical pass
    const double* N;      // vertical: the frame's N, transposed [W][perm_padded(H)]; null: this launch computes it (nc = 1) into Nout
    double* Nout;
    float* vol;           // optional [..][H][W]
    double* bestE;        // [H][W] running minimum across chunks
    float* disp;          // [H][W]
};
int launch_perm_scan_h(hipStream_t s, const PermLaunch& a);
int launch_perm_scan_v(hipStream_t s, const PermLaunch& a);

// ---- cost kernels (k_cost.hip) ----
int launch_scharr_x(hipStream_t s, const uint8_t* img, int H, int W, int pad, short* grad /* [H][W+pad][3] */);
// ord_scratch (similarity_parts_words() u32 words) / scales (optional): fused per-slice min/max -> normalize()
// parameters of every cost plane
size_t similarity_parts_words(int H, int W, int numD);
int launch_similarity(hipStream_t s, const uint8_t* L, const uint8_t* R, const short* gL, const short* gR, int H, int W,
                      int minD, int numD, double regularity, double thresC, double thresG, float* cost, uint32_t* ord_scratch,
                      float2* scales);
int launch_pad_reflect(hipStream_t s, const float* src, int n, int H, int W, int h, float* dst);
// per-slice normalize(NORM_MINMAX) parameters {scale, shift} of a dense f32 volume [n][plane]
int launch_slice_scales(hipStream_t s, const float* vol, int n, size_t plane, uint32_t* ord_scratch /* 2n */, float2* scales);
int launch_u8_scale(hipStream_t s, const uint8_t* img, size_t nbytes, uint32_t* ord_scratch /* 2 */, float2* scale1);
int launch_guide_scales_lr(hipStream_t s, const uint8_t* ref_img, const uint8_t* shifted_img, int H, int W, int minD, int numD,
                           int disp_type, uint32_t* ord_scratch, int* colmm_scratch /* 2W */, float2* scales /* numD */);

// ---- NCC cost (k_ncc.hip), computeNCC / getInputImgNCC, M.cpp:767-1013; launch_box_mean_u8 lives in k_guided.hip ----
struct NccLaunch {
    const uint8_t* gref;  // reference gray image [H][W]
    const float* mref;    // its box means
    const double* sref;   // its window sums of squares
    const uint8_t* goth;  // other gray image, REFLECT-padded to [H][Wp]
    const float* moth;
    const double* soth;
    int H, W, Wp, win, minD, numD, right, nwta;
    float* vol;   // optional [numD][H][W], un-normalised
    float* disp;  // optional [H][W], WTA over the first nwta candidates
};
int launch_pad_gray(hipStream_t s, const uint8_t* g, int H, int W, int padL, int padR, uint8_t* out);
int launch_box_mean_u8(hipStream_t s, const uint8_t* img, int H, int W, int win, float* mean);  // boxFilter(8U -> 32F)
int launch_ncc_selfsum(hipStream_t s, const uint8_t* g, const float* mean, int H, int W, int win, double* ss);
int launch_ncc(hipStream_t s, const NccLaunch& a);
// largest window launch_ncc serves: the last odd one whose two f32 tiles fit 64 KB of LDS (59: 64232 bytes)
int ncc_max_window();
int launch_apply_scales(hipStream_t s, float* vol, int n, size_t plane, const float2* scales);

// ---- driver-side pre/post-processing (k_prep.hip), SURVEY 8f row f3 ----
int launch_resize_linear(hipStream_t s, const uint8_t* src, int sh, int sw, uint8_t* dst, int dh, int dw);
int launch_bgr2hsv(hipStream_t s, const uint8_t* bgr, size_t n, const int* sdiv, const int* hdiv, uint8_t* hsv);
int launch_boost_hsv2bgr(hipStream_t s, const uint8_t* hsv, int H, int W, const int* taps, int ntaps, const float* color_lut,
                         uint8_t* bgr);
int launch_disp_to_u8(hipStream_t s, const float* disp, size_t n, int normalize, uint8_t* out, int* mm_scratch);

// ---- box means / guided filter (k_guided.hip) ----
// largest box side k of the sliding walk behind launch_cost_sad, launch_box_mean_u8 and launch_guided (`r` there): k - 1 halo columns
// must leave outputs in a two-columns-per-lane strip (64)
int walk_max_kernel();
int launch_cost_sad(hipStream_t s, const uint8_t* gl, const uint8_t* gr, int H, int W, int disp_type, int win, int minD,
                    int numD, float* cost);
struct GuidedLaunch {
    const uint32_t* guideA; // BGRX plane holding guide channels 0..2
    const uint32_t* guideB; // BGRX plane holding guide channels 3..5 (C = 6), else null
    int shiftA, shiftB;     // plane A / B is read at reflect(x + shift*d): GuidedF LEFT = (0,-1), RIGHT = (+1,0); else 0
    int C;                  // 3 or 6
    int guide_per_slice;    // 1: guide (hence its statistics and scales) changes with the slice
    const float2* gscales;  // guide normalize() parameters (1 or n entries)
    const float* P;         // raw cost volume [n][H][W]
    const float2* pscales;  // per-slice normalize() parameters of P
    int H, W, n, r, minD;
    double eps;
    int nan_safe;           // 1: P may hold NaN (NCC costs of flat windows; caller-supplied P): window sums are rebuilt when a running sum is poisoned
    float* stats;           // scratch, guided_stats_floats(): {meanI_c, var_c+eps} interleaved per pixel and BGRX word
    int* rep_scratch;       // scratch, n ints (or null): scale-group representative of every slice (6-channel per-slice guides)
    float* ab;              // scratch, guided_ab_floats(): {a_c, b} per pixel (3-channel guide: strip-major float2 tiles, k_guided.hip ABTiles)
    size_t ab_floats;       // capacity of `ab` in floats: the two-pass path needs guided_ab_floats(), the fused walk none
    int fused;              // 1: the fused a/b -> q walk (the caller's guided_uses_fused decision); launch_guided does not decide again
    float* q;               // out [n][H][W]
    const AswTuning* tune;  // the context's switches
};
size_t guided_stats_floats(int C, int nstat, int H, int W);
size_t guided_ab_floats(int C, int n, int H, int W, int r);
// true: the fused a/b -> q walk exists for this problem (3-channel slice-independent guide, finite costs, 15x15, H >= 16)
bool guided_fused_form_exists(int C, int guide_per_slice, int shifted, int nan_safe, int H, int r);
// true: run the fused walk (GuidedLaunch::fused) -- the form exists and the switches / frame size ask for it; decided once, by the caller
bool guided_uses_fused(const AswTuning& t, int C, int guide_per_slice, int shifted, int nan_safe, int H, int W, int n, int r);
int launch_pack_words(hipStream_t s, const uint8_t* img, int H, int W, int C, int w, uint32_t* out);
int launch_guided(hipStream_t s, const GuidedLaunch& a);

// ---- geodesic support weights (k_geodesic.hip) ----
int launch_pack_bgrx(hipStream_t s, const uint8_t* bgr, int H, int W, uint32_t* out);
int launch_geodesic_weights_u16(hipStream_t s, const uint32_t* img, int H, int W, int win, int iter, uint16_t* planes);
int launch_geodesic_weights_f32(hipStream_t s, const uint32_t* img, int H, int W, int win, int iter, float* planes);
int launch_planes_to_windows(hipStream_t s, const float* planes, int H, int W, int cells, float* out);
// c_begin / out_slice: only candidates [c_begin, nD), winners to slice out_slice of partE / partD (-1: to disp)
int launch_asw_geodesic(hipStream_t s, const uint32_t* imgL, const uint32_t* imgR, const uint16_t* wL, const uint16_t* wR,
                        int H, int W, int win, int minD, int nD, int flip, float* vol, float* disp, double* partE /* optional
                        scratch [8][H][W] */, float* partD, int c_begin = 0, int out_slice = -1);
// a few candidates [c_begin, nD) of a 15x15 problem (the remainder behind the xq passes), un-mirrored: imgF / wF = the fixed image
int launch_asw_geodesic_few(hipStream_t s, const uint32_t* imgF, const uint32_t* imgO, const uint16_t* wF, const uint16_t* wO, int H,
                            int W, int minD, int c_begin, int nD, bool right, float* vol, double* outE, float* outD);
// xq form (k_geodesic_xq.hip): one pass = candidates [cbase, cbase + 16 * nwave), nwave = 8 or 4, DISPARITY_LEFT, win = 15
int geodesic_xq_pass_candidates(int nwave);
int launch_geodesic_xq(hipStream_t s, hipStream_t s_border, int nwave, const uint32_t* imgL, const uint32_t* imgR, const uint16_t* wL,
                       const uint16_t* wR, int H, int W, int minD, int cbase, float* vol, double* outE, float* outD, bool right = false);

// ---- weighted median (k_wmedian.hip) ----
int launch_wm_weights(hipStream_t s, const uint8_t* img, int H, int W, int pad, int win, const float* lut2, const float* wd,
                      float* out);
int launch_wmedian(hipStream_t s, const float* cost, const float* wLd, const float* wRb, int H, int W, int win, int numD,
                   int max_off, float* out);
size_t wmedian_tile_list_slots(int H, int W, int d_count);
int launch_wmedian_tile(hipStream_t s, const float* cost, const float* wLd, const float* wRb, int H, int W, int numD, int max_off,
                        int d_begin, int d_count, uint32_t* listC, uint16_t* listP, float* out);
// windows 17x17 .. 37x37 (k_wmedian_tile_gen.hip)
bool wmedian_tile_gen_supported(int win);
int wmedian_tile_gen_slots(int win);
int launch_wmedian_tile_gen(hipStream_t s, const float* cost, const float* wLd, const float* wRb, int H, int W, int win, int numD,
                            int max_off, int d_begin, int d_count, uint32_t* listC, uint16_t* listP, float* out, int rows_per_part);

// ---- O(1)-bilateral ASW (BLO1), k_blo1.hip ----
int launch_blo1(hipStream_t s, const uint8_t* gl, const uint8_t* gr, const float* cost, int step, int H, int W, int disp_type,
                int win, int numD, float* vol, float* disp);
// largest window launch_blo1 serves: the last odd one whose tile fits 160 KB of LDS at chunk width 1.  run_blo1 also builds the SAD
// cost with the walk, so the entry serves min(blo1_max_window(), walk_max_kernel()) rounded down to odd
int blo1_max_window();

int launch_lr_check(hipStream_t s, const float* dl, const float* dr, int H, int W, float max_diff, float invalid, float* out,
                    unsigned* n_invalid);

// ---- left-right refinement (k_refine.hip): cross-check, scan-line fill, weighted median; DESIGN.md section 4.10 ----
struct RefineLaunch {
    const uint8_t* guide;  // dense interleaved 8U, C = 1 or 3 channels
    int C;
    const float* dl;       // left-view map, absolute disparities
    const float* dr;       // right-view map
    int H, W, minD, n;     // admissible values minD .. minD + n - 1
    float max_diff;
    int win;               // odd, 1..35
    const unsigned* tc;    // RefineTables
    int ntc;
    const unsigned* ts;
    uint8_t* mask;         // out [H][W]: 0 valid, 1 filled, 2 unfillable
    unsigned short* F;     // scratch [H][W]: filled map, disparity - minD (0xFFFF unfillable)
    float* out;            // out [H][W]; must not alias dl / dr
    unsigned* counters;    // 3 words: rejected pixels, unfillable pixels, != 0 when dl leaves the domain
};
int launch_refine(hipStream_t s, const RefineLaunch& a);

// ---- confidence-weighted edge-aware smoothing (k_smooth.hip): the fast global smoother; DESIGN.md section 4.25 ----
struct SmoothLaunch {
    const uint8_t* guide;  // dense interleaved 8U, C = 1 or 3 channels
    int C;
    const float* d;        // the map and its confidence: element i at d[i * stride], c[i * stride]
    const float* c;        // stride 1: two dense planes; 2: the interleaved {disparity, confidence} pairs of launch_confidence
    int stride;
    int H, W, T;           // T iterations, 1..8
    double lambda;
    const double* Wt;      // SmoothTable: [255 * C + 1]
    double* N;             // scratch, H * W doubles each: the two right-hand sides
    double* D;
    uint16_t* linkV;       // scratch, H * W each: the Wt index of a pixel's link to the pixel above / (transposed, [W][H]) to its left
    uint16_t* linkHT;
    double* cp;            // scratch, H * W doubles each: what a forward sweep leaves for its backward sweep
    double* fN;
    double* fD;
    float* out;            // [H][W]; must not alias d / c
};
// prep, 2 * T passes (row, column, row, ...), final: 2 * T + 2 launches
int launch_smooth(hipStream_t s, const SmoothLaunch& a);

// ---- bilateral-grid ASW, k_bilgrid.hip ----
// grid extents (last index per axis; both range axes share nz); ASW_ERR_BAD_ARGUMENT for rates <= 0 or a range axis too fine for LDS
int bilgrid_dims(int H, int W, double rate_s, double rate_r, int* nx, int* ny, int* nz);
int launch_bilgrid(hipStream_t s, const uint8_t* gl, const uint8_t* gr, int H, int W, double rate_s, double rate_r, int minD,
                   int numD, double* F, int* S, double* best, float* vol, float* disp);

// ---- cross-based support regions (k_cross.hip), DESIGN.md section 4.12 ----
// arms [H][W]: left | right << 8 | up << 16 | down << 24 of the view image (C = 1 or 3 channels), cnt [H][W]: the region size N
int launch_cross_arms(hipStream_t s, const uint8_t* img, int H, int W, int C, int win, int tau, uint32_t* arms, uint16_t* cnt);
// cost: a u8 cost volume [numD][H][W]; vol (optional) [numD][H][W]; disp [H][W]: WTA, strict '<' in ascending d
int launch_cross_aggregate(hipStream_t s, const uint8_t* cost, const uint32_t* arms, const uint16_t* cnt, int H, int W, int win,
                           int trunc, int minD, int numD, float* vol, float* disp);

// ---- census cost (k_census.hip), DESIGN.md section 4.13 ----
// gray [H][W] -> code [H][W]: the 62-bit census code of the 9 x 7 window, borders clamped; H <= 16 * 65535
int launch_census_transform(hipStream_t s, const uint8_t* gray, int H, int W, uint2* code);
// cost u8 [numD][H][W].  tables == nullptr: the Hamming distance of the two codes (0..62; L, R and C are not looked at);
// else tables = TA[256] | TC[64] (u8, each entry <= 127) and the cost is TA[AD of launch_cost_ad for L, R, C] + TC[Hamming].
// The staged rows must fit 160 KB of LDS, else ASW_ERR_BAD_ARGUMENT: W <= 10240 (Hamming), 9084 (C = 1), 7432 (C = 3).
int launch_cost_census(hipStream_t s, const uint8_t* L, const uint8_t* R, const uint2* codeL, const uint2* codeR, int H, int W, int C,
                       int disp_type, int minD, int numD, const uint8_t* tables, uint8_t* cost);

// ---- hooks for the batch scheduler (batch.hip) ----
int asw_internal_stage_slot(asw_ctx* ctx, int slot, int rows, int cols, int channels, Frame** out);
int asw_internal_enqueue_match(asw_ctx* ctx, int slot, int disparity_type, int algorithm, int win_size, int min_disparity,
                               int num_disparity);  // enqueues on ctx->stream, does not wait
int asw_internal_check_pair(const asw_image* l, const asw_image* r, const asw_image* d);

// ---- semi-global block matching (k_sgbm.hip): StereoSGBM MODE_SGBM_3WAY + filterSpeckles, DESIGN.md section 4.8 ----
struct SgbmLaunch {
    const uint8_t* L;  // dense interleaved 8U images, cn channels
    const uint8_t* R;
    int H, W, cn;
    int minD, D;       // D: a multiple of 16, at most 1024
    int w, ftzero, P1, P2, U, M;  // effective parameters (step 0)
    int speckle_window, speckle_range;
    int paths = ASW_SGBM_PATHS_3WAY;  // ASW_SGBM_PATH_* mask, a superset of the three (asw_sgbm_paths)
    bool census = false;  // asw_sgbm_census: L / R are the gray planes of gray_pair, cn and ftzero are not read
    void* scratch;     // sgbm_scratch_bytes()
    short* disp16;     // out [H][W], scaled by 16
    float* vol;        // optional S [D][H][W]
    AggMarks agg;      // optional: the clock's aggregate marks go around the path kernels (asw_timing::aggregate_ms)
};
size_t sgbm_scratch_bytes(int H, int W, int cn, int minD, int D);
int launch_sgbm(hipStream_t s, const SgbmLaunch& a);
int launch_filter_speckles(hipStream_t s, short* img, int H, int W, int new_val, int max_size, int max_diff,
                           int* scratch /* 2 * H * W ints */);
int launch_fill_s16(hipStream_t s, short* out, size_t n, short v);
// convertTo(CV_8U, 1/16) of a disp16 map: as f32 (the selector's CV_32F result) and as u8 (getDisparity_BM)
int launch_disp16_to_u8f(hipStream_t s, const short* disp16, size_t n, float* out);
int launch_disp16_to_u8(hipStream_t s, const short* disp16, size_t n, uint8_t* out);

// ---- block matching (k_bm.hip): StereoBM PREFILTER_XSOBEL + validateDisparity + filterSpeckles, DESIGN.md section 4.9 ----
struct BmLaunch {
    const uint8_t* L;  // dense 8U gray images
    const uint8_t* R;
    int H, W;
    int minD, D;       // D: a multiple of 16, at most 1024
    int w, cap, texture, U, M;  // blockSize, preFilterCap, textureThreshold, uniquenessRatio, disp12MaxDiff (< 0: no step 6)
    int speckle_window, speckle_range;  // step 7 runs when range >= 0 and window > 0 (range unscaled)
    void* scratch;     // bm_scratch_bytes()
    short* disp16;     // out [H][W], scaled by 16, FILTERED = 16 * (minD - 1)
    float* vol;        // optional SAD [D][H][W] (plane p <-> disparity minD + p), NaN where nothing is computed
    AggMarks agg;      // optional: the clock's aggregate marks go around k_bm_match (asw_timing::aggregate_ms)
};
size_t bm_scratch_bytes(int H, int W);
int launch_bm(hipStream_t s, const BmLaunch& a);
