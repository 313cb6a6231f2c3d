// Host-side pieces shared by the three translation units behind the C-ABI:
//   asw_context.hip  context, frame slots, host <-> HBM plumbing, pre/post-processing entry points
//   asw_methods.hip  the method table, the method runners (tables, scratch, launch sequences) and the selector
//   asw_api.hip      the per-method / cost-builder / building-block entry points of include/asw_mi355x.h
// MatchParams, MethodTraits and the decoding of the selector's two packed words live in asw_selector.h, which needs no HIP.
#pragma once
#include <type_traits>

#include "asw_internal.h"
#include "asw_selector.h"

inline unsigned blocks(size_t n, unsigned per) { return (unsigned)((n + per - 1) / per); }

// Kernels that keep D candidates in the lanes of one wavefront (k = c * 64 + lane) are templates on the candidates per lane:
// f(std::integral_constant<int, NPL>) with the smallest NPL of 1, 2, 4, 8, 16 that holds D; ASW_ERR_BAD_ARGUMENT beyond 1024
template <typename F>
int dispatch_npl(int D, F&& f)
{
    const int npl = (D + 63) / 64;
    if (npl <= 1) return f(std::integral_constant<int, 1>());
    if (npl <= 2) return f(std::integral_constant<int, 2>());
    if (npl <= 4) return f(std::integral_constant<int, 4>());
    if (npl <= 8) return f(std::integral_constant<int, 8>());
    if (npl <= 16) return f(std::integral_constant<int, 16>());
    return ASW_ERR_BAD_ARGUMENT;
}

// One row per selector value (asw_methods.hip: k_methods).  Everything the host layer knows about a method beyond its runner is a
// field of MethodTraits: asw_volume_planes, run_method, match_host, the word decoders and match_refined read the row, the runners
// of the inclusive ranges take their candidate count from it.
struct MethodInfo : MethodTraits {
    int algorithm;  // the ASW_ALG_* value == the row's index
    int (*run)(asw_ctx* ctx, Frame* f, const MatchParams& mp, bool keep_volume);  // null: the selector does not serve the value
};
const MethodInfo* method_info(int method);  // the row of a plain (decoded) selector value; null for a value outside the table

// AD-Census cost of a device pair into cost u8 [numD][H][W]: gray pair, two census transforms, then the
// Hamming distance alone (lambda_ad = 0) or TA[AD] + TC[Hamming] with the tables of the two lambdas (each 1..255)
int build_census_cost(asw_ctx* ctx, const uint8_t* dL, const uint8_t* dR, int H, int W, int channels, int disparity_type, int minD,
                      int numD, int lambda_ad, int lambda_census, uint8_t* cost);

int check_u8_image(const asw_image* im);
int check_pair(const asw_image* L, const asw_image* R);
int upload_image(asw_ctx* ctx, const asw_image* im, DevBuf& dst);
// pitched host rows <-> dense device rows on the context's stream (asw_context.hip)
hipError_t copy_rows(asw_ctx* ctx, void* dst, size_t dpitch, const void* src, size_t spitch, size_t rowbytes, size_t rows,
                     hipMemcpyKind kind);
// d: ASW_32F, rows x cols, 1 .. max_channels channels (2: disparity and confidence interleaved), step >= cols * 4 * channels
int check_disp_out(const asw_image* d, int rows, int cols, int max_channels = 1);
Frame* frame_slot(asw_ctx* ctx, int slot, bool create);
int upload_pair_into(asw_ctx* ctx, Frame* f, const asw_image* left, const asw_image* right);
// disp with 1 channel: the frame's map; with 2: the map and its confidence, computed here from the frame's kept volume unless the
// match already did (Frame::has_conf); ASW_ERR_NO_FRAME without either
int download_disparity_from(asw_ctx* ctx, Frame* f, asw_image* disp);
int download_volume_from(asw_ctx* ctx, Frame* f, float* out, size_t n_floats);
// 3 channels: cvtColor(BGR2GRAY) of both images into the scratch planes "grayL" / "grayR"; 1 channel: the images as they are
int gray_pair(asw_ctx* ctx, const uint8_t* dL, const uint8_t* dR, int channels, int H, int W, const uint8_t** gl, const uint8_t** gr);
int build_similarity_volume(asw_ctx* ctx, const uint8_t* dL, const uint8_t* dR, int H, int W, int minD, int numD,
                                   double regularity, double thresC, double thresG, float* cost,
                                   uint32_t* ord_scratch = nullptr, float2* scales = nullptr);
int run_ncc_cost(asw_ctx* ctx, const uint8_t* dL, const uint8_t* dR, int H, int W, int disparity_type, int win, int minD,
                        int numD, float* vol /* optional, un-normalised */, float* disp /* optional */, int nwta,
                        int channels = 3);
// StereoSGBM parameters as StereoSGBM::create takes them; sgbm_prepare validates them, derives the effective
// values of step 0 and sizes the scratch, run_sgbm enqueues the kernels on the context's stream
struct SgbmParams {
    int minD, numD, block_size, P1, P2, disp12_max_diff, pre_filter_cap, uniqueness_ratio, speckle_window_size, speckle_range, mode;
    int paths = ASW_SGBM_PATHS_3WAY;  // the ASW_SGBM_PATH_* mask of asw_sgbm_paths (mode stays 2)
    bool census = false;              // asw_sgbm_census: the census cost of DESIGN.md section 4.8c in place of steps 1-2 (pre_filter_cap unused)
};
int sgbm_prepare(asw_ctx* ctx, const SgbmParams& p, int H, int W, int cn, bool want_volume, SgbmLaunch* out);
// StereoBM parameters as StereoBM::create + its setters take them; bm_prepare validates them (step 0) and
// sizes the scratch
struct BmParams {
    int minD, numD, block_size, pre_filter_type, pre_filter_size, pre_filter_cap, texture_threshold, uniqueness_ratio,
        speckle_window_size, speckle_range, disp12_max_diff;
};
int bm_prepare(asw_ctx* ctx, const BmParams& p, int H, int W, BmLaunch* out);
// Left-right refinement.  check_refine_params: the argument rules of asw_refine_disparity; run_refine: the three
// kernels on device maps (out must not alias dl / dr), waits, reads the counters back; ASW_ERR_BAD_ARGUMENT when dl leaves its
// domain.  The mask stays in ctx->buf("refine_mask").  match_refined: both directions of `algorithm` on the frame's pair + run_refine
// with the frame's left image as guide; the refined map becomes the frame's disparity.
struct RefineParams {
    int minD, n;
    float max_diff;
    int win;
    double gamma_c, gamma_s;
};
int check_refine_params(const RefineParams& p, int rows, int cols, int channels);
int run_refine(asw_ctx* ctx, const uint8_t* guide, int channels, const float* dl, const float* dr, int H, int W, const RefineParams& p,
               float* out, int* n_rejected, int* n_unfillable);
int match_refined(asw_ctx* ctx, Frame* f, int algorithm, int win_size, int min_disparity, int num_disparity, float max_diff,
                  int refine_win, double gamma_c, double gamma_s, int* n_rejected, int* n_unfillable);
// Confidence-weighted smoothing, the refinement family's win_size / refine_win with ASW_REFINE_SMOOTH set.
// check_smooth_params: the frame-size rule of check_refine_params, the word, sigma_c and lambda, a mask asked for, the channels, in
// that order; fills *iterations.  run_smooth: the 2 T + 2 kernels on a device map and confidence (element stride 1 or 2, see
// SmoothLaunch) into `out`, enqueued on the context's stream; does not wait.  match_refined under the flag: ONE DISPARITY_LEFT
// match of `algorithm` with its confidence, smoothed with the frame's left image as guide into the frame's disparity.
int check_smooth_params(int rows, int cols, int channels, int word, double sigma_c, double lambda, bool wants_mask, int* iterations);
int run_smooth(asw_ctx* ctx, const uint8_t* guide, int channels, const float* d, const float* c, int stride, int H, int W,
               int iterations, double sigma_c, double lambda, float* out);
// confidence: also fill f->dconf from the volume the call returns (implies the volume is computed, as a sub-pixel flag does)
int run_method(asw_ctx* ctx, Frame* f, int algorithm, const MatchParams& mp, bool keep_volume, bool sync = true,
               bool confidence = false);
int match_host(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp, int algorithm,
                      const MatchParams& mp, float* cost_volume_out, size_t cost_volume_floats);
