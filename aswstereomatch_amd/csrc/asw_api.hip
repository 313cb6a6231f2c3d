// Per-method, cost-builder and building-block entry points of the C-ABI (include/asw_mi355x.h): argument checking, staging
// of caller-owned host buffers, dispatch to the method runners.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "asw_internal.h"
#include "asw_host.h"

// Host buffers in, host buffers out.  Works on the context's private frame: the caller's resident slots (asw_upload_pair /
// asw_match_resident) are never touched by a one-call entry point.
int match_host(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp, int algorithm,
                      const MatchParams& mp, float* cost_volume_out, size_t cost_volume_floats)
{
    if (!ctx) return ASW_ERR_BAD_ARGUMENT;
    ASW_TRY(check_pair(left, right));
    ASW_TRY(check_disp_out(disp, left->rows, left->cols, 2));  // 2 channels: disparity and confidence, interleaved
    if (cost_volume_out) {  // the caller states what its buffer holds; a short one is refused before anything is written
        const MethodInfo* m = method_info(algorithm);
        if (m && m->run && m->no_volume) return ASW_ERR_BAD_ARGUMENT;  // the selector's SGBM has no volume (asw_sgbm has S)
        const int planes = asw_volume_planes(algorithm, mp.numD);
        if (planes > 0 && cost_volume_floats < (size_t)planes * left->rows * left->cols) return ASW_ERR_BAD_ARGUMENT;
    }
    ASW_HIP_TRY(hipSetDevice(ctx->device));
    Frame* f = &ctx->host_frame;
    ASW_TRY(upload_pair_into(ctx, f, left, right));
    ASW_TRY(run_method(ctx, f, algorithm, mp, cost_volume_out != nullptr, true, disp->channels == 2));
    ASW_TRY(download_disparity_from(ctx, f, disp));
    if (cost_volume_out) {
        if (f->vol_floats > cost_volume_floats) return ASW_ERR_BAD_ARGUMENT;
        ASW_TRY(download_volume_from(ctx, f, cost_volume_out, f->vol_floats));
    }
    return ASW_OK;
}

extern "C" int asw_volume_planes(int algorithm, int num_disparity)
{
    if (decode_algorithm(algorithm, &algorithm, nullptr, method_info) != ASW_OK) return 0;
    const MethodInfo* m = method_info(algorithm);
    return m ? m->planes(num_disparity) : 0;
}

extern "C" int asw_stereo_match(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp,
                                int disparity_type, int algorithm, int win_size, int min_disparity,
                                int num_disparity, float* cost_volume_out, size_t cost_volume_floats)
{
    return match_host(ctx, left, right, disp, algorithm, match_params(disparity_type, win_size, min_disparity, num_disparity),
                      cost_volume_out, cost_volume_floats);
}

extern "C" int asw_aggregate_bilateral(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp,
                                       double gamma_c, double gamma_g, int disparity_type, int win_size,
                                       int min_disparity, int num_disparity, float* cost_volume_out, size_t cost_volume_floats)
{
    MatchParams mp = match_params(disparity_type, win_size, min_disparity, num_disparity);
    mp.gamma_c = gamma_c; mp.gamma_g = gamma_g;
    return match_host(ctx, left, right, disp, ASW_ALG_ADAPTIVE_WEIGHT, mp, cost_volume_out, cost_volume_floats);
}

extern "C" int asw_aggregate_direct8(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp,
                                     int disparity_type, int win_size, int min_disparity, int num_disparity,
                                     float* cost_volume_out, size_t cost_volume_floats)
{
    return match_host(ctx, left, right, disp, ASW_ALG_ADAPTIVE_WEIGHT_8DIRECT,
                      match_params(disparity_type, win_size, min_disparity, num_disparity), cost_volume_out, cost_volume_floats);
}

// ------------------------------------------------------------------------------------------
// cost builders and small building blocks
// ------------------------------------------------------------------------------------------
// the caller's two images into the stage buffers "stageL" / "stageR" (shared by every building block on purpose)
static int upload_stage_pair(asw_ctx* ctx, const asw_image* a, const asw_image* b, const uint8_t** da, const uint8_t** db)
{
    DevBuf& sa = ctx->buf("stageL");
    DevBuf& sb = ctx->buf("stageR");
    ASW_TRY(upload_image(ctx, a, sa));
    ASW_TRY(upload_image(ctx, b, sb));
    *da = sa.as<uint8_t>(); *db = sb.as<uint8_t>();
    return ASW_OK;
}

// a device result into the caller's buffer; returns once it is there
static int download_sync(asw_ctx* ctx, void* dst, const void* src, size_t bytes)
{
    ASW_HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    ASW_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ASW_OK;
}

static int cost_ad_common(asw_ctx* ctx, const asw_image* left, const asw_image* right, uint8_t* cost, int disparity_type,
                          int do_thresh, int threshold, int minD, int numD)
{
    if (!ctx || !cost) return ASW_ERR_BAD_ARGUMENT;
    ASW_TRY(check_pair(left, right));
    if (numD <= 0 || minD < 0) return ASW_ERR_BAD_ARGUMENT;
    if (left->channels != 1 && left->channels != 3) return ASW_ERR_UNSUPPORTED_LAYOUT;  // no branch in M.cpp:227,264
    if (disparity_type != ASW_DISPARITY_LEFT && disparity_type != ASW_DISPARITY_RIGHT) return ASW_ERR_BAD_ARGUMENT;
    ASW_HIP_TRY(hipSetDevice(ctx->device));
    const int H = left->rows, W = left->cols, C = left->channels;
    const uint8_t *dl, *dr;
    DevBuf& dc = ctx->buf("cost_u8");
    ASW_TRY(upload_stage_pair(ctx, left, right, &dl, &dr));
    size_t bytes = (size_t)numD * H * W;
    ASW_TRY(dc.ensure(bytes));
    ASW_TRY(launch_cost_ad(ctx->stream, dl, dr, H, W, C, disparity_type, minD, numD, do_thresh, threshold, dc.as<uint8_t>()));
    return download_sync(ctx, cost, dc.p, bytes);
}

extern "C" int asw_cost_ad(asw_ctx* ctx, const asw_image* left, const asw_image* right, uint8_t* cost,
                           int disparity_type, int min_disparity, int num_disparity)
{
    return cost_ad_common(ctx, left, right, cost, disparity_type, 0, 0, min_disparity, num_disparity);
}

// asw_cost_census (lambda_ad = 0: the Hamming distance alone) and asw_cost_adcensus, the header's inline forms over asw_cost_tad
static int cost_census_common(asw_ctx* ctx, const asw_image* left, const asw_image* right, uint8_t* cost, int disparity_type,
                              int lambda_ad, int lambda_census, int minD, int numD)
{
    if (!ctx || !cost) return ASW_ERR_BAD_ARGUMENT;
    ASW_TRY(check_pair(left, right));
    if (numD <= 0 || minD < 0) return ASW_ERR_BAD_ARGUMENT;
    if (left->channels != 1 && left->channels != 3) return ASW_ERR_UNSUPPORTED_LAYOUT;
    if (disparity_type != ASW_DISPARITY_LEFT && disparity_type != ASW_DISPARITY_RIGHT) return ASW_ERR_BAD_ARGUMENT;
    ASW_HIP_TRY(hipSetDevice(ctx->device));
    const int H = left->rows, W = left->cols;
    const uint8_t *dl, *dr;
    DevBuf& dc = ctx->buf("cost_u8");
    ASW_TRY(upload_stage_pair(ctx, left, right, &dl, &dr));
    const size_t bytes = (size_t)numD * H * W;
    ASW_TRY(dc.ensure(bytes));
    ASW_TRY(build_census_cost(ctx, dl, dr, H, W, left->channels, disparity_type, minD, numD, lambda_ad, lambda_census, dc.as<uint8_t>()));
    return download_sync(ctx, cost, dc.p, bytes);
}

extern "C" int asw_cost_tad(asw_ctx* ctx, const asw_image* left, const asw_image* right, uint8_t* cost,
                            int disparity_type, int threshold_t, int min_disparity, int num_disparity)
{
    if (threshold_t >= ASW_COST_CENSUS_PARAMS) {  // asw_cost_census / asw_cost_adcensus: bits 8..15 = lambda_ad, 0..7 = lambda_census
        const int la = (threshold_t >> 8) & 0xFF, lc = threshold_t & 0xFF;
        if ((threshold_t & 0x3FFF0000) || (la == 0) != (lc == 0)) return ASW_ERR_BAD_ARGUMENT;
        return cost_census_common(ctx, left, right, cost, disparity_type, la, lc, min_disparity, num_disparity);
    }
    return cost_ad_common(ctx, left, right, cost, disparity_type, 1, threshold_t, min_disparity, num_disparity);
}

extern "C" int asw_cost_sd(asw_ctx* ctx, const asw_image* left, const asw_image* right, uint8_t* cost,
                           int disparity_type, int min_disparity, int num_disparity)
{
    return cost_ad_common(ctx, left, right, cost, disparity_type, 2, 0, min_disparity, num_disparity);
}

extern "C" int asw_bgr2gray(asw_ctx* ctx, const asw_image* bgr, uint8_t* gray)
{
    if (!ctx || !gray) return ASW_ERR_BAD_ARGUMENT;
    ASW_TRY(check_u8_image(bgr));
    if (bgr->channels != 3) return ASW_ERR_UNSUPPORTED_LAYOUT;
    ASW_HIP_TRY(hipSetDevice(ctx->device));
    DevBuf& d = ctx->buf("stageL");
    DevBuf& g = ctx->buf("grayL");
    ASW_TRY(upload_image(ctx, bgr, d));
    size_t n = (size_t)bgr->rows * bgr->cols;
    ASW_TRY(g.ensure(n));
    ASW_TRY(launch_bgr2gray(ctx->stream, d.as<uint8_t>(), bgr->rows, bgr->cols, g.as<uint8_t>(), ctx->gray_bits));
    return download_sync(ctx, gray, g.p, n);
}

extern "C" int asw_wta(asw_ctx* ctx, const float* cost_volume, int n, int rows, int cols, int min_disparity, float* disp)
{
    if (!ctx || !cost_volume || !disp || n <= 0 || rows <= 0 || cols <= 0) return ASW_ERR_BAD_ARGUMENT;
    ASW_HIP_TRY(hipSetDevice(ctx->device));
    DevBuf& v = ctx->buf("wta_vol");
    DevBuf& d = ctx->buf("wta_disp");
    size_t plane = (size_t)rows * cols;
    ASW_TRY(v.ensure(plane * n * 4));
    ASW_TRY(d.ensure(plane * 4));
    ASW_HIP_TRY(hipMemcpyAsync(v.p, cost_volume, plane * n * 4, hipMemcpyHostToDevice, ctx->stream));
    ASW_TRY(launch_wta(ctx->stream, v.as<float>(), n, rows, cols, min_disparity, d.as<float>()));
    return download_sync(ctx, disp, d.p, plane * 4);
}

extern "C" int asw_lr_check(asw_ctx* ctx, const float* disp_left, const float* disp_right, int rows, int cols, float max_diff,
                            float invalid_value, float* out, int* n_invalid)
{
    if (!ctx || !disp_left || !disp_right || !out || rows <= 0 || cols <= 0 || !(max_diff >= 0)) return ASW_ERR_BAD_ARGUMENT;
    ASW_HIP_TRY(hipSetDevice(ctx->device));
    const size_t plane = (size_t)rows * cols;
    DevBuf& a = ctx->buf("lr_left");
    DevBuf& b = ctx->buf("lr_right");
    DevBuf& o = ctx->buf("lr_out");
    DevBuf& c = ctx->buf("lr_count");
    ASW_TRY(a.ensure(plane * 4));
    ASW_TRY(b.ensure(plane * 4));
    ASW_TRY(o.ensure(plane * 4));
    ASW_TRY(c.ensure(sizeof(unsigned)));
    ASW_HIP_TRY(hipMemcpyAsync(a.p, disp_left, plane * 4, hipMemcpyHostToDevice, ctx->stream));
    ASW_HIP_TRY(hipMemcpyAsync(b.p, disp_right, plane * 4, hipMemcpyHostToDevice, ctx->stream));
    ASW_TRY(launch_lr_check(ctx->stream, a.as<float>(), b.as<float>(), rows, cols, max_diff, invalid_value, o.as<float>(), c.as<unsigned>()));
    unsigned bad = 0;
    ASW_HIP_TRY(hipMemcpyAsync(out, o.p, plane * 4, hipMemcpyDeviceToHost, ctx->stream));
    ASW_HIP_TRY(hipMemcpyAsync(&bad, c.p, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    ASW_HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (n_invalid) *n_invalid = (int)bad;
    return ASW_OK;
}

extern "C" int asw_aggregate_guided(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp,
                                    int disparity_type, double eps, int win_size, int min_disparity, int num_disparity,
                                    float* cost_volume_out, size_t cost_volume_floats)
{
    MatchParams mp = match_params(disparity_type, win_size, min_disparity, num_disparity);
    mp.eps = eps;
    return match_host(ctx, left, right, disp, ASW_ALG_ADAPTIVE_WEIGHT_GUIDED_FILTER, mp, cost_volume_out, cost_volume_floats);
}

extern "C" int asw_aggregate_guided2(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp,
                                     int disparity_type, double eps, int win_size, int min_disparity, int num_disparity,
                                     float* cost_volume_out, size_t cost_volume_floats)
{
    MatchParams mp = match_params(disparity_type, win_size, min_disparity, num_disparity);
    mp.eps = eps;
    return match_host(ctx, left, right, disp, ASW_ALG_ADAPTIVE_WEIGHT_GUIDED_FILTER_2, mp, cost_volume_out, cost_volume_floats);
}

extern "C" int asw_cost_similarity(asw_ctx* ctx, const asw_image* left, const asw_image* right, float* cost,
                                   double regularity, double thres_c, double thres_g, int disparity_type, int win_size,
                                   int min_disparity, int num_disparity)
{
    if (!ctx || !cost) return ASW_ERR_BAD_ARGUMENT;
    if (win_size != 0 && win_size % 2 == 0) return ASW_ERR_EVEN_WINDOW;  // M.cpp:654-657 (before anything else)
    ASW_TRY(check_pair(left, right));
    if (num_disparity <= 0 || min_disparity < 0 || win_size < 0) return ASW_ERR_BAD_ARGUMENT;
    // only DISPARITY_LEFT + 3 channels executes in the reference; the other branches throw (App. B-7)
    if (left->channels != 3 || disparity_type != ASW_DISPARITY_LEFT) return ASW_ERR_UNSUPPORTED_LAYOUT;
    ASW_HIP_TRY(hipSetDevice(ctx->device));
    const int H = left->rows, W = left->cols, n = num_disparity, h = win_size / 2;
    const uint8_t *dl, *dr;
    DevBuf& raw = ctx->buf("g_raw");
    ASW_TRY(upload_stage_pair(ctx, left, right, &dl, &dr));
    ASW_TRY(raw.ensure((size_t)n * H * W * 4));
    ASW_TRY(build_similarity_volume(ctx, dl, dr, H, W, min_disparity, n, regularity, thres_c, thres_g, raw.as<float>()));
    const float* src = raw.as<float>();
    size_t out_floats = (size_t)n * H * W;
    if (win_size > 0) {
        DevBuf& pad = ctx->buf("g_pad");
        out_floats = (size_t)n * (H + 2 * h) * (W + 2 * h);
        ASW_TRY(pad.ensure(out_floats * 4));
        ASW_TRY(launch_pad_reflect(ctx->stream, raw.as<float>(), n, H, W, h, pad.as<float>()));
        src = pad.as<float>();
    }
    return download_sync(ctx, cost, src, out_floats * 4);
}

extern "C" int asw_cost_sad(asw_ctx* ctx, const asw_image* left, const asw_image* right, float* cost, int disparity_type,
                            int win_size, int min_disparity, int num_disparity)
{
    if (!ctx || !cost) return ASW_ERR_BAD_ARGUMENT;
    ASW_TRY(check_pair(left, right));
    if (win_size % 2 == 0) return ASW_ERR_EVEN_WINDOW;  // M.cpp:2458-2462
    if (num_disparity <= 0 || min_disparity < 0 || win_size < 1 || win_size > walk_max_kernel()) return ASW_ERR_BAD_ARGUMENT;
    if (left->channels != 3 && left->channels != 1) return ASW_ERR_UNSUPPORTED_LAYOUT;
    if (disparity_type != ASW_DISPARITY_LEFT && disparity_type != ASW_DISPARITY_RIGHT) return ASW_ERR_BAD_ARGUMENT;
    ASW_HIP_TRY(hipSetDevice(ctx->device));
    const int H = left->rows, W = left->cols, n = num_disparity;
    const uint8_t *pl, *pr;
    DevBuf& raw = ctx->buf("g_raw");
    ASW_TRY(upload_stage_pair(ctx, left, right, &pl, &pr));
    ASW_TRY(raw.ensure((size_t)n * H * W * 4));
    ASW_TRY(gray_pair(ctx, pl, pr, left->channels, H, W, &pl, &pr));  // M.cpp:2446-2456
    ASW_TRY(launch_cost_sad(ctx->stream, pl, pr, H, W, disparity_type, win_size, min_disparity, n, raw.as<float>()));
    return download_sync(ctx, cost, raw.p, (size_t)n * H * W * 4);
}

// getCostSAD_d (M.cpp:2442-2503) as the reference declares it: one disparity, the other view pre-bordered by the caller
extern "C" int asw_cost_sad_d(asw_ctx* ctx, const asw_image* left, const asw_image* right, float* cost, int disparity,
                              int disparity_type, int win_size)
{
    if (!ctx || !cost) return ASW_ERR_BAD_ARGUMENT;
    ASW_TRY(check_u8_image(left));
    ASW_TRY(check_u8_image(right));
    if ((left->channels != 1 && left->channels != 3) || (right->channels != 1 && right->channels != 3)) return ASW_ERR_UNSUPPORTED_LAYOUT;
    if (win_size % 2 == 0) return ASW_ERR_EVEN_WINDOW;  // M.cpp:2458-2462
    if (win_size < 1 || win_size > walk_max_kernel()) return ASW_ERR_BAD_ARGUMENT;
    if (disparity_type != ASW_DISPARITY_LEFT && disparity_type != ASW_DISPARITY_RIGHT) return ASW_ERR_BAD_ARGUMENT;
    const bool lref = disparity_type == ASW_DISPARITY_LEFT;
    const asw_image* ref = lref ? left : right;   // the view the cost plane belongs to
    const asw_image* bord = lref ? right : left;  // the bordered (wider) other view
    if (ref->rows != bord->rows) return ASW_ERR_BAD_ARGUMENT;  // absdiff of unequal sizes throws in the reference
    const int H = ref->rows, W = ref->cols, Wb = bord->cols;
    if (Wb <= W) return ASW_ERR_SIZE_MISMATCH;  // M.cpp:2473-2476 / 2488-2491: return Mat()
    const int x0 = lref ? Wb - W - disparity : disparity;  // M.cpp:2478 / 2493
    if (x0 < 0 || x0 + W > Wb) return ASW_ERR_BAD_ARGUMENT;
    ASW_HIP_TRY(hipSetDevice(ctx->device));
    const uint8_t *pref, *pbord;
    DevBuf& gref = ctx->buf("grayL");
    DevBuf& gbord = ctx->buf("sadd_gray_wide");
    DevBuf& gcrop = ctx->buf("grayR");
    DevBuf& raw = ctx->buf("g_raw");
    ASW_TRY(upload_stage_pair(ctx, ref, bord, &pref, &pbord));
    ASW_TRY(gref.ensure((size_t)H * W));
    ASW_TRY(gbord.ensure((size_t)H * Wb));
    ASW_TRY(gcrop.ensure((size_t)H * W));
    ASW_TRY(raw.ensure((size_t)H * W * 4));
    if (ref->channels == 3) {  // M.cpp:2446-2456
        ASW_TRY(launch_bgr2gray(ctx->stream, pref, H, W, gref.as<uint8_t>(), ctx->gray_bits));
        pref = gref.as<uint8_t>();
    }
    if (bord->channels == 3) {
        ASW_TRY(launch_bgr2gray(ctx->stream, pbord, H, Wb, gbord.as<uint8_t>(), ctx->gray_bits));
        pbord = gbord.as<uint8_t>();
    }
    // the ROI of the bordered view as a dense plane; then |ref - roi| -> f32 -> boxFilter mean is launch_cost_sad at offset 0
    ASW_HIP_TRY(hipMemcpy2DAsync(gcrop.p, (size_t)W, pbord + x0, (size_t)Wb, (size_t)W, H, hipMemcpyDeviceToDevice, ctx->stream));
    ASW_TRY(launch_cost_sad(ctx->stream, pref, gcrop.as<uint8_t>(), H, W, ASW_DISPARITY_LEFT, win_size, 0, 1, raw.as<float>()));
    return download_sync(ctx, cost, raw.p, (size_t)H * W * 4);
}

extern "C" int asw_cost_ncc(asw_ctx* ctx, const asw_image* left, const asw_image* right, float* cost, int disparity_type,
                            int win_size, int min_disparity, int num_disparity, int normalized)
{
    if (!ctx || !cost) return ASW_ERR_BAD_ARGUMENT;
    ASW_TRY(check_pair(left, right));
    if (win_size % 2 == 0) return ASW_ERR_EVEN_WINDOW;  // M.cpp:939-942
    if (num_disparity <= 0 || min_disparity < 0 || win_size < 1 || win_size > std::min(ncc_max_window(), walk_max_kernel()))
        return ASW_ERR_BAD_ARGUMENT;  // run_ncc_cost's limit, before the upload
    if (left->channels != 3 && left->channels != 1) return ASW_ERR_UNSUPPORTED_LAYOUT;
    if (disparity_type != ASW_DISPARITY_LEFT && disparity_type != ASW_DISPARITY_RIGHT) return ASW_ERR_BAD_ARGUMENT;
    ASW_HIP_TRY(hipSetDevice(ctx->device));
    const int H = left->rows, W = left->cols, n = num_disparity;
    const size_t plane = (size_t)H * W;
    const uint8_t *dl, *dr;
    DevBuf& raw = ctx->buf("g_raw");
    ASW_TRY(upload_stage_pair(ctx, left, right, &dl, &dr));
    ASW_TRY(raw.ensure(plane * n * 4));
    ASW_TRY(run_ncc_cost(ctx, dl, dr, H, W, disparity_type, win_size, min_disparity, n, raw.as<float>(), nullptr, 0, left->channels));
    if (normalized) {  // normalize(curCost_, curCost_norm, 0, 1, NORM_MINMAX), M.cpp:981-983
        DevBuf& ord = ctx->buf("g_ord");
        DevBuf& psc = ctx->buf("g_pscales");
        ASW_TRY(ord.ensure((size_t)(2 * n + 2) * 4));
        ASW_TRY(psc.ensure((size_t)n * sizeof(float2)));
        ASW_TRY(launch_slice_scales(ctx->stream, raw.as<float>(), n, plane, ord.as<uint32_t>(), psc.as<float2>()));
        ASW_TRY(launch_apply_scales(ctx->stream, raw.as<float>(), n, plane, psc.as<float2>()));
    }
    return download_sync(ctx, cost, raw.p, plane * n * 4);
}

extern "C" int asw_ncc_disparity(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp, int disparity_type,
                                 int win_size, int min_disparity, int num_disparity)
{
    return match_host(ctx, left, right, disp, ASW_ALG_NCC, match_params(disparity_type, win_size, min_disparity, num_disparity), nullptr,
                      0);
}

extern "C" int asw_aggregate_guided3(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp,
                                     int disparity_type, double eps, int win_size, int min_disparity, int num_disparity,
                                     float* cost_volume_out, size_t cost_volume_floats)
{
    MatchParams mp = match_params(disparity_type, win_size, min_disparity, num_disparity);
    mp.eps = eps;
    return match_host(ctx, left, right, disp, ASW_ALG_ADAPTIVE_WEIGHT_GUIDED_FILTER_3, mp, cost_volume_out, cost_volume_floats);
}

extern "C" int asw_guided_filter(asw_ctx* ctx, const asw_image* guide, const float* p, float* q, int r, double eps)
{
    if (!ctx || !p || !q) return ASW_ERR_BAD_ARGUMENT;
    ASW_TRY(check_u8_image(guide));
    if (guide->channels != 3 && guide->channels != 6) return ASW_ERR_UNSUPPORTED_LAYOUT;  // M.cpp:2732-2734
    if (r < 1 || r > walk_max_kernel()) return ASW_ERR_BAD_ARGUMENT;  // r is the box side of every walk
    ASW_HIP_TRY(hipSetDevice(ctx->device));
    const int H = guide->rows, W = guide->cols, C = guide->channels;
    const size_t plane = (size_t)H * W;
    DevBuf& dg = ctx->buf("stageL");
    DevBuf& raw = ctx->buf("g_raw");
    DevBuf& ord = ctx->buf("g_ord");
    DevBuf& psc = ctx->buf("g_pscales");
    DevBuf& gsc = ctx->buf("g_gscales");
    DevBuf& stats = ctx->buf("g_stats");
    DevBuf& ab = ctx->buf("g_ab");
    DevBuf& qv = ctx->buf("g_q1");
    DevBuf& pxa = ctx->buf("bgrxL");
    DevBuf& pxb = ctx->buf("bgrxR");
    ASW_TRY(upload_image(ctx, guide, dg));
    ASW_TRY(raw.ensure(plane * 4));
    ASW_TRY(ord.ensure(4 * 4));
    ASW_TRY(psc.ensure(sizeof(float2)));
    ASW_TRY(gsc.ensure(sizeof(float2)));
    ASW_TRY(stats.ensure(guided_stats_floats(C, 1, H, W) * 4));
    const size_t ab_floats = guided_ab_floats(C, 1, H, W, r);  // two-pass path: a caller's P may hold NaN, the fused walk does not apply
    ASW_TRY(ab.ensure(ab_floats * 4));
    ASW_TRY(qv.ensure(plane * 4));
    ASW_TRY(pxa.ensure((plane + 4) * 4));  // + slack: the q pass reads the guide words of a lane's two columns as one pair, the last one may start at column W-1
    ASW_TRY(pxb.ensure((plane + 4) * 4));
    ASW_TRY(launch_pack_words(ctx->stream, dg.as<uint8_t>(), H, W, C, 0, pxa.as<uint32_t>()));
    if (C == 6) ASW_TRY(launch_pack_words(ctx->stream, dg.as<uint8_t>(), H, W, C, 1, pxb.as<uint32_t>()));
    ASW_HIP_TRY(hipMemcpyAsync(raw.p, p, plane * 4, hipMemcpyHostToDevice, ctx->stream));
    ASW_TRY(launch_u8_scale(ctx->stream, dg.as<uint8_t>(), plane * C, ord.as<uint32_t>() + 2, gsc.as<float2>()));  // M.cpp:2774
    ASW_TRY(launch_slice_scales(ctx->stream, raw.as<float>(), 1, plane, ord.as<uint32_t>(), psc.as<float2>()));     // M.cpp:2775
    GuidedLaunch a;
    a.shiftA = 0; a.shiftB = 0; a.C = C; a.guide_per_slice = 0;
    a.nan_safe = 1;  // p is the caller's: it may hold NaN
    a.guideA = pxa.as<uint32_t>(); a.guideB = C == 6 ? pxb.as<uint32_t>() : nullptr;
    a.gscales = gsc.as<float2>(); a.P = raw.as<float>(); a.pscales = psc.as<float2>();
    a.H = H; a.W = W; a.n = 1; a.r = r; a.minD = 0; a.eps = eps;
    a.stats = stats.as<float>(); a.rep_scratch = nullptr; a.ab = ab.as<float>(); a.q = qv.as<float>();
    a.ab_floats = ab_floats; a.fused = 0;
    a.tune = &ctx->tune;
    ASW_TRY(launch_guided(ctx->stream, a));
    return download_sync(ctx, q, qv.p, plane * 4);
}

extern "C" int asw_aggregate_geodesic(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp,
                                      int disparity_type, int win_size, int min_disparity, int num_disparity,
                                      float* cost_volume_out, size_t cost_volume_floats)
{
    return match_host(ctx, left, right, disp, ASW_ALG_ADAPTIVE_WEIGHT_GEODESIC,
                      match_params(disparity_type, win_size, min_disparity, num_disparity), cost_volume_out, cost_volume_floats);
}

extern "C" int asw_geodesic_dist(asw_ctx* ctx, const asw_image* img, float* out, int win_size, int iter_time)
{
    if (!ctx || !out) return ASW_ERR_BAD_ARGUMENT;
    ASW_TRY(check_u8_image(img));
    if (win_size % 2 == 0) return ASW_ERR_EVEN_WINDOW;  // M.cpp:1394-1397
    if (img->channels != 3) return ASW_ERR_UNSUPPORTED_LAYOUT;
    if (win_size < 1 || win_size > 35 || iter_time < 0) return ASW_ERR_BAD_ARGUMENT;
    ASW_HIP_TRY(hipSetDevice(ctx->device));
    const int H = img->rows, W = img->cols, cells = win_size * win_size;
    const size_t plane = (size_t)H * W;
    DevBuf& di = ctx->buf("stageL");
    DevBuf& px = ctx->buf("bgrxL");
    DevBuf& pf = ctx->buf("geoPlanesF");
    DevBuf& wo = ctx->buf("geoWindows");
    ASW_TRY(upload_image(ctx, img, di));
    ASW_TRY(px.ensure(plane * 4));
    ASW_TRY(pf.ensure(plane * cells * 4));
    ASW_TRY(wo.ensure(plane * cells * 4));
    ASW_TRY(launch_pack_bgrx(ctx->stream, di.as<uint8_t>(), H, W, px.as<uint32_t>()));
    ASW_TRY(launch_geodesic_weights_f32(ctx->stream, px.as<uint32_t>(), H, W, win_size, iter_time, pf.as<float>()));
    ASW_TRY(launch_planes_to_windows(ctx->stream, pf.as<float>(), H, W, cells, wo.as<float>()));
    return download_sync(ctx, out, wo.p, plane * cells * 4);
}

extern "C" int asw_aggregate_blo1(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp,
                                  int disparity_type, double sample_rate_r, int win_size, int min_disparity,
                                  int num_disparity, float* cost_volume_out, size_t cost_volume_floats)
{
    MatchParams mp = match_params(disparity_type, win_size, min_disparity, num_disparity);
    mp.blo_rate_r = sample_rate_r;
    return match_host(ctx, left, right, disp, ASW_ALG_ADAPTIVE_WEIGHT_BLO1, mp, cost_volume_out, cost_volume_floats);
}

extern "C" int asw_aggregate_bilgrid(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp,
                                     int disparity_type, double sample_rate_s, double sample_rate_r, int min_disparity,
                                     int num_disparity, float* cost_volume_out, size_t cost_volume_floats)
{
    MatchParams mp = match_params(disparity_type, 1, min_disparity, num_disparity);
    mp.grid_rate_s = sample_rate_s; mp.grid_rate_r = sample_rate_r;
    return match_host(ctx, left, right, disp, ASW_ALG_ADAPTIVE_WEIGHT_BILATERAL_GRID, mp, cost_volume_out, cost_volume_floats);
}

extern "C" int asw_aggregate_wmedian(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp,
                                     int disparity_type, int win_size, double rate_s, double rate_r, int min_disparity,
                                     int num_disparity, float* cost_volume_out, size_t cost_volume_floats)
{
    MatchParams mp = match_params(disparity_type, win_size, min_disparity, num_disparity);
    mp.rate_s = rate_s; mp.rate_r = rate_r;
    return match_host(ctx, left, right, disp, ASW_ALG_ADAPTIVE_WEIGHT_MEDIAN, mp, cost_volume_out, cost_volume_floats);
}

// ---- left-right refinement ----
extern "C" int asw_refine_disparity(asw_ctx* ctx, const asw_image* guide, const float* disp_left, const float* disp_right,
                                    int min_disparity, int num_values, float max_diff, int win_size, double gamma_c, double gamma_s,
                                    float* out, uint8_t* mask_out, int* n_rejected, int* n_unfillable)
{
    if (!ctx || !disp_left || !disp_right || !out) return ASW_ERR_BAD_ARGUMENT;
    ASW_TRY(check_u8_image(guide));
    const int H = guide->rows, W = guide->cols;
    const bool smooth = win_size > 0 && (win_size & ASW_REFINE_SMOOTH);  // asw_smooth_disparity: no window has bit 30
    RefineParams rp;
    rp.minD = min_disparity; rp.n = num_values; rp.max_diff = max_diff; rp.win = win_size; rp.gamma_c = gamma_c; rp.gamma_s = gamma_s;
    int T = 0;
    if (smooth)  // disp_right is the confidence, gamma_c sigma_c, gamma_s lambda; the map's domain and max_diff are not looked at
        ASW_TRY(check_smooth_params(H, W, guide->channels, win_size, gamma_c, gamma_s, mask_out != nullptr, &T));
    else
        ASW_TRY(check_refine_params(rp, H, W, guide->channels));
    ASW_HIP_TRY(hipSetDevice(ctx->device));
    const size_t plane = (size_t)H * W;
    DevBuf& dg = ctx->buf("stageL");
    DevBuf& a = ctx->buf("refine_left");
    DevBuf& b = ctx->buf("refine_right");
    DevBuf& o = ctx->buf("refine_out");
    ASW_TRY(upload_image(ctx, guide, dg));
    ASW_TRY(a.ensure(plane * 4));
    ASW_TRY(b.ensure(plane * 4));
    ASW_TRY(o.ensure(plane * 4));
    ASW_HIP_TRY(hipMemcpyAsync(a.p, disp_left, plane * 4, hipMemcpyHostToDevice, ctx->stream));
    ASW_HIP_TRY(hipMemcpyAsync(b.p, disp_right, plane * 4, hipMemcpyHostToDevice, ctx->stream));
    if (smooth) {  // the counts are the cross-check's: not written
        ASW_TRY(run_smooth(ctx, dg.as<uint8_t>(), guide->channels, a.as<float>(), b.as<float>(), 1, H, W, T, gamma_c, gamma_s,
                           o.as<float>()));
        return download_sync(ctx, out, o.p, plane * 4);
    }
    int rejected = 0, unfillable = 0;
    ASW_TRY(run_refine(ctx, dg.as<uint8_t>(), guide->channels, a.as<float>(), b.as<float>(), H, W, rp, o.as<float>(), &rejected,
                       &unfillable));  // a map outside the domain returns here: nothing of the caller's has been written
    ASW_HIP_TRY(hipMemcpyAsync(out, o.p, plane * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (mask_out) ASW_HIP_TRY(hipMemcpyAsync(mask_out, ctx->buf("refine_mask").p, plane, hipMemcpyDeviceToHost, ctx->stream));
    ASW_HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (n_rejected) *n_rejected = rejected;
    if (n_unfillable) *n_unfillable = unfillable;
    return ASW_OK;
}

extern "C" int asw_stereo_match_refined(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp, int algorithm,
                                        int win_size, int min_disparity, int num_disparity, float max_diff, int refine_win,
                                        double gamma_c, double gamma_s, int* n_rejected, int* n_unfillable)
{
    if (!ctx) return ASW_ERR_BAD_ARGUMENT;
    ASW_TRY(check_pair(left, right));
    ASW_TRY(check_disp_out(disp, left->rows, left->cols));
    ASW_HIP_TRY(hipSetDevice(ctx->device));
    Frame* f = &ctx->host_frame;
    ASW_TRY(upload_pair_into(ctx, f, left, right));
    int rejected = 0, unfillable = 0;
    ASW_TRY(match_refined(ctx, f, algorithm, win_size, min_disparity, num_disparity, max_diff, refine_win, gamma_c, gamma_s, &rejected,
                          &unfillable));
    ASW_TRY(download_disparity_from(ctx, f, disp));
    if (n_rejected) *n_rejected = rejected;
    if (n_unfillable) *n_unfillable = unfillable;
    return ASW_OK;
}

// ---- semi-global block matching (StereoSGBM::compute, MODE_SGBM_3WAY) and cv::filterSpeckles ----
static int check_s16_image(const asw_image* im)
{
    if (!im || !im->data || im->rows <= 0 || im->cols <= 0) return ASW_ERR_BAD_ARGUMENT;
    if (im->depth != ASW_16S || im->channels != 1) return ASW_ERR_UNSUPPORTED_LAYOUT;
    if (im->step < (size_t)im->cols * sizeof(short)) return ASW_ERR_BAD_ARGUMENT;
    return ASW_OK;
}

// The staged-pair + disp16 path of asw_sgbm, asw_stereo_bm and asw_get_disparity_bm, around each one's own checks and launches.
// disp16_stage: the caller's volume buffer checked against numD planes, the pair into the context's private frame, the volume scratch
// `vol_name` sized (*vol_dev; null when no volume is asked for), the clock started.
static int disp16_stage(asw_ctx* ctx, const asw_image* left, const asw_image* right, int numD, const char* vol_name,
                        const float* cost_volume_out, size_t cost_volume_floats, Frame** frame, float** vol_dev)
{
    const size_t vol_floats = (size_t)left->rows * left->cols * (size_t)numD;
    if (cost_volume_out && cost_volume_floats < vol_floats) return ASW_ERR_BAD_ARGUMENT;
    Frame* f = &ctx->host_frame;
    ASW_TRY(upload_pair_into(ctx, f, left, right));
    f->invalidate_results();
    *vol_dev = nullptr;
    if (cost_volume_out) {
        DevBuf& vol = ctx->buf(vol_name);
        ASW_TRY(vol.ensure(vol_floats * sizeof(float)));
        *vol_dev = vol.as<float>();
    }
    *frame = f;
    return ctx->clock.begin_total();
}

// disp16_finish: the clock stopped, the device map (elements of `elem` bytes) into the caller's pitched map, the volume into its buffer
static int disp16_finish(asw_ctx* ctx, asw_image* map, const void* map_dev, size_t elem, float* cost_volume_out,
                         const float* vol_dev, int numD)
{
    ASW_TRY(ctx->clock.finish(true));
    const size_t row = (size_t)map->cols * elem;
    ASW_HIP_TRY(copy_rows(ctx, map->data, map->step, map_dev, row, row, map->rows, hipMemcpyDeviceToHost));
    if (cost_volume_out)
        ASW_HIP_TRY(hipMemcpyAsync(cost_volume_out, vol_dev, (size_t)map->rows * map->cols * numD * sizeof(float), hipMemcpyDeviceToHost,
                                   ctx->stream));
    ASW_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ASW_OK;
}

// asw_sgbm: mode 2 with the three paths of MODE_SGBM_3WAY, or with the mask that asw_sgbm_paths packed into mode; census: the cost
// of asw_sgbm_census in place of the prefilter and the Birchfield-Tomasi cost
static int sgbm_host(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp16, int min_disparity,
                     int num_disparities, int block_size, int p1, int p2, int disp12_max_diff, int pre_filter_cap,
                     int uniqueness_ratio, int speckle_window_size, int speckle_range, int mode, int paths, bool census,
                     float* cost_volume_out, size_t cost_volume_floats)
{
    if (!ctx) return ASW_ERR_BAD_ARGUMENT;
    ASW_TRY(check_pair(left, right));
    ASW_TRY(check_s16_image(disp16));  // the same status as asw_filter_speckles for a map that is not CV_16SC1
    if (disp16->rows != left->rows || disp16->cols != left->cols || disp16->step < (size_t)left->cols * sizeof(short))
        return ASW_ERR_BAD_ARGUMENT;
    const int H = left->rows, W = left->cols;
    SgbmParams p;
    p.minD = min_disparity; p.numD = num_disparities; p.block_size = block_size; p.P1 = p1; p.P2 = p2;
    p.disp12_max_diff = disp12_max_diff; p.pre_filter_cap = pre_filter_cap; p.uniqueness_ratio = uniqueness_ratio;
    p.speckle_window_size = speckle_window_size; p.speckle_range = speckle_range; p.mode = mode; p.paths = paths; p.census = census;
    ASW_HIP_TRY(hipSetDevice(ctx->device));
    SgbmLaunch a;
    ASW_TRY(sgbm_prepare(ctx, p, H, W, left->channels, cost_volume_out != nullptr, &a));
    Frame* f;
    ASW_TRY(disp16_stage(ctx, left, right, num_disparities, "sgbm_volume", cost_volume_out, cost_volume_floats, &f, &a.vol));
    a.L = f->L.as<uint8_t>(); a.R = f->R.as<uint8_t>();
    if (census) ASW_TRY(gray_pair(ctx, a.L, a.R, left->channels, H, W, &a.L, &a.R));  // the cost reads one gray plane per image
    // k_sgbm_top, k_sgbm_row + one k_sgbm_line per line geometry in use (columns, diagonals, anti-diagonals)
    const int launches = 2 + !!(paths & ASW_SGBM_PATH_BT) + !!(paths & (ASW_SGBM_PATH_TLBR | ASW_SGBM_PATH_BRTL)) +
                         !!(paths & (ASW_SGBM_PATH_TRBL | ASW_SGBM_PATH_BLTR));
    a.agg = {&ctx->clock, launches};
    ASW_TRY(launch_sgbm(ctx->stream, a));
    return disp16_finish(ctx, disp16, a.disp16, sizeof(short), cost_volume_out, a.vol, num_disparities);
}

extern "C" int asw_sgbm(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp16, int min_disparity,
                        int num_disparities, int block_size, int p1, int p2, int disp12_max_diff, int pre_filter_cap,
                        int uniqueness_ratio, int speckle_window_size, int speckle_range, int mode, float* cost_volume_out,
                        size_t cost_volume_floats)
{
    int paths = ASW_SGBM_PATHS_3WAY;
    bool census = false;
    if (mode > 0 && (mode & ASW_SGBM_MODE_PATHS)) {  // asw_sgbm_paths (asw_mi355x.h): the three-path pipeline over a path mask
        census = (mode & ASW_SGBM_MODE_CENSUS) != 0;  // asw_sgbm_census: the same with the census cost
        paths = mode & ~(ASW_SGBM_MODE_PATHS | ASW_SGBM_MODE_CENSUS);
        mode = 2;
    }
    return sgbm_host(ctx, left, right, disp16, min_disparity, num_disparities, block_size, p1, p2, disp12_max_diff, pre_filter_cap,
                     uniqueness_ratio, speckle_window_size, speckle_range, mode, paths, census, cost_volume_out, cost_volume_floats);
}

extern "C" int asw_filter_speckles(asw_ctx* ctx, asw_image* img, int new_val, int max_speckle_size, int max_diff)
{
    if (!ctx) return ASW_ERR_BAD_ARGUMENT;
    ASW_TRY(check_s16_image(img));
    if (new_val < -32768 || new_val > 32767) return ASW_ERR_BAD_ARGUMENT;
    const int H = img->rows, W = img->cols;
    const size_t plane = (size_t)H * W;
    if (plane >= ((size_t)1 << 31)) return ASW_ERR_BAD_ARGUMENT;
    ASW_HIP_TRY(hipSetDevice(ctx->device));
    DevBuf& buf = ctx->buf("speckle_img");
    DevBuf& scratch = ctx->buf("speckle_scratch");
    ASW_TRY(buf.ensure(plane * sizeof(short)));
    ASW_TRY(scratch.ensure(plane * 2 * sizeof(int)));
    const size_t row = (size_t)W * sizeof(short);
    ASW_HIP_TRY(copy_rows(ctx, buf.p, row, img->data, img->step, row, H, hipMemcpyHostToDevice));
    ASW_TRY(ctx->clock.begin_total());
    ASW_TRY(ctx->clock.begin_aggregate());
    ASW_TRY(launch_filter_speckles(ctx->stream, buf.as<short>(), H, W, new_val, max_speckle_size, max_diff, scratch.as<int>()));
    ASW_TRY(ctx->clock.end_aggregate(4));  // k_spk_init, union, flatten, apply (+ the pointer-jumping rounds between them)
    ASW_TRY(ctx->clock.finish(true));
    ASW_HIP_TRY(copy_rows(ctx, img->data, img->step, buf.p, row, row, H, hipMemcpyDeviceToHost));
    ASW_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ASW_OK;
}

// ---- block matching (StereoBM::compute with PREFILTER_XSOBEL) and the reference's getDisparity_BM ----
extern "C" int asw_stereo_bm(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp16, int min_disparity,
                             int num_disparities, int block_size, int pre_filter_type, int pre_filter_size, int pre_filter_cap,
                             int texture_threshold, int uniqueness_ratio, int speckle_window_size, int speckle_range,
                             int disp12_max_diff, float* cost_volume_out, size_t cost_volume_floats)
{
    if (!ctx) return ASW_ERR_BAD_ARGUMENT;
    ASW_TRY(check_pair(left, right));
    if (left->channels != 1) return ASW_ERR_UNSUPPORTED_LAYOUT;  // StereoBM takes CV_8UC1 only
    ASW_TRY(check_s16_image(disp16));
    if (disp16->rows != left->rows || disp16->cols != left->cols) return ASW_ERR_BAD_ARGUMENT;
    const int H = left->rows, W = left->cols;
    BmParams p;
    p.minD = min_disparity; p.numD = num_disparities; p.block_size = block_size; p.pre_filter_type = pre_filter_type;
    p.pre_filter_size = pre_filter_size; p.pre_filter_cap = pre_filter_cap; p.texture_threshold = texture_threshold;
    p.uniqueness_ratio = uniqueness_ratio; p.speckle_window_size = speckle_window_size; p.speckle_range = speckle_range;
    p.disp12_max_diff = disp12_max_diff;
    ASW_HIP_TRY(hipSetDevice(ctx->device));
    BmLaunch a;
    ASW_TRY(bm_prepare(ctx, p, H, W, &a));
    Frame* f;
    ASW_TRY(disp16_stage(ctx, left, right, num_disparities, "bm_volume", cost_volume_out, cost_volume_floats, &f, &a.vol));
    a.L = f->L.as<uint8_t>(); a.R = f->R.as<uint8_t>();
    a.agg = {&ctx->clock, 1};
    ASW_TRY(launch_bm(ctx->stream, a));
    return disp16_finish(ctx, disp16, a.disp16, sizeof(short), cost_volume_out, a.vol, num_disparities);
}

// getDisparity_BM (aswMethods.cpp:100-146): the CV_Error cases (numDisparity % 16 != 0, an even winSize, an empty image, and
// compute's assertions on numDisparities and blockSize = winSize > 0 ? winSize : 9) give ASW_ERR_UNSUPPORTED_METHOD; a 3-channel
// image is converted with cvtColor(BGR2GRAY) on the device (asw_set_gray_bits); StereoBM with the wrapper's settings, then
// convertTo(CV_8U, 1/16).
extern "C" int asw_get_disparity_bm(asw_ctx* ctx, const asw_image* left, const asw_image* right, asw_image* disp_u8, int win,
                                    int min_disparity, int num_disparities)
{
    if (!ctx || !left || !right || !disp_u8) return ASW_ERR_BAD_ARGUMENT;
    if (num_disparities % 16 != 0 || win % 2 == 0) return ASW_ERR_UNSUPPORTED_METHOD;
    if (!left->data || !right->data || left->rows <= 0 || left->cols <= 0 || right->rows <= 0 || right->cols <= 0)
        return ASW_ERR_UNSUPPORTED_METHOD;
    ASW_TRY(check_pair(left, right));
    const int cn = left->channels;
    if (cn != 1 && cn != 3) return ASW_ERR_UNSUPPORTED_LAYOUT;
    const int H = left->rows, W = left->cols;
    const int w = win > 0 ? win : 9;
    if (num_disparities <= 0 || w < 5 || w > 255 || w > std::min(H, W)) return ASW_ERR_UNSUPPORTED_METHOD;
    if (!disp_u8->data || disp_u8->depth != ASW_8U || disp_u8->channels != 1) return ASW_ERR_UNSUPPORTED_LAYOUT;
    if (disp_u8->rows != H || disp_u8->cols != W || disp_u8->step < (size_t)W) return ASW_ERR_BAD_ARGUMENT;
    BmParams p;
    p.minD = min_disparity; p.numD = num_disparities; p.block_size = w; p.pre_filter_type = 1; p.pre_filter_size = 9;
    p.pre_filter_cap = 31; p.texture_threshold = 10; p.uniqueness_ratio = 15; p.speckle_window_size = 100; p.speckle_range = 32;
    p.disp12_max_diff = 1;
    ASW_HIP_TRY(hipSetDevice(ctx->device));
    BmLaunch a;
    ASW_TRY(bm_prepare(ctx, p, H, W, &a));
    const size_t plane = (size_t)H * W;
    DevBuf& u8 = ctx->buf("bm_u8");
    ASW_TRY(u8.ensure(plane));
    Frame* f;
    ASW_TRY(disp16_stage(ctx, left, right, num_disparities, nullptr, nullptr, 0, &f, &a.vol));
    ASW_TRY(gray_pair(ctx, f->L.as<uint8_t>(), f->R.as<uint8_t>(), cn, H, W, &a.L, &a.R));
    a.agg = {&ctx->clock, 1};
    ASW_TRY(launch_bm(ctx->stream, a));
    ASW_TRY(launch_disp16_to_u8(ctx->stream, a.disp16, plane, u8.as<uint8_t>()));
    return disp16_finish(ctx, disp_u8, u8.p, 1, nullptr, nullptr, 0);
}
