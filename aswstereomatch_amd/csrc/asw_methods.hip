// Method runners behind the selector stereoMatching (M.cpp:46-88): tables, scratch buffers and launch sequences of every
// method, with the literals the selector hard-codes and the reference's error behaviour.
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <utility>
#include <vector>

#include "asw_internal.h"
#include "asw_host.h"

// ------------------------------------------------------------------------------------------
// pieces every runner is made of
// ------------------------------------------------------------------------------------------
static int check_direction(int disparity_type)
{
    return disparity_type == ASW_DISPARITY_LEFT || disparity_type == ASW_DISPARITY_RIGHT ? ASW_OK : ASW_ERR_BAD_ARGUMENT;
}

// the frame's disparity map and, when the caller keeps it (or the method's own WTA pass reads it: volume_needed), its volume of
// `planes` planes; f->vol_floats = what the caller keeps
static int ensure_outputs(Frame* f, int planes, bool keep_volume, bool volume_needed = false)
{
    const size_t plane = (size_t)f->rows * f->cols;
    ASW_TRY(f->disp.ensure(plane * 4));
    f->vol_floats = 0;
    if (keep_volume || volume_needed) ASW_TRY(f->vol.ensure(plane * planes * 4));
    if (keep_volume) f->vol_floats = plane * planes;
    return ASW_OK;
}

int gray_pair(asw_ctx* ctx, const uint8_t* dL, const uint8_t* dR, int channels, int H, int W, const uint8_t** gl, const uint8_t** gr)
{
    *gl = dL; *gr = dR;
    if (channels != 3) return ASW_OK;
    DevBuf& l = ctx->buf("grayL");
    DevBuf& r = ctx->buf("grayR");
    ASW_TRY(l.ensure((size_t)H * W));
    ASW_TRY(r.ensure((size_t)H * W));
    ASW_TRY(launch_bgr2gray(ctx->stream, dL, H, W, l.as<uint8_t>(), ctx->gray_bits));
    ASW_TRY(launch_bgr2gray(ctx->stream, dR, H, W, r.as<uint8_t>(), ctx->gray_bits));
    *gl = l.as<uint8_t>(); *gr = r.as<uint8_t>();
    return ASW_OK;
}

// per-slice winners of a candidate range split over slices: [slices][plane] costs and disparities
static int slice_scratch(asw_ctx* ctx, int slices, size_t plane, double** E, float** D)
{
    DevBuf& pe = ctx->buf("bil_partE");
    DevBuf& pd = ctx->buf("bil_partD");
    ASW_TRY(pe.ensure((size_t)slices * plane * sizeof(double)));
    ASW_TRY(pd.ensure((size_t)slices * plane * sizeof(float)));
    *E = pe.as<double>(); *D = pd.as<float>();
    return ASW_OK;
}

// the clock's marks around a method's aggregation kernels (asw_timing::aggregate_ms) and the launch count that goes with them
static int agg_begin(asw_ctx* ctx) { return ctx->clock.begin_aggregate(); }
static int agg_end(asw_ctx* ctx, int launches) { return ctx->clock.end_aggregate(launches); }

// ------------------------------------------------------------------------------------------
// classic bilateral ASW: host-side tables (tap list with the reference's two index conventions,
// weight LUT with the reference's expression) -- M.cpp:1044-1066, 1088-1102, SURVEY App. B-2
// ------------------------------------------------------------------------------------------
// mirror = 1: table for the x-mirrored problem (DISPARITY_RIGHT runs as DISPARITY_LEFT on mirrored, swapped images:
// M.cpp:1134-1138 is M.cpp:1104-1108 under x -> W-1-x), i.e. every x direction negated, tap ORDER unchanged.
// Tap table + weight LUT of the bilateral kernel.  kind 0: computeAdaptiveWeight (M.cpp:1041-1102);
// kind 1: computeAdaptiveWeight_direct8 (M.cpp:1195-1221, 1238-1259).
static int ensure_bilateral_tables(asw_ctx* ctx, int kind, int win, double gamma_c, double gamma_g, int mirror)
{
    BilateralTables& t = ctx->bil;
    const auto key = std::make_tuple(kind, win, gamma_c, gamma_g, mirror);
    if (t.cache.hit(key, ctx->stream)) return ASW_OK;
    const int ks = win, h = ks / 2;
    std::vector<int> dxw, dyw, dxs, dys;  // weight direction (build order) / sample offset (consume order)
    if (kind == 0) {
        const int nt = ks * ks - 1;
        dxs.resize(nt); dys.resize(nt);
        for (int j = -h; j < h + 1; j++)          // build order of the weight maps, M.cpp:1044-1053
            for (int i = -h; i < h + 1; i++) {
                if (i == 0 && j == 0) continue;
                dxw.push_back(i); dyw.push_back(j);
            }
        for (int i = 0; i < nt; i++) {            // consume order of the samples, M.cpp:1088-1102
            int kx, ky;
            if (i > ks * ks / 2) { kx = (i + 1) / ks; ky = (i + 1) % ks; }
            else { kx = i / ks; ky = i % ks; }
            dxs[i] = -h + kx; dys[i] = -h + ky;
        }
    } else {
        for (int j = -h; j < h + 1; j++)          // M.cpp:1195-1201 == 1238-1245: same order, same test
            for (int i = -h; i < h + 1; i++) {
                if (i == 0 && j == 0) continue;
                if (i == j || i == 0 || j == 0 || (i + j) == ks - 1) { dxw.push_back(i); dyw.push_back(j); }
            }
        dxs = dxw; dys = dyw;                     // the sample is the neighbour the weight was built for
    }
    const int nt = (int)dxw.size();
    // distance classes: distinct values of i*i + j*j
    std::vector<int> cls_of_r2(2 * h * h + 1, -1);
    std::vector<int> r2s;
    for (int i = 0; i < nt; i++) {
        int r2 = dxw[i] * dxw[i] + dyw[i] * dyw[i];
        if (cls_of_r2[r2] < 0) { cls_of_r2[r2] = (int)r2s.size(); r2s.push_back(r2); }
    }
    // The kernel consumes taps in groups of 4: pad with taps of an all-zero weight class (0*w*c adds +0.0 to both sums).
    const int nt_pad = (nt + 3) / 4 * 4, zero_cls = (int)r2s.size();
    std::vector<float> lut((r2s.size() + 1) * 256, 0.0f);
    const double k = 3;  // M.cpp:1024, 1175
    for (size_t c = 0; c < r2s.size(); c++) {
        double delta_g = sqrt((double)r2s[c]);  // M.cpp:1054, 1205
        for (int dc = 0; dc < 256; dc++) {
            double delta_c = (double)dc;
            lut[c * 256 + dc] = (float)(k * exp(-(delta_c / gamma_c + delta_g / gamma_g)));  // M.cpp:1065, 1214
        }
    }
    std::vector<int4> taps(nt_pad);
    const int LW = bilateral_lds_row_stride(win);  // row stride of the kernel's LDS sample tile
    for (int i = 0; i < nt; i++) {
        const int sx = mirror ? -1 : 1;
        taps[i].x = dys[i] * LW + sx * dxs[i];  // sample cell, consume order (classic: transposed, App. B-2)
        taps[i].y = sx * dxw[i];                // weight direction, build order
        taps[i].z = dyw[i];
        taps[i].w = cls_of_r2[dxw[i] * dxw[i] + dyw[i] * dyw[i]] * 256;
    }
    for (int i = nt; i < nt_pad; i++) taps[i] = make_int4(0, 0, 0, zero_cls * 256);
    // Cell-indexed form of the same table for k_asw_bilateral_xq: window cell (kx, ky) -> the weight map that is applied to the
    // sample at that cell, {dx, dy of the direction the map was BUILT for, class * 256}.  Columns kx = -3..17 (units run up to
    // three columns behind the step counter); the all-zero class stands for "no tap": outside the window and the one cell the
    // reference's index arithmetic skips (kernel_x 7, kernel_y 8: M.cpp:1090-1099 jumps from i = 112 to the cell of i + 1).
    std::vector<int4> cells;
    if (kind == 0 && win == 15) {  // image coordinates, for either direction (the xq kernel does not mirror)
        cells.assign(21 * 15, make_int4(0, 0, zero_cls * 256, 0));
        for (int i = 0; i < nt; i++) {
            const int kx = dxs[i] + h, ky = dys[i] + h;
            cells[(kx + 3) * 15 + ky] = make_int4(dxw[i], dyw[i], cls_of_r2[dxw[i] * dxw[i] + dyw[i] * dyw[i]] * 256, 1);
        }
    }
    if (taps.empty())  // win = 1 has no taps at all (every E is 0/0): never a null table all the same
        ASW_TRY(t.taps.ensure(4 * sizeof(int4)));
    else
        ASW_TRY(t.cache.upload(t.taps, taps.data(), taps.size() * sizeof(int4)));
    ASW_TRY(t.cache.upload(t.lut, lut.data(), lut.size() * sizeof(float)));
    std::vector<float> lut_xq;
    t.xq_lut_ok = false;
    if (!cells.empty()) {
        ASW_TRY(t.cache.upload(t.cells, cells.data(), cells.size() * sizeof(int4)));
        t.xq_lut_ok = bilateral_xq_lut_ok(lut.data(), lut.size());
        if (t.xq_lut_ok) {  // a power-of-two scale: exact for every entry (none overflows, none is lost)
            lut_xq.resize(lut.size());
            for (size_t i = 0; i < lut.size(); i++) lut_xq[i] = ldexpf(lut[i], XQ_LUT_SCALE_LOG2);
            ASW_TRY(t.cache.upload(t.lut_xq, lut_xq.data(), lut_xq.size() * sizeof(float)));
        }
    }
    t.ntaps = nt_pad;
    t.ncls = (int)r2s.size() + 1;
    return t.cache.commit(key);
}


// computeAdaptiveWeight (direct8 = false) and computeAdaptiveWeight_direct8 (direct8 = true: sparse support, its own
// gamma_g, DISPARITY_LEFT only -- the RIGHT branch of the reference indexes its weight vectors with a negative tap
// coordinate, M.cpp:1291-1295)
static int run_bilateral(asw_ctx* ctx, Frame* f, const MatchParams& mp, bool keep_volume, bool direct8)
{
    if (mp.win % 2 == 0) return ASW_ERR_EVEN_WINDOW;  // build decision: the reference has no guard
    if (mp.win < 1) return ASW_ERR_BAD_ARGUMENT;
    if (f->channels != 3) return ASW_ERR_UNSUPPORTED_LAYOUT;  // cvtColor(BGR2GRAY) asserts scn==3/4
    ASW_TRY(check_direction(mp.disparity_type));
    if (direct8 && mp.disparity_type != ASW_DISPARITY_LEFT) return ASW_ERR_UNSUPPORTED_LAYOUT;
    const int flip = mp.disparity_type == ASW_DISPARITY_RIGHT ? 1 : 0;
    if (mp.win > bilateral_max_window()) return ASW_ERR_BAD_ARGUMENT;  // before any table, buffer or launch
    const int H = f->rows, W = f->cols;
    const int nD = method_info(direct8 ? ASW_ALG_ADAPTIVE_WEIGHT_8DIRECT : ASW_ALG_ADAPTIVE_WEIGHT)->planes(mp.numD);
    if (direct8)
        ASW_TRY(ensure_bilateral_tables(ctx, 1, mp.win, 30.0, (double)(mp.win * 2 / 3), 0));  // M.cpp:1175: integer division
    else
        ASW_TRY(ensure_bilateral_tables(ctx, 0, mp.win, mp.gamma_c, mp.gamma_g, flip));
    const uint8_t *gl, *gr;
    ASW_TRY(ensure_outputs(f, nD, keep_volume));
    ASW_TRY(gray_pair(ctx, f->L.as<uint8_t>(), f->R.as<uint8_t>(), 3, H, W, &gl, &gr));
    BilateralLaunch a;
    a.gL = flip ? gr : gl;  // RIGHT: reference image = right, read mirrored in the kernel
    a.gR = flip ? gl : gr;
    a.flip = flip;
    a.H = H; a.W = W; a.win = mp.win; a.minD = mp.minD; a.nD = nD;
    a.taps = ctx->bil.taps.as<int4>(); a.lut = ctx->bil.lut.as<float>(); a.ntaps = ctx->bil.ntaps;
    a.vol = keep_volume ? f->vol.as<float>() : nullptr;
    a.disp = f->disp.as<float>();
    a.partE = nullptr; a.partD = nullptr; a.max_slices = 0;
    // Candidate ranges of the reference's own configuration (15x15, either direction) from 64 candidates up take the xq form of the
    // kernel for the first 128 (8 wavefronts per workgroup) or 64 (4 wavefronts: the reference's own call site passes
    // numDisparity 64 -> 65 candidates, aswStereoMatch.cpp:94) and this kernel for the tail.  The tile of the outermost workgroup must still hold the eight image
    // columns next to the border its positions clamp to: LEFT minD <= 48 (columns 0..7 in the first tile), RIGHT
    // x0_last + minD <= W - 1 (columns W-8..W-1 in the last).  The xq form sums in a scaled domain that is exact only for LUTs
    // whose nonzero weight products are >= 2^-68 (bilateral_xq_lut_ok: every gamma_c above about 10); other gammas take the
    // one-kernel form.  ASW_BILATERAL_XQ=0 forces the one-kernel path (A/B, tests).
    const bool xq_fits = flip ? (W - 1) / 64 * 64 + mp.minD <= W - 1 : mp.minD <= 48;
    const int xq_waves = nD >= bilateral_xq_candidates(8) ? 8 : 4;
    const bool use_xq = !direct8 && mp.win == 15 && nD >= bilateral_xq_candidates(xq_waves) && mp.minD >= 0 && xq_fits && W >= 64 &&
                        ctx->bil.xq_lut_ok && ctx->tune.bilateral_xq != 0;
    const size_t plane = (size_t)H * W;
    if (use_xq) {
        a.max_slices = 2;
        ASW_TRY(slice_scratch(ctx, a.max_slices, plane, &a.partE, &a.partD));
        a.c_begin = bilateral_xq_candidates(xq_waves);
        const bool tail = nD > a.c_begin;  // numDisparity = 127 / 63 ends exactly at the xq kernel's 128 / 64 candidates
        // One candidate more than the xq kernel's block -- the reference's inclusive range at numDisparity 128 / 64: the interior
        // tiles finish it themselves (LASTC) and write the disparity; the one-kernel launch for that candidate, its
        // slice and the merge shrink to the columns of the border tiles.  The launch count stays 4.
        int ic_lo = 0, ic_hi = 0;
        bilateral_xq_interior_columns(W, flip != 0, &ic_lo, &ic_hi);
        const bool last = nD == a.c_begin + 1 && ic_lo < ic_hi;
        const int bc_lo = flip ? 0 : ic_hi, bc_hi = flip ? ic_lo : W;  // the border tiles' columns (never empty)
        ASW_TRY(agg_begin(ctx));
        // fork: border tiles and the tail are independent of the interior launch (they write other pixels / another slice of the
        // per-slice winners); on side streams they overlap it instead of adding two latency-bound 0.5 ms launches to the frame
        SideStreams side(ctx->stream, ctx->side);
        hipStream_t s_border = nullptr, s_tail = nullptr;
        ASW_TRY(side.use(0, &s_border));
        ASW_TRY(launch_bilateral_xq(ctx->stream, s_border, xq_waves, a.gL, a.gR, H, W, mp.minD, ctx->bil.cells.as<int4>(), ctx->bil.lut_xq.as<float>(), a.vol,
                                    a.partE, a.partD, tail && !last ? nullptr : a.disp, flip != 0, last));
        if (tail) {
            ASW_TRY(side.use(1, &s_tail));
            a.out_slice = 1;  // candidates [128 | 64, nD) -> slice 1; the xq launches fill slice 0
            if (last) { a.col_lo = bc_lo; a.col_hi = bc_hi; }
            ASW_TRY(launch_bilateral(s_tail, a));
        }
        ASW_TRY(side.join());
        // strict '<', ascending d
        if (tail && last) ASW_TRY(launch_merge_slices_cols(ctx->stream, a.partE, a.partD, 2, H, W, bc_lo, bc_hi, a.disp));
        else if (tail) ASW_TRY(launch_merge_slices(ctx->stream, a.partE, a.partD, 2, plane, a.disp));
        return agg_end(ctx, tail ? 4 : 2);
    }
    if (plane <= (size_t)1 << 20) {  // small frames only: scratch for the grid.z split of the disparity range
        a.max_slices = 8;
        ASW_TRY(slice_scratch(ctx, a.max_slices, plane, &a.partE, &a.partD));
    }
    ASW_TRY(agg_begin(ctx));
    ASW_TRY(launch_bilateral(ctx->stream, a));
    return agg_end(ctx, 1);
}

// ------------------------------------------------------------------------------------------
// two-pass (separable) ASW (Wang et al. 2006): entry 2 with an asw_alg_twopass() value; not in the reference
// ------------------------------------------------------------------------------------------
static int ensure_twopass_table(asw_ctx* ctx, int win, int gamma_c, int gamma_g)
{
    TwoPassTable& t = ctx->twopass;
    const auto key = std::make_tuple(win, gamma_c, gamma_g);
    if (t.cache.hit(key, ctx->stream)) return ASW_OK;
    const int h = win / 2;
    std::vector<float> tab((size_t)(h + 1) * 256);
    for (int r = 0; r <= h; r++)
        for (int dc = 0; dc < 256; dc++) tab[(size_t)r * 256 + dc] = (float)exp(-((double)dc / gamma_c + (double)r / gamma_g));
    ASW_TRY(t.cache.upload(t.t, tab.data(), tab.size() * sizeof(float)));
    return t.cache.commit(key);
}

static int run_twopass(asw_ctx* ctx, Frame* f, const MatchParams& mp, bool keep_volume)
{
    if (mp.win % 2 == 0) return ASW_ERR_EVEN_WINDOW;
    if (mp.win < 1 || mp.win > twopass_max_window()) return ASW_ERR_BAD_ARGUMENT;  // before any table, buffer or launch
    if (f->channels != 3 && f->channels != 1) return ASW_ERR_UNSUPPORTED_LAYOUT;
    ASW_TRY(check_direction(mp.disparity_type));
    const int gamma_c = (int)mp.gamma_c, gamma_g = (int)mp.gamma_g;  // decode_algorithm: integers in 1..255
    if (gamma_c < 1 || gamma_c > 255 || gamma_g < 1 || gamma_g > 255) return ASW_ERR_BAD_ARGUMENT;
    const int flip = mp.disparity_type == ASW_DISPARITY_RIGHT ? 1 : 0;
    const int H = f->rows, W = f->cols, nD = method_info(ASW_ALG_ADAPTIVE_WEIGHT)->planes(mp.numD);
    ASW_TRY(ensure_twopass_table(ctx, mp.win, gamma_c, gamma_g));
    ASW_TRY(ensure_outputs(f, nD, keep_volume));
    const uint8_t *gl, *gr;
    ASW_TRY(gray_pair(ctx, f->L.as<uint8_t>(), f->R.as<uint8_t>(), f->channels, H, W, &gl, &gr));
    TwoPassLaunch a;
    a.gL = flip ? gr : gl;  // RIGHT: reference image = right, read mirrored in the kernel
    a.gR = flip ? gl : gr;
    a.flip = flip;
    a.H = H; a.W = W; a.win = mp.win; a.minD = mp.minD; a.nD = nD;
    a.table = ctx->twopass.t.as<float>();
    a.vol = keep_volume ? f->vol.as<float>() : nullptr;
    a.disp = f->disp.as<float>();
    ASW_TRY(agg_begin(ctx));
    ASW_TRY(launch_twopass(ctx->stream, a));
    return agg_end(ctx, 1);
}

static int run_bilateral_classic(asw_ctx* ctx, Frame* f, const MatchParams& mp, bool keep_volume)
{
    if (mp.twopass) return run_twopass(ctx, f, mp, keep_volume);
    return run_bilateral(ctx, f, mp, keep_volume, false);
}

static int run_direct8(asw_ctx* ctx, Frame* f, const MatchParams& mp, bool keep_volume)
{
    return run_bilateral(ctx, f, mp, keep_volume, true);
}


// ------------------------------------------------------------------------------------------
// guided-filter ASW: computeAdaptiveWeight_GuidedF_2 (M.cpp:2976-3050, TAD C+G cost, guide = left image)
// and computeAdaptiveWeight_GuidedF (M.cpp:2867-2963, SAD cost, 6-channel guide [L, R shifted by d])
// ------------------------------------------------------------------------------------------
int build_similarity_volume(asw_ctx* ctx, const uint8_t* dL, const uint8_t* dR, int H, int W, int minD, int numD,
                                   double regularity, double thresC, double thresG, float* cost,
                                   uint32_t* ord_scratch, float2* scales)
{
    const int max_off = minD + numD - 1;
    DevBuf& gl = ctx->buf("scharrL");
    DevBuf& gr = ctx->buf("scharrR");
    ASW_TRY(gl.ensure((size_t)H * W * 3 * sizeof(short)));
    ASW_TRY(gr.ensure((size_t)H * (W + max_off) * 3 * sizeof(short)));
    ASW_TRY(launch_scharr_x(ctx->stream, dL, H, W, 0, gl.as<short>()));
    ASW_TRY(launch_scharr_x(ctx->stream, dR, H, W, max_off, gr.as<short>()));  // gradient of the PADDED right image
    return launch_similarity(ctx->stream, dL, dR, gl.as<short>(), gr.as<short>(), H, W, minD, numD, regularity, thresC, thresG,
                             cost, ord_scratch, scales);
}

// ------------------------------------------------------------------------------------------
// NCC cost (computeNCC / getInputImgNCC, M.cpp:767-1013): gray images, box means, window sums of squares, then k_ncc
// ------------------------------------------------------------------------------------------
int run_ncc_cost(asw_ctx* ctx, const uint8_t* dL, const uint8_t* dR, int H, int W, int disparity_type, int win, int minD,
                        int numD, float* vol /* optional, un-normalised */, float* disp /* optional */, int nwta,
                        int channels)
{
    if (win % 2 == 0) return ASW_ERR_EVEN_WINDOW;  // M.cpp:828-831, 939-942
    // the box means go through the walk, the cost through k_ncc: both launchers' limits, before the first buffer or launch
    if (win < 1 || win > std::min(ncc_max_window(), walk_max_kernel())) return ASW_ERR_BAD_ARGUMENT;
    const bool right = disparity_type == ASW_DISPARITY_RIGHT;
    const int max_off = minD + numD - 1, Wp = W + max_off;
    const size_t plane = (size_t)H * W, pplane = (size_t)H * Wp;
    DevBuf& g0 = ctx->buf("ncc_gray_ref");
    DevBuf& g1 = ctx->buf("ncc_gray_oth");
    DevBuf& gp = ctx->buf("ncc_gray_pad");
    DevBuf& m0 = ctx->buf("ncc_mean_ref");
    DevBuf& m1 = ctx->buf("ncc_mean_oth");
    DevBuf& s0 = ctx->buf("ncc_ss_ref");
    DevBuf& s1 = ctx->buf("ncc_ss_oth");
    ASW_TRY(g0.ensure(plane)); ASW_TRY(g1.ensure(plane)); ASW_TRY(gp.ensure(pplane));
    ASW_TRY(m0.ensure(plane * 4)); ASW_TRY(m1.ensure(pplane * 4));
    ASW_TRY(s0.ensure(plane * 8)); ASW_TRY(s1.ensure(pplane * 8));
    // COLOR_RGB2GRAY on BGR data (M.cpp:835,840); reference image = left (LEFT) or right (RIGHT)
    if (channels == 3) {
        ASW_TRY(launch_rgb2gray(ctx->stream, right ? dR : dL, H, W, g0.as<uint8_t>(), ctx->gray_bits));
        ASW_TRY(launch_rgb2gray(ctx->stream, right ? dL : dR, H, W, g1.as<uint8_t>(), ctx->gray_bits));
    } else {  // single-channel input is used as it is (M.cpp:833-841: cvtColor only for 3 channels)
        ASW_HIP_TRY(hipMemcpyAsync(g0.p, right ? dR : dL, plane, hipMemcpyDeviceToDevice, ctx->stream));
        ASW_HIP_TRY(hipMemcpyAsync(g1.p, right ? dL : dR, plane, hipMemcpyDeviceToDevice, ctx->stream));
    }
    // the other image is padded by max_offset REFLECT columns: on the left (LEFT, M.cpp:852) / on the right (RIGHT, M.cpp:882)
    ASW_TRY(launch_pad_gray(ctx->stream, g1.as<uint8_t>(), H, W, right ? 0 : max_off, right ? max_off : 0, gp.as<uint8_t>()));
    ASW_TRY(launch_box_mean_u8(ctx->stream, g0.as<uint8_t>(), H, W, win, m0.as<float>()));   // M.cpp:785-786
    ASW_TRY(launch_box_mean_u8(ctx->stream, gp.as<uint8_t>(), H, Wp, win, m1.as<float>()));
    ASW_TRY(launch_ncc_selfsum(ctx->stream, g0.as<uint8_t>(), m0.as<float>(), H, W, win, s0.as<double>()));
    ASW_TRY(launch_ncc_selfsum(ctx->stream, gp.as<uint8_t>(), m1.as<float>(), H, Wp, win, s1.as<double>()));
    NccLaunch a;
    a.gref = g0.as<uint8_t>(); a.mref = m0.as<float>(); a.sref = s0.as<double>();
    a.goth = gp.as<uint8_t>(); a.moth = m1.as<float>(); a.soth = s1.as<double>();
    a.H = H; a.W = W; a.Wp = Wp; a.win = win; a.minD = minD; a.numD = numD; a.right = right ? 1 : 0; a.nwta = nwta;
    a.vol = vol; a.disp = disp;
    return launch_ncc(ctx->stream, a);
}

// computeNCC -> disparity (M.cpp:812-913): candidates minD .. max_offset-1 only, the SMALLEST cost wins (LEFT);
// DISPARITY_RIGHT compares `cost > DBL_MAX`: nothing is ever written -> zeros here (reference: uninitialised Mat).
static int run_ncc(asw_ctx* ctx, Frame* f, const MatchParams& mp, bool keep_volume)
{
    if (f->channels != 3) return ASW_ERR_UNSUPPORTED_LAYOUT;
    ASW_TRY(check_direction(mp.disparity_type));
    if (mp.win % 2 == 0) return ASW_ERR_EVEN_WINDOW;
    if (mp.win < 1 || mp.win > std::min(ncc_max_window(), walk_max_kernel())) return ASW_ERR_BAD_ARGUMENT;  // run_ncc_cost's limit, before agg_begin
    const int H = f->rows, W = f->cols;
    const bool right = mp.disparity_type == ASW_DISPARITY_RIGHT;
    if (right && keep_volume) return ASW_ERR_UNSUPPORTED_LAYOUT;  // the RIGHT view has no selector volume: before any work
    // LEFT, kept: the raw (un-normalised) costs of all numD offsets, for inspection
    ASW_TRY(ensure_outputs(f, mp.numD, keep_volume));
    ASW_TRY(agg_begin(ctx));
    if (right)
        ASW_HIP_TRY(hipMemsetAsync(f->disp.p, 0, (size_t)H * W * 4, ctx->stream));
    else
        ASW_TRY(run_ncc_cost(ctx, f->L.as<uint8_t>(), f->R.as<uint8_t>(), H, W, mp.disparity_type, mp.win, mp.minD, mp.numD,
                             keep_volume ? f->vol.as<float>() : nullptr, f->disp.as<float>(), mp.numD - 1));
    return agg_end(ctx, 1);
}

enum GuidedKind { GUIDED_SAD6 = 0 /* GuidedF */, GUIDED_SIM3 = 1 /* GuidedF_2 */, GUIDED_NCC = 2 /* GuidedF_3 */ };

static int run_guided(asw_ctx* ctx, Frame* f, const MatchParams& mp, bool keep_volume, int kind)
{
    const bool variant2 = kind == GUIDED_SIM3;
    // GuidedF_3 + DISPARITY_RIGHT: getGuidedFilter receives the plain right image (M.cpp:3110), a 3-channel guide
    const bool ncc = kind == GUIDED_NCC, plain3 = variant2 || (ncc && mp.disparity_type == ASW_DISPARITY_RIGHT);

    if (f->channels != 3) return ASW_ERR_UNSUPPORTED_LAYOUT;
    // GuidedF_2: RIGHT / gray branches of computeSimilarity throw in the reference (App. B-7).
    if (variant2 && mp.disparity_type != ASW_DISPARITY_LEFT) return ASW_ERR_UNSUPPORTED_LAYOUT;
    ASW_TRY(check_direction(mp.disparity_type));
    const bool right = mp.disparity_type == ASW_DISPARITY_RIGHT;
    if (!variant2 && mp.win % 2 == 0) return ASW_ERR_EVEN_WINDOW;  // getCostSAD_d, M.cpp:2458-2462; computeNCC, M.cpp:939-942
    // the window is the box side of every walk (SAD cost, statistics, a/b, q); GuidedF_3 builds its cost with k_ncc as well
    const int max_win = ncc ? std::min(walk_max_kernel(), ncc_max_window()) : walk_max_kernel();
    if (mp.win < 1 || mp.win > max_win) return ASW_ERR_BAD_ARGUMENT;
    const int H = f->rows, W = f->cols, n = mp.numD, C = plain3 ? 3 : 6;
    const size_t plane = (size_t)H * W;
    DevBuf& raw = ctx->buf("g_raw");
    DevBuf& ord = ctx->buf("g_ord");
    DevBuf& psc = ctx->buf("g_pscales");
    DevBuf& gsc = ctx->buf("g_gscales");
    DevBuf& stats = ctx->buf("g_stats");
    DevBuf& ab = ctx->buf("g_ab");
    DevBuf& pxa = ctx->buf("bgrxL");
    DevBuf& pxb = ctx->buf("bgrxR");
    const int nstat = plain3 ? 1 : n;
    ASW_TRY(raw.ensure(plane * n * 4));
    DevBuf& parts = ctx->buf("g_parts");
    ASW_TRY(parts.ensure(similarity_parts_words(H, W, n) * 4));
    ASW_TRY(ord.ensure((size_t)(2 * n + 2) * 4));
    ASW_TRY(psc.ensure((size_t)n * sizeof(float2)));
    ASW_TRY(gsc.ensure((size_t)n * sizeof(float2)));
    ASW_TRY(stats.ensure(guided_stats_floats(C, nstat, H, W) * 4));
    // (GuidedF_2 on large frames runs the fused walk: no a/b volume -- 4.4 GB at 1080p D=128)
    // the one place that decides fused or two-pass; launch_guided follows GuidedLaunch::fused
    const bool fused = guided_uses_fused(ctx->tune, C, plain3 ? 0 : 1, 0, ncc ? 1 : 0, H, W, n, mp.win);
    const size_t ab_floats = fused ? 16 : guided_ab_floats(C, n, H, W, mp.win);
    ASW_TRY(ab.ensure(ab_floats * 4));
    ASW_TRY(pxa.ensure((plane + 4) * 4));  // + slack: the q pass reads the guide words of a lane's two columns as one pair, the last one may start at column W-1
    ASW_TRY(pxb.ensure((plane + 4) * 4));
    ASW_TRY(ensure_outputs(f, n, keep_volume, true));  // q volume: always needed for the WTA pass
    const uint8_t* dL = f->L.as<uint8_t>();
    const uint8_t* dR = f->R.as<uint8_t>();

    GuidedLaunch a;
    // guide = [L, R shifted by -d] (LEFT, M.cpp:2907-2912) or [L shifted by +d, R] (RIGHT, M.cpp:2925-2929)
    a.shiftA = (!plain3 && right) ? 1 : 0; a.shiftB = (!plain3 && !right) ? -1 : 0; a.C = C; a.guide_per_slice = plain3 ? 0 : 1;
    a.nan_safe = ncc ? 1 : 0;  // SAD and TAD C+G costs are finite; an NCC cost is 0/0 where a window is flat
    const uint8_t* dGuide3 = variant2 ? dL : dR;  // the 3-channel guide: left image (GuidedF_2) / right image (GuidedF_3 RIGHT)
    ASW_TRY(launch_pack_words(ctx->stream, plain3 ? dGuide3 : dL, H, W, 3, 0, pxa.as<uint32_t>()));
    if (!plain3) ASW_TRY(launch_pack_words(ctx->stream, dR, H, W, 3, 0, pxb.as<uint32_t>()));
    a.guideA = pxa.as<uint32_t>(); a.guideB = plain3 ? nullptr : pxb.as<uint32_t>();
    if (ncc) {
        // costs_ds of computeNCC (M.cpp:3076): raw planes, then normalize(NORM_MINMAX) of every plane in place
        ASW_TRY(run_ncc_cost(ctx, dL, dR, H, W, mp.disparity_type, mp.win, mp.minD, n, raw.as<float>(), nullptr, 0));
        ASW_TRY(launch_slice_scales(ctx->stream, raw.as<float>(), n, plane, ord.as<uint32_t>(), psc.as<float2>()));
        ASW_TRY(launch_apply_scales(ctx->stream, raw.as<float>(), n, plane, psc.as<float2>()));
        if (plain3) {
            ASW_TRY(launch_u8_scale(ctx->stream, dGuide3, plane * 3, ord.as<uint32_t>() + 2 * n, gsc.as<float2>()));
        } else {
            DevBuf& colmm = ctx->buf("g_colmm");
            ASW_TRY(colmm.ensure((size_t)2 * W * sizeof(int)));
            ASW_TRY(launch_guide_scales_lr(ctx->stream, dL, dR, H, W, mp.minD, n, mp.disparity_type, ord.as<uint32_t>() + 2 * n,
                                           colmm.as<int>(), gsc.as<float2>()));
        }
    } else if (variant2) {
        ASW_TRY(build_similarity_volume(ctx, dL, dR, H, W, mp.minD, n, 0.4, 10, 50, raw.as<float>(), parts.as<uint32_t>(),
                                        psc.as<float2>()));  // M.cpp:2990 (+ the min/max of M.cpp:2775, fused)
        ASW_TRY(launch_u8_scale(ctx->stream, dL, plane * 3, ord.as<uint32_t>() + 2 * n, gsc.as<float2>()));
    } else {
        const uint8_t *gl, *gr;
        DevBuf& colmm = ctx->buf("g_colmm");
        ASW_TRY(colmm.ensure((size_t)2 * W * sizeof(int)));
        ASW_TRY(gray_pair(ctx, dL, dR, 3, H, W, &gl, &gr));
        ASW_TRY(launch_cost_sad(ctx->stream, gl, gr, H, W, mp.disparity_type, mp.win, mp.minD, n, raw.as<float>()));  // M.cpp:2884-2889
        ASW_TRY(launch_guide_scales_lr(ctx->stream, right ? dR : dL, right ? dL : dR, H, W, mp.minD, n, mp.disparity_type,
                                       ord.as<uint32_t>() + 2 * n, colmm.as<int>(), gsc.as<float2>()));
    }
    if (!variant2)
        ASW_TRY(launch_slice_scales(ctx->stream, raw.as<float>(), n, plane, ord.as<uint32_t>(), psc.as<float2>()));  // M.cpp:2775
    a.gscales = gsc.as<float2>(); a.P = raw.as<float>(); a.pscales = psc.as<float2>();
    a.H = H; a.W = W; a.n = n; a.r = mp.win; a.minD = mp.minD; a.eps = mp.eps;
    DevBuf& repb = ctx->buf("g_rep");
    ASW_TRY(repb.ensure((size_t)n * sizeof(int)));
    a.stats = stats.as<float>(); a.rep_scratch = repb.as<int>(); a.ab = ab.as<float>(); a.q = f->vol.as<float>();
    a.ab_floats = ab_floats; a.fused = fused ? 1 : 0;
    a.tune = &ctx->tune;
    ASW_TRY(agg_begin(ctx));
    ASW_TRY(launch_guided(ctx->stream, a));
    ASW_TRY(launch_wta(ctx->stream, f->vol.as<float>(), n, H, W, mp.minD, f->disp.as<float>()));  // M.cpp:3032-3048
    return agg_end(ctx, plain3 ? (fused ? 3 : 4) : 5);  // statistics, [a/b, q | fused walk], WTA
}

static int run_guided_sad6(asw_ctx* ctx, Frame* f, const MatchParams& mp, bool keep_volume) { return run_guided(ctx, f, mp, keep_volume, GUIDED_SAD6); }
static int run_guided_sim3(asw_ctx* ctx, Frame* f, const MatchParams& mp, bool keep_volume) { return run_guided(ctx, f, mp, keep_volume, GUIDED_SIM3); }
static int run_guided_ncc(asw_ctx* ctx, Frame* f, const MatchParams& mp, bool keep_volume) { return run_guided(ctx, f, mp, keep_volume, GUIDED_NCC); }

// ------------------------------------------------------------------------------------------
// geodesic ASW: computeAdaptiveWeight_geodesic (M.cpp:1436-1534)
// ------------------------------------------------------------------------------------------
static int run_geodesic(asw_ctx* ctx, Frame* f, const MatchParams& mp, bool keep_volume)
{
    if (mp.win % 2 == 0) return ASW_ERR_EVEN_WINDOW;  // M.cpp:1440-1443
    if (f->channels != 3) return ASW_ERR_UNSUPPORTED_LAYOUT;  // at<Vec3b>
    ASW_TRY(check_direction(mp.disparity_type));
    const int flip = mp.disparity_type == ASW_DISPARITY_RIGHT ? 1 : 0;  // M.cpp:1498-1520 == LEFT on the mirrored problem
    if (mp.win < 1 || mp.win > 35) return ASW_ERR_BAD_ARGUMENT;
    const int H = f->rows, W = f->cols, nD = method_info(ASW_ALG_ADAPTIVE_WEIGHT_GEODESIC)->planes(mp.numD);
    const size_t plane = (size_t)H * W, cells = (size_t)mp.win * mp.win;
    DevBuf& pl = ctx->buf("bgrxL");
    DevBuf& pr = ctx->buf("bgrxR");
    DevBuf& wl = ctx->buf("geoWL");
    DevBuf& wr = ctx->buf("geoWR");
    ASW_TRY(pl.ensure(plane * 4));
    ASW_TRY(pr.ensure(plane * 4));
    ASW_TRY(wl.ensure(plane * cells * 2));
    ASW_TRY(wr.ensure(plane * cells * 2));
    ASW_TRY(ensure_outputs(f, nD, keep_volume));
    ASW_TRY(launch_pack_bgrx(ctx->stream, f->L.as<uint8_t>(), H, W, pl.as<uint32_t>()));
    ASW_TRY(launch_pack_bgrx(ctx->stream, f->R.as<uint8_t>(), H, W, pr.as<uint32_t>()));
    ASW_TRY(agg_begin(ctx));
    ASW_TRY(launch_geodesic_weights_u16(ctx->stream, pl.as<uint32_t>(), H, W, mp.win, 3, wl.as<uint16_t>()));  // M.cpp:1464
    ASW_TRY(launch_geodesic_weights_u16(ctx->stream, pr.as<uint32_t>(), H, W, mp.win, 3, wr.as<uint16_t>()));  // M.cpp:1465
    double* partE = nullptr;
    float* partD = nullptr;
    if (plane <= (size_t)1 << 20)  // small frames only: scratch for the grid.z split of the disparity range
        ASW_TRY(slice_scratch(ctx, 8, plane, &partE, &partD));
    // fixed image (the one the disparity map belongs to) / other image
    const uint32_t* pf = flip ? pr.as<uint32_t>() : pl.as<uint32_t>();
    const uint32_t* po = flip ? pl.as<uint32_t>() : pr.as<uint32_t>();
    const uint16_t* wf = flip ? wr.as<uint16_t>() : wl.as<uint16_t>();
    const uint16_t* wo = flip ? wl.as<uint16_t>() : wr.as<uint16_t>();
    float* vol = keep_volume ? f->vol.as<float>() : nullptr;
    // Long candidate ranges of the 15x15 case (either direction) run as passes of the xq kernel (128 / 64 candidates each) plus
    // k_asw_geodesic for what is left (< 64 candidates); every pass leaves its winners in one slice, merged at the end with
    // the reference's strict '<' in ascending d.  ASW_GEODESIC_XQ=0 forces the one-kernel path.
    if (mp.win == 15 && nD >= geodesic_xq_pass_candidates(4) && W >= 64 && mp.minD >= 0 && ctx->tune.geodesic_xq != 0) {
        double* sE;
        float* sD;
        ASW_TRY(slice_scratch(ctx, nD / 64 + 2, plane, &sE, &sD));
        SideStreams side(ctx->stream, ctx->side);  // fork: border tiles and the leftover run beside the passes
        hipStream_t s_border = nullptr, s_left = nullptr;
        ASW_TRY(side.use(0, &s_border));
        int cb = 0, ns = 0;
        for (int nw = 8; nw >= 4; nw /= 2)
            while (nD - cb >= geodesic_xq_pass_candidates(nw)) {
                ASW_TRY(launch_geodesic_xq(ctx->stream, s_border, nw, pf, po, wf, wo, H, W, mp.minD, cb, vol,
                                           sE + (size_t)ns * plane, sD + (size_t)ns * plane, flip != 0));
                cb += geodesic_xq_pass_candidates(nw);
                ns++;
            }
        if (cb < nD) ASW_TRY(side.use(1, &s_left));
        if (cb < nD && nD - cb <= 4) {  // the reference's inclusive range: one candidate behind the passes at numDisparity = 192
            ASW_TRY(launch_asw_geodesic_few(s_left, pf, po, wf, wo, H, W, mp.minD, cb, nD, flip != 0, vol, sE + (size_t)ns * plane,
                                            sD + (size_t)ns * plane));
            ns++;
        } else if (cb < nD) {
            ASW_TRY(launch_asw_geodesic(s_left, pf, po, wf, wo, H, W, mp.win, mp.minD, nD, flip, vol, f->disp.as<float>(), sE, sD,
                                        cb, ns));
            ns++;
        }
        ASW_TRY(side.join());
        ASW_TRY(launch_merge_slices(ctx->stream, sE, sD, ns, plane, f->disp.as<float>()));
    } else
        ASW_TRY(launch_asw_geodesic(ctx->stream, pf, po, wf, wo, H, W, mp.win, mp.minD, nD, flip, vol, f->disp.as<float>(), partE, partD));
    return agg_end(ctx, 3);
}

// ------------------------------------------------------------------------------------------
// weighted-median ASW: computeAdaptiveWeight_WeightedMedian (M.cpp:3228-3383)
// ------------------------------------------------------------------------------------------
static int ensure_wmedian_tables(asw_ctx* ctx, int win, double rate_s, double rate_r)
{
    WMedianTables& t = ctx->wm;
    if (!t.lut2_cache.hit(rate_r, ctx->stream)) {
        // computeColorWeightGau: exp((d0+d1+d2)/rateR*(-1)) == exp(addWeighted(d0+d1, a, d2, a)) with
        // a = (float)(-1/rateR) (M.cpp:3177-3179); cv::exp restated as expf
        std::vector<float> lut((size_t)511 * 256);
        const float al = (float)((1.0 / rate_r) * (-1.0));
        for (int m = 0; m < 511; m++)
            for (int c = 0; c < 256; c++) {
                float arg = (float)m * al + (float)c * al;
                lut[(size_t)m * 256 + c] = expf(arg);
            }
        ASW_TRY(t.lut2_cache.upload(t.lut2, lut.data(), lut.size() * 4));
        ASW_TRY(t.lut2_cache.commit(rate_r));
    }
    const auto wd_key = std::make_tuple(rate_s, win);
    if (!t.wd_cache.hit(wd_key, ctx->stream)) {
        // computeSpaceWeightGau (M.cpp:3207-3226)
        const int h = win / 2;
        std::vector<float> wd((size_t)win * win);
        const float al = (float)((1.0 / rate_s) * (-1.0));
        for (int y = 0; y < win; y++)
            for (int x = 0; x < win; x++) {
                float v = (float)((x - h) * (x - h)) + (float)((y - h) * (y - h));
                wd[(size_t)x * win + y] = expf(v * al);
            }
        ASW_TRY(t.wd_cache.upload(t.wd, wd.data(), wd.size() * 4));
        ASW_TRY(t.wd_cache.commit(wd_key));
    }
    return ASW_OK;
}

static int run_wmedian(asw_ctx* ctx, Frame* f, const MatchParams& mp, bool keep_volume)
{
    if (mp.win % 2 == 0) return ASW_ERR_EVEN_WINDOW;  // M.cpp:3238-3241
    if (f->channels != 3) return ASW_ERR_UNSUPPORTED_LAYOUT;
    if (mp.disparity_type != ASW_DISPARITY_LEFT) return ASW_ERR_UNSUPPORTED_LAYOUT;  // App. B-7 / B-13
    if (mp.win < 1 || mp.win > 45) return ASW_ERR_BAD_ARGUMENT;  // 256-slot fast network up to 15x15, 64-bit general path up to 2048 slots
    const int H = f->rows, W = f->cols, n = mp.numD, cells = mp.win * mp.win;
    const int max_off = mp.minD + mp.numD - 1, Wb = W + max_off;
    const size_t plane = (size_t)H * W;
    ASW_TRY(ensure_wmedian_tables(ctx, mp.win, mp.rate_s, mp.rate_r));
    DevBuf& raw = ctx->buf("g_raw");
    DevBuf& wl = ctx->buf("wmWL");
    DevBuf& wr = ctx->buf("wmWR");
    ASW_TRY(raw.ensure(plane * n * 4));
    ASW_TRY(wl.ensure(plane * cells * 4));
    ASW_TRY(wr.ensure((size_t)H * Wb * cells * 4));
    ASW_TRY(ensure_outputs(f, n, keep_volume, true));  // the medians: always needed for the WTA pass
    const uint8_t* dL = f->L.as<uint8_t>();
    const uint8_t* dR = f->R.as<uint8_t>();
    ASW_TRY(build_similarity_volume(ctx, dL, dR, H, W, mp.minD, n, 0.4, 10, 50, raw.as<float>()));  // M.cpp:3250
    ASW_TRY(agg_begin(ctx));
    ASW_TRY(launch_wm_weights(ctx->stream, dL, H, W, 0, mp.win, ctx->wm.lut2.as<float>(), ctx->wm.wd.as<float>(), wl.as<float>()));
    ASW_TRY(launch_wm_weights(ctx->stream, dR, H, W, max_off, mp.win, ctx->wm.lut2.as<float>(), nullptr, wr.as<float>()));
    // 15x15 (the reference's call site): the neighbourhood of an 8x8 pixel block is sorted once per slice and every pixel walks
    // it (k_wmedian_tile.hip), 3 KB of list per block and slice; 3x3 .. 13x13, 17x17 .. 37x37: the same scheme with the window a
    // run-time parameter (k_wmedian_tile_gen.hip), 1.5 .. 12 KB; 1x1 and 39x39 .. 45x45 sort per pixel (k_wmedian.hip).  Slices go in
    // chunks that keep the sorted lists below 2 GiB.  ASW_WMEDIAN_TILE=0 forces the per-pixel sort (A/B measurements, tests).
    const bool tile15 = mp.win == 15;
    if ((tile15 || wmedian_tile_gen_supported(mp.win)) && ctx->tune.wmedian_tile != 0) {
        size_t per_slice = wmedian_tile_list_slots(H, W, 1);
        if (!tile15) per_slice = per_slice / 512 * (size_t)wmedian_tile_gen_slots(mp.win);
        int chunk = (int)std::min<size_t>((size_t)n, std::max<size_t>(8, (((size_t)2 << 30) / 6 / per_slice) / 8 * 8));
        if (ctx->tune.wmedian_tile_chunk > 0) chunk = std::max(1, std::min(n, ctx->tune.wmedian_tile_chunk));  // tests: odd chunkings
        DevBuf& lc = ctx->buf("wmListC");
        DevBuf& lp = ctx->buf("wmListP");
        ASW_TRY(lc.ensure(per_slice * chunk * 4));
        ASW_TRY(lp.ensure(per_slice * chunk * 2));
        for (int d0 = 0; d0 < n; d0 += chunk) {
            const int dn = std::min(chunk, n - d0);
            if (tile15)
                ASW_TRY(launch_wmedian_tile(ctx->stream, raw.as<float>(), wl.as<float>(), wr.as<float>(), H, W, n, max_off, d0, dn,
                                            lc.as<uint32_t>(), lp.as<uint16_t>(), f->vol.as<float>()));
            else
                ASW_TRY(launch_wmedian_tile_gen(ctx->stream, raw.as<float>(), wl.as<float>(), wr.as<float>(), H, W, mp.win, n, max_off,
                                                d0, dn, lc.as<uint32_t>(), lp.as<uint16_t>(), f->vol.as<float>(),
                                                ctx->tune.wmedian_gen_rows));
        }
    } else
        ASW_TRY(launch_wmedian(ctx->stream, raw.as<float>(), wl.as<float>(), wr.as<float>(), H, W, mp.win, n, max_off,
                               f->vol.as<float>()));
    ASW_TRY(launch_wta(ctx->stream, f->vol.as<float>(), n, H, W, mp.minD, f->disp.as<float>()));  // M.cpp:3365-3381
    return agg_end(ctx, 4);
}

// ------------------------------------------------------------------------------------------
// O(1)-bilateral ASW: computeAdaptiveWeight_BLO1 (M.cpp:2505-2725)
// ------------------------------------------------------------------------------------------
static int run_blo1(asw_ctx* ctx, Frame* f, const MatchParams& mp, bool keep_volume)
{
    if (mp.win % 2 == 0) return ASW_ERR_EVEN_WINDOW;  // getCostSAD_d -> Mat(), M.cpp:2458-2462
    if (f->channels != 3 && f->channels != 1) return ASW_ERR_UNSUPPORTED_LAYOUT;
    ASW_TRY(check_direction(mp.disparity_type));
    // the reference indexes setsJB_ks_ds_x[key][offset] with the ABSOLUTE offset (M.cpp:2659): out of range unless 0
    if (mp.minD != 0) return ASW_ERR_BAD_ARGUMENT;
    // the SAD cost comes from the walk, the aggregation from k_blo1
    if (mp.win < 1 || mp.win > std::min(blo1_max_window(), walk_max_kernel())) return ASW_ERR_BAD_ARGUMENT;
    const int step = (int)(256 * mp.blo_rate_r);  // M.cpp:2550
    if (step <= 0) return ASW_ERR_BAD_ARGUMENT;   // the reference's key loop would not terminate
    const int H = f->rows, W = f->cols, n = mp.numD;
    const size_t plane = (size_t)H * W;
    // keys 0, step, 2*step, ..., 255 (M.cpp:2551-2560) are implied by `step` in the kernel
    const uint8_t *gl, *gr;
    DevBuf& raw = ctx->buf("g_raw");
    ASW_TRY(raw.ensure(plane * n * 4));
    ASW_TRY(ensure_outputs(f, n, keep_volume));
    ASW_TRY(gray_pair(ctx, f->L.as<uint8_t>(), f->R.as<uint8_t>(), f->channels, H, W, &gl, &gr));  // M.cpp:2514-2521
    ASW_TRY(launch_cost_sad(ctx->stream, gl, gr, H, W, mp.disparity_type, mp.win, mp.minD, n, raw.as<float>()));  // M.cpp:2529-2547
    ASW_TRY(agg_begin(ctx));
    ASW_TRY(launch_blo1(ctx->stream, gl, gr, raw.as<float>(), step, H, W, mp.disparity_type, mp.win, n,
                        keep_volume ? f->vol.as<float>() : nullptr, f->disp.as<float>()));
    return agg_end(ctx, 1);
}

// computeAdaptiveWeight_bilateralGrid, M.cpp:2253-2430.  DISPARITY_LEFT only: the RIGHT branches read column `width` of the
// left image (min(x + offset, width), M.cpp:1929, 2356), one past the row.
static int run_bilgrid(asw_ctx* ctx, Frame* f, const MatchParams& mp, bool keep_volume)
{
    if (f->channels != 3 && f->channels != 1) return ASW_ERR_UNSUPPORTED_LAYOUT;
    if (mp.disparity_type != ASW_DISPARITY_LEFT) return ASW_ERR_UNSUPPORTED_LAYOUT;
    const int H = f->rows, W = f->cols, n = method_info(ASW_ALG_ADAPTIVE_WEIGHT_BILATERAL_GRID)->planes(mp.numD);
    int nx, ny, nz;
    ASW_TRY(bilgrid_dims(H, W, mp.grid_rate_s, mp.grid_rate_r, &nx, &ny, &nz));
    const size_t plane = (size_t)H * W;
    const size_t cells = (size_t)(nx + 1) * (ny + 1) * (nz + 1) * (nz + 1);
    if (cells > ((size_t)1 << 33)) return ASW_ERR_ALLOC;  // 8 G cells = 96 GB of grid
    const uint8_t *gl, *gr;
    DevBuf& gF = ctx->buf("grid_sum");
    DevBuf& gS = ctx->buf("grid_count");
    DevBuf& best = ctx->buf("grid_best");
    ASW_TRY(gF.ensure(cells * 8));
    ASW_TRY(gS.ensure(cells * 4));
    ASW_TRY(best.ensure(plane * 8));
    ASW_TRY(ensure_outputs(f, n, keep_volume));
    ASW_TRY(gray_pair(ctx, f->L.as<uint8_t>(), f->R.as<uint8_t>(), f->channels, H, W, &gl, &gr));  // M.cpp:2271-2278
    ASW_TRY(agg_begin(ctx));
    ASW_TRY(launch_bilgrid(ctx->stream, gl, gr, H, W, mp.grid_rate_s, mp.grid_rate_r, mp.minD, mp.numD, gF.as<double>(), gS.as<int>(),
                           best.as<double>(), keep_volume ? f->vol.as<float>() : nullptr, f->disp.as<float>()));
    return agg_end(ctx, 1);
}

// ------------------------------------------------------------------------------------------
// semi-global block matching: StereoSGBM MODE_SGBM_3WAY and the selector's getDisparity_SGBM
// (aswMethods.cpp:158-194)
// ------------------------------------------------------------------------------------------
int sgbm_prepare(asw_ctx* ctx, const SgbmParams& p, int H, int W, int cn, bool want_volume, SgbmLaunch* out)
{
    if (p.mode != 2) return ASW_ERR_UNSUPPORTED_METHOD;  // MODE_SGBM_3WAY only
    if (p.paths & ~ASW_SGBM_PATHS_HH) return ASW_ERR_BAD_ARGUMENT;
    if ((p.paths & ASW_SGBM_PATHS_3WAY) != ASW_SGBM_PATHS_3WAY) return ASW_ERR_UNSUPPORTED_METHOD;  // the three paths are the frame
    if (p.minD < 0 || p.numD <= 0 || p.numD % 16 != 0 || p.numD > 1024) return ASW_ERR_BAD_ARGUMENT;
    if (cn != 1 && cn != 3) return ASW_ERR_UNSUPPORTED_LAYOUT;
    if (16 * ((long long)p.minD + p.numD) > 32767) return ASW_ERR_BAD_ARGUMENT;  // the scaled map is int16
    if ((size_t)H * W >= ((size_t)1 << 31)) return ASW_ERR_BAD_ARGUMENT;         // pixel indices of the speckle filter are int
    SgbmLaunch a{};
    a.H = H; a.W = W; a.cn = cn; a.minD = p.minD; a.D = p.numD; a.paths = p.paths; a.census = p.census;
    // step 0: StereoSGBM::compute's effective parameters
    a.ftzero = std::max(p.pre_filter_cap, 15) | 1;
    a.P1 = p.P1 > 0 ? p.P1 : 2;
    a.P2 = std::max(p.P2 > 0 ? p.P2 : 5, a.P1 + 1);
    a.U = p.uniqueness_ratio < 0 ? 10 : p.uniqueness_ratio;
    a.M = p.disp12_max_diff <= 0 ? 1 : p.disp12_max_diff;
    a.w = p.block_size <= 0 ? 5 : p.block_size;
    a.speckle_window = p.speckle_window_size;
    a.speckle_range = (int)std::min<long long>(std::max(p.speckle_range, -(1 << 26)), 1 << 26);  // 16 * range stays an int
    if (a.P1 == INT_MAX) return ASW_ERR_BAD_ARGUMENT;  // P2 >= P1 + 1
    // every C, L and S is exact in int32: S <= n * (C_max + P2), n paths; the f32 volume needs the same bound below 2^24
    const double k = 2 * (a.w / 2) + 1;
    const double cmax = p.census ? 62.0 * k * k : (double)cn * (2.0 * a.ftzero + 63.0) * k * k;  // census: a Hamming distance per pixel
    const double bound = (double)__builtin_popcount(p.paths) * (cmax + a.P2);
    if (bound >= 2147483648.0) return ASW_ERR_BAD_ARGUMENT;
    if (want_volume && bound >= 16777216.0) return ASW_ERR_BAD_ARGUMENT;
    if (p.census && W > 10240) return ASW_ERR_BAD_ARGUMENT;  // k_sgbm_hcost_census stages both code rows in LDS: 16 W bytes <= 160 KB
    DevBuf& scratch = ctx->buf("sgbm_scratch");
    DevBuf& d16 = ctx->buf("sgbm_disp16");
    ASW_TRY(scratch.ensure(sgbm_scratch_bytes(H, W, cn, a.minD, a.D)));
    ASW_TRY(d16.ensure((size_t)H * W * sizeof(short)));
    a.scratch = scratch.p;
    a.disp16 = d16.as<short>();
    *out = a;
    return ASW_OK;
}

// getDisparity_SGBM: CV_Error for numDisparity % 16 != 0 or an even window (-> ASW_ERR_UNSUPPORTED_METHOD, the status of a method
// the library does not serve); the images as they are (cn 1 or 3); StereoSGBM::create(minD, numD, w) with the settings below;
// compute() -> convertTo(CV_8U, 1/16).  disparityType is ignored: both directions give the left-view map.  No volume is kept.
static int run_sgbm(asw_ctx* ctx, Frame* f, const MatchParams& mp, bool /* keep_volume: there is none to keep */)
{
    if (mp.numD % 16 != 0 || mp.win % 2 == 0) return ASW_ERR_UNSUPPORTED_METHOD;
    const int cn = f->channels, w = mp.win > 0 ? mp.win : 3;
    if (w > 4096) return ASW_ERR_BAD_ARGUMENT;  // 32 * cn * w * w stays an int (and far beyond the exactness bound anyway)
    SgbmParams p;
    p.minD = mp.minD; p.numD = mp.numD; p.block_size = w;
    p.P1 = 8 * cn * w * w; p.P2 = 32 * cn * w * w;
    p.disp12_max_diff = 200; p.pre_filter_cap = 10; p.uniqueness_ratio = 10;
    p.speckle_window_size = 175; p.speckle_range = 32; p.mode = 2;
    SgbmLaunch a;
    ASW_TRY(sgbm_prepare(ctx, p, f->rows, f->cols, cn, false, &a));
    a.L = f->L.as<uint8_t>(); a.R = f->R.as<uint8_t>();
    a.vol = nullptr;
    a.agg = {&ctx->clock, 2};
    ASW_TRY(ensure_outputs(f, 0, false));
    ASW_TRY(launch_sgbm(ctx->stream, a));
    return launch_disp16_to_u8f(ctx->stream, a.disp16, (size_t)f->rows * f->cols, f->disp.as<float>());
}

// ------------------------------------------------------------------------------------------
// block matching: StereoBM with PREFILTER_XSOBEL, behind asw_stereo_bm and asw_get_disparity_bm.  The
// selector's BM value (enum 0) is not routed here: it still returns ASW_ERR_UNSUPPORTED_METHOD.
// ------------------------------------------------------------------------------------------
int bm_prepare(asw_ctx* ctx, const BmParams& p, int H, int W, BmLaunch* out)
{
    if (p.pre_filter_type == 0) return ASW_ERR_UNSUPPORTED_METHOD;  // PREFILTER_NORMALIZED_RESPONSE is not served
    if (p.pre_filter_type != 1) return ASW_ERR_BAD_ARGUMENT;
    // StereoBM::compute's assertions (step 0)
    if (p.pre_filter_size < 5 || p.pre_filter_size > 255 || p.pre_filter_size % 2 == 0) return ASW_ERR_BAD_ARGUMENT;
    if (p.pre_filter_cap < 1 || p.pre_filter_cap > 63) return ASW_ERR_BAD_ARGUMENT;
    if (p.block_size < 5 || p.block_size > 255 || p.block_size % 2 == 0 || p.block_size > std::min(H, W)) return ASW_ERR_BAD_ARGUMENT;
    if (p.numD <= 0 || p.numD % 16 != 0) return ASW_ERR_BAD_ARGUMENT;
    if (p.texture_threshold < 0 || p.uniqueness_ratio < 0) return ASW_ERR_BAD_ARGUMENT;
    // what this library serves: minD >= 0, up to 1024 candidates, an int16 map, int pixel indices in the speckle filter
    if (p.minD < 0 || p.numD > 1024) return ASW_ERR_BAD_ARGUMENT;
    if (16 * ((long long)p.minD + p.numD) > 32767) return ASW_ERR_BAD_ARGUMENT;
    if ((size_t)H * W >= ((size_t)1 << 31)) return ASW_ERR_BAD_ARGUMENT;
    BmLaunch a{};
    a.H = H; a.W = W; a.minD = p.minD; a.D = p.numD; a.w = p.block_size; a.cap = p.pre_filter_cap;
    a.texture = p.texture_threshold; a.U = p.uniqueness_ratio; a.M = p.disp12_max_diff;
    a.speckle_window = p.speckle_window_size; a.speckle_range = p.speckle_range;
    DevBuf& scratch = ctx->buf("bm_scratch");
    DevBuf& d16 = ctx->buf("bm_disp16");
    ASW_TRY(scratch.ensure(bm_scratch_bytes(H, W)));
    ASW_TRY(d16.ensure((size_t)H * W * sizeof(short)));
    a.scratch = scratch.p;
    a.disp16 = d16.as<short>();
    *out = a;
    return ASW_OK;
}

// ------------------------------------------------------------------------------------------
// AD-Census cost (Mei et al. 2011): DESIGN.md section 4.13; not in the reference
// ------------------------------------------------------------------------------------------
// TA[v] = floor(127 (1 - exp(-v / lambda_ad)) + 0.5), v = 0..255, and TC[h] the same with lambda_census, h = 0..62, as
// TA[256] | TC[64]
static int ensure_census_tables(asw_ctx* ctx, int lambda_ad, int lambda_census)
{
    CensusTables& t = ctx->census;
    const auto key = std::make_tuple(lambda_ad, lambda_census);
    if (t.cache.hit(key, ctx->stream)) return ASW_OK;
    uint8_t tab[320] = {0};
    for (int v = 0; v < 256; v++) tab[v] = (uint8_t)floor(127.0 * (1.0 - exp(-(double)v / lambda_ad)) + 0.5);
    for (int h = 0; h < 63; h++) tab[256 + h] = (uint8_t)floor(127.0 * (1.0 - exp(-(double)h / lambda_census)) + 0.5);
    ASW_TRY(t.cache.upload(t.t, tab, sizeof(tab)));
    return t.cache.commit(key);
}

int build_census_cost(asw_ctx* ctx, const uint8_t* dL, const uint8_t* dR, int H, int W, int channels, int disparity_type, int minD,
                      int numD, int lambda_ad, int lambda_census, uint8_t* cost)
{
    const size_t plane = (size_t)H * W;
    DevBuf& cl = ctx->buf("censusL");
    DevBuf& cr = ctx->buf("censusR");
    ASW_TRY(cl.ensure(plane * sizeof(uint2)));
    ASW_TRY(cr.ensure(plane * sizeof(uint2)));
    if (lambda_ad > 0) ASW_TRY(ensure_census_tables(ctx, lambda_ad, lambda_census));
    const uint8_t *gl, *gr;
    ASW_TRY(gray_pair(ctx, dL, dR, channels, H, W, &gl, &gr));
    ASW_TRY(launch_census_transform(ctx->stream, gl, H, W, cl.as<uint2>()));
    ASW_TRY(launch_census_transform(ctx->stream, gr, H, W, cr.as<uint2>()));
    return launch_cost_census(ctx->stream, dL, dR, cl.as<uint2>(), cr.as<uint2>(), H, W, channels, disparity_type, minD, numD,
                              lambda_ad > 0 ? ctx->census.t.as<uint8_t>() : nullptr, cost);
}

// ------------------------------------------------------------------------------------------
// recursive (permeability) aggregation over the whole image (Cigla & Alatan 2013): entry 12 with an asw_alg_permeability() value;
// DESIGN.md section 4.17; not in the reference
// ------------------------------------------------------------------------------------------
static int ensure_perm_table(asw_ctx* ctx, int sigma)
{
    PermTable& t = ctx->perm;
    if (t.cache.hit(sigma, ctx->stream)) return ASW_OK;
    double tab[256];
    for (int k = 0; k < 256; k++) tab[k] = (double)(float)exp(-(double)k / sigma);  // rounded to f32 here: the kernels see doubles only
    ASW_TRY(t.cache.upload(t.t, tab, sizeof(tab)));
    return t.cache.commit(sigma);
}

// win is not read: the support is the whole image
static int run_permeability(asw_ctx* ctx, Frame* f, const MatchParams& mp, bool keep_volume)
{
    if (f->channels != 3 && f->channels != 1) return ASW_ERR_UNSUPPORTED_LAYOUT;  // what asw_cost_ad takes
    ASW_TRY(check_direction(mp.disparity_type));
    if (mp.perm_sigma < 1 || mp.perm_sigma > 255 || mp.perm_trunc < 1 || mp.perm_trunc > 255) return ASW_ERR_BAD_ARGUMENT;
    const int H = f->rows, W = f->cols, n = mp.numD;
    if ((size_t)H * W >= ((size_t)1 << 31)) return ASW_ERR_BAD_ARGUMENT;  // as entry 12; the scan kernels ask nothing else of a frame
    const size_t plane = (size_t)H * W;
    const size_t ck_per = std::max((size_t)H * perm_segments(W), (size_t)W * perm_segments(H));  // checkpoints of one candidate
    const size_t ph_doubles = (size_t)H * perm_padded(W), pv_doubles = (size_t)W * perm_padded(H);
    // candidates per chunk: horizontal sums + checkpoints of a chunk and the per-frame planes stay within 2 GiB; whole wavefronts of
    // 64 candidates where the range does not fit one chunk.  ASW_PERM_CHUNK forces another size (tests): the result is the same
    // per frame: best E, N's own horizontal sums and checkpoints, ph, pv and N (transposed, padded like pv), the plane of ones
    const size_t fixed = (2 * plane + ck_per + ph_doubles + 2 * pv_doubles) * sizeof(double) + plane, per_cand = (plane + ck_per) * sizeof(double);
    const size_t budget = (size_t)2 << 30;
    size_t fit = budget > fixed + per_cand ? (budget - fixed) / per_cand : 1;
    int chunk = (int)std::min<size_t>(fit, (size_t)std::min(n, 4096));
    if (chunk < n && chunk >= 64) chunk = chunk / 64 * 64;
    if (ctx->tune.perm_chunk > 0) chunk = std::max(1, std::min(std::min(n, 4096), ctx->tune.perm_chunk));
    const int chunks = (n + chunk - 1) / chunk;
    ASW_TRY(ensure_perm_table(ctx, mp.perm_sigma));
    DevBuf& raw = ctx->buf("cross_cost");  // the u8 AD volume, as entry 12 keeps it
    DevBuf& ones = ctx->buf("perm_ones");
    DevBuf& ph = ctx->buf("perm_ph");
    DevBuf& pv = ctx->buf("perm_pv");
    DevBuf& ck = ctx->buf("perm_ck");
    DevBuf& hs = ctx->buf("perm_hs");
    DevBuf& nrm = ctx->buf("perm_n");
    DevBuf& nck = ctx->buf("perm_n_ck");  // N's scans run beside the first chunk's horizontal pass: scratch of their own
    DevBuf& nhs = ctx->buf("perm_n_hs");
    DevBuf& best = ctx->buf("perm_best");
    ASW_TRY(raw.ensure(plane * n));
    ASW_TRY(ones.ensure(plane));
    ASW_TRY(ph.ensure(ph_doubles * sizeof(double)));
    ASW_TRY(pv.ensure(pv_doubles * sizeof(double)));
    ASW_TRY(ck.ensure(ck_per * chunk * sizeof(double)));
    ASW_TRY(hs.ensure(plane * chunk * sizeof(double)));
    ASW_TRY(nrm.ensure(pv_doubles * sizeof(double)));
    ASW_TRY(nck.ensure(ck_per * sizeof(double)));
    ASW_TRY(nhs.ensure(plane * sizeof(double)));
    ASW_TRY(best.ensure(plane * sizeof(double)));
    ASW_TRY(ensure_outputs(f, n, keep_volume));
    const uint8_t* dL = f->L.as<uint8_t>();
    const uint8_t* dR = f->R.as<uint8_t>();
    ASW_TRY(launch_cost_ad(ctx->stream, dL, dR, H, W, f->channels, mp.disparity_type, mp.minD, n, 0, 0, raw.as<uint8_t>()));
    ASW_HIP_TRY(hipMemsetAsync(ones.p, 1, plane, ctx->stream));
    ASW_TRY(agg_begin(ctx));
    ASW_TRY(launch_perm_weights(ctx->stream, mp.disparity_type == ASW_DISPARITY_RIGHT ? dR : dL, H, W, f->channels, ctx->perm.t.as<double>(),
                                ph.as<double>(), pv.as<double>()));
    PermLaunch a;
    a.H = H; a.W = W; a.trunc = mp.perm_trunc; a.minD = mp.minD;
    a.ph = ph.as<double>(); a.pvT = pv.as<double>(); a.ck = ck.as<double>(); a.hs = hs.as<double>();
    a.bestE = best.as<double>(); a.disp = f->disp.as<float>();
    // N: the two passes over a plane of ones, through the kernels every candidate goes through.  One lane of a wavefront works and
    // the scans are as long as any: on a side stream they run beside the first chunk's horizontal pass, which does not need N
    PermLaunch nl = a;
    nl.cost = ones.as<uint8_t>(); nl.nc = 1; nl.cbeg = 0; nl.first = 1; nl.ck = nck.as<double>(); nl.hs = nhs.as<double>();
    nl.N = nullptr; nl.Nout = nrm.as<double>(); nl.vol = nullptr;
    SideStreams side(ctx->stream, ctx->side);
    hipStream_t s_n = nullptr;
    ASW_TRY(side.use(0, &s_n));  // fork: behind the permeability planes
    ASW_TRY(launch_perm_scan_h(s_n, nl));
    ASW_TRY(launch_perm_scan_v(s_n, nl));
    a.N = nrm.as<double>(); a.Nout = nullptr; a.vol = keep_volume ? f->vol.as<float>() : nullptr;
    for (int c0 = 0; c0 < n; c0 += chunk) {  // ascending: the vertical pass merges a chunk's winners into the running minimum
        a.cost = raw.as<uint8_t>() + (size_t)c0 * plane; a.nc = std::min(chunk, n - c0); a.cbeg = c0; a.first = c0 == 0;
        ASW_TRY(launch_perm_scan_h(ctx->stream, a));
        if (c0 == 0) ASW_TRY(side.join());  // the vertical pass divides by N
        ASW_TRY(launch_perm_scan_v(ctx->stream, a));
    }
    return agg_end(ctx, 4 + 2 * chunks);  // two permeability planes, N's two passes, two passes per chunk
}

// ------------------------------------------------------------------------------------------
// cross-based support regions (Zhang, Lu, Lafruit 2009): DESIGN.md section 4.12; not in the reference
// ------------------------------------------------------------------------------------------
static int run_cross(asw_ctx* ctx, Frame* f, const MatchParams& mp, bool keep_volume)
{
    if (mp.permeability) return run_permeability(ctx, f, mp, keep_volume);  // no window: before the window checks
    if (mp.win % 2 == 0) return ASW_ERR_EVEN_WINDOW;
    if (mp.win < 1 || mp.win > 35) return ASW_ERR_BAD_ARGUMENT;
    if (f->channels != 3 && f->channels != 1) return ASW_ERR_UNSUPPORTED_LAYOUT;  // what asw_cost_ad takes
    ASW_TRY(check_direction(mp.disparity_type));
    if (mp.cross_tau < 0 || mp.cross_tau > 255 || mp.cross_trunc < 1 || mp.cross_trunc > 255) return ASW_ERR_BAD_ARGUMENT;
    const int H = f->rows, W = f->cols, n = mp.numD;
    // the sums the kernel keeps are local to a tile (a row prefix < 255 * 99, a column prefix < 255 * 35 * 66): no frame can take them
    // out of int32; what a frame can overflow is the int row / column arithmetic on H and W
    if ((size_t)H * W >= ((size_t)1 << 31)) return ASW_ERR_BAD_ARGUMENT;
    if (H > 4 * 65535) return ASW_ERR_BAD_ARGUMENT;  // the arm kernels put four rows on a workgroup of grid.y
    const size_t plane = (size_t)H * W;
    DevBuf& raw = ctx->buf("cross_cost");   // u8 cost volume (AD, or AD-Census): a quarter of the f32 volume
    DevBuf& arms = ctx->buf("cross_arms");
    DevBuf& cnt = ctx->buf("cross_count");
    ASW_TRY(raw.ensure(plane * n));
    ASW_TRY(arms.ensure(plane * sizeof(uint32_t)));
    ASW_TRY(cnt.ensure(plane * sizeof(uint16_t)));
    ASW_TRY(ensure_outputs(f, n, keep_volume));
    const uint8_t* dL = f->L.as<uint8_t>();
    const uint8_t* dR = f->R.as<uint8_t>();
    if (mp.cross_cost == 1)
        ASW_TRY(build_census_cost(ctx, dL, dR, H, W, f->channels, mp.disparity_type, mp.minD, n, mp.lambda_ad, mp.lambda_census,
                                  raw.as<uint8_t>()));
    else
        ASW_TRY(launch_cost_ad(ctx->stream, dL, dR, H, W, f->channels, mp.disparity_type, mp.minD, n, 0, 0, raw.as<uint8_t>()));
    ASW_TRY(agg_begin(ctx));
    ASW_TRY(launch_cross_arms(ctx->stream, mp.disparity_type == ASW_DISPARITY_RIGHT ? dR : dL, H, W, f->channels, mp.win, mp.cross_tau,
                              arms.as<uint32_t>(), cnt.as<uint16_t>()));
    ASW_TRY(launch_cross_aggregate(ctx->stream, raw.as<uint8_t>(), arms.as<uint32_t>(), cnt.as<uint16_t>(), H, W, mp.win, mp.cross_trunc,
                                   mp.minD, n, keep_volume ? f->vol.as<float>() : nullptr, f->disp.as<float>()));
    return agg_end(ctx, 3);  // arms, region sizes, aggregation + WTA
}

// ------------------------------------------------------------------------------------------
// the method table: one row per value of the selector's enum (M.cpp:49-87), in the enum's order.  A new method is a row here, its
// runner above and its enum value in asw_mi355x.h.
// ------------------------------------------------------------------------------------------
static const MethodInfo k_methods[] = {
    // {extra planes, no volume, ignores disparity_type, no sub-pixel, packed parameters}, algorithm, runner
    {{0, true, true, false, false}, ASW_ALG_BM, nullptr},     // served by asw_stereo_bm / asw_get_disparity_bm only
    {{0, true, true, false, false}, ASW_ALG_SGBM, run_sgbm},  // asw_sgbm has the volume S
    {{1, false, false, false, false}, ASW_ALG_ADAPTIVE_WEIGHT, run_bilateral_classic},  // offset <= max_offset, M.cpp:1021,1074
    {{1, false, false, false, false}, ASW_ALG_ADAPTIVE_WEIGHT_8DIRECT, run_direct8},    // M.cpp:1171
    {{1, false, false, false, false}, ASW_ALG_ADAPTIVE_WEIGHT_GEODESIC, run_geodesic},  // M.cpp:1447,1467
    {{1, false, false, false, false}, ASW_ALG_ADAPTIVE_WEIGHT_BILATERAL_GRID, run_bilgrid},  // M.cpp:2256,2280
    {{0, false, false, false, false}, ASW_ALG_ADAPTIVE_WEIGHT_BLO1, run_blo1},
    {{0, false, false, false, false}, ASW_ALG_ADAPTIVE_WEIGHT_GUIDED_FILTER, run_guided_sad6},
    {{0, false, false, false, false}, ASW_ALG_ADAPTIVE_WEIGHT_GUIDED_FILTER_2, run_guided_sim3},
    {{0, false, false, false, false}, ASW_ALG_ADAPTIVE_WEIGHT_GUIDED_FILTER_3, run_guided_ncc},
    {{0, false, false, false, false}, ASW_ALG_ADAPTIVE_WEIGHT_MEDIAN, run_wmedian},
    // computeNCC's disparity overload has its own candidate range and no selector volume in the RIGHT view
    {{0, false, false, true, false}, ASW_ALG_NCC, run_ncc},
    {{0, false, false, false, true}, ASW_ALG_ADAPTIVE_WEIGHT_CROSS, run_cross},
};

const MethodInfo* method_info(int method)
{
    const int n = (int)(sizeof(k_methods) / sizeof(k_methods[0]));
    return method >= 0 && method < n && k_methods[method].algorithm == method ? &k_methods[method] : nullptr;
}

// The four paths over the runner's volume, their sum over it, and its winner (k_scanline.hip)
static int run_scanline(asw_ctx* ctx, Frame* f, const MethodInfo* m, const MatchParams& mp)
{
    ScanlineLaunch a;
    a.H = f->rows; a.W = f->cols; a.n = m->planes(mp.numD); a.minD = mp.minD; a.P1 = mp.scan_p1; a.P2 = mp.scan_p2;
    DevBuf& sum = ctx->buf("scan_sum");
    DevBuf& ck = ctx->buf("scan_ck");
    ASW_TRY(sum.ensure((size_t)a.n * a.H * a.W * sizeof(float)));
    ASW_TRY(ck.ensure(std::max<size_t>(scanline_checkpoint_floats(a.H, a.W, a.n), 1) * sizeof(float)));
    a.vol = f->vol.as<float>(); a.sum = sum.as<float>(); a.ck = ck.as<float>(); a.disp = f->disp.as<float>();
    return launch_scanline(ctx->stream, a);
}

// The method on every level of the pair's 2x2-mean pyramid, coarsest first, then the combination of the levels' volumes and its
// winner (k_cross_scale.hip).  Everything goes on the context's stream; the coarse pairs and volumes live in ctx->coarse, the
// runners' named scratch is reused level after level.  The finest level runs last: the clock's aggregate marks stay on it.
static int run_cross_scale(asw_ctx* ctx, Frame* f, const MethodInfo* m, const MatchParams& mp, bool store)
{
    static_assert(DT_CROSS_SCALES.hi == CROSS_SCALE_MAX, "the levels decode_disparity_type accepts are those ctx->coarse holds");
    const int S = mp.cross_scales;
    CrossScaleLaunch a;
    const Frame* src = f;
    for (int s = 1; s < S; s++) {
        Frame* c = &ctx->coarse[s - 1];
        c->valid = false;
        c->rows = (src->rows + 1) / 2; c->cols = (src->cols + 1) / 2; c->channels = src->channels;
        const size_t bytes = (size_t)c->rows * c->cols * c->channels;
        ASW_TRY(c->L.ensure(bytes));
        ASW_TRY(c->R.ensure(bytes));
        ASW_TRY(launch_pyramid_down(ctx->stream, src->L.as<uint8_t>(), src->rows, src->cols, src->channels, c->L.as<uint8_t>()));
        ASW_TRY(launch_pyramid_down(ctx->stream, src->R.as<uint8_t>(), src->rows, src->cols, src->channels, c->R.as<uint8_t>()));
        c->valid = true;
        src = c;
    }
    for (int s = S - 1; s >= 1; s--) {
        Frame* c = &ctx->coarse[s - 1];
        MatchParams ms = mp;
        cross_scale_range(m, mp, s, &ms.minD, &ms.numD);
        ASW_TRY(m->run(ctx, c, ms, true));
        a.cv[s - 1] = c->vol.as<float>(); a.cH[s - 1] = c->rows; a.cW[s - 1] = c->cols; a.cminD[s - 1] = ms.minD;
    }
    ASW_TRY(m->run(ctx, f, mp, true));
    a.vol = f->vol.as<float>(); a.disp = f->disp.as<float>();
    a.H = f->rows; a.W = f->cols; a.n = m->planes(mp.numD); a.minD = mp.minD; a.S = S; a.store = store ? 1 : 0;
    cross_scale_weights(S, mp.cross_lambda_q, a.w);
    return launch_cross_scale_combine(ctx->stream, a);
}

int run_method(asw_ctx* ctx, Frame* f, int algorithm, const MatchParams& mp_in, bool keep_volume, bool sync, bool confidence)
{
    f->invalidate_results();  // whatever the slot's disparity / volume were, they are not this call's
    MatchParams mp = mp_in;
    if (mp.numD <= 0 || mp.minD < 0) return ASW_ERR_BAD_ARGUMENT;
    ASW_TRY(decode_algorithm(algorithm, &algorithm, &mp, method_info));  // an asw_alg_*() value -> the plain one + its parameters
    const MethodInfo* m = method_info(algorithm);
    ASW_TRY(decode_disparity_type(m, m && m->run, scanline_max_planes(), mp));  // the flags: every refusal before any work
    // the confidence is read off a selector volume with the selector's candidate range: no volume (SGBM, BM, a value outside the
    // table) or a range of its own (NCC) is refused like a sub-pixel flag on NCC
    if (confidence && (!m || !m->run || m->no_volume || m->no_subpixel)) return ASW_ERR_UNSUPPORTED_METHOD;
    // the sub-pixel and confidence kernels read the aggregated volume: the methods that can skip it (bilateral / direct8, geodesic,
    // BLO1, the bilateral grid) are asked for it; what the CALLER keeps is decided below
    const bool want_volume = keep_volume || mp.subpixel != 0 || mp.scan_p1 != 0 || confidence;
    ASW_HIP_TRY(hipSetDevice(ctx->device));
    ASW_TRY(ctx->clock.begin_total());
    int rc;
    if (mp.cross_scales)  // every level's volume is wanted; the combined one is stored over the finest only for a reader
        rc = run_cross_scale(ctx, f, m, mp, want_volume);
    else
        rc = m && m->run ? m->run(ctx, f, mp, want_volume) : ASW_ERR_UNSUPPORTED_METHOD;
    if (rc == ASW_OK && mp.scan_p1 != 0)  // like the sub-pixel step: behind the aggregation events
        rc = run_scanline(ctx, f, m, mp);
    if (rc == ASW_OK && mp.subpixel)  // after the aggregation events: counts in total_ms and cost_ms, not in aggregate_ms
        rc = launch_subpixel(ctx->stream, mp.subpixel, f->vol.as<float>(), m->planes(mp.numD), f->rows, f->cols,
                             mp.minD, f->disp.as<float>());
    if (rc == ASW_OK && confidence) {  // of the volume the call returns, beside the final map; timed like the sub-pixel step
        rc = f->dconf.ensure((size_t)f->rows * f->cols * sizeof(float2));
        if (rc == ASW_OK)
            rc = launch_confidence(ctx->stream, f->vol.as<float>(), m->planes(mp.numD), f->rows, f->cols, f->disp.as<float>(),
                                   f->dconf.as<float2>());
    }
    if (rc != ASW_OK) {
        f->invalidate_results();
        return rc;
    }
    const size_t kept_floats = keep_volume ? f->vol_floats : 0;  // a volume asked for by the sub-pixel step alone is not the caller's
    f->vol_floats = 0;  // restored together with has_disp once nothing can fail any more
    ASW_TRY(ctx->clock.finish(sync));  // !sync: pipelined callers (batch scheduler) order and wait on the stream themselves
    f->has_disp = true; f->disp_rows = f->rows; f->disp_cols = f->cols; f->vol_floats = kept_floats; f->has_conf = confidence;
    return ASW_OK;
}

extern "C" int asw_match_resident(asw_ctx* ctx, int slot, int disparity_type, int algorithm, int win_size,
                                  int min_disparity, int num_disparity, int keep_volume)
{
    if (!ctx) return ASW_ERR_BAD_ARGUMENT;
    Frame* f = frame_slot(ctx, slot, false);
    if (!f || !f->valid) return ASW_ERR_NO_FRAME;
    return run_method(ctx, f, algorithm, match_params(disparity_type, win_size, min_disparity, num_disparity), keep_volume != 0);
}

// ------------------------------------------------------------------------------------------
// left-right refinement: cross-check, scan-line fill, weighted median (not in the reference)
// ------------------------------------------------------------------------------------------
static int check_refine_frame(int rows, int cols)
{
    if (rows <= 0 || cols <= 0 || (size_t)rows * cols >= ((size_t)1 << 31) || rows > 4 * 65535) return ASW_ERR_BAD_ARGUMENT;
    return ASW_OK;
}

int check_refine_params(const RefineParams& p, int rows, int cols, int channels)
{
    ASW_TRY(check_refine_frame(rows, cols));
    if (p.n < 1 || p.n > 1025 || p.minD < -(1 << 20) || p.minD > (1 << 20)) return ASW_ERR_BAD_ARGUMENT;
    if (!(p.max_diff >= 0)) return ASW_ERR_BAD_ARGUMENT;
    if (p.win < 1 || p.win > 35 || p.win % 2 == 0) return ASW_ERR_BAD_ARGUMENT;
    if (!(p.gamma_c > 0) || !(p.gamma_s > 0)) return ASW_ERR_BAD_ARGUMENT;
    if (channels != 1 && channels != 3) return ASW_ERR_UNSUPPORTED_LAYOUT;
    return ASW_OK;
}

static int ensure_refine_tables(asw_ctx* ctx, int win, double gamma_c, double gamma_s, int channels)
{
    RefineTables& t = ctx->refine;
    const auto key = std::make_tuple(win, gamma_c, gamma_s, channels);
    if (t.cache.hit(key, ctx->stream)) return ASW_OK;
    const int k = win / 2, ntc = 255 * channels + 1;
    std::vector<unsigned> tc(ntc), ts((size_t)(k + 1) * (k + 1));
    for (int c = 0; c < ntc; c++) tc[c] = (unsigned)floor(4096.0 * exp(-(double)c / gamma_c) + 0.5);
    for (int j = 0; j <= k; j++)
        for (int i = 0; i <= k; i++) ts[(size_t)j * (k + 1) + i] = (unsigned)floor(256.0 * exp(-sqrt((double)(i * i + j * j)) / gamma_s) + 0.5);
    ASW_TRY(t.cache.upload(t.tc, tc.data(), tc.size() * sizeof(unsigned)));
    ASW_TRY(t.cache.upload(t.ts, ts.data(), ts.size() * sizeof(unsigned)));
    t.ntc = ntc;
    return t.cache.commit(key);
}

int run_refine(asw_ctx* ctx, const uint8_t* guide, int channels, const float* dl, const float* dr, int H, int W, const RefineParams& p,
               float* out, int* n_rejected, int* n_unfillable)
{
    ASW_TRY(check_refine_params(p, H, W, channels));
    ASW_TRY(ensure_refine_tables(ctx, p.win, p.gamma_c, p.gamma_s, channels));
    const size_t plane = (size_t)H * W;
    DevBuf& mask = ctx->buf("refine_mask");
    DevBuf& F = ctx->buf("refine_fill");
    DevBuf& cnt = ctx->buf("refine_count");
    ASW_TRY(mask.ensure(plane));
    ASW_TRY(F.ensure(plane * sizeof(unsigned short)));
    ASW_TRY(cnt.ensure(3 * sizeof(unsigned)));
    RefineLaunch a;
    a.guide = guide; a.C = channels; a.dl = dl; a.dr = dr; a.H = H; a.W = W; a.minD = p.minD; a.n = p.n; a.max_diff = p.max_diff;
    a.win = p.win; a.tc = ctx->refine.tc.as<unsigned>(); a.ntc = ctx->refine.ntc; a.ts = ctx->refine.ts.as<unsigned>();
    a.mask = mask.as<uint8_t>(); a.F = F.as<unsigned short>(); a.out = out; a.counters = cnt.as<unsigned>();
    ASW_TRY(launch_refine(ctx->stream, a));
    unsigned c[3] = {0, 0, 0};
    ASW_HIP_TRY(hipMemcpyAsync(c, cnt.p, sizeof(c), hipMemcpyDeviceToHost, ctx->stream));
    ASW_HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (c[2]) return ASW_ERR_BAD_ARGUMENT;  // step 0: some dl is not an integer in [minD, minD + n)
    if (n_rejected) *n_rejected = (int)c[0];
    if (n_unfillable) *n_unfillable = (int)c[1];
    return ASW_OK;
}

// ------------------------------------------------------------------------------------------
// confidence-weighted edge-aware smoothing: the fast global smoother (not in the reference)
// ------------------------------------------------------------------------------------------
int check_smooth_params(int rows, int cols, int channels, int word, double sigma_c, double lambda, bool wants_mask, int* iterations)
{
    ASW_TRY(check_refine_frame(rows, cols));
    const int T = word & ~ASW_REFINE_SMOOTH;
    if (!(word & ASW_REFINE_SMOOTH) || T < 1 || T > 8) return ASW_ERR_BAD_ARGUMENT;  // a stray bit makes T large (or the word negative)
    if (!(sigma_c > 0 && sigma_c <= DBL_MAX) || !(lambda > 0 && lambda <= DBL_MAX)) return ASW_ERR_BAD_ARGUMENT;  // NaN fails both
    if (wants_mask) return ASW_ERR_BAD_ARGUMENT;
    if (channels != 1 && channels != 3) return ASW_ERR_UNSUPPORTED_LAYOUT;
    *iterations = T;
    return ASW_OK;
}

static int ensure_smooth_table(asw_ctx* ctx, double sigma_c, int channels)
{
    SmoothTable& t = ctx->smooth;
    const auto key = std::make_tuple(sigma_c, channels);
    if (t.cache.hit(key, ctx->stream)) return ASW_OK;
    std::vector<double> wt((size_t)255 * channels + 1);
    for (size_t k = 0; k < wt.size(); k++) wt[k] = floor(65536.0 * exp(-(double)k / sigma_c) + 0.5) / 65536.0;
    ASW_TRY(t.cache.upload(t.t, wt.data(), wt.size() * sizeof(double)));
    return t.cache.commit(key);
}

int run_smooth(asw_ctx* ctx, const uint8_t* guide, int channels, const float* d, const float* c, int stride, int H, int W,
               int iterations, double sigma_c, double lambda, float* out)
{
    ASW_TRY(ensure_smooth_table(ctx, sigma_c, channels));
    const size_t plane = (size_t)H * W;
    DevBuf& nd = ctx->buf("smooth_nd");        // N | D
    DevBuf& fwd = ctx->buf("smooth_forward");  // cp | fN | fD
    DevBuf& link = ctx->buf("smooth_links");   // vertical | horizontal (transposed)
    ASW_TRY(nd.ensure(plane * 2 * sizeof(double)));
    ASW_TRY(fwd.ensure(plane * 3 * sizeof(double)));
    ASW_TRY(link.ensure(plane * 2 * sizeof(uint16_t)));
    SmoothLaunch a;
    a.guide = guide; a.C = channels; a.d = d; a.c = c; a.stride = stride; a.H = H; a.W = W; a.T = iterations; a.lambda = lambda;
    a.Wt = ctx->smooth.t.as<double>();
    a.N = nd.as<double>(); a.D = a.N + plane;
    a.cp = fwd.as<double>(); a.fN = a.cp + plane; a.fD = a.fN + plane;
    a.linkV = link.as<uint16_t>(); a.linkHT = a.linkV + plane;
    a.out = out;
    return launch_smooth(ctx->stream, a);
}

// match_refined under ASW_REFINE_SMOOTH: the smoothing's own checks first (nothing is computed for a call that would be refused
// after its match), then one LEFT match with its confidence under the checks of a plain match, then the smoothing of the frame's
// {disparity, confidence} pairs into the frame's map.  The pairs no longer describe that map afterwards.
static int match_smoothed(asw_ctx* ctx, Frame* f, int algorithm, int win_size, int min_disparity, int num_disparity, int word,
                          double sigma_c, double lambda)
{
    f->invalidate_results();
    int T = 0;
    ASW_TRY(check_smooth_params(f->rows, f->cols, f->channels, word, sigma_c, lambda, false, &T));
    ASW_TRY(run_method(ctx, f, algorithm, match_params(ASW_DISPARITY_LEFT, win_size, min_disparity, num_disparity), false, true, true));
    f->invalidate_results();  // whatever fails from here on, the slot holds no result
    const float* pairs = f->dconf.as<float>();
    ASW_TRY(ctx->clock.timed_step(ctx->clock.timing /* the match and its confidence */, [&] {
        return run_smooth(ctx, f->L.as<uint8_t>(), f->channels, pairs, pairs + 1, 2, f->rows, f->cols, T, sigma_c, lambda,
                          f->disp.as<float>());
    }));
    f->has_disp = true; f->disp_rows = f->rows; f->disp_cols = f->cols;
    return ASW_OK;
}

// Both directions of `algorithm` (RIGHT, then LEFT), each WTA map swapped out of the frame into context scratch as soon as it exists (the second
// match cannot overwrite the first, nothing travels through the host), then the refinement into the frame's own map.
int match_refined(asw_ctx* ctx, Frame* f, int algorithm, int win_size, int min_disparity, int num_disparity, float max_diff,
                  int refine_win, double gamma_c, double gamma_s, int* n_rejected, int* n_unfillable)
{
    if (refine_win > 0 && (refine_win & ASW_REFINE_SMOOTH))  // no window has bit 30: asw_match_smoothed_resident / asw_stereo_match_smoothed
        return match_smoothed(ctx, f, algorithm, win_size, min_disparity, num_disparity, refine_win, gamma_c, gamma_s);
    f->invalidate_results();
    const MethodInfo* m = method_info(algorithm);
    if (m && m->no_volume) return ASW_ERR_UNSUPPORTED_METHOD;  // SGBM / BM carry their own disp12MaxDiff
    if (num_disparity <= 0 || min_disparity < 0) return ASW_ERR_BAD_ARGUMENT;  // as a plain match (run_method)
    int plain;  // unused: a bad asw_alg_cross() / asw_alg_adcensus() value is refused here with its own status, as a plain match refuses it
    ASW_TRY(decode_algorithm(algorithm, &plain, nullptr, method_info));
    RefineParams rp;
    rp.minD = min_disparity; rp.n = asw_volume_planes(algorithm, num_disparity); rp.max_diff = max_diff; rp.win = refine_win;
    rp.gamma_c = gamma_c; rp.gamma_s = gamma_s;
    if (rp.n == 0) return ASW_ERR_UNSUPPORTED_METHOD;
    ASW_TRY(check_refine_params(rp, f->rows, f->cols, f->channels));
    MatchParams mp = match_params(ASW_DISPARITY_RIGHT, win_size, min_disparity, num_disparity);
    DevBuf* side[2] = {&ctx->buf("refine_left"), &ctx->buf("refine_right")};
    asw_timing sum = {0, 0, 0, 0};
    for (int dt = 1; dt >= 0; dt--) {  // RIGHT first: a method whose right branch is not served is refused before any work
        mp.disparity_type = dt == 0 ? ASW_DISPARITY_LEFT : ASW_DISPARITY_RIGHT;
        ASW_TRY(run_method(ctx, f, algorithm, mp, false));
        std::swap(f->disp, *side[dt]);
        f->invalidate_results();
        sum.total_ms += ctx->clock.timing.total_ms; sum.aggregate_ms += ctx->clock.timing.aggregate_ms;
        sum.aggregate_launches += ctx->clock.timing.aggregate_launches;
    }
    ASW_TRY(f->disp.ensure((size_t)f->rows * f->cols * sizeof(float)));
    ASW_TRY(ctx->clock.timed_step(sum, [&] {
        return run_refine(ctx, f->L.as<uint8_t>(), f->channels, side[0]->as<float>(), side[1]->as<float>(), f->rows, f->cols, rp,
                          f->disp.as<float>(), n_rejected, n_unfillable);
    }));
    f->has_disp = true; f->disp_rows = f->rows; f->disp_cols = f->cols;
    return ASW_OK;
}

extern "C" int asw_match_refined_resident(asw_ctx* ctx, int slot, int algorithm, int win_size, int min_disparity, int num_disparity,
                                          float max_diff, int refine_win, double gamma_c, double gamma_s, int* n_rejected,
                                          int* n_unfillable)
{
    if (!ctx) return ASW_ERR_BAD_ARGUMENT;
    Frame* f = frame_slot(ctx, slot, false);
    if (!f || !f->valid) return ASW_ERR_NO_FRAME;
    ASW_HIP_TRY(hipSetDevice(ctx->device));
    return match_refined(ctx, f, algorithm, win_size, min_disparity, num_disparity, max_diff, refine_win, gamma_c, gamma_s, n_rejected,
                         n_unfillable);
}

// ---- internal hooks of the batch scheduler (batch.hip): device buffers of a slot, enqueue without waiting ----
int asw_internal_stage_slot(asw_ctx* ctx, int slot, int rows, int cols, int channels, Frame** out)
{
    Frame* f = frame_slot(ctx, slot, true);
    if (!f) return ASW_ERR_BAD_ARGUMENT;
    const size_t bytes = (size_t)rows * cols * channels;
    ASW_TRY(f->L.ensure(bytes));
    ASW_TRY(f->R.ensure(bytes));
    ASW_TRY(f->disp.ensure((size_t)rows * cols * 4));
    f->rows = rows; f->cols = cols; f->channels = channels; f->valid = true;
    f->invalidate_results();
    *out = f;
    return ASW_OK;
}

int asw_internal_enqueue_match(asw_ctx* ctx, int slot, int disparity_type, int algorithm, int win_size, int min_disparity,
                               int num_disparity)
{
    Frame* f = frame_slot(ctx, slot, false);
    if (!f || !f->valid) return ASW_ERR_NO_FRAME;
    return run_method(ctx, f, algorithm, match_params(disparity_type, win_size, min_disparity, num_disparity), false, false);
}

int asw_internal_check_pair(const asw_image* l, const asw_image* r, const asw_image* d)
{
    ASW_TRY(check_pair(l, r));
    return check_disp_out(d, l->rows, l->cols);
}

