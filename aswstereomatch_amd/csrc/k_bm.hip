// Block matching, StereoBM (PREFILTER_XSOBEL) + validateDisparity as DESIGN.md section 4.9 states them (OpenCV 4.1.0
// stereobm.cpp).  Integer arithmetic throughout: a block SAD is below 126 * 255^2 < 2^23, so every sum is exact in int32 and f32.
//
// Candidate index k = 0..D-1 <-> disparity minD + D - 1 - k (OpenCV's order); lofs = minD + D - 1 is the first column OpenCV
// computes.  The window column c of a computed column reads the left image at clamp(c, 0, W-1) and the right image at
// clamp(c - lofs, 0, W - D) + k: OpenCV's lptr / rptr clamps, each image on its own.
//
//   k_bm_prefilter  step 1 for both images (u8 out)
//   k_bm_match      steps 3-4: one wavefront per tile of TX computed columns and a strip of valid rows, candidates in lanes
//                   (k = c * 64 + lane, NPL = ceil(D / 64) per lane); writes the int16 disparity and the int32 cost sad[mind] of
//                   each computed pixel, and the SAD volume only when the caller asks for it
//   k_bm_lrkey      step 6, first pass: min of (cost, x) per target column x2 (packed 64-bit atomicMin: the first x wins a tie)
//   k_bm_finish     step 6, second pass, and FILTERED outside the valid region
// getDisparity_BM's convertTo(CV_8U, 1/16) is k_sgbm.hip's k_disp16_to_u8 (launch_disp16_to_u8).
#include <limits.h>

#include <algorithm>

#include "asw_internal.h"
#include "asw_device.h"
#include "asw_host.h"

namespace {

// x-Sobel of rows y-1, y, y+1 (BORDER_REFLECT_101), clamp(v, -cap, cap) + cap; columns 0 and W-1 and, with an odd H, the whole
// last row hold cap (prefilterXSobel works on row pairs).  blockIdx.y: 0 left, 1 right.
__global__ __launch_bounds__(256) void k_bm_prefilter(const uint8_t* __restrict__ L, const uint8_t* __restrict__ R, int H, int W,
                                                      int cap, uint8_t* __restrict__ out)
{
    const size_t plane = (size_t)H * W;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= plane) return;
    const uint8_t* img = blockIdx.y ? R : L;
    const int y = (int)(i / W), x = (int)(i % W);
    int v = cap;
    if (x > 0 && x < W - 1 && !((H & 1) && y == H - 1)) {
        const int yp = y > 0 ? y - 1 : 1, yn = y < H - 1 ? y + 1 : H - 2;
        const uint8_t* r0 = img + (size_t)yp * W;
        const uint8_t* r1 = img + (size_t)y * W;
        const uint8_t* r2 = img + (size_t)yn * W;
        const int s = ((int)r0[x + 1] - (int)r0[x - 1]) + 2 * ((int)r1[x + 1] - (int)r1[x - 1]) + ((int)r2[x + 1] - (int)r2[x - 1]);
        v = min(max(s, -cap), cap) + cap;
    }
    out[blockIdx.y * plane + i] = (uint8_t)v;
}

// Horizontal window sums of one row along a tile: the window of column xb + t slides one column per step.  BmRow keeps, per
// chunk of candidates, the lane's running sum and the wave-uniform texture sum |L' - cap|.
template <int NPL>
struct BmRow {
    const uint8_t* Lr;  // prefiltered rows
    const uint8_t* Rr;
    int s[NPL];
    int st;
    // window column c: left clamp(c, 0, W-1), right clamp(c - lofs, 0, W - D) + k (kd: the lane's candidates, clamped to D-1)
    __device__ __forceinline__ void col(int c, int sign, int W, int lofs, int rmax, int cap, const int (&kd)[NPL])
    {
        const int lv = __builtin_amdgcn_readfirstlane((int)Lr[min(max(c, 0), W - 1)]);
        const uint8_t* rp = Rr + min(max(c - lofs, 0), rmax);
#pragma unroll
        for (int k = 0; k < NPL; k++) s[k] += sign * abs(lv - (int)rp[kd[k]]);
        st += sign * abs(lv - cap);
    }
    // the window of column xb - 1: columns xb - h - 1 .. xb + h - 1
    __device__ __forceinline__ void start(const uint8_t* pfL, const uint8_t* pfR, int r, int xb, int h, int W, int lofs, int rmax,
                                          int cap, const int (&kd)[NPL])
    {
        Lr = pfL + (size_t)r * W;
        Rr = pfR + (size_t)r * W;
#pragma unroll
        for (int k = 0; k < NPL; k++) s[k] = 0;
        st = 0;
        for (int c = xb - h - 1; c < xb + h; c++) col(c, 1, W, lofs, rmax, cap, kd);
    }
    // slide to the window of column x
    __device__ __forceinline__ void step(int x, int h, int W, int lofs, int rmax, int cap, const int (&kd)[NPL])
    {
        col(x + h, 1, W, lofs, rmax, cap, kd);
        col(x - h - 1, -1, W, lofs, rmax, cap, kd);
    }
};

// sad[k] of a wave-uniform candidate k
template <int NPL>
__device__ __forceinline__ int bm_sad_at(const int (&sad)[NPL], int k)
{
    const int c = k >> 6;
    int v = sad[0];
#pragma unroll
    for (int i = 1; i < NPL; i++) v = c == i ? sad[i] : v;
    return __builtin_amdgcn_readlane(v, k & 63);
}

// One wavefront per tile of TX computed columns xb + t and a strip of valid rows [yb, ye).  The vertical running sums of the
// tile stay in LDS, [TX][NPL * 64] ints (candidate k = c * 64 + lane), and the texture sums in register `tex` of lane t.  A row
// step adds row y + h and drops row y - h in one pass over the tile, settling every pixel of row y in between.
template <int NPL>
__global__ __launch_bounds__(64) void k_bm_match(const uint8_t* __restrict__ pf, int H, int W, int minD, int D, int h, int cap,
                                                 int tex_thr, int U, int TX, int rows_per, short* __restrict__ raw,
                                                 int* __restrict__ cost, float* __restrict__ vol)
{
    extern __shared__ int acc[];  // [TX][NPL * 64]
    const int lane = threadIdx.x;
    const int lofs = minD + D - 1, rmax = W - D;
    const int xb = lofs + (int)blockIdx.x * TX;
    const int yb = h + (int)blockIdx.y * rows_per, ye = min(yb + rows_per, H - h);
    const int nt = min(TX, W - xb);
    const size_t plane = (size_t)H * W;
    const uint8_t* pfL = pf;
    const uint8_t* pfR = pf + plane;
    const int FILTERED = 16 * (minD - 1);
    int kk[NPL], kd[NPL];
#pragma unroll
    for (int c = 0; c < NPL; c++) {
        kk[c] = c * 64 + lane;
        kd[c] = min(kk[c], D - 1);
    }
    for (int i = lane; i < TX * NPL * 64; i += 64) acc[i] = 0;
    int tex = 0;
    // rows yb - h .. yb + h - 1
    for (int r = yb - h; r < yb + h; r++) {
        BmRow<NPL> a;
        a.start(pfL, pfR, r, xb, h, W, lofs, rmax, cap, kd);
        for (int t = 0; t < nt; t++) {
            a.step(xb + t, h, W, lofs, rmax, cap, kd);
#pragma unroll
            for (int c = 0; c < NPL; c++) acc[t * NPL * 64 + c * 64 + lane] += a.s[c];
            if (lane == t) tex += a.st;
        }
    }
    for (int y = yb; y < ye; y++) {
        BmRow<NPL> a, b;  // the row that enters (y + h) and the row that leaves after this step (y - h)
        a.start(pfL, pfR, y + h, xb, h, W, lofs, rmax, cap, kd);
        b.start(pfL, pfR, y - h, xb, h, W, lofs, rmax, cap, kd);
        for (int t = 0; t < nt; t++) {
            const int X = xb + t;
            a.step(X, h, W, lofs, rmax, cap, kd);
            b.step(X, h, W, lofs, rmax, cap, kd);
            int sad[NPL];
            int m = INT_MAX;
#pragma unroll
            for (int c = 0; c < NPL; c++) {
                sad[c] = acc[t * NPL * 64 + c * 64 + lane] + a.s[c];
                acc[t * NPL * 64 + c * 64 + lane] = sad[c] - b.s[c];
                if (kk[c] < D) m = min(m, sad[c]);
            }
            const int tsum = __builtin_amdgcn_readlane(tex, t) + a.st;
            if (lane == t) tex = tsum - b.st;
            m = wave_min(m);
            int mind = -1;  // the smallest k with the minimal SAD: chunk-major, then the lowest lane
#pragma unroll
            for (int c = 0; c < NPL; c++) {
                const unsigned long long bal = __ballot(kk[c] < D && sad[c] == m);
                if (mind < 0 && bal) mind = c * 64 + __ffsll((long long)bal) - 1;
            }
            const size_t o = (size_t)y * W + X;
            if (vol) {
#pragma unroll
                for (int c = 0; c < NPL; c++)
                    if (kk[c] < D) vol[(size_t)(D - 1 - kk[c]) * plane + o] = (float)sad[c];
            }
            int out = FILTERED;
            if (tsum >= tex_thr) {
                bool bad = false;
                if (U > 0) {
                    const long long thresh = m + (long long)m * U / 100;
                    bool any = false;
#pragma unroll
                    for (int c = 0; c < NPL; c++) any |= kk[c] < D && abs(kk[c] - mind) > 1 && sad[c] <= thresh;
                    bad = __ballot(any) != 0;
                }
                if (!bad) {
                    // sad[-1] = sad[1], sad[D] = sad[D-2]
                    const int p = bm_sad_at<NPL>(sad, mind + 1 < D ? mind + 1 : D - 2);
                    const int n = bm_sad_at<NPL>(sad, mind > 0 ? mind - 1 : 1);
                    const int d = p + n - 2 * m + abs(p - n);
                    out = ((D - mind - 1 + minD) * 256 + (d != 0 ? (p - n) * 256 / d : 0) + 15) >> 4;
                }
            }
            if (lane == 0) {
                raw[o] = (short)out;
                cost[o] = m;
            }
        }
    }
}

// step 6, first pass: per target column x2 = x - round(d), the pixel of least cost, the first x on a tie
__global__ __launch_bounds__(256) void k_bm_lrkey(const short* __restrict__ raw, const int* __restrict__ cost, int W, int y0, int y1,
                                                  int minX1, int FILTERED, unsigned long long* __restrict__ key)
{
    const int Wc = W - minX1;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)(y1 - y0) * Wc) return;
    const int y = y0 + (int)(i / Wc), x = minX1 + (int)(i % Wc);
    const size_t o = (size_t)y * W + x;
    const int d = raw[o];
    if (d == FILTERED) return;
    const int x2 = x - ((d + 8) >> 4);  // >= 0: d <= 16 * (minD + D - 1) + 8 and x >= minD + D
    atomicMin(&key[(size_t)y * W + x2], ((unsigned long long)(unsigned)cost[o] << 32) | (unsigned)x);
}

// step 6, second pass (M16 < 0: no check) and the valid region [y0, y1) x [x0, x1): FILTERED elsewhere
__global__ __launch_bounds__(256) void k_bm_finish(const short* __restrict__ raw, const unsigned long long* __restrict__ key, int H,
                                                   int W, int y0, int y1, int x0, int x1, int FILTERED, int M16,
                                                   short* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)H * W) return;
    const int y = (int)(i / W), x = (int)(i % W);
    if (y < y0 || y >= y1 || x < x0 || x >= x1) {
        out[i] = (short)FILTERED;
        return;
    }
    const int d = raw[i];
    int v = d;
    if (M16 >= 0 && d != FILTERED) {
        const size_t row = (size_t)y * W;
        auto disagrees = [&](int t) {
            const int xx = x - t;
            if (xx < 0 || xx >= W) return false;
            const unsigned long long kv = key[row + xx];
            if (kv == ~0ull) return false;  // no pixel filed here: disp2 is INVALID
            const int d2 = raw[row + (unsigned)(kv & 0xffffffffu)];
            return abs(d2 - d) > M16;
        };
        if (disagrees(d >> 4) && disagrees((d + 15) >> 4)) v = FILTERED;
    }
    out[i] = (short)v;
}

template <int NPL>
int launch_match(hipStream_t s, const BmLaunch& a, const uint8_t* pf, short* raw, int* cost)
{
    const int H = a.H, W = a.W, D = a.D, h = a.w / 2;
    const int lofs = a.minD + D - 1;
    const int Hv = H - 2 * h;
    // at most 16 KiB of running sums per wavefront; narrower tiles (each row of a tile first sums a whole window) and shorter
    // strips (each strip first sums 2h rows) until there are about 4096 wavefronts, 4 per SIMD
    int TX = std::min(64, 4096 / (NPL * 64));
    while (TX > 8 && (long long)((W - lofs + TX - 1) / TX) * ((Hv + 15) / 16) < 4096) TX /= 2;
    const int tiles = (W - lofs + TX - 1) / TX;
    const int strips_wanted = std::max(1, 4096 / tiles);
    const int rows_per = std::max((Hv + strips_wanted - 1) / strips_wanted, 8);
    const int strips = (Hv + rows_per - 1) / rows_per;
    return ASW_LAUNCH(k_bm_match<NPL>, dim3(tiles, strips), dim3(64), (size_t)TX * NPL * 64 * sizeof(int), s, pf, H, W, a.minD, D, h,
                      a.cap, a.texture, a.U, TX, rows_per, raw, cost, a.vol);
}

}  // namespace

size_t bm_scratch_bytes(int H, int W)
{
    const size_t plane = (size_t)H * W;
    // prefiltered pair | keys | speckle scratch | costs | raw disparities (every region 8-byte aligned)
    return plane * 2 + 7 + plane * 8 + plane * 8 + plane * 4 + plane * 2;
}

int launch_bm(hipStream_t s, const BmLaunch& a)
{
    const int H = a.H, W = a.W, D = a.D, minD = a.minD, h = a.w / 2;
    const size_t plane = (size_t)H * W;
    const int FILTERED = 16 * (minD - 1);
    const int lofs = minD + D - 1;
    const int y0 = h, y1 = H - h, x0 = lofs + h, x1 = W - h;
    if (a.vol) ASW_HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)a.vol, 0x7fc00000, plane * D, s));  // NaN where nothing is computed
    if (y1 <= y0 || x1 <= x0) {  // empty valid region: the whole map is FILTERED (this library's definition)
        ASW_TRY(launch_fill_s16(s, a.disp16, plane, (short)FILTERED));
        ASW_TRY(a.agg.begin());
        ASW_TRY(a.agg.end());
        return ASW_OK;
    }
    // carve the scratch in bm_scratch_bytes' order
    char* p = (char*)a.scratch;
    uint8_t* pf = (uint8_t*)p; p += (plane * 2 + 7) / 8 * 8;
    unsigned long long* key = (unsigned long long*)p; p += plane * 8;
    int* spk = (int*)p; p += plane * 8;
    int* cost = (int*)p; p += plane * 4;
    short* raw = (short*)p;
    ASW_TRY(ASW_LAUNCH(k_bm_prefilter, dim3(blocks(plane, 256), 2), dim3(256), 0, s, a.L, a.R, H, W, a.cap, pf));
    ASW_TRY(a.agg.begin());
    ASW_TRY(dispatch_npl(D, [&](auto npl) { return launch_match<decltype(npl)::value>(s, a, pf, raw, cost); }));
    ASW_TRY(a.agg.end());
    const int minX1 = minD + D;
    if (a.M >= 0 && minX1 < W) {
        ASW_HIP_TRY(hipMemsetAsync(key, 0xff, plane * 8, s));
        ASW_TRY(ASW_LAUNCH(k_bm_lrkey, dim3(blocks((size_t)(y1 - y0) * (W - minX1), 256)), dim3(256), 0, s, raw, cost, W, y0, y1,
                           minX1, FILTERED, key));
    }
    const int M16 = a.M < 0 ? -1 : (int)std::min<long long>(16LL * a.M, INT_MAX / 2);
    ASW_TRY(ASW_LAUNCH(k_bm_finish, dim3(blocks(plane, 256)), dim3(256), 0, s, raw, key, H, W, y0, y1, x0, x1, FILTERED, M16,
                       a.disp16));
    if (a.speckle_range >= 0 && a.speckle_window > 0)
        ASW_TRY(launch_filter_speckles(s, a.disp16, H, W, FILTERED, a.speckle_window, a.speckle_range, spk));
    return ASW_OK;
}
