// Semi-global block matching, StereoSGBM MODE_SGBM_3WAY as DESIGN.md section 4.8 states it (OpenCV 4.1.0 stereosgbm.cpp), and
// cv::filterSpeckles; asw_sgbm_paths adds further path directions to the three (section 4.8b).  Integer arithmetic throughout;
// every intermediate is exact in 32 bits (the host refuses parameters for which n * (C_max + P2) >= 2^31, n paths, n >= 3).
//
// Layout: the volumes C (block cost), T (L_tb, then + the extra paths, + L_lr, then S) are int32 [H][Wv][D] with d innermost, over the valid
// columns x = x0 + xi, x0 = minX1 = minD + D, Wv = W - x0.  Candidate index d <-> absolute disparity minD + d.
//
//   k_sgbm_prefilter  step 1 + the Birchfield-Tomasi interval: {value, min, max} planes of every prefiltered plane
//   k_sgbm_hcost      steps 2 + horizontal half of 3: one thread per (y, d) walks the row with a running window sum
//   k_sgbm_hcost_census  asw_sgbm_census only (section 4.8c): the same hb from the Hamming distance of two census codes
//   k_sgbm_top        vertical half of 3 + the top->bottom path: one wavefront per column, candidates in lanes
//   k_sgbm_line       asw_sgbm_paths only: bottom->top and the four diagonal paths, one wavefront per column / (anti-)diagonal
//   k_sgbm_row        left->right and right->left paths, winner, uniqueness, subpixel, disp2 keys: one wavefront per row
//   k_sgbm_lr         the left-right rule of step 6 -> int16 map
//   k_median3_s16     step 7;  k_spk_*: step 8 (union-find over the whole frame);  k_disp16_to_u8<float>: step 9
#include "asw_internal.h"
#include "asw_device.h"
#include "asw_host.h"

namespace {

constexpr int SGBM_BIG = 0x3fffffff;  // "no predecessor": above every L (<= C_max + P2 < 2^31 / 3), and BIG + P1 < 2^31

// {value, min, max} of one prefiltered plane at x of row y; columns 0 and W-1 hold ftzero (OpenCV's border quirk)
__device__ __forceinline__ int sgbm_pre(const uint8_t* __restrict__ img, int H, int W, int cn, int k, int y, int x, int ftzero)
{
    if (x <= 0 || x >= W - 1) return ftzero;
    if (k >= cn) return img[((size_t)y * W + x) * cn + (k - cn)];
    const int yn = max(y - 1, 0), ys = min(y + 1, H - 1);
    const uint8_t* r0 = img + (size_t)y * W * cn + k;
    const uint8_t* rn = img + (size_t)yn * W * cn + k;
    const uint8_t* rs = img + (size_t)ys * W * cn + k;
    const int s = 2 * ((int)r0[(x + 1) * cn] - (int)r0[(x - 1) * cn]) + (int)rn[(x + 1) * cn] - (int)rn[(x - 1) * cn] +
                  (int)rs[(x + 1) * cn] - (int)rs[(x - 1) * cn];
    return min(max(s, -ftzero), ftzero) + ftzero;
}

// out: int3-like planes [img 0|1][k][H][W] of {v, vmin, vmax}
__global__ __launch_bounds__(256) void k_sgbm_prefilter(const uint8_t* __restrict__ L, const uint8_t* __restrict__ R, int H, int W,
                                                        int cn, int ftzero, int4* __restrict__ out)
{
    const size_t plane = (size_t)H * W;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= plane) return;
    const int y = (int)(i / W), x = (int)(i % W);
    for (int img = 0; img < 2; img++) {
        const uint8_t* src = img ? R : L;
        for (int k = 0; k < 2 * cn; k++) {
            const int a = sgbm_pre(src, H, W, cn, k, y, x, ftzero);
            const int l = x > 0 ? sgbm_pre(src, H, W, cn, k, y, x - 1, ftzero) : a;
            const int r = x < W - 1 ? sgbm_pre(src, H, W, cn, k, y, x + 1, ftzero) : a;
            const int hl = (a + l) >> 1, hr = (a + r) >> 1;
            out[((size_t)img * 2 * cn + k) * plane + i] = make_int4(a, min(a, min(hl, hr)), max(a, max(hl, hr)), 0);
        }
    }
}

// pixel cost of left column x against right column x - off (step 2)
__device__ __forceinline__ int sgbm_pix(const int4* __restrict__ pf, size_t plane, int cn, size_t rowL, size_t rowR)
{
    int tot = 0;
    for (int k = 0; k < 2 * cn; k++) {
        const int4 u = pf[(size_t)k * plane + rowL];
        const int4 v = pf[((size_t)2 * cn + k) * plane + rowR];
        const int c = min(max(max(0, u.x - v.z), v.y - u.x), max(max(0, v.x - u.z), u.y - v.x));
        tot += k < cn ? c : (c >> 2);
    }
    return tot;
}

// horizontal window sums of the pixel cost, clamped to the valid columns: hb[y][xi][d]
__global__ __launch_bounds__(256) void k_sgbm_hcost(const int4* __restrict__ pf, int H, int W, int cn, int minD, int D, int h,
                                                    int* __restrict__ hb)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)H * D) return;
    const int d = (int)(t % D), y = (int)(t / D);
    const int x0 = minD + D, Wv = W - x0, off = minD + d;
    const size_t plane = (size_t)H * W, row = (size_t)y * W;
    auto pix = [&](int xi) {
        xi = min(max(xi, 0), Wv - 1);
        const int x = x0 + xi;
        return sgbm_pix(pf, plane, cn, row + x, row + (x - off));
    };
    int sum = 0;
    for (int i = -h; i <= h; i++) sum += pix(i);
    int* out = hb + (size_t)y * Wv * D + d;
    for (int xi = 0; xi < Wv; xi++) {
        out[(size_t)xi * D] = sum;
        sum += pix(xi + h + 1) - pix(xi - h);
    }
}

// asw_sgbm_census: hb of the census cost, pix(y, xi, d) = popcount(codeL[y][x0 + xi] ^ codeR[y][x0 + xi -
// (minD + d)]) in place of steps 1-2, the same clamped window sum.  One workgroup: one row, both code rows staged in LDS (16 W
// bytes), and 256 / nd segments of seglen valid columns, nd = min(D, 256) candidates side by side; blockIdx.y continues the
// segments.  A thread owns (segment, d; d + 256 j when D > 256), seeds its window with 2 h + 1 terms and walks its segment with the
// running sum: the left code of a step is one address for all candidates of a segment (a broadcast read), the right codes are
// consecutive words, the stores consecutive in d.
__global__ __launch_bounds__(256) void k_sgbm_hcost_census(const unsigned long long* __restrict__ codeL,
                                                           const unsigned long long* __restrict__ codeR, int W, int minD, int D, int h,
                                                           int seglen, int* __restrict__ hb)
{
    extern __shared__ __align__(16) unsigned long long sgbm_code_rows[];  // [2][W]
    unsigned long long* cl = sgbm_code_rows;
    unsigned long long* cr = cl + W;
    const int y = blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i < W; i += 256) {
        cl[i] = codeL[(size_t)y * W + i];
        cr[i] = codeR[(size_t)y * W + i];
    }
    __syncthreads();
    const int x0 = minD + D, Wv = W - x0;
    const int nd = min(D, 256), spb = 256 / nd;
    const int sl = tid / nd;
    if (sl >= spb) return;
    const int xb = (blockIdx.y * spb + sl) * seglen, xe = min(Wv, xb + seglen);
    if (xb >= xe) return;
    const unsigned long long* l = cl + x0;  // l[xi]: the left code of valid column xi
    for (int d = tid - sl * nd; d < D; d += nd) {
        const unsigned long long* r = cr + (D - d);  // r[xi]: its partner, column x0 + xi - (minD + d) >= 1
        auto ham = [&](int xi) {
            xi = min(max(xi, 0), Wv - 1);
            return __popcll(l[xi] ^ r[xi]);
        };
        int sum = 0;
        for (int i = -h; i <= h; i++) sum += ham(xb + i);
        int* out = hb + ((size_t)y * Wv + xb) * D + d;
        for (int xi = xb; xi < xe; xi++, out += D) {
            *out = sum;
            sum += ham(xi + h + 1) - ham(xi - h);
        }
    }
}

// One path step over the candidates of a wavefront (d = k * 64 + lane): Lr holds L(p - r, d) on entry and L(p, d) on exit, m the
// minimum over d of the predecessor on entry and of the new L on exit.  nb: the LDS row of this step (2 x D ints, parity `par`).
template <int NPL>
__device__ __forceinline__ void sgbm_step(int (&Lr)[NPL], const int (&c)[NPL], int& m, int* nb, int D, int P1, int P2)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < NPL; k++) {
        const int d = k * 64 + lane;
        if (d < D) nb[d] = Lr[k];
    }
    __syncthreads();
    int mn = SGBM_BIG;
#pragma unroll
    for (int k = 0; k < NPL; k++) {
        const int d = k * 64 + lane;
        if (d < D) {
            int best = min(Lr[k], m + P2);
            if (d > 0) best = min(best, nb[d - 1] + P1);
            if (d < D - 1) best = min(best, nb[d + 1] + P1);
            Lr[k] = c[k] + best - m;
            mn = min(mn, Lr[k]);
        }
    }
    m = wave_min(mn);
}

// vertical window sums of hb (C, written out for the row paths) and the top->bottom path (L_tb): one wavefront per column
template <int NPL>
__global__ __launch_bounds__(64) void k_sgbm_top(const int* __restrict__ hb, int H, int Wv, int D, int h, int P1, int P2,
                                                 int* __restrict__ C, int* __restrict__ T)
{
    extern __shared__ int lds[];  // [2][D]
    const int xi = blockIdx.x, lane = threadIdx.x;
    const size_t rs = (size_t)Wv * D;  // row stride of the volumes
    const size_t base = (size_t)xi * D;
    int vs[NPL], Lr[NPL];
#pragma unroll
    for (int k = 0; k < NPL; k++) {
        const int d = k * 64 + lane;
        vs[k] = 0;
        Lr[k] = 0;
        if (d < D)
            for (int j = -h; j <= h; j++) vs[k] += hb[(size_t)min(max(j, 0), H - 1) * rs + base + d];
    }
    int m = 0;
    for (int y = 0; y < H; y++) {
        sgbm_step<NPL>(Lr, vs, m, lds + (y & 1) * D, D, P1, P2);
        const int ya = min(y + h + 1, H - 1), yr = max(y - h, 0);
#pragma unroll
        for (int k = 0; k < NPL; k++) {
            const int d = k * 64 + lane;
            if (d < D) {
                const size_t o = (size_t)y * rs + base + d;
                C[o] = vs[k];
                T[o] = Lr[k];
                vs[k] += hb[(size_t)ya * rs + base + d] - hb[(size_t)yr * rs + base + d];
            }
        }
    }
}

// left->right then right->left along one row; the second pass completes S, picks the winner (smallest d on a tie), applies the
// uniqueness rule and the subpixel fit, and files (minS, x) under the matching right-image column x2 for the left-right rule.
// disp_raw[y][x] (x >= x0): the scaled disparity or INVALID; key[y][x2]: min over the pixels that chose x2 of (minS << 32 | x).
template <int NPL>
__global__ __launch_bounds__(64) void k_sgbm_row(const int* __restrict__ C, int* __restrict__ T, int H, int W, int minD, int D,
                                                 int P1, int P2, int U, int keep_S, int* __restrict__ disp_raw,
                                                 unsigned long long* __restrict__ key)
{
    extern __shared__ int lds[];  // [2][D] path neighbours, [2][D] S row
    const int y = blockIdx.x, lane = threadIdx.x;
    const int x0 = minD + D, Wv = W - x0;
    const int INVALID = 16 * (minD - 1);
    const size_t rowbase = (size_t)y * Wv * D;
    int Lr[NPL], c[NPL];
    int m = 0;
#pragma unroll
    for (int k = 0; k < NPL; k++) Lr[k] = 0;
    for (int xi = 0; xi < Wv; xi++) {
        const size_t o = rowbase + (size_t)xi * D;
#pragma unroll
        for (int k = 0; k < NPL; k++) {
            const int d = k * 64 + lane;
            c[k] = d < D ? C[o + d] : 0;
        }
        sgbm_step<NPL>(Lr, c, m, lds + (xi & 1) * D, D, P1, P2);
#pragma unroll
        for (int k = 0; k < NPL; k++) {
            const int d = k * 64 + lane;
            if (d < D) T[o + d] += Lr[k];
        }
    }
    m = 0;
#pragma unroll
    for (int k = 0; k < NPL; k++) Lr[k] = 0;
    int* srow = lds + 2 * D;
    for (int xi = Wv - 1; xi >= 0; xi--) {
        const size_t o = rowbase + (size_t)xi * D;
#pragma unroll
        for (int k = 0; k < NPL; k++) {
            const int d = k * 64 + lane;
            c[k] = d < D ? C[o + d] : 0;
        }
        const int par = xi & 1;
        sgbm_step<NPL>(Lr, c, m, lds + par * D, D, P1, P2);
        int s[NPL];
        int mn = 0x7fffffff, bd = 0x7fffffff;
#pragma unroll
        for (int k = 0; k < NPL; k++) {
            const int d = k * 64 + lane;
            s[k] = 0x7fffffff;
            if (d < D) {
                s[k] = T[o + d] + Lr[k];
                if (keep_S) T[o + d] = s[k];  // only the volume reads S back
                srow[par * D + d] = s[k];
                if (s[k] < mn) { mn = s[k]; bd = d; }
            }
        }
        // (minS, smallest d) over the wavefront
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int om = __shfl_xor(mn, off), od = __shfl_xor(bd, off);
            if (om < mn || (om == mn && od < bd)) { mn = om; bd = od; }
        }
        bool bad = false;
#pragma unroll
        for (int k = 0; k < NPL; k++) {
            const int d = k * 64 + lane;
            if (d < D && abs(d - bd) > 1 && (long long)s[k] * (100 - U) < (long long)mn * 100) bad = true;
        }
        bad = __ballot(bad) != 0;
        __syncthreads();  // srow of this step is complete (the next write to it is two steps away, behind sgbm_step's barrier)
        if (lane == 0) {
            const int x = x0 + xi;
            int v = INVALID;
            if (!bad) {
                v = 16 * bd;
                if (bd > 0 && bd < D - 1) {
                    const long long sm = srow[par * D + bd - 1], sp = srow[par * D + bd + 1];
                    const long long den = max(sm + sp - 2ll * mn, 1ll);
                    v += (int)((16 * (sm - sp) + den) / (2 * den));  // C division: truncation toward zero
                }
                v += 16 * minD;
                const int x2 = x - (bd + minD);  // >= 1: x >= minD + D > bd + minD
                atomicMin(&key[(size_t)y * W + x2], ((unsigned long long)(unsigned)mn << 32) | (unsigned)x);
            }
            disp_raw[(size_t)y * W + x] = v;
        }
    }
}

// The extra path directions of asw_sgbm_paths: one wavefront per line of the H x Wv rectangle, candidates
// in lanes, L added into T as it is produced.  Runs between k_sgbm_top (which leaves T = L_tb) and k_sgbm_row.
//   geom 0: the column xi = line, walked top->bottom
//   geom 1: the diagonal xi - y = line - (H - 1), walked from its top-left end
//   geom 2: the anti-diagonal xi + y = line, walked from its top-right end
// dirs bit 0: walk forth (geom 0..2: PATH_TB, TLBR, TRBL); bit 1: walk back over the same line (PATH_BT, BRTL, BLTR).  The lines
// of one geometry are disjoint and both walks of a line belong to the same wavefront (lane d touches the same addresses in
// both), so nothing in a launch shares a T entry between wavefronts.
// The C row of the next step does not depend on the recurrence: it, and the T row of this step, are loaded before sgbm_step so
// that the dependent chain never waits on global memory (measured: DESIGN.md section 4.8b).
template <int NPL>
__device__ __forceinline__ void sgbm_line_walk(const int* __restrict__ C, int* T, ptrdiff_t first, ptrdiff_t stride, int len, int D,
                                               int P1, int P2, int* lds)
{
    const int lane = threadIdx.x;
    int Lr[NPL], c[NPL], cn[NPL], t[NPL];
    int m = 0;
#pragma unroll
    for (int k = 0; k < NPL; k++) {
        const int d = k * 64 + lane;
        Lr[k] = 0;
        cn[k] = d < D ? C[first + d] : 0;
    }
    ptrdiff_t o = first;
    for (int i = 0; i < len; i++, o += stride) {
#pragma unroll
        for (int k = 0; k < NPL; k++) c[k] = cn[k];
        const bool more = i + 1 < len;
#pragma unroll
        for (int k = 0; k < NPL; k++) {
            const int d = k * 64 + lane;
            if (d < D) {
                t[k] = T[o + d];
                if (more) cn[k] = C[o + stride + d];
            }
        }
        sgbm_step<NPL>(Lr, c, m, lds + (i & 1) * D, D, P1, P2);
#pragma unroll
        for (int k = 0; k < NPL; k++) {
            const int d = k * 64 + lane;
            if (d < D) T[o + d] = t[k] + Lr[k];
        }
    }
}

template <int NPL>
__global__ __launch_bounds__(64) void k_sgbm_line(const int* __restrict__ C, int* T, int H, int Wv, int D, int P1, int P2, int geom,
                                                  int dirs)
{
    extern __shared__ int lds[];  // [2][D]
    const int line = blockIdx.x;
    int y0, x0, len, sx;
    if (geom == 0) {
        y0 = 0; x0 = line; len = H; sx = 0;
    } else if (geom == 1) {
        y0 = max(0, H - 1 - line); x0 = max(0, line - (H - 1)); len = min(H - y0, Wv - x0); sx = 1;
    } else {
        y0 = max(0, line - (Wv - 1)); x0 = line - y0; len = min(H - y0, x0 + 1); sx = -1;
    }
    const ptrdiff_t stride = ((ptrdiff_t)Wv + sx) * D;  // one row down, sx columns across
    const ptrdiff_t first = ((ptrdiff_t)y0 * Wv + x0) * D;
    if (dirs & 1) sgbm_line_walk<NPL>(C, T, first, stride, len, D, P1, P2, lds);
    if (dirs & 2) {
        __syncthreads();  // the forth walk's last LDS row may share its parity with the back walk's first
        sgbm_line_walk<NPL>(C, T, first + (len - 1) * stride, -stride, len, D, P1, P2, lds);
    }
}

// step 6: a pixel is invalidated only when both of its neighbouring integer disparities disagree with the right-view winners
__global__ __launch_bounds__(256) void k_sgbm_lr(const int* __restrict__ disp_raw, const unsigned long long* __restrict__ key, int H,
                                                 int W, int minD, int D, int M, short* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)H * W) return;
    const int x = (int)(i % W);
    const size_t row = i - x;
    const int INVALID = 16 * (minD - 1);
    if (x < minD + D) {
        out[i] = (short)INVALID;
        return;
    }
    const int d1 = disp_raw[i];
    if (d1 == INVALID) {
        out[i] = (short)INVALID;
        return;
    }
    auto disagrees = [&](int t) {
        const int xx = x - t;
        if (xx < 0 || xx >= W) return false;
        const unsigned long long kv = key[row + xx];
        const int d2 = kv == ~0ull ? minD - 1 : (int)(unsigned)(kv & 0xffffffffu) - xx;
        return d2 >= minD && abs(d2 - t) > M;
    };
    const int lo = d1 >> 4, hi = (d1 + 15) >> 4;
    out[i] = (short)(disagrees(lo) && disagrees(hi) ? INVALID : d1);
}

__global__ __launch_bounds__(256) void k_fill_s16(short* __restrict__ out, size_t n, short v)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = v;
}

// S volume [D][H][W] f32, 0 outside the valid columns (exact: the host checks the bound against 2^24)
__global__ __launch_bounds__(256) void k_sgbm_volume(const int* __restrict__ S, int H, int W, int minD, int D, float* __restrict__ vol)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t plane = (size_t)H * W;
    if (i >= plane * D) return;
    const int d = (int)(i / plane);
    const size_t p = i % plane;
    const int x = (int)(p % W), y = (int)(p / W);
    const int x0 = minD + D, Wv = W - x0;
    vol[i] = x < x0 ? 0.0f : (float)S[((size_t)y * Wv + (x - x0)) * D + d];
}

// medianBlur(3) of an int16 map, replicated borders
__global__ __launch_bounds__(256) void k_median3_s16(const short* __restrict__ in, int H, int W, short* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)H * W) return;
    const int x = (int)(i % W), y = (int)(i / W);
    int v[9];
    int n = 0;
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++)
            v[n++] = in[(size_t)min(max(y + dy, 0), H - 1) * W + min(max(x + dx, 0), W - 1)];
#pragma unroll
    for (int a = 0; a < 5; a++)  // partial selection sort: v[4] ends as the 5th smallest
#pragma unroll
        for (int b = a + 1; b < 9; b++) {
            const int lo = min(v[a], v[b]), hi = max(v[a], v[b]);
            v[a] = lo;
            v[b] = hi;
        }
    out[i] = (short)v[4];
}

// ---- filterSpeckles: union-find over the whole frame.  parent[i] <= i always (a root is linked under the smaller root), so every
// value a parent ever holds is a member of the same set; path halving during the union phase is therefore benign under races.
__device__ __forceinline__ int spk_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void spk_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ int spk_find_halving(int* parent, int x)
{
    while (true) {
        const int p = spk_load(parent + x);
        if (p == x) return x;
        const int gp = spk_load(parent + p);
        if (gp != p) spk_store(parent + x, gp);
        x = gp;
    }
}

__global__ __launch_bounds__(256) void k_spk_init(const short* __restrict__ img, size_t n, int new_val, int* __restrict__ parent,
                                                  int* __restrict__ size)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    parent[i] = img[i] == new_val ? -1 : (int)i;
    size[i] = 0;
}

__device__ void spk_union(int* parent, int a, int b)
{
    while (true) {
        a = spk_find_halving(parent, a);
        b = spk_find_halving(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        if (atomicCAS(parent + a, a, b) == a) return;
    }
}

__global__ __launch_bounds__(256) void k_spk_union(const short* __restrict__ img, int H, int W, int new_val, int max_diff,
                                                   int* __restrict__ parent)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)H * W) return;
    const int v = img[i];
    if (v == new_val) return;
    const int x = (int)(i % W), y = (int)(i / W);
    if (x + 1 < W) {
        const int u = img[i + 1];
        if (u != new_val && abs(u - v) <= max_diff) spk_union(parent, (int)i, (int)i + 1);
    }
    if (y + 1 < H) {
        const int u = img[i + W];
        if (u != new_val && abs(u - v) <= max_diff) spk_union(parent, (int)i, (int)(i + W));
    }
}

// one round of pointer jumping, parent[i] = parent[parent[i]]: every value a parent takes is an ancestor, so concurrent rounds only
// shorten the chains faster; ceil(log2(n)) rounds leave every pixel one link below its root whatever chains the union phase left
// (a 1-pixel path of a component that snakes through the frame can be hundreds of thousands of links deep before)
__global__ __launch_bounds__(256) void k_spk_jump(size_t n, int* __restrict__ parent)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int p = spk_load(parent + i);
    if (p < 0) return;
    const int gp = spk_load(parent + p);
    if (gp != p) spk_store(parent + i, gp);
}

// root of every pixel (read-only walk: a concurrent flattening store only ever replaces a parent by its root) + component sizes.
// One atomicAdd per run of equal roots within a wavefront's 64 consecutive pixels, not per pixel: a large component would
// otherwise serialise a million atomics on its root's counter (19.7 ms at 1080p measured in the per-pixel form).
__global__ __launch_bounds__(256) void k_spk_flatten(size_t n, int* __restrict__ parent, int* __restrict__ size)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int x = i < n ? spk_load(parent + i) : -1;
    if (x >= 0) {
        while (true) {
            const int p = spk_load(parent + x);
            if (p == x) break;
            x = p;
        }
        spk_store(parent + i, x);
    }
    const int prev = __shfl_up(x, 1);
    const bool head = x >= 0 && (lane == 0 || prev != x);
    const unsigned long long ends = __ballot(lane == 0 || prev != x);  // every lane that starts a run (valid or not)
    if (head) {
        const unsigned long long above = lane == 63 ? 0ull : ends & (~0ull << (lane + 1));
        const int next = above ? __ffsll((long long)above) - 1 : 64;
        atomicAdd(size + x, next - lane);
    }
}

__global__ __launch_bounds__(256) void k_spk_apply(short* __restrict__ img, size_t n, int new_val, int max_size,
                                                   const int* __restrict__ parent, const int* __restrict__ size)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int r = parent[i];
    if (r >= 0 && size[r] <= max_size) img[i] = (short)new_val;
}

// convertTo(CV_8U, 1/16): round half to even, saturate -- T = float for the selector's CV_32F result, uint8_t for getDisparity_BM
template <typename T>
__global__ __launch_bounds__(256) void k_disp16_to_u8(const short* __restrict__ in, size_t n, T* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = (T)fminf(fmaxf(rintf((float)in[i] * 0.0625f), 0.0f), 255.0f);
}

// the path kernels of one frame; hb, C, T, disp_raw, key: regions of a.scratch as launch_sgbm carves them
template <int NPL>
int launch_paths(hipStream_t s, const SgbmLaunch& a, const int* hb, int* C, int* T, int* disp_raw, unsigned long long* key)
{
    const int H = a.H, W = a.W, minD = a.minD, D = a.D, h = a.w / 2, P1 = a.P1, P2 = a.P2, paths = a.paths;
    const int Wv = W - (minD + D);
    ASW_TRY(ASW_LAUNCH(k_sgbm_top<NPL>, dim3(Wv), dim3(64), 2 * D * sizeof(int), s, hb, H, Wv, D, h, P1, P2, C, T));
    // the directions beyond the three of k_sgbm_top / k_sgbm_row: one launch per line geometry, stream order between them
    const int dirs[3] = {paths & ASW_SGBM_PATH_BT ? 2 : 0,
                         (paths & ASW_SGBM_PATH_TLBR ? 1 : 0) | (paths & ASW_SGBM_PATH_BRTL ? 2 : 0),
                         (paths & ASW_SGBM_PATH_TRBL ? 1 : 0) | (paths & ASW_SGBM_PATH_BLTR ? 2 : 0)};
    for (int geom = 0; geom < 3; geom++) {
        if (!dirs[geom]) continue;
        ASW_TRY(ASW_LAUNCH(k_sgbm_line<NPL>, dim3(geom == 0 ? Wv : H + Wv - 1), dim3(64), 2 * D * sizeof(int), s, C, T, H, Wv, D, P1,
                           P2, geom, dirs[geom]));
    }
    return ASW_LAUNCH(k_sgbm_row<NPL>, dim3(H), dim3(64), 4 * D * sizeof(int), s, C, T, H, W, minD, D, P1, P2, a.U, a.vol != nullptr,
                      disp_raw, key);
}

// the census cost stage of asw_sgbm_census: a.L / a.R are the gray planes; codes: room for two code planes (8 bytes a pixel each)
int launch_hcost_census(hipStream_t s, const SgbmLaunch& a, unsigned long long* codes, int* hb)
{
    const int H = a.H, W = a.W, D = a.D, h = a.w / 2;
    const int Wv = W - (a.minD + D);
    const size_t plane = (size_t)H * W;
    unsigned long long* codeL = codes;
    unsigned long long* codeR = codes + plane;
    ASW_TRY(launch_census_transform(s, a.L, H, W, reinterpret_cast<uint2*>(codeL)));
    ASW_TRY(launch_census_transform(s, a.R, H, W, reinterpret_cast<uint2*>(codeR)));
    const size_t lds = (size_t)W * 16;
    // A row alone gives D threads work: few rows or few candidates leave the chip idle, so the valid columns are cut into
    // segments until there are about 2048 workgroups.  A segment pays 2 h + 1 terms for its seed: none is shorter than twice that.
    const int spb = 256 / std::min(D, 256);
    const int want = spb * ((2048 + H - 1) / H);
    const int nseg = std::max(1, std::min(want, Wv / std::max(32, 2 * (2 * h + 1))));
    const int seglen = (Wv + nseg - 1) / nseg;
    const unsigned gy = (unsigned)((Wv + seglen * spb - 1) / (seglen * spb));
    return ASW_LAUNCH(k_sgbm_hcost_census, dim3(H, gy), dim3(256), lds, s, codeL, codeR, W, a.minD, D, h, seglen, hb);
}

}  // namespace

size_t sgbm_scratch_bytes(int H, int W, int cn, int minD, int D)
{
    const size_t Wv = W > minD + D ? (size_t)(W - minD - D) : 0;
    const size_t plane = (size_t)H * W;
    // hb, C, T volumes | prefiltered planes (asw_sgbm_census: the two code planes, plane * 16 bytes) | disp2 keys | speckle scratch | raw disparities | left-right checked map
    return 3 * ((size_t)H * Wv * D * 4) + plane * 64 * cn + plane * 8 + plane * 8 + plane * 4 + (plane * 2 + 15) / 16 * 16;
}

int launch_sgbm(hipStream_t s, const SgbmLaunch& a)
{
    const int H = a.H, W = a.W, D = a.D, minD = a.minD;
    const size_t plane = (size_t)H * W;
    const int INVALID = 16 * (minD - 1);
    if (W <= minD + D) {  // no valid column: every pixel INVALID, nothing to filter
        ASW_TRY(launch_fill_s16(s, a.disp16, plane, (short)INVALID));
        if (a.vol) ASW_HIP_TRY(hipMemsetAsync(a.vol, 0, plane * D * sizeof(float), s));
        ASW_TRY(a.agg.begin());
        ASW_TRY(a.agg.end());
        return ASW_OK;
    }
    const int Wv = W - (minD + D);
    const size_t vol = (size_t)H * Wv * D;
    // carve the scratch in sgbm_scratch_bytes' order (every region starts 8-byte aligned)
    char* p = (char*)a.scratch;
    int* hb = (int*)p; p += vol * 4;
    int* C = (int*)p; p += vol * 4;
    int* T = (int*)p; p += vol * 4;
    int4* pf = (int4*)p; p += plane * 64 * a.cn;
    unsigned long long* key = (unsigned long long*)p; p += plane * 8;
    int* spk = (int*)p; p += plane * 8;
    int* disp_raw = (int*)p; p += plane * 4;
    short* lr = (short*)p;
    if (a.census) {
        ASW_TRY(launch_hcost_census(s, a, (unsigned long long*)pf, hb));
    } else {
        ASW_TRY(ASW_LAUNCH(k_sgbm_prefilter, dim3(blocks(plane, 256)), dim3(256), 0, s, a.L, a.R, H, W, a.cn, a.ftzero, pf));
        ASW_TRY(ASW_LAUNCH(k_sgbm_hcost, dim3(blocks((size_t)H * D, 256)), dim3(256), 0, s, pf, H, W, a.cn, minD, D, a.w / 2, hb));
    }
    ASW_HIP_TRY(hipMemsetAsync(key, 0xff, plane * 8, s));
    ASW_TRY(a.agg.begin());
    ASW_TRY(dispatch_npl(D, [&](auto npl) { return launch_paths<decltype(npl)::value>(s, a, hb, C, T, disp_raw, key); }));
    ASW_TRY(a.agg.end());
    if (a.vol) {
        ASW_TRY(ASW_LAUNCH(k_sgbm_volume, dim3(blocks(plane * D, 256)), dim3(256), 0, s, T, H, W, minD, D, a.vol));
    }
    ASW_TRY(ASW_LAUNCH(k_sgbm_lr, dim3(blocks(plane, 256)), dim3(256), 0, s, disp_raw, key, H, W, minD, D, a.M, lr));
    ASW_TRY(ASW_LAUNCH(k_median3_s16, dim3(blocks(plane, 256)), dim3(256), 0, s, lr, H, W, a.disp16));
    if (a.speckle_window > 0)
        ASW_TRY(launch_filter_speckles(s, a.disp16, H, W, INVALID, a.speckle_window, 16 * a.speckle_range, spk));
    return ASW_OK;
}

int launch_filter_speckles(hipStream_t s, short* img, int H, int W, int new_val, int max_size, int max_diff, int* scratch)
{
    const size_t n = (size_t)H * W;
    int* parent = scratch;
    int* size = scratch + n;
    ASW_TRY(ASW_LAUNCH(k_spk_init, dim3(blocks(n, 256)), dim3(256), 0, s, img, n, new_val, parent, size));
    ASW_TRY(ASW_LAUNCH(k_spk_union, dim3(blocks(n, 256)), dim3(256), 0, s, img, H, W, new_val, max_diff, parent));
    for (size_t span = 1; span < n; span *= 2) {
        ASW_TRY(ASW_LAUNCH(k_spk_jump, dim3(blocks(n, 256)), dim3(256), 0, s, n, parent));
    }
    ASW_TRY(ASW_LAUNCH(k_spk_flatten, dim3(blocks(n, 256)), dim3(256), 0, s, n, parent, size));
    return ASW_LAUNCH(k_spk_apply, dim3(blocks(n, 256)), dim3(256), 0, s, img, n, new_val, max_size, parent, size);
}

int launch_fill_s16(hipStream_t s, short* out, size_t n, short v)
{
    return ASW_LAUNCH(k_fill_s16, dim3(blocks(n, 256)), dim3(256), 0, s, out, n, v);
}

template <typename T>
static int launch_disp16_convert(hipStream_t s, const short* disp16, size_t n, T* out)
{
    return ASW_LAUNCH(k_disp16_to_u8<T>, dim3(blocks(n, 256)), dim3(256), 0, s, disp16, n, out);
}

int launch_disp16_to_u8f(hipStream_t s, const short* disp16, size_t n, float* out) { return launch_disp16_convert(s, disp16, n, out); }
int launch_disp16_to_u8(hipStream_t s, const short* disp16, size_t n, uint8_t* out) { return launch_disp16_convert(s, disp16, n, out); }
