// Scanline optimisation of an aggregated cost volume (Mei et al. 2011, the step behind AD-Census + cross regions; not in the
// reference), hand-written for gfx950.
//
// V [n][H][W] the method's f32 volume, c = V where V is finite, else +inf.  Four paths r: LR (predecessor q = x-1), RL (x+1), TB (y-1),
// BT (y+1).  minq = min_k L_r(q,k).  q outside the frame or minq == +inf: L_r(p,k) = c(p,k).  Otherwise, one f32 operation each:
//     t0 = L_r(q,k);  t1 = L_r(q,k-1) + P1 (k > 0);  t2 = L_r(q,k+1) + P1 (k < n-1);  t3 = minq + P2
//     m = min(t0, t1, t2, t3);  L_r(p,k) = c(p,k) + (m - minq)
// S = ((L_LR + L_RL) + L_TB) + L_BT;  out = V finite ? S : V;  map = k_wta's rule on out.
//
// Design:
//  * one wavefront per scan line, candidate k on lane k & 63 (ceil(n / 64) candidates per lane).  The path's previous vector lives in
//    an LDS line of n + 2 floats whose two end slots hold +inf: the neighbours k-1 and k+1 are two more LDS reads of the same line,
//    whichever lane owns them, and an absent neighbour is +inf + P1 = +inf, which min() drops -- the border statements are the general
//    ones.  Two lines alternate (read one, write the other); the wave-wide minimum of a step goes through wave_min (asw_device.h);
//  * V lies [k][y][x].  It reaches the lanes through an LDS tile of n rows x TC cells (TC = 4..32: pick_tc), row stride TC + 1
//    floats: rows in coalesced, one cell per lane out with no bank conflict.  No load stands
//    under a condition (addresses are clamped), and a lane issues SB / VB of them before the first LDS store: one load per loop
//    round would make every round a memory round trip;
//  * S lies [y][x][k]: scratch in the layout that makes every step's access of a wavefront one contiguous run, straight from and
//    to the lanes;
//  * horizontal pass, one wavefront per row: LR forward, keeping only the vector that ENTERS every tile (a checkpoint, 1/TC of the
//    volume); then backward tile by tile: LR of the tile again from its checkpoint into a second LDS tile -- the same operations in
//    the same order, hence the same bits -- and RL back through the tile, S = L_LR + L_RL.  LR never makes an HBM round trip;
//  * vertical pass, XW neighbouring columns (wavefronts) per workgroup and TY rows per tile (XW * TY = TC): TB forward S += L_TB;
//    BT backward out = V finite ? S + L_BT : V written into the tile in place of V and stored over V by the workgroup, so every
//    (p,k) is read by the workgroup that then writes it and by nobody after.  The winner is taken in the BT pass from the lanes'
//    registers (wave minimum, lowest k among equals): a separate WTA launch would read the whole volume once more.
//
// The sign of a zero may differ from another implementation's min(); it is invisible to == and to every later addition's value.
#include <limits.h>

#include <algorithm>

#include "asw_device.h"
#include "asw_internal.h"

namespace {

constexpr int TC_MAX = 32;        // most cells (columns; or rows x columns) of a tile row
constexpr int TC_MIN = 4;         // fewest: n = 1025 still fits
constexpr int XW_MAX = 8;         // most columns (wavefronts) per workgroup of the vertical pass
constexpr int LDS_BYTES = 60000;  // what a workgroup's tiles and lines may take of its 64 KB
constexpr int LDS_SHARE = 30000;  // what a row's workgroup should stay within: five of them resident in a CU's 160 KB.  1080 rows are
                                  // 4.2 workgroups per CU; with four resident the last 56 rows ran as a second round (8.4 ms against 4.3)
constexpr int SB = 8;             // loads a lane of the horizontal pass keeps in flight while it stages a tile
constexpr int VB = 4;             // the same for a lane of the vertical pass (tile and sum)

struct ScanParams {
    int H, W, n;
    int tc, tc_log2;  // cells per tile row (a power of two)
    int xw, xw_log2;  // vertical pass: columns of a tile (a power of two); its rows are tc / xw
    int minD;
    float P1, P2;
};

constexpr float F_INF = __builtin_huge_valf();

__device__ __forceinline__ float finite_or_inf(float v) { return fabsf(v) < F_INF ? v : F_INF; }  // NaN, +inf, -inf -> +inf

// One step of a path for the wavefront's pixel.  cell: the pixel's V in the tile (row stride `ts`); prev / cur: the path's lines, slot
// k + 1 = candidate k; minq: the minimum of prev, +inf = the path starts here.  Returns the minimum of cur.  visit(k, v, L) sees every
// candidate's raw V and new L.
template <class Visit>
__device__ __forceinline__ float scan_step(const float* __restrict__ cell, int ts, const float* __restrict__ prev, float* __restrict__ cur, int n, float minq, float P1,
                                           float P2, int lane, Visit&& visit)
{
    float lmin = F_INF;
    const bool start = !(minq < F_INF);
    const float t3 = minq + P2;
    for (int k = lane; k < n; k += 64) {
        const float v = cell[k * ts];
        const float c = finite_or_inf(v);
        float L = c;
        if (!start) {
            const float t0 = prev[k + 1];
            const float t1 = prev[k] + P1;
            const float t2 = prev[k + 2] + P1;
            const float m = fminf(fminf(fminf(t0, t1), t2), t3);
            const float d = m - minq;
            L = c + d;
        }
        cur[k + 1] = L;
        lmin = fminf(lmin, L);
        visit(k, v, L);
    }
    const float r = wave_min(lmin);
    wave_lds_sync();  // the next step reads cur's neighbours
    return r;
}

// Horizontal pass of one row (blockIdx.x): S [y][x][k] = L_LR + L_RL.  ck [H][ntile][n]: the LR vector entering every tile.
__global__ __launch_bounds__(64) void k_scanline_h(ScanParams p, const float* __restrict__ V, float* __restrict__ S, float* __restrict__ ck)
{
    extern __shared__ float smem[];
    const int lane = threadIdx.x, y = blockIdx.x;
    const int H = p.H, W = p.W, n = p.n, tc = p.tc, ts = tc + 1, ntile = (W + tc - 1) / tc;
    float* tileC = smem;                  // V of the tile
    float* tileL = tileC + (size_t)n * ts;  // L_LR of the tile (backward half)
    float* line[4];                       // 0, 1: LR; 2, 3: RL
    for (int i = 0; i < 4; i++) line[i] = tileL + (size_t)n * ts + (size_t)i * (n + 2);
    if (lane < 4) { line[lane][0] = F_INF; line[lane][n + 1] = F_INF; }
    const size_t plane = (size_t)H * W;
    const float* vrow = V + (size_t)y * W;
    float* ckrow = ck + (size_t)y * ntile * n;

    auto stage = [&](int x0) {
        wave_lds_sync();
        const int total = n * tc;
        for (int i0 = lane; i0 < total; i0 += 64 * SB) {  // SB loads in flight, then their LDS stores
            float v[SB];
#pragma unroll
            for (int j = 0; j < SB; j++) {
                const int i = min(i0 + 64 * j, total - 1), k = i >> p.tc_log2, xx = i & (tc - 1);
                v[j] = vrow[(size_t)k * plane + min(x0 + xx, W - 1)];
            }
#pragma unroll
            for (int j = 0; j < SB; j++) {
                const int i = i0 + 64 * j;
                if (i < total) tileC[(i >> p.tc_log2) * ts + (i & (tc - 1))] = v[j];
            }
        }
        wave_lds_sync();
    };
    auto none = [](int, float, float) {};

    // forward: the checkpoints
    int cur = 0;
    float minq = F_INF;
    for (int t = 0; t < ntile; t++) {
        const int x0 = t * tc, cells = min(tc, W - x0);
        stage(x0);
        if (t > 0)  // tile 0: the path starts there
            for (int k = lane; k < n; k += 64) ckrow[(size_t)t * n + k] = line[cur][k + 1];
        if (t == ntile - 1) break;  // the last tile is run again below from its checkpoint
        for (int xx = 0; xx < cells; xx++) {
            minq = scan_step(tileC + xx, ts, line[cur], line[cur ^ 1], n, minq, p.P1, p.P2, lane, none);
            cur ^= 1;
        }
    }
    // backward, tile by tile: LR again from the checkpoint into tileL, then RL and the sum
    int rcur = 2;
    float rmin = F_INF;
    for (int t = ntile - 1; t >= 0; t--) {
        const int x0 = t * tc, cells = min(tc, W - x0);
        if (t != ntile - 1) stage(x0);  // the forward half left the last tile staged
        float lmin = F_INF;
        if (t > 0) {
            for (int k = lane; k < n; k += 64) {
                const float v = ckrow[(size_t)t * n + k];
                line[0][k + 1] = v;
                lmin = fminf(lmin, v);
            }
            wave_lds_sync();
        }
        minq = wave_min(lmin);  // tile 0: +inf, the path starts
        cur = 0;
        for (int xx = 0; xx < cells; xx++) {
            float* tl = tileL + xx;
            minq = scan_step(tileC + xx, ts, line[cur], line[cur ^ 1], n, minq, p.P1, p.P2, lane,
                             [&](int k, float, float L) { tl[k * ts] = L; });
            cur ^= 1;
        }
        for (int xx = cells - 1; xx >= 0; xx--) {
            const float* tl = tileL + xx;
            float* srow = S + ((size_t)y * W + x0 + xx) * n;
            rmin = scan_step(tileC + xx, ts, line[rcur], line[rcur ^ 1], n, rmin, p.P1, p.P2, lane,
                             [&](int k, float, float L) { srow[k] = tl[k * ts] + L; });
            rcur ^= 1;
        }
    }
}

// Vertical pass of XW columns.  BT false: TB forward, S += L_TB.  BT true: backward, out = V finite ? S + L_BT : V over V, and the map.
template <bool BT>
__global__ __launch_bounds__(XW_MAX * 64) void k_scanline_v(ScanParams p, float* __restrict__ V, float* __restrict__ S, float* __restrict__ disp)
{
    extern __shared__ float smem[];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), nthr = blockDim.x;
    const int H = p.H, W = p.W, n = p.n, tc = p.tc, ts = tc + 1, xw = p.xw, ty = tc >> p.xw_log2, ntile = (H + ty - 1) / ty;
    float* tile = smem;
    float* line[2];
    for (int i = 0; i < 2; i++) line[i] = tile + (size_t)n * ts + (size_t)(w * 2 + i) * (n + 2);
    if (lane < 2) { line[lane][0] = F_INF; line[lane][n + 1] = F_INF; }
    const int x0 = blockIdx.x * xw, x = x0 + w;
    const bool active = x < W;  // wave-uniform
    const size_t plane = (size_t)H * W;

    int cur = 0;
    float minq = F_INF;
    for (int ti = 0; ti < ntile; ti++) {
        const int t = BT ? ntile - 1 - ti : ti, y0 = t * ty, rows = min(ty, H - y0);
        __syncthreads();  // the tile's readers of the previous round are through
        const int total = n * tc;
        for (int i0 = tid; i0 < total; i0 += nthr * VB) {  // VB loads in flight, then their LDS stores
            float v[VB];
#pragma unroll
            for (int j = 0; j < VB; j++) {
                const int i = min(i0 + nthr * j, total - 1), k = i >> p.tc_log2, r = i & (tc - 1), yy = r >> p.xw_log2, xx = r & (xw - 1);
                v[j] = V[(size_t)k * plane + (size_t)min(y0 + yy, H - 1) * W + min(x0 + xx, W - 1)];
            }
#pragma unroll
            for (int j = 0; j < VB; j++) {
                const int i = i0 + nthr * j;
                if (i < total) tile[(i >> p.tc_log2) * ts + (i & (tc - 1))] = v[j];
            }
        }
        __syncthreads();
        if (active)
            for (int j = 0; j < rows; j++) {
                const int yy = BT ? rows - 1 - j : j;
                float* cell = tile + yy * xw + w;
                float* srow = S + ((size_t)(y0 + yy) * W + x) * n;
                float best = F_INF;
                int bk = INT_MAX;
                minq = scan_step(cell, ts, line[cur], line[cur ^ 1], n, minq, p.P1, p.P2, lane, [](int, float, float) {});
                cur ^= 1;
                // the sum, outside the step's dependent chain: VB loads of S in flight at once (clamped, never under a condition), then
                // the lane's own L from the line it has just written
                const float* Lp = line[cur];
                for (int k0 = lane; k0 < n; k0 += 64 * VB) {
                    float sv[VB];
#pragma unroll
                    for (int jj = 0; jj < VB; jj++) sv[jj] = srow[min(k0 + 64 * jj, n - 1)];
#pragma unroll
                    for (int jj = 0; jj < VB; jj++) {
                        const int k = k0 + 64 * jj;
                        if (k >= n) continue;
                        const float s = sv[jj] + Lp[k + 1];
                        if (!BT) {
                            srow[k] = s;
                        } else {
                            const float v = cell[k * ts];
                            const float o = fabsf(v) < F_INF ? s : v;
                            cell[k * ts] = o;
                            if (o < best) { best = o; bk = k; }  // ascending k, strict '<' from +inf: NaN and +inf never win
                        }
                    }
                }
                if (BT) {
                    const float m = wave_min(best);
                    const int kk = wave_min(best == m ? bk : INT_MAX);  // no lane was updated: INT_MAX everywhere
                    if (lane == 0) disp[(size_t)(y0 + yy) * W + x] = kk == INT_MAX ? 0.0f : (float)(p.minD + kk);
                }
            }
        if (BT) {
            __syncthreads();
            for (int i = tid; i < n * tc; i += nthr) {
                const int k = i >> p.tc_log2, r = i & (tc - 1), yy = r >> p.xw_log2, xx = r & (xw - 1);
                if (yy < rows && x0 + xx < W) V[(size_t)k * plane + (size_t)(y0 + yy) * W + x0 + xx] = tile[k * ts + r];
            }
        }
    }
}

size_t h_bytes(int n, int tc) { return ((size_t)2 * n * (tc + 1) + (size_t)4 * (n + 2)) * sizeof(float); }
size_t v_bytes(int n, int tc, int xw) { return ((size_t)n * (tc + 1) + (size_t)2 * xw * (n + 2)) * sizeof(float); }

// Cells of a tile row (a power of two in TC_MIN .. TC_MAX); 0: none fits.  Vertical pass: the largest whose workgroup fits LDS_BYTES.
// Horizontal pass: the largest whose workgroup fits LDS_SHARE, and TC_MIN within LDS_BYTES where none does.
int pick_tc(int n, bool vertical)
{
    for (int tc = TC_MAX; tc >= TC_MIN; tc /= 2)
        if (vertical ? v_bytes(n, tc, std::min(tc, XW_MAX)) <= (size_t)LDS_BYTES : h_bytes(n, tc) <= (size_t)LDS_SHARE) return tc;
    return !vertical && h_bytes(n, TC_MIN) <= (size_t)LDS_BYTES ? TC_MIN : 0;
}

}  // namespace

int scanline_max_planes() { return 1025; }

size_t scanline_checkpoint_floats(int H, int W, int n)
{
    const int tc = pick_tc(n, false);
    return tc ? (size_t)H * ((W + tc - 1) / tc) * n : 0;
}

int launch_scanline(hipStream_t s, const ScanlineLaunch& a)
{
    if (a.H < 1 || a.W < 1 || (size_t)a.H * a.W >= ((size_t)1 << 31) || a.n < 1 || a.n > scanline_max_planes()) return ASW_ERR_BAD_ARGUMENT;
    if (!a.vol || !a.sum || !a.ck || !a.disp) return ASW_ERR_BAD_ARGUMENT;
    ScanParams p;
    p.H = a.H; p.W = a.W; p.n = a.n; p.minD = a.minD; p.P1 = a.P1; p.P2 = a.P2;
    p.tc = pick_tc(a.n, false); p.xw = 1; p.xw_log2 = 0;
    ScanParams v = p;
    v.tc = pick_tc(a.n, true);
    if (!p.tc || !v.tc) return ASW_ERR_BAD_ARGUMENT;
    p.tc_log2 = __builtin_ctz(p.tc); v.tc_log2 = __builtin_ctz(v.tc);
    v.xw = std::min(v.tc, XW_MAX); v.xw_log2 = __builtin_ctz(v.xw);
    ASW_TRY(ASW_LAUNCH(k_scanline_h, dim3(a.H), dim3(64), h_bytes(a.n, p.tc), s, p, a.vol, a.sum, a.ck));
    const dim3 grid((a.W + v.xw - 1) / v.xw), block(v.xw * 64);
    const size_t vb = v_bytes(a.n, v.tc, v.xw);
    ASW_TRY(ASW_LAUNCH(k_scanline_v<false>, grid, block, vb, s, v, a.vol, a.sum, a.disp));
    return ASW_LAUNCH(k_scanline_v<true>, grid, block, vb, s, v, a.vol, a.sum, a.disp);
}
