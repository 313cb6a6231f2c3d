// Census cost kernels in front of the cross-based aggregation: the AD-Census cost of Mei et al. 2011 (census of Zabih & Woodfill 1994).
// Not in the reference; the definition is DESIGN.md section 4.13.  All integer:
//   code   62 bits per pixel of a gray image G, one per offset (dy, dx), dy in -3..3, dx in -4..4, (0, 0) excluded: 1 exactly when
//          G[clamp(y + dy)][clamp(x + dx)] < G[y][x]; bit (dy + 3) * 9 + dx + 4 of a 64-bit word (bit 31, the centre, stays 0)
//   ham    popcount(codeA[x] ^ codeB[reflect(x + s * off)]), 0..62
//   e      TA[ad] + TC[ham], ad the u8 value of k_cost_ad for the same pair, direction and plane, both tables in 0..127
// k_census_transform runs once per image, k_cost_census over all candidates.
#include "asw_device.h"
#include "asw_internal.h"

namespace {

constexpr int CW = 64, CH = 16;      // pixels a workgroup of the transform owns: a thread takes 4 rows of one column
constexpr int RX = 4, RY = 3;        // half-window
constexpr int TS = CW + 2 * RX;      // bytes per staged row
constexpr int TROWS = CH + 2 * RY;
constexpr int TAB_BYTES = 256 + 64;  // TA[256], TC[63] + one byte of padding

__global__ __launch_bounds__(256) void k_census_transform(const uint8_t* __restrict__ gray, int H, int W, uint2* __restrict__ code)
{
    __shared__ uint8_t tile[TROWS * TS];
    const int tid = threadIdx.x, x0 = blockIdx.x * CW, y0 = blockIdx.y * CH;
    for (int i = tid; i < TROWS * TS; i += 256) {
        const int r = i / TS, c = i - r * TS;
        const int yy = min(max(y0 - RY + r, 0), H - 1), xx = min(max(x0 - RX + c, 0), W - 1);
        tile[i] = gray[(size_t)yy * W + xx];
    }
    __syncthreads();
    const int tx = tid & 63, r0 = (tid >> 6) * 4;  // rows y0 + r0 .. y0 + r0 + 3
    uint32_t centre[4], lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0};
#pragma unroll
    for (int p = 0; p < 4; p++) centre[p] = tile[(r0 + p + RY) * TS + tx + RX];
    // the ten tile rows under the four windows, each read once: row rr serves pixel p at dy = rr - RY - p
#pragma unroll
    for (int rr = 0; rr < 4 + 2 * RY; rr++) {
        uint32_t v[2 * RX + 1];
#pragma unroll
        for (int c = 0; c <= 2 * RX; c++) v[c] = tile[(r0 + rr) * TS + tx + c];
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const int dy = rr - RY - p;
            if (dy < -RY || dy > RY) continue;
#pragma unroll
            for (int c = 0; c <= 2 * RX; c++) {
                const int bit = (dy + RY) * (2 * RX + 1) + c;
                const uint32_t b = v[c] < centre[p] ? 1u : 0u;
                if (bit < 32) lo[p] |= b << bit; else hi[p] |= b << (bit - 32);
            }
        }
    }
    const int x = x0 + tx;
#pragma unroll
    for (int p = 0; p < 4; p++) {
        const int y = y0 + r0 + p;
        if (x < W && y < H) code[(size_t)y * W + x] = make_uint2(lo[p], hi[p]);
    }
}

// One workgroup: one row and a slab of dPerBlock candidates, like k_cost_ad.  In LDS: the two code rows, and for the combined
// form (C = 1 or 3 image channels; C = 0: the Hamming distance alone) the two tables and the two image rows.  A thread owns 4
// consecutive pixels, whose codes and colours stay in registers across the slab: one dword store per plane.
template <int C>
__global__ __launch_bounds__(256) void k_cost_census(const uint8_t* __restrict__ L, const uint8_t* __restrict__ R,
                                                     const uint2* __restrict__ codeL, const uint2* __restrict__ codeR,
                                                     const uint8_t* __restrict__ tables, int H, int W, int disp_type, int minD,
                                                     int numD, int dPerBlock, uint8_t* __restrict__ cost)
{
    extern __shared__ __align__(16) uint8_t census_smem[];
    uint2* ca = reinterpret_cast<uint2*>(census_smem);  // view-side codes (left for LEFT, right for RIGHT)
    uint2* cb = ca + W;
    uint8_t* ta = census_smem + (size_t)2 * W * sizeof(uint2);
    uint8_t* tc = ta + 256;
    uint8_t* sa = ta + TAB_BYTES;
    uint8_t* sb = sa + (size_t)W * (C ? C : 1);
    const int y = blockIdx.x;
    const bool left = disp_type == ASW_DISPARITY_LEFT;
    const uint2* ga = (left ? codeL : codeR) + (size_t)y * W;
    const uint2* gb = (left ? codeR : codeL) + (size_t)y * W;
    for (int i = threadIdx.x; i < W; i += 256) {
        ca[i] = ga[i];
        cb[i] = gb[i];
    }
    if (C) {
        const uint8_t* ra = (left ? L : R) + (size_t)y * W * C;
        const uint8_t* rb = (left ? R : L) + (size_t)y * W * C;
        for (int i = threadIdx.x; i < W * C; i += 256) {
            sa[i] = ra[i];
            sb[i] = rb[i];
        }
        for (int i = threadIdx.x; i < TAB_BYTES; i += 256) ta[i] = tables[i];
    }
    __syncthreads();
    const int k0 = blockIdx.y * dPerBlock, k1 = min(numD, k0 + dPerBlock);
    const int sgn = left ? -1 : 1;  // LEFT pairs x with x - off, RIGHT with x + off
    const bool dword_rows = (W & 3) == 0;
    for (int x4 = threadIdx.x * 4; x4 < W; x4 += 256 * 4) {
        uint2 a[4];
        int pa[4][C ? C : 1];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int x = min(x4 + j, W - 1);
            a[j] = ca[x];
#pragma unroll
            for (int c = 0; c < C; c++) pa[j][c] = sa[x * C + c];
        }
        for (int k = k0; k < k1; k++) {
            const int xs = x4 + sgn * (minD + k);
            int xp[4];  // the four partner columns
            if (xs >= 0 && xs + 3 < W) {  // xs .. xs + 3: no reflection
#pragma unroll
                for (int j = 0; j < 4; j++) xp[j] = xs + j;
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) xp[j] = reflect_idx(min(x4 + j, W - 1) + sgn * (minD + k), W);
            }
            uint32_t packed = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int xb = xp[j];
                const uint2 b = cb[xb];
                const int ham = __popc(a[j].x ^ b.x) + __popc(a[j].y ^ b.y);
                uint32_t v = (uint32_t)ham;
                if constexpr (C == 3) {
                    const uint32_t ad = mean3_u8(abs(pa[j][0] - (int)sb[xb * 3]), abs(pa[j][1] - (int)sb[xb * 3 + 1]),
                                                 abs(pa[j][2] - (int)sb[xb * 3 + 2]));
                    v = (uint32_t)ta[ad] + (uint32_t)tc[ham];
                } else if constexpr (C == 1) {
                    v = (uint32_t)ta[abs(pa[j][0] - (int)sb[xb])] + (uint32_t)tc[ham];
                }
                packed |= v << (8 * j);
            }
            uint8_t* out = cost + ((size_t)k * H + y) * W;
            if (dword_rows) {  // W % 4 == 0: every row starts on a dword and x4 + 3 < W
                *reinterpret_cast<uint32_t*>(out + x4) = packed;
            } else {
                for (int j = 0; j < 4 && x4 + j < W; j++) out[x4 + j] = (uint8_t)(packed >> (8 * j));
            }
        }
    }
}

}  // namespace

int launch_census_transform(hipStream_t s, const uint8_t* gray, int H, int W, uint2* code)
{
    const dim3 grid((W + CW - 1) / CW, (H + CH - 1) / CH);
    if (grid.y > 65535) return ASW_ERR_BAD_ARGUMENT;
    return ASW_LAUNCH(k_census_transform, grid, dim3(256), 0, s, gray, H, W, code);
}

int launch_cost_census(hipStream_t s, const uint8_t* L, const uint8_t* R, const uint2* codeL, const uint2* codeR, int H, int W, int C,
                       int disp_type, int minD, int numD, const uint8_t* tables, uint8_t* cost)
{
    if (tables && C != 1 && C != 3) return ASW_ERR_BAD_ARGUMENT;
    const int dPerBlock = 16;
    const dim3 grid(H, (numD + dPerBlock - 1) / dPerBlock);
    // staged rows: 16 W bytes of codes, and for the combined form 2 C W bytes of colours + the tables
    const size_t lds = (size_t)2 * W * sizeof(uint2) + (tables ? (size_t)2 * W * C + TAB_BYTES : 0);
    if (!tables)
        ASW_TRY(ASW_LAUNCH(k_cost_census<0>, grid, dim3(256), lds, s, L, R, codeL, codeR, tables, H, W, disp_type, minD, numD, dPerBlock, cost));
    else if (C == 3)
        ASW_TRY(ASW_LAUNCH(k_cost_census<3>, grid, dim3(256), lds, s, L, R, codeL, codeR, tables, H, W, disp_type, minD, numD, dPerBlock, cost));
    else
        ASW_TRY(ASW_LAUNCH(k_cost_census<1>, grid, dim3(256), lds, s, L, R, codeL, codeR, tables, H, W, disp_type, minD, numD, dPerBlock, cost));
    return ASW_OK;
}
