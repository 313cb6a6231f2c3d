// Classic bilateral adaptive-support-weight aggregation (computeAdaptiveWeight, M.cpp:1016-1156), second kernel form:
// thread = 4 pixels x 4 right-image positions ("xq blocking").  Used for DISPARITY_LEFT, 15x15 windows and long candidate
// ranges (the reference's call site at 1080p, configs C5/C3-sized frames); everything else stays on k_asw_bilateral.
//
// Per (pixel x, candidate d) the reference adds, in tap order i (kernel_x = i / 15 outer, kernel_y = i % 15 inner):
//     ab   = wL_i(y,x) * wR_i(y, max(0,x-d))          f32 product
//     num += ab * |gL(ny,nx) - gR(ny, max(0,nx-d))|   f64        nx = clamp(x - 7 + kernel_x), ny = clamp(y - 7 + kernel_y)
//     den += ab                                       f64
// Put q = x - d (the right-image position of the pair).  Then
//     * the weight pair of a unit is (wL_i(x), wR_i(q))                       -> outer product over a block of x's and q's
//     * away from the right image border its cost sample is |gL(x+kx-7) - gR(q+kx-7)|: the SAME value that the unit
//       (x+1, q+1) -- same d, next pixel -- needs one tap column earlier.
// A thread owns pixels X..X+3 and positions Q..Q+3 (16 units, d = X+a - (Q+b)); unit (a,b) runs b tap columns behind the
// thread's step counter K (kx = K - b), so all units on a diagonal a-b (one d, up to four pixels) consume ONE cost value per
// step: 7 integer instructions per 16 units.  Every unit still adds its own taps in ascending i, in f64, with the exact
// product -- E is bit-identical to the reference order (fma(ab,c,num) == num + ab*c because ab*c is exact: 24-bit x 8-bit
// significands).
//
// Scaled domain.  The cost sample |gL - gR| in 0..255 is produced by one v_sad into the low word of a register pair whose
// high word is zero: as an f64 that pair is the denormal c * 2^-1074 (the kernel preserves f64 denormals), so no f64
// subtraction or conversion is needed.  The weights are staged from a LUT scaled by 2^60 (exact in f32), so that the f32
// product is ab' = ab * 2^120 and
//     den' = sum ab'                      = den * 2^120                 exactly,
//     num' = sum fma(ab', c * 2^-1074)     = num * 2^-954                exactly,
// E = ldexp(num', 954) / ldexp(den', -120) is then the same IEEE quotient num / den as in the reference.  This holds when every
// nonzero product ab >= 2^-68: the f32 products stay normal in both domains, every nonzero ab * c * 2^-954 is >= 2^-1022, so
// every partial sum of num' is normal (or zero) and rounds as num does, only 954 binades lower.  The host checks the bound on the
// LUT (bilateral_xq_lut_ok) and takes the one-kernel form where it does not hold.
//
// Workgroup = one image row x 64 pixels x 32 position blocks (d = minD + 4j + a - b, j < 32): 8 wavefronts, lane -> (pixel
// group g, position block 4*wave + ((lane >> 3) & 3)); the lane -> g map is chosen for the LDS banks, see the kernel.  All 512
// threads share the staged weights of a step:
//     left : wL(x, tap column kx)   for the 64 pixels        -> ring of 5 tap columns in LDS (a column is used for 4 steps)
//     right: wR(q, tap column K-b)  for the 188 positions    -> b = (q - Q) mod 4 is a property of the position, so the buffer of
//            step K holds, per position, exactly the tap column that position's units consume at step K (double buffered)
// i.e. 7.5 weight evaluations per thread and step instead of 33 with wave-private staging, one workgroup barrier per step
// (18 steps of 15 rows), no cost tile, gray tiles as u32 in LDS.
// Block j = 0 holds six units with d < minD (a < b) and a block j = 32 would hold exactly six units with c = d - minD < 128
// in the same slots (c = 128 + a - b): the j = 0 threads run those instead ("wrapped" units: second position base qrel2,
// second right gray), so the 512 threads finish candidates [0, 128) with no idle unit.  A tail [128, nD) of more than one
// candidate is left to k_asw_bilateral (its winners go to a second slice, k_merge_slices picks the first minimum).
//
// The inclusive last candidate (LASTC).  The reference's range is inclusive (M.cpp:1021,1074): numDisparity 128 / 64 are 129 /
// 65 candidates, NFIN + 1.  Every operand of candidate NFIN is staged in the workgroup already -- the left weights of the 64
// pixels in the ring, the right weights and grays of positions posmin + 0..63 (RIGHT: + 4 NJ) for the wrapped units -- so the
// interior tiles' LASTC instantiation finishes it: 64 more units, one per pixel, in ONE plain wavefront, the last (UWAVE = NW -
// 1: not on wave 0's SIMD, and the wavefront that stages a window row fewer than the others, which pays for most of the
// unit).  Lane -> pixel 4g + a with a = (lane >> 3) & 3 (the four lanes that share a g), position index 4g + a (+ 4 NJ), unit
// row b = a, so the right buffer of step K holds tap column K - a for it and the unit runs a columns behind like every other:
// left weight from ring slot (K - a) mod 5, right weight from buffer K & 1, grays at tile columns 4g + K (left: the diagonal-0
// sample of the row's own quads) and 4g + K (+ 4 NJ) (right) -- the skew cancels in both; one v_sad_u16, one f32 multiply, one
// cvt, one fma, one add per row, taps in the same ascending order: E is bit-identical.  Lane-steps with K - a outside 0..14 add
// +0.0 to both sums: the right weight is the all-zero class there, and the left operand is finite -- the ring slots of columns
// -3..-1 (slots 2..4) are zeroed in the prologue, columns 15..17 find older columns, and the slot index is a non-negative
// modulus.  Registers are the whole difficulty (wave 0 needs all 128): the LASTC kernels carry nothing that is a function of
// the lane number through the row loops (FRESH: the lane number is taken afresh in every step, in all eight wavefronts, and what
// hangs on it -- clamped positions, the row loop's bases -- is read from the step tables), the unit's wavefront runs with its wave number as a constant (its
// missing staging row folds away), and the other wavefronts' row loops carry nothing of the unit's sums.  Epilogue: sE holds NFIN + 1 planes, plane NFIN goes to vol and enters the
// WTA last with the same strict '<' (still the first minimum in ascending d), and the kernel writes disp.
// The border tiles (EDGE; they spill at one row per body and cannot host the unit) keep the slice sequence on their own
// columns: EDGE launch -> slice 0, k_asw_bilateral for candidate NFIN on a column window -> slice 1, k_merge_slices_cols over the
// window.  Interior and border launches write disjoint columns of disp and vol, so the launch count stays 4 and nothing is
// written twice.
//
// DISPARITY_RIGHT (M.cpp:1113-1142; RIGHT = true): the fixed image is the right one (the host passes it as gL) and the pair of
// pixel x is the left-image position q = min(W-1, x + d).  Nothing in the blocking depends on the sign of d: unit (a,b) is
// still (pixel X+a, position Q+b) with tap column K - b, d = (Q+b) - (X+a) = minD + 4j + b - a, so the dead units of block 0 are
// those with b < a and the positions run to the right of the tile.  Sample columns clamp the other way round: the tile clamps
// coincide with the reference's at the right image border, not at the left one, so the border tiles are the first of a row.

#include <algorithm>
#include <cmath>
#include <type_traits>

#include "asw_device.h"
#include "asw_internal.h"

namespace {

constexpr int HH = 7;                     // half window
constexpr int KS = 2 * HH + 1;            // 15
constexpr int PXW = 64;                   // pixels per workgroup
constexpr int LWC = PXW + 2 * HH;         // left tile columns  [x0 - 7, x0 + 70]
constexpr int NSTEP = KS + 3;             // 18 steps: unit row b runs b tap columns behind
constexpr int RING = 5;                   // tap columns of left weights kept (4 in use + the one being staged)
constexpr int URI = 3;                    // window rows per body of the row loop (interior tiles)
constexpr int CROW = 6;                   // rows in front of the mid-step stage_commit
// How far ahead of their use the interior tiles' row loops read LDS (run_step), per register class of the wavefront:
//   class 0  plain wavefronts of the LASTC kernels (six of eight) and everything at NW = 4 (168 VGPRs)
//   class 1  wave 0 (second right weights / gray) and the unit's wavefront of the NW = 8 LASTC kernels
//   class 2  the NW = 8 kernels without LASTC, which carry the lane-derived values through the loops
// PF_HEAD[class][loop]: what of a row's head is read during the previous row's last block, in the loop in front of the mid-step
// commit (the staged weights of the next step are live there: eight more registers) and in the loop behind it -- PF_GRAY the
// right gray and the left gray quads, PF_WR the right weights, PF_WL the left weights of the row's first block; the rest is read
// at the head of the row itself, as it used to be.  PF_WLEAD[class]: blocks between the read of a left-weight quad and its block.
// Each entry is the deepest form at which every kernel of the class keeps to 128 VGPRs without scratch (NW = 4: 168).
constexpr int PF_GRAY = 4, PF_WR = 2, PF_WL = 1, PF_ALL = 7;
constexpr int PF_HEAD[3][2] = {{PF_ALL, PF_ALL}, {PF_WR | PF_WL, PF_GRAY | PF_WL}, {0, PF_GRAY}}, PF_WLEAD[3] = {2, 2, 1};
static_assert(KS % URI == 0 && CROW % URI == 0, "whole bodies");
constexpr int NCELLCOL = NSTEP + 3;       // cell-table columns kx = -3 .. 17
constexpr int LW8 = 80;                   // u8 row stride of the left tile (multiple of 4)
constexpr int LWP = 80;                   // u32 row stride of the left gray tile (multiple of 4 >= LWC)

// Everything that depends on the number of wavefronts NW of a workgroup (8: 128 candidates per pass -- the reference's
// configuration at 1080p; 4: 64 candidates -- its own call site, aswStereoMatch.cpp:94, numDisparity 64 -> 65 candidates):
//   NJ    position blocks per workgroup (+ the wrapped units of block NJ)
//   NPOS  right-image positions a workgroup touches: [posmin, posmin + NPOS - 1]
//   RWC   right tile columns [posmin - 7, posmin + NPOS + 6]
//   NFIN  candidates [0, NFIN) are finished by the kernel
// LDS layout (bytes): left block [KS] x {float [RING][PXW] left weights, u32 [LWP] left gray} | right block [KS] x {float [2][NPOS]
// right weights, u32 [RWP] right gray} | u8 [KS][LW8] | u8 [KS][RW8] | u8 [4][64] lane table | u16 [3][64] row-loop bases |
// u32 [NCELLCOL * KS] cell table (the three tables: see "Step tables" below).  Weights and
// grays of a window row share one row stride per side, so that every LDS address of the row loop is one of two per-lane bases
// (three in wave 0) plus an immediate offset: two address increments per body of three rows.
// Epilogue (over the dead tiles): double [NFIN + 1][PXW] E | per-part WTA partials double E[NW][PXW], float d[NW][PXW].
// NW = 8: 70 KB (the epilogue's), two workgroups = 16 wavefronts per CU; NW = 4: 52 KB, three workgroups = 12 wavefronts per CU.
template <int NW>
struct XqCfg {
    static constexpr int NWAVE = NW;
    static constexpr int NTHR = 64 * NW;
    static constexpr int NJ = 4 * NW;
    static constexpr int NPOS = PXW + 4 * NJ;
    static constexpr int RWC = NPOS + 2 * HH;
    static constexpr int NFIN = 4 * NJ;
    static constexpr int RW8 = (RWC + 3) / 4 * 4;
    static constexpr int NROWS = (KS + NW - 1) / NW;  // window rows a wavefront stages
    // Gray tiles for the cost samples: u32, the operands of v_sad (the left rows padded to a multiple of four words, so that the
    // grays of a step are read as 16-byte aligned quads)
    static constexpr int RWP = (RWC + 3) / 4 * 4;
    static constexpr int LROW = RING * PXW + LWP;  // words per window row, left block
    static constexpr int RROW = 2 * NPOS + RWP;    // words per window row, right block
    static constexpr int LGRAY = RING * PXW;       // left gray, word offset in a row
    static constexpr int RGRAY = 2 * NPOS;         // right gray, word offset in a row
    static constexpr int OFF_LB = 0;
    static constexpr int OFF_RB = OFF_LB + KS * LROW * 4;
    static constexpr int OFF_L8 = OFF_RB + KS * RROW * 4;
    static constexpr int OFF_R8 = OFF_L8 + KS * LW8;
    // (the cell table last: its addresses are built from a constant in a register anyway, the other two tables' have to fit the
    // 16-bit offset field next to the lane number)
    static constexpr int OFF_LANE = OFF_R8 + KS * RW8;
    static constexpr int OFF_BASE = OFF_LANE + 4 * 64;
    static constexpr int OFF_CELL = OFF_BASE + 3 * 64 * 2;
    static constexpr int OFF_STEP_END = OFF_CELL + NCELLCOL * KS * 4;
    static constexpr int OFF_E64 = 0;
    static constexpr int OFF_PART = (NFIN + 1) * PXW * 8;  // plane NFIN: the last-candidate units' (LASTC)
    // the epilogue buffers reuse the dead tiles; for NW = 8 they are the larger of the two
    static constexpr int LDS_TOTAL = std::max((OFF_STEP_END + 15) / 16 * 16, OFF_PART + NW * PXW * 12);
    static_assert(LDS_TOTAL <= (NW == 8 ? 80 : 53) * 1024, "two (NW = 8) / three (NW = 4) workgroups per CU");
    static_assert(OFF_RB % 16 == 0 && (LROW * 4) % 16 == 0 && (RROW * 4) % 16 == 0 && (NPOS * 4) % 16 == 0 && (LGRAY * 4) % 16 == 0, "b128 alignment");
    static_assert(NPOS % 64 == 0 && NPOS / 64 <= 3, "positions are staged in whole wavefront passes; three columns of the lane table");
    static_assert(OFF_CELL % 4 == 0 && OFF_BASE % 2 == 0 && OFF_CELL < 65536 && OFF_RB + 4 * NPOS < 65536, "table alignment; offset fields; u16 bases");
    static_assert((2 * HH) * LW8 + 2 * HH < (1 << 11) && (2 * HH) * RW8 + 2 * HH < (1 << 12), "cell entry fields");
};
#define XQ_CONSTS(NW)                                                                                                           \
    typedef XqCfg<NW> Cfg;                                                                                                       \
    constexpr int NWAVE = Cfg::NWAVE, NTHR = Cfg::NTHR, NJ = Cfg::NJ, NPOS = Cfg::NPOS, RWC = Cfg::RWC, NFIN = Cfg::NFIN, RW8 = Cfg::RW8,      \
                  NROWS = Cfg::NROWS, LROW = Cfg::LROW, RROW = Cfg::RROW, LGRAY = Cfg::LGRAY, RGRAY = Cfg::RGRAY,               \
                  OFF_LB = Cfg::OFF_LB, OFF_RB = Cfg::OFF_RB, OFF_L8 = Cfg::OFF_L8, OFF_R8 = Cfg::OFF_R8, OFF_CELL = Cfg::OFF_CELL,  \
                  OFF_LANE = Cfg::OFF_LANE, OFF_BASE = Cfg::OFF_BASE,                                                            \
                  LDS_TOTAL = Cfg::LDS_TOTAL, OFF_E64 = Cfg::OFF_E64, OFF_PART = Cfg::OFF_PART;                                  \
    (void)NWAVE; (void)NTHR; (void)NJ; (void)NPOS; (void)RWC; (void)NFIN; (void)RW8; (void)NROWS; (void)LROW; (void)RROW; (void)LGRAY;  \
    (void)RGRAY; (void)OFF_LB; (void)OFF_RB; (void)OFF_L8; (void)OFF_R8; (void)OFF_CELL; (void)OFF_LANE; (void)OFF_BASE; (void)LDS_TOTAL; (void)OFF_E64; (void)OFF_PART;

struct XqParams {
    int H, W, minD;
    int tile0;  // first 64-pixel tile of this launch (interior tiles and border tiles are separate launches)
};

// The cost sample of the scaled domain: |gl - gr| (both in 0..255) in the low word of a pair whose high word is zero, i.e. the
// f64 denormal |gl - gr| * 2^-1074.  The zero high word is an opaque register (hi0, set once per step outside the row loop)
// so that the compiler keeps it in place instead of rematerialising a v_mov per sample in the loop.
__device__ __forceinline__ double cost_sample(uint32_t gl, uint32_t gr, uint32_t hi0)
{
    const uint32_t c = __builtin_amdgcn_sad_u16(gl, gr, 0u);  // the high halves are zero: |gl - gr|
    return __builtin_bit_cast(double, (uint64_t)c | ((uint64_t)hi0 << 32));
}

// Step tables: everything a step needs that depends on the window cell, the lane and two workgroup-uniform clamps only is
// built once in the prologue and looked up in every step, instead of being derived again 18 times.
//   cell table  u32 per cell (kx = -3..17, ky): the byte offsets of the weight's neighbour sample in the u8 gray tiles, relative
//               to the tile column of the pixel / position itself -- left (HH + dyw) * LW8 + HH + dxw (11 bits: bits 0..7 and
//               16..18), right (HH + dyw) * RW8 + HH + dxw (bits 20..31) -- and the class in its place in the LUT index (bits
//               8..15).  The right fields, the ones every lane decodes, cost one instruction each; the left entry is
//               wave-uniform and is taken apart by the scalar unit.
//   lane table  u8 [4][64]: columns r3 = 0..2 the clamped position of lane + 64 r3, column 3 the lane's cell-table skew
//               4 KS (lane & 3) (its positions run lane & 3 tap columns behind the step counter)
//   bases       u16 [3][64]: the row loop's LDS bases of a lane: left 16 g, right OFF_RB + 4 qrel and wave 0's wrapped
//               OFF_RB + 4 qrel2, the right ones for wave 0 (wavefront w is 64 w bytes below (LEFT) / above (RIGHT) them)
__host__ __device__ constexpr uint32_t cell_entry(int dxw, int dyw, int cls256, int RW8)
{
    const uint32_t loff = (uint32_t)((HH + dyw) * LW8 + HH + dxw), roff = (uint32_t)((HH + dyw) * RW8 + HH + dxw);
    return (loff & 255u) | (uint32_t)cls256 | ((loff >> 8) << 16) | (roff << 20);
}

// Stage the weights step `Kn` consumes: left tap column Kn (ring slot Kn % RING) and the right buffer Kn & 1.
// Wave w evaluates window rows ky = w and w + 8.  Cell (kx, ky) -> {dxw, dyw, class}: the direction the reference BUILT
// weight map i for (transposed w.r.t. the sample it is applied to), all-zero class for the skipped cell and
// for kx outside the window.
// Split in two so that the LUT gathers of step Kn are in flight while step Kn - 1 is being accumulated: stage_issue (index
// pass + gathers, at the top of the step) and stage_commit (LDS writes, in the middle of the step's row loop).  Done in one
// piece in front of the step, the staging cost 10 % of the kernel for 5 % of its instructions: eight wavefronts waiting for
// the same two memory round trips (ablation: profiles/r02/ablation_*.csv).
template <int NW> struct Staged { float v[XqCfg<NW>::NROWS][1 + XqCfg<NW>::NPOS / 64]; };

template <int NW>
__device__ __forceinline__ void stage_issue(int Kn, const float* __restrict__ lut, const unsigned char* smem, int wave, int lane,
                                            Staged<NW>& st)
{
    XQ_CONSTS(NW)
    const uint8_t* sL8 = smem + OFF_L8;
    const uint8_t* sR8 = smem + OFF_R8;
    const uint8_t* sLane = smem + OFF_LANE;
    // the weight is evaluated AT max(0, x - d) (M.cpp:1105); its neighbour is clamped from there (tile columns are
    // replicate-clamped, so adding the direction needs no further clamp)
    int pc[NPOS / 64], ctr[NPOS / 64];  // clamped position of lane + 64 r3 and the gray there
#pragma unroll
    for (int r3 = 0; r3 < NPOS / 64; r3++) pc[r3] = sLane[64 * r3 + lane];
    // posmin == Q (mod 4): the unit row b = lane & 3 a position belongs to is a property of the position; skew = 4 KS b
    const int skew = sLane[64 * 3 + lane];
#pragma unroll
    for (int r3 = 0; r3 < NPOS / 64; r3++) ctr[r3] = sR8[HH * RW8 + HH + pc[r3]];
    const int ctrL = Kn < KS ? sL8[HH * LW8 + HH + lane] : 0;
    // the lane's cell entry of the wavefront's first row; the other rows are NWAVE entries on (opaque: one address per step)
    typedef __attribute__((address_space(3))) const unsigned char lds_u8;
    lds_u8* pcell = (lds_u8*)smem + OFF_CELL + 4 * ((Kn + 3) * KS + wave) - skew;
    asm("" : "+v"(pcell));
#pragma unroll
    for (int rr = 0; rr < NROWS; rr++) {
        const int ky = wave + NWAVE * rr;
        if (ky >= KS) break;  // wave-uniform
        const uint32_t u = *(const __attribute__((address_space(3))) uint32_t*)(pcell + 4 * NWAVE * rr);
        if (Kn < KS) {        // left column Kn exists
            // its entry is the one of the lanes with b = 0, lane 0 among them (every lane of the wavefront is active here): taken
            // from there as a scalar, it is decoded by the scalar unit
            const uint32_t u0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)u);
            const int nb = sL8[((u0 & 255u) | ((u0 >> 8) & 0x700u)) + lane];
            st.v[rr][0] = lut_at(lut, __builtin_amdgcn_sad_u16(nb, ctrL, u0 & 0xff00u));
        }
        const int roff = (int)(u >> 20), cls = (int)(u & 0xff00u);
#pragma unroll
        for (int r3 = 0; r3 < NPOS / 64; r3++) {
            const int nb = sR8[roff + pc[r3]];
            st.v[rr][1 + r3] = lut_at(lut, __builtin_amdgcn_sad_u16(nb, ctr[r3], cls));
        }
    }
}

template <int NW>
__device__ __forceinline__ void stage_commit(int Kn, unsigned char* smem, int wave, int lane, const Staged<NW>& st)
{
    XQ_CONSTS(NW)
    // one address per side (the lane's word in the wavefront's first row), everything else in the offset fields.  The right one
    // stands OFF_RB % 256 bytes in, so that what the offsets add is a multiple of 256 and pairs of stores need no base of their own.
    typedef __attribute__((address_space(3))) float lds_f32;
    typedef __attribute__((address_space(3))) unsigned char lds_u8w;
    lds_u8w* cL = (lds_u8w*)smem + 4 * LROW * wave + 4 * lane;
    lds_u8w* cR = (lds_u8w*)smem + 4 * RROW * wave + 4 * lane + OFF_RB % 256;
    asm("" : "+v"(cL), "+v"(cR));
#pragma unroll
    for (int rr = 0; rr < NROWS; rr++) {
        const int ky = wave + NWAVE * rr;
        if (ky >= KS) break;
        if (Kn < KS) *(lds_f32*)(cL + OFF_LB + 4 * (Kn % RING) * PXW + 4 * LROW * NWAVE * rr) = st.v[rr][0];
#pragma unroll
        for (int r3 = 0; r3 < NPOS / 64; r3++)
            *(lds_f32*)(cR + (OFF_RB - OFF_RB % 256) + 4 * (Kn & 1) * NPOS + 4 * RROW * NWAVE * rr + 4 * 64 * r3) = st.v[rr][1 + r3];
    }
}

template <int NW>
__device__ __forceinline__ void stage_weights(int Kn, const float* __restrict__ lut, unsigned char* smem, int wave, int lane)
{
    Staged<NW> st;
    stage_issue<NW>(Kn, lut, smem, wave, lane, st);
    stage_commit<NW>(Kn, smem, wave, lane, st);
}

// LASTC kernels (FRESH) carry nothing that is a function of the lane number through the row loops: the lane number is taken
// afresh in every step (and once more at the mid-step commit) and the row loop's bases are read from the bases table, in ALL
// wavefronts of those kernels (one register file size serves every path): a handful of instructions per step and wavefront buy
// the registers the unit's sums need.
__device__ __forceinline__ int fresh_lane()
{
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=&v"(l));
    return l;
}
// The wavefront of the last-candidate units is the last one: plain, on another SIMD than wave 0 (waves w and w + 4 share one),
// and the one that stages a window row fewer than the others (rows w, w + NW, ... < 15), which pays for most of the unit.
template <int NW> constexpr int UWAVE = NW - 1;
// the sums of a lane's last-candidate unit; empty where there is none, so that the row loops of the other wavefronts carry nothing
// of it (their steps still take the lane-derived values afresh, see FRESH above)
template <bool ON> struct USums {};
template <> struct USums<true> { double num = 0.0, den = 0.0; };

// One step: window rows ky = 0..14 of tap column K - b for every active unit row b (BLO <= b <= BHI).
//   EDGE = false: the workgroup's windows never clamp at the right image border: one right gray per step (two with the
//                 wrapped units).
//   EDGE = true : per-diagonal sample columns (lc = min(x + kx - 7, W-1), rc = lc - d), computed once per step.
// Units with a < b (RIGHT: b < a) take their position from qrel2 / dbase2 (== qrel / dbase except in the threads of block
// j = 0, where they are the wrapped units of block 32).
// WRAPW: this wavefront holds the threads of block j = 0 (wave 0).  Elsewhere qrel2 == qrel and the second loads are skipped.
// LASTW: this wavefront also runs the 64 last-candidate units of the workgroup (see the header comment): lane -> pixel
// 4g + a, a = (lane >> 3) & 3, candidate NFIN, tap column K - a.
template <int NW, int K, bool EDGE, bool WRAPW, bool COMMIT, bool RIGHT, bool LASTW, bool FRESH>
__device__ __forceinline__ void run_step(unsigned char* smem, int g, int qrel, int qrel2, int xabs, int dbase, int dbase2,
                                         int W, int x0, int posmin, double (&num)[4][4], double (&den)[4][4], USums<LASTW>& us,
                                         int wave, int lane, const Staged<NW>& st)
{
    static_assert(!LASTW || (!EDGE && !WRAPW), "the last-candidate units live in a plain wavefront of an interior tile");
    XQ_CONSTS(NW)
    constexpr int BLO = K > KS - 1 ? K - (KS - 1) : 0;  // kx = K - b <= 14
    constexpr int BHI = K < 3 ? K : 3;                  // kx = K - b >= 0
    constexpr int DLO = 0 - BHI, DHI = 3 - BLO;         // diagonals a - b in use
    const uint32_t* sLd = reinterpret_cast<const uint32_t*>(smem + OFF_LB) + LGRAY;  // + ky * LROW
    const uint32_t* sRd = reinterpret_cast<const uint32_t*>(smem + OFF_RB) + RGRAY;  // + ky * RROW

    int iL[7], iR[7];
    if constexpr (EDGE) {
#pragma unroll
        for (int dl = DLO; dl <= DHI; dl++) {
            // clamped sample column of the fixed image, then the other image's column from THERE (M.cpp:1101-1106, 1129-1134);
            // the far clamp of that one (max(0, .) / min(W-1, .)) is the tile's
            const int lc = min(max(xabs + dl + K - HH, 0), W - 1);
            const int rc = RIGHT ? lc + ((dl > 0 ? dbase2 : dbase) - dl) : lc - ((dl < 0 ? dbase2 : dbase) + dl);
            iL[dl + 3] = min(max(lc - (x0 - HH), 0), LWC - 1);
            iR[dl + 3] = min(max(rc - (posmin - HH), 0), RWC - 1);
        }
    }
    // the row loop's LDS addresses: three per-lane bases (left block, right block, wrapped right block) that advance once per
    // loop body; everything else, the row within the body included, is an immediate offset.  The empty asm hides the bases'
    // relation from the loop optimiser, which otherwise rebuilds them from an SGPR row counter with one more add per row.
    typedef __attribute__((address_space(3))) const unsigned char lds_u8;
    lds_u8* bL = (lds_u8*)smem + OFF_LB + 16 * g;
    lds_u8* bR = (lds_u8*)smem + OFF_RB + 4 * qrel;
    lds_u8* bR2 = (lds_u8*)smem + OFF_RB + 4 * qrel2;
    // the last-candidate unit's three addresses (see the unit in the row): left weight, right weight, right gray
    lds_u8* uL = nullptr; lds_u8* uW = nullptr; lds_u8* uG = nullptr;
    if constexpr (FRESH) {
        static_assert(!EDGE, "interior tiles");
        // `lane` is this step's own (run_all_steps); the bases come from the table: wave 0's, 64 w bytes off for wavefront w
        const uint16_t* sBase = reinterpret_cast<const uint16_t*>(smem + OFF_BASE);
        const int oL = sBase[lane], oR = sBase[64 + lane] + (RIGHT ? 64 : -64) * wave;
        bL = (lds_u8*)smem + oL;
        bR = (lds_u8*)smem + oR;
        bR2 = WRAPW ? (lds_u8*)smem + sBase[128 + lane] : bR;
        g = (oL - OFF_LB) >> 4;
    }
    if constexpr (LASTW) {
        static_assert(FRESH, "g is this step's own");
        const int a = (lane >> 3) & 3;
        // non-negative modulus: columns -3..-1 are the slots the prologue zeroed, 15..17 hold older (finite) columns
        const int slot = a == 0 ? (K + RING) % RING : a == 1 ? (K - 1 + RING) % RING : a == 2 ? (K - 2 + RING) % RING : (K - 3 + RING) % RING;
        uL = (lds_u8*)smem + OFF_LB + 16 * g + 4 * a + 4 * PXW * slot;
        uW = (lds_u8*)smem + OFF_RB + 16 * g + (RIGHT ? 16 * NJ : 0) + 4 * a + 4 * (K & 1) * NPOS;
        uG = (lds_u8*)smem + OFF_RB + 16 * g + (RIGHT ? 16 * NJ : 0);
        asm("" : "+v"(uL), "+v"(uW), "+v"(uG));
    }
    uint32_t hi0[7];
#pragma unroll
    for (int i = 0; i < 7; i++) asm volatile("v_mov_b32 %0, 0" : "=v"(hi0[i]));  // seven distinct registers the compiler cannot fold
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef __attribute__((address_space(3))) const f32x4 lds_f32x4;
    typedef __attribute__((address_space(3))) const uint32_t lds_u32;
    typedef __attribute__((address_space(3))) const float lds_f32;

    if constexpr (EDGE) {
        // Border tiles, as they were: one row per loop body (UR = 1: the per-diagonal addresses leave no registers for more),
        // every read where it is used, and ONE fence per row, which keeps the next row's loads behind it: unfenced, the scheduler
        // hoists them and spills hundreds of registers.  The row is written out here and not built from the pieces of the
        // interior tiles below: these kernels spill already, and their machine code is held to what it was (tools/isa_same.py).
        static_assert(!COMMIT, "the border tiles stage in one piece in front of the step");
        constexpr int UR = 1;
        auto rows = [&](int ky0, int nbody) {
#pragma unroll 1
            for (int it = 0; it < nbody; it++) {
#pragma unroll
                for (int u = 0; u < UR; u++) {
                    lds_u8* rL = bL + u * 4 * LROW;
                    lds_u8* rR = bR + u * 4 * RROW;
                    lds_u8* rR2 = bR2 + u * 4 * RROW;
                    double c[7];  // cost samples of the diagonals, scaled domain: |gL - gR| * 2^-1074
                    const int ky = ky0 + it * UR + u;
#pragma unroll
                    for (int dl = DLO; dl <= DHI; dl++) c[dl + 3] = cost_sample(sLd[ky * LROW + iL[dl + 3]], sRd[ky * RROW + iR[dl + 3]], hi0[dl + 3]);
                    const f32x4 wr4 = *(lds_f32x4*)(rR + 4 * (K & 1) * NPOS);
                    // the right weights as the two register pairs the packed multiplies broadcast from (op_sel picks either half of a
                    // pair).  The upper pair is made opaque: the compiler otherwise copies element 3 into the low half of a fresh pair,
                    // one v_mov per row.
                    f32x2 wrp[2] = {{wr4.x, wr4.y}, {wr4.z, wr4.w}};
                    asm("" : "+v"(wrp[1]));
                    f32x2 wr2p[2] = {wrp[0], wrp[1]};
                    if constexpr (RIGHT ? BLO <= 2 : BHI >= 1) {  // some active unit is a wrapped one
                        const f32x4 w2 = *(lds_f32x4*)(rR2 + 4 * (K & 1) * NPOS);
                        wr2p[0] = f32x2{w2.x, w2.y};
                        wr2p[1] = f32x2{w2.z, w2.w};
                        asm("" : "+v"(wr2p[1]));
                    }
#pragma unroll
                    for (int b = BLO; b <= BHI; b++) {
                        const f32x4 wl4 = *(lds_f32x4*)(rL + 4 * ((K - b) % RING) * PXW);
                        float ab[4];  // (see `block` below)
#pragma unroll
                        for (int a = 0; a < 4; a += 2) {
                            const f32x2 wl2 = {wl4[a], wl4[a + 1]};
                            const bool w0 = RIGHT ? b < a : a < b, w1 = RIGHT ? b < a + 1 : a + 1 < b;  // wrapped units
                            const f32x2 s0 = (w0 ? wr2p : wrp)[b >> 1], s1 = (w1 ? wr2p : wrp)[b >> 1];
                            f32x2 wrb;
                            if (w0 == w1) wrb = (b & 1) ? __builtin_shufflevector(s0, s0, 1, 1) : __builtin_shufflevector(s0, s0, 0, 0);
                            else wrb = f32x2{s0[b & 1], s1[b & 1]};
                            const f32x2 pr = wl2 * wrb;
                            ab[a] = pr.x; ab[a + 1] = pr.y;
                        }
#pragma unroll
                        for (int a = 0; a < 4; a++) {
                            const double abd = (double)ab[a];
                            num[a][b] = __builtin_fma(abd, c[a - b + 3], num[a][b]);  // exact product: == num + ab*c (x 2^-954)
                            den[a][b] = den[a][b] + abd;                              // M.cpp:1107-1108 (x 2^120)
                        }
                    }
                    // the fence: the row's sums are complete here (the arithmetic has no side effect the barrier alone would order)
                    // and no LDS read crosses
#pragma unroll
                    for (int b = BLO; b <= BHI; b++)
                        asm volatile("" :: "v"(num[0][b]), "v"(num[1][b]), "v"(num[2][b]), "v"(num[3][b]),
                                           "v"(den[0][b]), "v"(den[1][b]), "v"(den[2][b]), "v"(den[3][b]) : "memory");
                    __builtin_amdgcn_sched_barrier(0);
                }
                bL += UR * 4 * LROW;
                bR += UR * 4 * RROW;
                asm("" : "+v"(bL), "+v"(bR));
                bR2 += UR * 4 * RROW;
                asm("" : "+v"(bR2));
            }
        };
        rows(0, KS / UR);
    } else {
        // Interior tiles: URI rows per loop body -- the row strides fold into the offset fields (URI rows of the right stride plus
        // the largest in-row offset stay far below 16 bits), so the bases advance once per body -- and the LDS reads of a row are
        // issued ahead of their use as far as the registers of the wavefront's class allow (PF_HEAD / PF_WLEAD at the top of the
        // file).  A row's sums are fenced per b-block (the empty asm on the block's eight sums with a memory clobber, then
        // sched_barrier): no read crosses a fence, so a read written in front of a block's fence is issued in front of that block's
        // arithmetic or among it, and one written a block earlier has at least that block's 14 VALU instructions between its issue
        // and its use.  The waits are the compiler's (s_waitcnt lgkmcnt(n), the younger reads left in flight):
        //   head   what a row needs in front of its first block -- right gray, left gray quads, right weights, the left weights of
        //          block BLO, wave 0's second right gray and weights.  The parts the class prefetches are read at the start of the
        //          PREVIOUS row's last block and carried across the rows of a body, across the loop's back edge and across the
        //          mid-step commit; the others are read at the head of the row, where all of them used to be.
        //   wl     the left weights of block b + WLEAD are read at the start of block b: the quads rotate.
        //   unit   the three words of the last-candidate unit are read at the head of the row and used behind its second block.
        // Boundaries.  The mid-step commit stages step K + 1: it writes ring slot (K + 1) % 5 and right buffer (K + 1) & 1.  The
        // head reads the gray tiles (never written after the prologue), right buffer K & 1 and ring slot (K - BLO) % 5; the
        // slots a step reads are those of columns K - 3 .. K, and K + 1 == K - 4 (mod 5) is none of them: the head of row CROW,
        // read in front of the commit, is still the right one behind it.  The head read by a step's last row is row KS's: it
        // lies one row stride past the blocks, inside smem (static_assert below), and nothing consumes it -- nothing is carried
        // across the step's barrier, and the step's first row waits for its head in full.
        constexpr int E0 = (K + DLO) & ~3, NQ = (K + DHI - E0 + 4) / 4;
        static_assert(E0 >= 0 && E0 + 4 * NQ + 4 * 15 <= LWP, "the quads stay inside a tile row");
        static_assert(DLO <= 0 && DHI >= 0, "diagonal 0 is in use in every step");
        static_assert(OFF_RB + (KS + 1) * RROW * 4 <= LDS_TOTAL, "the head of row KS is read inside smem");
        constexpr bool W2G = WRAPW && (RIGHT ? DHI > 0 : DLO < 0);   // some active diagonal belongs to wrapped units
        constexpr bool W2W = WRAPW && (RIGHT ? BLO <= 2 : BHI >= 1);  // some active unit is a wrapped one
        constexpr int CLS = NW != 8 ? 0 : !FRESH ? 2 : (WRAPW || LASTW) ? 1 : 0;
        constexpr int WLEAD = PF_WLEAD[CLS];
        constexpr int PF_PRE = PF_HEAD[CLS][COMMIT ? 0 : 1], PF_POST = PF_HEAD[CLS][1];  // (the last step has one loop only)
        // One b-block of a row: the four units (a, b) of unit row b.  wl4: the left weights of tap column K - b; wrp / wr2p: the
        // right weights (and the wrapped units') as the two register pairs the packed multiplies broadcast from (op_sel picks
        // either half of a pair).
        auto block = [&](int b, const f32x4 wl4, const double (&c)[7], const f32x2 (&wrp)[2], const f32x2 (&wr2p)[2])
                         __attribute__((always_inline)) {
            // the f32 products (M.cpp:1104-1105, x 2^120) written as the two packed multiplies they are issued as: pixels
            // (a, a + 1) times the position's weight broadcast -- left to the vectoriser, the unrolled body pairs units
            // across b and assembles the pairs with moves
            float ab[4];
#pragma unroll
            for (int a = 0; a < 4; a += 2) {
                const f32x2 wl2 = {wl4[a], wl4[a + 1]};
                const bool w0 = RIGHT ? b < a : a < b, w1 = RIGHT ? b < a + 1 : a + 1 < b;  // wrapped units
                const f32x2 s0 = (w0 ? wr2p : wrp)[b >> 1], s1 = (w1 ? wr2p : wrp)[b >> 1];
                f32x2 wrb;
                if (w0 == w1) wrb = (b & 1) ? __builtin_shufflevector(s0, s0, 1, 1) : __builtin_shufflevector(s0, s0, 0, 0);
                else wrb = f32x2{s0[b & 1], s1[b & 1]};
                const f32x2 pr = wl2 * wrb;
                ab[a] = pr.x; ab[a + 1] = pr.y;
            }
#pragma unroll
            for (int a = 0; a < 4; a++) {
                const double abd = (double)ab[a];
                num[a][b] = __builtin_fma(abd, c[a - b + 3], num[a][b]);  // exact product: == num + ab*c (x 2^-954)
                den[a][b] = den[a][b] + abd;                              // M.cpp:1107-1108 (x 2^120)
            }
        };
        // the right weights as register pairs.  The upper pair is made opaque: the compiler otherwise copies element 3 into the
        // low half of a fresh pair, one v_mov per row.
        auto pairs = [](const f32x4 w, f32x2 (&p)[2]) __attribute__((always_inline)) {
            p[0] = f32x2{w.x, w.y};
            p[1] = f32x2{w.z, w.w};
            asm("" : "+v"(p[1]));
        };
        struct Head {
            uint32_t gr, gr2;  // right gray: tile column of Q + K - 7 (and the wrapped units')
            u32x4 gl[NQ];      // left grays of the step's diagonals
            f32x4 wr, wr2, wl;
        };
        // read the parts `pf` of the head of row u of the body (u = URI: the next body's first) into h
        auto load_head = [&](int u, auto pf, Head h) __attribute__((always_inline)) {
            constexpr int PF = decltype(pf)::value;
            lds_u8* rL = bL + u * 4 * LROW;
            lds_u8* rR = bR + u * 4 * RROW;
            lds_u8* rR2 = bR2 + u * 4 * RROW;
            if constexpr (PF & PF_GRAY) {
                h.gr = *(lds_u32*)(rR + 4 * (RGRAY + K));
                h.gr2 = h.gr;
                if constexpr (W2G) h.gr2 = *(lds_u32*)(rR2 + 4 * (RGRAY + K));
                // the left grays, read as 16-byte aligned quads from a tile column that is a multiple of four (4g, LWP and E0
                // are): a run the compiler cannot prove aligned is split into narrower reads (ds_read2_*), which cost several
                // times the LDS cycles of ds_read_b128
                const __attribute__((address_space(3))) u32x4* pl4 = (const __attribute__((address_space(3))) u32x4*)(rL + 4 * (LGRAY + E0));
#pragma unroll
                for (int i = 0; i < NQ; i++) h.gl[i] = pl4[i];
            }
            if constexpr (PF & PF_WR) {
                h.wr = *(lds_f32x4*)(rR + 4 * (K & 1) * NPOS);
                h.wr2 = h.wr;
                if constexpr (W2W) h.wr2 = *(lds_f32x4*)(rR2 + 4 * (K & 1) * NPOS);
            }
            if constexpr (PF & PF_WL) h.wl = *(lds_f32x4*)(rL + 4 * ((K - BLO) % RING) * PXW);
            return h;
        };
        Head h = load_head(0, std::integral_constant<int, PF_PRE>{}, Head{});
        auto rows = [&](int nbody, auto pf) {
            constexpr int PF = decltype(pf)::value;
#pragma unroll 1
            for (int it = 0; it < nbody; it++) {
#pragma unroll
                for (int u = 0; u < URI; u++) {
                    lds_u8* rL = bL + u * 4 * LROW;
                    const Head cur = load_head(u, std::integral_constant<int, PF_ALL & ~PF>{}, h);  // what was not prefetched
                    f32x4 wl[4];
                    wl[BLO] = cur.wl;
#pragma unroll
                    for (int b = BLO + 1; b < BLO + WLEAD && b <= BHI; b++) wl[b] = *(lds_f32x4*)(rL + 4 * ((K - b) % RING) * PXW);
                    // lane -> pixel 4g + a, a = (lane >> 3) & 3, candidate NFIN: position 4g + a (+ 4 NJ), unit row b = a, tap column
                    // K - a; the grays are the tile columns 4g + K (left: the diagonal-0 sample of the row's own quads) and
                    // 4g + K (+ 4 NJ) (right): the skew a cancels in both
                    float wlU = 0.0f, wrU = 0.0f;
                    uint32_t grU = 0;
                    if constexpr (LASTW) {
                        wlU = *(lds_f32*)(uL + u * 4 * LROW);
                        wrU = *(lds_f32*)(uW + u * 4 * RROW);
                        grU = *(lds_u32*)(uG + u * 4 * RROW + 4 * (RGRAY + K));
                    }
                    double c[7];  // cost samples of the diagonals, scaled domain: |gL - gR| * 2^-1074
                    uint32_t glv[4 * NQ];
#pragma unroll
                    for (int i = 0; i < NQ; i++) {
                        u32x4 t = cur.gl[i];
                        asm("" : "+v"(t));  // all four words in use: otherwise the compiler narrows a quad whose first word no diagonal
                                            // needs into a misaligned 12-byte read and splits that into ds_read2_b32 + ds_read_b32
                        glv[4 * i] = t.x; glv[4 * i + 1] = t.y; glv[4 * i + 2] = t.z; glv[4 * i + 3] = t.w;
                    }
#pragma unroll
                    for (int dl = DLO; dl <= DHI; dl++) c[dl + 3] = cost_sample(glv[K + dl - E0], (RIGHT ? dl > 0 : dl < 0) ? cur.gr2 : cur.gr, hi0[dl + 3]);
                    f32x2 wrp[2], wr2p[2];
                    pairs(cur.wr, wrp);
                    wr2p[0] = wrp[0]; wr2p[1] = wrp[1];
                    if constexpr (W2W) pairs(cur.wr2, wr2p);
#pragma unroll
                    for (int b = BLO; b <= BHI; b++) {
                        if (b + WLEAD <= BHI) wl[b + WLEAD] = *(lds_f32x4*)(rL + 4 * ((K - b - WLEAD) % RING) * PXW);
                        if (b == BHI) h = load_head(u + 1, std::integral_constant<int, PF>{}, Head{});  // (before the bases advance)
                        block(b, wl[b], c, wrp, wr2p);
                        if constexpr (LASTW) if (b == (BLO < BHI ? BLO + 1 : BLO)) {
                            // inactive lane-steps (K - a outside 0..14): wrU is the all-zero class and wlU is finite (a zeroed slot or an
                            // older column), so ab = +0: fma(+0, c, num) = num + (+0) = num (c >= 0 is finite; num is +0 or positive, so
                            // the sum keeps its sign) and den + (+0) = den, in the scaled domain as in the plain one
                            const double abU = (double)(wlU * wrU);
                            us.num = __builtin_fma(abU, cost_sample(glv[K - E0], grU, hi0[3]), us.num);
                            us.den = us.den + abU;
                            asm volatile("" :: "v"(us.num), "v"(us.den));
                        }
                        asm volatile("" :: "v"(num[0][b]), "v"(num[1][b]), "v"(num[2][b]), "v"(num[3][b]),
                                           "v"(den[0][b]), "v"(den[1][b]), "v"(den[2][b]), "v"(den[3][b]) : "memory");
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                bL += URI * 4 * LROW;
                bR += URI * 4 * RROW;
                asm("" : "+v"(bL), "+v"(bR));
                if constexpr (WRAPW) {
                    bR2 += URI * 4 * RROW;
                    asm("" : "+v"(bR2));
                }
                if constexpr (LASTW) {
                    uL += URI * 4 * LROW;
                    uW += URI * 4 * RROW;
                    uG += URI * 4 * RROW;
                    asm("" : "+v"(uL), "+v"(uW), "+v"(uG));
                }
            }
        };
        if constexpr (COMMIT) {
            // the gathers issued before this loop have landed after CROW rows
            rows(CROW / URI, std::integral_constant<int, PF_PRE>{});
            stage_commit<NW>(K + 1, smem, wave, FRESH ? fresh_lane() : lane, st);
            h = load_head(0, std::integral_constant<int, PF_POST & ~PF_PRE>{}, h);  // what the second loop carries and the first did not
            rows((KS - CROW) / URI, std::integral_constant<int, PF_POST>{});
        } else {
            rows(KS / URI, std::integral_constant<int, PF_PRE>{});
        }
    }
}

template <int NW, bool EDGE, bool WRAPW, bool RIGHT, bool LASTW = false, bool FRESH = false>
__device__ __forceinline__ void run_all_steps(unsigned char* smem, const float* __restrict__ lut, int wave, int lane,
                                              int g, int qrel, int qrel2, int xabs, int dbase, int dbase2,
                                              int W, int x0, int posmin, double (&num)[4][4], double (&den)[4][4], USums<LASTW>& us)
{
    Staged<NW> st;
#define ASW_XQ_STEP(KK)                                                                                        \
    if constexpr (FRESH) lane = fresh_lane();  /* once for the staging and the row loop's bases */              \
    if ((KK) + 1 < NSTEP) {                                                                                      \
        if constexpr (EDGE) stage_weights<NW>((KK) + 1, lut, smem, wave, lane);  /* border tiles: registers are scarcer there */ \
        else stage_issue<NW>((KK) + 1, lut, smem, wave, lane, st);                             \
    }                                                                                                           \
    run_step<NW, (KK), EDGE, WRAPW, (!EDGE && (KK) + 1 < NSTEP), RIGHT, LASTW, FRESH>(smem, g, qrel, qrel2, xabs, dbase, dbase2, W, x0, \
                                                                           posmin, num, den, us, wave, lane, st); \
    __syncthreads();
    ASW_XQ_STEP(0) ASW_XQ_STEP(1) ASW_XQ_STEP(2) ASW_XQ_STEP(3) ASW_XQ_STEP(4) ASW_XQ_STEP(5)
    ASW_XQ_STEP(6) ASW_XQ_STEP(7) ASW_XQ_STEP(8) ASW_XQ_STEP(9) ASW_XQ_STEP(10) ASW_XQ_STEP(11)
    ASW_XQ_STEP(12) ASW_XQ_STEP(13) ASW_XQ_STEP(14) ASW_XQ_STEP(15) ASW_XQ_STEP(16) ASW_XQ_STEP(17)
#undef ASW_XQ_STEP
}

// grid (tiles of this launch, H), 512 threads.  gL / gR: gray planes [H][W].  vol (optional): [>= NFIN][H][W] (LASTC: NFIN + 1).
// bestE / bestD: [H][W] running minimum over candidates [0, NFIN) (strict '<' in ascending d, M.cpp:1145-1150) for the tail
// launch to resume from; disp (when there is no tail): the disparity itself.
// LASTC (interior tiles only): the workgroup finishes candidates [0, NFIN]: vol has NFIN + 1 planes and disp is written.
template <int NW, bool EDGE, bool RIGHT, bool LASTC = false>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(NW == 8 ? 4 : 3, NW == 8 ? 4 : 3))) void k_asw_bilateral_xq(
    XqParams p, const uint8_t* __restrict__ gL, const uint8_t* __restrict__ gR, const int4* __restrict__ cells,
    const float* __restrict__ lut, float* __restrict__ vol, double* __restrict__ bestE, float* __restrict__ bestD,
    float* __restrict__ disp)
{
    // static: the LDS base is then a compile-time 0 and folds into the instructions' offset fields (with the dynamic-LDS
    // symbol every address in the step loop carried its own "v_add_u32 v, <base>, v": 6 of 78 VALU instructions)
    XQ_CONSTS(NW)
    static_assert(!(EDGE && LASTC), "the border tiles cannot host the last-candidate units");
    __shared__ __align__(16) unsigned char smem[LDS_TOTAL];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H = p.H, W = p.W;
    const int x0 = (p.tile0 + blockIdx.x) * PXW, y = blockIdx.y;
    const int posmin = RIGHT ? x0 + p.minD : x0 - p.minD - 4 * NJ;  // == Q (mod 4) either way

    // ---- gray tiles, replicate-clamped (M.cpp:1059-1060, 1101-1106), as bytes (weight staging) and as u32 (cost samples)
    {
        uint8_t* sL8 = smem + OFF_L8;
        uint8_t* sR8 = smem + OFF_R8;
        uint32_t* sLd = reinterpret_cast<uint32_t*>(smem + OFF_LB) + Cfg::LGRAY;
        uint32_t* sRd = reinterpret_cast<uint32_t*>(smem + OFF_RB) + Cfg::RGRAY;
        // wavefront -> window rows r = wave + NWAVE rr, lane -> tile columns lane + 64 k (no division), and every global load of
        // the thread -- its gray bytes and its cells of the table -- is issued before its first LDS store: one memory round trip
        // at the head of the workgroup's life.  Every address is clamped into the image, so the lanes and rows past the tile
        // load too (a byte they do not store).
        constexpr int NCL = (LWC + 63) / 64, NCR = (RWC + 63) / 64, NCI = (NCELLCOL * KS + NTHR - 1) / NTHR;
        uint32_t vL[NROWS][NCL], vR[NROWS][NCR];
        int4 ci[NCI];
#pragma unroll
        for (int k = 0; k < NCI; k++) ci[k] = cells[min(tid + NTHR * k, NCELLCOL * KS - 1)];
#pragma unroll
        for (int rr = 0; rr < NROWS; rr++) {
            const int yy = min(max(y - HH + wave + NWAVE * rr, 0), H - 1);  // wave-uniform
            const uint8_t* rowL = gL + (size_t)yy * W;
            const uint8_t* rowR = gR + (size_t)yy * W;
#pragma unroll
            for (int k = 0; k < NCL; k++) vL[rr][k] = rowL[min(max(x0 - HH + lane + 64 * k, 0), W - 1)];
#pragma unroll
            for (int k = 0; k < NCR; k++) vR[rr][k] = rowR[min(max(posmin - HH + lane + 64 * k, 0), W - 1)];
        }
#pragma unroll
        for (int rr = 0; rr < NROWS; rr++) {
            const int r = wave + NWAVE * rr;
            if (r >= KS) break;  // wave-uniform
#pragma unroll
            for (int k = 0; k < NCL; k++) {
                const int c = lane + 64 * k;
                if (c < LWC) {
                    sL8[r * LW8 + c] = (uint8_t)vL[rr][k];
                    sLd[r * Cfg::LROW + c] = vL[rr][k];
                }
            }
#pragma unroll
            for (int k = 0; k < NCR; k++) {
                const int c = lane + 64 * k;
                if (c < RWC) {
                    sR8[r * RW8 + c] = (uint8_t)vR[rr][k];
                    sRd[r * Cfg::RROW + c] = vR[rr][k];
                }
            }
            if constexpr (LASTC) {
                // ring slots 2..4 stand for tap columns -3..-1 until columns 2..4 are staged (steps 1..3): the last-candidate units
                // of lanes with a > K read them in steps 0..2 and must find a finite weight there
                float* sWL = reinterpret_cast<float*>(smem + OFF_LB);
#pragma unroll
                for (int k = 0; k < 3; k++) sWL[r * Cfg::LROW + 2 * PXW + lane + 64 * k] = 0.0f;
            }
        }
        // ---- the step tables (see stage_issue)
        uint32_t* sCell = reinterpret_cast<uint32_t*>(smem + OFF_CELL);
#pragma unroll
        for (int k = 0; k < NCI; k++)
            if (tid + NTHR * k < NCELLCOL * KS) sCell[tid + NTHR * k] = cell_entry(ci[k].x, ci[k].y, ci[k].z, RW8);
        if (tid < 64) {  // wave 0: tid is the lane number
            // positions are clamped into the image before the weight is looked up: max(0, x - d) / min(W-1, x + d) (the other
            // bound only matters for the lanes of a partial tile, whose results are discarded)
            const int pclamp_lo = min(max(0 - posmin, 0), NPOS - 1), pclamp_hi = min(max(W - 1 - posmin, 0), NPOS - 1);
            static_assert(NPOS <= 256 && 4 * KS * 3 < 256, "a clamped position and a skew fit a byte");
            uint8_t* sLane = smem + OFF_LANE;
#pragma unroll
            for (int r3 = 0; r3 < NPOS / 64; r3++) sLane[64 * r3 + tid] = (uint8_t)min(max(tid + 64 * r3, pclamp_lo), pclamp_hi);
            sLane[64 * 3 + tid] = (uint8_t)(4 * KS * (tid & 3));
            if constexpr (LASTC) {  // the bases of wave 0's lanes (run_step derives the other wavefronts' from them)
                const int g0 = (tid & 7) | ((tid >> 2) & 8), j0 = (tid >> 3) & 3;
                const int q0 = RIGHT ? 4 * g0 + 4 * j0 : 4 * g0 + 4 * (NJ - j0);
                const int q2 = j0 == 0 ? (RIGHT ? 4 * g0 + 4 * NJ : 4 * g0) : q0;
                uint16_t* sBase = reinterpret_cast<uint16_t*>(smem + OFF_BASE);
                sBase[tid] = (uint16_t)(OFF_LB + 16 * g0);
                sBase[64 + tid] = (uint16_t)(OFF_RB + 4 * q0);
                sBase[128 + tid] = (uint16_t)(OFF_RB + 4 * q2);
            }
        }
    }
    __syncthreads();

    // lane -> (pixel group g, position block jl): g's low three bits from the lane's low three bits and its bit 3 from lane bit
    // 5, so that the sixteen lanes one ds_read_b128 services together hold eight distinct g's (the f64 gray reads are 32 B
    // apart per g: g and g + 8 share a bank; measured: 2.9e9 -> 0.9e9 conflict cycles per frame; kept for the u32 gray quads and
    // the 16-byte weight reads, which are 16 B apart per g)
    const int g = (lane & 7) | ((lane >> 2) & 8);
    const int jl = 4 * wave + ((lane >> 3) & 3);
    // Q - posmin; LEFT: Q = x0 + 4g - minD - 4 jl, RIGHT: Q = x0 + 4g + minD + 4 jl
    const int qrel = RIGHT ? 4 * g + 4 * jl : 4 * g + 4 * (NJ - jl);
    // block 32's positions for the wrapped units of block 0
    const int qrel2 = jl == 0 ? (RIGHT ? 4 * g + 4 * NJ : 4 * g) : qrel;
    const int xabs = x0 + 4 * g;                           // X
    const int dbase = p.minD + 4 * jl;                     // d of the diagonal a == b
    const int dbase2 = jl == 0 ? p.minD + 4 * NJ : dbase;

    double num[4][4], den[4][4];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) { num[a][b] = 0.0; den[a][b] = 0.0; }

    USums<LASTC> us;  // the last-candidate unit of this lane (LASTC, wave UWAVE)
    USums<false> none;
    stage_weights<NW>(0, lut, smem, wave, lane);
    __syncthreads();
    // wave 0 holds the threads of block j = 0 (the wrapped units): its steps load the second right weights / gray; ONE branch
    // around the whole step sequence (a branch per step made the register allocator spill 488 VGPRs)
    if (EDGE || wave == 0)
        run_all_steps<NW, EDGE, true, RIGHT, false, LASTC>(smem, lut, wave, lane, g, qrel, qrel2, xabs, dbase, dbase2, W,
                                                           x0, posmin, num, den, none);
    else if (LASTC && wave == UWAVE<NW>)  // (the wave number as a constant: the staging rows this wavefront does not have fold away)
        run_all_steps<NW, EDGE, false, RIGHT, LASTC, LASTC>(smem, lut, UWAVE<NW>, lane, g, qrel, qrel2, xabs, dbase, dbase2, W,
                                                            x0, posmin, num, den, us);
    else
        run_all_steps<NW, EDGE, false, RIGHT, false, LASTC>(smem, lut, wave, lane, g, qrel, qrel2, xabs, dbase, dbase2, W,
                                                            x0, posmin, num, den, none);
    // (the last step ended with a barrier: the tiles are dead)

    // ---- E = num / den (M.cpp:1111) -> LDS [candidate][pixel]; back from the scaled domain first (both ldexp are exact)
    // (g and jl are taken from the lane number afresh: carried through the steps for this use they cost two of the 128 registers)
    int le = lane;
    asm volatile("" : "+v"(le));
    const int ge = (le & 7) | ((le >> 2) & 8), jle = 4 * wave + ((le >> 3) & 3);
    const int cb = 4 * jle, cb2 = jle == 0 ? 4 * NJ : cb;  // dbase - minD, dbase2 - minD
    double* sE = reinterpret_cast<double*>(smem + OFF_E64);
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int c = RIGHT ? (b < a ? cb2 : cb) + b - a : (a < b ? cb2 : cb) + a - b;  // in [0, 128) for every unit
            sE[c * PXW + 4 * ge + a] = __builtin_ldexp(num[a][b], 954) / __builtin_ldexp(den[a][b], -120);
        }
    if constexpr (LASTC)
        if (wave == UWAVE<NW>) sE[NFIN * PXW + 4 * ge + ((le >> 3) & 3)] = __builtin_ldexp(us.num, 954) / __builtin_ldexp(us.den, -120);
    __syncthreads();
    // ---- WTA (strict '<' while d ascends) and volume: thread -> (pixel, 16 consecutive candidates)
    const int px = lane, part = wave;
    const int x = x0 + px;
    double be = 1.7976931348623157e308;  // numeric_limits<double>::max(), M.cpp:1037
    float bd = 0.0f;
    if (x < W) {
        for (int c = 16 * part; c < 16 * part + 16; c++) {
            const double E = sE[c * PXW + px];
            if (vol) vol[((size_t)c * H + y) * W + x] = (float)E;
            if (E < be) { be = E; bd = (float)(p.minD + c); }
        }
    }
    double* sPE = reinterpret_cast<double*>(smem + OFF_PART);
    float* sPD = reinterpret_cast<float*>(smem + OFF_PART + NWAVE * PXW * 8);
    sPE[part * PXW + px] = be;
    sPD[part * PXW + px] = bd;
    __syncthreads();
    if (wave == 0 && x < W) {  // tid == px there: nothing but the lane number has to outlive the steps
        double e = 1.7976931348623157e308;
        float d = 0.0f;
#pragma unroll
        for (int q = 0; q < NWAVE; q++) {
            const double eq = sPE[q * PXW + px];
            if (eq < e) { e = eq; d = sPD[q * PXW + px]; }
        }
        if constexpr (LASTC) {  // candidate NFIN enters last, with the same strict '<': still the first minimum in ascending d
            const double eq = sE[NFIN * PXW + px];
            if (vol) vol[((size_t)NFIN * H + y) * W + x] = (float)eq;
            if (eq < e) { e = eq; d = (float)(p.minD + NFIN); }
        }
        if (LASTC || disp) {
            disp[(size_t)y * W + x] = d;
        } else {
            bestE[(size_t)y * W + x] = e;
            bestD[(size_t)y * W + x] = d;
        }
    }
}

}  // namespace

int bilateral_xq_candidates(int nwave) { return 16 * nwave; }

// The scaled domain of the kernel is exact when every nonzero product of two LUT entries is >= 2^-68 (then every f32 product
// is normal in both domains and every nonzero ab * c * 2^-954 >= 2^-1022) and when the scaled products stay finite:
// (max * 2^60)^2 < 2^128.  At the reference's gammas (30, 20) the smallest product is about 2^-23.
bool bilateral_xq_lut_ok(const float* lut, size_t n)
{
    double mn = 0, mx = 0;
    for (size_t i = 0; i < n; i++) {
        const double v = lut[i];
        if (!(v >= 0)) return false;  // weights are exp() values: never negative or NaN
        if (v > 0 && (mn == 0 || v < mn)) mn = v;
        if (v > mx) mx = v;
    }
    return mn * mn >= std::ldexp(1.0, -68) && mx * mx < std::ldexp(1.0, 128 - 2 * XQ_LUT_SCALE_LOG2 - 1);
}

namespace {
template <int NW>
int launch_xq_t(hipStream_t s, hipStream_t s_border, const uint8_t* gL, const uint8_t* gR, int H, int W, int minD, const int4* cells,
                const float* lut, float* vol, double* bestE, float* bestD, float* disp, bool right, bool last)
{
    // last: the interior launch finishes candidate NFIN as well and writes disp and plane NFIN of vol for its columns; the border
    // tiles write bestE / bestD (the caller runs candidate NFIN and the merge over their columns)
    const int ntiles = (W + PXW - 1) / PXW;
    const dim3 blk(64 * NW);
    if (right) {
        // border tile = the first of a row (windows of x < 7 clamp at column 0); the clamped positions' weight neighbours
        // (columns W-8 .. W-1) must lie in the last tile's right-gray tile: x0_last + minD <= W - 1
        if ((ntiles - 1) * PXW + minD > W - 1) return ASW_ERR_BAD_ARGUMENT;
        XqParams pe{H, W, minD, 0};
        ASW_TRY(ASW_LAUNCH((k_asw_bilateral_xq<NW, true, true>), dim3(1, H), blk, 0, s_border, pe, gL, gR, cells, lut, vol,
                           bestE, bestD, last ? nullptr : disp));
        if (ntiles > 1) {
            XqParams pi{H, W, minD, 1};
            if (last)
                ASW_TRY(ASW_LAUNCH((k_asw_bilateral_xq<NW, false, true, true>), dim3(ntiles - 1, H), blk, 0, s, pi, gL, gR, cells,
                                   lut, vol, bestE, bestD, disp));
            else
                ASW_TRY(ASW_LAUNCH((k_asw_bilateral_xq<NW, false, true>), dim3(ntiles - 1, H), blk, 0, s, pi, gL, gR, cells, lut,
                                   vol, bestE, bestD, disp));
        }
        return ASW_OK;
    }
    // tiles whose windows (of in-image pixels) stay left of the right border: x0 + 63 + 7 <= W - 1
    const int n_int = W >= PXW + HH ? std::min(ntiles, (W - PXW - HH) / PXW + 1) : 0;
    auto ki = k_asw_bilateral_xq<NW, false, false>;
    auto ke = k_asw_bilateral_xq<NW, true, false>;
    if (n_int > 0) {
        XqParams p{H, W, minD, 0};
        if (last)
            ASW_TRY(ASW_LAUNCH((k_asw_bilateral_xq<NW, false, false, true>), dim3(n_int, H), blk, 0, s, p, gL, gR, cells, lut, vol,
                               bestE, bestD, disp));
        else
            ASW_TRY(ASW_LAUNCH(ki, dim3(n_int, H), blk, 0, s, p, gL, gR, cells, lut, vol, bestE, bestD, disp));
    }
    if (ntiles > n_int) {
        XqParams p{H, W, minD, n_int};
        ASW_TRY(ASW_LAUNCH(ke, dim3(ntiles - n_int, H), blk, 0, s_border, p, gL, gR, cells, lut, vol, bestE, bestD,
                           last ? nullptr : disp));
    }
    return ASW_OK;
}
}  // namespace

// nwave: 8 = candidates [0, 128), 4 = candidates [0, 64).
// cells: int4[21 * 15] {dxw, dyw, class * 256, -} per window cell, kx = -3..17; lut: float[ncls][256] with an all-zero class,
// scaled by 2^XQ_LUT_SCALE_LOG2, from an unscaled LUT that bilateral_xq_lut_ok accepts.
// disp != nullptr: the launch covers the whole candidate range: write the disparity; else bestE / bestD.
// s_border: stream of the border-tile launch (may equal s; a side stream lets the 1/30 of the tiles overlap the main launch)
// right: DISPARITY_RIGHT -- gL is then the fixed (right) image's gray plane and gR the left image's.
// last: the candidate range is [0, 16 nwave] exactly and bilateral_xq_interior_columns() is not empty: the interior tiles finish
// it (vol gets plane 16 nwave, disp is written, both for the interior columns only); the border tiles write bestE / bestD.
int launch_bilateral_xq(hipStream_t s, hipStream_t s_border, int nwave, const uint8_t* gL, const uint8_t* gR, int H, int W, int minD,
                        const int4* cells, const float* lut, float* vol, double* bestE, float* bestD, float* disp, bool right, bool last)
{
    if (last && !disp) return ASW_ERR_BAD_ARGUMENT;
    if (nwave == 8) return launch_xq_t<8>(s, s_border, gL, gR, H, W, minD, cells, lut, vol, bestE, bestD, disp, right, last);
    if (nwave == 4) return launch_xq_t<4>(s, s_border, gL, gR, H, W, minD, cells, lut, vol, bestE, bestD, disp, right, last);
    return ASW_ERR_BAD_ARGUMENT;
}

// Image columns [*lo, *hi) of the interior tiles (the rest are the border tiles'); empty when there is no interior tile.
void bilateral_xq_interior_columns(int W, bool right, int* lo, int* hi)
{
    const int ntiles = (W + PXW - 1) / PXW;
    if (right) {
        *lo = ntiles > 1 ? PXW : W; *hi = W;
    } else {
        const int n_int = W >= PXW + HH ? std::min(ntiles, (W - PXW - HH) / PXW + 1) : 0;
        *lo = 0; *hi = std::min(W, n_int * PXW);
    }
}
