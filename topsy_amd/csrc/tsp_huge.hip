// tsp_huge.hip -- kernel H2 of the splat pipeline, gfx950: the footprints of 64 px and up that kernel S defers (tsp_pipeline.hip),
// with its band bins, the non-finite-weight pass and its launchers.  (The mid footprints: tsp_mid.hip.)
//
// What it computes is fragment_* + additive blend of the reference (src/topsy/shaders/sph.wgsl:139-165, sampler
// src/topsy/sph.py:425-426) in the arithmetic of tsp_math.h; the records it consumes (pixel-space centre, width, weights) are
// written by kernel S.  A wave owns a strip of the image, its accumulators sit in registers:
//   kernel H2  splat_huge2_kernel          row-uniform gather: every footprint >= 64 px (bilinear on mip 0), every mode
//   + the binning pass huge_band_fill_kernel and huge_nonfinite_kernel
// (Rounds 1-4 also carried the per-pixel gather kernel H, the matrix-core kernels H3 / H4 and the option kernel I: none was
// selected by a default rule -- f32 MFMA has no peak advantage over the VALU on gfx950 and H2 issues half the flop; kernel I is
// exact only to ~1e-6 of a footprint's peak -- so round 5 removed them; HISTORY.md keeps their designs and measurements.)
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "tsp_pipeline.h"

namespace tsp {

// ---------------------------------------------------------------------------------------------
// kernel H2: huge footprints, row-uniform tile gather
// ---------------------------------------------------------------------------------------------
// For P >= 64 px a texel of the 64^2 kernel image is >= 1 pixel wide, so along a pixel ROW the y-interpolation
// factors (fy, gy) and the texel row are the same for every pixel, and along a pixel COLUMN the x-interpolated
// texel rows  L[r](col) = T[r][c]*gx + T[r][c+1]*fx  change only when the texel row r does -- every P/64 pixels.
// H2 maps that structure onto the wave: a lane owns W pixel COLUMNS (64 apart) x HR rows in registers, all 64
// lanes share the same HR pixel rows.  Per footprint a wave
//   * computes the row factors once, one row per lane (canonical texel coordinate, tsp_math.h), and redistributes
//     them through a per-wave LDS table so that lane l holds (fy, gy) of rows 4k + (l & 3), k = 0 .. HR/4 - 1:
//     every QUAD of lanes then carries the four rows of group k and a row's factor reaches all 64 lanes as the
//     DPP operand of the FMA itself (quad_perm:[t,t,t,t]) -- no LDS read, no scalar register per row;
//   * walks its rows with WAVE-UNIFORM control flow (bit tests on ballot masks):
//       on a texel-row change:  top = bot ; bot = L[r + 1](col) from the prefetched pair ; prefetch row r + 2
//       every covered row:      acc += gy*top ; acc += fy*bot                              -- 2 VALU per pixel
// against ~14.5 VALU + one 16-byte LDS read per pixel in a per-pixel bilinear gather (the round-1 kernel H).  The sum has the same non-negative terms as the
// canonical bilinear form in a different association (relative rounding differences of ~1e-7).

// ---- the row walk as one asm body (option h2_walk = 1; single channel, W = 1, the 64 x 32 / 64 x 16 strips at 8 waves/SIMD) -------
// The C++ walk below copies top = bot on every texel-row change and forms the prefetch address with a v_add: 4 vector instructions
// per change.  Here the two rolling rows (r0, r1) swap roles instead, and the prefetch reads texel row r0 + 2 + i at an immediate
// offset 260 (i mod 4) + 260 from a base stepped once every four changes: 2.25 vector instructions per change.  The walk is a state
// machine whose state s = (changes so far) mod 4 is the program counter: state s has its own copy of the row code, with
// top = r(s & 1), bot = r(~s & 1) and its own prefetch offset.  A group of four rows without a texel-row change runs its eight FMAs
// without a per-row bit test (one s_and for the group); a group with changes takes the per-row tested copy.  Every operation on
// the accumulators, the rolling rows and the prefetch is the C++ walk's, in the same order, so the float32 strip sums are
// bit-identical (the jmpmask double step included).  The asm owns: its LDS waits (lgkmcnt; LDS returns in order), the row factors
// (two ds_read_b32 per group, fetched one group ahead into two register pairs, as in the C++ walk's JIT path), and the DPP rule
// (a VGPR a VALU wrote is not a DPP source within two wait states: the DPP sources here are the row factors, written by LDS only).
#define H2A_S_(x) #x
#define H2A_S(x) H2A_S_(x)
#define H2A_TOP0 "%[r0]"
#define H2A_TOP1 "%[r1]"
#define H2A_TOP2 "%[r0]"
#define H2A_TOP3 "%[r1]"
#define H2A_BOT0 "%[r1]"
#define H2A_BOT1 "%[r0]"
#define H2A_BOT2 "%[r1]"
#define H2A_BOT3 "%[r0]"
#define H2A_NEXT0 "1"
#define H2A_NEXT1 "2"
#define H2A_NEXT2 "3"
#define H2A_NEXT3 "0"
#define H2A_STEP0 ""
#define H2A_STEP1 ""
#define H2A_STEP2 ""
#define H2A_STEP3 "v_add_u32 %[va], 0x410, %[va]\n\t"      /* 4 texel rows: the base moves on after the fourth change */
#define H2A_DPP(q) " quad_perm:[" #q "," #q "," #q "," #q "] row_mask:0xf bank_mask:0xf\n\t"
// pixel row t in state S: acc += gy*top ; acc += fy*bot, the factors of row t from quad lane q of the group's factor pair p
#define H2A_ROW(S, t, q, p)                                                                                    \
    "v_fmac_f32_dpp %[a" #t "], %[gy" #p "], " H2A_TOP##S H2A_DPP(q)                                           \
    "v_fmac_f32_dpp %[a" #t "], %[fy" #p "], " H2A_BOT##S H2A_DPP(q)
// the same row behind its texel-row test: a change leaves to .Lh2c<S>_<t> and resumes at .Lh2r<S+1>_<t>
#define H2A_TROW(S, t, q, p)                                                                                   \
    "s_bitcmp1_b32 %[chg], " #t "\n\t"                                                                         \
    "s_cbranch_scc1 .Lh2c" #S "_" #t "_%=\n"                                                                   \
    ".Lh2r" #S "_" #t "_%=:\n\t" H2A_ROW(S, t, q, p)
// group K (rows t0..t3, factor pair p) in state S: fetch the next group's factors (pair pn), skip an uncovered group, run the
// eight FMAs untested when the group has no change.  The fast path falls through to the next group's head.
#define H2A_GROUP(S, K, p, pn, t0, t1, t2, t3)                                                                 \
    ".Lh2g" #S "_" #K "_%=:\n\t"                                                                               \
    "ds_read_b32 %[fy" #pn "], %[rt] offset:32*(" #K "+1)\n\t"                                                 \
    "ds_read_b32 %[gy" #pn "], %[rt] offset:32*(" #K "+1)+4\n\t"                                               \
    "s_and_b32 %[tmp], %[cov], 15<<(4*" #K ")\n\t"                                                             \
    "s_cbranch_scc0 .Lh2k" #S "_" #K "_%=\n\t"                                                                 \
    "s_waitcnt lgkmcnt(2)\n\t"                  /* this group's factors (only the next group's two reads are younger) */ \
    "s_and_b32 %[tmp], %[chg], 15<<(4*" #K ")\n\t"                                                             \
    "s_cbranch_scc1 .Lh2s" #S "_" #K "_%=\n\t"                                                                 \
    H2A_ROW(S, t0, 0, p) H2A_ROW(S, t1, 1, p) H2A_ROW(S, t2, 2, p) H2A_ROW(S, t3, 3, p)
#define H2A_GROUP_LAST(S, K, p, t0, t1, t2, t3)                                                                \
    ".Lh2g" #S "_" #K "_%=:\n\t"                                                                               \
    "s_and_b32 %[tmp], %[cov], 15<<(4*" #K ")\n\t"                                                             \
    "s_cbranch_scc0 .Lh2end_%=\n\t"                                                                            \
    "s_waitcnt lgkmcnt(0)\n\t"                                                                                 \
    "s_and_b32 %[tmp], %[chg], 15<<(4*" #K ")\n\t"                                                             \
    "s_cbranch_scc1 .Lh2s" #S "_" #K "_%=\n\t"                                                                 \
    H2A_ROW(S, t0, 0, p) H2A_ROW(S, t1, 1, p) H2A_ROW(S, t2, 2, p) H2A_ROW(S, t3, 3, p)                        \
    "s_branch .Lh2end_%=\n"
// out of line, group K of state S: the tested rows, then the next group (N: its label, `end` after the last);  the skip of an
// uncovered group (the covered rows are contiguous: none below -> the next group, none above -> done; the row clip keeps them so,
// the chord of a strip's column interval being one interval of rows: see the row pass of splat_huge2_kernel)
#define H2A_SLOW(S, K, N, p, t0, t1, t2, t3)                                                                   \
    ".Lh2s" #S "_" #K "_%=:\n\t"                                                                               \
    H2A_TROW(S, t0, 0, p) H2A_TROW(S, t1, 1, p) H2A_TROW(S, t2, 2, p) H2A_TROW(S, t3, 3, p)                    \
    "s_branch .Lh2" #N "_%=\n"
#define H2A_SKIP(S, K, N)                                                                                      \
    ".Lh2k" #S "_" #K "_%=:\n\t"                                                                               \
    "s_lshr_b32 %[tmp], %[cov], 4*(" #K "+1)\n\t"                                                              \
    "s_cbranch_scc0 .Lh2end_%=\n\t"                                                                            \
    "s_branch .Lh2" #N "_%=\n"
// texel-row change at row t in state S: the row on top becomes the new bottom row = lerp(prefetched pair) (v_mul + v_fmac, the
// C++ walk's), the pair of the row after it loads; a double step (jmpmask) clears its bit and changes once more from state S + 1
#define H2A_CHG(S, t)                                                                                          \
    ".Lh2c" #S "_" #t "_%=:\n\t"                                                                               \
    "s_waitcnt lgkmcnt(0)\n\t"                                                                                 \
    "v_mul_f32 " H2A_TOP##S ", %[nx], %[gx]\n\t"                                                               \
    "v_fmac_f32 " H2A_TOP##S ", %[ny], %[fx]\n\t"                                                              \
    "ds_read_b32 %[nx], %[va] offset:260*(" #S "+1)\n\t"                                                       \
    "ds_read_b32 %[ny], %[va] offset:260*(" #S "+1)+4\n\t"                                                     \
    H2A_STEP##S                                                                                                \
    "s_bitcmp1_b32 %[jmp], " #t "\n\t"                                                                         \
    "s_cbranch_scc0 .Lh2r" H2A_NEXT##S "_" #t "_%=\n\t"                                                        \
    "s_bitset0_b32 %[jmp], " #t "\n\t"                                                                         \
    "s_branch .Lh2c" H2A_NEXT##S "_" #t "_%=\n"
#define H2A_CHG4(S, a, b, c, d) H2A_CHG(S, a) H2A_CHG(S, b) H2A_CHG(S, c) H2A_CHG(S, d)
// one state: groups (fall-through), then its out-of-line code
#define H2A_STATE16(S)                                                                                         \
    H2A_GROUP(S, 0, 0, 1, 0, 1, 2, 3) H2A_GROUP(S, 1, 1, 0, 4, 5, 6, 7) H2A_GROUP(S, 2, 0, 1, 8, 9, 10, 11)     \
    H2A_GROUP_LAST(S, 3, 1, 12, 13, 14, 15)                                                                    \
    H2A_SLOW(S, 0, g##S##_1, 0, 0, 1, 2, 3) H2A_SLOW(S, 1, g##S##_2, 1, 4, 5, 6, 7)                            \
    H2A_SLOW(S, 2, g##S##_3, 0, 8, 9, 10, 11) H2A_SLOW(S, 3, end, 1, 12, 13, 14, 15)                           \
    H2A_SKIP(S, 0, g##S##_1) H2A_SKIP(S, 1, g##S##_2) H2A_SKIP(S, 2, g##S##_3)                                 \
    H2A_CHG4(S, 0, 1, 2, 3) H2A_CHG4(S, 4, 5, 6, 7) H2A_CHG4(S, 8, 9, 10, 11) H2A_CHG4(S, 12, 13, 14, 15)
#define H2A_STATE32(S)                                                                                         \
    H2A_GROUP(S, 0, 0, 1, 0, 1, 2, 3) H2A_GROUP(S, 1, 1, 0, 4, 5, 6, 7) H2A_GROUP(S, 2, 0, 1, 8, 9, 10, 11)     \
    H2A_GROUP(S, 3, 1, 0, 12, 13, 14, 15) H2A_GROUP(S, 4, 0, 1, 16, 17, 18, 19)                                \
    H2A_GROUP(S, 5, 1, 0, 20, 21, 22, 23) H2A_GROUP(S, 6, 0, 1, 24, 25, 26, 27)                                \
    H2A_GROUP_LAST(S, 7, 1, 28, 29, 30, 31)                                                                    \
    H2A_SLOW(S, 0, g##S##_1, 0, 0, 1, 2, 3) H2A_SLOW(S, 1, g##S##_2, 1, 4, 5, 6, 7)                            \
    H2A_SLOW(S, 2, g##S##_3, 0, 8, 9, 10, 11) H2A_SLOW(S, 3, g##S##_4, 1, 12, 13, 14, 15)                      \
    H2A_SLOW(S, 4, g##S##_5, 0, 16, 17, 18, 19) H2A_SLOW(S, 5, g##S##_6, 1, 20, 21, 22, 23)                    \
    H2A_SLOW(S, 6, g##S##_7, 0, 24, 25, 26, 27) H2A_SLOW(S, 7, end, 1, 28, 29, 30, 31)                         \
    H2A_SKIP(S, 0, g##S##_1) H2A_SKIP(S, 1, g##S##_2) H2A_SKIP(S, 2, g##S##_3) H2A_SKIP(S, 3, g##S##_4)         \
    H2A_SKIP(S, 4, g##S##_5) H2A_SKIP(S, 5, g##S##_6) H2A_SKIP(S, 6, g##S##_7)                                 \
    H2A_CHG4(S, 0, 1, 2, 3) H2A_CHG4(S, 4, 5, 6, 7) H2A_CHG4(S, 8, 9, 10, 11) H2A_CHG4(S, 12, 13, 14, 15)      \
    H2A_CHG4(S, 16, 17, 18, 19) H2A_CHG4(S, 20, 21, 22, 23) H2A_CHG4(S, 24, 25, 26, 27) H2A_CHG4(S, 28, 29, 30, 31)
// entry: the first group's factors and the pair of texel row r0 + 2 load; exit: nothing of the asm's left in flight
#define H2A_HEAD                                                                                               \
    "ds_read_b32 %[nx], %[va]\n\t"                                                                             \
    "ds_read_b32 %[ny], %[va] offset:4\n\t"                                                                    \
    "ds_read_b32 %[fy0], %[rt]\n\t"                                                                            \
    "ds_read_b32 %[gy0], %[rt] offset:4\n"
#define H2A_TAIL ".Lh2end_%=:\n\t" "s_waitcnt lgkmcnt(0)"
#define H2A_A4(a, i, j, k, l) [a##i] "+v"(acc[i][0]), [a##j] "+v"(acc[j][0]), [a##k] "+v"(acc[k][0]), [a##l] "+v"(acc[l][0])
#define H2A_OPERANDS                                                                                           \
    [r0] "+v"(top), [r1] "+v"(bot), [nx] "=&v"(nx), [ny] "=&v"(ny), [fy0] "=&v"(fy0), [gy0] "=&v"(gy0),         \
    [fy1] "=&v"(fy1), [gy1] "=&v"(gy1), [va] "+v"(va), [jmp] "+s"(jmp), [tmp] "=&s"(tmp)
#define H2A_INPUTS [gx] "v"(gx), [fx] "v"(fx), [rt] "v"(rt), [cov] "s"(cov), [chg] "s"(chg)

// acc: the strip's accumulators; top / bot: x-interpolated texel rows r0, r0 + 1 of the first covered row; va: LDS byte address of
// this lane's pair (r0 + 2, c); rt: LDS byte address of this lane's slot in the hit's row-factor table; masks as in the C++ walk
template <int HR>
__device__ __forceinline__ void h2_walk_asm(float (&acc)[HR][1], float top, float bot, float gx, float fx, int va, int rt,
                                            unsigned cov, unsigned chg, unsigned jmp) {
    float nx, ny, fy0, gy0, fy1, gy1;
    unsigned tmp;
    if constexpr (HR == 16) {
        asm volatile(H2A_HEAD H2A_STATE16(0) H2A_STATE16(1) H2A_STATE16(2) H2A_STATE16(3) H2A_TAIL
                     : H2A_A4(a, 0, 1, 2, 3), H2A_A4(a, 4, 5, 6, 7), H2A_A4(a, 8, 9, 10, 11), H2A_A4(a, 12, 13, 14, 15),
                       H2A_OPERANDS
                     : H2A_INPUTS
                     : "memory", "scc");
    } else {
        static_assert(HR == 32, "asm row walk: 64 x 16 and 64 x 32 strips");
        asm volatile(H2A_HEAD H2A_STATE32(0) H2A_STATE32(1) H2A_STATE32(2) H2A_STATE32(3) H2A_TAIL
                     : H2A_A4(a, 0, 1, 2, 3), H2A_A4(a, 4, 5, 6, 7), H2A_A4(a, 8, 9, 10, 11), H2A_A4(a, 12, 13, 14, 15),
                       H2A_A4(a, 16, 17, 18, 19), H2A_A4(a, 20, 21, 22, 23), H2A_A4(a, 24, 25, 26, 27), H2A_A4(a, 28, 29, 30, 31),
                       H2A_OPERANDS
                     : H2A_INPUTS
                     : "memory", "scc");
    }
}

constexpr int PT_ROWS = 66;          // LDS kernel image rows: 64 + two clamp-to-edge copies of row 63 (for r + 1, r + 2)
constexpr int PT_STRIDE = 65;        // floats per row: 64 + one clamp-to-edge copy of column 63 (for c + 1); odd -> no bank conflicts

// CNT: fragment counting compiled in (tsp_set_option "count_fragments"); the product instantiation carries none of it
// AW: the row walk as one asm body (h2_walk_asm; option h2_walk), single channel, one column register
template <int MODE, int NACC, int W, int HR, int OCC, bool CNT, bool AW>
__global__ __launch_bounds__(H2T, OCC) void splat_huge2_kernel(TileArgs a) {
    static_assert(!AW || (NACC == 1 && W == 1 && (HR == 16 || HR == 32)), "asm row walk: single channel, 64 x 16 / 64 x 32 strips");
    constexpr int C = (MODE == TSP_MODE_RGB) ? 4 : 2;
    constexpr int NW = (MODE == TSP_MODE_RGB) ? 2 : 1;
    constexpr int TW = 2 * 64 * W, TH = 2 * HR;            // tile: 2 x 2 wave strips of (64 W) x HR pixels
    constexpr int NG = HR / 4;                             // row groups (one quad of lanes carries a group's factors)
    static_assert(HR == 16 || HR == 32 || HR == 64, "rows per wave strip");
    typedef typename std::conditional<HR == 64, unsigned long long, unsigned>::type mask_t;     // one bit per pixel row of the strip
    extern __shared__ __attribute__((aligned(16))) float smem[];
    // level-0 kernel image with clamp-to-edge padding: texels (r, c) and (r, c + 1) of an x-interpolation are adjacent
    // dwords, fetched by one ds_read2_b32
    float *PT = smem;                                                        // [PT_ROWS][PT_STRIDE]
    float2 *rt_all = reinterpret_cast<float2 *>(smem + ((PT_ROWS * PT_STRIDE + 3) & ~3));   // per wave: (fy, gy) of its HR rows

    // (the wave index as a scalar: the strip's origin and edges then live in scalar registers -- as vector values two of them were
    // spilled and re-read from scratch for every 64 records, behind the record prefetch they then waited for)
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int R = a.cam.R;
    // (blockIdx = tile * split + sp: an XCD-aware order -- the workgroups resident on one XCD walking several tiles per slice of the
    // record list, so that the list crosses the fabric once per tile group -- measured 7-11 % SLOWER at 1e9 particles: round 5)
    const int tile_id = blockIdx.x / a.split, sp = blockIdx.x % a.split;
    const int tx0 = (tile_id % a.tiles_x) * TW, ty0 = (tile_id / a.tiles_x) * TH;
    for (int i = tid; i < PT_ROWS * PT_STRIDE; i += H2T) {
        const int j = min(i / PT_STRIDE, 63), x = min(i % PT_STRIDE, 63);
        PT[i] = a.mips[j * 64 + x];
    }
    float2 *rt = rt_all + wv * 64;
    const float2 *rt_quad = rt + (lane & 3);               // this lane's slot in every row group
    const int sx = tx0 + 64 * W * (wv & 1), sy = ty0 + HR * (wv >> 1);
    // (the strip's edges as floats, pinned in scalar registers: converted on the vector ALU they were wave-uniform values in VGPRs, and
    // three of them were spilled and re-read from scratch for every 64 records)
    // (as asm: the compiler knows the value is uniform, folds the builtin away and keeps the converted value in a VGPR)
    auto uniform_f = [](int v) -> float { float s; asm("v_readfirstlane_b32 %0, %1" : "=s"(s) : "v"((float)v)); return s; };
    const float sx0 = uniform_f(sx), sx1 = uniform_f(sx + 64 * W), sy0 = uniform_f(sy), sy1 = uniform_f(sy + HR);
    float pxc[W];
#pragma unroll
    for (int w = 0; w < W; ++w) pxc[w] = (sx + 64 * w + lane < R) ? (float)(sx + 64 * w + lane) + 0.5f : __builtin_inff();
    const int myrow = lane & (HR - 1);
    const float pyc_own = (sy + myrow < R) ? (float)(sy + myrow) + 0.5f : __builtin_inff();

    // float32 accumulators hold at most FOLD_EVERY (2048) footprints, then go to the float64 render target: a sum of n non-negative
    // terms accumulates ~sqrt(n) 2^-24 of relative rounding error at the worst pixel; measured on a 4e7-particle sample of the 1e9
    // snapshot the image's largest relative error is 2.9e-7 / 3.1e-7 / 3.3e-7 at 512 / 1024 / 2048 (it is the final float32 rounding
    // that shows), while the float64 flush atomics were 2/3 of the rgb render's HBM writes at 512.  Second-level register totals
    // would cost HR * W more VGPRs and spill here
    constexpr int FOLD_EVERY = TSP_FOLD_EVERY;
    float acc[HR * W][NACC];
#pragma unroll
    for (int p = 0; p < HR * W; ++p)
#pragma unroll
        for (int c = 0; c < NACC; ++c) acc[p][c] = 0.0f;
    unsigned long long n_frag = 0;
    const char *PTb = reinterpret_cast<const char *>(PT);
    __syncthreads();                                       // the only workgroup barrier: from here on the waves run free
    if (sx >= R || sy >= R) return;                        // a strip wholly outside the image (R not a multiple of the tile)

    // Every wave scans the workgroup's share of the record list on its own, 64 records at a time (one per lane),
    // and keeps those whose square and disc reach ITS strip -- no shared queue, so no wave ever waits for another.
    // The four waves read the same records at about the same time (L1 / L2 hits).  Records are dealt to the `split`
    // workgroups of a tile in runs of HDEAL: consecutive records are spatial neighbours (consecutive chunks), so
    // every workgroup sees an even sample of the tile's footprints.
    // 32-bit record indices (the launcher refuses lists of 2^31 records or more)
    // With band bins (huge_band_fill_kernel) the tile scans only the records whose squares reach its 64-row image band:
    // ~1/3 of the list for the reference h-law at 1024^2, the same records in the same dealing
    const float4 *geom = a.geom;
    const float *wts = a.w;
    unsigned n_rec = (unsigned)a.n_records;
    if (a.bin_count) {
        const int band = ty0 / HBAND_H;
        geom += (size_t)band * a.band_stride;
        wts += (size_t)band * a.band_stride * NW;
        n_rec = (unsigned)a.bin_count[band];
    }
    const unsigned n_runs = (n_rec + HDEAL - 1) / HDEAL, usplit = (unsigned)a.split, n_last = max(n_rec, 1u) - 1u;
    // record index of this lane in batch run0: ((run0 + lane / HDEAL) * split + sp) * HDEAL + lane % HDEAL = a wave-uniform base + lane_off
    const unsigned lane_off = (unsigned)(lane / HDEAL) * usplit * HDEAL + (unsigned)(lane & (HDEAL - 1));      // (loop-invariant)
    auto batch_base = [&](unsigned run0) -> unsigned { return (run0 * usplit + sp) * HDEAL; };
    auto fetch = [&](unsigned run0, float4 &g, float &gw1, float &gw2) {
        // unconditional loads (a slot past the end re-reads the last record; the batch empties such slots when it starts): under a
        // branch the compiler cannot count the loads in flight and waits for this prefetch right after issuing it
        const unsigned rc = min(batch_base(run0) + lane_off, n_last);
        g = geom[rc];
        gw1 = (NACC >= 2) ? wts[rc * NW] : 0.0f;
        gw2 = (NW == 2) ? wts[rc * NW + 1] : 0.0f;
    };
    float4 g_next; float gw1_next, gw2_next;
    fetch(0, g_next, gw1_next, gw2_next);
    // (the first batch lands before the loop: with loads of the preheader still in flight at the loop header the compiler's
    // counter model gives up and waits for every prefetch right after issuing it -- vmcnt(0) at the top of each batch: round 6)
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
    // The record loop is cut into segments of >= FOLD_EVERY footprints (<= FOLD_EVERY + 63); the accumulators go to the
    // float64 target between segments: ONE flush site, outside the hot loops (under the innermost loop
    // its offsets filled the scalar file and the accumulators were parked in scratch around every 64-record batch)
    unsigned run0 = 0;
    do {
    int since_fold = 0;
    for (; run0 * usplit < n_runs && since_fold < FOLD_EVERY; run0 += 64 / HDEAL) {
        float4 g = g_next;
        const float gw1 = gw1_next, gw2 = gw2_next;
        if (batch_base(run0) + lane_off >= n_rec) g.z = 0.0f;      // (a slot past the end of the list)
        fetch(run0 + 64 / HDEAL, g_next, gw1_next, gw2_next);      // the next 64 records load while these are rasterised
        const float g_half = 0.5f * g.z;
        // (g.z = 0 marks an empty slot; the kernel vanishes outside the disc inscribed in the footprint square)
        unsigned long long hits = __ballot(reaches_strip(g, sx0, sx1, sy0, sy1, a.disc_k2));
        if (hits == 0ull) continue;
        since_fold += __popcll(hits);
        const float g_invP = 1.0f / g.z;
        // the row clip's limit for this record on this strip (tsp_pipeline.h chord_limit), once per batch: a pixel row at d from the
        // centre in y with d d >= g_lim has its chord of the disc outside the strip's columns
        const float g_lim = chord_limit(g.x, g.z, sx0, sx1, a.chord_k2);
        const float g_w1 =(MODE == TSP_MODE_RGB) ? gw1 : g.w * gw1;
        // The rows of NH = 64 / HR hits are evaluated in ONE pass: lane j works out pixel row j % HR for hit j / HR (with HR = 32 the
        // upper half of the wave used to repeat the lower half's work); the hits' parameters reach their lanes through ds_bpermute
        // (the LDS crossbar, not the vector ALU) instead of a v_readlane each per hit.  Columns and the row walk follow hit by hit.
        constexpr int NH = 64 / HR;
        while (hits) {
            int srcs[NH], n_h = 0;
#pragma unroll
            for (int i = 0; i < NH; ++i) {
                srcs[i] = i ? srcs[0] : 0;
                if (hits) { srcs[i] = __ffsll((long long)hits) - 1; hits &= hits - 1; n_h = i + 1; }
            }
            // ---- rows: lane j evaluates row j % HR of hit j / HR and the texel row of the row above it -----------------
            unsigned long long cov64, chg64, jmp64;
            int r512;                                   // byte offset of this lane's texel row in PT
            {
                int src_l = srcs[0];
#pragma unroll
                for (int i = 1; i < NH; ++i) src_l = (lane >= HR * i) ? srcs[i] : src_l;
                const int bp = src_l << 2;
                const float pcy_l = __int_as_float(__builtin_amdgcn_ds_bpermute(bp, __float_as_int(g.y)));
                const float half_l = __int_as_float(__builtin_amdgcn_ds_bpermute(bp, __float_as_int(g_half)));
                const float invP_l = __int_as_float(__builtin_amdgcn_ds_bpermute(bp, __float_as_int(g_invP)));
                const float lim_l = __int_as_float(__builtin_amdgcn_ds_bpermute(bp, __float_as_int(g_lim)));
                const float d = pyc_own - pcy_l;
                // The row clip (option h2_chord): a row of the square whose chord of the inscribed disc misses this strip's 64 W columns
                // is taken for uncovered -- every pixel of it would receive weight x (0 top + 0 bot), an exact zero: the records here
                // have finite weights (huge_nonfinite_kernel draws the others itself and negates their widths), so 0 x weight is 0 and
                // no float32 strip sum changes by a bit.  Its factors go to (0, 0) like an uncovered row's (cv).  The rows a disc leaves
                // to a column interval are ONE interval of rows (|d| below a bound), so the covered rows stay contiguous: what the
                // masks below, `first`, r_off and both walks assume.  A NaN limit clears nothing (the comparison is false).
                const bool covered_row = __builtin_fabsf(d) < half_l && !row_outside_chord(d, lim_l);
                const float cv = covered_row ? 1.0f : 0.0f;
                // the canonical float32 texel coordinate (tsp_math.h: the oracle forms it with the same operations -- a value next to
                // a zero texel is proportional to its fraction, so even one ulp of difference here shows at 1e-5 relative)
                const float v = (d + half_l) * invP_l;
                const float tv = __builtin_amdgcn_fmed3f(__builtin_fmaf(v, 64.0f, -0.5f), 0.0f, 63.0f);
                const float fr = __builtin_amdgcn_fractf(tv) * cv;      // (tv - floor(tv), exact for 0 <= tv <= 63, in one instruction)
                const int r = (int)tv;                  // (tv >= 0: the conversion truncates = floor)
                // texel row of the pixel row above = the value of the lane before (v_mov_b32_dpp wave_shr:1); row 0 of every hit
                // is excluded below
                const int rprev = __builtin_amdgcn_mov_dpp(r, 0x138, 0xf, 0xf, false);
                r512 = __mul24(r, PT_STRIDE * 4);      // (v_mul_u32_u24: full rate; v_mul_lo_u32 takes four issue slots)
                asm volatile("" ::: "memory");          // (in-order LDS: the previous footprints' table reads are done)
                rt[lane] = make_float2(fr, cv - fr);      // (the table has 64 slots per wave: HR rows for each of the NH hits)
                asm volatile("" ::: "memory");
                // the row masks straight from vector compares (as __ballot(bool expression) each costs a v_cndmask + v_cmp round trip)
                constexpr unsigned long long ROW0S = (HR == 64) ? 1ull : ((HR == 32) ? 0x0000000100000001ull : 0x0001000100010001ull);
                cov64 = __builtin_amdgcn_fcmpf(__builtin_fabsf(d), half_l, 4 /* FCMP_OLT */) &
                        ~__builtin_amdgcn_fcmpf(d * d, lim_l, 3 /* FCMP_OGE */);      // (= the lanes of covered_row)
                chg64 = __builtin_amdgcn_uicmp((unsigned)r, (unsigned)rprev, 33 /* ICMP_NE */) & cov64 & ~ROW0S;
                // texel rows advance by at most one per pixel row when P >= 64; rounding at P ~ 64 may still skip one
                jmp64 = __builtin_amdgcn_uicmp((unsigned)r, (unsigned)(rprev + 1), 33 /* ICMP_NE */) & chg64;
            }
            for (int hh = 0; hh < n_h; ++hh) {
            int src = srcs[0];
#pragma unroll
            for (int i = 1; i < NH; ++i) src = (hh == i) ? srcs[i] : src;
            constexpr unsigned long long ROWS = (HR == 64) ? ~0ull : ((1ull << (HR & 63)) - 1ull);      // (the bits above belong to the next hit)
            mask_t covmask = (mask_t)((cov64 >> ((HR * hh) & 63)) & ROWS), chgmask = (mask_t)((chg64 >> ((HR * hh) & 63)) & ROWS),
                   jmpmask = (mask_t)((jmp64 >> ((HR * hh) & 63)) & ROWS);
            // the footprint's parameters, wave-uniform (scalar registers)
            const float pcx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(g.x), src));
            const float half = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(g_half), src));
            const float invP = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(g_invP), src));
            float4 wq;
            wq.x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(g.w), src));
            wq.y = (NACC >= 2) ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(g_w1), src)) : 0.0f;
            wq.z = (NACC >= 3) ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(gw2), src)) : 0.0f;
            wq.w = 0.0f;
            if (NACC >= 2) {
                // the channel weights feed tied-operand FMAs on every row: park them in VGPRs once per footprint (left to
                // itself the compiler re-copies the scalar before every use: three extra v_mov per row)
                asm volatile("v_mov_b32 %0, %1" : "=v"(wq.x) : "s"(wq.x));
                asm volatile("v_mov_b32 %0, %1" : "=v"(wq.y) : "s"(wq.y));
                if (NACC >= 3) asm volatile("v_mov_b32 %0, %1" : "=v"(wq.z) : "s"(wq.z));
            }
            const float2 *rt_quad_h = rt_quad + HR * hh;      // this hit's rows of the table
            if (covmask == 0) continue;
            // the first covered row's texel rows are loaded before the row walk (below): it is never a "change"
            const mask_t first = covmask & ((mask_t)0 - covmask);
            chgmask &= ~first; jmpmask &= ~first;
            // row factors of group k for the DPP broadcast: lane l takes rows 4k + (l & 3)
            // HR = 16: the four groups' factors sit in registers; HR = 32: two registers pairs in turn (group K + 1 loads while
            // group K is walked), 12 VGPRs fewer -- what lets the 64 x 32 strips run at 6 waves per SIMD
            constexpr bool JIT = (HR >= 32);
            constexpr int NRF = JIT ? 2 : NG;
            float2 rowf[NRF];
            if constexpr (JIT) rowf[0] = rt_quad_h[0];
            else {
#pragma unroll
                for (int k = 0; k < NG; ++k) rowf[k] = rt_quad_h[4 * k];
            }
            // ---- columns: W per lane ----
            int caddr[W];
            float fxs[W], gxs[W];
            int ncov_x = 0;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const float d = pxc[w] - pcx;
                const bool covered = __builtin_fabsf(d) < half;
                const float u = (d + half) * invP;
                const float tu = __builtin_amdgcn_fmed3f(__builtin_fmaf(u, 64.0f, -0.5f), 0.0f, 63.0f);
                caddr[w] = ((int)tu) * 4;
                // uncovered column: both weights 0.  Density: the particle weight rides on the column factors, so a pixel costs two FMAs
                // (fr * (c w) and (1 - fr) * (c w) with c = 0 or 1: the same bits as (fr c) * w and (c - fr c) * w)
                const float cw = covered ? ((NACC == 1) ? wq.x : 1.0f) : 0.0f;
                const float fr = __builtin_amdgcn_fractf(tu);
                fxs[w] = fr * cw;
                gxs[w] = (1.0f - fr) * cw;
                if (CNT) ncov_x += covered ? 1 : 0;
            }
            if constexpr (AW) {
                typedef const __attribute__((address_space(3))) float LdsF;
                const int r_off = __builtin_amdgcn_readlane(r512, __ffs((int)covmask) - 1 + HR * hh);
                auto lerp_at = [&](int byteoff) -> float {      // = lerp(0, pair_at(0, byteoff)) of the C++ walk
                    const float *t = reinterpret_cast<const float *>(PTb + byteoff + caddr[0]);
                    return __builtin_fmaf(t[1], fxs[0], t[0] * gxs[0]);
                };
                const float t0 = lerp_at(r_off), t1 = lerp_at(r_off + PT_STRIDE * 4);
                const int va = (int)(unsigned)(unsigned long long)(LdsF *)PT + r_off + 2 * PT_STRIDE * 4 + caddr[0];
                const int rtq = (int)(unsigned)(unsigned long long)(LdsF *)(const float *)rt_quad_h;
                h2_walk_asm<HR>(acc, t0, t1, gxs[0], fxs[0], va, rtq, (unsigned)covmask, (unsigned)chgmask, (unsigned)jmpmask);
            } else {
            float top[W], bot[W];
            float2 nxt[W];                              // prefetched pair of texel row r + 2
            auto pair_at = [&](int w, int byteoff) -> float2 {
                const float *t = reinterpret_cast<const float *>(PTb + byteoff + caddr[w]);
                return make_float2(t[0], t[1]);
            };
            auto lerp = [&](int w, float2 t) -> float { return __builtin_fmaf(t.y, fxs[w], t.x * gxs[w]); };
            // texel rows of the first covered pixel row (wave-uniform byte offset of its texel row in PT), the pair after them in flight
            int r_off = __builtin_amdgcn_readlane(r512, (HR == 64 ? __ffsll((long long)covmask) : __ffs((int)covmask)) - 1 + HR * hh);
#pragma unroll
            for (int w = 0; w < W; ++w) {
                top[w] = lerp(w, pair_at(w, r_off)); bot[w] = lerp(w, pair_at(w, r_off + PT_STRIDE * 4));
                nxt[w] = pair_at(w, r_off + 2 * PT_STRIDE * 4);
            }
            // ONE way to advance a texel row -- top = bot, bot = the x-interpolated prefetched pair, the next pair loads -- so that the
            // rolling registers never meet a second definition at a control-flow merge (with a separate reload-from-scratch path for
            // the first row and for skips the compiler copied the pair aside on every change: three v_mov).  Where float32 rounding
            // at P ~ 64 makes the texel row skip one, the step runs twice.
            auto row_step = [&]() {
                r_off += PT_STRIDE * 4;
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    // top = bot; bot = nxt.x * gx + nxt.y * fx -- in place (left to the compiler the new row lands in a third register
                    // and is moved: one more v_mov per texel-row change)
                    asm volatile("v_mov_b32 %0, %1\n\tv_mul_f32 %1, %2, %4\n\tv_fmac_f32 %1, %3, %5"
                                 : "=&v"(top[w]), "+v"(bot[w]) : "v"(nxt[w].x), "v"(nxt[w].y), "v"(gxs[w]), "v"(fxs[w]));
                    nxt[w] = pair_at(w, r_off + 2 * PT_STRIDE * 4);
                }
            };
            auto row_change = [&](int /*ty*/, bool skip) {      // `skip` is wave-uniform
                if (skip) row_step();                           // (rare; first, so that the common step below ends at the join)
                row_step();
            };
            // DPP hazard (gfx9: a VGPR written by a VALU instruction may not be read as a DPP operand in the next two issue
            // slots).  The DPP operands below are the row factors: they come from LDS (no VALU write) long before their use,
            // and the compiler does not see inside the asm statements, so pin them in registers here and leave two wait
            // states; the other operands of the DPP FMAs (top, bot) are ordinary sources and carry no such restriction.
            if constexpr (!JIT) {
#pragma unroll
                for (int k = 0; k < NG; ++k) asm volatile("" : "+v"(rowf[k].x), "+v"(rowf[k].y));
                asm volatile("s_nop 1");
            }
#define TSP_H2_ROW(K, T)                                                                                       \
            {                                                                                                  \
                constexpr int ty_ = 4 * (K) + (T);                                                             \
                if ((chgmask >> ty_) & 1) row_change(ty_, ((jmpmask >> ty_) & 1) != 0);                       \
                _Pragma("unroll") for (int w = 0; w < W; ++w) {                                                \
                    float *ac = acc[ty_ * W + w];                                                              \
                    if (NACC == 1) {                                                                           \
                        fmac_quad<T>(ac[0], rowf[JIT ? ((K) & 1) : (K)].y, top[w]);                                                \
                        fmac_quad<T>(ac[0], rowf[JIT ? ((K) & 1) : (K)].x, bot[w]);                                                \
                    } else {                                                                                   \
                        float kv = mul_quad<T>(rowf[JIT ? ((K) & 1) : (K)].y, top[w]);                                             \
                        fmac_quad<T>(kv, rowf[JIT ? ((K) & 1) : (K)].x, bot[w]);                                                   \
                        fmac_plain(ac[0], kv, wq.x);                                                           \
                        fmac_plain(ac[NACC >= 2 ? 1 : 0], kv, wq.y);                                           \
                        if (NACC >= 3) fmac_plain(ac[NACC - 1], kv, wq.z);                                     \
                    }                                                                                          \
                }                                                                                              \
            }
            // Only the rolling texel rows (top, bot, nxt) are touched under a (wave-uniform) branch; the accumulation itself
            // is straight-line (an uncovered row has fy = gy = 0); groups of four rows wholly outside the footprint are
            // skipped.  (Laying the change out of line as the unlikely path measured slower: this kernel serves the
            // footprints of 64 px and up, whose texel rows change every 1-8 pixel rows below 512 px.)
            // (Round 5: a second, test-free copy of a group's eight FMAs for the groups without a texel-row change -- the per-row bit
            // tests are three quarters of this kernel's scalar instructions -- made the register allocator spill around every
            // footprint's set-up at the control-flow merges: 32.7 -> 49 ms at 1e9 particles.  One code path per row it stays here;
            // h2_walk_asm has both, its registers allocated by hand.)
#define TSP_H2_GROUP(K)                                                                                        \
            if constexpr ((K) < NG) {                                                                          \
                if constexpr (JIT && (K) + 1 < NG) rowf[((K) + 1) & 1] = rt_quad_h[4 * ((K) + 1)];               \
                if (((covmask >> (4 * (K))) & 15) != 0) {                                                    \
                    if constexpr (JIT) asm volatile("" : "+v"(rowf[(K) & 1].x), "+v"(rowf[(K) & 1].y));        \
                    TSP_H2_ROW(K, 0) TSP_H2_ROW(K, 1) TSP_H2_ROW(K, 2) TSP_H2_ROW(K, 3)                          \
                }                                                                                              \
            }
            TSP_H2_GROUP(0) TSP_H2_GROUP(1) TSP_H2_GROUP(2) TSP_H2_GROUP(3)
            TSP_H2_GROUP(4) TSP_H2_GROUP(5) TSP_H2_GROUP(6) TSP_H2_GROUP(7)
            TSP_H2_GROUP(8) TSP_H2_GROUP(9) TSP_H2_GROUP(10) TSP_H2_GROUP(11)
            TSP_H2_GROUP(12) TSP_H2_GROUP(13) TSP_H2_GROUP(14) TSP_H2_GROUP(15)
#undef TSP_H2_GROUP
#undef TSP_H2_ROW
            }      // (C++ walk)
            if (CNT) n_frag += (unsigned long long)(ncov_x * __popcll((unsigned long long)covmask));
#ifdef TSP_H2_DEBUG      // analysis build: (footprint, strip) pairs, covered rows and texel-row changes instead of the S / G fragment counts
            if (CNT && lane == 0) {
                atomicAdd(&a.cnt->n_frag_class[0], 1ull);
                atomicAdd(&a.cnt->n_frag_class[1], (unsigned long long)__popcll((unsigned long long)covmask));
                unsigned long long groups = 0;        // row groups of four with a covered row (each costs 8 FMAs per column register)
                for (int k = 0; k < NG; ++k) groups += (((unsigned long long)covmask >> (4 * k)) & 15ull) ? 1ull : 0ull;
                atomicAdd(&a.cnt->n_frag_class[3], (unsigned long long)__popcll((unsigned long long)chgmask) + (groups << 32));
            }
#endif
            }      // (hits of this row pass)
        }
    }
    // ---- add this wave's partial strip into the render target ---------------------------------------
    {
        int Rl = R;                                   // laundered: the row offsets are formed here, not hoisted out of the record loop
        asm volatile("" : "+s"(Rl));
        double *img = a.img + ((size_t)sy * Rl + (sx + lane)) * C;
        asm volatile("" : "+v"(img));
#pragma unroll
        for (int ty = 0; ty < HR; ++ty)
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const int p = ty * W + w, gx = sx + 64 * w + lane, gy = sy + ty;
                if (gx < Rl && gy < Rl) {
                    double *d = img + ((size_t)ty * Rl + 64 * w) * C;
#pragma unroll
                    for (int c = 0; c < NACC; ++c) {
                        if (acc[p][c] != 0.0f) gatomic_add(d + c, acc[p][c]);
                        acc[p][c] = 0.0f;
                    }
                }
            }
    }
    } while (run0 * usplit < n_runs);
    if (CNT) {
        for (int o = 32; o; o >>= 1) n_frag += __shfl_xor((long long)n_frag, o);
        if (lane == 0 && n_frag) { atomicAdd(&a.cnt->n_fragments, n_frag); atomicAdd(&a.cnt->n_frag_class[2], n_frag); }
    }
}

// ---------------------------------------------------------------------------------------------
// band bins of the huge records
// ---------------------------------------------------------------------------------------------
// Huge records whose weights are not finite (an infinite or NaN mass, quantity or colour, or m / h^2 beyond float32)
// ---------------------------------------------------------------------------------------------
// A particle changes only the pixels its square covers (no fragment runs outside the reference's quad).  Kernel H2 cannot keep that
// for such a weight: its row walk multiplies the weight by the factors of every column and row of a strip, and the factors of the
// columns and rows the square does not cover are 0 -- 0 x inf = NaN in pixels the particle never reaches.  This pass finds those
// records before kernel H2 (and the band fill) read the list, draws each of them pixel by pixel over its square with the canonical
// arithmetic of the generic kernel, and negates its width in the list: kernel H2 and the band fill take only records of positive
// width, the rgb rectangle counts use |width|.  Records with finite weights pass through untouched, so kernel H2's code is the same.
// One read of the list per render block; the drawing is the rare path (one workgroup per found record, 256 pixels per step).
template <int MODE>
__global__ __launch_bounds__(256) void huge_nonfinite_kernel(float4 *__restrict__ geom, const float *__restrict__ w, long long n,
                                                             int second_channel, TileArgs a) {
    constexpr int C = (MODE == TSP_MODE_RGB) ? 4 : 2;
    constexpr int NW = (MODE == TSP_MODE_RGB) ? 2 : 1;
    constexpr int PER = 4;                 // records per thread
    __shared__ int s_n;
    __shared__ int s_rec[256 * PER];
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const long long first = (long long)blockIdx.x * 256 * PER + threadIdx.x;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const long long i = first + k * 256;
        if (i >= n) break;
        const float w0 = geom[i].w;
        bool ok = __builtin_fabsf(w0) < __builtin_inff();
        if (MODE == TSP_MODE_RGB || second_channel) ok = ok && __builtin_fabsf(w[i * NW]) < __builtin_inff();
        if (NW == 2) ok = ok && __builtin_fabsf(w[i * NW + 1]) < __builtin_inff();
        if (!ok) s_rec[atomicAdd(&s_n, 1)] = (int)(i - (long long)blockIdx.x * 256 * PER);
    }
    __syncthreads();
    const int n_odd = s_n;
    if (n_odd == 0) return;
    const int R = a.cam.R;
    unsigned long long nfrag = 0;
    for (int r = 0; r < n_odd; ++r) {
        const long long i = (long long)blockIdx.x * 256 * PER + s_rec[r];
        const float4 g = geom[i];
        Proj p;
        p.pcx = g.x; p.pcy = g.y; p.P = g.z; p.half = 0.5f * g.z; p.invP = 1.0f / g.z;
        const float a0 = g.w, a1 = (MODE == TSP_MODE_RGB || second_channel) ? w[i * NW] : 0.0f, a2 = (NW == 2) ? w[i * NW + 1] : 0.0f;
        int ilo, ihi, jlo, jhi;
        cover_range(p.pcx, p.half, R, ilo, ihi);
        cover_range(p.pcy, p.half, R, jlo, jhi);
        const int nx = ihi - ilo + 1;
        const long long npx = (ilo <= ihi && jlo <= jhi) ? (long long)nx * (jhi - jlo + 1) : 0;
        for (long long idx = threadIdx.x; idx < npx; idx += 256) {
            const int jj = (int)(idx / nx);
            const int j = jlo + jj, ii = ilo + (int)(idx - (long long)jj * nx);
            const float k = sample_kernel(a.mips, p, -1, ((float)ii + 0.5f) - p.pcx, ((float)j + 0.5f) - p.pcy);
            double *px = a.img + ((size_t)j * R + ii) * C;
            if (MODE == TSP_MODE_RGB) {      // (channel 3, the square count, comes from the rectangle sums like every huge record's)
                gatomic_add(px + 0, (double)(k * a0));
                gatomic_add(px + 1, (double)(k * a1));
                gatomic_add(px + 2, (double)(k * a2));
            } else {
                const float val = k * a0;
                gatomic_add(px + 0, (double)val);
                if (second_channel) gatomic_add(px + 1, (double)(val * a1));
            }
        }
        nfrag += (unsigned long long)npx;
        __syncthreads();                    // (every thread has read the record before it is marked)
        if (threadIdx.x == 0) geom[i].z = -g.z;
    }
    if (a.count_frag && threadIdx.x == 0 && nfrag) {
        atomicAdd(&a.cnt->n_fragments, nfrag);
        atomicAdd(&a.cnt->n_frag_class[2], nfrag);
    }
}

// ---------------------------------------------------------------------------------------------
// Every tile of kernel H2 used to scan the WHOLE huge list (at 1e9 particles: 128 tiles x 85 MB through eight non-coherent
// L2s = 12.7 GB of fabric reads per launch, and 1/12 of the kernel's instructions spent on records that cannot reach the tile).
// One pass copies every record into the bin of each 64-row image band its square reaches (a square of P pixels reaches
// P / 64 + 1 or + 2 of them; one pixel of margin per side so that float rounding can only add a band, never drop one -- kernel
// H2 repeats the exact test per strip).  Bins are fixed regions of n_huge records each, so no sizes need to be known first;
// a workgroup reserves its slots per band with ONE global atomic (counts formed in LDS): the 12-ns same-address atomics that
// made per-record binning cost 3.3 ms in round 2 are ~n_bands per 1024 records here.
template <int NW>
__global__ __launch_bounds__(256) void huge_band_fill_kernel(const float4 *__restrict__ geom, const float *__restrict__ w, long long n,
                                                             int R, int n_bands, float4 *__restrict__ out_geom, float *__restrict__ out_w,
                                                             long long stride, int *__restrict__ band_count, const long long *__restrict__ band_base) {
    constexpr int PER = 4;                 // records per thread
    extern __shared__ int s_band[];        // [n_bands] counts, then [n_bands] bases
    int *s_cnt = s_band, *s_base = s_band + n_bands;
    for (int b = threadIdx.x; b < n_bands; b += 256) s_cnt[b] = 0;
    __syncthreads();
    const long long first = ((long long)blockIdx.x * 256 + threadIdx.x) * PER;
    float4 g[PER];
    int b0[PER], b1[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        b0[k] = 1; b1[k] = 0;
        if (first + k < n) {
            g[k] = geom[first + k];
            const float half = 0.5f * g[k].z, mg = bin_margin(g[k].y, half), lo = g[k].y - half - mg, hi = g[k].y + half + mg;
            // (non-finite or off-image squares: no band; kernel S emits only records that cover a pixel)
            // (a negative width: a record with a weight that is not finite, drawn by huge_nonfinite_kernel)
            if (g[k].z > 0.0f && hi >= 0.0f && lo < (float)R && lo == lo && hi == hi) {
                b0[k] = max(0, (int)__builtin_floorf(fmaxf(lo, 0.0f) * (1.0f / HBAND_H)));
                b1[k] = min(n_bands - 1, (int)__builtin_floorf(fminf(hi, (float)R) * (1.0f / HBAND_H)));
            }
            for (int b = b0[k]; b <= b1[k]; ++b) atomicAdd(&s_cnt[b], 1);
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < n_bands; b += 256) {
        const int c = s_cnt[b];
        s_base[b] = c ? atomicAdd(&band_count[b], c) : 0;
        s_cnt[b] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        if (first + k >= n || b0[k] > b1[k]) continue;
        float w0 = w[(first + k) * NW], w1 = (NW == 2) ? w[(first + k) * NW + 1] : 0.0f;
        for (int b = b0[k]; b <= b1[k]; ++b) {
            const long long slot = (band_base ? band_base[b] : (long long)b * stride) + s_base[b] + atomicAdd(&s_cnt[b], 1);
            out_geom[slot] = g[k];
            out_w[slot * NW] = w0;
            if (NW == 2) out_w[slot * NW + 1] = w1;
        }
    }
}

// bins the huge list when that pays and fits the memory budget; sets ta.{geom, w, bin_count, band_stride} (or leaves the bins null)
template <int NW>
static int bin_huge_records(tsp_context *ctx, TileArgs &ta, const float4 *huge_geom, const float *huge_w, long long n_huge) {
    ta.bin_count = nullptr; ta.band_stride = 0; ta.bin_base = nullptr;
    Workspace &ws = ctx->ws;
    const int n_bands = (ctx->R + HBAND_H - 1) / HBAND_H;
    const size_t rec_bytes = sizeof(float4) + NW * sizeof(float);
    // (one band: nothing to gain; a short list is scanned in microseconds; a huge image with a long list would not fit)
    if (n_bands < 2 || n_huge < 4096 || (long long)n_bands * n_huge * (long long)rec_bytes > ctx->huge_band_budget) return TSP_OK;
    if (ws.hband_stride < n_huge || ws.hband_bands < n_bands) {
        int64_t stride = n_huge + n_huge / 8 + 1024;
        if ((long long)n_bands * stride * (long long)(sizeof(float4) + 2 * sizeof(float)) > ctx->huge_band_budget + (ctx->huge_band_budget >> 2)) stride = n_huge;
        const size_t slots = (size_t)n_bands * (size_t)stride;
        const int rc = alloc_group(ctx, {{"hband_geom", &ws.hband_geom, slots * sizeof(float4)}, {"hband_w", &ws.hband_w, slots * 2 * sizeof(float)},
                                         {"hband_count", (void **)&ws.hband_count, 256 * sizeof(int)}},
                                   {{&ws.hband_stride, stride}, {&ws.hband_bands, n_bands}});
        if (rc) return rc;
    }
    if (int rc = check_workspace(ctx)) return rc;
    hipStream_t st = ctx->stream;
    TSP_HIP(hipMemsetAsync(ws.hband_count, 0, 256 * sizeof(int), st));
    const unsigned grid = (unsigned)((n_huge + 1023) / 1024);
    hipLaunchKernelGGL((huge_band_fill_kernel<NW>), dim3(grid), dim3(256), 2 * n_bands * sizeof(int), st, huge_geom, huge_w, n_huge, ctx->R, n_bands,
                       (float4 *)ws.hband_geom, (float *)ws.hband_w, (long long)ws.hband_stride, ws.hband_count, (const long long *)nullptr);
    TSP_HIP(hipGetLastError());
    ta.geom = (const float4 *)ws.hband_geom; ta.w = (const float *)ws.hband_w;
    ta.bin_count = ws.hband_count; ta.band_stride = ws.hband_stride;
    return TSP_OK;
}

template <int MODE, int NACC, int W, int HR, int OCC>
static int launch_huge2(tsp_context *ctx, TileArgs ta, long long n_huge) {
    TSP_REQUIRE(ta.n_records < (1ll << 31), TSP_EINVAL, "%lld deferred footprints in one render block (the tile-gather kernels index them with 32 bits)", ta.n_records);
    const size_t smem = (size_t)((PT_ROWS * PT_STRIDE + 3) & ~3) * sizeof(float) + (H2T / 64) * 64 * sizeof(float2);
    const int tw = 2 * 64 * W, th = 2 * HR;
    const int htiles_x = (ctx->R + tw - 1) / tw, htiles_y = (ctx->R + th - 1) / th;
    const int htiles = htiles_x * htiles_y;
    const long long batches = (n_huge + 63) / 64;
    int split = ctx->huge_split;
    // many short workgroups: a wave lives ~1 ms at split 64 and the tail of the launch (tiles differ 10x in work)
    // cost 2.5 ms of 21; measured 64 -> 128: 21.9 -> 19.5 ms, 256: 19.2 ms, 512: 22.5 ms
    if (split <= 0) {
        split = std::max(1, (ctx->cu_count * 128 + htiles - 1) / htiles);
        // Fewer, longer workgroups for shorter record lists: every workgroup loads the kernel image and each of its waves walks its
        // share of the list at memory latency (64 records per step), so below ~2e6 records the scan outweighs the balance that many
        // short workgroups buy.  Round 5, 1024^2, workgroups per 128x64 tile (64x32 strips): 4.2e6 records 192 / 256 / 384 -> 33.2 /
        // 33.05 / 32.8 ms; 1.2e6: 128 / 192 / 256 / 384 -> 10.29 / 10.05 / 10.37 / 11.1; 5.3e5 (one of 8 shards of the 1e9 snapshot):
        // 64 / 96 / 128 / 192 / 256 -> 5.32 / 4.90 / 4.76 / 4.85 / 5.38; 3.4e5: 64 / 128 / 256 -> 4.24 / 3.42 / 4.45
        if (n_huge < (1ll << 16)) split = std::max(32, (int)((long long)split * n_huge >> 16));      // a small render block: in proportion
        else if (HR == 32 && NACC == 1) split = n_huge >= 2000000 ? split : (n_huge >= 1000000 ? (split * 3) / 4 : split / 2);
        else if (HR == 16 && NACC == 1) split = std::max(1, split / 2);      // (64x16 strips serve < 2.5e5 records: 32 / 64 / 128 per 128x32 tile -> 2.64 / 2.18 / 2.38 ms at 1.5e5)
        else if (HR == 16 && NACC == 2 && n_huge < 1000000) split = std::max(1, split / 2);      // two channels, 3.4e5 records: 64 / 128 / 192 / 256 -> 4.49 / 5.16 / 6.49 / 8.16 ms
    }
    split = (int)std::min<long long>(split, std::max<long long>(batches, 1));
    ta.split = split;
    ta.tiles_x = htiles_x;
    // the asm row walk (option h2_walk) exists for the single-channel strips at 8 waves/SIMD, the density frame's two shapes
    constexpr bool AW_BUILT = NACC == 1 && W == 1 && OCC == 8;
    with_bool<AW_BUILT>(ctx->h2_walk != 0, [&](auto AW) { with_bool(ta.count_frag != 0, [&](auto CNT) {
        hipLaunchKernelGGL((splat_huge2_kernel<MODE, NACC, W, HR, OCC, decltype(CNT)::value, decltype(AW)::value>), dim3(htiles * split), dim3(H2T), smem,
                           ctx->stream, ta);
    }); });
    TSP_HIP(hipGetLastError());
    return TSP_OK;
}

// ---------------------------------------------------------------------------------------------
// host side: strip shape and occupancy by mode and record count
// ---------------------------------------------------------------------------------------------
template <int MODE>
static int launch_gather_mode(tsp_context *ctx, TileArgs ta, bool second_channel, const float4 *huge_geom, const float *huge_w,
                              long long n_huge) {
    hipStream_t st = ctx->stream;
    int rc = TSP_OK;
    if (n_huge > 0) {
        ta.geom = huge_geom; ta.w = huge_w; ta.n_records = n_huge;
        TSP_REQUIRE(n_huge < (1ll << 31), TSP_EINVAL, "%lld deferred footprints in one render block (the tile-gather kernel indexes them with 32 bits)", n_huge);
        hipLaunchKernelGGL(huge_nonfinite_kernel<MODE>, dim3((unsigned)((n_huge + 1023) / 1024)), dim3(256), 0, st,
                           const_cast<float4 *>(huge_geom), huge_w, n_huge, second_channel ? 1 : 0, ta);
        TSP_HIP(hipGetLastError());
        if ((rc = bin_huge_records<(MODE == TSP_MODE_RGB) ? 2 : 1>(ctx, ta, huge_geom, huge_w, n_huge))) return rc;
        if (MODE == TSP_MODE_RGB) {
            // three accumulator sets: 96 VGPRs at 5 waves/SIMD (11.5 against 12.5 ms at 4 for the 64-128 px band of config 4)
            if (ctx->huge_variant == 4) rc = launch_huge2<MODE, 3, 1, 16, 4>(ctx, ta, n_huge);
            else rc = launch_huge2<MODE, 3, 1, 16, 5>(ctx, ta, n_huge);
        } else if (second_channel) {
            // 72 VGPRs at 7 waves/SIMD (24 B of scratch outside the row loop): 9.48 against 9.78 ms at 6 (80 VGPRs), 10.8 at 8 (spills)
            if (ctx->huge_variant == 4) rc = launch_huge2<MODE, 2, 1, 16, 4>(ctx, ta, n_huge);
            else rc = launch_huge2<MODE, 2, 1, 16, 7>(ctx, ta, n_huge);
        }
        else if (ctx->huge_variant == 2) rc = launch_huge2<MODE, 1, 1, 32, 6>(ctx, ta, n_huge);
        else if (ctx->huge_variant == 4) rc = launch_huge2<MODE, 1, 1, 16, 7>(ctx, ta, n_huge);
        else if (ctx->huge_variant == 5) rc = launch_huge2<MODE, 1, 1, 16, 8>(ctx, ta, n_huge);
        else if (ctx->huge_variant == 6) rc = launch_huge2<MODE, 1, 1, 32, 7>(ctx, ta, n_huge);
        // Density: 64x32 strips with the row factors fetched group by group -- half as many (footprint, strip) pairs to set up --
        // at 8 waves/SIMD (64 VGPRs): this kernel is latency-bound per wave, occupancy is what pays.  1.25e8 particles, records
        // 64-768 px: 10.20 / 9.86 / 9.59 ms at 6 / 7 / 8 waves (1e9: 28.7 / 26.9 / 26.9); 64x16 strips at 8: 10.7.  Round 5 re-measured
        // the cross-over with the workgroup count tuned per strip shape (launch_huge2): 64x32 strips win from ~2.5e5 records
        // (5.3e5: 4.76 against 5.47 ms; 3.4e5: 3.42 against 3.81; 1.5e5: 2.22 against 2.18)
        else if (ctx->huge_variant == 7 || (ctx->huge_variant == 1 && n_huge >= 250000)) rc = launch_huge2<MODE, 1, 1, 32, 8>(ctx, ta, n_huge);
        else rc = launch_huge2<MODE, 1, 1, 16, 8>(ctx, ta, n_huge);
        if (rc) return rc;
    }
    TSP_HIP(hipEventRecord(ctx->ev[EV_HUGE_END], st));
    return TSP_OK;
}

int launch_gather_kernels(tsp_context *ctx, TileArgs ta, int mode, bool second_channel, const float4 *huge_geom, const float *huge_w,
                          long long n_huge) {
    return with_mode(mode, [&](auto M) {      // (depth and rgb always carry their second channel)
        constexpr int MODE = decltype(M)::value;
        return launch_gather_mode<MODE>(ctx, ta, MODE != TSP_MODE_WEIGHTED || second_channel, huge_geom, huge_w, n_huge);
    });
}

}  // namespace tsp
