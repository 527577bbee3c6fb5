// tsp_pipeline.h -- what the translation units of the splat pipeline share: tile constants, the float64 atomic helpers,
// the argument block of the tile kernels, and the launchers of the tile-gather kernels (tsp_huge.hip, tsp_mid.hip).
#pragma once
#include <type_traits>

#include "tsp_internal.h"

namespace tsp {


#ifndef TSP_S_BLOCK
#define TSP_S_BLOCK 256
#endif
#ifndef TSP_S_KPT
#define TSP_S_KPT 2
#endif
constexpr int SBLOCK = TSP_S_BLOCK;  // threads per workgroup of kernel S
constexpr int SWAVES = SBLOCK / 64;
constexpr int KPT = TSP_S_KPT;       // particles per thread per chunk
constexpr int CHUNK = SBLOCK * KPT;  // particles per chunk
// LDS accumulators are DOUBLE: on gfx950 a conflict-free ds_add_f64 costs ~9 clk per wave-instruction
// (~11 clk more per extra lane on the same address) while ds_add_f32 costs ~190 (measured,
// tools/ubench/lds_partial.hip, lds_atomics.hip), and the sums gain precision.
#ifndef TSP_WIN1
#define TSP_WIN1 60
#define TSP_WIN2 44
#define TSP_WIN4 40
#endif
#ifndef TSP_S_OCC
#define TSP_S_OCC 5
#endif
// edge of kernel S's LDS window by the number of channels it holds (1: density, 2: weighted / depth, 4: rgb)
template <int WC> struct WinSize { static constexpr int value = (WC == 1) ? TSP_WIN1 : (WC == 2 ? TSP_WIN2 : TSP_WIN4); };

constexpr int HBAND_H = 64;          // image rows per band of the huge-record bins (kernel H2's tallest tile)

enum { CLS_NONE = 0, CLS_SMALL = 1, CLS_MID = 2, CLS_HUGE = 3 };

// the render target is accumulated in float64 (global_atomic_add_f64) and rounded to float32 once per
// tsp_render call, so cross-workgroup summation adds no float32 noise however many flushes hit a pixel
__device__ __forceinline__ void gatomic_add(double *addr, double v) {
#ifdef TSP_DEBUG_NO_FLUSH      // measurement aid: what the float64 flush atomics cost (the image is then empty)
    if (v == 123.456) *addr = v;
#else
    __hip_atomic_fetch_add(addr, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}
// top-left quadrants of the four mip levels of a mirror-symmetric kernel image (32^2 + 16^2 + 8^2 + 4^2 floats)
constexpr int MIPQ_TOTAL = 1024 + 256 + 64 + 16;
__device__ __forceinline__ int mipq_offset(int lvl) { return lvl == 0 ? 0 : (lvl == 1 ? 1024 : (lvl == 2 ? 1280 : 1344)); }

// DPP modifier: every lane reads the operand from lane t of its own quad
#define TSP_DPP_QUAD(t) "quad_perm:[" #t "," #t "," #t "," #t "] row_mask:0xf bank_mask:0xf"
// the FMAs of the strip walks of kernels H2, N and G (tsp_huge.hip, tsp_mid.hip): a row factor as the DPP operand / in place
template <int T> __device__ __forceinline__ void fmac_quad(float &acc, float rowval, float v) {
    static_assert(T >= 0 && T < 4, "quad lane");
    if (T == 0) asm volatile("v_fmac_f32_dpp %0, %1, %2 " TSP_DPP_QUAD(0) : "+v"(acc) : "v"(rowval), "v"(v));
    if (T == 1) asm volatile("v_fmac_f32_dpp %0, %1, %2 " TSP_DPP_QUAD(1) : "+v"(acc) : "v"(rowval), "v"(v));
    if (T == 2) asm volatile("v_fmac_f32_dpp %0, %1, %2 " TSP_DPP_QUAD(2) : "+v"(acc) : "v"(rowval), "v"(v));
    if (T == 3) asm volatile("v_fmac_f32_dpp %0, %1, %2 " TSP_DPP_QUAD(3) : "+v"(acc) : "v"(rowval), "v"(v));
}
template <int T> __device__ __forceinline__ float mul_quad(float rowval, float v) {
    float r;
    if (T == 0) asm volatile("v_mul_f32_dpp %0, %1, %2 " TSP_DPP_QUAD(0) : "=v"(r) : "v"(rowval), "v"(v));
    if (T == 1) asm volatile("v_mul_f32_dpp %0, %1, %2 " TSP_DPP_QUAD(1) : "=v"(r) : "v"(rowval), "v"(v));
    if (T == 2) asm volatile("v_mul_f32_dpp %0, %1, %2 " TSP_DPP_QUAD(2) : "=v"(r) : "v"(rowval), "v"(v));
    if (T == 3) asm volatile("v_mul_f32_dpp %0, %1, %2 " TSP_DPP_QUAD(3) : "=v"(r) : "v"(rowval), "v"(v));
    return r;
}
__device__ __forceinline__ void fmac_plain(float &acc, float x, float y) {     // tied operand: the accumulator stays in place
    asm volatile("v_fmac_f32_e32 %0, %1, %2" : "+v"(acc) : "v"(x), "v"(y));
}

// The test of a (record, strip) pair: the footprint square of g = (pcx, pcy, P, .) and the disc inscribed in it (disc_k2 > 0) reach the
// strip [sx0, sx1] x [sy0, sy1]; P <= 0 marks an empty slot.  Kernels G and H2 make it per pair, the strip bins of kernel N once per
// copy (tsp_mid.hip strip_hit): kernel N draws every record of a bin unasked, so there is one copy of the test.
// The disc test -- here and in kernel H2's row clip below, which is its second entry: the nearest point of the strip (of a pixel row's
// part of it) lies at (sdx, sdy) from the centre, at or beyond the radius sqrt(disc_k2) P = 0.5235 P (TileArgs::disc_k2; 0: no test).
// Why the one constant serves a strip rectangle and a pixel centre alike: the bilinear texels a pixel reads with a non-zero weight lie
// within one texel pitch (P / 64) of it per axis, so a pixel at >= (0.5 + sqrt(2) / 64) P = 0.5221 P from the centre takes them from
// >= 0.5 P = 2 h away, where they are exactly 0 when lut_zero_outside_disc holds.  (The clamp at the low edge reads texel 0 with weight 1
// and texel 1, farther off, with weight exactly 0; at the high edge it repeats texel 63.  tests/test_h2_chord_cpu.py checks this
// against the kernel image.)  Every pixel of a rectangle is at least as far as its nearest point.  0.5235 leaves 2.7e-3 of the radius
// for the float32 rounding of sdx, sdy and the products (~1e-7 each).
__device__ __forceinline__ bool reaches_strip(const float4 g, float sx0, float sx1, float sy0, float sy1, float disc_k2) {
    const float half = 0.5f * g.z;
    const float sdx = fmaxf(fmaxf(sx0 - g.x, g.x - sx1), 0.0f), sdy = fmaxf(fmaxf(sy0 - g.y, g.y - sy1), 0.0f);
    return g.z > 0.0f && sdx < half && sdy < half && !(disc_k2 > 0.0f && sdx * sdx + sdy * sdy >= disc_k2 * g.z * g.z);
}
// The second entry, kernel H2's row clip: the same comparison, sdx * sdx + d * d >= disc_k2 * P * P, for the pixel row whose centre is
// d from the footprint's centre in y (sdy = |d|: the row's part of the strip is a segment) -- the row's chord of the disc misses the
// strip's columns, all its pixels read zero texels.  The kernel makes the test for 64 rows at once, so the part that does not depend on
// the row is formed once per record and strip,
//     chord_limit = disc_k2 P P - sdx sdx,     row outside  <=>  d d >= chord_limit,
// which is that comparison with sdx sdx moved across (one more rounding of ~1e-7 P P against the margin of 1.5e-3 P P above).  Without
// a disc (disc_k2 = 0) the limit is +inf: no finite d is outside.  A NaN limit (inf - inf at widths beyond 1e19 px) clears nothing.
// (reaches_strip keeps its own text of sdx and of the comparison: called through shared helpers it compiles to other machine code in
// kernels N and G, which this clip does not concern.)
__device__ __forceinline__ float chord_limit(float pcx, float P, float sx0, float sx1, float disc_k2) {
    const float sdx = fmaxf(fmaxf(sx0 - pcx, pcx - sx1), 0.0f);
    return disc_k2 > 0.0f ? disc_k2 * P * P - sdx * sdx : __builtin_inff();
}
__device__ __forceinline__ bool row_outside_chord(float d, float limit) { return d * d >= limit; }
// Margin of the binning passes around a footprint's extent c -+ half: one pixel plus two ulps of the coordinate, so that it still
// covers the rounding of c -+ half at any magnitude (float rounding can only add a bin, never drop one)
__device__ __forceinline__ float bin_margin(float c, float half) { return 1.0f + 2.4e-7f * (__builtin_fabsf(c) + half); }

constexpr int H2T = 256;             // threads per workgroup of kernels H2, N and G: 4 waves (H2: 2 x 2 strips sharing one pair table)

__device__ __forceinline__ void latomic_add(double *addr, float v) {
    __hip_atomic_fetch_add(addr, (double)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

#ifndef TSP_FOLD_EVERY
#define TSP_FOLD_EVERY 2048    // footprints a float32 accumulator of kernels N / G / H2 holds before it goes to the float64 target (512 until the end of round 5)
#endif
#ifndef TSP_HDEAL
#define TSP_HDEAL 16
#endif
constexpr int HDEAL = TSP_HDEAL;            // records per dealing run of the tile-gather kernels (1: 13.6 ms, 4: 10.67, 16: 10.49, 64: 10.71 for H2)

struct TileArgs {
    const float4 *geom; const float *w;
    long long n_records;
    Camera cam;
    const float *mips;
    double *img;
    Counters *cnt;
    int tiles_x, split;
    int count_frag;
    float disc_k2;     // (0.5235)^2 when the LUT is zero outside the inscribed disc (exact corner culling), else 0
    // The records in bins; a bin is an image band for kernel H2 and a strip for kernels N and G.
    // kernel H2 (huge_band_fill_kernel): band b (rows [b, b + 1) * HBAND_H) holds bin_count[b] records at geom + b * band_stride (w
    // likewise), bin_base unused; bin_count = nullptr: one list for every tile (geom, n_records)
    // kernels N and G (bin_mid_records): exact-size bins, strip t holds bin_count[t] records from record bin_base[t] on, band_stride unused
    const int *bin_count; long long band_stride; const long long *bin_base;
    // kernels N and G: wave i draws work item i = item_records consecutive records of strip item_tile[i]'s bin (that strip's items start
    // at item_base[strip]; item_base[n_tiles] = their number)
    int n_tiles; const int *item_tile; const int *item_base; int item_records;      // item_records: records per work item (a power of two)
    // kernel H2's row clip (chord_limit): disc_k2 with option h2_chord on, else 0 (every row of the square is walked).  Last, so that
    // the kernels that do not read it find every other argument where it was
    float chord_k2;
};

// A run-time flag / mode as a compile-time constant: f receives std::true_type or std::false_type (a std::integral_constant of
// the mode) and names its template arguments with decltype(x)::value.  with_bool<false> passes false_type whatever the flag:
// for a variant that is not built.
template <bool BUILT = true, class F> auto with_bool(bool b, F &&f) {
    if constexpr (BUILT) { if (b) return f(std::true_type{}); }
    return f(std::false_type{});
}
template <class F> int with_mode(int mode, F &&f) {
    switch (mode) {
        case TSP_MODE_WEIGHTED: return f(std::integral_constant<int, TSP_MODE_WEIGHTED>{});
        case TSP_MODE_DEPTH: return f(std::integral_constant<int, TSP_MODE_DEPTH>{});
        case TSP_MODE_RGB: return f(std::integral_constant<int, TSP_MODE_RGB>{});
    }
    set_error("bad mode %d", mode);
    return TSP_EINVAL;
}

// Kernel H2 (tsp_huge.hip) for the footprints >= 64 px of one render block (the records kernel S appended to the huge list).
// Records EV_HUGE_END after the launch (per-kernel time: EV_HUGE_BEGIN .. EV_HUGE_END).
int launch_gather_kernels(tsp_context *ctx, TileArgs ta, int mode, bool second_channel, const float4 *huge_geom, const float *huge_w,
                          long long n_huge);

// Kernels N and G (tsp_mid.hip): the MID records of one render block as a register gather; launched on `st`.
int launch_mid_gather(tsp_context *ctx, TileArgs ta, int mode, bool second_channel, const float4 *mid_geom, const float *mid_w,
                      long long n_mid, hipStream_t st);

}  // namespace tsp
