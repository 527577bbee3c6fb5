// tsp_math.h -- device-side arithmetic of the splat + colormap path (gfx950).
//
// The semantics follow the reference's shaders: vertex stage src/topsy/shaders/sph.wgsl:54-83,
// fragment stage :139-146,161-165, sampler src/topsy/sph.py:396-426, colormap
// src/topsy/shaders/colormap.wgsl:75-159.  Coverage and nearest-texel decisions use ONE fixed
// float32 operation order (documented in DESIGN.md "canonical arithmetic") so that discrete
// decisions are reproducible; this translation unit must be built with -ffp-contract=off, and
// fused multiply-adds appear only where written explicitly (__builtin_fmaf) in value-only code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tsp {

constexpr float P_BILINEAR = 64.0f;               // P >= 64 px  -> LOD <= 0 -> mag filter (bilinear, mip 0)
constexpr float P_L0 = 45.254833995939045f;       // 64 / 2^0.5 : P >  -> nearest, mip 0
constexpr float P_L1 = 22.627416997969522f;       // 64 / 2^1.5 : P >  -> mip 1
constexpr float P_L2 = 11.313708498984761f;       // 64 / 2^2.5 : P >  -> mip 2, else mip 3
constexpr int MIP_TOTAL = 5440;                   // 64^2 + 32^2 + 16^2 + 8^2

struct Camera {          // passed by value to kernels (lives in SGPRs / kernarg)
    float m[12];         // first three rows of the row-major 4x4: clip = M * (x,y,z,1)
    float sf;            // 1/scale
    float Rf;            // resolution as float
    float halfR;         // 0.5 * R
    int R;
};

struct Proj {            // a particle in pixel units
    float pcx, pcy;      // centre: column / row coordinate (pixel i centre = i + 0.5)
    float P;             // quad width in pixels
    float half;          // 0.5 * P
    float invP;          // 1 / P
    float cz;            // clip-space z
    bool keep;
};

template <bool WITH_INVP = true>
__device__ __forceinline__ Proj project(const Camera &c, float x, float y, float z, float h) {
    Proj r;
    const float cx = ((c.m[0] * x + c.m[1] * y) + c.m[2] * z) + c.m[3];
    const float cy = ((c.m[4] * x + c.m[5] * y) + c.m[6] * z) + c.m[7];
    r.cz = ((c.m[8] * x + c.m[9] * y) + c.m[10] * z) + c.m[11];
    const float s = (c.sf * h) * 2.0f;               // sph.wgsl:58  scale_factor * pos.w * 2
    r.P = s * c.Rf;
    r.half = 0.5f * r.P;
    r.pcx = (cx + 1.0f) * c.halfR;
    r.pcy = (1.0f - cy) * c.halfR;
    r.invP = WITH_INVP ? 1.0f / r.P : 0.0f;      // (kernel S forms it only in the waves that rasterise)
    // fixed-function clip: 0 <= z <= 1; non-finite geometry draws nothing
    r.keep = (r.cz >= 0.0f) && (r.cz <= 1.0f) && (r.P > 0.0f) && (r.P < __builtin_inff()) &&
             (__builtin_fabsf(r.pcx) < __builtin_inff()) && (__builtin_fabsf(r.pcy) < __builtin_inff());
    return r;
}

// Exact interval [lo, hi] of covered pixels along one axis, clipped to the image; lo > hi when empty.
// Coverage is the canonical test |(i + 0.5) - pc| < half evaluated in float32; it holds on a contiguous
// run of pixels whose ends lie within one pixel of the real-arithmetic bounds, so three candidate
// tests per side decide it without loops or branches.
__device__ __forceinline__ bool covers(float pc, float half, float i) {
    return __builtin_fabsf((i + 0.5f) - pc) < half;
}
__device__ __forceinline__ void cover_range(float pc, float half, int R, int &lo, int &hi) {
    const float l0 = __builtin_floorf(pc - half - 0.5f) + 1.0f;    // first covered pixel in real arithmetic
    const float h0 = __builtin_ceilf(pc + half - 0.5f) - 1.0f;     // last covered pixel in real arithmetic
    float l = covers(pc, half, l0 - 1.0f) ? l0 - 1.0f : (covers(pc, half, l0) ? l0 : l0 + 1.0f);
    float h = covers(pc, half, h0 + 1.0f) ? h0 + 1.0f : (covers(pc, half, h0) ? h0 : h0 - 1.0f);
    // clip to [0, R-1] while still in float (the bounds may be far outside the int range)
    l = l < 0.0f ? 0.0f : l;
    const float rm = (float)(R - 1);
    h = h > rm ? rm : h;
    // an empty or fully clipped run must come out as lo > hi
    const bool empty = !(l <= h);
    lo = empty ? 1 : (int)l;
    hi = empty ? 0 : (int)h;
}

__device__ __forceinline__ int level_for(float P) {   // -1 = bilinear on mip 0
    return P >= P_BILINEAR ? -1 : (P > P_L0 ? 0 : (P > P_L1 ? 1 : (P > P_L2 ? 2 : 3)));
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ int nearest_index(float u, int n) {
    return clampi((int)__builtin_floorf(u * (float)n), 0, n - 1);
}

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "libtopsy_splat is written for gfx950 (MI355X) only: its inline assembly uses that target's instructions (v_cvt_flr_i32_f32, DPP, ds_add_f64)"
#endif
// clampi((int)floorf(x), 0, hi) in two instructions instead of four: v_cvt_flr_i32_f32 converts with floor rounding (and saturates
// like the plain conversion), v_med3_i32 clamps.  The same integers for every x; `hi` wave-uniform (_s) or per lane (_v).
__device__ __forceinline__ int floor_clamp_s(float x, int hi) {
    int r;
    asm("v_cvt_flr_i32_f32 %0, %1\n\tv_med3_i32 %0, %0, 0, %2" : "=&v"(r) : "v"(x), "s"(hi));
    return r;
}
__device__ __forceinline__ int floor_clamp_v(float x, int hi) {
    int r;
    asm("v_cvt_flr_i32_f32 %0, %1\n\tv_med3_i32 %0, %0, 0, %2" : "=&v"(r) : "v"(x), "v"(hi));
    return r;
}

__device__ __forceinline__ int mip_offset(int lvl) {  // 0, 4096, 5120, 5376
    return lvl == 0 ? 0 : (lvl == 1 ? 4096 : (lvl == 2 ? 5120 : 5376));
}

struct AxisB {  // bilinear addressing along one axis
    int i0, i1;
    float f;
};
__device__ __forceinline__ AxisB axis_bilinear(float u) {
    AxisB a;
    const float tu = u * 64.0f - 0.5f;
    const float x0 = __builtin_floorf(tu);
    a.f = tu - x0;
    const int ix = (int)x0;
    a.i0 = clampi(ix, 0, 63);
    a.i1 = clampi(ix + 1, 0, 63);
    return a;
}

// Kernel sample for pixel offset (dx, dy) from the particle centre.  T = mip pyramid (LDS or global).
template <typename LUT>
__device__ __forceinline__ float sample_kernel(const LUT &T, const Proj &p, int lvl, float dx, float dy) {
    const float u = (dx + p.half) * p.invP;
    const float v = (dy + p.half) * p.invP;
    if (lvl < 0) {
        const AxisB ax = axis_bilinear(u), ay = axis_bilinear(v);
        const float gx = 1.0f - ax.f, gy = 1.0f - ay.f;
        const float top = T[ay.i0 * 64 + ax.i0] * gx + T[ay.i0 * 64 + ax.i1] * ax.f;
        const float bot = T[ay.i1 * 64 + ax.i0] * gx + T[ay.i1 * 64 + ax.i1] * ax.f;
        return top * gy + bot * ay.f;
    }
    const int n = 64 >> lvl;
    return T[mip_offset(lvl) + nearest_index(v, n) * n + nearest_index(u, n)];
}

// The same with a selectable sampling rule (TSP_SAMPLE_*): 0 = "O1" as above; 1 = bilinear on
// mip 0 whatever the footprint width; 2 = bilinear within the mip the rounded LOD selects.  Diagnostic only.
template <typename LUT>
__device__ __forceinline__ float sample_kernel_rule(const LUT &T, const Proj &p, float dx, float dy, int rule) {
    int lvl = level_for(p.P);
    if (rule == 0 || (rule != 1 && lvl < 0)) return sample_kernel(T, p, lvl, dx, dy);
    if (rule == 1) return sample_kernel(T, p, -1, dx, dy);
    const int n = 64 >> lvl, off = mip_offset(lvl);
    const float tu = ((dx + p.half) * p.invP) * (float)n - 0.5f, tv = ((dy + p.half) * p.invP) * (float)n - 0.5f;
    const float x0 = __builtin_floorf(tu), y0 = __builtin_floorf(tv);
    const float fx = tu - x0, fy = tv - y0, gx = 1.0f - fx, gy = 1.0f - fy;
    const int ix0 = clampi((int)x0, 0, n - 1), ix1 = clampi((int)x0 + 1, 0, n - 1);
    const int iy0 = clampi((int)y0, 0, n - 1), iy1 = clampi((int)y0 + 1, 0, n - 1);
    const float top = T[off + iy0 * n + ix0] * gx + T[off + iy0 * n + ix1] * fx;
    const float bot = T[off + iy1 * n + ix0] * gx + T[off + iy1 * n + ix1] * fx;
    return top * gy + bot * fy;
}

// ------------------------------------------------------------------------------------------
// canonical float32 log / exp / pow (colormap).  WGSL leaves log()/pow() precision
// implementation-defined; the path fixes one algorithm so the uint8 image is reproducible.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float canon_logf(float x) {
    if (x != x || x < 0.0f) return __builtin_nanf("");
    if (x == 0.0f) return -__builtin_inff();
    if (x == __builtin_inff()) return x;
    int eadj = 0;
    if (x < 1.17549435e-38f) { x = x * 8388608.0f; eadj = -23; }
    const int bits = __float_as_int(x);
    int e = ((bits >> 23) & 0xff) - 127 + eadj;
    float m = __int_as_float((bits & 0x007fffff) | 0x3f800000);
    if (m > 1.41421354f) { m = m * 0.5f; e += 1; }
    const float s = (m - 1.0f) / (m + 1.0f);
    const float z = s * s;
    float p = 0.18181819f;
    p = p * z + 0.22222222f;
    p = p * z + 0.2857143f;
    p = p * z + 0.4f;
    p = p * z + 0.6666667f;
    const float lm = (s + s) + (s * z) * p;
    const float ef = (float)e;
    return (ef * 0.693359375f + lm) + ef * -2.12194440e-4f;
}

__device__ __forceinline__ float canon_expf(float y) {
    if (y != y) return y;
    if (y > 88.72f) return __builtin_inff();
    if (y < -103.9f) return 0.0f;
    const float nf = __builtin_floorf(y * 1.44269504f + 0.5f);
    const float r = (y - nf * 0.693359375f) - nf * -2.12194440e-4f;
    float p = 1.9841270e-4f;
    p = p * r + 1.3888889e-3f;
    p = p * r + 8.3333333e-3f;
    p = p * r + 4.1666667e-2f;
    p = p * r + 0.16666667f;
    p = p * r + 0.5f;
    p = p * r + 1.0f;
    p = p * r + 1.0f;
    const int n = (int)nf;
    const int n1 = clampi(n, -126, 127);
    const int n2 = clampi(n - n1, -126, 127);
    return (p * __int_as_float((n1 + 127) << 23)) * __int_as_float((n2 + 127) << 23);
}

__device__ __forceinline__ float canon_log10f(float x) { return canon_logf(x) / 2.30258509f; }  // colormap.wgsl:75-77

__device__ __forceinline__ float canon_powf(float x, float g) {
    if (g == 1.0f) return x;
    if (x == 0.0f && g > 0.0f) return 0.0f;
    if (g == 0.0f && x == x) return 1.0f;
    return canon_expf(g * canon_logf(x));
}

__device__ __forceinline__ uint32_t unorm8(float c) {   // rgba8unorm store: round(255 * clamp(c))
    c = (c != c) ? 0.0f : c;
    c = c < 0.0f ? 0.0f : (c > 1.0f ? 1.0f : c);
    return (uint32_t)__builtin_floorf(c * 255.0f + 0.5f);
}

// ------------------------------------------------------------------------------------------
// the per-pixel maps of the colormap post-pass (colormap.wgsl :91-159), shared by kernels B / B' (tsp_colormap.hip) and the
// frame composition (tsp_present.hip); `range` = vmax - vmin, formed once by the caller
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t map_scalar_rgba8(float r, float g, const float4 *__restrict__ lut, int n_lut, float vmin,
                                                     float range, int log_scale, int weighted) {
    float v = weighted ? g / r : r;
    if (log_scale) v = canon_log10f(v);
    float t = (v - vmin) / range;
    t = (t != t) ? 0.0f : t;
    t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
    const float c = t * (float)n_lut - 0.5f;
    const float c0 = __builtin_floorf(c);
    const float f = c - c0;
    const int i0 = clampi((int)c0, 0, n_lut - 1), i1 = clampi((int)c0 + 1, 0, n_lut - 1);
    const float gq = 1.0f - f;
    const float4 a = lut[i0], b = lut[i1];
    const uint32_t R8 = unorm8(a.x * gq + b.x * f);
    const uint32_t G8 = unorm8(a.y * gq + b.y * f);
    const uint32_t B8 = unorm8(a.z * gq + b.z * f);
    const uint32_t A8 = unorm8(a.w * gq + b.w * f);
    return R8 | (G8 << 8) | (B8 << 16) | (A8 << 24);
}

__device__ __forceinline__ uint32_t map_bivariate_rgba8(float r, float g, const float4 *__restrict__ lut, int n, float vmin,
                                                        float range, float dvmin, float drange, int log_scale, int weighted) {
    float x = (canon_log10f(r) - dvmin) / drange;
    float y = weighted ? g / r : r;
    if (log_scale) y = canon_log10f(y);
    y = (y - vmin) / range;
    x = (x != x || x < 0.0f) ? 0.0f : (x > 1.0f ? 1.0f : x);
    y = (y != y || y < 0.0f) ? 0.0f : (y > 1.0f ? 1.0f : y);
    const float cx = x * (float)n - 0.5f, cy = y * (float)n - 0.5f;
    const float x0 = __builtin_floorf(cx), y0 = __builtin_floorf(cy);
    const float fx = cx - x0, fy = cy - y0, gx = 1.0f - fx, gy = 1.0f - fy;
    const int i0 = clampi((int)x0, 0, n - 1), i1 = clampi((int)x0 + 1, 0, n - 1);
    const int j0 = clampi((int)y0, 0, n - 1), j1 = clampi((int)y0 + 1, 0, n - 1);
    const float4 a = lut[(size_t)j0 * n + i0], b = lut[(size_t)j0 * n + i1];
    const float4 c = lut[(size_t)j1 * n + i0], d = lut[(size_t)j1 * n + i1];
    const uint32_t R8 = unorm8((a.x * gx + b.x * fx) * gy + (c.x * gx + d.x * fx) * fy);
    const uint32_t G8 = unorm8((a.y * gx + b.y * fx) * gy + (c.y * gx + d.y * fx) * fy);
    const uint32_t B8 = unorm8((a.z * gx + b.z * fx) * gy + (c.z * gx + d.z * fx) * fy);
    const uint32_t A8 = unorm8((a.w * gx + b.w * fx) * gy + (c.w * gx + d.w * fx) * fy);
    return R8 | (G8 << 8) | (B8 << 16) | (A8 << 24);
}

// one channel of fragment_main_tri: gamma_map(log10(value)) (colormap.wgsl:131-159), unclamped above (the HDR canvas value)
__device__ __forceinline__ float map_rgb_channel(float value, float vmin, float range, float gamma) {
    const float v = canon_log10f(value);
    float x = (v - vmin) / range;
    x = (x != x) ? 0.0f : x;
    x = x < 0.0f ? 0.0f : x;
    return canon_powf(x, gamma);
}

// ------------------------------------------------------------------------------------------
// the per-pixel moments of a kinematic image (include/topsy_splat.h "Kinematic maps"), shared by tsp_velocity_moments' kernel
// (tsp_kinematics.hip), the moment bases of the frame composition (tsp_present.hip) and tsp_moment_sort (tsp_data.hip): from the
// sums S, A, B in float64, every operation a correctly rounded IEEE one, mean = A / S and sigma = sqrt(max(B / S - mean^2, 0)),
// each rounded to float32; both NaN unless S > 0 and S, A, B are finite
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ bool finite_f32(float x) { return __builtin_fabsf(x) < __builtin_inff(); }   // false for NaN

__device__ __forceinline__ void velocity_moments_f32(float S32, float A32, float B32, float &mean, float &sigma) {
    mean = sigma = __uint_as_float(0x7fc00000u);
    if (S32 > 0.0f && finite_f32(S32) && finite_f32(A32) && finite_f32(B32)) {
        const double S = (double)S32, A = (double)A32, B = (double)B32;
        const double mu = __ddiv_rn(A, S);
        double var = __ddiv_rn(B, S) - mu * mu;
        if (var < 0.0) var = 0.0;
        mean = (float)mu;
        sigma = (float)__dsqrt_rn(var);
    }
}

// ------------------------------------------------------------------------------------------
// the lit shading of the surface map (surface.wgsl:28-123), shared by tsp_surface_present's shading kernel (tsp_surface.hip)
// and the surface base of the frame composition (tsp_present.hip)
// ------------------------------------------------------------------------------------------
struct ShadeParams {
    float depth_scale, vmin, vmax, nz;      // nz: the normal's z before normalisation, texelSize.x = 1 / (image or canvas width)
    float L[3], lc[3], amb[3];
    int weighted, log_scale, n_lut;
};

// q: the material quantity of the pixel; Dc and its four neighbours: depths already multiplied by depth_scale
__device__ __forceinline__ uint32_t surface_shade_rgba8(float q, float Dc, float Dl, float Dr, float Du, float Dd, const ShadeParams &sp,
                                                        const float4 *__restrict__ lut) {
    const float nx0 = -((Dr - Dl) * 0.5f), ny0 = -((Dd - Du) * 0.5f), nz0 = sp.nz;
    const float len = sqrtf((nx0 * nx0 + ny0 * ny0) + nz0 * nz0);
    const float nx = nx0 / len, ny = ny0 / len, nz = nz0 / len;
    float ndl = (nx * sp.L[0] + ny * sp.L[1]) + nz * sp.L[2];
    ndl = ndl > 0.0f ? ndl : 0.0f;
    float mat[3] = {1.0f, 1.0f, 1.0f};
    if (sp.weighted) {
        float v = q;
        if (sp.log_scale) v = canon_log10f(v);
        float u = (v - sp.vmin) / (sp.vmax - sp.vmin);
        u = (u != u) ? 0.0f : u;
        u = u < 0.0f ? 0.0f : (u > 1.0f ? 1.0f : u);
        const float cc = u * (float)sp.n_lut - 0.5f;
        const float c0 = __builtin_floorf(cc);
        const float f = cc - c0;
        const int i0 = clampi((int)c0, 0, sp.n_lut - 1), i1 = clampi((int)c0 + 1, 0, sp.n_lut - 1);
        const float g = 1.0f - f;
        const float4 a = lut[i0], b = lut[i1];
        mat[0] = a.x * g + b.x * f;
        mat[1] = a.y * g + b.y * f;
        mat[2] = a.z * g + b.z * f;
    }
    float k = Dc < 0.0f ? 0.0f : (Dc > 0.5f ? 0.5f : Dc);
    k = k * 2.0f;
    uint32_t rgb[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float diffuse = (sp.lc[c] * ndl) * mat[c];
        const float ambient = sp.amb[c] * mat[c];
        rgb[c] = unorm8((diffuse + ambient) * k);
    }
    return rgb[0] | (rgb[1] << 8) | (rgb[2] << 16) | (255u << 24);
}

}  // namespace tsp
