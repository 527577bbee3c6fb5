// tsp_present.hip -- frame composition (kernel P): the presentation image colormapped onto a W x H canvas, then the layers.
//
// Reference: VisualizerBase._encode_draw / get_presentation_image (src/topsy/visualizer.py:367-384,480-491), the aspect squash
// and sampler of the colormap pass (shaders/colormap.wgsl:42-73, colormap/implementation.py:240-325), textured overlays
// (shaders/overlay.wgsl, overlay.py) and line sets (shaders/line.wgsl, line.py:12-35).  The canonical arithmetic is written
// out in include/topsy_splat.h "Frame composition"; tests/present_ref.py restates it in numpy.
//
// One pixel per lane, one pass: the lane samples the float32 image, maps it with the colormap arithmetic of tsp_math.h, then
// applies the primitives in draw order, quantising after each as the 8-bit (or float16) target does.  The host turns every
// layer into primitives (pixel-space rectangles, line quads with their edge functions) and a conservative pixel bounding box;
// a wave covers 64 pixels of one row, so a primitive whose box misses that row segment is skipped on a uniform branch.  The
// frame is read once and written once; the textures and the table stay in L2.
//
// Surface base (tsp_present_surface): the kernel is a template over its base, so the lit surface is an instantiation of its own
// and the code of the four maps is what it was.  The (q, depth) image is filtered into a per-call scratch by the bilateral kernel
// of tsp_surface.hip; every lane then samples the filtered image five times (centre and one canvas pixel to each side, the base
// layer's sampling rule on both channels) and shades with the arithmetic of tsp_surface_present (surface_shade_rgba8,
// tsp_math.h).  The filtered image is 8 bytes per texel and stays in L2.
//
// Moment bases (TSP_PRESENT_MOMENT_MEAN / _SIGMA): one more instantiation.  Every lane samples the four channels (S, A, B, n) of
// the kinematic image by the base layer's rule (16 bytes per texel, up to four texels), forms the moment of the sampled sums in
// float64 (velocity_moments_f32, tsp_math.h: the function tsp_velocity_moments' kernel calls) and maps it with the scalar map.
//
// Movie frames (tsp_present_yuv420): a second, small kernel converts the composed RGBA8 staging frame to I420 planes on the
// device, so the composition kernel is the same and only 1.5 bytes per pixel are copied out.
#include "tsp_internal.h"

#include <hip/hip_fp16.h>

#include <cmath>
#include <type_traits>

namespace tsp {

namespace {

constexpr int MAX_PRIMS = 65536;
constexpr int MAX_LAYERS = 1024;
constexpr int MAX_INSTANCES = 128;      // Overlay.MAX_INSTANCES (overlay.py)
constexpr int MAX_SIDE = 16384;

struct PresentPrim {            // one textured-quad instance or one line segment
    int kind;                   // TSP_LAYER_QUAD / TSP_LAYER_LINES
    int bx0, bx1, by0, by1;     // pixels the primitive may cover (inclusive; conservative), bx0 > bx1 when none
    int tex_off, tw, th;        // quad: first texel in the texture buffer, texture size
    float X0, X1, Y0, Y1;       // quad: pixel-space rectangle, [X0, X1) x [Y0, Y1)
    float u0, du, v0, dv, weight;
    float px[4], py[4];         // line: corners in pixels, in an order that puts the inside at E > 0
    float ex[4], ey[4];         // line: edge vectors
    int closed;                 // line: bit e set = edge e is a top or left edge (E == 0 counts as inside)
    float color[4];
};

struct BaseArgs {
    const float *img;
    int R, C, W, H;
    float k, ox, oy;
    int linear;                 // k <= 1
    int map;                    // TSP_PRESENT_*
    const float4 *lut;          // scalar: 1-D LUT; bivariate: the n x n LUT
    int n_lut;
    float vmin, range, dvmin, drange, gamma;
    int log_scale, weighted;
};

struct Tap {
    int i0, i1;
    float f;
};
// linear filter, clamp-to-edge, along one axis of n texels; t = texel-space coordinate (texel i spans [i, i + 1))
__device__ __forceinline__ Tap linear_tap(float t, int n) {
    Tap a;
    const float tx = t - 0.5f;
    const float x0 = __builtin_floorf(tx);
    a.f = tx - x0;
    a.i0 = clampi((int)x0, 0, n - 1);
    a.i1 = clampi((int)x0 + 1, 0, n - 1);
    return a;
}
__device__ __forceinline__ float lerp0(float a, float b, float f) { return f == 0.0f ? a : a * (1.0f - f) + b * f; }
__device__ __forceinline__ float4 lerp4(const float4 &a, const float4 &b, float f) {
    return make_float4(lerp0(a.x, b.x, f), lerp0(a.y, b.y, f), lerp0(a.z, b.z, f), lerp0(a.w, b.w, f));
}
__device__ __forceinline__ float4 load_texel(const float *img, int C, int64_t idx) {
    if (C == 4) return reinterpret_cast<const float4 *>(img)[idx];
    const float2 v = reinterpret_cast<const float2 *>(img)[idx];
    return make_float4(v.x, v.y, 0.0f, 0.0f);
}
__device__ __forceinline__ float4 bilinear(const float *img, int C, int w, int h, float tx, float ty) {
    const Tap ax = linear_tap(tx, w), ay = linear_tap(ty, h);
    const float4 a = load_texel(img, C, (int64_t)ay.i0 * w + ax.i0), b = load_texel(img, C, (int64_t)ay.i0 * w + ax.i1);
    const float4 c = load_texel(img, C, (int64_t)ay.i1 * w + ax.i0), d = load_texel(img, C, (int64_t)ay.i1 * w + ax.i1);
    return lerp4(lerp4(a, b, ax.f), lerp4(c, d, ax.f), ay.f);
}

__device__ __forceinline__ float unorm_to_float(uint32_t px, int sh) { return (float)((px >> sh) & 255u) / 255.0f; }

// out = src * src.a + dst * (1 - src.a), colour and alpha (overlay.py _blending)
__device__ __forceinline__ float blend1(float s, float sa, float d, float oma) { return s * sa + d * oma; }

// ---- surface base: the filtered (q, depth) image F shaded from five samples per canvas pixel (include/topsy_splat.h
// "tsp_present_surface"), on the rgba8unorm canvas
struct SurfaceArgs {
    const float2 *F;
    int R, W, H;
    float k, ox, oy;
    float du, dv;               // one canvas pixel in texels of F: (float)R / (float)W, (float)R / (float)H
    int linear;                 // k <= 1
    ShadeParams sp;
    const float4 *lut;          // the material's 1-D LUT (weighted_average)
};

// both channels of F at texel-space (tx, ty) by the base layer's rule
__device__ __forceinline__ float2 sample_surface(const SurfaceArgs &a, float tx, float ty) {
    if (a.linear) {
        const Tap sx = linear_tap(tx, a.R), sy = linear_tap(ty, a.R);
        const float2 p = a.F[(int64_t)sy.i0 * a.R + sx.i0], q = a.F[(int64_t)sy.i0 * a.R + sx.i1];
        const float2 r = a.F[(int64_t)sy.i1 * a.R + sx.i0], s = a.F[(int64_t)sy.i1 * a.R + sx.i1];
        return make_float2(lerp0(lerp0(p.x, q.x, sx.f), lerp0(r.x, s.x, sx.f), sy.f),
                           lerp0(lerp0(p.y, q.y, sx.f), lerp0(r.y, s.y, sx.f), sy.f));
    }
    const int i = clampi((int)__builtin_floorf(tx), 0, a.R - 1), j = clampi((int)__builtin_floorf(ty), 0, a.R - 1);
    return a.F[(int64_t)j * a.R + i];
}

__device__ __forceinline__ uint32_t surface_base_rgba8(const SurfaceArgs &a, float xc, float yc) {
    const float ax = (xc - a.ox) * a.k, ay = (yc - a.oy) * a.k;
    const float2 c = sample_surface(a, ax, ay);
    const float Dc = c.y * a.sp.depth_scale;
    const float Dl = sample_surface(a, ax - a.du, ay).y * a.sp.depth_scale;
    const float Dr = sample_surface(a, ax + a.du, ay).y * a.sp.depth_scale;
    const float Du = sample_surface(a, ax, ay - a.dv).y * a.sp.depth_scale;
    const float Dd = sample_surface(a, ax, ay + a.dv).y * a.sp.depth_scale;
    return surface_shade_rgba8(c.x, Dc, Dl, Dr, Du, Dd, a.sp, a.lut);
}

// ---- moment bases (TSP_PRESENT_MOMENT_MEAN / _SIGMA): the four raw channels (S, A, B, n) of the kinematic image sampled by the
// base layer's rule, the moment formed from the sampled sums (velocity_moments_f32, tsp_math.h: the mass-weighted interpolation),
// then the scalar map, unweighted, on the rgba8unorm canvas
struct MomentArgs {
    const float *img;           // R x R x 4
    int R, W, H;
    float k, ox, oy;
    int linear;                 // k <= 1
    int sigma;                  // 0: the mean, 1: the dispersion
    const float4 *lut;
    int n_lut;
    float vmin, range;
    int log_scale;
};

__device__ __forceinline__ uint32_t moment_base_rgba8(const MomentArgs &a, float xc, float yc) {
    const float ax = (xc - a.ox) * a.k, ay = (yc - a.oy) * a.k;
    float4 v;
    if (a.linear) {
        v = bilinear(a.img, 4, a.R, a.R, ax, ay);
    } else {
        const int i = clampi((int)__builtin_floorf(ax), 0, a.R - 1), j = clampi((int)__builtin_floorf(ay), 0, a.R - 1);
        v = load_texel(a.img, 4, (int64_t)j * a.R + i);
    }
    float mean, sigma;
    velocity_moments_f32(v.x, v.y, v.z, mean, sigma);
    return map_scalar_rgba8(a.sigma ? sigma : mean, 0.0f, a.lut, a.n_lut, a.vmin, a.range, a.log_scale, 0);
}

// One pixel per lane: its base colour (Base = BaseArgs: the four maps; SurfaceArgs: the lit surface; MomentArgs: a moment map of
// the kinematic image; the last two with HDR = false), the primitives in draw order, the single write.
template <bool HDR, typename Base>
__global__ __launch_bounds__(256) void present_kernel(Base b, const PresentPrim *__restrict__ prims, int n_prims,
                                                      const float4 *__restrict__ tex, void *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);      // wave-uniform
    const int xw0 = blockIdx.x * 64, xw1 = xw0 + 63;
    const int x = xw0 + lane;
    if (y >= b.H || x >= b.W) return;
    const float xc = (float)x + 0.5f, yc = (float)y + 0.5f;

    uint32_t px8 = 0;
    float4 pxf = make_float4(0.f, 0.f, 0.f, 1.f);
    if constexpr (std::is_same<Base, SurfaceArgs>::value) {
        px8 = surface_base_rgba8(b, xc, yc);
    } else if constexpr (std::is_same<Base, MomentArgs>::value) {
        px8 = moment_base_rgba8(b, xc, yc);
    } else {
        // ---- base layer: sample the raw channels, then map
        const float ax = (xc - b.ox) * b.k, ay = (yc - b.oy) * b.k;
        float4 v;
        if (b.linear) {
            v = bilinear(b.img, b.C, b.R, b.R, ax, ay);
        } else {
            const int i = clampi((int)__builtin_floorf(ax), 0, b.R - 1), j = clampi((int)__builtin_floorf(ay), 0, b.R - 1);
            v = load_texel(b.img, b.C, (int64_t)j * b.R + i);
        }
        if (b.map == TSP_PRESENT_SCALAR) {
            px8 = map_scalar_rgba8(v.x, v.y, b.lut, b.n_lut, b.vmin, b.range, b.log_scale, b.weighted);
        } else if (b.map == TSP_PRESENT_BIVARIATE) {
            px8 = map_bivariate_rgba8(v.x, v.y, b.lut, b.n_lut, b.vmin, b.range, b.dvmin, b.drange, b.log_scale, b.weighted);
        } else {
            const float c0 = map_rgb_channel(v.x, b.vmin, b.range, b.gamma);
            const float c1 = map_rgb_channel(v.y, b.vmin, b.range, b.gamma);
            const float c2 = map_rgb_channel(v.z, b.vmin, b.range, b.gamma);
            if (HDR) pxf = make_float4(__half2float(__float2half_rn(c0)), __half2float(__float2half_rn(c1)),
                                       __half2float(__float2half_rn(c2)), 1.0f);
            else px8 = unorm8(c0) | (unorm8(c1) << 8) | (unorm8(c2) << 16) | (255u << 24);
        }
    }

    // ---- the primitives, in draw order
    for (int p = 0; p < n_prims; ++p) {
        const PresentPrim &q = prims[p];
        if (q.by0 > y || q.by1 < y || q.bx0 > xw1 || q.bx1 < xw0) continue;    // uniform: the box misses this wave's pixels
        float4 s;
        if (q.kind == TSP_LAYER_QUAD) {
            if (!(q.X0 <= xc && xc < q.X1 && q.Y0 <= yc && yc < q.Y1)) continue;
            const float u = q.u0 + ((xc - q.X0) / (q.X1 - q.X0)) * q.du;
            const float w = q.v0 + ((yc - q.Y0) / (q.Y1 - q.Y0)) * q.dv;
            const float4 t = bilinear(reinterpret_cast<const float *>(tex + q.tex_off), 4, q.tw, q.th, u * (float)q.tw,
                                      w * (float)q.th);
            s = make_float4(t.x * q.weight, t.y * q.weight, t.z * q.weight, t.w * q.weight);
        } else {
            bool in = true;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float E = q.ex[e] * (yc - q.py[e]) - q.ey[e] * (xc - q.px[e]);
                in = in && (E > 0.0f || (E == 0.0f && ((q.closed >> e) & 1)));
            }
            if (!in) continue;
            s = make_float4(q.color[0], q.color[1], q.color[2], q.color[3]);
        }
        const float oma = 1.0f - s.w;
        if (HDR) {
            pxf = make_float4(__half2float(__float2half_rn(blend1(s.x, s.w, pxf.x, oma))),
                              __half2float(__float2half_rn(blend1(s.y, s.w, pxf.y, oma))),
                              __half2float(__float2half_rn(blend1(s.z, s.w, pxf.z, oma))),
                              __half2float(__float2half_rn(blend1(s.w, s.w, pxf.w, oma))));
        } else {
            px8 = unorm8(blend1(s.x, s.w, unorm_to_float(px8, 0), oma)) |
                  (unorm8(blend1(s.y, s.w, unorm_to_float(px8, 8), oma)) << 8) |
                  (unorm8(blend1(s.z, s.w, unorm_to_float(px8, 16), oma)) << 16) |
                  (unorm8(blend1(s.w, s.w, unorm_to_float(px8, 24), oma)) << 24);
        }
    }

    const int64_t o = (int64_t)y * b.W + x;
    if (HDR) {
        const uint32_t lo = (uint32_t)__half_as_ushort(__float2half_rn(pxf.x)) | ((uint32_t)__half_as_ushort(__float2half_rn(pxf.y)) << 16);
        const uint32_t hi = (uint32_t)__half_as_ushort(__float2half_rn(pxf.z)) | ((uint32_t)__half_as_ushort(__float2half_rn(pxf.w)) << 16);
        reinterpret_cast<uint2 *>(out)[o] = make_uint2(lo, hi);
    } else {
        reinterpret_cast<uint32_t *>(out)[o] = px8;
    }
}

// ---- movie frames: the RGBA8 frame to I420 planes (include/topsy_splat.h "tsp_present_yuv420"); integer arithmetic, alpha ignored
__device__ __forceinline__ uint32_t luma(uint32_t p) {
    return ((47u * (p & 255u) + 157u * ((p >> 8) & 255u) + 16u * ((p >> 16) & 255u) + 128u) >> 8) + 16u;
}
// U | V << 8 of one 2 x 2 block: pixels a, b on the upper row, c, d below; `>>` on a negative int is a floor (arithmetic shift)
__device__ __forceinline__ uint32_t chroma(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    const int r = (int)(((a & 255u) + (b & 255u) + (c & 255u) + (d & 255u) + 2u) >> 2);
    const int g = (int)((((a >> 8) & 255u) + ((b >> 8) & 255u) + ((c >> 8) & 255u) + ((d >> 8) & 255u) + 2u) >> 2);
    const int bl = (int)((((a >> 16) & 255u) + ((b >> 16) & 255u) + ((c >> 16) & 255u) + ((d >> 16) & 255u) + 2u) >> 2);
    const int u = ((-26 * r - 86 * g + 112 * bl + 128) >> 8) + 128;
    const int v = ((112 * r - 102 * g - 10 * bl + 128) >> 8) + 128;
    return (uint32_t)u | ((uint32_t)v << 8);
}

// One lane per 4 x 2 block (two chroma samples): 16-byte loads of each row, 4-byte luma stores.  W4 = (W % 4 == 0); otherwise
// W = 2 (mod 4), the odd rows start 8 bytes into a 16-byte line, so the rows come in as 8-byte halves, luma goes out as 2-byte
// halves, chroma byte by byte, and the last lane of each row pair takes the remaining 2 x 2 block.
template <bool W4>
__global__ __launch_bounds__(256) void yuv420_kernel(const uint32_t *__restrict__ rgba, int W, int H, int lanes_per_row,
                                                     uint8_t *__restrict__ yuv) {
    const int t = (int)blockIdx.x * 256 + (int)threadIdx.x;
    const int j = t / lanes_per_row;                         // row pair: rows 2j, 2j + 1; chroma row j
    if (j >= H / 2) return;
    const int x = (t - j * lanes_per_row) * 4;
    const int64_t p0 = (int64_t)(2 * j) * W + x, p1 = p0 + W;
    const int64_t c = (int64_t)j * (W / 2) + x / 2;
    uint8_t *__restrict__ Y = yuv;
    uint8_t *__restrict__ U = yuv + (int64_t)W * H;
    uint8_t *__restrict__ V = U + (int64_t)(W / 2) * (H / 2);
    if (W4) {
        const uint4 a = *reinterpret_cast<const uint4 *>(rgba + p0), b = *reinterpret_cast<const uint4 *>(rgba + p1);
        *reinterpret_cast<uint32_t *>(Y + p0) = luma(a.x) | (luma(a.y) << 8) | (luma(a.z) << 16) | (luma(a.w) << 24);
        *reinterpret_cast<uint32_t *>(Y + p1) = luma(b.x) | (luma(b.y) << 8) | (luma(b.z) << 16) | (luma(b.w) << 24);
        const uint32_t uv0 = chroma(a.x, a.y, b.x, b.y), uv1 = chroma(a.z, a.w, b.z, b.w);
        *reinterpret_cast<uint16_t *>(U + c) = (uint16_t)((uv0 & 255u) | ((uv1 & 255u) << 8));
        *reinterpret_cast<uint16_t *>(V + c) = (uint16_t)((uv0 >> 8) | (uv1 & 0xff00u));
    } else {
        const int n = x + 4 <= W ? 2 : 1;                    // 2 x 2 blocks of this lane
        for (int k = 0; k < n; ++k) {
            const uint2 a = *reinterpret_cast<const uint2 *>(rgba + p0 + 2 * k);
            const uint2 b = *reinterpret_cast<const uint2 *>(rgba + p1 + 2 * k);
            *reinterpret_cast<uint16_t *>(Y + p0 + 2 * k) = (uint16_t)(luma(a.x) | (luma(a.y) << 8));
            *reinterpret_cast<uint16_t *>(Y + p1 + 2 * k) = (uint16_t)(luma(b.x) | (luma(b.y) << 8));
            const uint32_t uv = chroma(a.x, a.y, b.x, b.y);
            U[c + k] = (uint8_t)(uv & 255u);
            V[c + k] = (uint8_t)(uv >> 8);
        }
    }
}

bool finite(float v) { return std::isfinite(v); }

// Conservative pixel box of a primitive spanning [lo, hi] in pixels along one axis: float rounding of the coverage tests
// cannot reach further than a few ulps of the largest coordinate involved, far inside the margin.
void pixel_span(double lo, double hi, double maxabs, int n, int &a, int &b) {
    const double m = 1.0 + 1e-5 * maxabs;
    if (!(lo <= hi)) { a = 1; b = 0; return; }          // NaN
    double l = std::floor(lo - m), h = std::ceil(hi + m);
    l = l < 0.0 ? 0.0 : l;
    h = h > (double)(n - 1) ? (double)(n - 1) : h;
    if (!(l <= h)) { a = 1; b = 0; return; }
    a = (int)l;
    b = (int)h;
}

void quad_prims(const tsp_present_layer &L, int W, int H, int tex_off, std::vector<PresentPrim> &out) {
    const float hw = 0.5f * (float)W, hh = 0.5f * (float)H;
    for (int k = 0; k < L.n_instances; ++k) {
        PresentPrim q = {};
        q.kind = TSP_LAYER_QUAD;
        const float qx = L.clip_origin[0] + L.instance_offsets[2 * k], qy = L.clip_origin[1] + L.instance_offsets[2 * k + 1];
        q.X0 = (qx + 1.0f) * hw;
        q.X1 = ((qx + L.clip_extent[0]) + 1.0f) * hw;
        q.Y0 = (1.0f - (qy + L.clip_extent[1])) * hh;
        q.Y1 = (1.0f - qy) * hh;
        q.u0 = L.tex_origin[0];
        q.du = L.tex_extent[0];
        q.v0 = L.tex_origin[1];
        q.dv = L.tex_extent[1];
        q.weight = L.instance_weights[k];
        q.tex_off = tex_off;
        q.tw = L.tex_width;
        q.th = L.tex_height;
        const double maxabs = std::fmax(std::fmax(std::fabs(q.X0), std::fabs(q.X1)), std::fmax(std::fabs(q.Y0), std::fabs(q.Y1)));
        pixel_span(std::fmin(q.X0, q.X1), std::fmax(q.X0, q.X1), maxabs, W, q.bx0, q.bx1);
        pixel_span(std::fmin(q.Y0, q.Y1), std::fmax(q.Y0, q.Y1), maxabs, H, q.by0, q.by1);
        if (q.bx0 > q.bx1 || q.by0 > q.by1) q.bx0 = q.by0 = 1, q.bx1 = q.by1 = 0;
        out.push_back(q);
    }
}

void line_prims(const tsp_present_layer &L, int W, int H, std::vector<PresentPrim> &out) {
    const float Wf = (float)W, Hf = (float)H, hw = 0.5f * Wf, hh = 0.5f * Hf;
    const float *M = L.transform;
    for (int s = 0; s < L.n_segments; ++s) {
        const float *P = L.starts + 4 * s, *Q = L.ends + 4 * s;
        const float ax = (((M[0] * P[0] + M[1] * P[1]) + M[2] * P[2]) + M[3] * P[3]) * Wf;
        const float ay = (((M[4] * P[0] + M[5] * P[1]) + M[6] * P[2]) + M[7] * P[3]) * Hf;
        const float bx = (((M[0] * Q[0] + M[1] * Q[1]) + M[2] * Q[2]) + M[3] * Q[3]) * Wf;
        const float by = (((M[4] * Q[0] + M[5] * Q[1]) + M[6] * Q[2]) + M[7] * Q[3]) * Hf;
        const float dx = bx - ax, dy = by - ay;
        const float len = std::sqrt(dx * dx + dy * dy);
        const float nx = -(dy / len), ny = dx / len;
        const float ox = (nx * L.width_px) * 0.5f, oy = (ny * L.width_px) * 0.5f;
        const float cx[4] = {ax - ox, ax + ox, bx + ox, bx - ox}, cy[4] = {ay - oy, ay + oy, by + oy, by - oy};
        float X[4], Y[4];
        for (int c = 0; c < 4; ++c) {
            X[c] = (cx[c] / Wf + 1.0f) * hw;
            Y[c] = (1.0f - cy[c] / Hf) * hh;
        }
        float A = 0.0f;
        for (int c = 0; c < 4; ++c) A = A + (X[c] * Y[(c + 1) & 3] - X[(c + 1) & 3] * Y[c]);
        PresentPrim q = {};
        q.kind = TSP_LAYER_LINES;
        for (int k = 0; k < 4; ++k) q.color[k] = L.color[k];
        if (!(A > 0.0f || A < 0.0f)) {          // zero or not a number: covers nothing
            q.bx0 = q.by0 = 1;
            out.push_back(q);
            continue;
        }
        double lo_x = X[0], hi_x = X[0], lo_y = Y[0], hi_y = Y[0], maxabs = 0.0;
        for (int c = 0; c < 4; ++c) {
            const int k = A > 0.0f ? c : 3 - c;
            q.px[c] = X[k];
            q.py[c] = Y[k];
            lo_x = std::fmin(lo_x, X[k]); hi_x = std::fmax(hi_x, X[k]);
            lo_y = std::fmin(lo_y, Y[k]); hi_y = std::fmax(hi_y, Y[k]);
            maxabs = std::fmax(maxabs, std::fmax(std::fabs((double)X[k]), std::fabs((double)Y[k])));
        }
        bool any_nan = false;
        for (int c = 0; c < 4; ++c) {
            q.ex[c] = q.px[(c + 1) & 3] - q.px[c];
            q.ey[c] = q.py[(c + 1) & 3] - q.py[c];
            if (q.ey[c] < 0.0f || (q.ey[c] == 0.0f && q.ex[c] > 0.0f)) q.closed |= 1 << c;
            any_nan = any_nan || std::isnan(q.px[c]) || std::isnan(q.py[c]);
        }
        if (any_nan) {
            q.bx0 = q.by0 = 1;
            q.bx1 = q.by1 = 0;
        } else {
            pixel_span(lo_x, hi_x, maxabs, W, q.bx0, q.bx1);
            pixel_span(lo_y, hi_y, maxabs, H, q.by0, q.by1);
            if (q.bx0 > q.bx1 || q.by0 > q.by1) q.bx0 = q.by0 = 1, q.bx1 = q.by1 = 0;
        }
        out.push_back(q);
    }
}

int check_layer(const tsp_present_layer &L, int index, int64_t &n_prims, int64_t &n_texels) {
    if (L.kind == TSP_LAYER_QUAD) {
        TSP_REQUIRE(L.texture_rgba && L.instance_offsets && L.instance_weights, TSP_EINVAL, "layer %d: NULL texture or instance array", index);
        TSP_REQUIRE(L.tex_width >= 1 && L.tex_width <= MAX_SIDE && L.tex_height >= 1 && L.tex_height <= MAX_SIDE, TSP_EINVAL,
                    "layer %d: texture of %d x %d texels", index, L.tex_width, L.tex_height);
        TSP_REQUIRE(L.n_instances >= 1 && L.n_instances <= MAX_INSTANCES, TSP_EINVAL, "layer %d: %d instances", index, L.n_instances);
        bool ok = true;
        for (int a = 0; a < 2; ++a) {
            ok = ok && finite(L.clip_origin[a]) && finite(L.clip_extent[a]) && L.clip_extent[a] > 0.0f && finite(L.tex_origin[a]) &&
                 finite(L.tex_extent[a]) && std::fabs(L.tex_origin[a]) + std::fabs(L.tex_extent[a]) <= 1024.0f;
        }
        for (int k = 0; k < L.n_instances && ok; ++k)
            ok = finite(L.instance_offsets[2 * k]) && finite(L.instance_offsets[2 * k + 1]) && finite(L.instance_weights[k]);
        TSP_REQUIRE(ok, TSP_EINVAL, "layer %d: quad geometry, texture coordinates or instances not finite / in range", index);
        n_prims += L.n_instances;
        n_texels += (int64_t)L.tex_width * L.tex_height;
        return TSP_OK;
    }
    TSP_REQUIRE(L.kind == TSP_LAYER_LINES, TSP_EINVAL, "layer %d: unknown kind %d", index, L.kind);
    TSP_REQUIRE(L.starts && L.ends, TSP_EINVAL, "layer %d: NULL segment array", index);
    TSP_REQUIRE(L.n_segments >= 1 && L.n_segments <= MAX_PRIMS, TSP_EINVAL, "layer %d: %d segments", index, L.n_segments);
    bool ok = finite(L.width_px) && L.width_px >= 0.0f;
    for (int k = 0; k < 16; ++k) ok = ok && finite(L.transform[k]);
    for (int k = 0; k < 4; ++k) ok = ok && finite(L.color[k]);
    for (int64_t k = 0; k < 4 * (int64_t)L.n_segments && ok; ++k) ok = finite(L.starts[k]) && finite(L.ends[k]);
    TSP_REQUIRE(ok, TSP_EINVAL, "layer %d: line width, transform, colour or points not finite", index);
    n_prims += L.n_segments;
    return TSP_OK;
}

// One frame: exactly one of `base` (the maps of tsp_present) and `surf` (the lit surface) is given.  ms_out: base: the
// composition (+ conversion); surf: [filter, composition (+ conversion)].
int compose(tsp_context *ctx, int W, int H, const tsp_present_base *base, const tsp_surface_params *surf,
            const tsp_present_layer *layers, int n_layers, void *out, double *ms_out, bool yuv420) {
    TSP_REQUIRE(W >= 1 && W <= MAX_SIDE && H >= 1 && H <= MAX_SIDE, TSP_EINVAL, "canvas %d x %d outside [1, %d]", W, H, MAX_SIDE);
    if (yuv420) TSP_REQUIRE(W >= 2 && H >= 2 && W % 2 == 0 && H % 2 == 0, TSP_EINVAL, "4:2:0 needs an even canvas, not %d x %d", W, H);
    TSP_REQUIRE(n_layers >= 0 && n_layers <= MAX_LAYERS && (n_layers == 0 || layers), TSP_EINVAL, "bad layer list (%d layers)", n_layers);
    const int map = base ? base->map : -1;
    const bool moment = map == TSP_PRESENT_MOMENT_MEAN || map == TSP_PRESENT_MOMENT_SIGMA;
    const float *h_lut = nullptr;       // the 1-D LUT of the call, if its base has one
    int n_lut = 0;
    if (base) {
        TSP_REQUIRE(map >= TSP_PRESENT_SCALAR && map <= TSP_PRESENT_MOMENT_SIGMA, TSP_EINVAL, "unknown base map %d", map);
        if (yuv420) TSP_REQUIRE(map != TSP_PRESENT_RGB_HDR, TSP_EINVAL, "4:2:0 frames are 8-bit: the rgb-hdr map has no such frame");
        if (moment)
            TSP_REQUIRE(ctx->image_source == W_KINEMATIC && ctx->C == 4, TSP_ESTATE,
                        "the image is not a kinematic one (render with TSP_MODE_KINEMATIC first)");
        if (map == TSP_PRESENT_SCALAR || moment) {
            TSP_REQUIRE(base->lut_rgba && base->n_lut >= 2 && base->n_lut <= 65536, TSP_EINVAL, "bad colormap LUT (n=%d)", base->n_lut);
            h_lut = base->lut_rgba;
            n_lut = base->n_lut;
        }
        if (map == TSP_PRESENT_BIVARIATE) TSP_REQUIRE(ctx->lut2d, TSP_ESTATE, "tsp_colormap_set_lut2d must be called first");
        if (map == TSP_PRESENT_RGB || map == TSP_PRESENT_RGB_HDR) TSP_REQUIRE(ctx->C == 4, TSP_EINVAL, "rgb maps need a 4-channel image");
    } else if (surf->weighted_average) {     // (checked by the caller: 2..65536 entries)
        h_lut = surf->lut_rgba;
        n_lut = surf->n_lut;
    }
    int64_t n_prims = 0, n_texels = 0;
    for (int l = 0; l < n_layers; ++l) {
        const int rc = check_layer(layers[l], l, n_prims, n_texels);
        if (rc) return rc;
        TSP_REQUIRE(n_prims <= MAX_PRIMS, TSP_EINVAL, "more than %d primitives", MAX_PRIMS);
        TSP_REQUIRE(n_texels < (1ll << 31), TSP_EINVAL, "more than 2^31 texels in the layer textures");
    }

    std::vector<PresentPrim> prims;
    prims.reserve((size_t)n_prims);
    std::vector<int64_t> tex_at((size_t)n_layers, -1);
    int64_t tex_off = 0;
    for (int l = 0; l < n_layers; ++l) {
        const tsp_present_layer &L = layers[l];
        if (L.kind == TSP_LAYER_QUAD) {
            tex_at[l] = tex_off;
            quad_prims(L, W, H, (int)tex_off, prims);
            tex_off += (int64_t)L.tex_width * L.tex_height;
        } else {
            line_prims(L, W, H, prims);
        }
    }

    TSP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const bool hdr = map == TSP_PRESENT_RGB_HDR;
    const size_t frame_bytes = (size_t)W * H * (hdr ? 8 : 4);
    const size_t out_bytes = yuv420 ? (size_t)W * H + 2 * ((size_t)(W / 2) * (H / 2)) : frame_bytes;
    DeviceScratch d_tex, d_prims, d_lut, d_frame, d_yuv, d_filtered;
    TSP_SCRATCH_ALLOC(ctx, SITE("present_frame"), d_frame, frame_bytes);
    if (yuv420) TSP_SCRATCH_ALLOC(ctx, SITE("present_yuv"), d_yuv, out_bytes);
    TSP_SCRATCH_ALLOC(ctx, SITE("present_prims"), d_prims, prims.size() * sizeof(PresentPrim));
    TSP_SCRATCH_ALLOC(ctx, SITE("present_textures"), d_tex, (size_t)n_texels * sizeof(float4));
    if (h_lut) TSP_SCRATCH_ALLOC(ctx, SITE("present_lut"), d_lut, (size_t)n_lut * sizeof(float4));
    if (surf) TSP_SCRATCH_ALLOC(ctx, SITE("present_filtered"), d_filtered, (size_t)ctx->R * ctx->R * sizeof(float2));

    for (int l = 0; l < n_layers; ++l)
        if (tex_at[l] >= 0)
            TSP_HIP(hipMemcpyAsync(d_tex.as<float4>() + tex_at[l], layers[l].texture_rgba,
                                   (size_t)layers[l].tex_width * layers[l].tex_height * sizeof(float4), hipMemcpyHostToDevice, st));
    if (!prims.empty())
        TSP_HIP(hipMemcpyAsync(d_prims.p, prims.data(), prims.size() * sizeof(PresentPrim), hipMemcpyHostToDevice, st));
    if (h_lut) TSP_HIP(hipMemcpyAsync(d_lut.p, h_lut, (size_t)n_lut * sizeof(float4), hipMemcpyHostToDevice, st));

    const int S = W > H ? W : H;
    const float k = (float)ctx->R / (float)S, ox = 0.5f * (float)(W - S), oy = 0.5f * (float)(H - S);
    const dim3 grid((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4));
    if (surf) {
        TSP_HIP(hipEventRecord(ctx->ev[EV_T2], st));
        if (int rc = launch_bilateral(ctx, surf->smoothing_scale, d_filtered.as<float2>())) return rc;
        TSP_HIP(hipEventRecord(ctx->ev[EV_T3], st));
        SurfaceArgs a;
        a.F = d_filtered.as<float2>();
        a.R = ctx->R;
        a.W = W;
        a.H = H;
        a.k = k;
        a.ox = ox;
        a.oy = oy;
        a.du = (float)ctx->R / (float)W;
        a.dv = (float)ctx->R / (float)H;
        a.linear = k <= 1.0f;
        a.sp = shade_params(*surf, W);
        a.lut = d_lut.as<float4>();
        hipLaunchKernelGGL((present_kernel<false, SurfaceArgs>), grid, dim3(256), 0, st, a, d_prims.as<PresentPrim>(), (int)prims.size(),
                           d_tex.as<float4>(), d_frame.p);
    } else if (moment) {
        MomentArgs a;
        a.img = ctx->image;
        a.R = ctx->R;
        a.W = W;
        a.H = H;
        a.k = k;
        a.ox = ox;
        a.oy = oy;
        a.linear = k <= 1.0f;
        a.sigma = map == TSP_PRESENT_MOMENT_SIGMA;
        a.lut = d_lut.as<float4>();
        a.n_lut = n_lut;
        a.vmin = base->vmin;
        a.range = base->vmax - base->vmin;
        a.log_scale = base->log_scale ? 1 : 0;
        TSP_HIP(hipEventRecord(ctx->ev[EV_T3], st));
        hipLaunchKernelGGL((present_kernel<false, MomentArgs>), grid, dim3(256), 0, st, a, d_prims.as<PresentPrim>(), (int)prims.size(),
                           d_tex.as<float4>(), d_frame.p);
    } else {
        BaseArgs b;
        b.img = ctx->image;
        b.R = ctx->R;
        b.C = ctx->C;
        b.W = W;
        b.H = H;
        b.k = k;
        b.ox = ox;
        b.oy = oy;
        b.linear = b.k <= 1.0f;
        b.map = map;
        b.lut = map == TSP_PRESENT_SCALAR ? d_lut.as<float4>() : reinterpret_cast<const float4 *>(ctx->lut2d);
        b.n_lut = map == TSP_PRESENT_SCALAR ? n_lut : ctx->lut2d_n;
        b.vmin = base->vmin;
        b.range = base->vmax - base->vmin;
        b.dvmin = base->density_vmin;
        b.drange = base->density_vmax - base->density_vmin;
        b.gamma = base->gamma;
        b.log_scale = base->log_scale ? 1 : 0;
        b.weighted = base->weighted ? 1 : 0;
        TSP_HIP(hipEventRecord(ctx->ev[EV_T3], st));
        if (hdr)
            hipLaunchKernelGGL((present_kernel<true, BaseArgs>), grid, dim3(256), 0, st, b, d_prims.as<PresentPrim>(), (int)prims.size(),
                               d_tex.as<float4>(), d_frame.p);
        else
            hipLaunchKernelGGL((present_kernel<false, BaseArgs>), grid, dim3(256), 0, st, b, d_prims.as<PresentPrim>(), (int)prims.size(),
                               d_tex.as<float4>(), d_frame.p);
    }
    TSP_HIP(hipGetLastError());
    if (yuv420) {
        const bool w4 = W % 4 == 0;
        const int lanes_per_row = w4 ? W / 4 : (W + 2) / 4;
        const int n_lanes = lanes_per_row * (H / 2);        // <= 4096 * 8192
        const dim3 ygrid((unsigned)((n_lanes + 255) / 256));
        if (w4)
            hipLaunchKernelGGL(yuv420_kernel<true>, ygrid, dim3(256), 0, st, d_frame.as<const uint32_t>(), W, H, lanes_per_row,
                               d_yuv.as<uint8_t>());
        else
            hipLaunchKernelGGL(yuv420_kernel<false>, ygrid, dim3(256), 0, st, d_frame.as<const uint32_t>(), W, H, lanes_per_row,
                               d_yuv.as<uint8_t>());
        TSP_HIP(hipGetLastError());
    }
    TSP_HIP(hipEventRecord(ctx->ev[EV_T4], st));
    TSP_HIP(hipStreamSynchronize(st));      // the frame is complete before anything of the caller's is written
    TSP_HIP(hipMemcpyAsync(out, yuv420 ? d_yuv.p : d_frame.p, out_bytes, hipMemcpyDeviceToHost, st));
    TSP_HIP(hipStreamSynchronize(st));
    if (ms_out) {
        float ms = 0.f;
        if (surf) {
            TSP_HIP(hipEventElapsedTime(&ms, ctx->ev[EV_T2], ctx->ev[EV_T3]));
            *ms_out++ = ms;
        }
        TSP_HIP(hipEventElapsedTime(&ms, ctx->ev[EV_T3], ctx->ev[EV_T4]));
        *ms_out = ms;
    }
    return TSP_OK;
}

}  // namespace

int present(tsp_context *ctx, int W, int H, const tsp_present_base &base, const tsp_present_layer *layers, int n_layers,
            void *out, double *gpu_ms_out, bool yuv420) {
    return compose(ctx, W, H, &base, nullptr, layers, n_layers, out, gpu_ms_out, yuv420);
}

int present_surface(tsp_context *ctx, int W, int H, const tsp_surface_params &prm, const tsp_present_layer *layers, int n_layers,
                    void *out, double *ms_out, bool yuv420) {
    return compose(ctx, W, H, nullptr, &prm, layers, n_layers, out, ms_out, yuv420);
}

}  // namespace tsp
