// tsp_surface.hip -- surface rendering: the occlusion pass, its resolve, the rho order statistics, the bilateral filter and the
// lit shading (include/topsy_splat.h "Surface rendering").
//
// Reference semantics: DepthSPHWithOcclusion (src/topsy/sph.py:448-656) = vertex_depth_with_cut + fragment_raw with
// depth_compare greater and the depth cleared to 0 (shaders/sph.wgsl:94-122,149-158); ColorAsSurfaceMap (colormap/surface.py)
// = the bilateral filter of shaders/smooth.wgsl:12-48 and the shading of shaders/surface.wgsl:28-123.
//
// Occlusion: a depth test is a max.  Every fragment forms the 64-bit key (bits(dc) << 32) | (0xFFFFFFFF - index) -- dc > 0, so
// its bits order like the value, and on equal dc the lower index has the larger key ("first drawn wins" of a strict greater
// test) -- and takes the atomic max with the pixel's key in the float64 accumulator, read as uint64.  Any split of the particles
// into blocks and any order give the same keys.  The resolve then recomputes the winner's depth at each pixel with the same
// device function (surface_fragment) and reads its q.
//
// Mapping of the draw: one lane per particle for footprints of at most 16 pixels; larger ones are broadcast over the wave and
// drawn 64 pixels per step, so that no lane holds hundreds of atomics.  An atomic is only issued when the pixel's current key
// (a plain load: keys only grow) is smaller.
//
// Filter: a 16 x 16 pixel tile plus its clamped halo in LDS, and the spatial weights of every (dx, dy) of the window computed
// once per workgroup with the per-tap expression, so they equal the per-tap ones bit for bit.
#include <string.h>

#include <algorithm>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "tsp_internal.h"

namespace tsp {

// ------------------------------------------------------------------------------------------------
// occlusion pass
// ------------------------------------------------------------------------------------------------
struct SurfParticle {
    Proj pr;
    float zs;        // (h * sf) * 0.5: depth extent of the sphere (sph.wgsl:113-120)
    float q;
    bool drawn;
};

__device__ __forceinline__ SurfParticle surface_particle(const Particles &p, int64_t i, const Camera &cam, float cut) {
    SurfParticle s = {};
    const float h = p.h[i];
    const float rho = p.m[i] / ((h * h) * h);         // vertex_depth_with_cut: quantities.x / pow(pos.w, 3)
    s.drawn = false;
    if (!(rho > cut)) return s;
    s.pr = project(cam, p.x[i], p.y[i], p.z[i], h);
    s.zs = (h * cam.sf) * 0.5f;
    s.q = p.q ? p.q[i] : 0.0f;
    s.drawn = s.pr.keep;
    return s;
}

// The fragment at pixel (i, j): its unclamped depth in `depth`, and whether it competes (k >= 0 and min(depth, 1) > 0).  The draw
// and the resolve both come here, so the resolve recomputes the winner's depth bit for bit.
template <typename LUT>
__device__ __forceinline__ bool surface_fragment(const LUT &T, const SurfParticle &s, int lvl, int i, int j, float &depth) {
    const float dx = ((float)i + 0.5f) - s.pr.pcx;
    const float dy = ((float)j + 0.5f) - s.pr.pcy;
    const float k = sample_kernel(T, s.pr, lvl, dx, dy);
    depth = s.pr.cz + s.zs * k;
    const float dc = depth < 1.0f ? depth : 1.0f;      // the depth attachment clamps
    return (k >= 0.0f) && (dc > 0.0f);
}

__device__ __forceinline__ unsigned long long surface_key(float depth, uint32_t idx) {
    const float dc = depth < 1.0f ? depth : 1.0f;
    return ((unsigned long long)__float_as_uint(dc) << 32) | (unsigned long long)(0xFFFFFFFFu - idx);
}

__device__ __forceinline__ void key_max(unsigned long long *px, unsigned long long key) {
    if (key > __hip_atomic_load(px, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(px, key);
}

// ranges layout on device: [0,n) starts, [n,2n) lens, [2n,3n+1) prefix of lens (as tsp_splat_generic.hip)
__device__ __forceinline__ int64_t surface_work_to_particle(const int64_t *ranges, int n_ranges, int64_t w) {
    if (n_ranges == 1) return ranges[0] + w;
    const int64_t *prefix = ranges + 2 * n_ranges;
    int lo = 0, hi = n_ranges - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (prefix[mid] <= w) lo = mid; else hi = mid - 1;
    }
    return ranges[lo] + (w - prefix[lo]);
}

__global__ __launch_bounds__(256) void surface_draw_kernel(Particles p, const int64_t *ranges, int n_ranges, int64_t total,
                                                           Camera cam, float cut, const float *sphere_g,
                                                           unsigned long long *keys, unsigned long long *n_drawn) {
    __shared__ float T[MIP_TOTAL];
    for (int t = threadIdx.x; t < MIP_TOTAL; t += 256) T[t] = sphere_g[t];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int R = cam.R;
    unsigned long long drawn = 0;
    for (int64_t base = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63); base < total; base += (int64_t)gridDim.x * 256) {
        const int64_t w = base + lane;
        SurfParticle s = {};
        uint32_t idx = 0;
        int ilo = 1, ihi = 0, jlo = 1, jhi = 0;
        if (w < total) {
            const int64_t i = surface_work_to_particle(ranges, n_ranges, w);
            idx = (uint32_t)i;
            s = surface_particle(p, i, cam, cut);
            if (s.drawn) {
                cover_range(s.pr.pcx, s.pr.half, R, ilo, ihi);
                cover_range(s.pr.pcy, s.pr.half, R, jlo, jhi);
            }
        }
        const bool active = s.drawn && ilo <= ihi && jlo <= jhi;
        drawn += active;
        const int nx = ihi - ilo + 1;
        const int npx = active ? nx * (jhi - jlo + 1) : 0;
        const int lvl = level_for(s.pr.P);
        const bool small = active && npx <= 16;
        if (small) {
            for (int j = jlo; j <= jhi; ++j)
                for (int i = ilo; i <= ihi; ++i) {
                    float depth;
                    if (surface_fragment(T, s, lvl, i, j, depth)) key_max(keys + (size_t)j * R + i, surface_key(depth, idx));
                }
        }
        unsigned long long big = __ballot(active && !small);
        while (big) {
            const int src = __ffsll((long long)big) - 1;
            big &= big - 1;
            SurfParticle b;
            b.pr.pcx = __shfl(s.pr.pcx, src); b.pr.pcy = __shfl(s.pr.pcy, src);
            b.pr.P = __shfl(s.pr.P, src); b.pr.half = __shfl(s.pr.half, src); b.pr.invP = __shfl(s.pr.invP, src);
            b.pr.cz = __shfl(s.pr.cz, src);
            b.zs = __shfl(s.zs, src);
            const uint32_t bidx = (uint32_t)__shfl((int)idx, src);
            const int bi = __shfl(ilo, src), bj = __shfl(jlo, src), bnx = __shfl(nx, src), bn = __shfl(npx, src);
            const int blvl = level_for(b.pr.P);
            for (int t = lane; t < bn; t += 64) {
                const int jj = t / bnx;
                const int j = bj + jj, i = bi + (t - jj * bnx);
                float depth;
                if (surface_fragment(T, b, blvl, i, j, depth)) key_max(keys + (size_t)j * R + i, surface_key(depth, bidx));
            }
        }
    }
    for (int o = 32; o; o >>= 1) drawn += __shfl_xor((long long)drawn, o);
    if (lane == 0 && drawn) atomicAdd(n_drawn, drawn);
}

// One lane per pixel: the winner's (q, unclamped depth), or (0, 0).
__global__ __launch_bounds__(256) void surface_resolve_kernel(Particles p, Camera cam, float cut, const float *sphere_g,
                                                              const unsigned long long *keys, float2 *img) {
    const int R = cam.R;
    const int64_t npix = (int64_t)R * R;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < npix; t += (int64_t)gridDim.x * 256) {
        const unsigned long long key = keys[t];
        float2 out = make_float2(0.0f, 0.0f);
        if (key) {
            const uint32_t idx = 0xFFFFFFFFu - (uint32_t)key;
            const SurfParticle s = surface_particle(p, idx, cam, cut);
            float depth = 0.0f;
            (void)surface_fragment(sphere_g, s, level_for(s.pr.P), (int)(t % R), (int)(t / R), depth);
            out = make_float2(s.q, depth);
        }
        img[t] = out;
    }
}

int render_surface(tsp_context *ctx, const Camera &cam, float cut, const int64_t *h_starts, const int64_t *h_lens,
                   int n_ranges, int64_t total, int clear, double *ms_draw, double *ms_resolve) {
    hipStream_t st = ctx->stream;
    const int64_t npix = (int64_t)ctx->R * ctx->R;
    // per-call memory first, so that a failed allocation leaves the target as it was
    DeviceScratch d_ranges, d_count;
    std::vector<int64_t> pack(3 * (size_t)n_ranges + 1);
    int64_t acc = 0;
    for (int i = 0; i < n_ranges; ++i) {
        pack[i] = h_starts[i];
        pack[n_ranges + i] = h_lens[i];
        pack[2 * n_ranges + i] = acc;
        acc += h_lens[i];
    }
    pack[3 * n_ranges] = acc;
    TSP_SCRATCH_ALLOC(ctx, SITE("surface_ranges"), d_ranges, pack.size() * sizeof(int64_t));
    TSP_SCRATCH_ALLOC(ctx, SITE("surface_drawn_count"), d_count, sizeof(unsigned long long));
    TSP_HIP(hipMemcpyAsync(d_ranges.p, pack.data(), pack.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    TSP_HIP(hipMemsetAsync(d_count.p, 0, sizeof(unsigned long long), st));
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(ctx->image64);
    TSP_HIP(hipEventRecord(ctx->ev[EV_T0], st));
    if (clear) TSP_HIP(hipMemsetAsync(keys, 0, (size_t)npix * sizeof(unsigned long long), st));
    Particles parts = ctx->p;
    if (!ctx->use_quantity) parts.q = nullptr;
    const float *sphere = ctx->mips + MIP_TOTAL;
    if (total > 0) {
        const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, (int64_t)ctx->cu_count * 8);
        hipLaunchKernelGGL(surface_draw_kernel, dim3(grid), dim3(256), 0, st, parts, d_ranges.as<int64_t>(), n_ranges, total, cam,
                           cut, sphere, keys, d_count.as<unsigned long long>());
        TSP_HIP(hipGetLastError());
    }
    TSP_HIP(hipEventRecord(ctx->ev[EV_T1], st));
    const unsigned pgrid = (unsigned)std::min<int64_t>((npix + 255) / 256, (int64_t)ctx->cu_count * 16);
    hipLaunchKernelGGL(surface_resolve_kernel, dim3(pgrid), dim3(256), 0, st, parts, cam, cut, sphere,
                       (const unsigned long long *)keys, reinterpret_cast<float2 *>(ctx->image));
    TSP_HIP(hipGetLastError());
    TSP_HIP(hipEventRecord(ctx->ev[EV_T2], st));
    unsigned long long drawn = 0;
    TSP_HIP(hipMemcpyAsync(&drawn, d_count.p, sizeof(drawn), hipMemcpyDeviceToHost, st));
    TSP_HIP(hipStreamSynchronize(st));
    float a = 0.f, b = 0.f;
    TSP_HIP(hipEventElapsedTime(&a, ctx->ev[EV_T0], ctx->ev[EV_T1]));
    TSP_HIP(hipEventElapsedTime(&b, ctx->ev[EV_T1], ctx->ev[EV_T2]));
    *ms_draw = a;
    *ms_resolve = b;
    ctx->stats = tsp_stats{};
    ctx->stats.n_particles = total;
    ctx->stats.n_culled = total - (int64_t)drawn;
    return TSP_OK;
}

// ------------------------------------------------------------------------------------------------
// order statistics of rho = m / h^3 (the density cut, sph.py:480-515)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t rho_key(float f) {   // monotone float -> uint map; every NaN last (numpy's sort order)
    if (f != f) return 0xFFFFFFFFu;
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(256) void rho_key_kernel(const float *__restrict__ m, const float *__restrict__ h, int64_t n,
                                                      uint32_t *__restrict__ keys) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float hh = h[i];
        keys[i] = rho_key(m[i] / ((hh * hh) * hh));
    }
}

__global__ void gather_keys_kernel(const uint32_t *__restrict__ sorted, const int64_t *__restrict__ ranks, int n,
                                   uint32_t *__restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) out[t] = sorted[ranks[t]];
}

int density_order_stats(tsp_context *ctx, const int64_t *ranks, int n_ranks, float *values_out) {
    const int64_t n = ctx->p.n;
    hipStream_t st = ctx->stream;
    DeviceScratch keys, keys2, tmp, d_ranks, d_out;
    size_t tmp_bytes = 0;
    TSP_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, n, 0, 32, st));
    TSP_SCRATCH_ALLOC(ctx, SITE("rho_keys"), keys, (size_t)n * 4);
    TSP_SCRATCH_ALLOC(ctx, SITE("rho_keys_sorted"), keys2, (size_t)n * 4);
    TSP_SCRATCH_ALLOC(ctx, SITE("rho_sort_tmp"), tmp, tmp_bytes);
    TSP_SCRATCH_ALLOC(ctx, SITE("rho_ranks"), d_ranks, (size_t)n_ranks * sizeof(int64_t));
    TSP_SCRATCH_ALLOC(ctx, SITE("rho_values"), d_out, (size_t)n_ranks * 4);
    const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, (int64_t)ctx->cu_count * 16);
    hipLaunchKernelGGL(rho_key_kernel, dim3(grid), dim3(256), 0, st, ctx->p.m, ctx->p.h, n, keys.as<uint32_t>());
    TSP_HIP(hipGetLastError());
    TSP_HIP(hipcub::DeviceRadixSort::SortKeys(tmp.p, tmp_bytes, keys.as<uint32_t>(), keys2.as<uint32_t>(), n, 0, 32, st));
    if (n_ranks > 0) {
        TSP_HIP(hipMemcpyAsync(d_ranks.p, ranks, (size_t)n_ranks * sizeof(int64_t), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(gather_keys_kernel, dim3((n_ranks + 255) / 256), dim3(256), 0, st, keys2.as<uint32_t>(),
                           d_ranks.as<int64_t>(), n_ranks, d_out.as<uint32_t>());
        TSP_HIP(hipGetLastError());
    }
    std::vector<uint32_t> hk((size_t)n_ranks);
    if (n_ranks > 0) TSP_HIP(hipMemcpyAsync(hk.data(), d_out.p, (size_t)n_ranks * 4, hipMemcpyDeviceToHost, st));
    TSP_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < n_ranks; ++i) {
        const uint32_t k = hk[(size_t)i];
        const uint32_t bits = (k == 0xFFFFFFFFu) ? 0x7FC00000u : ((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
        memcpy(&values_out[i], &bits, 4);
    }
    return TSP_OK;
}

// ------------------------------------------------------------------------------------------------
// bilateral filter (smooth.wgsl:12-48)
// ------------------------------------------------------------------------------------------------
constexpr int FT = 16;   // output tile side: one pixel per lane of a 256-lane workgroup

__device__ __forceinline__ float spatial_weight(int dx, int dy, float ss) {
    const float ds = sqrtf((float)(dx * dx + dy * dy));
    return canon_expf(-(ds * ds) / ((2.0f * ss) * ss));
}

__global__ __launch_bounds__(256) void bilateral_kernel(const float2 *__restrict__ img, float2 *__restrict__ out, int R, int half,
                                                        float ss, float rs) {
    extern __shared__ float lds[];
    const int W = FT + 2 * half;          // tile + halo
    const int nk = 2 * half + 1;
    float *tile = lds;                    // W x W depths, clamped coordinates
    float *wsp = lds + W * W;             // nk x nk spatial weights
    const int x0 = blockIdx.x * FT - half, y0 = blockIdx.y * FT - half;
    for (int t = threadIdx.x; t < W * W; t += 256) {
        const int ty = t / W, tx = t - ty * W;
        const int y = clampi(y0 + ty, 0, R - 1), x = clampi(x0 + tx, 0, R - 1);
        tile[t] = img[(size_t)y * R + x].y;
    }
    for (int t = threadIdx.x; t < nk * nk; t += 256) {
        const int ky = t / nk, kx = t - ky * nk;
        wsp[t] = spatial_weight(kx - half, ky - half, ss);
    }
    __syncthreads();
    const int lx = threadIdx.x % FT, ly = threadIdx.x / FT;
    const int px = blockIdx.x * FT + lx, py = blockIdx.y * FT + ly;
    if (px >= R || py >= R) return;
    const float dc = tile[(ly + half) * W + lx + half];
    const float r2 = (2.0f * rs) * rs;
    float sum = 0.0f, wsum = 0.0f;
    for (int ky = 0; ky < nk; ++ky) {
        const float *row = tile + (ly + ky) * W + lx;
        const float *wrow = wsp + ky * nk;
        for (int kx = 0; kx < nk; ++kx) {
            const float d = row[kx];
            const float dd = __builtin_fabsf(d - dc);
            const float wr = canon_expf(-(dd * dd) / r2);
            const float w = wrow[kx] * wr;
            sum += d * w;
            wsum += w;
        }
    }
    out[(size_t)py * R + px] = make_float2(img[(size_t)py * R + px].x, sum / wsum);
}

// ------------------------------------------------------------------------------------------------
// shading (surface.wgsl:28-123)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void surface_shade_kernel(const float2 *__restrict__ F, int R, ShadeParams sp,
                                                            const float4 *__restrict__ lut, uint32_t *__restrict__ out) {
    const int64_t npix = (int64_t)R * R;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < npix; t += (int64_t)gridDim.x * 256) {
        const int j = (int)(t / R), i = (int)(t - (int64_t)j * R);
        const float2 c = F[t];
        const float Dc = c.y * sp.depth_scale;
        const float Dl = F[(size_t)j * R + max(i - 1, 0)].y * sp.depth_scale;
        const float Dr = F[(size_t)j * R + min(i + 1, R - 1)].y * sp.depth_scale;
        const float Du = F[(size_t)max(j - 1, 0) * R + i].y * sp.depth_scale;
        const float Dd = F[(size_t)min(j + 1, R - 1) * R + i].y * sp.depth_scale;
        out[t] = surface_shade_rgba8(c.x, Dc, Dl, Dr, Du, Dd, sp, lut);
    }
}

ShadeParams shade_params(const tsp_surface_params &prm, int width) {
    ShadeParams sp;
    sp.depth_scale = prm.depth_scale;
    sp.vmin = prm.vmin;
    sp.vmax = prm.vmax;
    sp.nz = 1.0f / (float)width;       // texelSize.x
    for (int q = 0; q < 3; ++q) {
        sp.L[q] = prm.light_direction[q];
        sp.lc[q] = prm.light_color[q];
        sp.amb[q] = prm.ambient_color[q];
    }
    sp.weighted = prm.weighted_average ? 1 : 0;
    sp.log_scale = prm.log_scale ? 1 : 0;
    sp.n_lut = prm.weighted_average ? prm.n_lut : 0;
    return sp;
}

int launch_bilateral(tsp_context *ctx, double smoothing_scale, float2 *filtered) {
    const int R = ctx->R;
    // filter parameters as colormap/surface.py:259-287 forms them (float64, stored as float32; kernel_size from the float32)
    const double sig = smoothing_scale < 1e-5 ? 1e-5 : smoothing_scale;
    const float ss = (float)(sig * (double)R), rs = (float)(sig * 2.0);
    const float ss4 = ss * 4.0f;
    const int n_pix = ss4 >= 100.0f ? 100 : (int)ss4 + 1;     // min(int(ss * 4) + 1, MAX_SURFACE_SMOOTH_PIXELS = 100)
    const int half = n_pix / 2;
    const int W = FT + 2 * half, nk = 2 * half + 1;
    const size_t lds = (size_t)(W * W + nk * nk) * sizeof(float);
    if (lds > 65536)     // (at most 94.6 KB: half <= 50)
        TSP_HIP(hipFuncSetAttribute((const void *)bilateral_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const unsigned tiles = (unsigned)((R + FT - 1) / FT);
    hipLaunchKernelGGL(bilateral_kernel, dim3(tiles, tiles), dim3(256), lds, ctx->stream, reinterpret_cast<const float2 *>(ctx->image),
                       filtered, R, half, ss, rs);
    TSP_HIP(hipGetLastError());
    return TSP_OK;
}

int surface_present(tsp_context *ctx, const tsp_surface_params &prm, float *content_out, uint8_t *rgba8_out, double *ms_out) {
    const int R = ctx->R;
    const int64_t npix = (int64_t)R * R;
    hipStream_t st = ctx->stream;
    DeviceScratch filtered, lut;
    TSP_SCRATCH_ALLOC(ctx, SITE("surface_filtered"), filtered, (size_t)npix * sizeof(float2));
    if (rgba8_out && prm.weighted_average) {
        TSP_SCRATCH_ALLOC(ctx, SITE("surface_lut"), lut, (size_t)prm.n_lut * sizeof(float4));
        TSP_HIP(hipMemcpyAsync(lut.p, prm.lut_rgba, (size_t)prm.n_lut * sizeof(float4), hipMemcpyHostToDevice, st));
    }
    TSP_HIP(hipEventRecord(ctx->ev[EV_T3], st));
    if (int rc = launch_bilateral(ctx, prm.smoothing_scale, filtered.as<float2>())) return rc;
    TSP_HIP(hipEventRecord(ctx->ev[EV_T4], st));
    if (rgba8_out) {
        const ShadeParams sp = shade_params(prm, R);
        const unsigned grid = (unsigned)std::min<int64_t>((npix + 255) / 256, (int64_t)ctx->cu_count * 16);
        hipLaunchKernelGGL(surface_shade_kernel, dim3(grid), dim3(256), 0, st, filtered.as<float2>(), R, sp, lut.as<float4>(),
                           reinterpret_cast<uint32_t *>(ctx->out8));
        TSP_HIP(hipGetLastError());
    }
    TSP_HIP(hipEventRecord(ctx->ev[EV_T5], st));
    if (content_out) TSP_HIP(hipMemcpyAsync(content_out, filtered.p, (size_t)npix * sizeof(float2), hipMemcpyDeviceToHost, st));
    if (rgba8_out) TSP_HIP(hipMemcpyAsync(rgba8_out, ctx->out8, (size_t)npix * 4, hipMemcpyDeviceToHost, st));
    TSP_HIP(hipStreamSynchronize(st));
    if (ms_out) {
        float a = 0.f, b = 0.f;
        TSP_HIP(hipEventElapsedTime(&a, ctx->ev[EV_T3], ctx->ev[EV_T4]));
        TSP_HIP(hipEventElapsedTime(&b, ctx->ev[EV_T4], ctx->ev[EV_T5]));
        ms_out[0] = a;
        ms_out[1] = b;
    }
    return TSP_OK;
}

}  // namespace tsp
