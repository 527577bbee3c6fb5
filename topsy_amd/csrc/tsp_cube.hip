// tsp_cube.hip -- spectral cubes (tsp_spectral_cube, include/topsy_splat.h "Spectral cubes"): every resident particle drawn into a
// position-position-velocity cube, its kernel footprint on the image times the Gaussian of its line integrated over each channel.
//
// A gather over (image tile, channel block) bins, no floating-point atomics:
//   1. record pass: per particle of a slice the geometry (pcx, pcy, P, w0), the line (u, s, first and last channel) and the number
//      of (tile, block) pairs its footprint and line reach;
//   2. an exclusive scan of the pair counts, a fill pass that writes (bin, particle) in particle order, and a stable radix sort by
//      bin: every bin's list is in ascending particle index;
//   3. tile kernel: one 256-thread workgroup per bin, thread t owns pixel t of the tile and its CHANNEL_BLOCK float64 sums in LDS
//      ([channel][pixel]: a wave's accesses are consecutive, no two threads share a cell).  Eight list entries are staged per step:
//      thread t computes the channel response g of channel t & 31 of entry t >> 5 (float64 erf / erfc, once per entry and block) into
//      LDS; then every thread forms k for its pixel per entry and adds (k w0) g_c for the entry's channels.  At the end the
//      workgroup adds its sums to the float32 cube with plain loads and stores: it owns those cells for the launch.
// The slices' boundaries and every list capacity come from tsp_cube_layout.h.  Arithmetic in the order written, no contraction.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>

#include "tsp_cube_layout.h"
#include "tsp_internal.h"

namespace tsp {
namespace {

using namespace cube;

constexpr int STAGE = 8;      // list entries staged per step of the tile kernel: 256 threads = STAGE entries x CHANNEL_BLOCK channels
static_assert(STAGE * CHANNEL_BLOCK == 256 && TILE * TILE == 256, "one thread per pixel, and per (staged entry, channel)");
constexpr double TRUNCATE = 5.0;     // channels wholly further than this many s from u are skipped (erfc(5 / sqrt 2) = 5.8e-7)

struct Line {       // 24 bytes
    double s;       // line width, sqrt(sigma_v^2 + sigma_p^2)
    float u;        // velocity along the line of sight (the u of the kinematic weights)
    int c_lo, c_hi; // channels the particle adds to; c_lo > c_hi: none
    int pad;
};
static_assert(sizeof(Line) == 24 && sizeof(Line) + sizeof(float4) == RECORD_BYTES, "tsp_cube_layout.h sizes the records");

struct Channels {
    double v_min, dv;
    int n;
};
__device__ __forceinline__ double edge(const Channels &ch, int k) { return ch.v_min + (double)k * ch.dv; }

// the Gaussian of width s about u integrated over [e0, e1), without cancellation in the tails; s == 0: the indicator of the channel
__device__ double channel_response(double u, double s, double e0, double e1) {
    if (s == 0.0) return (e0 <= u && u < e1) ? 1.0 : 0.0;
    const double sqrt2 = 1.4142135623730951;
    const double a = (e0 - u) / s, b = (e1 - u) / s;
    if (a >= 0.0) return 0.5 * (erfc(a / sqrt2) - erfc(b / sqrt2));
    if (b <= 0.0) return 0.5 * (erfc(-b / sqrt2) - erfc(-a / sqrt2));
    return 0.5 * (erf(b / sqrt2) - erf(a / sqrt2));
}

struct LineOfSight {
    float a[3], v[3];
};

// the tiles a footprint's pixel range [lo, hi] reaches
__device__ __forceinline__ void tile_range(int lo, int hi, int &t_lo, int &t_hi) { t_lo = lo / TILE, t_hi = hi / TILE; }

// One lane per particle of the slice [first, first + count).  sigma is in the caller's order: read through the load-time permutation.
__global__ __launch_bounds__(256) void cube_record_kernel(Particles p, int64_t first, int count, Camera cam, LineOfSight los,
                                                          Channels ch, double sigma_v, const float *__restrict__ sigma,
                                                          float4 *__restrict__ geom, Line *__restrict__ line,
                                                          uint32_t *__restrict__ pairs) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t > count) return;
    if (t == count) {       // (the scan's last element: its exclusive sum is the slice's total)
        pairs[t] = 0;
        return;
    }
    const int64_t i = first + t;
    const float h = p.h[i], m = p.m[i];
    const Proj pr = project(cam, p.x[i], p.y[i], p.z[i], h);
    const float vx = p.vx[i], vy = p.vy[i], vz = p.vz[i];
    const float u = ((los.a[0] * (vx - los.v[0]) + los.a[1] * (vy - los.v[1])) + los.a[2] * (vz - los.v[2]));     // kinematic_weight's
    const float sp = sigma ? sigma[p.perm ? (int64_t)p.perm[i] : i] : 0.0f;
    const float hh = h * h;
    Line ln;
    ln.s = 0.0, ln.u = u, ln.c_lo = 1, ln.c_hi = 0, ln.pad = 0;
    int ilo = 1, ihi = 0, jlo = 1, jhi = 0;
    bool alive = pr.keep && finite_f32(m) && finite_f32(u) && finite_f32(sp) && sp >= 0.0f;
    if (alive) {
        cover_range(pr.pcx, pr.half, cam.R, ilo, ihi);
        cover_range(pr.pcy, pr.half, cam.R, jlo, jhi);
        alive = ilo <= ihi && jlo <= jhi;
    }
    if (alive) {
        const double s = sqrt(sigma_v * sigma_v + (double)sp * (double)sp), ud = (double)u;
        ln.s = s;
        // the channels [floor, floor] of u -+ TRUNCATE s, clamped while still in float64 (they may lie far outside the int range)
        double lo = floor(((ud - TRUNCATE * s) - ch.v_min) / ch.dv), hi = floor(((ud + TRUNCATE * s) - ch.v_min) / ch.dv);
        if (hi >= 0.0 && lo <= (double)(ch.n - 1)) {
            int c_lo = (int)(lo < 0.0 ? 0.0 : lo), c_hi = (int)(hi > (double)(ch.n - 1) ? (double)(ch.n - 1) : hi);
            if (s == 0.0) {     // the one channel with e_c <= u < e_{c+1}, decided by the edges themselves
                int c = c_lo;
                while (c > 0 && edge(ch, c) > ud) --c;
                while (c < ch.n - 1 && edge(ch, c + 1) <= ud) ++c;
                const bool inside = edge(ch, c) <= ud && ud < edge(ch, c + 1);
                c_lo = inside ? c : 1, c_hi = inside ? c : 0;
            }
            ln.c_lo = c_lo, ln.c_hi = c_hi;
        }
    }
    uint32_t n_pairs = 0;
    if (alive && ln.c_lo <= ln.c_hi) {
        int tx0, tx1, ty0, ty1;
        tile_range(ilo, ihi, tx0, tx1);
        tile_range(jlo, jhi, ty0, ty1);
        n_pairs = (uint32_t)(tx1 - tx0 + 1) * (uint32_t)(ty1 - ty0 + 1) * (uint32_t)(ln.c_hi / CHANNEL_BLOCK - ln.c_lo / CHANNEL_BLOCK + 1);
    } else {
        ln.c_lo = 1, ln.c_hi = 0;
    }
    geom[t] = make_float4(pr.pcx, pr.pcy, pr.P, m / hh);
    line[t] = ln;
    pairs[t] = n_pairs;
}

// One lane per particle: its pairs, bins ascending, at the offset the scan gave it.  The footprint's tiles are those of the record
// pass (the same cover_range of the same floats).
__global__ __launch_bounds__(256) void cube_fill_kernel(int count, int R, int tiles, int blocks, const float4 *__restrict__ geom,
                                                        const Line *__restrict__ line, const uint32_t *__restrict__ pairs,
                                                        const uint32_t *__restrict__ offset, uint32_t capacity,
                                                        uint32_t *__restrict__ keys, uint32_t *__restrict__ index) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= count || pairs[t] == 0) return;
    const float4 g = geom[t];
    const Line ln = line[t];
    int ilo, ihi, jlo, jhi, tx0, tx1, ty0, ty1;
    cover_range(g.x, 0.5f * g.z, R, ilo, ihi);
    cover_range(g.y, 0.5f * g.z, R, jlo, jhi);
    tile_range(ilo, ihi, tx0, tx1);
    tile_range(jlo, jhi, ty0, ty1);
    uint32_t o = offset[t];
    const uint32_t end = o + pairs[t];
    for (int ty = ty0; ty <= ty1; ++ty)
        for (int tx = tx0; tx <= tx1; ++tx)
            for (int b = ln.c_lo / CHANNEL_BLOCK; b <= ln.c_hi / CHANNEL_BLOCK; ++b) {
                if (o >= end || o >= capacity) return;      // (cannot happen: the counts are the record pass's; never write past the lists)
                keys[o] = (uint32_t)((ty * tiles + tx) * blocks + b);
                index[o] = (uint32_t)t;
                ++o;
            }
}

// first and end entry of every bin in the sorted keys (both zeroed before: an empty bin has first == end == 0)
__global__ __launch_bounds__(256) void cube_bounds_kernel(const uint32_t *__restrict__ keys, uint32_t total, uint32_t bins,
                                                          uint32_t *__restrict__ bin_first, uint32_t *__restrict__ bin_end) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= total) return;
    const uint32_t k = keys[e];
    if (k >= bins) return;
    if (e == 0 || keys[e - 1] != k) bin_first[k] = e;
    if (e + 1 == total || keys[e + 1] != k) bin_end[k] = e + 1;
}

// One workgroup per (tile, block) bin.  Dynamic LDS: the sums [CHANNEL_BLOCK][256] float64, then the responses [2][STAGE][CHANNEL_BLOCK].
__global__ __launch_bounds__(256) void cube_tile_kernel(const float4 *__restrict__ geom, const Line *__restrict__ line,
                                                        const uint32_t *__restrict__ list, const uint32_t *__restrict__ bin_first,
                                                        const uint32_t *__restrict__ bin_end, int tiles, int blocks, int R, Channels ch,
                                                        const float *__restrict__ T, float *__restrict__ cube_out) {
    extern __shared__ double lds[];
    double *acc = lds, *resp = lds + CHANNEL_BLOCK * 256;
    __shared__ float4 s_geom[2][STAGE];
    __shared__ int2 s_range[2][STAGE];

    const uint32_t bin = blockIdx.x;
    const uint32_t begin = bin_first[bin], end = bin_end[bin];
    if (begin >= end) return;                       // (uniform: an empty bin)
    const int block = (int)(bin % (uint32_t)blocks), tile = (int)(bin / (uint32_t)blocks);
    const int ty = tile / tiles, tx = tile - ty * tiles;
    const int t = threadIdx.x;
    const int px = tx * TILE + (t & (TILE - 1)), py = ty * TILE + (t >> 4);
    const bool inside = px < R && py < R;
    const float fx = (float)px, fy = (float)py;
    const int c0 = block * CHANNEL_BLOCK;
#pragma unroll
    for (int c = 0; c < CHANNEL_BLOCK; ++c) acc[c * 256 + t] = 0.0;       // (thread t alone ever touches column t)

    const int sj = t >> 5, sc = t & (CHANNEL_BLOCK - 1);        // what this thread stages: entry sj of the step, channel c0 + sc
    int touched_lo = CHANNEL_BLOCK, touched_hi = -1;
    int buf = 0;
    for (uint32_t e0 = begin; e0 < end; e0 += STAGE, buf ^= 1) {
        const uint32_t e = e0 + (uint32_t)sj;
        if (e < end) {
            const uint32_t idx = list[e];
            const Line ln = line[idx];
            const int c = c0 + sc;
            double g = 0.0;
            if (c >= ln.c_lo && c <= ln.c_hi) g = channel_response((double)ln.u, ln.s, edge(ch, c), edge(ch, c + 1));
            resp[(buf * STAGE + sj) * CHANNEL_BLOCK + sc] = g;
            if (sc == 0) {
                s_geom[buf][sj] = geom[idx];
                s_range[buf][sj] = make_int2(max(ln.c_lo, c0) - c0, min(ln.c_hi, c0 + CHANNEL_BLOCK - 1) - c0);
            }
        }
        // one barrier per step: the buffers alternate, and a thread stages step k + 1 only after it has read step k - 1
        __syncthreads();
        const int staged = (int)min((uint32_t)STAGE, end - e0);
        for (int j = 0; j < staged; ++j) {
            const float4 g4 = s_geom[buf][j];
            const int2 rg = s_range[buf][j];
            if (rg.x <= rg.y) touched_lo = min(touched_lo, rg.x), touched_hi = max(touched_hi, rg.y);
            Proj pr;
            pr.pcx = g4.x, pr.pcy = g4.y, pr.P = g4.z, pr.half = 0.5f * g4.z;
            if (!(inside && covers(pr.pcx, pr.half, fx) && covers(pr.pcy, pr.half, fy))) continue;
            pr.invP = 1.0f / pr.P;
            const float dx = (fx + 0.5f) - pr.pcx, dy = (fy + 0.5f) - pr.pcy;
            const float k = sample_kernel(T, pr, level_for(pr.P), dx, dy);
            const double kw = (double)k * (double)g4.w;
            const double *r = resp + (buf * STAGE + j) * CHANNEL_BLOCK;
            for (int c = rg.x; c <= rg.y; ++c) acc[c * 256 + t] += kw * r[c];
        }
    }
    if (!inside) return;
    for (int c = touched_lo; c <= touched_hi; ++c) {          // (c0 + c < n_channels: a line's channels are)
        float *cell = cube_out + ((size_t)(c0 + c) * R + py) * R + px;
        *cell = (float)((double)*cell + acc[c * 256 + t]);
    }
}

constexpr size_t TILE_LDS = (size_t)(CHANNEL_BLOCK * 256 + 2 * STAGE * CHANNEL_BLOCK) * sizeof(double);
constexpr uint32_t ATTR_BIT_CUBE = 1u << 24;        // tsp_context::kernel_attr_done

int ceil_blocks(int64_t n) { return (int)((n + 255) / 256); }

}  // namespace

// The host side of tsp_spectral_cube (the arguments are checked by the entry point).  Device memory through the two sites of the
// gather calls, carved by tsp_cube_layout.h; nothing of the context changes.
int spectral_cube(tsp_context *ctx, const Camera &cam, double v_min, double dv, int n_channels, double sigma_v, const float *sigma,
                  float *cube_out) {
    hipStream_t st = ctx->stream;
    const Particles &p = ctx->p;
    const int R = ctx->R;
    const int64_t n = p.n;
    const Grid grid = grid_of(R, n_channels);
    const int64_t per_slice = slice_particles(n, R, n_channels, ctx->cube_slice_particles);
    const int64_t n_slices = slice_count(n, per_slice);
    const int64_t capacity = list_capacity(per_slice, grid);

    size_t scan_bytes = 0, sort_bytes = 0;
    TSP_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, (int)(per_slice + 1), st));
    TSP_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                               (uint32_t *)nullptr, (int)capacity, 0, grid.key_bits, st));
    const Carve c = carve(n, per_slice, R, n_channels, sigma != nullptr, std::max(scan_bytes, sort_bytes));

    DeviceScratch dh, da;
    const int rc_scratch = gather_scratch(ctx, dh, c.h_bytes, da, c.a_bytes);
    if (rc_scratch != TSP_OK) return rc_scratch;
    char *hb = dh.as<char>(), *ab = da.as<char>();
    float *d_sigma = sigma ? reinterpret_cast<float *>(hb + c.h_sigma) : nullptr;
    float4 *d_geom = reinterpret_cast<float4 *>(hb + c.h_geom);
    Line *d_line = reinterpret_cast<Line *>(hb + c.h_line);
    float *d_cube = reinterpret_cast<float *>(ab + c.a_cube);
    uint32_t *d_count = reinterpret_cast<uint32_t *>(ab + c.a_count), *d_offset = reinterpret_cast<uint32_t *>(ab + c.a_offset);
    uint32_t *d_keys = reinterpret_cast<uint32_t *>(ab + c.a_keys), *d_keys_sorted = reinterpret_cast<uint32_t *>(ab + c.a_keys_sorted);
    uint32_t *d_index = reinterpret_cast<uint32_t *>(ab + c.a_index), *d_index_sorted = reinterpret_cast<uint32_t *>(ab + c.a_index_sorted);
    uint32_t *d_bin_first = reinterpret_cast<uint32_t *>(ab + c.a_bin_first), *d_bin_end = reinterpret_cast<uint32_t *>(ab + c.a_bin_end);
    void *d_tmp = ab + c.a_tmp;

    if (!(ctx->kernel_attr_done & ATTR_BIT_CUBE)) {      // (more than 64 KB of dynamic LDS needs the attribute)
        TSP_HIP(hipFuncSetAttribute((const void *)cube_tile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TILE_LDS));
        ctx->kernel_attr_done |= ATTR_BIT_CUBE;
    }
    const size_t cube_bytes = (size_t)n_channels * R * R * sizeof(float);
    TSP_HIP(hipMemsetAsync(d_cube, 0, cube_bytes, st));
    if (sigma) TSP_HIP(hipMemcpyAsync(d_sigma, sigma, (size_t)n * sizeof(float), hipMemcpyHostToDevice, st));
    LineOfSight los;
    for (int k = 0; k < 3; ++k) { los.a[k] = ctx->los[k]; los.v[k] = ctx->los[3 + k]; }
    const Channels ch = {v_min, dv, n_channels};

    for (int64_t k = 0; k < n_slices; ++k) {
        int64_t first, count;
        slice_range(n, per_slice, k, &first, &count);
        hipLaunchKernelGGL(cube_record_kernel, dim3(ceil_blocks(count + 1)), dim3(256), 0, st, p, first, (int)count, cam, los, ch, sigma_v,
                           d_sigma, d_geom, d_line, d_count);
        TSP_HIP(hipGetLastError());
        size_t bytes = scan_bytes;
        TSP_HIP(hipcub::DeviceScan::ExclusiveSum(d_tmp, bytes, d_count, d_offset, (int)(count + 1), st));
        uint32_t total = 0;
        TSP_HIP(hipMemcpyAsync(&total, d_offset + count, sizeof(total), hipMemcpyDeviceToHost, st));
        TSP_HIP(hipStreamSynchronize(st));
        if (total == 0) continue;
        TSP_REQUIRE((int64_t)total <= capacity, TSP_ESTATE, "spectral cube: a slice emitted %u pairs, above the lists' %lld", total,
                    (long long)capacity);
        hipLaunchKernelGGL(cube_fill_kernel, dim3(ceil_blocks(count)), dim3(256), 0, st, (int)count, R, grid.tiles, grid.blocks, d_geom,
                           d_line, d_count, d_offset, (uint32_t)capacity, d_keys, d_index);
        TSP_HIP(hipGetLastError());
        bytes = sort_bytes;
        TSP_HIP(hipcub::DeviceRadixSort::SortPairs(d_tmp, bytes, d_keys, d_keys_sorted, d_index, d_index_sorted, (int)total, 0,
                                                   grid.key_bits, st));
        TSP_HIP(hipMemsetAsync(d_bin_first, 0, (size_t)grid.bins * 4, st));
        TSP_HIP(hipMemsetAsync(d_bin_end, 0, (size_t)grid.bins * 4, st));
        hipLaunchKernelGGL(cube_bounds_kernel, dim3(ceil_blocks(total)), dim3(256), 0, st, d_keys_sorted, total, (uint32_t)grid.bins,
                           d_bin_first, d_bin_end);
        TSP_HIP(hipGetLastError());
        hipLaunchKernelGGL(cube_tile_kernel, dim3((unsigned)grid.bins), dim3(256), TILE_LDS, st, d_geom, d_line, d_index_sorted, d_bin_first,
                           d_bin_end, grid.tiles, grid.blocks, R, ch, ctx->mips, d_cube);
        TSP_HIP(hipGetLastError());
    }
    TSP_HIP(hipMemcpyAsync(cube_out, d_cube, cube_bytes, hipMemcpyDeviceToHost, st));
    TSP_HIP(hipStreamSynchronize(st));
    return TSP_OK;
}

}  // namespace tsp
