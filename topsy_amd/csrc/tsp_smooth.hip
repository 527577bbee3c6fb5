// tsp_smooth.hip -- SPH smoothing lengths by k nearest neighbours (tsp_smoothing_lengths): what the reference asks of
// pynbody.sph.smooth when a snapshot carries no smoothing lengths (src/topsy/loader.py:222-240).
//
// Contract (include/topsy_splat.h): for every particle i with finite coordinates, h[i] = 0.5 * sqrt(the k-th smallest
// d2 = (dx*dx + dy*dy) + dz*dz over every particle j with finite coordinates, j = i included), in float32 with the operation
// order written out in dist2() below; a periodic box first maps each dx to its nearest image, dx - L * rint(dx / L).
// A particle with a non-finite coordinate gets NaN and is nobody's neighbour.
//
// The search:
//   1. bounding box of the finite positions; 63-bit Morton keys of the positions quantised to 2^21 steps per axis (a periodic
//      box: the positions wrapped into [0, L), for binning only -- distances always use the raw coordinates); invalid
//      particles get the key ~0 and sort last.  hipcub radix sort of (key, index), gather of the sorted x, y, z.
//   2. an upper bound r0 of every query's answer: the k-th smallest d2 over the 2k + 1 particles around it in Morton order
//      (any k real particles bound the k-th smallest from above).
//   3. the exact search: the prefixes of the sorted keys form an octree whose cells are contiguous runs.  The query takes the
//      finest level at which its box of half-width sqrt(r0) touches at most two cells per axis, finds those (at most eight)
//      runs by binary search and scans them -- its own cell first -- keeping the k smallest d2 in a sorted register list.
//      A cell whose box lies farther than the current k-th distance is skipped.  The box test is conservative: cell faces
//      are widened by a margin that covers the float32 rounding of the quantisation, the wrap and the distances themselves,
//      so a point the rounding puts into the neighbouring cell is still found.
//   4. h in the caller's order, scattered through the sort's index.
// One thread per query, queries in Morton order: the lanes of a wave share their cells, so the candidates they stream
// come from the same cache lines.
#include <hipcub/hipcub.hpp>

#include <math.h>
#include <stdlib.h>

#include "tsp_internal.h"

namespace tsp {
namespace {

constexpr int QBITS = 21;                          // quantisation steps per axis: 2^21 (3 x 21 = 63 key bits)
constexpr int QMAX = (1 << QBITS) - 1;
constexpr uint64_t INVALID_KEY = ~0ull;            // a particle with a non-finite coordinate: sorts after every valid key
constexpr float CULL_SLACK = 1.0f + 1e-5f;         // relative slack of every comparison between a box distance and a d2

struct Grid {
    float lo[3];       // quantisation origin (0 for a periodic box)
    float inv[3];      // steps per unit length; 0 on an axis of zero extent (every particle in step 0)
    float step[3];     // length of one step (0 with inv = 0)
    float eps;         // absolute margin of the box tests (rounding of the quantisation, the wrap and the cell faces)
    float period;      // 0: open box
};

__device__ __forceinline__ bool finite3(float x, float y, float z) {
    return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
}

// the position binned on axis a: wrapped into [0, L) in a periodic box
__device__ __forceinline__ float grid_coord(float v, float period) {
    return period > 0.0f ? v - period * floorf(v / period) : v;
}

// floor((v - lo) * inv), held inside +-2^23 (enough for any box of half-width up to the whole domain; an overflowing
// v - lo saturates instead of becoming undefined)
__device__ __forceinline__ int qstep(float v, float lo, float inv) {
    if (inv == 0.0f) return 0;
    float t = (v - lo) * inv;
    t = fminf(fmaxf(t, -8388608.0f), 8388608.0f);
    return (int)floorf(t);
}
__device__ __forceinline__ int qclamp(int u) { return min(max(u, 0), QMAX); }

__device__ __forceinline__ uint64_t spread3(uint64_t x) {     // 21 bits -> every third bit
    x &= 0x1fffffull;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}
__device__ __forceinline__ uint64_t morton3(uint32_t a, uint32_t b, uint32_t c) {
    return spread3(a) | (spread3(b) << 1) | (spread3(c) << 2);
}

// The contract's distance: float32, these operations in this order (-ffp-contract=off keeps them unfused).
__device__ __forceinline__ float min_image(float d, float period) {
    float t = __fdiv_rn(d, period);
    t = rintf(t);
    return d - period * t;
}
__device__ __forceinline__ float dist2(float qx, float qy, float qz, float px, float py, float pz, float period) {
    float dx = px - qx, dy = py - qy, dz = pz - qz;
    if (period > 0.0f) {
        dx = min_image(dx, period);
        dy = min_image(dy, period);
        dz = min_image(dz, period);
    }
    return (dx * dx + dy * dy) + dz * dz;
}

// The k smallest values so far, ascending, in KP registers (KP = k rounded up to 8, 16, 32 or 64).  The first KP - k entries
// hold -inf and are never displaced, so list[KP - 1] -- a compile-time index -- is always the k-th smallest value; every index
// is a constant, so the list stays in VGPRs (a run-time index would send it to scratch).
template <int KP>
__device__ __forceinline__ void list_init(float (&list)[KP], int k) {
#pragma unroll
    for (int t = 0; t < KP; ++t) list[t] = t < KP - k ? -__builtin_inff() : __builtin_inff();
}
template <int KP>
__device__ __forceinline__ void list_insert(float (&list)[KP], float d) {
    if (d < list[KP - 1]) {
#pragma unroll
        for (int t = KP - 1; t > 0; --t) list[t] = fmaxf(list[t - 1], fminf(list[t], d));
        list[0] = fminf(list[0], d);
    }
}

__device__ __forceinline__ unsigned ordered_bits(float f) {   // monotone float -> uint map
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ __forceinline__ float unordered_bits(unsigned u) {
    const unsigned v = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    float f;
    memcpy(&f, &v, 4);
    return f;
}

// min / max of every axis over the particles with finite coordinates, as ordered bits (mm: 3 minima, 3 maxima)
__global__ __launch_bounds__(256) void smooth_bbox_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                          const float *__restrict__ z, int64_t n, unsigned *mm) {
    unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0, 0, 0};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float v[3] = {x[i], y[i], z[i]};
        if (!finite3(v[0], v[1], v[2])) continue;
        for (int a = 0; a < 3; ++a) {
            const unsigned o = ordered_bits(v[a]);
            lo[a] = min(lo[a], o);
            hi[a] = max(hi[a], o);
        }
    }
    for (int a = 0; a < 3; ++a) {
        for (int off = 32; off; off >>= 1) {
            lo[a] = min(lo[a], (unsigned)__shfl_xor((int)lo[a], off));
            hi[a] = max(hi[a], (unsigned)__shfl_xor((int)hi[a], off));
        }
        if ((threadIdx.x & 63) == 0) {
            atomicMin(&mm[a], lo[a]);
            atomicMax(&mm[3 + a], hi[a]);
        }
    }
}

__global__ __launch_bounds__(256) void smooth_key_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                         const float *__restrict__ z, int64_t n, Grid g,
                                                         uint64_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                                         unsigned long long *n_valid) {
    unsigned long long valid = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float v[3] = {x[i], y[i], z[i]};
        uint64_t key = INVALID_KEY;
        if (finite3(v[0], v[1], v[2])) {
            uint32_t u[3];
            for (int a = 0; a < 3; ++a) u[a] = (uint32_t)qclamp(qstep(grid_coord(v[a], g.period), g.lo[a], g.inv[a]));
            key = morton3(u[0], u[1], u[2]);
            ++valid;
        }
        keys[i] = key;
        vals[i] = (uint32_t)i;
    }
    for (int off = 32; off; off >>= 1) valid += __shfl_xor(valid, off);
    if ((threadIdx.x & 63) == 0 && valid) atomicAdd(n_valid, valid);
}

__global__ __launch_bounds__(256) void smooth_gather_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                            const float *__restrict__ z, const uint32_t *__restrict__ idx,
                                                            int64_t nv, float *__restrict__ sx, float *__restrict__ sy,
                                                            float *__restrict__ sz) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t j = idx[i];
        sx[i] = x[j];
        sy[i] = y[j];
        sz[i] = z[j];
    }
}

__global__ __launch_bounds__(256) void smooth_scatter_kernel(const float *__restrict__ h_sorted, const uint32_t *__restrict__ idx,
                                                             int64_t n, int64_t nv, float *__restrict__ h) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        h[idx[i]] = i < nv ? h_sorted[i] : __builtin_nanf("");
}

// first index in [0, nv) whose key is >= key
__device__ __forceinline__ int64_t key_lower_bound(const uint64_t *__restrict__ keys, int64_t nv, uint64_t key) {
    int64_t lo = 0, hi = nv;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// distance along one axis from q to the step interval [c 2^s, (c + 1) 2^s) of the grid (and its periodic images), less the margin
__device__ __forceinline__ float axis_gap(const Grid &g, int a, float q, int c, int s) {
    if (g.inv[a] == 0.0f) return 0.0f;
    const float lo = g.lo[a] + ldexpf((float)c, s) * g.step[a];
    const float hi = g.lo[a] + ldexpf((float)(c + 1), s) * g.step[a];
    float d = fmaxf(fmaxf(lo - q, q - hi), 0.0f);
    if (g.period > 0.0f) {
        const float L = g.period;
        d = fminf(d, fmaxf(fmaxf(lo + L - q, q - hi - L), 0.0f));
        d = fminf(d, fmaxf(fmaxf(lo - L - q, q - hi + L), 0.0f));
    }
    return fmaxf(d - g.eps, 0.0f);
}

template <int KP>
__global__ __launch_bounds__(256) void smooth_knn_kernel(const float *__restrict__ sx, const float *__restrict__ sy,
                                                         const float *__restrict__ sz, const uint64_t *__restrict__ keys,
                                                         int64_t nv, int k, Grid g, float *__restrict__ h_sorted,
                                                         unsigned long long *n_dist) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long evaluated = 0;
    if (i < nv) {
        const float qx = sx[i], qy = sy[i], qz = sz[i];
        const float L = g.period;
        float list[KP];

        // 2. upper bound from the Morton-order window of 2k + 1 particles around the query
        list_init(list, k);
        const int64_t W = min(nv, (int64_t)(2 * k + 1));
        const int64_t w0 = min(max(i - (int64_t)k, (int64_t)0), nv - W);
        for (int64_t j = w0; j < w0 + W; ++j) list_insert(list, dist2(qx, qy, qz, sx[j], sy[j], sz[j], L));
        const float r0 = list[KP - 1];
        evaluated += (unsigned long long)W;

        // 3. the level at which the box of half-width R >= sqrt(r0) touches at most two cells per axis
        const float R = sqrtf(r0) * CULL_SLACK + g.eps;
        const float q[3] = {grid_coord(qx, L), grid_coord(qy, L), grid_coord(qz, L)};
        int uq[3], ua[3], ub[3];
        for (int a = 0; a < 3; ++a) {
            uq[a] = qclamp(qstep(q[a], g.lo[a], g.inv[a]));
            ua[a] = qstep(q[a] - R, g.lo[a], g.inv[a]);
            ub[a] = qstep(q[a] + R, g.lo[a], g.inv[a]);
            if (L == 0.0f) {
                ua[a] = qclamp(ua[a]);
                ub[a] = qclamp(ub[a]);
            }
            ua[a] = min(ua[a], uq[a]);      // the own cell is inside the range even where the wrap rounds q up to L
            ub[a] = max(ub[a], uq[a]);
        }
        int s = 0;
        while (s < QBITS && ((ub[0] >> s) - (ua[0] >> s) > 1 || (ub[1] >> s) - (ua[1] >> s) > 1 || (ub[2] >> s) - (ua[2] >> s) > 1))
            ++s;
        const int level = QBITS - s;
        const int ncell = 1 << level;
        // per axis: the query's own cell, and the other cell the box touches (unwrapped index; equal to own when none)
        int own[3], other[3];
        for (int a = 0; a < 3; ++a) {
            own[a] = uq[a] >> s;
            const int ca = ua[a] >> s, cb = ub[a] >> s;
            other[a] = (ncell == 1) ? own[a] : (ca != own[a] ? ca : cb);
        }
        list_init(list, k);
        for (int combo = 0; combo < 8; ++combo) {
            int c[3];
            bool skip = false;
            for (int a = 0; a < 3; ++a) {
                const bool second = (combo >> a) & 1;
                if (second && other[a] == own[a]) skip = true;
                c[a] = second ? other[a] : own[a];
            }
            if (skip) continue;
            const float bound = fminf(r0, list[KP - 1]) * CULL_SLACK;
            const float gx = axis_gap(g, 0, q[0], c[0], s);
            const float gy = axis_gap(g, 1, q[1], c[1], s);
            const float gz = axis_gap(g, 2, q[2], c[2], s);
            if ((gx * gx + gy * gy) + gz * gz > bound) continue;
            const uint64_t prefix = morton3((uint32_t)(c[0] & (ncell - 1)), (uint32_t)(c[1] & (ncell - 1)), (uint32_t)(c[2] & (ncell - 1)));
            const int shift = 3 * s;
            const int64_t b = key_lower_bound(keys, nv, prefix << shift);
            const int64_t e = key_lower_bound(keys, nv, (prefix + 1) << shift);
            for (int64_t j = b; j < e; ++j) list_insert(list, dist2(qx, qy, qz, sx[j], sy[j], sz[j], L));
            evaluated += (unsigned long long)(e - b);
        }
        h_sorted[i] = 0.5f * sqrtf(list[KP - 1]);     // correctly rounded here (__fsqrt_rn compiles to the 1-ulp v_sqrt_f32)
    }
    for (int off = 32; off; off >>= 1) evaluated += __shfl_xor(evaluated, off);
    if ((threadIdx.x & 63) == 0 && evaluated) atomicAdd(n_dist, evaluated);
}

#define SMOOTH_ALLOC(buf, bytes)                                                                                         \
    do {                                                                                                                 \
        const hipError_t e_ = (buf).alloc(bytes);                                                                        \
        if (e_ != hipSuccess) {                                                                                          \
            (void)hipGetLastError();                                                                                     \
            tsp::set_error("tsp_smoothing_lengths: cannot allocate %zu bytes of device memory: %s", (size_t)(bytes),     \
                           hipGetErrorString(e_));                                                                       \
            return e_ == hipErrorOutOfMemory ? TSP_ENOMEM : TSP_EHIP;                                                    \
        }                                                                                                                \
    } while (0)

}  // namespace

int smoothing_lengths(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, int k, float period,
                      float *h_out) {
    hipStream_t st = ctx->stream;
    const size_t fbytes = (size_t)n * sizeof(float);
    DeviceScratch dx, dy, dz, keys, keys2, vals, vals2, sx, sy, sz, mm;
    SMOOTH_ALLOC(dx, fbytes);
    SMOOTH_ALLOC(dy, fbytes);
    SMOOTH_ALLOC(dz, fbytes);
    SMOOTH_ALLOC(mm, 6 * sizeof(unsigned) + 2 * sizeof(unsigned long long));
    TSP_HIP(hipMemcpyAsync(dx.p, x, fbytes, hipMemcpyHostToDevice, st));
    TSP_HIP(hipMemcpyAsync(dy.p, y, fbytes, hipMemcpyHostToDevice, st));
    TSP_HIP(hipMemcpyAsync(dz.p, z, fbytes, hipMemcpyHostToDevice, st));

    // 1. bounding box, grid, keys, sort
    unsigned *d_mm = mm.as<unsigned>();
    unsigned long long *d_count = reinterpret_cast<unsigned long long *>(d_mm + 6);   // [0] valid particles, [1] distances
    const unsigned init[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0, 0, 0};
    TSP_HIP(hipMemcpyAsync(d_mm, init, sizeof(init), hipMemcpyHostToDevice, st));
    TSP_HIP(hipMemsetAsync(d_count, 0, 2 * sizeof(unsigned long long), st));
    const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(smooth_bbox_kernel, dim3(grid), dim3(256), 0, st, dx.as<float>(), dy.as<float>(), dz.as<float>(), n, d_mm);
    TSP_HIP(hipGetLastError());
    unsigned hmm[6];
    TSP_HIP(hipMemcpyAsync(hmm, d_mm, sizeof(hmm), hipMemcpyDeviceToHost, st));
    TSP_HIP(hipStreamSynchronize(st));

    Grid g = {};
    g.period = period;
    double maxabs = period;
    for (int a = 0; a < 3; ++a) {
        const float lo = unordered_bits(hmm[a]), hi = unordered_bits(hmm[3 + a]);
        if (hmm[a] > hmm[3 + a]) break;      // no finite particle at all (refused below)
        maxabs = std::max(maxabs, std::max(fabs((double)lo), fabs((double)hi)));
        const double extent = period > 0.0f ? (double)period : (double)hi - (double)lo;
        g.lo[a] = period > 0.0f ? 0.0f : lo;
        if (extent > 1e-30 && extent < 1e38) {
            g.inv[a] = (float)((double)(1 << QBITS) / extent);
            g.step[a] = (float)(extent / (double)(1 << QBITS));
        }
    }
    g.eps = (float)(1e-5 * maxabs) + 1e-30f;

    SMOOTH_ALLOC(keys, (size_t)n * sizeof(uint64_t));
    SMOOTH_ALLOC(keys2, (size_t)n * sizeof(uint64_t));
    SMOOTH_ALLOC(vals, (size_t)n * sizeof(uint32_t));
    SMOOTH_ALLOC(vals2, (size_t)n * sizeof(uint32_t));
    hipLaunchKernelGGL(smooth_key_kernel, dim3(grid), dim3(256), 0, st, dx.as<float>(), dy.as<float>(), dz.as<float>(), n, g,
                       keys.as<uint64_t>(), vals.as<uint32_t>(), d_count);
    TSP_HIP(hipGetLastError());
    unsigned long long nv_u = 0;
    TSP_HIP(hipMemcpyAsync(&nv_u, d_count, sizeof(nv_u), hipMemcpyDeviceToHost, st));
    TSP_HIP(hipStreamSynchronize(st));
    const int64_t nv = (int64_t)nv_u;
    TSP_REQUIRE(nv >= k, TSP_EINVAL, "tsp_smoothing_lengths: %lld particles have finite coordinates, n_neighbours = %d needs at least as many",
                (long long)nv, k);
    {
        DeviceScratch tmp;
        size_t tmp_bytes = 0;
        TSP_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, keys.as<uint64_t>(), keys2.as<uint64_t>(), vals.as<uint32_t>(),
                                                   vals2.as<uint32_t>(), (int)n, 0, 64, st));
        SMOOTH_ALLOC(tmp, tmp_bytes);
        TSP_HIP(hipcub::DeviceRadixSort::SortPairs(tmp.p, tmp_bytes, keys.as<uint64_t>(), keys2.as<uint64_t>(), vals.as<uint32_t>(),
                                                   vals2.as<uint32_t>(), (int)n, 0, 64, st));
        TSP_HIP(hipStreamSynchronize(st));
    }
    keys.reset(nullptr);
    SMOOTH_ALLOC(sx, (size_t)nv * sizeof(float));
    SMOOTH_ALLOC(sy, (size_t)nv * sizeof(float));
    SMOOTH_ALLOC(sz, (size_t)nv * sizeof(float));
    hipLaunchKernelGGL(smooth_gather_kernel, dim3(grid), dim3(256), 0, st, dx.as<float>(), dy.as<float>(), dz.as<float>(),
                       vals2.as<uint32_t>(), nv, sx.as<float>(), sy.as<float>(), sz.as<float>());
    TSP_HIP(hipGetLastError());

    // 2. + 3. one thread per query in Morton order; h_sorted reuses the unsorted index buffer
    float *h_sorted = vals.as<float>();
    const dim3 knn_grid((unsigned)((nv + 255) / 256));
    const uint64_t *sorted_keys = keys2.as<uint64_t>();
    if (k <= 8)
        hipLaunchKernelGGL(smooth_knn_kernel<8>, knn_grid, dim3(256), 0, st, sx.as<float>(), sy.as<float>(), sz.as<float>(), sorted_keys, nv, k, g, h_sorted, d_count + 1);
    else if (k <= 16)
        hipLaunchKernelGGL(smooth_knn_kernel<16>, knn_grid, dim3(256), 0, st, sx.as<float>(), sy.as<float>(), sz.as<float>(), sorted_keys, nv, k, g, h_sorted, d_count + 1);
    else if (k <= 32)
        hipLaunchKernelGGL(smooth_knn_kernel<32>, knn_grid, dim3(256), 0, st, sx.as<float>(), sy.as<float>(), sz.as<float>(), sorted_keys, nv, k, g, h_sorted, d_count + 1);
    else
        hipLaunchKernelGGL(smooth_knn_kernel<64>, knn_grid, dim3(256), 0, st, sx.as<float>(), sy.as<float>(), sz.as<float>(), sorted_keys, nv, k, g, h_sorted, d_count + 1);
    TSP_HIP(hipGetLastError());

    // 4. back to the caller's order (the raw x buffer is free now)
    hipLaunchKernelGGL(smooth_scatter_kernel, dim3(grid), dim3(256), 0, st, h_sorted, vals2.as<uint32_t>(), n, nv, dx.as<float>());
    TSP_HIP(hipGetLastError());
    unsigned long long n_dist = 0;
    TSP_HIP(hipMemcpyAsync(&n_dist, d_count + 1, sizeof(n_dist), hipMemcpyDeviceToHost, st));
    TSP_HIP(hipStreamSynchronize(st));
    TSP_HIP(hipMemcpy(h_out, dx.p, fbytes, hipMemcpyDeviceToHost));
    // measurement aid: TOPSY_SMOOTH_STATS=1 reports the distances evaluated per query (the search's cost over the k it needs)
    const char *env = getenv("TOPSY_SMOOTH_STATS");
    if (env && env[0] == '1')
        fprintf(stderr, "tsp_smoothing_lengths: n=%lld valid=%lld k=%d distances=%llu per_query=%.2f\n", (long long)n, (long long)nv,
                k, n_dist, nv ? (double)n_dist / (double)nv : 0.0);
    return TSP_OK;
}

}  // namespace tsp
