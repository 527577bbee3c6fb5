// tsp_center.hip -- the shrinking-sphere centre of a snapshot (tsp_shrink_sphere_center): what the reference asks of
// pynbody.analysis.halo.center when it centres a snapshot at load (src/topsy/loader.py:201-217; Power et al. 2003).
//
// Contract (include/topsy_splat.h), float64 unless said otherwise:
//   - particle i is valid iff x, y, z, mass[i] are finite and mass[i] > 0 and, with mass_cut_factor > 0,
//     (double)mass[i] < (double)mass_cut_factor * (double)m_min (m_min: the smallest mass among the otherwise valid particles);
//   - c = sum m p / sum m over the valid particles; r = r_start, or ((double)max x - (double)min x) / 2 over them;
//   - until max_iterations updates are done: r_try = r * shrink_factor; the inside set is the valid i with d2 < r_try * r_try,
//     dx = (double)x[i] - c[0] (dy, dz alike), d2 = (dx * dx + dy * dy) + dz * dz; fewer than min_particles members: stop;
//     else c += sum m (dx, dy, dz) / sum m over the set, r = r_try.
//
// The passes:
//   0. (mass_cut_factor > 0 only) m_min: an integer atomicMin over the bits of the positive finite masses.
//   1. center_prepare_kernel: the device copy of the masses becomes w[i] = valid ? mass[i] : 0, so that the later passes read
//      validity and selection as w > 0; the moments about the origin, the count, min / max x; and for every block of CBLK
//      consecutive particles the float32 bounding box of its valid members (an empty block: +inf .. -inf).
//   2. center_pass_kernel, once per iteration: a workgroup takes blocks blockIdx.x, blockIdx.x + gridDim.x, ...  A block whose
//      box lies at a squared distance >= r_try^2 from c is skipped unread.  The box distance is formed in float64 with the
//      operations and the order of d2 itself; subtraction, squaring and addition round monotonically, so no member of a skipped
//      block can have d2 < r_try^2: the skip never changes the inside set, points on a box face at distance r_try included.
//      Every other block is read as one float4 per lane and array (16 B per particle), tested and summed per lane in float64.
//   3. The lanes' sums are added over the wave by an xor butterfly, over the workgroup's four waves in wave order, and stored as
//      one partial per workgroup; center_final_kernel adds the partials in index order.  No floating-point atomic takes part, the
//      grid is a function of n and the device alone: the same call returns the same bits.
// The host reads the sums (64 bytes) after every pass and decides.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "tsp_blocks.h"
#include "tsp_internal.h"

namespace tsp {
namespace {

constexpr unsigned INF_BITS = 0x7f800000u;

struct Partial {                // 64 bytes: what a workgroup (and the whole pass) sums
    double sm, sx, sy, sz;      // sum m, sum m * (dx, dy, dz)   (prepare: m * (x, y, z))
    long long count;            // members
    double lo, hi;              // prepare: min / max of x over the members
    long long blocks;           // blocks read
};

__device__ __forceinline__ Partial partial_zero() {
    Partial a;
    a.sm = a.sx = a.sy = a.sz = 0.0;
    a.count = 0;
    a.lo = __builtin_inf();
    a.hi = -__builtin_inf();
    a.blocks = 0;
    return a;
}

__device__ __forceinline__ void partial_add(Partial &a, const Partial &b) {
    a.sm += b.sm;
    a.sx += b.sx;
    a.sy += b.sy;
    a.sz += b.sz;
    a.count += b.count;
    a.lo = fmin(a.lo, b.lo);
    a.hi = fmax(a.hi, b.hi);
    a.blocks += b.blocks;
}

// the workgroup's sum in a fixed order (butterfly over each wave, then the waves in order), stored by thread 0
__device__ __forceinline__ void workgroup_sum_store(Partial a, Partial *out) {
    __shared__ Partial wave_sum[4];
    for (int off = 32; off; off >>= 1) {
        Partial b;
        b.sm = __shfl_xor(a.sm, off);
        b.sx = __shfl_xor(a.sx, off);
        b.sy = __shfl_xor(a.sy, off);
        b.sz = __shfl_xor(a.sz, off);
        b.count = __shfl_xor(a.count, off);
        b.lo = __shfl_xor(a.lo, off);
        b.hi = __shfl_xor(a.hi, off);
        b.blocks = __shfl_xor(a.blocks, off);
        partial_add(a, b);
    }
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        Partial t = wave_sum[0];
        for (int w = 1; w < 4; ++w) partial_add(t, wave_sum[w]);
        *out = t;
    }
}

// 0. the smallest positive finite mass of a particle with finite coordinates (positive floats order as their bits)
__global__ __launch_bounds__(256) void center_min_mass_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                              const float *__restrict__ z, const float *__restrict__ m, int64_t n,
                                                              unsigned *min_bits) {
    unsigned lo = INF_BITS;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float mi = m[i];
        if (finite_position_and_mass(x[i], y[i], z[i], mi)) lo = min(lo, __float_as_uint(mi));
    }
    for (int off = 32; off; off >>= 1) lo = min(lo, (unsigned)__shfl_xor((int)lo, off));
    if ((threadIdx.x & 63) == 0 && lo != INF_BITS) atomicMin(min_bits, lo);
}

// 1. validity and selection into w, the moments about the origin, the block boxes.  The arrays are padded to whole blocks with
// zeros (a zero mass is invalid).
__global__ __launch_bounds__(256) void center_prepare_kernel(const float4 *__restrict__ x4, const float4 *__restrict__ y4,
                                                             const float4 *__restrict__ z4, float4 *__restrict__ w4,
                                                             int64_t nblocks, double mass_limit, float *__restrict__ boxes,
                                                             Partial *__restrict__ partials) {
    Partial a = partial_zero();
    for (int64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
        const int64_t i4 = b * (CBLK / 4) + threadIdx.x;
        const float4 X = x4[i4], Y = y4[i4], Z = z4[i4];
        float4 W = w4[i4];
        const float px[4] = {X.x, X.y, X.z, X.w}, py[4] = {Y.x, Y.y, Y.z, Y.w}, pz[4] = {Z.x, Z.y, Z.z, Z.w};
        float pw[4] = {W.x, W.y, W.z, W.w};
        float box[6];
        box_empty(box);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool ok = finite_position_and_mass(px[k], py[k], pz[k], pw[k]) && (double)pw[k] < mass_limit;
            if (ok) {
                const double m = (double)pw[k];
                a.sm += m;
                a.sx += m * (double)px[k];
                a.sy += m * (double)py[k];
                a.sz += m * (double)pz[k];
                ++a.count;
                a.lo = fmin(a.lo, (double)px[k]);
                a.hi = fmax(a.hi, (double)px[k]);
                box_include(box, px[k], py[k], pz[k]);
            } else {
                pw[k] = 0.0f;
            }
        }
        w4[i4] = make_float4(pw[0], pw[1], pw[2], pw[3]);
        workgroup_box_store(box, boxes + 6 * b);
        if (threadIdx.x == 0) ++a.blocks;
    }
    workgroup_sum_store(a, partials + blockIdx.x);
}

__device__ __forceinline__ void center_accumulate(Partial &a, float x, float y, float z, float w, double cx, double cy, double cz,
                                                  double r2) {
    if (w > 0.0f) {
        const double dx = (double)x - cx, dy = (double)y - cy, dz = (double)z - cz;
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 < r2) {
            const double m = (double)w;
            a.sm += m;
            a.sx += m * dx;
            a.sy += m * dy;
            a.sz += m * dz;
            ++a.count;
        }
    }
}

// 2. one iteration's sums over the valid particles inside the sphere of squared radius r2 around c
__global__ __launch_bounds__(256) void center_pass_kernel(const float4 *__restrict__ x4, const float4 *__restrict__ y4,
                                                          const float4 *__restrict__ z4, const float4 *__restrict__ w4,
                                                          const float *__restrict__ boxes, int64_t nblocks, double cx, double cy,
                                                          double cz, double r2, Partial *__restrict__ partials) {
    Partial a = partial_zero();
    for (int64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
        if (box_outside_sphere(boxes + 6 * b, cx, cy, cz, r2)) continue;      // (uniform over the workgroup)
        const int64_t i4 = b * (CBLK / 4) + threadIdx.x;
        const float4 X = x4[i4], Y = y4[i4], Z = z4[i4], W = w4[i4];
        center_accumulate(a, X.x, Y.x, Z.x, W.x, cx, cy, cz, r2);
        center_accumulate(a, X.y, Y.y, Z.y, W.y, cx, cy, cz, r2);
        center_accumulate(a, X.z, Y.z, Z.z, W.z, cx, cy, cz, r2);
        center_accumulate(a, X.w, Y.w, Z.w, W.w, cx, cy, cz, r2);
        if (threadIdx.x == 0) ++a.blocks;
    }
    workgroup_sum_store(a, partials + blockIdx.x);
}

// 3. the partials in index order (one workgroup: lane t takes t, t + 256, ...), into partials[n_partials]
__global__ __launch_bounds__(256) void center_final_kernel(Partial *__restrict__ partials, int n_partials) {
    Partial a = partial_zero();
    for (int i = threadIdx.x; i < n_partials; i += 256) partial_add(a, partials[i]);
    workgroup_sum_store(a, partials + n_partials);
}

}  // namespace

int shrink_sphere_center(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, const float *mass,
                         float mass_cut_factor, double r_start, double shrink_factor, int64_t min_particles, int max_iterations,
                         double center_out[3], tsp_center_info *info_out) {
    hipStream_t st = ctx->stream;
    // measurement aid: TOPSY_CENTER_STATS=1 reports the time of the upload, the preparation and every pass, and the blocks each
    // pass read
    const char *env = getenv("TOPSY_CENTER_STATS");
    const bool stats = env && env[0] == '1';
    const int64_t nblocks = (n + CBLK - 1) / CBLK, npad = nblocks * CBLK;
    const size_t fbytes = (size_t)n * sizeof(float), pad_bytes = (size_t)(npad - n) * sizeof(float);
    // workgroups: eight per CU at most, and two blocks each at least, so that every snapshot of more than one block takes the
    // stride loop (one path at every size)
    const int grid = (int)std::min<int64_t>((nblocks + 1) / 2, (int64_t)ctx->cu_count * 8);

    DeviceScratch dx, dy, dz, dw, dboxes, dpartials, dmin;
    TSP_SCRATCH_ALLOC(ctx, SITE("center_x"), dx, (size_t)npad * sizeof(float));
    TSP_SCRATCH_ALLOC(ctx, SITE("center_y"), dy, (size_t)npad * sizeof(float));
    TSP_SCRATCH_ALLOC(ctx, SITE("center_z"), dz, (size_t)npad * sizeof(float));
    TSP_SCRATCH_ALLOC(ctx, SITE("center_mass"), dw, (size_t)npad * sizeof(float));
    TSP_SCRATCH_ALLOC(ctx, SITE("center_boxes"), dboxes, (size_t)nblocks * 6 * sizeof(float));
    TSP_SCRATCH_ALLOC(ctx, SITE("center_partials"), dpartials, (size_t)(grid + 1) * sizeof(Partial));
    TSP_SCRATCH_ALLOC(ctx, SITE("center_min_mass"), dmin, sizeof(unsigned));

    auto t0 = std::chrono::steady_clock::now();
    const float *host[4] = {x, y, z, mass};
    DeviceScratch *dev[4] = {&dx, &dy, &dz, &dw};
    for (int a = 0; a < 4; ++a) {
        if (pad_bytes) TSP_HIP(hipMemsetAsync(dev[a]->as<float>() + n, 0, pad_bytes, st));
        TSP_HIP(hipMemcpyAsync(dev[a]->p, host[a], fbytes, hipMemcpyHostToDevice, st));
    }
    if (stats) TSP_HIP(hipStreamSynchronize(st));
    const double ms_upload = wall_ms(t0);

    t0 = std::chrono::steady_clock::now();
    double mass_limit = INFINITY;
    if (mass_cut_factor > 0.0f) {
        unsigned bits = INF_BITS;
        TSP_HIP(hipMemcpyAsync(dmin.p, &bits, sizeof(bits), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(center_min_mass_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, (int64_t)ctx->cu_count * 8)),
                           dim3(256), 0, st, dx.as<float>(), dy.as<float>(), dz.as<float>(), dw.as<float>(), n, dmin.as<unsigned>());
        TSP_HIP(hipGetLastError());
        TSP_HIP(hipMemcpyAsync(&bits, dmin.p, sizeof(bits), hipMemcpyDeviceToHost, st));
        TSP_HIP(hipStreamSynchronize(st));
        TSP_REQUIRE(bits != INF_BITS, TSP_EINVAL, "tsp_shrink_sphere_center: no particle has finite coordinates and a finite mass > 0");
        float m_min;
        memcpy(&m_min, &bits, sizeof(m_min));
        mass_limit = (double)mass_cut_factor * (double)m_min;
    }

    Partial *partials = dpartials.as<Partial>();
    Partial sum;
    auto reduce_and_read = [&]() -> int {
        hipLaunchKernelGGL(center_final_kernel, dim3(1), dim3(256), 0, st, partials, grid);
        TSP_HIP(hipGetLastError());
        TSP_HIP(hipMemcpyAsync(&sum, partials + grid, sizeof(sum), hipMemcpyDeviceToHost, st));
        TSP_HIP(hipStreamSynchronize(st));
        return TSP_OK;
    };
    hipLaunchKernelGGL(center_prepare_kernel, dim3(grid), dim3(256), 0, st, dx.as<float4>(), dy.as<float4>(), dz.as<float4>(),
                       dw.as<float4>(), nblocks, mass_limit, dboxes.as<float>(), partials);
    TSP_HIP(hipGetLastError());
    int rc = reduce_and_read();
    if (rc != TSP_OK) return rc;
    const double ms_prepare = wall_ms(t0);
    TSP_REQUIRE(sum.count > 0, TSP_EINVAL, "tsp_shrink_sphere_center: no particle has finite coordinates and a finite mass > 0");

    tsp_center_info info = {};
    info.n_valid = info.n_inside = sum.count;
    info.mass_inside = sum.sm;
    double c[3] = {sum.sx / sum.sm, sum.sy / sum.sm, sum.sz / sum.sm};
    double r = r_start > 0.0 ? r_start : (sum.hi - sum.lo) / 2.0;
    int iterations = 0;
    std::vector<double> pass_wall, pass_gpu;
    std::vector<long long> pass_blocks, pass_count;
    while (iterations < max_iterations) {
        const double r_try = r * shrink_factor;
        t0 = std::chrono::steady_clock::now();
        if (stats) TSP_HIP(hipEventRecord(ctx->ev[EV_T0], st));
        hipLaunchKernelGGL(center_pass_kernel, dim3(grid), dim3(256), 0, st, dx.as<float4>(), dy.as<float4>(), dz.as<float4>(),
                           dw.as<float4>(), dboxes.as<float>(), nblocks, c[0], c[1], c[2], r_try * r_try, partials);
        TSP_HIP(hipGetLastError());
        if (stats) TSP_HIP(hipEventRecord(ctx->ev[EV_T1], st));
        if ((rc = reduce_and_read()) != TSP_OK) return rc;
        if (stats) {
            float ms = 0.0f;
            TSP_HIP(hipEventElapsedTime(&ms, ctx->ev[EV_T0], ctx->ev[EV_T1]));
            pass_wall.push_back(wall_ms(t0));
            pass_gpu.push_back(ms);
            pass_blocks.push_back(sum.blocks);
            pass_count.push_back(sum.count);
        }
        if (sum.count < min_particles) break;
        c[0] += sum.sx / sum.sm;
        c[1] += sum.sy / sum.sm;
        c[2] += sum.sz / sum.sm;
        r = r_try;
        ++iterations;
        info.n_inside = sum.count;
        info.mass_inside = sum.sm;
    }
    info.iterations = iterations;
    info.radius = r;
    if (stats) {
        fprintf(stderr, "tsp_shrink_sphere_center: n=%lld valid=%lld blocks=%lld workgroups=%d upload_ms=%.3f prepare_ms=%.3f "
                        "iterations=%d\n", (long long)n, (long long)info.n_valid, (long long)nblocks, grid, ms_upload, ms_prepare,
                iterations);
        for (size_t k = 0; k < pass_gpu.size(); ++k)
            fprintf(stderr, "tsp_shrink_sphere_center: pass=%zu kernel_ms=%.4f wall_ms=%.4f blocks_read=%lld inside=%lld\n", k,
                    pass_gpu[k], pass_wall[k], pass_blocks[k], pass_count[k]);
    }
    center_out[0] = c[0];
    center_out[1] = c[1];
    center_out[2] = c[2];
    if (info_out) *info_out = info;
    return TSP_OK;
}

}  // namespace tsp
