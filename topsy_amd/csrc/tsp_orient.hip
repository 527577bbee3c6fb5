// tsp_orient.hip -- the moments of the particles inside a sphere (tsp_sphere_moments): the mass, the centre of mass, the angular
// momentum about the sphere's own mean velocity and the second-moment tensor, from which the host layer takes the rotation that
// shows a disc face-on or side-on (pynbody.analysis.angmom.faceon / sideon: the velocity centre of a small sphere, then L of a
// larger one).
//
// Contract (include/topsy_splat.h), float64 unless said otherwise, nothing fused:
//   - particle i is valid iff x, y, z, mass[i] (and vx, vy, vz[i] when given) are finite and mass[i] > 0;
//   - dx = (double)x[i] - center[0] (dy, dz alike), d2 = (dx * dx + dy * dy) + dz * dz; inside a sphere of radius s: d2 < s * s;
//   - pass A (with velocities): sum m, sum m v and the count over the r_vel sphere; v_cen = sum m v / sum m on the host;
//   - pass B: over the r sphere the count, sum m, sum m d, S = sum m d_i d_j and, with velocities, u = (double)v - v_cen,
//     L = sum m d x u, A = sum m sqrt(d2) sqrt((ux * ux + uy * uy) + uz * uz).
//
// The passes, in the shape of tsp_center.hip (tsp_blocks.h holds what the two files share):
//   1. orient_prepare_kernel: the device copy of the masses becomes w[i] = valid ? mass[i] : 0, so that the passes read validity
//      as w > 0; the valid count; and for every block of CBLK consecutive particles the float32 bounding box of its valid members.
//   2. orient_pass_kernel<VEL, FULL>: a workgroup takes blocks blockIdx.x, blockIdx.x + gridDim.x, ...  A block whose box lies
//      at a squared distance >= s^2 from the centre is skipped unread (box_outside_sphere: no member of a skipped block can have
//      d2 < s^2, so the skip never changes a sum).  Every other block is read as one float4 per lane and array -- 16 B per
//      particle, 28 B with velocities -- and summed per lane in float64: pass A carries 4 sums, pass B 14 with velocities and 10
//      without, and a count each.
//   3. The lanes' sums are added over the wave by an xor butterfly, over the workgroup's four waves in wave order, and stored as
//      one partial per workgroup; orient_final_kernel adds the partials in index order.  No floating-point atomic takes part
//      (the valid count is an integer atomic), the grid is a function of n and the device alone: the same call returns the same
//      bits.
// Registers: pass B holds 14 float64 sums (28 VGPRs) and seven float4 loads (28 VGPRs) per lane, which with the arithmetic is
// above the 64 VGPRs that eight waves per SIMD would allow.  __launch_bounds__(256, 4) asks for no more than four waves per SIMD
// (128 VGPRs), so that the allocator is never pushed into spilling the sums; as built pass B with velocities takes 84 VGPRs (five
// waves per SIMD, five workgroups per CU), pass A and pass B without velocities 62 (eight), none spills.  The passes stream with
// no reuse and few instructions per byte: twenty waves per CU with seven 16-byte loads in flight each cover the memory latency.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "tsp_blocks.h"
#include "tsp_internal.h"

namespace tsp {
namespace {

constexpr int NSUM = 14;        // sums of pass B: mass | m d (3) | L (3) | S xx xy xz yy yz zz (6) | A; pass A: mass | m v (3)
enum { S_MASS = 0, S_MD = 1, S_L = 4, S_S = 7, S_A = 13 };

struct Sums {                   // what a lane, a workgroup and a whole pass sum
    double s[NSUM];
    long long count;            // members
    long long blocks;           // blocks read
};

__device__ __forceinline__ Sums sums_zero() {
    Sums a;
#pragma unroll
    for (int k = 0; k < NSUM; ++k) a.s[k] = 0.0;
    a.count = a.blocks = 0;
    return a;
}

__device__ __forceinline__ void sums_add(Sums &a, const Sums &b) {
#pragma unroll
    for (int k = 0; k < NSUM; ++k) a.s[k] += b.s[k];
    a.count += b.count;
    a.blocks += b.blocks;
}

// the workgroup's sum in a fixed order (butterfly over each wave, then the waves in order), stored by thread 0
__device__ __forceinline__ void workgroup_sum_store(Sums a, Sums *out) {
    __shared__ Sums wave_sum[4];
    for (int off = 32; off; off >>= 1) {
        Sums b;
#pragma unroll
        for (int k = 0; k < NSUM; ++k) b.s[k] = __shfl_xor(a.s[k], off);
        b.count = __shfl_xor(a.count, off);
        b.blocks = __shfl_xor(a.blocks, off);
        sums_add(a, b);
    }
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        Sums t = wave_sum[0];
        for (int w = 1; w < 4; ++w) sums_add(t, wave_sum[w]);
        *out = t;
    }
}

__device__ __forceinline__ void unpack(const float4 &v, float out[4]) {
    out[0] = v.x;
    out[1] = v.y;
    out[2] = v.z;
    out[3] = v.w;
}

// 1. validity into w, the valid count, the block boxes.  The arrays are padded to whole blocks with zeros (a zero mass is
// invalid).
template <bool VEL>
__global__ __launch_bounds__(256) void orient_prepare_kernel(const float4 *__restrict__ x4, const float4 *__restrict__ y4,
                                                             const float4 *__restrict__ z4, float4 *__restrict__ w4,
                                                             const float4 *__restrict__ vx4, const float4 *__restrict__ vy4,
                                                             const float4 *__restrict__ vz4, int64_t nblocks,
                                                             float *__restrict__ boxes, unsigned long long *__restrict__ n_valid) {
    unsigned count = 0;
    for (int64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
        const int64_t i4 = b * (CBLK / 4) + threadIdx.x;
        float px[4], py[4], pz[4], pw[4], pu[4] = {0, 0, 0, 0}, pv[4] = {0, 0, 0, 0}, pq[4] = {0, 0, 0, 0};
        unpack(x4[i4], px);
        unpack(y4[i4], py);
        unpack(z4[i4], pz);
        unpack(w4[i4], pw);
        if (VEL) {
            unpack(vx4[i4], pu);
            unpack(vy4[i4], pv);
            unpack(vz4[i4], pq);
        }
        float box[6];
        box_empty(box);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool ok = finite_position_and_mass(px[k], py[k], pz[k], pw[k]) &&
                            (!VEL || (__builtin_isfinite(pu[k]) && __builtin_isfinite(pv[k]) && __builtin_isfinite(pq[k])));
            if (ok) {
                ++count;
                box_include(box, px[k], py[k], pz[k]);
            } else {
                pw[k] = 0.0f;
            }
        }
        w4[i4] = make_float4(pw[0], pw[1], pw[2], pw[3]);
        workgroup_box_store(box, boxes + 6 * b);
    }
    for (int off = 32; off; off >>= 1) count += (unsigned)__shfl_xor((int)count, off);
    if ((threadIdx.x & 63) == 0 && count) atomicAdd(n_valid, (unsigned long long)count);
}

// pass A: the mass and the momentum of a member
__device__ __forceinline__ void accumulate_velocity_centre(Sums &a, float x, float y, float z, float w, float vx, float vy, float vz,
                                                           double cx, double cy, double cz, double r2) {
    if (w > 0.0f) {
        const double dx = (double)x - cx, dy = (double)y - cy, dz = (double)z - cz;
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 < r2) {
            const double m = (double)w;
            a.s[S_MASS] += m;
            a.s[S_MD + 0] += m * (double)vx;
            a.s[S_MD + 1] += m * (double)vy;
            a.s[S_MD + 2] += m * (double)vz;
            ++a.count;
        }
    }
}

// pass B: the moments of a member
template <bool VEL>
__device__ __forceinline__ void accumulate_moments(Sums &a, float x, float y, float z, float w, float vx, float vy, float vz,
                                                   double cx, double cy, double cz, double r2, double ox, double oy, double oz) {
    if (w > 0.0f) {
        const double dx = (double)x - cx, dy = (double)y - cy, dz = (double)z - cz;
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 < r2) {
            const double m = (double)w;
            const double mx = m * dx, my = m * dy, mz = m * dz;
            a.s[S_MASS] += m;
            a.s[S_MD + 0] += mx;
            a.s[S_MD + 1] += my;
            a.s[S_MD + 2] += mz;
            a.s[S_S + 0] += mx * dx;
            a.s[S_S + 1] += mx * dy;
            a.s[S_S + 2] += mx * dz;
            a.s[S_S + 3] += my * dy;
            a.s[S_S + 4] += my * dz;
            a.s[S_S + 5] += mz * dz;
            ++a.count;
            if (VEL) {
                const double ux = (double)vx - ox, uy = (double)vy - oy, uz = (double)vz - oz;
                a.s[S_L + 0] += m * (dy * uz - dz * uy);
                a.s[S_L + 1] += m * (dz * ux - dx * uz);
                a.s[S_L + 2] += m * (dx * uy - dy * ux);
                a.s[S_A] += m * sqrt(d2) * sqrt((ux * ux + uy * uy) + uz * uz);
            }
        }
    }
}

// 2. the sums over the valid particles inside the sphere of squared radius r2 around c.  FULL = false: pass A (the velocity
// centre; VEL is true); FULL = true: pass B, about the velocity (ox, oy, oz) when VEL.
template <bool VEL, bool FULL>
__global__ __launch_bounds__(256, 4) void orient_pass_kernel(const float4 *__restrict__ x4, const float4 *__restrict__ y4,
                                                             const float4 *__restrict__ z4, const float4 *__restrict__ w4,
                                                             const float4 *__restrict__ vx4, const float4 *__restrict__ vy4,
                                                             const float4 *__restrict__ vz4, const float *__restrict__ boxes,
                                                             int64_t nblocks, double cx, double cy, double cz, double r2, double ox,
                                                             double oy, double oz, Sums *__restrict__ partials) {
    Sums a = sums_zero();
    for (int64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
        if (box_outside_sphere(boxes + 6 * b, cx, cy, cz, r2)) continue;      // (uniform over the workgroup)
        const int64_t i4 = b * (CBLK / 4) + threadIdx.x;
        float px[4], py[4], pz[4], pw[4], pu[4] = {0, 0, 0, 0}, pv[4] = {0, 0, 0, 0}, pq[4] = {0, 0, 0, 0};
        unpack(x4[i4], px);
        unpack(y4[i4], py);
        unpack(z4[i4], pz);
        unpack(w4[i4], pw);
        if (VEL) {
            unpack(vx4[i4], pu);
            unpack(vy4[i4], pv);
            unpack(vz4[i4], pq);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (FULL) accumulate_moments<VEL>(a, px[k], py[k], pz[k], pw[k], pu[k], pv[k], pq[k], cx, cy, cz, r2, ox, oy, oz);
            else accumulate_velocity_centre(a, px[k], py[k], pz[k], pw[k], pu[k], pv[k], pq[k], cx, cy, cz, r2);
        }
        if (threadIdx.x == 0) ++a.blocks;
    }
    workgroup_sum_store(a, partials + blockIdx.x);
}

// 3. the partials in index order (one workgroup: lane t takes t, t + 256, ...), into partials[n_partials]
__global__ __launch_bounds__(256) void orient_final_kernel(Sums *__restrict__ partials, int n_partials) {
    Sums a = sums_zero();
    for (int i = threadIdx.x; i < n_partials; i += 256) sums_add(a, partials[i]);
    workgroup_sum_store(a, partials + n_partials);
}

}  // namespace

int sphere_moments(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, const float *mass, const float *vx,
                   const float *vy, const float *vz, const double center[3], double r, double r_vel, tsp_moments *out) {
    hipStream_t st = ctx->stream;
    // measurement aid: TOPSY_ORIENT_STATS=1 reports the time of the upload, the preparation and each pass, and the blocks each
    // pass read
    const char *env = getenv("TOPSY_ORIENT_STATS");
    const bool stats = env && env[0] == '1';
    const bool vel = vx != nullptr;
    const int n_arrays = vel ? 7 : 4;
    const int64_t nblocks = (n + CBLK - 1) / CBLK, npad = nblocks * CBLK;
    const size_t fbytes = (size_t)n * sizeof(float), pad_bytes = (size_t)(npad - n) * sizeof(float);
    // workgroups: eight per CU at most (they queue where fewer are resident), and two blocks each at least, so that every
    // snapshot of more than one block takes the stride loop (one path at every size)
    const int grid = (int)std::min<int64_t>((nblocks + 1) / 2, (int64_t)ctx->cu_count * 8);

    const float *host[7] = {x, y, z, mass, vx, vy, vz};
    static const char *const dev_site[7] = {SITE("moments_x"),  SITE("moments_y"),  SITE("moments_z"), SITE("moments_mass"),
                                            SITE("moments_vx"), SITE("moments_vy"), SITE("moments_vz")};
    DeviceScratch dev[7], dboxes, dpartials, dcount;
    for (int a = 0; a < n_arrays; ++a) TSP_SCRATCH_ALLOC(ctx, dev_site[a], dev[a], (size_t)npad * sizeof(float));
    TSP_SCRATCH_ALLOC(ctx, SITE("moments_boxes"), dboxes, (size_t)nblocks * 6 * sizeof(float));
    TSP_SCRATCH_ALLOC(ctx, SITE("moments_partials"), dpartials, (size_t)(grid + 1) * sizeof(Sums));
    TSP_SCRATCH_ALLOC(ctx, SITE("moments_valid_count"), dcount, sizeof(unsigned long long));

    auto t0 = std::chrono::steady_clock::now();
    for (int a = 0; a < n_arrays; ++a) {
        if (pad_bytes) TSP_HIP(hipMemsetAsync(dev[a].as<float>() + n, 0, pad_bytes, st));
        TSP_HIP(hipMemcpyAsync(dev[a].p, host[a], fbytes, hipMemcpyHostToDevice, st));
    }
    TSP_HIP(hipMemsetAsync(dcount.p, 0, sizeof(unsigned long long), st));
    if (stats) TSP_HIP(hipStreamSynchronize(st));
    const double ms_upload = wall_ms(t0);

    const float4 *x4 = dev[0].as<float4>(), *y4 = dev[1].as<float4>(), *z4 = dev[2].as<float4>(), *w4 = dev[3].as<float4>();
    const float4 *vx4 = dev[4].as<float4>(), *vy4 = dev[5].as<float4>(), *vz4 = dev[6].as<float4>();     // null without velocities
    t0 = std::chrono::steady_clock::now();
    hipLaunchKernelGGL(vel ? orient_prepare_kernel<true> : orient_prepare_kernel<false>, dim3(grid), dim3(256), 0, st, x4, y4, z4,
                       dev[3].as<float4>(), vx4, vy4, vz4, nblocks, dboxes.as<float>(), dcount.as<unsigned long long>());
    TSP_HIP(hipGetLastError());
    unsigned long long n_valid = 0;
    TSP_HIP(hipMemcpyAsync(&n_valid, dcount.p, sizeof(n_valid), hipMemcpyDeviceToHost, st));
    TSP_HIP(hipStreamSynchronize(st));
    const double ms_prepare = wall_ms(t0);
    TSP_REQUIRE(n_valid > 0, TSP_EINVAL, "tsp_sphere_moments: no particle has finite coordinates%s and a finite mass > 0",
                vel ? " and velocities" : "");

    Sums *partials = dpartials.as<Sums>();
    Sums sum;
    float pass_ms[2] = {0.0f, 0.0f};
    long long pass_blocks[2] = {0, 0};
    // one pass over the sphere of radius s: the launch, the sum of the partials, the read-back
    auto run_pass = [&](int which, double s, const double o[3]) -> int {
        if (stats) TSP_HIP(hipEventRecord(ctx->ev[EV_T0], st));
        auto kernel = which == 0 ? orient_pass_kernel<true, false> : vel ? orient_pass_kernel<true, true> : orient_pass_kernel<false, true>;
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, st, x4, y4, z4, w4, vx4, vy4, vz4, dboxes.as<float>(), nblocks,
                           center[0], center[1], center[2], s * s, o[0], o[1], o[2], partials);
        TSP_HIP(hipGetLastError());
        if (stats) TSP_HIP(hipEventRecord(ctx->ev[EV_T1], st));
        hipLaunchKernelGGL(orient_final_kernel, dim3(1), dim3(256), 0, st, partials, grid);
        TSP_HIP(hipGetLastError());
        TSP_HIP(hipMemcpyAsync(&sum, partials + grid, sizeof(sum), hipMemcpyDeviceToHost, st));
        TSP_HIP(hipStreamSynchronize(st));
        if (stats) TSP_HIP(hipEventElapsedTime(&pass_ms[which], ctx->ev[EV_T0], ctx->ev[EV_T1]));
        pass_blocks[which] = sum.blocks;
        return TSP_OK;
    };

    tsp_moments mo = {};
    mo.n_valid = (int64_t)n_valid;
    int rc;
    if (vel) {
        const double zero[3] = {0.0, 0.0, 0.0};
        if ((rc = run_pass(0, r_vel, zero)) != TSP_OK) return rc;
        TSP_REQUIRE(sum.count > 0, TSP_EINVAL, "tsp_sphere_moments: the r_vel sphere (radius %g) holds no valid particle", r_vel);
        mo.n_inside_vel = sum.count;
        mo.mass_vel = sum.s[S_MASS];
        for (int c = 0; c < 3; ++c) mo.v_cen[c] = sum.s[S_MD + c] / sum.s[S_MASS];
    }
    if ((rc = run_pass(1, r, mo.v_cen)) != TSP_OK) return rc;
    TSP_REQUIRE(sum.count > 0, TSP_EINVAL, "tsp_sphere_moments: the r sphere (radius %g) holds no valid particle", r);
    mo.n_inside = sum.count;
    mo.mass = sum.s[S_MASS];
    for (int c = 0; c < 3; ++c) {
        mo.com[c] = sum.s[S_MD + c] / sum.s[S_MASS];
        mo.L[c] = sum.s[S_L + c];
    }
    for (int c = 0; c < 6; ++c) mo.S[c] = sum.s[S_S + c];
    mo.A = sum.s[S_A];
    if (stats) {
        fprintf(stderr, "tsp_sphere_moments: n=%lld valid=%lld blocks=%lld workgroups=%d upload_ms=%.3f prepare_ms=%.3f\n",
                (long long)n, (long long)mo.n_valid, (long long)nblocks, grid, ms_upload, ms_prepare);
        if (vel)
            fprintf(stderr, "tsp_sphere_moments: pass=A kernel_ms=%.4f blocks_read=%lld inside=%lld\n", pass_ms[0], pass_blocks[0],
                    (long long)mo.n_inside_vel);
        fprintf(stderr, "tsp_sphere_moments: pass=B kernel_ms=%.4f blocks_read=%lld inside=%lld\n", pass_ms[1], pass_blocks[1],
                (long long)mo.n_inside);
    }
    *out = mo;
    return TSP_OK;
}

}  // namespace tsp
