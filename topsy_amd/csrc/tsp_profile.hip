// tsp_profile.hip -- radial profiles (tsp_radial_profile): per radial bin -- spherical shells, or cylindrical annuli about the third
// axis of a frame -- the count, the mass, the mass-weighted radius, the first and second moments of the velocity components along
// the bin's own triad, and the angular momentum: what pynbody.analysis.profile.Profile and halo.virial_radius are built from.
//
// Contract (include/topsy_splat.h), float64 throughout, nothing fused, every sum starting at +0.0:
//   - valid particles and displacements as tsp_sphere_moments; d' = frame * d, u' = frame * (v - v_cen), rows as (f0 a + f1 b) + f2 c;
//   - s2 = (dx * dx + dy * dy) + dz * dz (geometry 0) or x' * x' + y' * y' with |z'| <= half_height (geometry 1);
//   - E2[k] = edges[k] * edges[k]; bin k iff E2[k] <= s2 < E2[k + 1]; s2 < E2[0]: n_inner / mass_inner; s2 >= E2[n_bins]: nowhere;
//   - per bin 11 sums: mass, m s | m c_j | (m c_j) c_j | m (d x u), c the velocity along the cylindrical or spherical triad.
//
// The passes, in the shape of tsp_orient.hip (tsp_blocks.h holds what is shared):
//   1. profile_prepare_kernel: w[i] = valid ? mass[i] : 0, the valid count, the float32 bounding box of every block of CBLK
//      consecutive particles.
//   2. profile_pass_kernel<VEL, GEOM>: a workgroup takes blocks blockIdx.x, blockIdx.x + gridDim.x, ...; a block whose box lies at
//      a squared distance >= skip_r2 from the centre is skipped unread (box_outside_sphere; skip_r2 bounds every member, so the
//      skip never changes a sum).  Every other block is read as one float4 per lane and array.  For each of a lane's four
//      particles in turn the lane finds its row of the table (0: inside edges[0]; k + 1: bin k) by binary search in the squared
//      edges, which sit in LDS, and forms its eleven terms.  The binned reduction, bit-reproducible:
//        - a wave loops over the distinct rows among its lanes, lowest unserved lane first: the row of that lane is broadcast, a
//          ballot finds the lanes that share it, an xor butterfly sums each term over the wave with +0.0 from the other lanes, and
//          lane 0 adds the eleven sums and the ballot's population count to a table in LDS;
//        - up to 103 bins every wave has a table of its own (four fit 40 KB) and never waits; the workgroup's partial is the four
//          tables added in wave order.  Above, the workgroup has one table and the four waves take turns in wave order, a barrier
//          after each turn: nothing else writes the table between two barriers.
//      Either way the order of every addition is fixed.  The workgroup stores one partial.
//   3. profile_final_kernel: one thread per table entry adds the partials in index order.
// No floating-point atomic takes part (the valid count and blocks_read are integer atomics); the grid is a function of n, n_bins
// and the device alone: the same call returns the same bits.
//
// Cost: a spatially ordered snapshot shows a wave a handful of distinct rows per particle slot; a shuffled one up to 64 rounds of
// 66 (without velocities 12) 64-bit shuffles: slow, not wrong.
// LDS, dynamic: (n_bins + 1) * (8 + 4 * 96) bytes up to 103 bins (39.6 KB at 100: four workgroups per CU of 160 KB), above
// (n_bins + 1) * (8 + 96): 10.9 KB at 104 bins, 53.4 KB at 512 (three workgroups per CU; the grid asks for two).
// Registers, as built (the resource report of hipcc --offload-arch=gfx950): the pass takes 100 VGPRs in shells with velocities (four
// waves per SIMD), 90 in annuli (five), 43 without velocities (eight); the preparation 56 / 48, the final kernel 8; no kernel of
// this file spills or uses scratch.  Measured times: DESIGN.md section 4.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "tsp_blocks.h"
#include "tsp_internal.h"

namespace tsp {
namespace {

constexpr int NSUM = 11;        // mass | m s | m c (3) | (m c) c (3) | m d x u (3)
constexpr int ROW = NSUM + 1;   // doubles per table row: the sums, then the count as a 64-bit integer
enum { P_MASS = 0, P_MS = 1, P_MC = 2, P_MC2 = 5, P_MJ = 8, P_COUNT = 11 };

struct PassParams {
    double c[3], o[3], f[9];    // centre, velocity centre, frame (row-major)
    double half_height;
    double skip_r2;             // a block at a squared box distance >= this holds no member
    int n_bins;
    int n_tables;               // 4: a table per wave; 1: one table, the waves take turns
};

__device__ __forceinline__ void unpack(const float4 &v, float out[4]) {
    out[0] = v.x;
    out[1] = v.y;
    out[2] = v.z;
    out[3] = v.w;
}

// 1. validity into w, the valid count, the block boxes.  The arrays are padded to whole blocks with zeros (a zero mass is
// invalid).
template <bool VEL>
__global__ __launch_bounds__(256) void profile_prepare_kernel(const float4 *__restrict__ x4, const float4 *__restrict__ y4,
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

// the table row of a squared bin coordinate: the number of squared edges <= s2 (0: inside edges[0]; k + 1: bin k;
// n_bins + 1: outside the last edge)
__device__ __forceinline__ int row_of(const double *__restrict__ E2, int n_edges, double s2) {
    int lo = 0, len = n_edges;
    while (len > 0) {
        const int half = len >> 1;
        if (E2[lo + half] <= s2) {
            lo += half + 1;
            len -= half + 1;
        } else {
            len = half;
        }
    }
    return lo;
}

// a particle's row (-1: no member) and its terms, in the expression order of the header
template <bool VEL, int GEOM>
__device__ __forceinline__ int particle_terms(const PassParams &p, const double *__restrict__ E2, float x, float y, float z, float w,
                                              float vx, float vy, float vz, double t[NSUM]) {
    if (!(w > 0.0f)) return -1;
    const double dx = (double)x - p.c[0], dy = (double)y - p.c[1], dz = (double)z - p.c[2];
    const double xp = (p.f[0] * dx + p.f[1] * dy) + p.f[2] * dz;
    const double yp = (p.f[3] * dx + p.f[4] * dy) + p.f[5] * dz;
    const double zp = (p.f[6] * dx + p.f[7] * dy) + p.f[8] * dz;
    const double R2 = xp * xp + yp * yp;
    double s2;
    if (GEOM == 0) {
        s2 = (dx * dx + dy * dy) + dz * dz;
    } else {
        s2 = R2;
        if (!(fabs(zp) <= p.half_height)) return -1;
    }
    const int row = row_of(E2, p.n_bins + 1, s2);
    if (row > p.n_bins) return -1;
    const double m = (double)w;
    t[P_MASS] = m;
    t[P_MS] = m * sqrt(s2);
    if (VEL) {
        const double ux = (double)vx - p.o[0], uy = (double)vy - p.o[1], uz = (double)vz - p.o[2];
        const double upx = (p.f[0] * ux + p.f[1] * uy) + p.f[2] * uz;
        const double upy = (p.f[3] * ux + p.f[4] * uy) + p.f[5] * uz;
        const double upz = (p.f[6] * ux + p.f[7] * uy) + p.f[8] * uz;
        const double R = sqrt(R2);
        const bool offaxis = R > 0.0;
        const double eRx = offaxis ? xp / R : 1.0, eRy = offaxis ? yp / R : 0.0;
        double c0, c1, c2;
        c1 = eRx * upy - eRy * upx;                               // u_phi
        if (GEOM == 0) {
            const double D = sqrt(R2 + zp * zp);
            const bool offcentre = D > 0.0;
            const double erx = offcentre ? xp / D : 0.0, ery = offcentre ? yp / D : 0.0, erz = offcentre ? zp / D : 1.0;
            c0 = (erx * upx + ery * upy) + erz * upz;             // u_r
            c2 = ((eRx * erz) * upx + (eRy * erz) * upy) - (eRx * erx + eRy * ery) * upz;     // u_theta
        } else {
            c0 = eRx * upx + eRy * upy;                           // u_R
            c2 = upz;                                             // u_z
        }
        const double mc0 = m * c0, mc1 = m * c1, mc2 = m * c2;
        t[P_MC + 0] = mc0;
        t[P_MC + 1] = mc1;
        t[P_MC + 2] = mc2;
        t[P_MC2 + 0] = mc0 * c0;
        t[P_MC2 + 1] = mc1 * c1;
        t[P_MC2 + 2] = mc2 * c2;
        t[P_MJ + 0] = m * (dy * uz - dz * uy);
        t[P_MJ + 1] = m * (dz * ux - dx * uz);
        t[P_MJ + 2] = m * (dx * uy - dy * ux);
    }
    return row;
}

// 2. the table of one workgroup over its blocks: partials[blockIdx.x][row][ROW]
template <bool VEL, int GEOM>
__global__ __launch_bounds__(256) void profile_pass_kernel(const float4 *__restrict__ x4, const float4 *__restrict__ y4,
                                                           const float4 *__restrict__ z4, const float4 *__restrict__ w4,
                                                           const float4 *__restrict__ vx4, const float4 *__restrict__ vy4,
                                                           const float4 *__restrict__ vz4, const float *__restrict__ boxes,
                                                           int64_t nblocks, const PassParams p, const double *__restrict__ E2_global,
                                                           double *__restrict__ partials, unsigned long long *__restrict__ blocks_read) {
    extern __shared__ double lds[];
    constexpr int NV = VEL ? NSUM : 2;          // the terms that are summed: without velocities the other nine stay +0.0
    const int n_rows = p.n_bins + 1;
    double *E2 = lds;                           // n_bins + 1 squared edges
    double *table = lds + n_rows;               // n_tables tables of n_rows rows of ROW
    const int n_tables = p.n_tables, n_turns = n_tables == 1 ? 4 : 1;
    for (int i = threadIdx.x; i < n_rows; i += 256) E2[i] = E2_global[i];
    for (int i = threadIdx.x; i < n_tables * n_rows * ROW; i += 256) table[i] = 0.0;       // (+0.0 is the integer 0 too)
    __syncthreads();

    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    double *my_table = table + (n_tables == 1 ? 0 : wave) * n_rows * ROW;      // the table this wave adds to
    unsigned nread = 0;
    for (int64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
        if (box_outside_sphere(boxes + 6 * b, p.c[0], p.c[1], p.c[2], p.skip_r2)) continue;      // (uniform over the workgroup)
        ++nread;
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
            double t[NSUM];
#pragma unroll
            for (int j = 0; j < NSUM; ++j) t[j] = 0.0;
            const int row = particle_terms<VEL, GEOM>(p, E2, px[k], py[k], pz[k], pw[k], pu[k], pv[k], pq[k], t);
            for (int turn = 0; turn < n_turns; ++turn) {
                if (n_tables != 1 || wave == turn) {
                    unsigned long long todo = __ballot(row >= 0);
                    while (todo) {
                        const int leader = __ffsll(todo) - 1;
                        const int cur = __shfl(row, leader);
                        const bool mine = row == cur;
                        const unsigned long long members = __ballot(mine);
                        double v[NV];
#pragma unroll
                        for (int j = 0; j < NV; ++j) v[j] = mine ? t[j] : 0.0;
                        for (int off = 32; off; off >>= 1) {
#pragma unroll
                            for (int j = 0; j < NV; ++j) v[j] += __shfl_xor(v[j], off);
                        }
                        if (lane == 0) {
                            double *r = my_table + cur * ROW;
#pragma unroll
                            for (int j = 0; j < NV; ++j) r[j] += v[j];
                            long long *count = reinterpret_cast<long long *>(r + P_COUNT);
                            *count += __popcll(members);
                        }
                        todo &= ~members;
                    }
                }
                if (n_tables == 1) __syncthreads();
            }
        }
    }
    __syncthreads();
    // the workgroup's partial: its table, or its waves' tables added in wave order
    double *out = partials + (size_t)blockIdx.x * n_rows * ROW;
    for (int i = threadIdx.x; i < n_rows * ROW; i += 256) {
        if (n_tables == 1) {
            out[i] = table[i];
        } else if (i % ROW == P_COUNT) {
            const long long *c = reinterpret_cast<const long long *>(table) + i;
            reinterpret_cast<long long *>(out)[i] = ((c[0] + c[n_rows * ROW]) + c[2 * n_rows * ROW]) + c[3 * n_rows * ROW];
        } else {
            const double *t = table + i;
            out[i] = ((t[0] + t[n_rows * ROW]) + t[2 * n_rows * ROW]) + t[3 * n_rows * ROW];
        }
    }
    if (threadIdx.x == 0 && nread) atomicAdd(blocks_read, (unsigned long long)nread);
}

// 3. every table entry over the partials in index order, into result[n_entries]
__global__ __launch_bounds__(256) void profile_final_kernel(const double *__restrict__ partials, int n_partials, int n_entries,
                                                            double *__restrict__ result) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_entries) return;
    if (i % ROW == P_COUNT) {
        long long a = 0;
        for (int q = 0; q < n_partials; ++q) a += reinterpret_cast<const long long *>(partials)[(size_t)q * n_entries + i];
        reinterpret_cast<long long *>(result)[i] = a;
    } else {
        double a = 0.0;
        for (int q = 0; q < n_partials; ++q) a += partials[(size_t)q * n_entries + i];
        result[i] = a;
    }
}

}  // namespace

// the workgroups of a pass: a function of the block count, n_bins and the device (up to four per CU; two where the tables are
// large, which also bounds the partials to 256 CUs * 2 * 53 KB), and two blocks each at least, so that every snapshot of more than
// one block takes the stride loop
static int profile_grid(int64_t nblocks, int n_bins, int cu_count) {
    const int per_cu = n_bins <= 128 ? 4 : 2;
    return (int)std::min<int64_t>((nblocks + 1) / 2, (int64_t)cu_count * per_cu);
}

// the tables of a workgroup: one per wave where four fit WAVE_TABLE_BYTES of LDS with the squared edges (up to 103 bins: four
// workgroups per CU stay resident), so that no wave waits for another; else one, which the waves add to in turn
#ifndef TSP_PROFILE_WAVE_TABLE_BYTES
#define TSP_PROFILE_WAVE_TABLE_BYTES 40960
#endif
static int profile_tables(int n_bins) {
    return (size_t)(n_bins + 1) * (1 + 4 * ROW) * sizeof(double) <= (size_t)TSP_PROFILE_WAVE_TABLE_BYTES ? 4 : 1;
}

static size_t profile_partial_bytes(int grid, int n_bins) {
    return (size_t)grid * (size_t)(n_bins + 1) * ROW * sizeof(double);
}

int radial_profile(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, const float *mass, const float *vx,
                   const float *vy, const float *vz, const tsp_profile_spec *spec, int64_t *count_out, double *sums_out,
                   tsp_profile_info *info_out) {
    hipStream_t st = ctx->stream;
    // measurement aid: TOPSY_PROFILE_STATS=1 reports the time of the upload, the preparation and the pass, and the blocks it read
    const char *env = getenv("TOPSY_PROFILE_STATS");
    const bool stats = env && env[0] == '1';
    const bool vel = vx != nullptr;
    const int n_arrays = vel ? 7 : 4;
    const int n_bins = spec->n_bins, n_rows = n_bins + 1, n_entries = n_rows * ROW;
    const int64_t nblocks = (n + CBLK - 1) / CBLK, npad = nblocks * CBLK;
    const size_t fbytes = (size_t)n * sizeof(float), pad_bytes = (size_t)(npad - n) * sizeof(float);
    const int grid = profile_grid(nblocks, n_bins, ctx->cu_count);
    const int prepare_grid = (int)std::min<int64_t>((nblocks + 1) / 2, (int64_t)ctx->cu_count * 8);
    const int n_tables = profile_tables(n_bins);
    const size_t lds_bytes = (size_t)n_rows * (1 + n_tables * ROW) * sizeof(double);

    PassParams p;
    std::vector<double> E2(n_rows);
    for (int k = 0; k < n_rows; ++k) E2[k] = spec->edges[k] * spec->edges[k];
    for (int c = 0; c < 3; ++c) {
        p.c[c] = spec->center[c];
        p.o[c] = vel ? spec->v_cen[c] : 0.0;
    }
    for (int c = 0; c < 9; ++c) p.f[c] = spec->frame[c];
    p.n_bins = n_bins;
    p.n_tables = n_tables;
    p.half_height = spec->geometry == 1 ? spec->half_height : 0.0;
    // no member beyond it: geometry 0 bins d2 itself; geometry 1 has x'^2 + y'^2 < E2[n_bins] and z'^2 <= half_height^2, and d2
    // equals |d'|^2 up to the frame's orthonormality (1e-6, checked by the caller) and rounding: the factor 1 + 1e-5 covers both
    p.skip_r2 = spec->geometry == 0 ? E2[n_bins] : (E2[n_bins] + spec->half_height * spec->half_height) * (1.0 + 1e-5);

    const float *host[7] = {x, y, z, mass, vx, vy, vz};
    static const char *const dev_site[7] = {SITE("profile_x"),  SITE("profile_y"),  SITE("profile_z"), SITE("profile_mass"),
                                            SITE("profile_vx"), SITE("profile_vy"), SITE("profile_vz")};
    DeviceScratch dev[7], dboxes, dpartials, dresult, dedges, dcount;
    for (int a = 0; a < n_arrays; ++a) TSP_SCRATCH_ALLOC(ctx, dev_site[a], dev[a], (size_t)npad * sizeof(float));
    TSP_SCRATCH_ALLOC(ctx, SITE("profile_boxes"), dboxes, (size_t)nblocks * 6 * sizeof(float));
    TSP_SCRATCH_ALLOC(ctx, SITE("profile_partials"), dpartials, profile_partial_bytes(grid, n_bins));
    TSP_SCRATCH_ALLOC(ctx, SITE("profile_result"), dresult, (size_t)n_entries * sizeof(double));
    TSP_SCRATCH_ALLOC(ctx, SITE("profile_edges"), dedges, (size_t)n_rows * sizeof(double));
    TSP_SCRATCH_ALLOC(ctx, SITE("profile_counters"), dcount, 2 * sizeof(unsigned long long));

    auto t0 = std::chrono::steady_clock::now();
    for (int a = 0; a < n_arrays; ++a) {
        if (pad_bytes) TSP_HIP(hipMemsetAsync(dev[a].as<float>() + n, 0, pad_bytes, st));
        TSP_HIP(hipMemcpyAsync(dev[a].p, host[a], fbytes, hipMemcpyHostToDevice, st));
    }
    TSP_HIP(hipMemcpyAsync(dedges.p, E2.data(), (size_t)n_rows * sizeof(double), hipMemcpyHostToDevice, st));
    TSP_HIP(hipMemsetAsync(dcount.p, 0, 2 * sizeof(unsigned long long), st));
    TSP_HIP(hipStreamSynchronize(st));          // (E2 is pageable host memory: it must not be read after this function's return)
    const double ms_upload = wall_ms(t0);

    const float4 *x4 = dev[0].as<float4>(), *y4 = dev[1].as<float4>(), *z4 = dev[2].as<float4>(), *w4 = dev[3].as<float4>();
    const float4 *vx4 = dev[4].as<float4>(), *vy4 = dev[5].as<float4>(), *vz4 = dev[6].as<float4>();     // null without velocities
    unsigned long long *counters = dcount.as<unsigned long long>();      // [0] the valid count, [1] the blocks read
    t0 = std::chrono::steady_clock::now();
    hipLaunchKernelGGL(vel ? profile_prepare_kernel<true> : profile_prepare_kernel<false>, dim3(prepare_grid), dim3(256), 0, st, x4,
                       y4, z4, dev[3].as<float4>(), vx4, vy4, vz4, nblocks, dboxes.as<float>(), counters);
    TSP_HIP(hipGetLastError());
    unsigned long long n_valid = 0;
    TSP_HIP(hipMemcpyAsync(&n_valid, counters, sizeof(n_valid), hipMemcpyDeviceToHost, st));
    TSP_HIP(hipStreamSynchronize(st));
    const double ms_prepare = wall_ms(t0);
    TSP_REQUIRE(n_valid > 0, TSP_EINVAL, "tsp_radial_profile: no particle has finite coordinates%s and a finite mass > 0",
                vel ? " and velocities" : "");

    auto kernel = spec->geometry == 0 ? (vel ? profile_pass_kernel<true, 0> : profile_pass_kernel<false, 0>)
                                      : (vel ? profile_pass_kernel<true, 1> : profile_pass_kernel<false, 1>);
    if (stats) TSP_HIP(hipEventRecord(ctx->ev[EV_T0], st));
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds_bytes, st, x4, y4, z4, w4, vx4, vy4, vz4, dboxes.as<float>(), nblocks, p,
                       dedges.as<double>(), dpartials.as<double>(), counters + 1);
    TSP_HIP(hipGetLastError());
    if (stats) TSP_HIP(hipEventRecord(ctx->ev[EV_T1], st));
    hipLaunchKernelGGL(profile_final_kernel, dim3((n_entries + 255) / 256), dim3(256), 0, st, dpartials.as<double>(), grid, n_entries,
                       dresult.as<double>());
    TSP_HIP(hipGetLastError());
    std::vector<double> result(n_entries);
    unsigned long long blocks_read = 0;
    TSP_HIP(hipMemcpyAsync(result.data(), dresult.p, (size_t)n_entries * sizeof(double), hipMemcpyDeviceToHost, st));
    TSP_HIP(hipMemcpyAsync(&blocks_read, counters + 1, sizeof(blocks_read), hipMemcpyDeviceToHost, st));
    TSP_HIP(hipStreamSynchronize(st));
    float kernel_ms = 0.0f;
    if (stats) TSP_HIP(hipEventElapsedTime(&kernel_ms, ctx->ev[EV_T0], ctx->ev[EV_T1]));

    auto count_of = [&](int row) {
        long long c;
        memcpy(&c, &result[(size_t)row * ROW + P_COUNT], sizeof(c));
        return c;
    };
    tsp_profile_info info = {};
    info.n_valid = (int64_t)n_valid;
    info.n_inner = count_of(0);
    info.mass_inner = result[P_MASS];
    for (int k = 0; k < n_bins; ++k) {
        count_out[k] = count_of(k + 1);
        info.n_binned += count_out[k];
        memcpy(sums_out + (size_t)k * NSUM, &result[(size_t)(k + 1) * ROW], NSUM * sizeof(double));
    }
    if (info_out) *info_out = info;
    if (stats) {
        fprintf(stderr, "tsp_radial_profile: n=%lld valid=%lld blocks=%lld workgroups=%d tables=%d upload_ms=%.3f prepare_ms=%.3f\n",
                (long long)n, (long long)info.n_valid, (long long)nblocks, grid, n_tables, ms_upload, ms_prepare);
        fprintf(stderr, "tsp_radial_profile: geometry=%d bins=%d kernel_ms=%.4f blocks_read=%lld binned=%lld inner=%lld\n",
                spec->geometry, n_bins, kernel_ms, (long long)blocks_read, (long long)info.n_binned, (long long)info.n_inner);
    }
    return TSP_OK;
}

}  // namespace tsp
