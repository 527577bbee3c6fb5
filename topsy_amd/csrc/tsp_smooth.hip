// tsp_smooth.hip -- SPH smoothing lengths by k nearest neighbours (tsp_smoothing_lengths): what the reference asks of
// pynbody.sph.smooth when a snapshot carries no smoothing lengths (src/topsy/loader.py:222-240).
//
// Contract (include/topsy_splat.h): for every particle i with finite coordinates, h[i] = 0.5 * sqrt(the k-th smallest
// d2 = (dx*dx + dy*dy) + dz*dz over every particle j with finite coordinates, j = i included), in float32 with the operation
// order written out in dist2() (tsp_morton.h); a periodic box first maps each dx to its nearest image, dx - L * rint(dx / L).
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
//
// tsp_sph_sum, the gather-form SPH sum (with a = mass: the density pynbody derives as 'rho'), is a range query of radius 2 h[i]
// over the same index (step 1 is shared: build_morton_index); its kernel is described at sph_sum_kernel below.
// tsp_sph_velocity_gradient, the divergence and curl of the velocity (pynbody's 'v_div' and 'v_curl'), is the same range query
// with four sums per query (sph_velocity_gradient_kernel); one host routine, sph_sum(), serves both calls.
// tsp_sph_sample_lattice evaluates the sums at the points of a lattice, which are no particles: a k-NN search for h at the point
// (lattice_knn_kernel), then the range query with up to four sums (lattice_sum_kernel); its host routine is sph_sample_lattice().
#include <hipcub/hipcub.hpp>

#include <math.h>
#include <stdlib.h>

#include <chrono>

#include "tsp_morton.h"

namespace tsp {
namespace {

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
        const QueryCells qc = query_cells(g, qx, qy, qz, R);
        list_init(list, k);
        for (int combo = 0; combo < 8; ++combo) {
            int c[3];
            if (!combo_cell(qc, combo, c)) continue;
            const float bound = fminf(r0, list[KP - 1]) * CULL_SLACK;
            const float gx = axis_gap(g, 0, qc.q[0], c[0], qc.s);
            const float gy = axis_gap(g, 1, qc.q[1], c[1], qc.s);
            const float gz = axis_gap(g, 2, qc.q[2], c[2], qc.s);
            if ((gx * gx + gy * gy) + gz * gz > bound) continue;
            int64_t b, e;
            cell_run(keys, nv, c, qc.s, b, e);
            for (int64_t j = b; j < e; ++j) list_insert(list, dist2(qx, qy, qz, sx[j], sy[j], sz[j], L));
            evaluated += (unsigned long long)(e - b);
        }
        h_sorted[i] = 0.5f * sqrtf(list[KP - 1]);     // correctly rounded here (__fsqrt_rn compiles to the 1-ulp v_sqrt_f32)
    }
    for (int off = 32; off; off >>= 1) evaluated += __shfl_xor(evaluated, off);
    if ((threadIdx.x & 63) == 0 && evaluated) atomicAdd(n_dist, evaluated);
}

// ---- tsp_sph_sum: the gather-form SPH sum over the same index -------------------------------------------------------------
// gather of the per-particle h and a into Morton order
__global__ __launch_bounds__(256) void sph_gather_kernel(const float *__restrict__ h, const float *__restrict__ a,
                                                         const uint32_t *__restrict__ idx, int64_t nv, float *__restrict__ sh,
                                                         float *__restrict__ sa) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t j = idx[i];
        sh[i] = h[j];
        sa[i] = a[j];
    }
}

// The contract's term for a candidate at squared distance d2: float32, these operations in this order; 0 terms when u >= 2.
__device__ __forceinline__ void sph_term(float d2, float aj, float hq, double &S, unsigned &terms) {
    const float u = __fdiv_rn(sqrtf(d2), hq);
    if (u < 2.0f) {
        const float u2 = u * u;
        const float t = 2.0f - u;
        const float w = u < 1.0f ? (1.0f - 1.5f * u2) + 0.75f * (u2 * u) : 0.25f * ((t * t) * t);
        S += (double)(aj * w);
        ++terms;
    }
}

// A range query of radius 2 h[i] over the octree of key prefixes (the level choice, the runs and the conservative box test of
// smooth_knn_kernel), every candidate of the surviving runs tested with the contract's own u < 2.
// Step A, one lane per query in Morton order: the (at most eight) runs of the query, into LDS.
// Step B, one wave per query: the wave takes the queries of its lanes in turn and scans each one's runs 64 candidates at a time
// (coalesced loads, every lane busy but in a run's last step); a lane sums its own candidates in a double, the 64 partial sums are
// added by a butterfly, whose order is fixed, so the same call returns the same bits (no atomics take part in the sum).
// With one lane per query a wave scanned as long as its longest run at each cell: measured on clustered positions, 21 % of its
// lanes' steps had a candidate, and every lane streamed cache lines of its own.
__global__ __launch_bounds__(256) void sph_sum_kernel(const float *__restrict__ sx, const float *__restrict__ sy,
                                                      const float *__restrict__ sz, const float *__restrict__ sh,
                                                      const float *__restrict__ sa, const uint64_t *__restrict__ keys,
                                                      int64_t nv, Grid g, float *__restrict__ out_sorted,
                                                      unsigned long long *counters) {
    __shared__ uint32_t run_b[256][8], run_e[256][8];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63, wave0 = threadIdx.x & ~63;
    const float L = g.period;
    unsigned long long scanned = 0, steps = 0;
    unsigned terms = 0;
    float hq = 0.0f, qx = 0.0f, qy = 0.0f, qz = 0.0f, reach2 = 0.0f;
    bool answerable = false;
    for (int r = 0; r < 8; ++r) run_b[threadIdx.x][r] = run_e[threadIdx.x][r] = 0;
    if (i < nv) {
        hq = sh[i];
        answerable = __builtin_isfinite(hq) && hq > 0.0f;
    }
    if (answerable) {
        qx = sx[i], qy = sy[i], qz = sz[i];
        // every term has sqrtf(d2) / hq < 2, so d2 <= reach2 (the slack covers the two roundings; an overflowing reach2
        // is +inf and rejects nothing, one too small to be formed reliably is not used)
        const float reach = (2.0f * hq) * CULL_SLACK;
        const float R = reach + g.eps;
        reach2 = reach * reach >= 1e-30f ? reach * reach : __builtin_inff();
        const double cull2 = ((double)reach * (double)reach) * (double)CULL_SLACK;
        scanned = for_each_run(g, keys, nv, qx, qy, qz, R, cull2, [&](int combo, int64_t b, int64_t e) {
            run_b[threadIdx.x][combo] = (uint32_t)b;      // (nv < 2^31)
            run_e[threadIdx.x][combo] = (uint32_t)e;
        });
    }
    __syncthreads();

    double S = 0.0;
    const unsigned long long todo = __ballot(answerable);
    for (int l = 0; l < 64; ++l) {
        if (!((todo >> l) & 1)) continue;                   // (uniform over the wave)
        const float lx = __shfl(qx, l), ly = __shfl(qy, l), lz = __shfl(qz, l), lh = __shfl(hq, l), lreach2 = __shfl(reach2, l);
        double part = 0.0;
        for (int r = 0; r < 8; ++r) {
            const int64_t b = run_b[wave0 + l][r], e = run_e[wave0 + l][r];
            for (int64_t j = b + lane; j < e; j += 64) {
                const float d2 = dist2(lx, ly, lz, sx[j], sy[j], sz[j], L);
                if (d2 <= lreach2) sph_term(d2, sa[j], lh, part, terms);
            }
            steps += (unsigned long long)((e - b + 63) >> 6);
        }
        for (int off = 32; off; off >>= 1) part += __shfl_xor(part, off);
        if (lane == l) S = part;
    }
    if (i < nv) out_sorted[i] = answerable ? (float)(S / (M_PI * (double)((hq * hq) * hq))) : __builtin_nanf("");

    unsigned long long nterms = terms;
    for (int off = 32; off; off >>= 1) {
        scanned += __shfl_xor(scanned, off);
        nterms += __shfl_xor(nterms, off);
    }
    if (lane == 0 && scanned) {
        atomicAdd(&counters[0], scanned);
        atomicAdd(&counters[1], nterms);
        atomicAdd(&counters[2], steps);
    }
}

// ---- tsp_sph_velocity_gradient: divergence and curl of the velocity by the same gather ------------------------------------------
// gather of the per-query h and rho and of the per-candidate payload (mass, vx, vy, vz: one 16-byte load) into Morton order
__global__ __launch_bounds__(256) void sph_gather_velocity_kernel(const float *__restrict__ h, const float *__restrict__ mass,
                                                                  const float *__restrict__ rho, const float *__restrict__ vx,
                                                                  const float *__restrict__ vy, const float *__restrict__ vz,
                                                                  const uint32_t *__restrict__ idx, int64_t nv,
                                                                  float *__restrict__ sh, float *__restrict__ srho,
                                                                  float4 *__restrict__ smv) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t j = idx[i];
        sh[i] = h[j];
        srho[i] = rho[j];
        smv[i] = make_float4(mass[j], vx[j], vy[j], vz[j]);
    }
}

// The contract's four terms for a candidate at displacement (dx, dy, dz), squared distance d2: float32, these operations in this
// order; no term when d2 == 0 (the particle itself, an exact duplicate) or u >= 2.  mv = (mass, vx, vy, vz) of the candidate.
__device__ __forceinline__ void velocity_gradient_term(float dx, float dy, float dz, float d2, float4 mv, float hq, float qvx,
                                                       float qvy, float qvz, double (&S)[4], unsigned &terms) {
    const float u = __fdiv_rn(sqrtf(d2), hq);
    if (d2 > 0.0f && u < 2.0f) {
        const float t = 2.0f - u;
        const float f = u < 1.0f ? 3.0f - 2.25f * u : __fdiv_rn(0.75f * (t * t), u);
        const float c = mv.x * f;
        const float dvx = mv.y - qvx, dvy = mv.z - qvy, dvz = mv.w - qvz;
        S[0] += (double)(c * ((dvx * dx + dvy * dy) + dvz * dz));
        S[1] += (double)(c * (dy * dvz - dz * dvy));
        S[2] += (double)(c * (dz * dvx - dx * dvz));
        S[3] += (double)(c * (dx * dvy - dy * dvx));
        ++terms;
    }
}

// The range query of sph_sum_kernel (step A: a lane per query finds its runs, into LDS; step B: a wave per query scans them 64
// candidates at a time) with four float64 partial sums per lane, each added over the wave by the same fixed butterfly.  A candidate
// is three position loads and one 16-byte load; the query's own velocity is its own payload entry.
// Block size 256 as there: the two run tables are 16 KiB of LDS, of which ten blocks fit in a CU's 160 KiB, more than the eight
// blocks of four waves that its 32 wave slots take -- LDS does not limit the occupancy.  Registers do: the four double partials,
// the wider candidate and the query's velocity bring the kernel to 80 VGPRs, six waves per SIMD (sph_sum_kernel: 57, eight), with
// no spill.  A block of 128 would halve the tables and change neither figure.
__global__ __launch_bounds__(256) void sph_velocity_gradient_kernel(const float *__restrict__ sx, const float *__restrict__ sy,
                                                                    const float *__restrict__ sz, const float *__restrict__ sh,
                                                                    const float *__restrict__ srho, const float4 *__restrict__ smv,
                                                                    const uint64_t *__restrict__ keys, int64_t nv, Grid g,
                                                                    float *__restrict__ div_sorted, float *__restrict__ cx_sorted,
                                                                    float *__restrict__ cy_sorted, float *__restrict__ cz_sorted,
                                                                    unsigned long long *counters) {
    __shared__ uint32_t run_b[256][8], run_e[256][8];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63, wave0 = threadIdx.x & ~63;
    const float L = g.period;
    unsigned long long scanned = 0, steps = 0;
    unsigned terms = 0;
    float hq = 0.0f, qx = 0.0f, qy = 0.0f, qz = 0.0f, reach2 = 0.0f, qvx = 0.0f, qvy = 0.0f, qvz = 0.0f;
    bool answerable = false;
    for (int r = 0; r < 8; ++r) run_b[threadIdx.x][r] = run_e[threadIdx.x][r] = 0;
    if (i < nv) {
        hq = sh[i];
        answerable = __builtin_isfinite(hq) && hq > 0.0f;
    }
    if (answerable) {
        qx = sx[i], qy = sy[i], qz = sz[i];
        const float4 own = smv[i];
        qvx = own.y, qvy = own.z, qvz = own.w;
        // every term has sqrtf(d2) / hq < 2, so d2 <= reach2 (see sph_sum_kernel)
        const float reach = (2.0f * hq) * CULL_SLACK;
        const float R = reach + g.eps;
        reach2 = reach * reach >= 1e-30f ? reach * reach : __builtin_inff();
        const double cull2 = ((double)reach * (double)reach) * (double)CULL_SLACK;
        scanned = for_each_run(g, keys, nv, qx, qy, qz, R, cull2, [&](int combo, int64_t b, int64_t e) {
            run_b[threadIdx.x][combo] = (uint32_t)b;      // (nv < 2^31)
            run_e[threadIdx.x][combo] = (uint32_t)e;
        });
    }
    __syncthreads();

    double S[4] = {0.0, 0.0, 0.0, 0.0};
    const unsigned long long todo = __ballot(answerable);
    for (int l = 0; l < 64; ++l) {
        if (!((todo >> l) & 1)) continue;                   // (uniform over the wave)
        const float lx = __shfl(qx, l), ly = __shfl(qy, l), lz = __shfl(qz, l), lh = __shfl(hq, l), lreach2 = __shfl(reach2, l);
        const float lvx = __shfl(qvx, l), lvy = __shfl(qvy, l), lvz = __shfl(qvz, l);
        double part[4] = {0.0, 0.0, 0.0, 0.0};
        for (int r = 0; r < 8; ++r) {
            const int64_t b = run_b[wave0 + l][r], e = run_e[wave0 + l][r];
            for (int64_t j = b + lane; j < e; j += 64) {
                float dx, dy, dz;
                const float d2 = displacement(lx, ly, lz, sx[j], sy[j], sz[j], L, dx, dy, dz);
                if (d2 <= lreach2) velocity_gradient_term(dx, dy, dz, d2, smv[j], lh, lvx, lvy, lvz, part, terms);
            }
            steps += (unsigned long long)((e - b + 63) >> 6);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            for (int off = 32; off; off >>= 1) part[c] += __shfl_xor(part[c], off);
            if (lane == l) S[c] = part[c];
        }
    }
    if (i < nv) {
        float out[4];
        const double hd = (double)hq;
        const double den = M_PI * (((hd * hd) * (hd * hd)) * hd) * (double)(answerable ? srho[i] : 0.0f);
#pragma unroll
        for (int c = 0; c < 4; ++c) out[c] = answerable ? (float)(S[c] / den) : __builtin_nanf("");
        div_sorted[i] = out[0];
        cx_sorted[i] = out[1];
        cy_sorted[i] = out[2];
        cz_sorted[i] = out[3];
    }

    unsigned long long nterms = terms;
    for (int off = 32; off; off >>= 1) {
        scanned += __shfl_xor(scanned, off);
        nterms += __shfl_xor(nterms, off);
    }
    if (lane == 0 && scanned) {
        atomicAdd(&counters[0], scanned);
        atomicAdd(&counters[1], nterms);
        atomicAdd(&counters[2], steps);
    }
}

// ---- tsp_sph_sample_lattice: the SPH sums at the points of a lattice (3-D grids, slices, rays) ---------------------------------
// The queries are the lattice points, formed on the device from the tsp_lattice argument.  A query number ("slot") maps to
// (i, j, k) by compact bricks of 64 points -- 4 x 4 x 4, 8 x 8 x 1 for a slice (nw == 1), 64 x 1 x 1 for a ray (nv == nw == 1),
// chosen by the host -- so that the 64 queries of a wave are neighbours in space and share their cells and cache lines; the slots
// of a partial brick that fall outside the lattice are masked.  h and the results are stored at the point's C-ordered [k][j][i]
// position, so the kernels un-brick as they write and every output is read back by one contiguous copy.
struct LatticeQueries {
    tsp_lattice lat;
    int bu, bv, bw;          // the brick: bu * bv * bw == 64
    int nbu, nbv;            // bricks along u and along v
    int64_t n_slots;         // 64 x the number of bricks
};

__device__ __forceinline__ bool lattice_slot(const LatticeQueries &lq, int64_t slot, int &i, int &j, int &k) {
    if (slot >= lq.n_slots) return false;
    const int64_t brick = slot >> 6, row = brick / lq.nbu;
    const int within = (int)(slot & 63);
    i = (int)(brick - row * lq.nbu) * lq.bu + within % lq.bu;
    j = (int)(row % lq.nbv) * lq.bv + (within / lq.bu) % lq.bv;
    k = (int)(row / lq.nbv) * lq.bw + within / (lq.bu * lq.bv);
    return i < lq.lat.nu && j < lq.lat.nv && k < lq.lat.nw;
}
__device__ __forceinline__ int64_t lattice_linear(const tsp_lattice &lat, int i, int j, int k) {
    return ((int64_t)k * lat.nv + j) * lat.nu + i;
}

// The k-NN search of smooth_knn_kernel for a query that is no particle: one lane per lattice point.  The window of the upper
// bound r0 lies around the place the point's own Morton key (the key smooth_key_kernel would give it) has among the sorted keys.
// A point outside the particles' bounding box (open box) takes the key of the edge cell it clamps into; any k real particles
// bound the k-th smallest distance from above, so r0 is still an upper bound.  query_cells() clamps the steps of the box
// [q - R, q + R] into the grid (monotone, so every particle inside the box lies in a cell it names) and axis_gap() measures from
// the point's real coordinate to the cell, so the cull is the true distance to the cell: read for this, both serve a query
// outside the grid unchanged.  In a periodic box grid_coord() wraps the point like a particle.
template <int KP>
__global__ __launch_bounds__(256) void lattice_knn_kernel(const float *__restrict__ sx, const float *__restrict__ sy,
                                                          const float *__restrict__ sz, const uint64_t *__restrict__ keys,
                                                          int64_t nv, int k, Grid g, LatticeQueries lq, float *__restrict__ h_lin,
                                                          unsigned long long *n_dist) {
    const int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long evaluated = 0;
    int qi, qj, qk;
    if (lattice_slot(lq, slot, qi, qj, qk)) {
        float qx, qy, qz;
        lattice_point(lq.lat, qi, qj, qk, qx, qy, qz);
        const float L = g.period;
        float list[KP];

        // 2. upper bound from the Morton-order window of 2k + 1 particles around the point's own key
        const uint64_t key = morton3((uint32_t)qclamp(qstep(grid_coord(qx, L), g.lo[0], g.inv[0])),
                                     (uint32_t)qclamp(qstep(grid_coord(qy, L), g.lo[1], g.inv[1])),
                                     (uint32_t)qclamp(qstep(grid_coord(qz, L), g.lo[2], g.inv[2])));
        const int64_t at = key_lower_bound(keys, nv, key);
        list_init(list, k);
        const int64_t W = min(nv, (int64_t)(2 * k + 1));
        const int64_t w0 = min(max(at - (int64_t)k, (int64_t)0), nv - W);
        for (int64_t j = w0; j < w0 + W; ++j) list_insert(list, dist2(qx, qy, qz, sx[j], sy[j], sz[j], L));
        const float r0 = list[KP - 1];
        evaluated += (unsigned long long)W;

        // 3. the exact search, as smooth_knn_kernel
        const float R = sqrtf(r0) * CULL_SLACK + g.eps;
        const QueryCells qc = query_cells(g, qx, qy, qz, R);
        list_init(list, k);
        for (int combo = 0; combo < 8; ++combo) {
            int c[3];
            if (!combo_cell(qc, combo, c)) continue;
            const float bound = fminf(r0, list[KP - 1]) * CULL_SLACK;
            const float gx = axis_gap(g, 0, qc.q[0], c[0], qc.s);
            const float gy = axis_gap(g, 1, qc.q[1], c[1], qc.s);
            const float gz = axis_gap(g, 2, qc.q[2], c[2], qc.s);
            if ((gx * gx + gy * gy) + gz * gz > bound) continue;
            int64_t b, e;
            cell_run(keys, nv, c, qc.s, b, e);
            for (int64_t j = b; j < e; ++j) list_insert(list, dist2(qx, qy, qz, sx[j], sy[j], sz[j], L));
            evaluated += (unsigned long long)(e - b);
        }
        h_lin[lattice_linear(lq.lat, qi, qj, qk)] = 0.5f * sqrtf(list[KP - 1]);
    }
    for (int off = 32; off; off >>= 1) evaluated += __shfl_xor(evaluated, off);
    if ((threadIdx.x & 63) == 0 && evaluated) atomicAdd(n_dist, evaluated);
}

// The candidate payload: the F fields of a particle as one 4 W-byte record in Morton order, W = 1, 2 or 4 floats (F = 3 is padded
// with a zero to W = 4), so that a candidate costs three position loads and one payload load.
template <int W>
__global__ __launch_bounds__(256) void lattice_gather_kernel(const float *__restrict__ raw, int64_t n, int n_fields,
                                                             const uint32_t *__restrict__ idx, int64_t nv,
                                                             float *__restrict__ payload) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t j = idx[i];
        float a[W];
#pragma unroll
        for (int c = 0; c < W; ++c) a[c] = c < n_fields ? raw[(size_t)c * (size_t)n + j] : 0.0f;
        if constexpr (W == 1) payload[i] = a[0];
        else if constexpr (W == 2) reinterpret_cast<float2 *>(payload)[i] = make_float2(a[0], a[1]);
        else reinterpret_cast<float4 *>(payload)[i] = make_float4(a[0], a[1], a[2], a[3]);
    }
}

// The contract's terms for a candidate at squared distance d2: the weight of sph_term(), float32, the same operations in the same
// order, times each field of the candidate's payload record.
template <int W>
__device__ __forceinline__ void lattice_term(float d2, const float *__restrict__ payload, int64_t j, float hq, double (&S)[W],
                                             unsigned &terms) {
    const float u = __fdiv_rn(sqrtf(d2), hq);
    if (u < 2.0f) {
        const float u2 = u * u;
        const float t = 2.0f - u;
        const float w = u < 1.0f ? (1.0f - 1.5f * u2) + 0.75f * (u2 * u) : 0.25f * ((t * t) * t);
        float a[W];
        if constexpr (W == 1) {
            a[0] = payload[j];
        } else if constexpr (W == 2) {
            const float2 v = reinterpret_cast<const float2 *>(payload)[j];
            a[0] = v.x, a[1] = v.y;
        } else {
            const float4 v = reinterpret_cast<const float4 *>(payload)[j];
            a[0] = v.x, a[1] = v.y, a[2] = v.z, a[3] = v.w;
        }
#pragma unroll
        for (int c = 0; c < W; ++c) S[c] += (double)(a[c] * w);
        ++terms;
    }
}

// The range query of sph_sum_kernel for the lattice points, radius 2 h(r) with the h of lattice_knn_kernel (step A: a lane per
// query finds its runs, into LDS; step B: a wave per query scans them 64 candidates at a time), with W float64 partial sums per
// lane, each added over the wave by the same fixed butterfly: no atomics in the sums, the same call returns the same bits.
// Instantiated per payload width W = 1, 2, 4, not per F: F = 3 runs the W = 4 kernel, whose fourth sum adds zeros and is not stored.
// Block size 256 as there: the two run tables are 16 KiB of LDS, ten blocks of which fit in a CU's 160 KiB, more than the eight
// blocks of four waves that its 32 wave slots take, so LDS does not limit the occupancy.  The compiler's resource report for
// gfx950 (-Rpass-analysis=kernel-resource-usage): W = 1: 57 VGPRs, eight waves per SIMD (sph_sum_kernel's figures); W = 2: 61,
// eight; W = 4: 70, seven (sph_velocity_gradient_kernel: 80, six); each 16384 bytes of LDS per block and no scratch.
// lattice_knn_kernel<8 | 16 | 32 | 64>: 50 | 63 | 89 | 153 VGPRs, 8 | 8 | 5 | 3 waves per SIMD, no LDS, no scratch.
template <int W>
__global__ __launch_bounds__(256) void lattice_sum_kernel(const float *__restrict__ sx, const float *__restrict__ sy,
                                                          const float *__restrict__ sz, const float *__restrict__ payload,
                                                          const uint64_t *__restrict__ keys, int64_t nv, Grid g, LatticeQueries lq,
                                                          const float *__restrict__ h_lin, int n_fields, int64_t nq,
                                                          float *__restrict__ out_lin, unsigned long long *counters) {
    __shared__ uint32_t run_b[256][8], run_e[256][8];
    const int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63, wave0 = threadIdx.x & ~63;
    const float L = g.period;
    unsigned long long scanned = 0, steps = 0;
    unsigned terms = 0;
    float hq = 0.0f, qx = 0.0f, qy = 0.0f, qz = 0.0f, reach2 = 0.0f;
    int qi, qj, qk;
    int64_t lin = 0;
    bool answerable = false;
    for (int r = 0; r < 8; ++r) run_b[threadIdx.x][r] = run_e[threadIdx.x][r] = 0;
    const bool inside = lattice_slot(lq, slot, qi, qj, qk);
    if (inside) {
        lin = lattice_linear(lq.lat, qi, qj, qk);
        hq = h_lin[lin];
        answerable = __builtin_isfinite(hq) && hq > 0.0f;
    }
    if (answerable) {
        lattice_point(lq.lat, qi, qj, qk, qx, qy, qz);
        // every term has sqrtf(d2) / hq < 2, so d2 <= reach2 (see sph_sum_kernel)
        const float reach = (2.0f * hq) * CULL_SLACK;
        const float R = reach + g.eps;
        reach2 = reach * reach >= 1e-30f ? reach * reach : __builtin_inff();
        const double cull2 = ((double)reach * (double)reach) * (double)CULL_SLACK;
        scanned = for_each_run(g, keys, nv, qx, qy, qz, R, cull2, [&](int combo, int64_t b, int64_t e) {
            run_b[threadIdx.x][combo] = (uint32_t)b;      // (nv < 2^31)
            run_e[threadIdx.x][combo] = (uint32_t)e;
        });
    }
    __syncthreads();

    double S[W];
#pragma unroll
    for (int c = 0; c < W; ++c) S[c] = 0.0;
    const unsigned long long todo = __ballot(answerable);
    for (int l = 0; l < 64; ++l) {
        if (!((todo >> l) & 1)) continue;                   // (uniform over the wave)
        const float lx = __shfl(qx, l), ly = __shfl(qy, l), lz = __shfl(qz, l), lh = __shfl(hq, l), lreach2 = __shfl(reach2, l);
        double part[W];
#pragma unroll
        for (int c = 0; c < W; ++c) part[c] = 0.0;
        for (int r = 0; r < 8; ++r) {
            const int64_t b = run_b[wave0 + l][r], e = run_e[wave0 + l][r];
            for (int64_t j = b + lane; j < e; j += 64) {
                const float d2 = dist2(lx, ly, lz, sx[j], sy[j], sz[j], L);
                if (d2 <= lreach2) lattice_term<W>(d2, payload, j, lh, part, terms);
            }
            steps += (unsigned long long)((e - b + 63) >> 6);
        }
#pragma unroll
        for (int c = 0; c < W; ++c) {
            for (int off = 32; off; off >>= 1) part[c] += __shfl_xor(part[c], off);
            if (lane == l) S[c] = part[c];
        }
    }
    if (inside) {
        const double den = M_PI * (double)((hq * hq) * hq);
#pragma unroll
        for (int c = 0; c < W; ++c)
            if (c < n_fields) out_lin[(size_t)c * (size_t)nq + lin] = answerable ? (float)(S[c] / den) : __builtin_nanf("");
    }

    unsigned long long nterms = terms;
    for (int off = 32; off; off >>= 1) {
        scanned += __shfl_xor(scanned, off);
        nterms += __shfl_xor(nterms, off);
    }
    if (lane == 0 && scanned) {
        atomicAdd(&counters[0], scanned);
        atomicAdd(&counters[1], nterms);
        atomicAdd(&counters[2], steps);
    }
}

}  // namespace

// Step 1 of every entry point over the index (tsp_morton.h).
// min_valid: the call is refused (TSP_EINVAL) when fewer particles have finite coordinates
int build_morton_index(tsp_context *ctx, const char *who, int64_t n, const float *x, const float *y, const float *z, float period,
                       int min_valid, MortonIndex &ix) {
    hipStream_t st = ctx->stream;
    const size_t fbytes = (size_t)n * sizeof(float);
    DeviceScratch &dx = ix.dx, &dy = ix.dy, &dz = ix.dz, &keys2 = ix.keys2, &vals = ix.vals, &vals2 = ix.vals2, &sx = ix.sx,
                  &sy = ix.sy, &sz = ix.sz, &mm = ix.mm;
    DeviceScratch keys;
    TSP_SCRATCH_ALLOC(ctx, SITE("index_x"), dx, fbytes);
    TSP_SCRATCH_ALLOC(ctx, SITE("index_y"), dy, fbytes);
    TSP_SCRATCH_ALLOC(ctx, SITE("index_z"), dz, fbytes);
    TSP_SCRATCH_ALLOC(ctx, SITE("index_bounds"), mm, 6 * sizeof(unsigned) + 4 * sizeof(unsigned long long));
    TSP_HIP(hipMemcpyAsync(dx.p, x, fbytes, hipMemcpyHostToDevice, st));
    TSP_HIP(hipMemcpyAsync(dy.p, y, fbytes, hipMemcpyHostToDevice, st));
    TSP_HIP(hipMemcpyAsync(dz.p, z, fbytes, hipMemcpyHostToDevice, st));

    // bounding box, grid, keys, sort
    unsigned *d_mm = mm.as<unsigned>();
    unsigned long long *d_count = reinterpret_cast<unsigned long long *>(d_mm + 6);
    ix.d_count = d_count;
    const unsigned init[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0, 0, 0};
    TSP_HIP(hipMemcpyAsync(d_mm, init, sizeof(init), hipMemcpyHostToDevice, st));
    TSP_HIP(hipMemsetAsync(d_count, 0, 4 * sizeof(unsigned long long), st));
    const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
    ix.grid = grid;
    hipLaunchKernelGGL(smooth_bbox_kernel, dim3(grid), dim3(256), 0, st, dx.as<float>(), dy.as<float>(), dz.as<float>(), n, d_mm);
    TSP_HIP(hipGetLastError());
    unsigned hmm[6];
    TSP_HIP(hipMemcpyAsync(hmm, d_mm, sizeof(hmm), hipMemcpyDeviceToHost, st));
    TSP_HIP(hipStreamSynchronize(st));

    Grid &g = ix.g;
    g = {};
    g.period = period;
    double maxabs = period;
    for (int a = 0; a < 3; ++a) {
        const float lo = unordered_bits(hmm[a]), hi = unordered_bits(hmm[3 + a]);
        if (hmm[a] > hmm[3 + a]) break;      // no finite particle at all
        maxabs = std::max(maxabs, std::max(fabs((double)lo), fabs((double)hi)));
        const double extent = period > 0.0f ? (double)period : (double)hi - (double)lo;
        ix.extent[a] = extent;
        g.lo[a] = period > 0.0f ? 0.0f : lo;
        if (extent > 1e-30 && extent < 1e38) {
            g.inv[a] = (float)((double)(1 << QBITS) / extent);
            g.step[a] = (float)(extent / (double)(1 << QBITS));
        }
    }
    g.eps = (float)(1e-5 * maxabs) + 1e-30f;

    TSP_SCRATCH_ALLOC(ctx, SITE("index_keys"), keys, (size_t)n * sizeof(uint64_t));
    TSP_SCRATCH_ALLOC(ctx, SITE("index_keys_sorted"), keys2, (size_t)n * sizeof(uint64_t));
    TSP_SCRATCH_ALLOC(ctx, SITE("index_order"), vals, (size_t)n * sizeof(uint32_t));
    TSP_SCRATCH_ALLOC(ctx, SITE("index_order_sorted"), vals2, (size_t)n * sizeof(uint32_t));
    hipLaunchKernelGGL(smooth_key_kernel, dim3(grid), dim3(256), 0, st, dx.as<float>(), dy.as<float>(), dz.as<float>(), n, g,
                       keys.as<uint64_t>(), vals.as<uint32_t>(), d_count);
    TSP_HIP(hipGetLastError());
    unsigned long long nv_u = 0;
    TSP_HIP(hipMemcpyAsync(&nv_u, d_count, sizeof(nv_u), hipMemcpyDeviceToHost, st));
    TSP_HIP(hipStreamSynchronize(st));
    const int64_t nv = (int64_t)nv_u;
    ix.nv = nv;
    TSP_REQUIRE(nv >= min_valid, TSP_EINVAL, "%s: %lld particles have finite coordinates, n_neighbours = %d needs at least as many",
                who, (long long)nv, min_valid);
    {
        DeviceScratch tmp;
        size_t tmp_bytes = 0;
        TSP_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, keys.as<uint64_t>(), keys2.as<uint64_t>(), vals.as<uint32_t>(),
                                                   vals2.as<uint32_t>(), (int)n, 0, 64, st));
        TSP_SCRATCH_ALLOC(ctx, SITE("index_sort_tmp"), tmp, tmp_bytes);
        TSP_HIP(hipcub::DeviceRadixSort::SortPairs(tmp.p, tmp_bytes, keys.as<uint64_t>(), keys2.as<uint64_t>(), vals.as<uint32_t>(),
                                                   vals2.as<uint32_t>(), (int)n, 0, 64, st));
        TSP_HIP(hipStreamSynchronize(st));
    }
    keys.reset(nullptr);
    TSP_SCRATCH_ALLOC(ctx, SITE("index_sorted_x"), sx, (size_t)nv * sizeof(float));
    TSP_SCRATCH_ALLOC(ctx, SITE("index_sorted_y"), sy, (size_t)nv * sizeof(float));
    TSP_SCRATCH_ALLOC(ctx, SITE("index_sorted_z"), sz, (size_t)nv * sizeof(float));
    hipLaunchKernelGGL(smooth_gather_kernel, dim3(grid), dim3(256), 0, st, dx.as<float>(), dy.as<float>(), dz.as<float>(),
                       vals2.as<uint32_t>(), nv, sx.as<float>(), sy.as<float>(), sz.as<float>());
    TSP_HIP(hipGetLastError());
    return TSP_OK;
}

int smoothing_lengths(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, int k, float period,
                      float *h_out) {
    hipStream_t st = ctx->stream;
    const size_t fbytes = (size_t)n * sizeof(float);
    MortonIndex ix;
    const int rc = build_morton_index(ctx, "tsp_smoothing_lengths", n, x, y, z, period, k, ix);
    if (rc != TSP_OK) return rc;
    DeviceScratch &dx = ix.dx, &keys2 = ix.keys2, &vals = ix.vals, &vals2 = ix.vals2, &sx = ix.sx, &sy = ix.sy, &sz = ix.sz;
    const Grid &g = ix.g;
    const int64_t nv = ix.nv;
    const unsigned grid = ix.grid;
    unsigned long long *d_count = ix.d_count;

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

// The host side of both gather calls over the index.  mode SPH_GATHER_SUM: fields = {a}, outs = {out} (tsp_sph_sum);
// SPH_GATHER_VELOCITY_GRADIENT: fields = {mass, rho, vx, vy, vz}, outs = {div, curl_x, curl_y, curl_z}.
// Device memory beyond the index: the raw h ("sph_sum_h", n floats) and one buffer ("sph_sum_a") partitioned by offsets --
//   sum:      [a: n]                                                                        (4 bytes per particle)
//   gradient: [mass, rho, vx, vy, vz: 5 n, padded to 16 bytes][(mass, vx, vy, vz) sorted: 4 nv]   (36 bytes per particle)
// -- and the buffers of the index that are free once the positions are gathered: the raw y and z hold the sorted h and the sorted
// second per-query field (a | rho).  The sorted results go where nothing is read any more (sum: the unsorted index buffer;
// gradient: the first four raw planes, dead once they are gathered), the results in the caller's order into the raw x (sum) or the
// raw x, the raw h, the unsorted index buffer and the fifth raw plane (gradient).  The stream orders every reuse.
int sph_sum(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, const float *h, int mode,
            const float *const *fields, int n_fields, float period, float *const *outs, int n_outs) {
    const bool gradient = mode == SPH_GATHER_VELOCITY_GRADIENT;
    const char *who = gradient ? "tsp_sph_velocity_gradient" : "tsp_sph_sum";
    TSP_REQUIRE(n_fields == (gradient ? 5 : 1) && n_outs == (gradient ? 4 : 1), TSP_EINVAL, "%s: %d fields and %d outputs", who,
                n_fields, n_outs);
    hipStream_t st = ctx->stream;
    const size_t fbytes = (size_t)n * sizeof(float);
    MortonIndex ix;
    const int rc = build_morton_index(ctx, who, n, x, y, z, period, 0, ix);
    if (rc != TSP_OK) return rc;
    const int64_t nv = ix.nv;

    // h and the fields into Morton order; the raw y and z buffers are free once the positions are gathered
    DeviceScratch dh, da;
    const size_t raw_floats = ((size_t)n_fields * (size_t)n + 3) & ~(size_t)3;     // (the float4 payload starts 16-byte aligned)
    const size_t a_floats = gradient ? raw_floats + 4 * (size_t)nv : (size_t)n;
    const int rc_scratch = gather_scratch(ctx, dh, fbytes, da, a_floats * sizeof(float));
    if (rc_scratch != TSP_OK) return rc_scratch;
    TSP_HIP(hipMemcpyAsync(dh.p, h, fbytes, hipMemcpyHostToDevice, st));
    float *raw[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int f = 0; f < n_fields; ++f) {
        raw[f] = da.as<float>() + (size_t)f * (size_t)n;
        TSP_HIP(hipMemcpyAsync(raw[f], fields[f], fbytes, hipMemcpyHostToDevice, st));
    }
    float *sh = ix.dy.as<float>(), *sa = ix.dz.as<float>();
    const float *sorted[4] = {nullptr, nullptr, nullptr, nullptr};     // the results in Morton order
    float *unsorted[4] = {nullptr, nullptr, nullptr, nullptr};         // and in the caller's order
    const dim3 query_grid((unsigned)((nv + 255) / 256));
    if (!gradient) {
        hipLaunchKernelGGL(sph_gather_kernel, dim3(ix.grid), dim3(256), 0, st, dh.as<float>(), raw[0], ix.vals2.as<uint32_t>(), nv, sh,
                           sa);
        TSP_HIP(hipGetLastError());
        // queries in Morton order; the sorted result reuses the unsorted index buffer
        float *out_sorted = ix.vals.as<float>();
        if (nv > 0) {
            hipLaunchKernelGGL(sph_sum_kernel, query_grid, dim3(256), 0, st, ix.sx.as<float>(), ix.sy.as<float>(), ix.sz.as<float>(), sh,
                               sa, ix.keys2.as<uint64_t>(), nv, ix.g, out_sorted, ix.d_count + 1);
            TSP_HIP(hipGetLastError());
        }
        sorted[0] = out_sorted;
        unsorted[0] = ix.dx.as<float>();
    } else {
        float4 *smv = reinterpret_cast<float4 *>(da.as<float>() + raw_floats);
        hipLaunchKernelGGL(sph_gather_velocity_kernel, dim3(ix.grid), dim3(256), 0, st, dh.as<float>(), raw[0], raw[1], raw[2], raw[3],
                           raw[4], ix.vals2.as<uint32_t>(), nv, sh, sa, smv);
        TSP_HIP(hipGetLastError());
        if (nv > 0) {
            hipLaunchKernelGGL(sph_velocity_gradient_kernel, query_grid, dim3(256), 0, st, ix.sx.as<float>(), ix.sy.as<float>(),
                               ix.sz.as<float>(), sh, sa, smv, ix.keys2.as<uint64_t>(), nv, ix.g, raw[0], raw[1], raw[2], raw[3],
                               ix.d_count + 1);
            TSP_HIP(hipGetLastError());
        }
        for (int c = 0; c < 4; ++c) sorted[c] = raw[c];
        unsorted[0] = ix.dx.as<float>(), unsorted[1] = dh.as<float>(), unsorted[2] = ix.vals.as<float>(), unsorted[3] = raw[4];
    }
    // back to the caller's order; invalid particles get NaN
    for (int c = 0; c < n_outs; ++c) {
        hipLaunchKernelGGL(smooth_scatter_kernel, dim3(ix.grid), dim3(256), 0, st, sorted[c], ix.vals2.as<uint32_t>(), n, nv, unsorted[c]);
        TSP_HIP(hipGetLastError());
    }
    unsigned long long counts[3] = {0, 0, 0};
    TSP_HIP(hipMemcpyAsync(counts, ix.d_count + 1, sizeof(counts), hipMemcpyDeviceToHost, st));
    TSP_HIP(hipStreamSynchronize(st));
    for (int c = 0; c < n_outs; ++c) TSP_HIP(hipMemcpy(outs[c], unsorted[c], fbytes, hipMemcpyDeviceToHost));
    // measurement aid: TOPSY_SMOOTH_STATS=1 reports the candidates scanned and the terms summed per query, and the share of
    // the lanes' scan steps that had a candidate (the last step of a run is rarely full)
    const char *env = getenv("TOPSY_SMOOTH_STATS");
    if (env && env[0] == '1')
        fprintf(stderr, "%s: n=%lld valid=%lld candidates=%llu per_query=%.2f terms=%llu per_query=%.2f lane_use=%.3f\n", who,
                (long long)n, (long long)nv, counts[0], nv ? (double)counts[0] / (double)nv : 0.0, counts[1],
                nv ? (double)counts[1] / (double)nv : 0.0, counts[2] ? (double)counts[0] / (64.0 * (double)counts[2]) : 0.0);
    return TSP_OK;
}

// The host side of tsp_sph_sample_lattice (the arguments are checked by the entry point).  nq = nu nv nw lattice points, F fields,
// W = the payload width (1, 2 or 4 floats; F = 3 -> 4).  Device memory beyond the index, through the two sites of the gather calls:
//   "sph_sum_h": [h of the lattice points, C order: nq floats]
//   "sph_sum_a": [the raw fields: F n floats, padded to 16 bytes][the payload records in Morton order: W nv floats, padded to 16
//                bytes][the F results, C order: F nq floats]
// Nothing of the index is reused: its buffers are sized by n, the results by nq.  The kernels write h and the results at the
// points' C-ordered positions, so each output comes back by one contiguous copy, after every allocation and kernel has succeeded.
int sph_sample_lattice(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, int n_fields,
                       const float *const *fields, int k, float period, const tsp_lattice *lattice, float *h_out,
                       float *const *outs) {
    const char *who = "tsp_sph_sample_lattice";
    const char *env = getenv("TOPSY_SMOOTH_STATS");
    const bool stats = env && env[0] == '1';
    hipStream_t st = ctx->stream;
    const auto t0 = std::chrono::steady_clock::now();
    MortonIndex ix;
    const int rc = build_morton_index(ctx, who, n, x, y, z, period, k, ix);
    if (rc != TSP_OK) return rc;
    const int64_t nv = ix.nv;

    // the bricks of the query order: a ray, a slice or a volume
    LatticeQueries lq;
    lq.lat = *lattice;
    const bool ray = lattice->nv == 1 && lattice->nw == 1, slice = lattice->nw == 1;
    lq.bu = ray ? 64 : slice ? 8 : 4;
    lq.bv = ray ? 1 : slice ? 8 : 4;
    lq.bw = ray || slice ? 1 : 4;
    lq.nbu = (lattice->nu + lq.bu - 1) / lq.bu;
    lq.nbv = (lattice->nv + lq.bv - 1) / lq.bv;
    const int64_t nbw = (lattice->nw + lq.bw - 1) / lq.bw;
    lq.n_slots = 64 * ((int64_t)lq.nbu * lq.nbv * nbw);
    const int64_t nq = (int64_t)lattice->nu * lattice->nv * lattice->nw;
    const int64_t query_blocks = (lq.n_slots + 255) / 256;
    TSP_REQUIRE(query_blocks < (1ll << 31), TSP_EINVAL, "%s: a %d x %d x %d lattice takes too many bricks", who, lattice->nu,
                lattice->nv, lattice->nw);

    DeviceScratch dh, da;
    const int W = n_fields == 3 ? 4 : n_fields;
    const size_t fbytes = (size_t)n * sizeof(float);
    const size_t raw_floats = ((size_t)n_fields * (size_t)n + 3) & ~(size_t)3;
    const size_t payload_floats = ((size_t)W * (size_t)nv + 3) & ~(size_t)3;
    const int rc_scratch = gather_scratch(ctx, dh, (size_t)nq * sizeof(float),
                                          da, (raw_floats + payload_floats + (size_t)n_fields * (size_t)nq) * sizeof(float));
    if (rc_scratch != TSP_OK) return rc_scratch;
    float *raw = da.as<float>(), *payload = raw + raw_floats, *out_lin = payload + payload_floats, *h_lin = dh.as<float>();
    for (int f = 0; f < n_fields; ++f)
        TSP_HIP(hipMemcpyAsync(raw + (size_t)f * (size_t)n, fields[f], fbytes, hipMemcpyHostToDevice, st));
    const uint32_t *order = ix.vals2.as<uint32_t>();
    if (W == 1)
        hipLaunchKernelGGL(lattice_gather_kernel<1>, dim3(ix.grid), dim3(256), 0, st, raw, n, n_fields, order, nv, payload);
    else if (W == 2)
        hipLaunchKernelGGL(lattice_gather_kernel<2>, dim3(ix.grid), dim3(256), 0, st, raw, n, n_fields, order, nv, payload);
    else
        hipLaunchKernelGGL(lattice_gather_kernel<4>, dim3(ix.grid), dim3(256), 0, st, raw, n, n_fields, order, nv, payload);
    TSP_HIP(hipGetLastError());
    if (stats) TSP_HIP(hipStreamSynchronize(st));
    const auto t1 = std::chrono::steady_clock::now();

    // step A: h at the lattice points, a lane per point
    const float *sx = ix.sx.as<float>(), *sy = ix.sy.as<float>(), *sz = ix.sz.as<float>();
    const uint64_t *keys = ix.keys2.as<uint64_t>();
    const dim3 query_grid((unsigned)query_blocks);
    if (k <= 8)
        hipLaunchKernelGGL(lattice_knn_kernel<8>, query_grid, dim3(256), 0, st, sx, sy, sz, keys, nv, k, ix.g, lq, h_lin, ix.d_count + 1);
    else if (k <= 16)
        hipLaunchKernelGGL(lattice_knn_kernel<16>, query_grid, dim3(256), 0, st, sx, sy, sz, keys, nv, k, ix.g, lq, h_lin, ix.d_count + 1);
    else if (k <= 32)
        hipLaunchKernelGGL(lattice_knn_kernel<32>, query_grid, dim3(256), 0, st, sx, sy, sz, keys, nv, k, ix.g, lq, h_lin, ix.d_count + 1);
    else
        hipLaunchKernelGGL(lattice_knn_kernel<64>, query_grid, dim3(256), 0, st, sx, sy, sz, keys, nv, k, ix.g, lq, h_lin, ix.d_count + 1);
    TSP_HIP(hipGetLastError());
    // the search's counter makes room for the three of the sums (the stream orders the copy before the memset)
    unsigned long long n_dist = 0;
    TSP_HIP(hipMemcpyAsync(&n_dist, ix.d_count + 1, sizeof(n_dist), hipMemcpyDeviceToHost, st));
    TSP_HIP(hipMemsetAsync(ix.d_count + 1, 0, sizeof(unsigned long long), st));
    if (stats) TSP_HIP(hipStreamSynchronize(st));
    const auto t2 = std::chrono::steady_clock::now();

    // step B: the sums, a wave per point
    if (W == 1)
        hipLaunchKernelGGL(lattice_sum_kernel<1>, query_grid, dim3(256), 0, st, sx, sy, sz, payload, keys, nv, ix.g, lq, h_lin, n_fields,
                           nq, out_lin, ix.d_count + 1);
    else if (W == 2)
        hipLaunchKernelGGL(lattice_sum_kernel<2>, query_grid, dim3(256), 0, st, sx, sy, sz, payload, keys, nv, ix.g, lq, h_lin, n_fields,
                           nq, out_lin, ix.d_count + 1);
    else
        hipLaunchKernelGGL(lattice_sum_kernel<4>, query_grid, dim3(256), 0, st, sx, sy, sz, payload, keys, nv, ix.g, lq, h_lin, n_fields,
                           nq, out_lin, ix.d_count + 1);
    TSP_HIP(hipGetLastError());
    unsigned long long counts[3] = {0, 0, 0};
    TSP_HIP(hipMemcpyAsync(counts, ix.d_count + 1, sizeof(counts), hipMemcpyDeviceToHost, st));
    TSP_HIP(hipStreamSynchronize(st));
    const auto t3 = std::chrono::steady_clock::now();
    const size_t qbytes = (size_t)nq * sizeof(float);
    if (h_out) TSP_HIP(hipMemcpy(h_out, h_lin, qbytes, hipMemcpyDeviceToHost));
    for (int f = 0; f < n_fields; ++f) TSP_HIP(hipMemcpy(outs[f], out_lin + (size_t)f * (size_t)nq, qbytes, hipMemcpyDeviceToHost));
    const auto t4 = std::chrono::steady_clock::now();
    // measurement aid: TOPSY_SMOOTH_STATS=1 reports the stage times (the stream is synchronised between the stages then), the
    // distances of the search, the candidates scanned and the terms summed per lattice point, and the share of the lanes' scan
    // steps that had a candidate
    if (stats) {
        const auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        fprintf(stderr, "%s: n=%lld valid=%lld k=%d fields=%d lattice=%dx%dx%d brick=%dx%dx%d index_ms=%.3f knn_ms=%.3f sum_ms=%.3f "
                "readback_ms=%.3f distances_per_query=%.2f candidates=%llu per_query=%.2f terms=%llu per_query=%.2f lane_use=%.3f\n",
                who, (long long)n, (long long)nv, k, n_fields, lattice->nu, lattice->nv, lattice->nw, lq.bu, lq.bv, lq.bw, ms(t0, t1),
                ms(t1, t2), ms(t2, t3), ms(t3, t4), (double)n_dist / (double)nq, counts[0], (double)counts[0] / (double)nq, counts[1],
                (double)counts[1] / (double)nq, counts[2] ? (double)counts[0] / (64.0 * (double)counts[2]) : 0.0);
    }
    return TSP_OK;
}

}  // namespace tsp
