// tsp_fof.hip -- friends-of-friends groups of caller-ordered host positions (tsp_fof_groups): the halo catalogue that arrays
// do not carry, what the reference's center = "halo-N" needs (PynbodyDataLoader._perform_centering, src/topsy/loader.py:203-206).
//
// Contract (include/topsy_splat.h): two particles with finite coordinates are linked iff the float32 d2 of tsp_smoothing_lengths
// (dist2(), tsp_morton.h; nearest image in a periodic box) is <= ll2 = linking_length * linking_length (float32); the groups are
// the connected components, ranked 1, 2, ... by (size descending, smallest member index ascending) when they have at least
// min_members members.  Everything is an integer and the partition is unique, so the output does not depend on the order in which
// the atomics below resolve.
//
// The passes, over the Morton index of tsp_morton.h (build_morton_index), every array in Morton order:
//   1. parent[]: a union-find forest on 32-bit parents.  A parent is never larger than its child, so a root is the smallest
//      Morton position of its tree.  hook: find both roots (path halving), atomicCAS the larger root under the smaller, retry
//      when the CAS lost.  No lane ever waits for another one (lock-free, no spin on a flag).
//   2. the same-cell shortcut.  s_c = the coarsest octree level (cells of 2^s_c steps) with
//          sum over the axes of (W_a + 4 eps)^2 * (1 + 1e-4) <= ll2,      W_a = the cell's width on axis a, eps = Grid::eps.
//      Two particles of one such cell are linked by the contract's own test: their binned (wrapped) coordinates differ by at
//      most W_a plus the rounding of the binning (the subtraction of the origin, the product with the rounded steps-per-length,
//      the wrap v - L floor(v / L): a few ulp of the largest coordinate, < eps = 1e-5 of it), the float32 dx of raw coordinates
//      -- the nearest-image step included -- differs from that by a few ulp of the largest coordinate again (< eps), and the
//      three products and two sums of d2 add a relative 4 * 2^-24, far inside the factor 1 + 1e-4.  So d2 <= ll2 holds for every
//      pair of the cell, in float32, with a margin of more than eps per axis.  An axis whose extent the grid cannot bin (inv = 0)
//      counts with its whole extent as W_a.  parent[i] then starts at the first particle of i's cell (one binary search), which
//      chains all occupants without an atomic.  The shortcut is used when the fullest cell of that level holds at least
//      SHORTCUT_MIN_CELL particles (measured: below that it costs more than it saves); otherwise, and without a level that
//      passes, parent[i] = i and every pair is tested.
//   3. the link kernel: a range query of radius linking_length over the octree of key prefixes (for_each_run: the level choice,
//      conservative box test and eps margin of sph_sum_kernel).  Step A, one lane per query: its runs into LDS.  Step B, one wave
//      per query: 64 candidates per step, coalesced, each tested with d2 <= ll2.  A link is symmetric, so a query looks only at
//      candidates before its own cell in Morton order (before itself without the shortcut): the later particle of a pair finds
//      it.  Of the hits of a step, the first one of every shortcut cell hooks (its cell-mates are in its tree already), and when
//      the last hit's cell runs past the step the scan jumps to the end of that cell (one binary search): a query in a dense
//      core tests about 64 candidates per neighbouring cell, not the cell's whole population.
//   4. flatten + sizes: root[i] = find(i) (read-only); group sizes and smallest member index (caller's order) by integer
//      atomics on the root, one per run of equal roots in a wave.
//   5. ranking: roots with size >= min_members get the 64-bit key (~size << 32 | smallest index), everything else ~0; hipcub
//      radix sort of (key, position); the r-th sorted root has rank r + 1.
//   6. group_out in the caller's order through the sort's index: the rank of the root, 0 for a small group, -1 for an invalid
//      particle.
// Device memory: the index (48 bytes per particle at its peak, 40 afterwards) and 8 bytes per particle of ranking keys; every
// other array reuses a buffer of the index that is free by then: about 48 bytes per particle.
#include <hipcub/hipcub.hpp>

#include <math.h>
#include <stdlib.h>

#include "tsp_morton.h"

namespace tsp {
namespace {

// parent[] is read and written by every workgroup of a launch: relaxed agent-scope atomics, so no load is served from a
// cache another workgroup's store did not reach.  (A stale parent would still be an ancestor -- parents only ever move up the
// tree -- and the CAS validates the root; the atomics are what guarantees progress.)
__device__ __forceinline__ uint32_t uf_load(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void uf_store(uint32_t *p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// root of x, halving the path: every write replaces a parent by the grandparent, an ancestor still
__device__ __forceinline__ uint32_t uf_find(uint32_t *parent, uint32_t x) {
    for (;;) {
        const uint32_t u = uf_load(parent + x);
        if (u == x) return x;
        const uint32_t gp = uf_load(parent + u);
        if (gp == u) return u;
        uf_store(parent + x, gp);
        x = gp;
    }
}
__device__ __forceinline__ uint32_t uf_find_readonly(const uint32_t *parent, uint32_t x) {
    for (;;) {
        const uint32_t u = uf_load(parent + x);
        if (u == x) return x;
        x = u;
    }
}
// true when the call joined two trees
__device__ __forceinline__ bool uf_hook(uint32_t *parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return false;
        const uint32_t hi = max(a, b), lo = min(a, b);
        const uint32_t old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return true;
        a = old, b = lo;      // hi got a parent meanwhile: go on from there
    }
}

// The shortcut is used when its largest cell holds at least this many particles.  Measured: where no cell
// outgrows a few wave steps the jump never happens, and the cell id of every candidate (8 more bytes next to its 12 of
// coordinates) makes the scan 10-55 % slower; 16 steps' worth of one cell is where a query starts to save whole steps.
constexpr unsigned long long SHORTCUT_MIN_CELL = 1024;

// the shortcut cell of a key (shift = 3 s_c)
__device__ __forceinline__ uint64_t cell_of(uint64_t key, int shift) { return key >> shift; }

// 2. parent[i] = the first particle of i's shortcut cell; shift < 0: i.  max_cell: the largest population of a cell (the last
// particle of a cell sees all of it)
__global__ __launch_bounds__(256) void fof_init_kernel(const uint64_t *__restrict__ keys, int64_t nv, int shift,
                                                       uint32_t *__restrict__ parent, unsigned long long *max_cell) {
    unsigned long long most = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t head = shift < 0 ? i : key_lower_bound(keys, 0, i, cell_of(keys[i], shift) << shift);
        parent[i] = (uint32_t)head;
        most = max(most, (unsigned long long)(i - head + 1));
    }
    for (int off = 32; off; off >>= 1) most = max(most, (unsigned long long)__shfl_xor(most, off));
    if ((threadIdx.x & 63) == 0 && most > 1) atomicMax(max_cell, most);
}

// 3. counters: [0] candidates tested, [1] hooks that joined two trees, [2] wave steps
__global__ __launch_bounds__(256) void fof_link_kernel(const float *__restrict__ sx, const float *__restrict__ sy,
                                                       const float *__restrict__ sz, const uint64_t *__restrict__ keys, int64_t nv,
                                                       Grid g, float ll, float ll2, int shift, uint32_t *parent,
                                                       unsigned long long *counters) {
    __shared__ uint32_t run_b[256][8], run_e[256][8];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63, wave0 = threadIdx.x & ~63;
    const float L = g.period;
    unsigned long long tested = 0, steps = 0, links = 0;
    float qx = 0.0f, qy = 0.0f, qz = 0.0f;
    for (int r = 0; r < 8; ++r) run_b[threadIdx.x][r] = run_e[threadIdx.x][r] = 0;
    if (i < nv) {
        qx = sx[i], qy = sy[i], qz = sz[i];
        // every link has d2 <= ll2; the slack covers the rounding of ll2 and of d2
        const float reach = ll * CULL_SLACK;
        const float R = reach + g.eps;
        const double cull2 = ((double)reach * (double)reach) * (double)CULL_SLACK;
        // candidates before the query's own cell only (before the query itself without the shortcut)
        const int64_t limit = shift < 0 ? i : key_lower_bound(keys, 0, i, cell_of(keys[i], shift) << shift);
        for_each_run(g, keys, nv, qx, qy, qz, R, cull2, [&](int combo, int64_t b, int64_t e) {
            e = min(e, limit);
            if (b < e) {
                run_b[threadIdx.x][combo] = (uint32_t)b;      // (nv < 2^31)
                run_e[threadIdx.x][combo] = (uint32_t)e;
            }
        });
    }
    __syncthreads();

    const unsigned long long todo = __ballot(i < nv);
    for (int l = 0; l < 64; ++l) {
        if (!((todo >> l) & 1)) continue;                   // (uniform over the wave)
        const float lx = __shfl(qx, l), ly = __shfl(qy, l), lz = __shfl(qz, l);
        const uint32_t qi = (uint32_t)(i - lane + l);
        for (int r = 0; r < 8; ++r) {
            const int64_t b = run_b[wave0 + l][r], e = run_e[wave0 + l][r];
            int64_t j0 = b;
            while (j0 < e) {                                // (uniform over the wave)
                const int64_t j = j0 + lane;
                bool hit = false;
                uint64_t cj = 0;
                if (j < e) {
                    hit = dist2(lx, ly, lz, sx[j], sy[j], sz[j], L) <= ll2;
                    if (shift >= 0) cj = cell_of(keys[j], shift);
                    ++tested;
                }
                ++steps;
                const unsigned long long mask = __ballot(hit);
                int64_t next = j0 + 64;
                if (mask) {
                    bool leader = hit;
                    if (shift >= 0) {
                        // one hook per cell: a hit whose predecessor in the step is a hit of the same cell leaves it to that one
                        const uint64_t cprev = __shfl_up(cj, 1);
                        if (lane > 0 && ((mask >> (lane - 1)) & 1) && cprev == cj) leader = false;
                        // the last hit's cell is done; when it reaches past this step, go on behind it
                        const int top = 63 - __builtin_clzll(mask);
                        const uint64_t ctop = __shfl(cj, top), clast = __shfl(cj, 63);
                        if (next < e && ctop == clast) next = key_lower_bound(keys, next, e, (clast + 1) << shift);
                    }
                    if (leader && uf_hook(parent, qi, (uint32_t)j)) ++links;
                }
                j0 = next;
            }
        }
    }

    for (int off = 32; off; off >>= 1) {
        tested += __shfl_xor(tested, off);
        links += __shfl_xor(links, off);
    }
    if (lane == 0 && steps) {
        atomicAdd(&counters[0], tested);
        atomicAdd(&counters[1], links);
        atomicAdd(&counters[2], steps);
    }
}

// 4. root[] (a buffer of its own: nothing is written into parent[], which the other waves still walk), size[root] and
// first[root] = the smallest caller's index of the tree.  Launched with whole waves; size zeroed, first filled with ~0.
__global__ __launch_bounds__(256) void fof_flatten_kernel(const uint32_t *__restrict__ parent, const uint32_t *__restrict__ idx,
                                                          int64_t nv, uint32_t *__restrict__ root, uint32_t *size, uint32_t *first) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool in = i < nv;
    uint32_t r = 0xffffffffu, m = 0xffffffffu;      // (no root: nv < 2^31)
    if (in) {
        r = uf_find_readonly(parent, (uint32_t)i);
        root[i] = r;
        m = idx[i];
    }
    // one pair of atomics per run of equal roots in the wave: Morton neighbours mostly share their group
    // (the lanes past the array hold a root of their own, so a run also ends where the array does)
    const uint32_t rprev = __shfl_up(r, 1);
    const bool head = lane == 0 || rprev != r;
    const unsigned long long heads = __ballot(head);
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t mo = __shfl_down(m, off), ro = __shfl_down(r, off);
        if (lane + off < 64 && ro == r) m = min(m, mo);
    }
    if (head && in) {
        const unsigned long long later = lane == 63 ? 0ull : (heads >> (lane + 1));
        const int len = later ? __builtin_ctzll(later) + 1 : 64 - lane;
        atomicAdd(size + r, (uint32_t)len);
        atomicMin(first + r, m);
    }
}

// 5. counters: [0] ranked groups, [1] particles in them, [2] the largest size
__global__ __launch_bounds__(256) void fof_rank_key_kernel(const uint32_t *__restrict__ root, const uint32_t *__restrict__ size,
                                                           const uint32_t *__restrict__ first, int64_t nv, int64_t min_members,
                                                           uint64_t *__restrict__ rkeys, uint32_t *__restrict__ pos,
                                                           unsigned long long *counters) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
        uint64_t key = ~0ull;
        if (root[i] == (uint32_t)i && (int64_t)size[i] >= min_members) {
            key = ((uint64_t)(~size[i]) << 32) | first[i];
            atomicAdd(&counters[0], 1ull);
            atomicAdd(&counters[1], (unsigned long long)size[i]);
            atomicMax(&counters[2], (unsigned long long)size[i]);
        }
        rkeys[i] = key;
        pos[i] = (uint32_t)i;
    }
}

__global__ __launch_bounds__(256) void fof_rank_kernel(const uint32_t *__restrict__ sorted_pos, const unsigned long long *counters,
                                                       int32_t *__restrict__ rank_of) {
    const int64_t n_groups = (int64_t)counters[0];
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_groups; r += (int64_t)gridDim.x * blockDim.x)
        rank_of[sorted_pos[r]] = (int32_t)(r + 1);
}

// 6. the caller's order; the invalid particles are the last n - nv of the sort
__global__ __launch_bounds__(256) void fof_scatter_kernel(const uint32_t *__restrict__ root, const int32_t *__restrict__ rank_of,
                                                          const uint32_t *__restrict__ idx, int64_t n, int64_t nv,
                                                          int32_t *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[idx[i]] = i < nv ? rank_of[root[i]] : -1;
}

}  // namespace

int fof_groups(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, float linking_length, float period,
               int64_t min_members, int32_t *group_out, tsp_fof_info *info_out) {
    const char *who = "tsp_fof_groups";
    hipStream_t st = ctx->stream;
    MortonIndex ix;
    const int rc = build_morton_index(ctx, who, n, x, y, z, period, 0, ix);
    if (rc != TSP_OK) return rc;
    const int64_t nv = ix.nv;
    const Grid &g = ix.g;
    const float ll2 = linking_length * linking_length;

    // 2. the shortcut level (the argument is at the head of this file).  TOPSY_FOF_SHORTCUT=0 / 1 (measurement and test aid):
    // never / whenever a level passes; otherwise when a cell of that level holds at least SHORTCUT_MIN_CELL particles
    int shift = -1;
    const char *env = getenv("TOPSY_FOF_SHORTCUT");
    const bool never = env && env[0] == '0', always = env && env[0] == '1';
    if (!never) {
        for (int s = QBITS; s >= 0 && shift < 0; --s) {
            double sum = 0.0;
            for (int a = 0; a < 3; ++a) {
                const double w = (g.inv[a] == 0.0f ? ix.extent[a] : ldexp((double)g.step[a], s)) + 4.0 * (double)g.eps;
                sum += w * w;
            }
            if (sum * (1.0 + 1e-4) <= (double)ll2) shift = 3 * s;
        }
    }
    const int level = shift < 0 ? -1 : QBITS - shift / 3;
    unsigned long long max_cell = 0;

    // every array below reuses a buffer of the index that is free by now (n or nv elements of 4 bytes each)
    uint32_t *parent = ix.vals.as<uint32_t>();       // the unsorted index: free since the sort
    uint32_t *size = ix.dx.as<uint32_t>();           // the raw coordinates: free since the gather
    uint32_t *first = ix.dy.as<uint32_t>();
    unsigned long long counts[3] = {0, 0, 0}, ranked[3] = {0, 0, 0};
    int32_t *out = ix.dz.as<int32_t>();
    if (nv > 0) {
        const dim3 per_particle((unsigned)((nv + 255) / 256));
        const uint64_t *keys = ix.keys2.as<uint64_t>();
        hipLaunchKernelGGL(fof_init_kernel, dim3(ix.grid), dim3(256), 0, st, keys, nv, shift, parent, ix.d_count + 1);
        TSP_HIP(hipGetLastError());
        if (shift >= 0) {
            TSP_HIP(hipMemcpyAsync(&max_cell, ix.d_count + 1, sizeof(max_cell), hipMemcpyDeviceToHost, st));
            TSP_HIP(hipMemsetAsync(ix.d_count + 1, 0, sizeof(max_cell), st));
            TSP_HIP(hipStreamSynchronize(st));
            if (!always && max_cell < SHORTCUT_MIN_CELL) {
                shift = -1;
                hipLaunchKernelGGL(fof_init_kernel, dim3(ix.grid), dim3(256), 0, st, keys, nv, shift, parent, ix.d_count + 1);
                TSP_HIP(hipGetLastError());
            }
        }
        hipLaunchKernelGGL(fof_link_kernel, per_particle, dim3(256), 0, st, ix.sx.as<float>(), ix.sy.as<float>(), ix.sz.as<float>(),
                           keys, nv, g, linking_length, ll2, shift, parent, ix.d_count + 1);
        TSP_HIP(hipGetLastError());
        TSP_HIP(hipMemcpyAsync(counts, ix.d_count + 1, sizeof(counts), hipMemcpyDeviceToHost, st));

        // 4. (the sorted positions are free once the links are made: sz becomes root[])
        uint32_t *root = ix.sz.as<uint32_t>();
        TSP_HIP(hipMemsetAsync(size, 0, (size_t)nv * sizeof(uint32_t), st));
        TSP_HIP(hipMemsetAsync(first, 0xff, (size_t)nv * sizeof(uint32_t), st));
        hipLaunchKernelGGL(fof_flatten_kernel, per_particle, dim3(256), 0, st, parent, ix.vals2.as<uint32_t>(), nv, root, size, first);
        TSP_HIP(hipGetLastError());

        // 5. (the sorted keys are free too: they take the sorted ranking keys; sx the sorted positions, sy the ranks)
        DeviceScratch rkeys, tmp;
        TSP_SCRATCH_ALLOC(ctx, SITE("fof_rank_keys"), rkeys, (size_t)nv * sizeof(uint64_t));
        uint32_t *pos = ix.dz.as<uint32_t>(), *sorted_pos = ix.sx.as<uint32_t>();
        int32_t *rank_of = ix.sy.as<int32_t>();
        TSP_HIP(hipMemsetAsync(ix.d_count + 1, 0, 3 * sizeof(unsigned long long), st));
        hipLaunchKernelGGL(fof_rank_key_kernel, dim3(ix.grid), dim3(256), 0, st, root, size, first, nv, min_members,
                           rkeys.as<uint64_t>(), pos, ix.d_count + 1);
        TSP_HIP(hipGetLastError());
        size_t tmp_bytes = 0;
        TSP_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, rkeys.as<uint64_t>(), ix.keys2.as<uint64_t>(), pos, sorted_pos,
                                                   (int)nv, 0, 64, st));
        TSP_SCRATCH_ALLOC(ctx, SITE("fof_sort_tmp"), tmp, tmp_bytes);
        TSP_HIP(hipcub::DeviceRadixSort::SortPairs(tmp.p, tmp_bytes, rkeys.as<uint64_t>(), ix.keys2.as<uint64_t>(), pos, sorted_pos,
                                                   (int)nv, 0, 64, st));
        TSP_HIP(hipMemsetAsync(rank_of, 0, (size_t)nv * sizeof(int32_t), st));
        hipLaunchKernelGGL(fof_rank_kernel, dim3(ix.grid), dim3(256), 0, st, sorted_pos, ix.d_count + 1, rank_of);
        TSP_HIP(hipGetLastError());
        TSP_HIP(hipMemcpyAsync(ranked, ix.d_count + 1, sizeof(ranked), hipMemcpyDeviceToHost, st));

        // 6. (pos is free since the sort: dz takes the output)
        hipLaunchKernelGGL(fof_scatter_kernel, dim3(ix.grid), dim3(256), 0, st, root, rank_of, ix.vals2.as<uint32_t>(), n, nv, out);
        TSP_HIP(hipGetLastError());
        TSP_HIP(hipStreamSynchronize(st));      // (before rkeys and tmp are released)
    } else {
        TSP_HIP(hipMemsetAsync(out, 0xff, (size_t)n * sizeof(int32_t), st));     // nobody is valid: -1 everywhere
        TSP_HIP(hipStreamSynchronize(st));
    }
    TSP_HIP(hipMemcpy(group_out, out, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (info_out) {
        info_out->n_valid = nv;
        info_out->n_groups = (int64_t)ranked[0];
        info_out->n_grouped = (int64_t)ranked[1];
        info_out->largest = (int64_t)ranked[2];
    }
    // measurement aid: TOPSY_SMOOTH_STATS=1 reports the candidates tested per query, the hooks that joined two trees and the
    // share of the lanes' scan steps that had a candidate
    const char *stats = getenv("TOPSY_SMOOTH_STATS");
    if (stats && stats[0] == '1')
        fprintf(stderr, "tsp_fof_groups: n=%lld valid=%lld shortcut_level=%d cell_level=%d max_cell=%llu candidates=%llu per_query=%.2f links=%llu lane_use=%.3f "
                        "groups=%llu grouped=%llu largest=%llu\n",
                (long long)n, (long long)nv, shift < 0 ? -1 : level, level, max_cell, counts[0], nv ? (double)counts[0] / (double)nv : 0.0,
                counts[1], counts[2] ? (double)counts[0] / (64.0 * (double)counts[2]) : 0.0, ranked[0], ranked[1], ranked[2]);
    return TSP_OK;
}

}  // namespace tsp
