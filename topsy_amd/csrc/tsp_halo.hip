// tsp_halo.hip -- the haloes of a catalogue in one call: the self-potential of every halo by a direct sum confined to the halo
// (tsp_group_potential) and per-halo reductions -- mass, centre, velocity, shape, spin, energies, radii (tsp_halo_properties).
// Contracts: include/topsy_splat.h.  Layout, rounding, resources and measured rates: DESIGN.md section 4.
//
// Shared front end.  key = the label of a valid member, ~0 for everything else; one stable 32-bit radix sort of (key, index): the
// members of a halo are then contiguous ("sorted positions" p) and in the caller's index order, start[label] / end[label] bound
// them (halo_bounds_kernel: single writers, no atomics), the anchor is the member at start[label].  Offsets d from the anchor in
// float64 without fused multiply-adds (the Makefile's -ffp-contract=off).
//
// tsp_group_potential.  halo_pairs_kernel is gravity_pairs_kernel (tsp_gravity.hip) over the sorted members: 256 lanes, TPL = 4
// targets per lane, so a workgroup owns HALO_BLOCK = 1024 consecutive sorted targets, whatever halo boundaries fall inside.  The
// union of its targets' source ranges is a contiguous range of sorted positions; it is staged through LDS in tiles of 512 aligned
// to the sorted array, (x, y, z, m) float4 + eps^2 + label, broadcast reads, the next tile's loads in flight.  A pair counts iff
// the labels agree, the positions differ and r2 >= 2^-126: these tests run only in a tile that needs one of them (CHECK, per tile
// for the whole workgroup); a tile wholly inside the one halo that all of the block's targets belong to, away from the block's own
// positions and without a tiny eps^2, takes gravity_tile's unchecked form.  A masked pair adds +0 to a float32 run, which changes
// no bit, so both forms give the same bits.  A block whose range is long is cut into up to 16 work items of at least 2 tiles each
// (a function of the range alone, not of the device); the items' float64 partials are added in item order by
// halo_pairs_reduce_kernel, which also scatters to the caller's order.  Launches are chunked to 4096 items (32 MB of partials).
//
// tsp_halo_properties.  Every pass is the same fixed two-level scheme: a workgroup takes a slice of 256 consecutive sorted
// positions, each lane forms its member's terms, and the first lane of every run of equal labels adds the run in position order
// (slice_pieces): one partial ("piece") per (halo, slice).  A piece that starts a slice lives in A[slice], one that starts inside a
// slice (it is then the halo's first) in B[label].  halo_combine: one wave per halo; lane l adds the l-th chunk of ceil(pieces / 64)
// consecutive pieces in order, lane 0 adds the lanes in order.  The association is a function of start and end alone.  Pass 3 sorts
// (label << 32 | float bits of |e|, position) once more (stable: ties keep the index order) and forms the running mass the same
// way: piece sums, their exclusive prefix per halo, then the prefix inside the slice.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "tsp_internal.h"

namespace tsp {
namespace {

constexpr int TILE = TSP_HALO_SOURCE_TILE;       // sources per LDS tile
constexpr int LANES = 256;
constexpr int TPL = 4;                            // targets per lane
constexpr int BL = TSP_HALO_TARGET_BLOCK;        // sorted targets of a workgroup
constexpr int RUN = 16;                           // consecutive sources summed in float32 (gravity_tile's)
constexpr int PER_LANE = TILE / LANES;
constexpr int SPLIT_TILES = 2;                    // a work item takes at least this many tiles (unless the block's range is shorter)
constexpr int MAX_SPLITS = 16;                    // work items of a block at most
constexpr int MAX_ITEMS = 4096;                   // work items of a launch at most (their partials: 32 MB)
constexpr int SLICE = 256;                        // sorted positions of a reduction workgroup
constexpr float R2_NORMAL = 1.17549435e-38f;      // 2^-126
constexpr float E2_UNCHECKED = 7.88860905e-31f;   // 2^-100
constexpr uint32_t NO_LABEL = 0xffffffffu;
static_assert(BL == LANES * TPL && TILE % LANES == 0 && TILE % RUN == 0 && SLICE == LANES, "tile and block shapes");

// counters[]: integers only (floating-point values as their bit patterns, which order like the values when these are >= 0)
enum { C_MEMBERS, C_NONEMPTY, C_PAIRS, C_SKIPPED_GROUPS, C_SKIPPED_MEMBERS, C_MAX_EXTENT, C_COUNT = 8 };

struct ValidSpec {        // a member is valid iff every f[k][i] is finite and, if positive is set, positive[i] > 0
    const float *f[8];
    int nf;
    const float *positive;
    float eps_all;        // checked when has_eps_all
    int has_eps_all;
};

__device__ __forceinline__ double wave_max(double v) {
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ __launch_bounds__(256) void halo_keys_kernel(const int32_t *__restrict__ group, int64_t n, uint32_t n_groups, ValidSpec spec,
                                                        uint32_t *__restrict__ keys, uint32_t *__restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t g = group[i];
    bool valid = g >= 1 && (uint32_t)g <= n_groups;
    for (int k = 0; k < spec.nf; ++k) valid = valid && isfinite(spec.f[k][i]);
    if (spec.positive) valid = valid && spec.positive[i] > 0.0f;
    if (spec.has_eps_all) valid = valid && isfinite(spec.eps_all);
    keys[i] = valid ? (uint32_t)g : NO_LABEL;
    idx[i] = (uint32_t)i;
}

// start / end (zeroed before) of every label that has members, and the member count: every word has one writer
__global__ __launch_bounds__(256) void halo_bounds_kernel(const uint32_t *__restrict__ keys, int64_t n, uint32_t *__restrict__ start,
                                                          uint32_t *__restrict__ end, unsigned long long *__restrict__ counters) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const uint32_t k = keys[p];
    if (k == NO_LABEL) return;
    if (p == 0 || keys[p - 1] != k) start[k] = (uint32_t)p;
    if (p == n - 1 || keys[p + 1] != k) {
        end[k] = (uint32_t)(p + 1);
        if (p == n - 1 || keys[p + 1] == NO_LABEL) counters[C_MEMBERS] = (unsigned long long)(p + 1);
    }
}

__global__ __launch_bounds__(256) void halo_group_stats_kernel(const uint32_t *__restrict__ start, const uint32_t *__restrict__ end,
                                                               uint32_t n_groups, uint32_t max_members,
                                                               unsigned long long *__restrict__ counters) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x + 1;
    unsigned long long c = 0;
    if (g <= (int64_t)n_groups) c = end[g] - start[g];
    const bool skipped = max_members && c > max_members;
    const unsigned long long nonempty = wave_sum(c ? 1ull : 0ull), pairs = wave_sum(skipped ? 0ull : c * (c ? c - 1 : 0)),
                             sg = wave_sum(skipped ? 1ull : 0ull), sm = wave_sum(skipped ? c : 0ull);
    if ((threadIdx.x & 63) == 0) {
        if (nonempty) atomicAdd(counters + C_NONEMPTY, nonempty);
        if (pairs) atomicAdd(counters + C_PAIRS, pairs);
        if (sg) atomicAdd(counters + C_SKIPPED_GROUPS, sg);
        if (sm) atomicAdd(counters + C_SKIPPED_MEMBERS, sm);
    }
}

// the offset of the member at sorted position p from its halo's anchor, per axis: float64, nearest image when period > 0
__device__ __forceinline__ double anchor_offset(float xi, float xa, double period) {
    double d = (double)xi - (double)xa;
    if (period > 0.0) d -= period * rint(d / period);
    return d;
}

__device__ __forceinline__ void note_extent(double ext, unsigned long long *counters) {
    ext = wave_max(ext);
    if ((threadIdx.x & 63) == 0 && ext > 0.0) atomicMax(counters + C_MAX_EXTENT, (unsigned long long)__double_as_longlong(ext));
}

__global__ __launch_bounds__(256) void halo_potential_prepare_kernel(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ idx,
                                                                     const uint32_t *__restrict__ start, uint32_t n_members,
                                                                     const float *__restrict__ x, const float *__restrict__ y,
                                                                     const float *__restrict__ z, const float *__restrict__ m,
                                                                     const float *__restrict__ eps, float eps_all, double period,
                                                                     float4 *__restrict__ e4, float *__restrict__ e2,
                                                                     unsigned long long *__restrict__ counters) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    double ext = 0.0;
    if (p < n_members) {
        const uint32_t i = idx[p], a = idx[start[keys[p]]];
        const double dx = anchor_offset(x[i], x[a], period), dy = anchor_offset(y[i], y[a], period), dz = anchor_offset(z[i], z[a], period);
        const float e = eps ? eps[i] : eps_all;
        e4[p] = make_float4((float)dx, (float)dy, (float)dz, m[i]);
        e2[p] = e * e;
        ext = fmax(fabs(dx), fmax(fabs(dy), fabs(dz)));
    }
    note_extent(ext, counters);
}

// per block of BL sorted targets: the tiles [x, y) that hold the members of its targets' haloes, the skipped haloes left out
__global__ __launch_bounds__(256) void halo_block_ranges_kernel(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ start,
                                                                const uint32_t *__restrict__ end, uint32_t n_members,
                                                                uint32_t max_members, int n_blocks, int2 *__restrict__ ranges) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= n_blocks) return;
    const uint32_t first = (uint32_t)b * BL, last = min(n_members, first + BL);       // targets [first, last)
    uint32_t lo = NO_LABEL, hi = 0, p = first;
    while (p < last) {                                                               // from halo to halo
        const uint32_t k = keys[p], s = start[k], e = end[k];
        if (!(max_members && e - s > max_members)) {
            lo = min(lo, s);
            hi = max(hi, e);
        }
        p = e;
    }
    ranges[b] = lo < hi ? make_int2((int)(lo / TILE), (int)((hi + TILE - 1) / TILE)) : make_int2(0, 0);
}

// gravity_tile (tsp_gravity.hip) with the label test: potential only
template <bool CHECK>
__device__ __forceinline__ void halo_tile(const float4 *__restrict__ s4, const float *__restrict__ se2, const uint32_t *__restrict__ sl,
                                          uint32_t tile_base, const uint32_t (&tl)[TPL], const uint32_t (&tp)[TPL],
                                          const float (&px)[TPL], const float (&py)[TPL], const float (&pz)[TPL], double (&sum)[TPL]) {
    // (every checked pair in flight holds lane masks in scalar registers: unrolled by 2 they fit, by 16 the tile loop's scalars spill)
    constexpr int UNROLL = CHECK ? 2 : RUN;
    for (int k0 = 0; k0 < TILE; k0 += RUN) {
        float f[TPL];
#pragma unroll
        for (int t = 0; t < TPL; ++t) f[t] = 0.0f;
#pragma unroll UNROLL
        for (int kk = 0; kk < RUN; ++kk) {
            const float4 s = s4[k0 + kk];
            const float e2 = se2[k0 + kk];
            const uint32_t lab = CHECK ? sl[k0 + kk] : 0u;
#pragma unroll
            for (int t = 0; t < TPL; ++t) {
                const float dx = px[t] - s.x, dy = py[t] - s.y, dz = pz[t] - s.z;
                const float r2 = __builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, __builtin_fmaf(dz, dz, e2)));
                float inv = __builtin_amdgcn_rsqf(r2);
                if (CHECK) inv = (r2 >= R2_NORMAL && tl[t] == lab && tp[t] != tile_base + (uint32_t)(k0 + kk)) ? inv : 0.0f;
                f[t] += s.w * inv;
            }
        }
#pragma unroll
        for (int t = 0; t < TPL; ++t) sum[t] += (double)f[t];
    }
}

// items[w] = (block, first tile, end tile, partial slot); partials[slot * BL + local], local = t * 256 + lane
__global__ __launch_bounds__(256) void halo_pairs_kernel(const float4 *__restrict__ e4, const float *__restrict__ e2,
                                                         const uint32_t *__restrict__ keys, const uint32_t *__restrict__ start,
                                                         const uint32_t *__restrict__ end, uint32_t n_members, uint32_t max_members,
                                                         const int4 *__restrict__ items, double *__restrict__ partials) {
    __shared__ float4 s4[TILE];
    __shared__ float se2s[TILE];
    __shared__ uint32_t sls[TILE];
    const int lane = threadIdx.x;
    const int4 item = items[blockIdx.x];
    const uint32_t first = (uint32_t)item.x * BL;
    const int tile_lo = item.y, tile_hi = item.z;

    float px[TPL], py[TPL], pz[TPL];
    uint32_t tl[TPL], tp[TPL];
    double sum[TPL];
    const uint32_t lab0 = keys[first];       // (a block exists only where first < n_members)
    int same = 1;
#pragma unroll
    for (int t = 0; t < TPL; ++t) {
        const uint32_t p = first + t * LANES + lane;
        const bool in = p < n_members;
        const uint32_t pc = min(p, n_members - 1);      // (loads at a clamped position, then a select: no divergent branch)
        const uint32_t lab = keys[pc];
        const bool skipped = max_members && end[lab] - start[lab] > max_members;      // a skipped halo: no source matches
        const float4 q = e4[pc];
        px[t] = q.x, py[t] = q.y, pz[t] = q.z;
        tl[t] = in && !skipped ? lab : NO_LABEL, tp[t] = p;
        sum[t] = 0.0;
        same &= !in || tl[t] == lab0;
    }
    // every target of the block belongs to the one halo [u_lo, u_hi): its inner tiles need no label test
    const bool uniform = __syncthreads_and(same);
    const uint32_t u_lo = uniform ? start[lab0] : 0u, u_hi = uniform ? end[lab0] : 0u;

    float4 r4[PER_LANE];
    float re2[PER_LANE];
    uint32_t rl[PER_LANE];
    auto fetch = [&](int tile) {
#pragma unroll
        for (int q = 0; q < PER_LANE; ++q) {
            const uint32_t j = (uint32_t)tile * TILE + q * LANES + lane;
            const bool in = j < n_members;
            const uint32_t jc = min(j, n_members - 1);
            const float4 s = e4[jc];
            r4[q] = in ? s : make_float4(0.0f, 0.0f, 0.0f, 0.0f);      // past the members: the padding source (label 0: no target's)
            re2[q] = in ? e2[jc] : 1.0f;
            rl[q] = in ? keys[jc] : 0u;
        }
    };
    if (tile_lo < tile_hi) fetch(tile_lo);
    for (int tile = tile_lo; tile < tile_hi; ++tile) {
        __syncthreads();      // every wave is done with the tile before
        int tiny = 0;
#pragma unroll
        for (int q = 0; q < PER_LANE; ++q) {
            s4[q * LANES + lane] = r4[q];
            se2s[q * LANES + lane] = re2[q];
            sls[q * LANES + lane] = rl[q];
            tiny |= !(re2[q] >= E2_UNCHECKED);
        }
        const uint32_t tile_base = (uint32_t)tile * TILE;
        const bool own = tile_base < first + BL && tile_base + TILE > first;
        const bool inside = uniform && tile_base >= u_lo && tile_base + TILE <= u_hi;
        const bool check = __syncthreads_or(tiny) || own || !inside;
        if (tile + 1 < tile_hi) fetch(tile + 1);
        if (check)
            halo_tile<true>(s4, se2s, sls, tile_base, tl, tp, px, py, pz, sum);
        else
            halo_tile<false>(s4, se2s, sls, tile_base, tl, tp, px, py, pz, sum);
    }
    double *out = partials + (size_t)item.w * BL;
#pragma unroll
    for (int t = 0; t < TPL; ++t) out[t * LANES + lane] = sum[t];
}

// the targets [p0, p1) of one launch: the block's partials in item order, the sign, NaN for a skipped halo, the caller's order
__global__ __launch_bounds__(256) void halo_pairs_reduce_kernel(const double *__restrict__ partials, const int2 *__restrict__ block_items,
                                                                const uint32_t *__restrict__ keys, const uint32_t *__restrict__ idx,
                                                                const uint32_t *__restrict__ start, const uint32_t *__restrict__ end,
                                                                uint32_t max_members, uint32_t p0, uint32_t p1,
                                                                double *__restrict__ phi) {
    const uint32_t p = p0 + blockIdx.x * 256u + threadIdx.x;
    if (p >= p1) return;
    const int2 bi = block_items[p / BL];       // (first slot, items)
    const double *q = partials + (size_t)bi.x * BL + p % BL;
    double s = 0.0;
    for (int k = 0; k < bi.y; ++k) s += q[(size_t)k * BL];
    const uint32_t lab = keys[p];
    const bool skipped = max_members && end[lab] - start[lab] > max_members;
    phi[idx[p]] = skipped ? (double)NAN : 0.0 - s;
}

__global__ __launch_bounds__(256) void halo_fill_kernel(double *__restrict__ a, int64_t n, double v) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) a[i] = v;
}

// ---- tsp_halo_properties ---------------------------------------------------------------------------------------------------
// One piece per run of equal labels in the slice: the run's first lane adds it in position order.
template <class P>
__device__ __forceinline__ void slice_pieces(const P &mine, bool valid, uint32_t lab, uint32_t p, P *__restrict__ A, P *__restrict__ B) {
    __shared__ P sh[SLICE];
    __shared__ uint32_t shl[SLICE];
    const int tid = threadIdx.x;
    sh[tid] = mine;
    shl[tid] = valid ? lab : NO_LABEL;
    __syncthreads();
    if (valid && (tid == 0 || shl[tid - 1] != lab)) {
        P s = mine;
        for (int k = tid + 1; k < SLICE && shl[k] == lab; ++k) s = P::combine(s, sh[k]);
        if (tid == 0)
            A[p / SLICE] = s;
        else
            B[lab] = s;
    }
}

// The pieces of the halo [s, e) in order: B[lab] if it starts inside a slice, then A[q] of every slice it starts or continues in.
struct PieceList {
    uint32_t has_b, qa, np;
    __device__ PieceList(uint32_t s, uint32_t e) {
        has_b = s % SLICE != 0 ? 1u : 0u;
        qa = (s + SLICE - 1) / SLICE;
        np = s < e ? has_b + ((e + SLICE - 1) / SLICE - qa) : 0u;
    }
    template <class P> __device__ const P &piece(const P *A, const P *B, uint32_t lab, uint32_t k) const {
        return has_b ? (k == 0 ? B[lab] : A[qa + k - 1]) : A[qa + k];
    }
};

// One wave per halo (every wave of the workgroup calls it): lane l adds its chunk of consecutive pieces, lane 0 the lanes.  The
// result is lane 0's; false for a halo without members.
template <class P>
__device__ __forceinline__ bool halo_combine(const P *__restrict__ A, const P *__restrict__ B, uint32_t lab, uint32_t s, uint32_t e, P &out) {
    __shared__ P sh[LANES / 64][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const PieceList pl(s, e);
    const uint32_t chunk = pl.np ? (pl.np + 63) / 64 : 1u;
    const uint32_t k0 = lane * chunk, k1 = min(pl.np, k0 + chunk);
    if (k0 < k1) {
        P acc = pl.piece(A, B, lab, k0);
        for (uint32_t k = k0 + 1; k < k1; ++k) acc = P::combine(acc, pl.piece(A, B, lab, k));
        sh[w][lane] = acc;
    }
    __syncthreads();
    if (lane != 0 || pl.np == 0) return false;
    const uint32_t nl = (pl.np + chunk - 1) / chunk;
    out = sh[w][0];
    for (uint32_t l = 1; l < nl; ++l) out = P::combine(out, sh[w][l]);
    return true;
}

struct P1 {      // pass 1
    double c, m, md[3], mv[3];
    __device__ static P1 combine(const P1 &a, const P1 &b) {
        P1 r;
        r.c = a.c + b.c, r.m = a.m + b.m;
        for (int k = 0; k < 3; ++k) r.md[k] = a.md[k] + b.md[k], r.mv[k] = a.mv[k] + b.mv[k];
        return r;
    }
};
struct P2 {      // pass 2
    double S[6], L[3], ke, rmax, mphi, mb, nb, nbad, phimin, imin;
    __device__ static P2 combine(const P2 &a, const P2 &b) {
        P2 r;
        for (int k = 0; k < 6; ++k) r.S[k] = a.S[k] + b.S[k];
        for (int k = 0; k < 3; ++k) r.L[k] = a.L[k] + b.L[k];
        r.ke = a.ke + b.ke, r.rmax = fmax(a.rmax, b.rmax), r.mphi = a.mphi + b.mphi, r.mb = a.mb + b.mb, r.nb = a.nb + b.nb;
        r.nbad = a.nbad + b.nbad;
        const bool first = a.phimin < b.phimin || (a.phimin == b.phimin && a.imin < b.imin) || !(b.phimin == b.phimin);
        r.phimin = first ? a.phimin : b.phimin, r.imin = first ? a.imin : b.imin;
        return r;
    }
};
struct PM {      // pass 3: the mass of a piece in the radial order
    double m;
    __device__ static PM combine(const PM &a, const PM &b) { return PM{a.m + b.m}; }
};
struct P3 {      // pass 3: the first rank that reaches half the mass; the largest cum / r and its (smallest) rank
    double khalf, v2, kv;
    __device__ static P3 combine(const P3 &a, const P3 &b) {
        P3 r;
        r.khalf = fmin(a.khalf, b.khalf);
        const bool first = a.v2 > b.v2 || (a.v2 == b.v2 && a.kv < b.kv);
        r.v2 = first ? a.v2 : b.v2, r.kv = first ? a.kv : b.kv;
        return r;
    }
};
struct Halo1 {   // per halo after pass 1
    double count, mass, com_off[3], v_com[3];
};

// the sorted member planes: d (the anchor offsets), mass, velocities, phi, by sorted position
struct Members {
    double *d[3];
    float *m, *v[3];
    double *phi;      // nullptr without a potential
    double *re;       // |e|, written by pass 2
    int has_vel;
};

__global__ __launch_bounds__(256) void halo_members_kernel(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ idx,
                                                           const uint32_t *__restrict__ start, uint32_t n_members,
                                                           const float *__restrict__ x, const float *__restrict__ y,
                                                           const float *__restrict__ z, const float *__restrict__ m,
                                                           const float *__restrict__ vx, const float *__restrict__ vy,
                                                           const float *__restrict__ vz, const double *__restrict__ phi, double period,
                                                           Members mem, unsigned long long *__restrict__ counters) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    double ext = 0.0;
    if (p < n_members) {
        const uint32_t i = idx[p], a = idx[start[keys[p]]];
        const double dx = anchor_offset(x[i], x[a], period), dy = anchor_offset(y[i], y[a], period), dz = anchor_offset(z[i], z[a], period);
        mem.d[0][p] = dx, mem.d[1][p] = dy, mem.d[2][p] = dz;
        mem.m[p] = m[i];
        if (mem.has_vel) mem.v[0][p] = vx[i], mem.v[1][p] = vy[i], mem.v[2][p] = vz[i];
        if (mem.phi) mem.phi[p] = phi[i];
        ext = fmax(fabs(dx), fmax(fabs(dy), fabs(dz)));
    }
    note_extent(ext, counters);
}

__global__ __launch_bounds__(256) void halo_pass1_kernel(const uint32_t *__restrict__ keys, uint32_t n_members, Members mem,
                                                         P1 *__restrict__ A, P1 *__restrict__ B) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    const bool valid = p < n_members;
    P1 t = {};
    uint32_t lab = NO_LABEL;
    if (valid) {
        lab = keys[p];
        const double m = (double)mem.m[p];
        t.c = 1.0, t.m = m;
        for (int k = 0; k < 3; ++k) {
            t.md[k] = m * mem.d[k][p];
            t.mv[k] = mem.has_vel ? m * (double)mem.v[k][p] : 0.0;
        }
    }
    slice_pieces(t, valid, lab, p, A, B);
}

__global__ __launch_bounds__(256) void halo_pass1_combine_kernel(const P1 *__restrict__ A, const P1 *__restrict__ B,
                                                                 const uint32_t *__restrict__ start, const uint32_t *__restrict__ end,
                                                                 uint32_t n_groups, Halo1 *__restrict__ halo1) {
    const uint32_t lab = blockIdx.x * (LANES / 64) + (threadIdx.x >> 6) + 1;
    const bool in = lab <= n_groups;
    const uint32_t s = in ? start[lab] : 0u, e = in ? end[lab] : 0u;
    P1 t;
    const bool have = halo_combine(A, B, lab, s, e, t);
    if (!in || (threadIdx.x & 63) != 0) return;
    Halo1 h = {};
    if (have) {
        h.count = t.c, h.mass = t.m;
        for (int k = 0; k < 3; ++k) h.com_off[k] = t.md[k] / t.m, h.v_com[k] = t.mv[k] / t.m;
    }
    halo1[lab] = h;
}

__global__ __launch_bounds__(256) void halo_pass2_kernel(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ idx,
                                                         uint32_t n_members, Members mem, const Halo1 *__restrict__ halo1,
                                                         P2 *__restrict__ A, P2 *__restrict__ B, uint64_t *__restrict__ rkeys,
                                                         uint32_t *__restrict__ rvals) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    const bool valid = p < n_members;
    P2 t = {};
    uint32_t lab = NO_LABEL;
    if (valid) {
        lab = keys[p];
        const Halo1 h = halo1[lab];
        const double m = (double)mem.m[p];
        double e[3], w[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < 3; ++k) {
            e[k] = mem.d[k][p] - h.com_off[k];
            if (mem.has_vel) w[k] = (double)mem.v[k][p] - h.v_com[k];
        }
        t.S[0] = m * e[0] * e[0], t.S[1] = m * e[0] * e[1], t.S[2] = m * e[0] * e[2];
        t.S[3] = m * e[1] * e[1], t.S[4] = m * e[1] * e[2], t.S[5] = m * e[2] * e[2];
        t.L[0] = m * (e[1] * w[2] - e[2] * w[1]), t.L[1] = m * (e[2] * w[0] - e[0] * w[2]), t.L[2] = m * (e[0] * w[1] - e[1] * w[0]);
        const double w2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
        t.ke = m * w2;
        const double r = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
        t.rmax = r;
        mem.re[p] = r;
        rkeys[p] = (uint64_t)lab << 32 | (uint64_t)__float_as_uint((float)r);
        rvals[p] = p;
        if (mem.phi) {
            const double phi = mem.phi[p];
            const bool bound = 0.5 * w2 + phi < 0.0;
            t.mphi = m * phi, t.mb = bound ? m : 0.0, t.nb = bound ? 1.0 : 0.0, t.nbad = isfinite(phi) ? 0.0 : 1.0;
            t.phimin = phi, t.imin = (double)idx[p];
        }
    }
    slice_pieces(t, valid, lab, p, A, B);
}

struct Outputs {
    int64_t *count, *n_bound, *i_pot;
    double *props;
};

__global__ __launch_bounds__(256) void halo_pass2_combine_kernel(const P2 *__restrict__ A, const P2 *__restrict__ B,
                                                                 const uint32_t *__restrict__ start, const uint32_t *__restrict__ end,
                                                                 const uint32_t *__restrict__ idx, uint32_t n_groups,
                                                                 const Halo1 *__restrict__ halo1, const float *__restrict__ x,
                                                                 const float *__restrict__ y, const float *__restrict__ z,
                                                                 int has_vel, int has_phi, double period, Outputs out) {
    const uint32_t lab = blockIdx.x * (LANES / 64) + (threadIdx.x >> 6) + 1;
    const bool in = lab <= n_groups;
    const uint32_t s = in ? start[lab] : 0u, e = in ? end[lab] : 0u;
    P2 t;
    const bool have = halo_combine(A, B, lab, s, e, t);
    if (!in || (threadIdx.x & 63) != 0) return;
    const size_t g = lab - 1;
    double *row = out.props + g * TSP_HALO_NPROPS;
    for (int k = 0; k < TSP_HALO_NPROPS; ++k) row[k] = (double)NAN;
    out.count[g] = 0, out.n_bound[g] = -1, out.i_pot[g] = -1;
    row[TSP_HALO_MASS] = 0.0;
    if (!have) return;
    const Halo1 h = halo1[lab];
    out.count[g] = (int64_t)h.count;
    row[TSP_HALO_MASS] = h.mass;
    const uint32_t a = idx[s];
    const float anchor[3] = {x[a], y[a], z[a]};
    for (int k = 0; k < 3; ++k) {
        double c = (double)anchor[k] + h.com_off[k];
        if (period > 0.0) {
            c -= period * floor(c / period);
            if (c >= period) c -= period;
        }
        row[TSP_HALO_COM + k] = c;
    }
    for (int k = 0; k < 6; ++k) row[TSP_HALO_S + k] = t.S[k];
    row[TSP_HALO_RMAX] = t.rmax;
    if (has_vel) {
        for (int k = 0; k < 3; ++k) row[TSP_HALO_VCOM + k] = h.v_com[k], row[TSP_HALO_L + k] = t.L[k];
        row[TSP_HALO_EKIN] = 0.5 * t.ke;
        row[TSP_HALO_SIGMA2] = 2.0 * (0.5 * t.ke) / (3.0 * h.mass);
    }
    if (has_phi && t.nbad == 0.0) {
        row[TSP_HALO_EPOT] = 0.5 * t.mphi;
        row[TSP_HALO_MBOUND] = t.mb;
        out.n_bound[g] = (int64_t)t.nb;
        const uint32_t i = (uint32_t)t.imin;
        out.i_pot[g] = (int64_t)i;
        row[TSP_HALO_POTPOS] = (double)x[i], row[TSP_HALO_POTPOS + 1] = (double)y[i], row[TSP_HALO_POTPOS + 2] = (double)z[i];
    }
}

// pass 3, level A: the mass of every piece in the radial order (position k of that order holds member rpos[k]; the halo of
// position k is keys[k], because both orders keep the haloes' ranges)
__global__ __launch_bounds__(256) void halo_radial_mass_kernel(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ rpos,
                                                               uint32_t n_members, const float *__restrict__ m, PM *__restrict__ A,
                                                               PM *__restrict__ B) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    const bool valid = k < n_members;
    PM t = {0.0};
    uint32_t lab = NO_LABEL;
    if (valid) lab = keys[k], t.m = (double)m[rpos[k]];
    slice_pieces(t, valid, lab, k, A, B);
}

// level B: the pieces' sums become their exclusive prefixes within the halo, in place, with halo_combine's association
__global__ __launch_bounds__(256) void halo_radial_offsets_kernel(PM *__restrict__ A, PM *__restrict__ B, const uint32_t *__restrict__ start,
                                                                  const uint32_t *__restrict__ end, uint32_t n_groups) {
    __shared__ double sh[LANES / 64][64];
    const uint32_t lab = blockIdx.x * (LANES / 64) + (threadIdx.x >> 6) + 1;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool in = lab <= n_groups;
    const PieceList pl(in ? start[lab] : 0u, in ? end[lab] : 0u);
    const uint32_t chunk = pl.np ? (pl.np + 63) / 64 : 1u;
    const uint32_t k0 = lane * chunk, k1 = min(pl.np, k0 + chunk);
    double acc = 0.0;
    for (uint32_t k = k0; k < k1; ++k) acc += pl.piece(A, B, lab, k).m;
    sh[w][lane] = acc;
    __syncthreads();
    double before = 0.0;
    for (int l = 0; l < lane; ++l) before += sh[w][l];       // (lanes past the pieces hold 0)
    for (uint32_t k = k0; k < k1; ++k) {
        PM *q = const_cast<PM *>(&pl.piece(A, B, lab, k));
        const double mine = q->m;
        q->m = before;
        before += mine;
    }
}

// level C: the running mass of every member, what it says about r_half and v_max, and the pieces of that
__global__ __launch_bounds__(256) void halo_radial_scan_kernel(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ rpos,
                                                               const uint32_t *__restrict__ start, uint32_t n_members,
                                                               const float *__restrict__ m, const double *__restrict__ re,
                                                               const Halo1 *__restrict__ halo1, const PM *__restrict__ offA,
                                                               const PM *__restrict__ offB, P3 *__restrict__ A, P3 *__restrict__ B) {
    __shared__ double shm[SLICE];
    __shared__ uint32_t shlab[SLICE];
    const int tid = threadIdx.x;
    const uint32_t k = blockIdx.x * 256u + tid;
    const bool valid = k < n_members;
    uint32_t lab = NO_LABEL, member = 0;
    if (valid) lab = keys[k], member = rpos[k];
    shm[tid] = valid ? (double)m[member] : 0.0;
    shlab[tid] = lab;
    __syncthreads();
    P3 t = {INFINITY, -1.0, INFINITY};
    if (valid) {
        int h = tid;
        while (h > 0 && shlab[h - 1] == lab) --h;
        double within = shm[h];
        for (int j = h + 1; j <= tid; ++j) within += shm[j];
        const double cum = (h == 0 ? offA[k / SLICE].m : offB[lab].m) + within;
        const double rank = (double)(k - start[lab] + 1);
        const double r = re[member];
        if (cum >= halo1[lab].mass / 2.0) t.khalf = rank;
        if (rank >= 10.0 && r > 0.0) t.v2 = cum / r, t.kv = rank;
    }
    __syncthreads();
    slice_pieces(t, valid, lab, k, A, B);
}

__global__ __launch_bounds__(256) void halo_radial_combine_kernel(const P3 *__restrict__ A, const P3 *__restrict__ B,
                                                                  const uint32_t *__restrict__ start, const uint32_t *__restrict__ end,
                                                                  const uint32_t *__restrict__ idx, const uint32_t *__restrict__ rpos,
                                                                  const double *__restrict__ re, uint32_t n_groups, double *__restrict__ props) {
    const uint32_t lab = blockIdx.x * (LANES / 64) + (threadIdx.x >> 6) + 1;
    const bool in = lab <= n_groups;
    const uint32_t s = in ? start[lab] : 0u, e = in ? end[lab] : 0u;
    P3 t;
    const bool have = halo_combine(A, B, lab, s, e, t);
    if (!in || (threadIdx.x & 63) != 0 || !have) return;
    double *row = props + (size_t)(lab - 1) * TSP_HALO_NPROPS;
    if (t.khalf <= (double)(e - s)) {
        const uint32_t member = rpos[s + (uint32_t)t.khalf - 1];
        row[TSP_HALO_RHALF] = re[member];
        row[TSP_HALO_IHALF] = (double)idx[member];
    }
    if (t.v2 >= 0.0) {
        const uint32_t member = rpos[s + (uint32_t)t.kv - 1];
        row[TSP_HALO_V2MAX] = t.v2;
        row[TSP_HALO_RVMAX] = re[member];
        row[TSP_HALO_IVMAX] = (double)idx[member];
    }
}

size_t align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
struct Carve {      // offsets into one buffer
    size_t size = 0;
    size_t take(size_t bytes) {
        const size_t off = size;
        size += align256(std::max<size_t>(bytes, 16));
        return off;
    }
};

// what both calls share: the sort of (key, index), the haloes' bounds and the counters
struct FrontEnd {
    size_t o_keys_in, o_idx_in, o_keys, o_idx, o_tmp, o_start, o_end, o_counters, tmp_bytes;
    uint32_t *keys = nullptr, *idx = nullptr, *start = nullptr, *end = nullptr;
    unsigned long long *counters = nullptr;
    int plan(Carve &c, int64_t n, int64_t n_groups, hipStream_t st) {
        size_t sort64 = 0;
        tmp_bytes = 0;
        TSP_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                                   (uint32_t *)nullptr, (int)n, 0, 32, st));
        TSP_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort64, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr,
                                                   (uint32_t *)nullptr, (int)n, 0, 64, st));
        tmp_bytes = std::max(tmp_bytes, sort64);      // (the radial sort of the properties uses the same storage)
        o_keys_in = c.take((size_t)n * 4), o_idx_in = c.take((size_t)n * 4), o_keys = c.take((size_t)n * 4), o_idx = c.take((size_t)n * 4);
        o_tmp = c.take(tmp_bytes);
        o_start = c.take((size_t)(n_groups + 1) * 4), o_end = c.take((size_t)(n_groups + 1) * 4);
        o_counters = c.take(C_COUNT * sizeof(unsigned long long));
        return TSP_OK;
    }
    // sorts and bounds; host_counters = the counters after the bounds and the group statistics (synchronises)
    int run(char *b, hipStream_t st, const int32_t *d_group, int64_t n, int64_t n_groups, const ValidSpec &spec, uint32_t max_members,
            unsigned long long (&host_counters)[C_COUNT]) {
        uint32_t *keys_in = reinterpret_cast<uint32_t *>(b + o_keys_in), *idx_in = reinterpret_cast<uint32_t *>(b + o_idx_in);
        keys = reinterpret_cast<uint32_t *>(b + o_keys), idx = reinterpret_cast<uint32_t *>(b + o_idx);
        start = reinterpret_cast<uint32_t *>(b + o_start), end = reinterpret_cast<uint32_t *>(b + o_end);
        counters = reinterpret_cast<unsigned long long *>(b + o_counters);
        const unsigned grid_n = (unsigned)((n + 255) / 256), grid_g = (unsigned)((n_groups + 255) / 256);
        hipLaunchKernelGGL(halo_keys_kernel, dim3(grid_n), dim3(256), 0, st, d_group, n, (uint32_t)n_groups, spec, keys_in, idx_in);
        TSP_HIP(hipGetLastError());
        size_t bytes = tmp_bytes;
        TSP_HIP(hipcub::DeviceRadixSort::SortPairs(b + o_tmp, bytes, keys_in, keys, idx_in, idx, (int)n, 0, 32, st));
        TSP_HIP(hipMemsetAsync(start, 0, (size_t)(n_groups + 1) * 4, st));
        TSP_HIP(hipMemsetAsync(end, 0, (size_t)(n_groups + 1) * 4, st));
        TSP_HIP(hipMemsetAsync(counters, 0, C_COUNT * sizeof(unsigned long long), st));
        hipLaunchKernelGGL(halo_bounds_kernel, dim3(grid_n), dim3(256), 0, st, keys, n, start, end, counters);
        TSP_HIP(hipGetLastError());
        hipLaunchKernelGGL(halo_group_stats_kernel, dim3(grid_g), dim3(256), 0, st, start, end, (uint32_t)n_groups, max_members, counters);
        TSP_HIP(hipGetLastError());
        TSP_HIP(hipMemcpyAsync(host_counters, counters, sizeof(host_counters), hipMemcpyDeviceToHost, st));
        TSP_HIP(hipStreamSynchronize(st));
        return TSP_OK;
    }
};

double bits_to_double(unsigned long long u) {
    double d;
    memcpy(&d, &u, sizeof(d));
    return d;
}

}  // namespace

// The host side of tsp_group_potential (the arguments are checked by the entry point).  Device memory, through the two sites of
// the gather calls: "sph_sum_h" holds the uploaded planes x, y, z, m, eps and the labels; "sph_sum_a" everything else, by offsets.
int group_potential(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, const float *mass, const float *eps,
                    float eps_all, const int32_t *group, int64_t n_groups, double period, int64_t max_members, double *phi_out,
                    tsp_group_potential_info *info_out) {
    hipStream_t st = ctx->stream;
    const char *env = getenv("TOPSY_HALO_STATS");      // measurement aid: the time of the pair and reduce kernels
    const bool stats = env && env[0] == '1';
    const uint32_t maxm = (uint32_t)std::min<int64_t>(max_members, 0x7fffffff);
    const size_t plane = align256((size_t)n * 4);
    const int n_blocks_max = (int)((n + BL - 1) / BL);
    const size_t items_max = (size_t)n_blocks_max * MAX_SPLITS, slots_max = std::min<size_t>(items_max, MAX_ITEMS);

    Carve c;
    FrontEnd fe;
    const int rc_plan = fe.plan(c, n, n_groups, st);
    if (rc_plan != TSP_OK) return rc_plan;
    const size_t o_e4 = c.take((size_t)n * 16), o_e2 = c.take((size_t)n * 4), o_phi = c.take((size_t)n * 8);
    const size_t o_ranges = c.take((size_t)n_blocks_max * sizeof(int2)), o_block_items = c.take((size_t)n_blocks_max * sizeof(int2));
    const size_t o_items = c.take(items_max * sizeof(int4)), o_partials = c.take(slots_max * BL * sizeof(double));

    DeviceScratch dh, da;
    const int rc_scratch = gather_scratch(ctx, dh, 6 * plane, da, c.size);
    if (rc_scratch != TSP_OK) return rc_scratch;
    float *pl[5];
    for (int a = 0; a < 5; ++a) pl[a] = reinterpret_cast<float *>(dh.as<char>() + a * plane);
    int32_t *d_group = reinterpret_cast<int32_t *>(dh.as<char>() + 5 * plane);
    char *b = da.as<char>();
    float4 *e4 = reinterpret_cast<float4 *>(b + o_e4);
    float *e2 = reinterpret_cast<float *>(b + o_e2);
    double *d_phi = reinterpret_cast<double *>(b + o_phi);
    int2 *d_ranges = reinterpret_cast<int2 *>(b + o_ranges), *d_block_items = reinterpret_cast<int2 *>(b + o_block_items);
    int4 *d_items = reinterpret_cast<int4 *>(b + o_items);
    double *d_partials = reinterpret_cast<double *>(b + o_partials);

    const float *host[5] = {x, y, z, mass, eps};
    for (int a = 0; a < (eps ? 5 : 4); ++a) TSP_HIP(hipMemcpyAsync(pl[a], host[a], (size_t)n * 4, hipMemcpyHostToDevice, st));
    TSP_HIP(hipMemcpyAsync(d_group, group, (size_t)n * 4, hipMemcpyHostToDevice, st));
    ValidSpec spec = {};
    for (int a = 0; a < (eps ? 5 : 4); ++a) spec.f[spec.nf++] = pl[a];
    spec.eps_all = eps_all, spec.has_eps_all = eps ? 0 : 1;
    unsigned long long cnt[C_COUNT];
    const int rc_front = fe.run(b, st, d_group, n, n_groups, spec, maxm, cnt);
    if (rc_front != TSP_OK) return rc_front;
    const uint32_t n_members = (uint32_t)cnt[C_MEMBERS];
    const int n_blocks = (int)((n_members + BL - 1) / BL);

    hipLaunchKernelGGL(halo_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_phi, n, (double)NAN);
    TSP_HIP(hipGetLastError());
    int64_t pair_slots = 0;
    float kernel_ms = 0.0f;
    if (n_members) {
        hipLaunchKernelGGL(halo_potential_prepare_kernel, dim3((n_members + 255) / 256), dim3(256), 0, st, fe.keys, fe.idx, fe.start,
                           n_members, pl[0], pl[1], pl[2], pl[3], eps ? pl[4] : nullptr, eps_all, period, e4, e2, fe.counters);
        TSP_HIP(hipGetLastError());
        hipLaunchKernelGGL(halo_block_ranges_kernel, dim3((unsigned)((n_blocks + 255) / 256)), dim3(256), 0, st, fe.keys, fe.start, fe.end,
                           n_members, maxm, n_blocks, d_ranges);
        TSP_HIP(hipGetLastError());
        std::vector<int2> ranges((size_t)n_blocks);
        TSP_HIP(hipMemcpyAsync(ranges.data(), d_ranges, ranges.size() * sizeof(int2), hipMemcpyDeviceToHost, st));
        TSP_HIP(hipStreamSynchronize(st));

        // the work items: a block's range in up to MAX_SPLITS parts of at least SPLIT_TILES tiles; launches of up to MAX_ITEMS items
        std::vector<int4> items;
        std::vector<int2> block_items((size_t)n_blocks);
        struct Launch { int block0, block1, item0, item1; };
        std::vector<Launch> launches;
        Launch cur = {0, 0, 0, 0};
        for (int blk = 0; blk < n_blocks; ++blk) {
            const int t0 = ranges[blk].x, nt = ranges[blk].y - ranges[blk].x;
            const int splits = nt > 0 ? std::min(MAX_SPLITS, (nt + SPLIT_TILES - 1) / SPLIT_TILES) : 0;
            if (cur.item1 - cur.item0 + splits > MAX_ITEMS) {
                launches.push_back(cur);
                cur = {blk, blk, cur.item1, cur.item1};
            }
            block_items[blk] = make_int2(cur.item1 - cur.item0, splits);
            for (int s = 0; s < splits; ++s) {
                const int a0 = t0 + (int)((int64_t)nt * s / splits), a1 = t0 + (int)((int64_t)nt * (s + 1) / splits);
                items.push_back(make_int4(blk, a0, a1, cur.item1 - cur.item0));
                ++cur.item1;
                pair_slots += (int64_t)(a1 - a0) * TILE * BL;
            }
            cur.block1 = blk + 1;
        }
        launches.push_back(cur);
        if (!items.empty()) TSP_HIP(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(int4), hipMemcpyHostToDevice, st));
        TSP_HIP(hipMemcpyAsync(d_block_items, block_items.data(), block_items.size() * sizeof(int2), hipMemcpyHostToDevice, st));
        if (stats) TSP_HIP(hipEventRecord(ctx->ev[EV_T0], st));
        for (const Launch &l : launches) {
            if (l.item1 > l.item0) {
                hipLaunchKernelGGL(halo_pairs_kernel, dim3((unsigned)(l.item1 - l.item0)), dim3(LANES), 0, st, e4, e2, fe.keys, fe.start,
                                   fe.end, n_members, maxm, d_items + l.item0, d_partials);
                TSP_HIP(hipGetLastError());
            }
            const uint32_t p0 = (uint32_t)l.block0 * BL, p1 = std::min<uint32_t>(n_members, (uint32_t)l.block1 * BL);
            if (p1 > p0) {
                hipLaunchKernelGGL(halo_pairs_reduce_kernel, dim3((p1 - p0 + 255) / 256), dim3(256), 0, st, d_partials, d_block_items,
                                   fe.keys, fe.idx, fe.start, fe.end, maxm, p0, p1, d_phi);
                TSP_HIP(hipGetLastError());
            }
        }
        if (stats) TSP_HIP(hipEventRecord(ctx->ev[EV_T1], st));
    }
    std::vector<double> result((size_t)n);
    TSP_HIP(hipMemcpyAsync(result.data(), d_phi, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    TSP_HIP(hipMemcpyAsync(cnt, fe.counters, sizeof(cnt), hipMemcpyDeviceToHost, st));
    TSP_HIP(hipStreamSynchronize(st));
    if (stats && n_members) TSP_HIP(hipEventElapsedTime(&kernel_ms, ctx->ev[EV_T0], ctx->ev[EV_T1]));

    memcpy(phi_out, result.data(), (size_t)n * 8);
    if (info_out) {
        info_out->n_members = (int64_t)cnt[C_MEMBERS];
        info_out->n_groups_nonempty = (int64_t)cnt[C_NONEMPTY];
        info_out->pairs = (int64_t)cnt[C_PAIRS];
        info_out->pair_slots = pair_slots;
        info_out->n_skipped_groups = (int64_t)cnt[C_SKIPPED_GROUPS];
        info_out->n_skipped_members = (int64_t)cnt[C_SKIPPED_MEMBERS];
        info_out->max_extent = bits_to_double(cnt[C_MAX_EXTENT]);
    }
    if (stats)
        fprintf(stderr, "tsp_group_potential: n=%lld members=%llu pairs=%llu slots=%lld kernel_ms=%.4f pairs_per_s=%.4g\n", (long long)n,
                cnt[C_MEMBERS], cnt[C_PAIRS], (long long)pair_slots, kernel_ms,
                kernel_ms > 0.0f ? (double)cnt[C_PAIRS] / (1e-3 * kernel_ms) : 0.0);
    return TSP_OK;
}

// The host side of tsp_halo_properties.  "sph_sum_h": the uploaded planes and labels; "sph_sum_a": everything else, by offsets.
int halo_properties(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, const float *mass, const float *vx,
                    const float *vy, const float *vz, const double *phi, const int32_t *group, int64_t n_groups, double period,
                    int64_t *count_out, int64_t *n_bound_out, int64_t *i_pot_out, double *props_out, tsp_halo_info *info_out) {
    hipStream_t st = ctx->stream;
    const char *env = getenv("TOPSY_HALO_STATS");      // measurement aid: the time of every pass
    const bool stats = env && env[0] == '1';
    const bool has_vel = vx != nullptr, has_phi = phi != nullptr;
    const size_t plane = align256((size_t)n * 4), plane8 = align256((size_t)n * 8);
    const size_t n_slices = (size_t)((n + SLICE - 1) / SLICE), ng1 = (size_t)n_groups + 1;

    Carve c;
    FrontEnd fe;
    const int rc_plan = fe.plan(c, n, n_groups, st);
    if (rc_plan != TSP_OK) return rc_plan;
    size_t o_d[3], o_v[3];
    for (int k = 0; k < 3; ++k) o_d[k] = c.take((size_t)n * 8);
    const size_t o_m = c.take((size_t)n * 4);
    for (int k = 0; k < 3; ++k) o_v[k] = c.take(has_vel ? (size_t)n * 4 : 16);
    const size_t o_phi = c.take(has_phi ? (size_t)n * 8 : 16), o_re = c.take((size_t)n * 8);
    const size_t o_A = c.take(n_slices * sizeof(P2)), o_B = c.take(ng1 * sizeof(P2));      // (P2 is the largest piece)
    const size_t o_offA = c.take(n_slices * sizeof(PM)), o_offB = c.take(ng1 * sizeof(PM));
    const size_t o_halo1 = c.take(ng1 * sizeof(Halo1));
    const size_t o_rkeys = c.take((size_t)n * 8), o_rkeys2 = c.take((size_t)n * 8), o_rvals = c.take((size_t)n * 4), o_rpos = c.take((size_t)n * 4);
    const size_t o_count = c.take((size_t)n_groups * 8), o_nbound = c.take((size_t)n_groups * 8), o_ipot = c.take((size_t)n_groups * 8);
    const size_t o_props = c.take((size_t)n_groups * TSP_HALO_NPROPS * 8);
    static_assert(sizeof(P2) >= sizeof(P1) && sizeof(P2) >= sizeof(P3), "the piece buffers are sized for P2");

    DeviceScratch dh, da;
    const int rc_scratch = gather_scratch(ctx, dh, 8 * plane + plane8, da, c.size);
    if (rc_scratch != TSP_OK) return rc_scratch;
    float *pl[7];
    for (int a = 0; a < 7; ++a) pl[a] = reinterpret_cast<float *>(dh.as<char>() + a * plane);
    int32_t *d_group = reinterpret_cast<int32_t *>(dh.as<char>() + 7 * plane);
    double *d_phi_in = reinterpret_cast<double *>(dh.as<char>() + 8 * plane);
    char *b = da.as<char>();
    Members mem = {};
    for (int k = 0; k < 3; ++k) mem.d[k] = reinterpret_cast<double *>(b + o_d[k]), mem.v[k] = reinterpret_cast<float *>(b + o_v[k]);
    mem.m = reinterpret_cast<float *>(b + o_m);
    mem.phi = has_phi ? reinterpret_cast<double *>(b + o_phi) : nullptr;
    mem.re = reinterpret_cast<double *>(b + o_re);
    mem.has_vel = has_vel ? 1 : 0;
    Halo1 *halo1 = reinterpret_cast<Halo1 *>(b + o_halo1);
    uint64_t *rkeys = reinterpret_cast<uint64_t *>(b + o_rkeys), *rkeys2 = reinterpret_cast<uint64_t *>(b + o_rkeys2);
    uint32_t *rvals = reinterpret_cast<uint32_t *>(b + o_rvals), *rpos = reinterpret_cast<uint32_t *>(b + o_rpos);
    PM *offA = reinterpret_cast<PM *>(b + o_offA), *offB = reinterpret_cast<PM *>(b + o_offB);
    Outputs out = {reinterpret_cast<int64_t *>(b + o_count), reinterpret_cast<int64_t *>(b + o_nbound),
                   reinterpret_cast<int64_t *>(b + o_ipot), reinterpret_cast<double *>(b + o_props)};

    const float *host[7] = {x, y, z, mass, vx, vy, vz};
    for (int a = 0; a < (has_vel ? 7 : 4); ++a) TSP_HIP(hipMemcpyAsync(pl[a], host[a], (size_t)n * 4, hipMemcpyHostToDevice, st));
    TSP_HIP(hipMemcpyAsync(d_group, group, (size_t)n * 4, hipMemcpyHostToDevice, st));
    if (has_phi) TSP_HIP(hipMemcpyAsync(d_phi_in, phi, (size_t)n * 8, hipMemcpyHostToDevice, st));
    ValidSpec spec = {};
    for (int a = 0; a < (has_vel ? 7 : 4); ++a) spec.f[spec.nf++] = pl[a];
    spec.positive = pl[3];
    unsigned long long cnt[C_COUNT];
    const int rc_front = fe.run(b, st, d_group, n, n_groups, spec, 0, cnt);
    if (rc_front != TSP_OK) return rc_front;
    const uint32_t n_members = (uint32_t)cnt[C_MEMBERS], ng = (uint32_t)n_groups;
    const dim3 grid_m((n_members + 255) / 256), grid_h((unsigned)((n_groups + LANES / 64 - 1) / (LANES / 64))), wg(256);

    int ev = EV_T0;
    auto mark = [&]() { return stats && ev <= EV_T5 ? hipEventRecord(ctx->ev[ev++], st) : hipSuccess; };
    TSP_HIP(mark());
    if (n_members) {
        hipLaunchKernelGGL(halo_members_kernel, grid_m, wg, 0, st, fe.keys, fe.idx, fe.start, n_members, pl[0], pl[1], pl[2], pl[3], pl[4],
                           pl[5], pl[6], has_phi ? d_phi_in : nullptr, period, mem, fe.counters);
        TSP_HIP(hipGetLastError());
        hipLaunchKernelGGL(halo_pass1_kernel, grid_m, wg, 0, st, fe.keys, n_members, mem, reinterpret_cast<P1 *>(b + o_A),
                           reinterpret_cast<P1 *>(b + o_B));
        TSP_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(halo_pass1_combine_kernel, grid_h, wg, 0, st, reinterpret_cast<const P1 *>(b + o_A),
                       reinterpret_cast<const P1 *>(b + o_B), fe.start, fe.end, ng, halo1);
    TSP_HIP(hipGetLastError());
    TSP_HIP(mark());
    if (n_members) {
        hipLaunchKernelGGL(halo_pass2_kernel, grid_m, wg, 0, st, fe.keys, fe.idx, n_members, mem, halo1, reinterpret_cast<P2 *>(b + o_A),
                           reinterpret_cast<P2 *>(b + o_B), rkeys, rvals);
        TSP_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(halo_pass2_combine_kernel, grid_h, wg, 0, st, reinterpret_cast<const P2 *>(b + o_A),
                       reinterpret_cast<const P2 *>(b + o_B), fe.start, fe.end, fe.idx, ng, halo1, pl[0], pl[1], pl[2], has_vel ? 1 : 0,
                       has_phi ? 1 : 0, period, out);
    TSP_HIP(hipGetLastError());
    TSP_HIP(mark());
    if (n_members) {
        size_t bytes = fe.tmp_bytes;
        TSP_HIP(hipcub::DeviceRadixSort::SortPairs(b + fe.o_tmp, bytes, rkeys, rkeys2, rvals, rpos, (int)n_members, 0, 64, st));
        TSP_HIP(mark());
        hipLaunchKernelGGL(halo_radial_mass_kernel, grid_m, wg, 0, st, fe.keys, rpos, n_members, mem.m, offA, offB);
        TSP_HIP(hipGetLastError());
        hipLaunchKernelGGL(halo_radial_offsets_kernel, grid_h, wg, 0, st, offA, offB, fe.start, fe.end, ng);
        TSP_HIP(hipGetLastError());
        hipLaunchKernelGGL(halo_radial_scan_kernel, grid_m, wg, 0, st, fe.keys, rpos, fe.start, n_members, mem.m, mem.re, halo1, offA, offB,
                           reinterpret_cast<P3 *>(b + o_A), reinterpret_cast<P3 *>(b + o_B));
        TSP_HIP(hipGetLastError());
        hipLaunchKernelGGL(halo_radial_combine_kernel, grid_h, wg, 0, st, reinterpret_cast<const P3 *>(b + o_A),
                           reinterpret_cast<const P3 *>(b + o_B), fe.start, fe.end, fe.idx, rpos, mem.re, ng, out.props);
        TSP_HIP(hipGetLastError());
        TSP_HIP(mark());
    }
    std::vector<int64_t> ints((size_t)n_groups * 3);
    std::vector<double> props((size_t)n_groups * TSP_HALO_NPROPS);
    TSP_HIP(hipMemcpyAsync(ints.data(), out.count, (size_t)n_groups * 8, hipMemcpyDeviceToHost, st));
    TSP_HIP(hipMemcpyAsync(ints.data() + n_groups, out.n_bound, (size_t)n_groups * 8, hipMemcpyDeviceToHost, st));
    TSP_HIP(hipMemcpyAsync(ints.data() + 2 * n_groups, out.i_pot, (size_t)n_groups * 8, hipMemcpyDeviceToHost, st));
    TSP_HIP(hipMemcpyAsync(props.data(), out.props, props.size() * 8, hipMemcpyDeviceToHost, st));
    TSP_HIP(hipMemcpyAsync(cnt, fe.counters, sizeof(cnt), hipMemcpyDeviceToHost, st));
    TSP_HIP(hipStreamSynchronize(st));
    if (stats) {
        fprintf(stderr, "tsp_halo_properties: n=%lld members=%u groups=%lld ms:", (long long)n, n_members, (long long)n_groups);
        for (int k = EV_T0; k + 1 < ev; ++k) {
            float ms = 0.0f;
            TSP_HIP(hipEventElapsedTime(&ms, ctx->ev[k], ctx->ev[k + 1]));
            fprintf(stderr, " %s=%.4f", k == 0 ? "pass1" : k == 1 ? "pass2" : k == 2 ? "sort" : "pass3", ms);
        }
        fprintf(stderr, "\n");
    }
    memcpy(count_out, ints.data(), (size_t)n_groups * 8);
    memcpy(n_bound_out, ints.data() + n_groups, (size_t)n_groups * 8);
    memcpy(i_pot_out, ints.data() + 2 * n_groups, (size_t)n_groups * 8);
    memcpy(props_out, props.data(), props.size() * 8);
    if (info_out) {
        info_out->n_members = (int64_t)cnt[C_MEMBERS];
        info_out->max_extent = bits_to_double(cnt[C_MAX_EXTENT]);
    }
    return TSP_OK;
}

}  // namespace tsp
