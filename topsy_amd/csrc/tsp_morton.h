// tsp_morton.h -- the Morton index over caller-ordered host positions and the exact float32 fixed-radius range query over it:
// what tsp_smooth.hip (tsp_smoothing_lengths, tsp_sph_sum, tsp_sph_velocity_gradient) and tsp_fof.hip (tsp_fof_groups) share.
//
// The index (build_morton_index, tsp_smooth.hip): bounding box of the finite positions; 63-bit Morton keys of the positions
// quantised to 2^21 steps per axis (a periodic box: the positions wrapped into [0, L), for binning only -- distances always
// use the raw coordinates); invalid particles get the key ~0 and sort last; hipcub radix sort of (key, index), gather of the
// sorted x, y, z.  The prefixes of the sorted keys form an octree whose cells are contiguous runs.
//
// The range query (query_cells, for_each_run): the finest level at which the query's box of half-width R touches at most two
// cells per axis, those (at most eight) runs by binary search -- the own cell first.  A cell whose box lies farther than the
// reach is skipped.  The box test is conservative: cell faces are widened by a margin (Grid::eps) that covers the float32
// rounding of the quantisation, the wrap and the distances themselves, so a point the rounding puts into the neighbouring
// cell is still found.
#pragma once
#include "tsp_internal.h"

namespace tsp {

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

static __device__ __forceinline__ bool finite3(float x, float y, float z) {
    return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
}

// the position binned on axis a: wrapped into [0, L) in a periodic box
static __device__ __forceinline__ float grid_coord(float v, float period) {
    return period > 0.0f ? v - period * floorf(v / period) : v;
}

// floor((v - lo) * inv), held inside +-2^23 (enough for any box of half-width up to the whole domain; an overflowing
// v - lo saturates instead of becoming undefined)
static __device__ __forceinline__ int qstep(float v, float lo, float inv) {
    if (inv == 0.0f) return 0;
    float t = (v - lo) * inv;
    t = fminf(fmaxf(t, -8388608.0f), 8388608.0f);
    return (int)floorf(t);
}
static __device__ __forceinline__ int qclamp(int u) { return min(max(u, 0), QMAX); }

static __device__ __forceinline__ uint64_t spread3(uint64_t x) {     // 21 bits -> every third bit
    x &= 0x1fffffull;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}
static __device__ __forceinline__ uint64_t morton3(uint32_t a, uint32_t b, uint32_t c) {
    return spread3(a) | (spread3(b) << 1) | (spread3(c) << 2);
}

// The contract's distance: float32, these operations in this order (-ffp-contract=off keeps them unfused).  Every step is
// odd-symmetric in dx (negation, division, rint to nearest-even, the product and the difference all commute with a sign
// change), so dist2(i, j) and dist2(j, i) are the same bits.
static __device__ __forceinline__ float min_image(float d, float period) {
    float t = __fdiv_rn(d, period);
    t = rintf(t);
    return d - period * t;
}
static __device__ __forceinline__ float dist2(float qx, float qy, float qz, float px, float py, float pz, float period) {
    float dx = px - qx, dy = py - qy, dz = pz - qz;
    if (period > 0.0f) {
        dx = min_image(dx, period);
        dy = min_image(dy, period);
        dz = min_image(dz, period);
    }
    return (dx * dx + dy * dy) + dz * dz;
}
// The displacement itself, p - q at the nearest image, for the sums that need its direction (tsp_sph_velocity_gradient); returns
// d2 formed from it by the operations of dist2 in dist2's order, so the bits are dist2's.
static __device__ __forceinline__ float displacement(float qx, float qy, float qz, float px, float py, float pz, float period,
                                                     float &dx, float &dy, float &dz) {
    dx = px - qx, dy = py - qy, dz = pz - qz;
    if (period > 0.0f) {
        dx = min_image(dx, period);
        dy = min_image(dy, period);
        dz = min_image(dz, period);
    }
    return (dx * dx + dy * dy) + dz * dz;
}

// The contract's lattice point (tsp_sph_sample_lattice): ((origin + i du) + j dv) + k dw per axis in float64, these operations in
// this order, unfused, rounded once to float32.  The host forms the corners by the same code when it checks the lattice.
static __host__ __device__ __forceinline__ void lattice_point(const tsp_lattice &lat, int i, int j, int k, float &x, float &y, float &z) {
    float p[3];
    for (int a = 0; a < 3; ++a)
        p[a] = (float)(((lat.origin[a] + (double)i * lat.du[a]) + (double)j * lat.dv[a]) + (double)k * lat.dw[a]);
    x = p[0], y = p[1], z = p[2];
}

// first index in [lo, hi) whose key is >= key (hi when none)
static __device__ __forceinline__ int64_t key_lower_bound(const uint64_t *__restrict__ keys, int64_t lo, int64_t hi, uint64_t key) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
static __device__ __forceinline__ int64_t key_lower_bound(const uint64_t *__restrict__ keys, int64_t nv, uint64_t key) {
    return key_lower_bound(keys, 0, nv, key);
}

// distance along one axis from q to the step interval [c 2^s, (c + 1) 2^s) of the grid (and its periodic images), less the margin
static __device__ __forceinline__ float axis_gap(const Grid &g, int a, float q, int c, int s) {
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

// The cells a query's box touches: the level at which the box of half-width R around (qx, qy, qz) touches at most two cells
// per axis.  q = the binned coordinates of the query, s = the level's shift (cells of 2^s steps; the grid has
// 2^(QBITS - s) cells per axis), and per axis the query's own cell and the other cell the box touches (unwrapped index;
// equal to own when none).
struct QueryCells {
    float q[3];
    int s;
    int own[3], other[3];
};
static __device__ __forceinline__ QueryCells query_cells(const Grid &g, float qx, float qy, float qz, float R) {
    QueryCells qc;
    const float L = g.period;
    qc.q[0] = grid_coord(qx, L), qc.q[1] = grid_coord(qy, L), qc.q[2] = grid_coord(qz, L);
    int uq[3], ua[3], ub[3];
    for (int a = 0; a < 3; ++a) {
        uq[a] = qclamp(qstep(qc.q[a], g.lo[a], g.inv[a]));
        ua[a] = qstep(qc.q[a] - R, g.lo[a], g.inv[a]);
        ub[a] = qstep(qc.q[a] + R, g.lo[a], g.inv[a]);
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
    qc.s = s;
    const int ncell = 1 << (QBITS - s);
    for (int a = 0; a < 3; ++a) {
        qc.own[a] = uq[a] >> s;
        const int ca = ua[a] >> s, cb = ub[a] >> s;
        qc.other[a] = (ncell == 1) ? qc.own[a] : (ca != qc.own[a] ? ca : cb);
    }
    return qc;
}

// combo = 0 .. 7 selects per axis the own (bit clear) or the other cell; false when the combination repeats another one
static __device__ __forceinline__ bool combo_cell(const QueryCells &qc, int combo, int (&c)[3]) {
    bool skip = false;
    for (int a = 0; a < 3; ++a) {
        const bool second = (combo >> a) & 1;
        if (second && qc.other[a] == qc.own[a]) skip = true;
        c[a] = second ? qc.other[a] : qc.own[a];
    }
    return !skip;
}

// the run [b, e) of the sorted keys that is cell c of the level with shift s
static __device__ __forceinline__ void cell_run(const uint64_t *__restrict__ keys, int64_t nv, const int (&c)[3], int s, int64_t &b,
                                                int64_t &e) {
    const int ncell = 1 << (QBITS - s);
    const uint64_t prefix = morton3((uint32_t)(c[0] & (ncell - 1)), (uint32_t)(c[1] & (ncell - 1)), (uint32_t)(c[2] & (ncell - 1)));
    const int shift = 3 * s;
    b = key_lower_bound(keys, nv, prefix << shift);
    e = key_lower_bound(keys, nv, (prefix + 1) << shift);
}

// A range query of squared radius < cull2 / CULL_SLACK (float64, the slack included by the caller) around a query whose
// box has half-width R: emit(combo, b, e) for every run that may hold a particle inside.  Returns the candidates in them.
template <typename Emit>
static __device__ __forceinline__ unsigned long long for_each_run(const Grid &g, const uint64_t *__restrict__ keys, int64_t nv,
                                                                 float qx, float qy, float qz, float R, double cull2, Emit emit) {
    const QueryCells qc = query_cells(g, qx, qy, qz, R);
    unsigned long long scanned = 0;
    for (int combo = 0; combo < 8; ++combo) {
        int c[3];
        if (!combo_cell(qc, combo, c)) continue;
        const double gx = axis_gap(g, 0, qc.q[0], c[0], qc.s);
        const double gy = axis_gap(g, 1, qc.q[1], c[1], qc.s);
        const double gz = axis_gap(g, 2, qc.q[2], c[2], qc.s);
        if ((gx * gx + gy * gy) + gz * gz > cull2) continue;
        int64_t b, e;
        cell_run(keys, nv, c, qc.s, b, e);
        emit(combo, b, e);
        scanned += (unsigned long long)(e - b);
    }
    return scanned;
}

// Step 1 of every entry point over the index: the raw positions on the device (dx, dy, dz), the grid, the sorted keys
// (keys2) with the sort's index (vals2: sorted -> caller's order), and the positions of the nv valid particles in Morton order
// (sx, sy, sz).  vals (n x 4 bytes) is free for the caller's per-query result once the sort is done.
struct MortonIndex {
    DeviceScratch dx, dy, dz, keys2, vals, vals2, sx, sy, sz, mm;
    Grid g = {};
    double extent[3] = {0, 0, 0};            // what the 2^21 steps of every axis span (the period, or max - min of the finite positions)
    int64_t nv = 0;
    unsigned grid = 0;                       // blocks of the grid-stride kernels
    unsigned long long *d_count = nullptr;   // [0] valid particles, [1] .. [3] the caller's counters (zeroed)
};

// min_valid: the call is refused (TSP_EINVAL) when fewer particles have finite coordinates
int build_morton_index(tsp_context *ctx, const char *who, int64_t n, const float *x, const float *y, const float *z, float period,
                       int min_valid, MortonIndex &ix);

}  // namespace tsp
