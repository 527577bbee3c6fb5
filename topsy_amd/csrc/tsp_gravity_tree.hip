// tsp_gravity_tree.hip -- Barnes-Hut tree gravity (tsp_gravity_tree): the sums of tsp_gravity_direct (tsp_gravity.hip) in
// O(n log n), by a tree that is implicit in the Morton order of the sources and has no pointers.  Contract: include/topsy_splat.h.
//
// The tree.  build_morton_index (tsp_morton.h) sorts the sources with finite coordinates along the 63-bit Morton curve and hands
// back the sorted positions and the sort's index.  tree_gather_kernel puts (x, y, z, m) and eps^2 of the sorted particles side by
// side, padded to whole leaves with massless particles; a source whose mass or eps is not finite gets m = 0, eps^2 = 1 there and
// is not counted.  A leaf is LEAF = 32 consecutive sorted particles, a node of level l + 1 is FANOUT = 8 consecutive nodes of
// level l: the children of node k are nodes 8 k .. 8 k + 7 of the level below, the levels lie one after the other in the node
// arrays (tsp_gravity_tree_layout.h: levels_of).  tree_leaf_kernel (a lane per leaf) and tree_level_kernel (a lane per node, one
// launch per level, bottom-up) form in float64, in index order and without atomics: M = sum m; c = sum m x / M; the second
// moments about c, Q = sum m (x - c)(x - c)^T, a parent's from its children by the parallel-axis rule Q_c + M_c (c_c - c)(c_c - c)^T;
// sum m eps^2; the bounding box of ALL members; the range of eps^2 over the members with mass.  The float64 sums stay in the node's
// build record (a parent is formed from them, not from rounded values); what the walk reads is rounded once to float32:
// (c, M), e2 = sum m eps^2 / M, Q, and
//     b    = the distance from the float32 c to the farthest corner of the box, formed in float64, rounded to float32 and
//            multiplied by 1 + 2^-20: never below the true distance to any member (the rounding and the product err by 2^-23);
//     rule = 8 (e2_max - e2_min) - e2_min, multiplied by 1 + 2^-20 where positive.
// A node with M = 0 is stored as zeros; it is never accepted, opened or evaluated.
//
// The walk (tree_walk_kernel): one wave (a workgroup of 64 lanes) per group of 64 targets, a lane per target; targets = sources:
// 64 consecutive sorted particles; separate targets: 64 consecutive targets of the caller's order (correct in any order; the
// pruning is as good as the group's box is small).  The group's box is the bounding box of its valid targets, dmin the distance
// from it to a node's c, formed per axis as max(lo - c, c - hi, 0).  A node with mass is ACCEPTED iff
//     dmin^2 theta^2 > b^2   and   dmin^2 >= rule
// in float32; otherwise it is OPENED.  The float32 test errs by less than 10 * 2^-24 relative, b^2 is 2^-19 above the true
// radius squared, so a node that holds a target of the group (dmin <= |c - t| <= true radius) is opened for every theta <= 1: the
// self pair only arises in a leaf.  The second rule is the extra opening rule for softening lengths that vary inside a node: the
// monopole formed with the mean e2 differs from the members' own by about (3/8) var(eps^2) / (r^2 + e2)^2 relative, which the
// rule holds below (3/32) / 64 = 1.5e-3; where every member with mass has the same eps it is always met.
//   Pending lists: per level l >= 1 an LDS list of opened nodes of that level whose children are not yet tested.  A step takes up
// to 8 nodes from the lowest level that has any and tests their up to 64 children, a lane each; accepted children go to the node
// list, opened leaves to the leaf list, opened inner nodes to the pending list of their level, each compacted by ballot and a
// prefix count of the mask, in lane order.  CAPACITY (the proof is at PENDING_PER_LEVEL in tsp_gravity_tree_layout.h): when a
// step takes from level l every list below is empty, so a list receives at most 64 entries while it is empty and nothing until it
// is empty again: 64 entries per level, 9 levels (n < 2^31: at most 2^26 leaves, 10 levels with the leaves'), 2304 bytes per
// wave, for every input.  The nine counts (0 .. 64) are 7-bit fields of one 64-bit scalar.  The node and leaf lists hold 128
// entries each and are evaluated and emptied before any step that finds fewer than 64 slots free in one of them.
//   Evaluation: 64 listed nodes at a time are staged in LDS by the lanes (three float4 each) and read back by every lane at a
// wave-uniform address (a broadcast ds_read_b128, as gravity_tile reads its sources): with d = t - c, r2 = fma(dx, dx, fma(dy,
// dy, fma(dz, dz, e2))), inv = v_rsq_f32(r2), inv2 = inv inv, u = d inv, Qu = Q u, s = u . Qu, T = tr Q,
//     pot term  inv (M + inv2 (1.5 s - 0.5 T)),     acc term  inv2 ((M + inv2 (7.5 s - 1.5 T)) u - 3 inv2 Qu)
// (the softened monopole plus quadrupole: the expansion of sum m (|d - x|^2 + e2)^(-1/2) to second order in x; every factor stays
// of the order of the monopole's, nothing like r^-7 is formed).  Leaves are staged two at a time (64 particles) and summed with
// the pair arithmetic of gravity_tile, its CHECK form (r2 below 2^-126 or the target's own index: nothing) in the batches that
// hold the group's own leaves or an eps^2 below 2^-100.  Terms are added in float32 runs of 16 and the runs in float64.
// Determinism: list orders and batch boundaries are functions of the data alone; no floating-point atomics; the pair counts are
// integer atomics.  A target's value may depend on which targets share its group (their box decides what is opened).
//
// Rounding (u = 2^-24).  A pair term: as tsp_gravity.hip, 6u (potential) and 19u (acceleration); runs of 16 add 15u, the float64
// additions less than 4u: 25u and 38u, TSP_GRAVITY_TREE_ERROR_K = 64 as there; with theta = 0 every term is a pair term and the
// bound holds against the direct sum.  A node term: inv within 5u, inv2 11u, u 7u; where Q = 0 (a node whose mass is one
// particle's: c is that particle exactly, since (m x) / m is exact in float64 for float32 m and x, and e2 its eps^2) the potential
// term is M inv within 6u and the acceleration term inv2 (M u) within 20u: the single-source bound of the header, 32u.  In general
// c is the float32 of the float64 centre of mass, an absolute error of u |c| per coordinate, which the term sees as a relative
// error of u |c| / r in d (a pair's d has u |d|): sources far from the origin relative to their separation should be centred by
// the caller (topsy_amd.rotation_curve does).  M, e2 and Q carry one rounding each; the quadrupole part is at most theta^2 of the
// monopole, so the rounding of Q and the about 20 operations on it stay below 25u theta^2 of the term.  These are roundings of
// the terms evaluated; the truncation error of the expansion is measured in DESIGN.md section 4, not bounded here.
//
// Resources as built and measured rates: DESIGN.md section 4.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <type_traits>
#include <vector>

#include "tsp_gravity_tree_layout.h"
#include "tsp_internal.h"
#include "tsp_morton.h"

namespace tsp {
namespace {

using namespace tree;

static_assert(LEAF == TSP_GRAVITY_TREE_LEAF && FANOUT == TSP_GRAVITY_TREE_FANOUT, "the header's constants");
static_assert(WAVE == 2 * LEAF, "a batch of particles is two leaves, a lane each");
constexpr int RUN = 16;                              // consecutive terms summed in float32
constexpr float R2_NORMAL = 1.17549435e-38f;         // 2^-126: below it a pair contributes nothing
constexpr float E2_UNCHECKED = 7.88860905e-31f;      // 2^-100: a batch whose eps^2 all reach it needs no r2 test
constexpr float ROUND_UP = 1.0f + 9.5367431640625e-7f;   // 1 + 2^-20
constexpr unsigned NO_LEAF = 0xffffffffu;

struct NodeArrays {
    float4 *cm;         // (cx, cy, cz, M)
    float2 *rule;       // (b, rule)
    float4 *q0;         // (e2, Qxx, Qyy, Qzz)
    float4 *q1;         // (Qxy, Qxz, Qyz, 0)
    double *sums;       // NODE_SUMS per node: M, c (3), Q (xx, yy, zz, xy, xz, yz), sum m eps^2, 0
    float *box;         // 8 per node: lo (3), hi (3), 0, 0
    float2 *e2range;    // (min, max) of eps^2 over the members with mass (+inf, -inf: none)
};

__global__ __launch_bounds__(256) void tree_gather_kernel(const float *__restrict__ sx, const float *__restrict__ sy,
                                                          const float *__restrict__ sz, const uint32_t *__restrict__ idx,
                                                          const float *__restrict__ raw_m, const float *__restrict__ raw_e,
                                                          int has_eps, float eps_all, int64_t nv, int64_t padded,
                                                          float4 *__restrict__ out4, float *__restrict__ out_e2,
                                                          unsigned long long *__restrict__ n_valid) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool valid = false;
    if (i < padded) {
        float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float e2 = 1.0f;
        if (i < nv) {
            const uint32_t j = idx[i];
            const float m = raw_m[j], e = has_eps ? raw_e[j] : eps_all;
            valid = isfinite(m) && isfinite(e);
            p = make_float4(sx[i], sy[i], sz[i], valid ? m : 0.0f);
            e2 = valid ? e * e : 1.0f;
        }
        out4[i] = p;
        out_e2[i] = e2;
    }
    const unsigned long long mask = __ballot(valid);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd(n_valid, (unsigned long long)__popcll(mask));
}

// the particles of the leaf that starts at sorted index j0 (the last leaf may be partial)
__device__ __forceinline__ int members_of(int64_t nv, int64_t j0) { return nv - j0 < LEAF ? (int)(nv - j0) : LEAF; }

// The records of node g from its float64 sums: s = (M, c, Q, sum m eps^2), the box of all members, the eps^2 range of the massive.
__device__ __forceinline__ void store_node(const NodeArrays &na, uint32_t g, const double (&s)[NODE_SUMS], const float (&lo)[3],
                                           const float (&hi)[3], float e2min, float e2max) {
#pragma unroll
    for (int k = 0; k < NODE_SUMS; ++k) na.sums[(size_t)g * NODE_SUMS + k] = s[k];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        na.box[(size_t)g * 8 + a] = lo[a];
        na.box[(size_t)g * 8 + 3 + a] = hi[a];
    }
    na.box[(size_t)g * 8 + 6] = na.box[(size_t)g * 8 + 7] = 0.0f;
    na.e2range[g] = make_float2(e2min, e2max);
    const double M = s[0];
    if (!(M > 0.0)) {
        na.cm[g] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        na.rule[g] = make_float2(0.0f, 0.0f);
        na.q0[g] = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
        na.q1[g] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float c[3] = {(float)s[1], (float)s[2], (float)s[3]};
    double b2 = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double far = fmax((double)c[a] - (double)lo[a], (double)hi[a] - (double)c[a]);
        b2 += far * far;
    }
    const float b = (float)sqrt(b2) * ROUND_UP;
    const double r = 8.0 * ((double)e2max - (double)e2min) - (double)e2min;
    const float rule = r > 0.0 ? (float)r * ROUND_UP : 0.0f;
    na.cm[g] = make_float4(c[0], c[1], c[2], (float)M);
    na.rule[g] = make_float2(b, rule);
    na.q0[g] = make_float4((float)(s[10] / M), (float)s[4], (float)s[5], (float)s[6]);
    na.q1[g] = make_float4((float)s[7], (float)s[8], (float)s[9], 0.0f);
}

// a lane per leaf: the sums over its (at most LEAF) particles, in index order
__global__ __launch_bounds__(256) void tree_leaf_kernel(const float4 *__restrict__ src4, const float *__restrict__ src_e2, int64_t nv,
                                                        uint32_t n_leaves, NodeArrays na) {
    const uint32_t leaf = blockIdx.x * 256u + threadIdx.x;
    if (leaf >= n_leaves) return;
    const int64_t j0 = (int64_t)leaf * LEAF;
    const int members = members_of(nv, j0);
    double s[NODE_SUMS];
#pragma unroll
    for (int k = 0; k < NODE_SUMS; ++k) s[k] = 0.0;
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    float e2min = __builtin_inff(), e2max = -__builtin_inff();
    for (int k = 0; k < members; ++k) {
        const float4 p = src4[j0 + k];
        const float e2 = src_e2[j0 + k];
        const double m = p.w;
        s[0] += m;
        s[1] += m * (double)p.x;
        s[2] += m * (double)p.y;
        s[3] += m * (double)p.z;
        s[10] += m * (double)e2;
        lo[0] = fminf(lo[0], p.x), lo[1] = fminf(lo[1], p.y), lo[2] = fminf(lo[2], p.z);
        hi[0] = fmaxf(hi[0], p.x), hi[1] = fmaxf(hi[1], p.y), hi[2] = fmaxf(hi[2], p.z);
        if (p.w > 0.0f) e2min = fminf(e2min, e2), e2max = fmaxf(e2max, e2);
    }
    if (s[0] > 0.0) {
        s[1] /= s[0], s[2] /= s[0], s[3] /= s[0];
        for (int k = 0; k < members; ++k) {
            const float4 p = src4[j0 + k];
            const double m = p.w, dx = (double)p.x - s[1], dy = (double)p.y - s[2], dz = (double)p.z - s[3];
            s[4] += m * dx * dx, s[5] += m * dy * dy, s[6] += m * dz * dz;
            s[7] += m * dx * dy, s[8] += m * dx * dz, s[9] += m * dy * dz;
        }
    }
    store_node(na, leaf, s, lo, hi, e2min, e2max);
}

// a lane per node of one level: the sums over its (at most FANOUT) children, in index order
__global__ __launch_bounds__(256) void tree_level_kernel(uint32_t first, uint32_t count, uint32_t child_first, uint32_t child_count,
                                                         NodeArrays na) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= count) return;
    const uint32_t c0 = k * FANOUT, c1 = min(c0 + FANOUT, child_count);
    double s[NODE_SUMS];
#pragma unroll
    for (int q = 0; q < NODE_SUMS; ++q) s[q] = 0.0;
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    float e2min = __builtin_inff(), e2max = -__builtin_inff();
    for (uint32_t c = c0; c < c1; ++c) {
        const size_t g = (size_t)child_first + c;
        const double *cs = na.sums + g * NODE_SUMS;
        const double m = cs[0];
        s[0] += m;
        s[1] += m * cs[1], s[2] += m * cs[2], s[3] += m * cs[3];
        s[10] += cs[10];
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], na.box[g * 8 + a]);
            hi[a] = fmaxf(hi[a], na.box[g * 8 + 3 + a]);
        }
        const float2 er = na.e2range[g];
        e2min = fminf(e2min, er.x), e2max = fmaxf(e2max, er.y);
    }
    if (s[0] > 0.0) {
        s[1] /= s[0], s[2] /= s[0], s[3] /= s[0];
        for (uint32_t c = c0; c < c1; ++c) {
            const double *cs = na.sums + ((size_t)child_first + c) * NODE_SUMS;
            const double m = cs[0];
            if (!(m > 0.0)) continue;
            const double dx = cs[1] - s[1], dy = cs[2] - s[2], dz = cs[3] - s[3];
            s[4] += cs[4] + m * dx * dx, s[5] += cs[5] + m * dy * dy, s[6] += cs[6] + m * dz * dz;
            s[7] += cs[7] + m * dx * dy, s[8] += cs[8] + m * dx * dz, s[9] += cs[9] + m * dy * dz;
        }
    }
    store_node(na, first + k, s, lo, hi, e2min, e2max);
}

struct WalkArgs {
    const float4 *node_cm;
    const float2 *node_rule;
    const float4 *node_q0, *node_q1;
    const float4 *src4;              // the sorted particles, padded to whole leaves
    const float *src_e2;
    int64_t nv;
    const float *tx, *ty, *tz;       // separate targets (SELF: unused, the targets are src4)
    int64_t n_tgt;                   // targets of the walk (SELF: nv)
    float theta2;
    double *walk_out;                // SELF: the sums in the walk's order, plane c at walk_out + c nv (signs not yet changed)
    double *pot, *acc;               // separate targets: the results in the caller's order
    unsigned long long *counters;    // [1] valid targets, [2] pairs_direct, [3] pairs_node
    Levels lv;
};

template <bool ACC, bool SELF>
__global__ __launch_bounds__(64) void tree_walk_kernel(const WalkArgs a) {
    constexpr int NC = ACC ? 4 : 1;
    __shared__ uint32_t pend[PENDING_LEVELS][PENDING_PER_LEVEL];
    __shared__ uint32_t nlist[LIST_SLOTS], llist[LIST_SLOTS];
    __shared__ float4 stage[3][WAVE];
    const int lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int64_t i = (int64_t)blockIdx.x * WAVE + lane;
    const bool in = i < a.n_tgt;
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (in) {
        if (SELF) {
            const float4 p = a.src4[i];
            px = p.x, py = p.y, pz = p.z;
        } else {
            px = a.tx[i], py = a.ty[i], pz = a.tz[i];
        }
    }
    const bool valid = in && finite3(px, py, pz);
    const unsigned long long vmask = __ballot(valid);
    const unsigned ti = SELF ? (unsigned)i : NO_LEAF;      // the target's own index among the sorted sources
    double sum[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) sum[c] = 0.0;
    unsigned long long n_direct = 0, n_node = 0;           // per lane

    if (vmask) {      // (uniform)
        float lo[3] = {valid ? px : __builtin_inff(), valid ? py : __builtin_inff(), valid ? pz : __builtin_inff()};
        float hi[3] = {valid ? px : -__builtin_inff(), valid ? py : -__builtin_inff(), valid ? pz : -__builtin_inff()};
#pragma unroll
        for (int k = 0; k < 3; ++k)
            for (int off = 32; off; off >>= 1) {
                lo[k] = fminf(lo[k], __shfl_xor(lo[k], off));
                hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], off));
            }
        int nn = 0, nl = 0;                  // entries of the node and leaf lists (uniform)
        unsigned long long packed = 0;       // the counts of the pending lists, 7 bits per level 1 .. 9 (uniform)

        // one candidate per lane: accepted -> node list, opened -> leaf list (level 0) or the pending list of its level
        auto classify = [&](int level, uint32_t idx, bool present) {
            const uint32_t g = a.lv.first[level] + idx;
            float4 cm = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            float2 rl = make_float2(0.0f, 0.0f);
            if (present) {
                cm = a.node_cm[g];
                rl = a.node_rule[g];
            }
            const bool massive = present && cm.w > 0.0f;
            const float gx = fmaxf(fmaxf(lo[0] - cm.x, cm.x - hi[0]), 0.0f);
            const float gy = fmaxf(fmaxf(lo[1] - cm.y, cm.y - hi[1]), 0.0f);
            const float gz = fmaxf(fmaxf(lo[2] - cm.z, cm.z - hi[2]), 0.0f);
            const float d2 = (gx * gx + gy * gy) + gz * gz;
            const bool accept = massive && d2 * a.theta2 > rl.x * rl.x && d2 >= rl.y;
            const bool open = massive && !accept;
            const unsigned long long am = __ballot(accept), om = __ballot(open);
            if (accept) nlist[nn + __popcll(am & below)] = g;
            nn += __popcll(am);
            if (level == 0) {
                if (open) llist[nl + __popcll(om & below)] = idx;
                nl += __popcll(om);
            } else {
                const int shift = PENDING_COUNT_BITS * (level - 1);
                const int have = (int)((packed >> shift) & 127ull);
                if (open) pend[level - 1][have + __popcll(om & below)] = idx;
                packed += (unsigned long long)__popcll(om) << shift;
            }
        };

        auto eval_nodes = [&]() {
            for (int b0 = 0; b0 < nn; b0 += WAVE) {
                const int m = min(WAVE, nn - b0);
                if (lane < m) {
                    const uint32_t g = nlist[b0 + lane];
                    stage[0][lane] = a.node_cm[g];
                    stage[1][lane] = a.node_q0[g];
                    stage[2][lane] = a.node_q1[g];
                }
                __syncthreads();
                for (int k0 = 0; k0 < m; k0 += RUN) {
                    const int kend = min(k0 + RUN, m);
                    float f[NC];
#pragma unroll
                    for (int c = 0; c < NC; ++c) f[c] = 0.0f;
                    for (int k = k0; k < kend; ++k) {
                        const float4 cm = stage[0][k], q0 = stage[1][k], q1 = stage[2][k];
                        const float dx = px - cm.x, dy = py - cm.y, dz = pz - cm.z;
                        const float r2 = __builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, __builtin_fmaf(dz, dz, q0.x)));
                        const float inv = __builtin_amdgcn_rsqf(r2);
                        const float inv2 = inv * inv;
                        const float ux = dx * inv, uy = dy * inv, uz = dz * inv;
                        const float qux = __builtin_fmaf(q0.y, ux, __builtin_fmaf(q1.x, uy, q1.y * uz));
                        const float quy = __builtin_fmaf(q1.x, ux, __builtin_fmaf(q0.z, uy, q1.z * uz));
                        const float quz = __builtin_fmaf(q1.y, ux, __builtin_fmaf(q1.z, uy, q0.w * uz));
                        const float s = __builtin_fmaf(ux, qux, __builtin_fmaf(uy, quy, uz * quz));
                        const float T = (q0.y + q0.z) + q0.w;
                        f[0] += inv * __builtin_fmaf(inv2, __builtin_fmaf(1.5f, s, -0.5f * T), cm.w);
                        if constexpr (ACC) {
                            const float w = __builtin_fmaf(inv2, __builtin_fmaf(7.5f, s, -1.5f * T), cm.w);
                            const float w3 = -3.0f * inv2;
                            f[1] += inv2 * __builtin_fmaf(w, ux, w3 * qux);
                            f[2] += inv2 * __builtin_fmaf(w, uy, w3 * quy);
                            f[3] += inv2 * __builtin_fmaf(w, uz, w3 * quz);
                        }
                    }
#pragma unroll
                    for (int c = 0; c < NC; ++c) sum[c] += (double)f[c];
                }
                if (valid) n_node += (unsigned long long)m;
                __syncthreads();
            }
            nn = 0;
        };

        // the pairs of one staged batch (two leaves, 64 particles; padding: massless) with this lane's target
        auto batch_pairs = [&](auto check_tag, unsigned base_a, unsigned base_b) {
            constexpr bool CHECK = decltype(check_tag)::value;
            const float *se2 = reinterpret_cast<const float *>(stage[1]);
            for (int k0 = 0; k0 < WAVE; k0 += RUN) {
                float f[NC];
#pragma unroll
                for (int c = 0; c < NC; ++c) f[c] = 0.0f;
#pragma unroll
                for (int kk = 0; kk < RUN; ++kk) {
                    const int k = k0 + kk;
                    const float4 s = stage[0][k];
                    const float e2 = se2[k];
                    const float dx = px - s.x, dy = py - s.y, dz = pz - s.z;
                    const float r2 = __builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, __builtin_fmaf(dz, dz, e2)));
                    float inv = __builtin_amdgcn_rsqf(r2);
                    if constexpr (CHECK) {
                        const unsigned j = (k < LEAF ? base_a : base_b) + (unsigned)(k & (LEAF - 1));
                        inv = (r2 >= R2_NORMAL && ti != j) ? inv : 0.0f;
                    }
                    const float p = s.w * inv;
                    f[0] += p;
                    if constexpr (ACC) {
                        const float w = p * (inv * inv);
                        f[1] = __builtin_fmaf(w, dx, f[1]);
                        f[2] = __builtin_fmaf(w, dy, f[2]);
                        f[3] = __builtin_fmaf(w, dz, f[3]);
                    }
                }
#pragma unroll
                for (int c = 0; c < NC; ++c) sum[c] += (double)f[c];
            }
        };

        auto eval_leaves = [&]() {
            for (int b0 = 0; b0 < nl; b0 += 2) {
                const bool two = b0 + 1 < nl;
                const uint32_t leaf_a = (uint32_t)__builtin_amdgcn_readfirstlane((int)llist[b0]);
                const uint32_t leaf_b = two ? (uint32_t)__builtin_amdgcn_readfirstlane((int)llist[b0 + 1]) : NO_LEAF;
                const bool has = lane < LEAF || two;
                const int64_t j = (int64_t)(lane < LEAF ? leaf_a : leaf_b) * LEAF + (lane & (LEAF - 1));     // (< the padded count)
                const float4 s = has ? a.src4[j] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                const float e2 = has ? a.src_e2[j] : 1.0f;
                stage[0][lane] = s;
                reinterpret_cast<float *>(stage[1])[lane] = e2;
                const bool tiny = __ballot(!(e2 >= E2_UNCHECKED)) != 0;
                const uint32_t own = (uint32_t)blockIdx.x * 2u;      // SELF: the group's targets are leaves own and own + 1
                const bool mine = SELF && (leaf_a - own < 2u || (two && leaf_b - own < 2u));
                __syncthreads();
                const unsigned base_a = leaf_a * LEAF, base_b = two ? leaf_b * LEAF : 0xffffff00u;
                if (tiny || mine)
                    batch_pairs(std::true_type(), base_a, base_b);
                else
                    batch_pairs(std::false_type(), base_a, base_b);
                if (valid) {
                    const int members = members_of(a.nv, (int64_t)base_a) + (two ? members_of(a.nv, (int64_t)base_b) : 0);
                    const bool self_hit = SELF && ((uint32_t)(i >> 5) == leaf_a || (two && (uint32_t)(i >> 5) == leaf_b));
                    n_direct += (unsigned long long)(members - (self_hit ? 1 : 0));
                }
                __syncthreads();
            }
            nl = 0;
        };

        const int top = a.lv.n_levels - 1;
        classify(top, 0u, lane == 0);
        __syncthreads();
        for (;;) {
            if (nn > LIST_SLOTS - WAVE) eval_nodes();
            if (nl > LIST_SLOTS - WAVE) eval_leaves();
            if (!packed) break;
            const int level = __builtin_ctzll(packed) / PENDING_COUNT_BITS + 1;      // the lowest level with pending nodes
            const int shift = PENDING_COUNT_BITS * (level - 1);
            const int have = (int)((packed >> shift) & 127ull);
            const int take = min(have, WAVE / FANOUT);
            packed -= (unsigned long long)take << shift;
            const int slot = lane / FANOUT;
            bool present = slot < take;
            const uint32_t parent = present ? pend[level - 1][have - take + slot] : 0u;
            const uint32_t child = parent * FANOUT + (uint32_t)(lane % FANOUT);
            present = present && child < a.lv.count[level - 1];
            __syncthreads();
            classify(level - 1, child, present);
            __syncthreads();
        }
        eval_nodes();
        eval_leaves();
    }

    if (in) {
        if (SELF) {
#pragma unroll
            for (int c = 0; c < NC; ++c) a.walk_out[(size_t)c * (size_t)a.nv + (size_t)i] = sum[c];
        } else {
            if (a.pot) a.pot[i] = valid ? 0.0 - sum[0] : (double)NAN;
            if constexpr (ACC) {
#pragma unroll
                for (int c = 1; c < NC; ++c) a.acc[(size_t)3 * i + (c - 1)] = valid ? 0.0 - sum[c] : (double)NAN;
            }
        }
    }
    for (int off = 32; off; off >>= 1) {
        n_direct += __shfl_xor(n_direct, off);
        n_node += __shfl_xor(n_node, off);
    }
    if (lane == 0 && vmask) {
        atomicAdd(&a.counters[1], (unsigned long long)__popcll(vmask));
        if (n_direct) atomicAdd(&a.counters[2], n_direct);
        if (n_node) atomicAdd(&a.counters[3], n_node);
    }
}

// targets = sources: the walk's sums (sorted order, nv of them) into the caller's order with the signs changed; the sources
// without finite coordinates (the tail of the sort's index) get NaN
__global__ __launch_bounds__(256) void tree_scatter_kernel(const double *__restrict__ walk_out, const uint32_t *__restrict__ idx,
                                                           int64_t n, int64_t nv, int nc, double *__restrict__ pot,
                                                           double *__restrict__ acc) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t dst = idx[i];
    pot[dst] = i < nv ? 0.0 - walk_out[i] : (double)NAN;
    for (int c = 1; c < nc; ++c) acc[3 * dst + (c - 1)] = i < nv ? 0.0 - walk_out[(size_t)c * (size_t)nv + (size_t)i] : (double)NAN;
}

}  // namespace

// The host side of tsp_gravity_tree (the arguments are checked by the entry point).  Device memory: the index (its own sites) and
// the two buffers of gather_scratch(), carved by tsp_gravity_tree_layout.h: carve().
int gravity_tree(tsp_context *ctx, int64_t n_src, const float *sx, const float *sy, const float *sz, const float *mass,
                 const float *eps, float eps_all, int64_t n_tgt, const float *tx, const float *ty, const float *tz, float theta,
                 double *pot_out, double *acc_out, tsp_gravity_tree_info *info_out) {
    hipStream_t st = ctx->stream;
    // measurement aid: TOPSY_GRAVITY_STATS=1 reports the sizes, the pair counts and the times of the index, the tree and the walk
    const char *env = getenv("TOPSY_GRAVITY_STATS");
    const bool stats = env && env[0] == '1';
    const bool self = tx == nullptr;
    const bool want_acc = acc_out != nullptr;
    const int nc = want_acc ? 4 : 1;

    const auto t_index = std::chrono::steady_clock::now();
    MortonIndex ix;
    const int rc = build_morton_index(ctx, "tsp_gravity_tree", n_src, sx, sy, sz, 0.0f, 0, ix);
    if (rc != TSP_OK) return rc;
    const int64_t nv = ix.nv;
    TSP_REQUIRE(nv > 0, TSP_EINVAL, "tsp_gravity_tree: no source has finite coordinates");
    if (stats) TSP_HIP(hipStreamSynchronize(st));
    const double index_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_index).count();

    const Levels lv = levels_of(nv);
    const Carve cv = carve(n_src, nv, lv.n_nodes, n_tgt, self);
    DeviceScratch dh, da;
    const int rc_scratch = gather_scratch(ctx, dh, cv.h_bytes, da, cv.a_bytes);
    if (rc_scratch != TSP_OK) return rc_scratch;
    char *h = dh.as<char>(), *b = da.as<char>();
    float *raw_m = reinterpret_cast<float *>(h + cv.h_mass), *raw_e = reinterpret_cast<float *>(h + cv.h_eps);
    float4 *src4 = reinterpret_cast<float4 *>(h + cv.h_sorted4);
    float *src_e2 = reinterpret_cast<float *>(h + cv.h_sorted_e2);
    NodeArrays na;
    na.cm = reinterpret_cast<float4 *>(b + cv.a_node_cm);
    na.rule = reinterpret_cast<float2 *>(b + cv.a_node_rule);
    na.q0 = reinterpret_cast<float4 *>(b + cv.a_node_q0);
    na.q1 = reinterpret_cast<float4 *>(b + cv.a_node_q1);
    na.sums = reinterpret_cast<double *>(b + cv.a_node_sums);
    na.box = reinterpret_cast<float *>(b + cv.a_node_box);
    na.e2range = reinterpret_cast<float2 *>(b + cv.a_node_e2range);
    double *d_walk = reinterpret_cast<double *>(b + cv.a_walk);
    double *d_pot = reinterpret_cast<double *>(b + cv.a_out), *d_acc = d_pot + n_tgt;
    unsigned long long *d_counters = reinterpret_cast<unsigned long long *>(b + cv.a_counters);
    const size_t tgt_bytes = (size_t)n_tgt * sizeof(float);
    float *tplane[3] = {nullptr, nullptr, nullptr};
    if (!self)
        for (int k = 0; k < 3; ++k) tplane[k] = reinterpret_cast<float *>(b + cv.a_targets + k * align16(tgt_bytes));

    TSP_HIP(hipMemcpyAsync(raw_m, mass, (size_t)n_src * sizeof(float), hipMemcpyHostToDevice, st));
    if (eps) TSP_HIP(hipMemcpyAsync(raw_e, eps, (size_t)n_src * sizeof(float), hipMemcpyHostToDevice, st));
    const float *host_tgt[3] = {tx, ty, tz};
    if (!self)
        for (int k = 0; k < 3; ++k) TSP_HIP(hipMemcpyAsync(tplane[k], host_tgt[k], tgt_bytes, hipMemcpyHostToDevice, st));
    TSP_HIP(hipMemsetAsync(d_counters, 0, N_COUNTERS * sizeof(unsigned long long), st));

    // the tree
    if (stats) TSP_HIP(hipEventRecord(ctx->ev[EV_T0], st));
    hipLaunchKernelGGL(tree_gather_kernel, dim3((unsigned)((cv.padded + 255) / 256)), dim3(256), 0, st, ix.sx.as<float>(),
                       ix.sy.as<float>(), ix.sz.as<float>(), ix.vals2.as<uint32_t>(), raw_m, raw_e, eps ? 1 : 0, eps_all, nv, cv.padded,
                       src4, src_e2, d_counters);
    TSP_HIP(hipGetLastError());
    hipLaunchKernelGGL(tree_leaf_kernel, dim3((lv.count[0] + 255u) / 256u), dim3(256), 0, st, src4, src_e2, nv, lv.count[0], na);
    TSP_HIP(hipGetLastError());
    for (int l = 1; l < lv.n_levels; ++l) {
        hipLaunchKernelGGL(tree_level_kernel, dim3((lv.count[l] + 255u) / 256u), dim3(256), 0, st, lv.first[l], lv.count[l],
                           lv.first[l - 1], lv.count[l - 1], na);
        TSP_HIP(hipGetLastError());
    }
    if (stats) TSP_HIP(hipEventRecord(ctx->ev[EV_T1], st));

    // the walk
    WalkArgs wa = {};
    wa.node_cm = na.cm, wa.node_rule = na.rule, wa.node_q0 = na.q0, wa.node_q1 = na.q1;
    wa.src4 = src4, wa.src_e2 = src_e2, wa.nv = nv;
    wa.tx = tplane[0], wa.ty = tplane[1], wa.tz = tplane[2];
    wa.n_tgt = self ? nv : n_tgt;
    wa.theta2 = theta * theta;
    wa.walk_out = d_walk, wa.pot = d_pot, wa.acc = d_acc;
    wa.counters = d_counters;
    wa.lv = lv;
    const dim3 walk_grid((unsigned)((wa.n_tgt + WAVE - 1) / WAVE));
    auto kernel = self ? (want_acc ? tree_walk_kernel<true, true> : tree_walk_kernel<false, true>)
                       : (want_acc ? tree_walk_kernel<true, false> : tree_walk_kernel<false, false>);
    hipLaunchKernelGGL(kernel, walk_grid, dim3(WAVE), 0, st, wa);
    TSP_HIP(hipGetLastError());
    if (self) {
        hipLaunchKernelGGL(tree_scatter_kernel, dim3((unsigned)((n_src + 255) / 256)), dim3(256), 0, st, d_walk, ix.vals2.as<uint32_t>(),
                           n_src, nv, nc, d_pot, d_acc);
        TSP_HIP(hipGetLastError());
    }
    if (stats) TSP_HIP(hipEventRecord(ctx->ev[EV_T2], st));

    std::vector<double> result((size_t)n_tgt * nc);
    unsigned long long counts[N_COUNTERS] = {0, 0, 0, 0};
    TSP_HIP(hipMemcpyAsync(result.data(), d_pot, result.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    TSP_HIP(hipMemcpyAsync(counts, d_counters, sizeof(counts), hipMemcpyDeviceToHost, st));
    TSP_HIP(hipStreamSynchronize(st));
    TSP_REQUIRE(counts[0] > 0, TSP_EINVAL, "tsp_gravity_tree: no source has finite coordinates, mass and softening length");
    float build_ms = 0.0f, walk_ms = 0.0f;
    if (stats) {
        TSP_HIP(hipEventElapsedTime(&build_ms, ctx->ev[EV_T0], ctx->ev[EV_T1]));
        TSP_HIP(hipEventElapsedTime(&walk_ms, ctx->ev[EV_T1], ctx->ev[EV_T2]));
    }

    if (pot_out) memcpy(pot_out, result.data(), (size_t)n_tgt * sizeof(double));
    if (acc_out) memcpy(acc_out, result.data() + n_tgt, (size_t)3 * n_tgt * sizeof(double));
    if (info_out) {
        info_out->n_valid_sources = (int64_t)counts[0];
        info_out->n_valid_targets = (int64_t)counts[1];
        info_out->n_nodes = lv.n_nodes;
        info_out->n_levels = lv.n_levels;
        info_out->pairs_direct = (int64_t)counts[2];
        info_out->pairs_node = (int64_t)counts[3];
    }
    if (stats)
        fprintf(stderr,
                "tsp_gravity_tree: n_src=%lld valid=%llu n_tgt=%lld valid_tgt=%llu acc=%d theta=%.4f nodes=%lld levels=%d pairs_direct=%llu "
                "pairs_node=%llu index_ms=%.4f build_ms=%.4f kernel_ms=%.4f\n",
                (long long)n_src, counts[0], (long long)n_tgt, counts[1], (int)want_acc, (double)theta, (long long)lv.n_nodes, lv.n_levels,
                counts[2], counts[3], index_ms, (double)build_ms, (double)walk_ms);
    return TSP_OK;
}

}  // namespace tsp
