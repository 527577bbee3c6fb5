// tsp_gravity_tree_layout.h -- the host arithmetic of tsp_gravity_tree that needs no device: the sizes of the tree's levels, the
// capacity of the walk's pending lists, and the offsets at which the call carves its two scratch buffers.  Plain C++ (no HIP), so
// that a stand-alone host program can exercise it under the address and undefined-behaviour sanitizers (tools/gravity_tree_layout_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace tsp {
namespace tree {

constexpr int LEAF = 32;           // TSP_GRAVITY_TREE_LEAF: sorted particles per leaf
constexpr int FANOUT = 8;          // TSP_GRAVITY_TREE_FANOUT: nodes of level l per node of level l + 1
constexpr int WAVE = 64;           // targets per group, lanes per wave
// Levels, the leaves' included: n < 2^31 particles are at most 2^26 leaves, and ceil(2^26 / 8^k) reaches 1 at k = 9: ten levels.
constexpr int MAX_LEVELS = 10;
// The walk keeps, per level l >= 1, a list of nodes of that level that were opened and whose children are not yet tested.  A step
// takes up to WAVE / FANOUT nodes from the LOWEST level that has any, and tests their children (at most WAVE, one per lane); the
// children that are opened go to the list of the level below.  When a step takes from level l, every list below l is empty (l is
// the lowest with entries), so the list of level l - 1 receives at most WAVE entries while it is empty, and receives nothing more
// until it is empty again (until then it is itself the lowest, or a list below it is).  The top list only ever holds the root.
// Hence no list ever holds more than WAVE = 64 entries, for any input, and the lists take PENDING_SLOTS entries in all.
constexpr int PENDING_PER_LEVEL = WAVE;
constexpr int PENDING_LEVELS = MAX_LEVELS - 1;                       // levels 1 .. 9 (the leaves are never pending)
constexpr int PENDING_SLOTS = PENDING_LEVELS * PENDING_PER_LEVEL;    // 576 entries of 4 bytes per wave
constexpr int PENDING_COUNT_BITS = 7;                                // a count 0 .. 64 per level, nine of them packed in 64 bits
static_assert((1 << PENDING_COUNT_BITS) > PENDING_PER_LEVEL && PENDING_LEVELS * PENDING_COUNT_BITS <= 64, "packed counts");
static_assert(WAVE % FANOUT == 0, "a step tests the children of WAVE / FANOUT nodes");
// The lists of accepted nodes and opened leaves: a step adds at most WAVE to either; they are evaluated and emptied before a step
// whenever fewer than WAVE slots are free.
constexpr int LIST_SLOTS = 2 * WAVE;

struct Levels {
    int n_levels;                     // 1 (one leaf is the root) .. MAX_LEVELS; 0 when there is no particle
    uint32_t count[MAX_LEVELS];       // nodes of level l (level 0: the leaves)
    uint32_t first[MAX_LEVELS];       // index of the level's first node in the node arrays (levels stored one after the other)
    int64_t n_nodes;
};

// nv sorted particles, 0 <= nv < 2^31
inline Levels levels_of(int64_t nv) {
    Levels lv = {};
    if (nv <= 0) return lv;
    int64_t c = (nv + LEAF - 1) / LEAF, first = 0;
    for (int l = 0; l < MAX_LEVELS; ++l) {
        lv.count[l] = (uint32_t)c;
        lv.first[l] = (uint32_t)first;
        first += c;
        lv.n_levels = l + 1;
        if (c == 1) break;
        c = (c + FANOUT - 1) / FANOUT;
    }
    lv.n_nodes = first;
    return lv;
}

inline size_t align16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

// The two buffers of the call (the sites of gather_scratch()), as byte offsets.
//   h: [raw mass: n_src floats][raw eps: n_src floats][sorted (x, y, z, m): nv float4, padded to whole leaves][sorted eps^2]
//   a: [node (c, M): float4][node (b, rule): float2][node (e2, Qxx, Qyy, Qzz): float4][node (Qxy, Qxz, Qyz, -): float4]
//      [node sums: 12 doubles][node boxes: 8 floats][node eps^2 range: float2][results in the order of the walk: 4 n_walk doubles]
//      [results in the caller's order: pot n_tgt, acc 3 n_tgt doubles][target planes: 3 n_tgt floats (separate targets)][counters]
struct Carve {
    size_t h_mass, h_eps, h_sorted4, h_sorted_e2, h_bytes;
    size_t a_node_cm, a_node_rule, a_node_q0, a_node_q1, a_node_sums, a_node_box, a_node_e2range, a_walk, a_out, a_targets,
           a_counters, a_bytes;
    int64_t padded;      // nv rounded up to whole leaves
};
constexpr int NODE_SUMS = 12;      // doubles per node: M, c (3), Q (xx, yy, zz, xy, xz, yz), sum m eps^2, unused
constexpr int N_COUNTERS = 4;      // valid sources, valid targets, pairs_direct, pairs_node

inline Carve carve(int64_t n_src, int64_t nv, int64_t n_nodes, int64_t n_tgt, bool self) {
    Carve c = {};
    c.padded = (nv + LEAF - 1) / LEAF * LEAF;
    size_t o = 0;
    c.h_mass = o, o += align16((size_t)n_src * 4);
    c.h_eps = o, o += align16((size_t)n_src * 4);
    c.h_sorted4 = o, o += (size_t)c.padded * 16;
    c.h_sorted_e2 = o, o += align16((size_t)c.padded * 4);
    c.h_bytes = o;
    const size_t nn = (size_t)n_nodes;
    o = 0;
    c.a_node_cm = o, o += nn * 16;
    c.a_node_rule = o, o += align16(nn * 8);
    c.a_node_q0 = o, o += nn * 16;
    c.a_node_q1 = o, o += nn * 16;
    c.a_node_sums = o, o += nn * NODE_SUMS * 8;
    c.a_node_box = o, o += nn * 32;
    c.a_node_e2range = o, o += align16(nn * 8);
    c.a_walk = o, o += self ? align16((size_t)nv * 4 * 8) : 0;
    c.a_out = o, o += align16((size_t)n_tgt * 4 * 8);
    c.a_targets = o, o += self ? 0 : 3 * align16((size_t)n_tgt * 4);
    c.a_counters = o, o += align16(N_COUNTERS * 8);
    c.a_bytes = o;
    return c;
}

}  // namespace tree
}  // namespace tsp
