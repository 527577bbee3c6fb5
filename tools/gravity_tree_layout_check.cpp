// Stand-alone host check of topsy_amd/csrc/tsp_gravity_tree_layout.h (no GPU, no HIP): the level sizes, the pending-list
// capacity and the carving offsets of tsp_gravity_tree, meant to be built with the sanitizers and run on the CPU:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I topsy_amd/csrc \
//         tools/gravity_tree_layout_check.cpp -o gravity_tree_layout_check && ./gravity_tree_layout_check
// It also replays the walk's list discipline on the host (every node opened, the worst case for the pending lists) with real
// arrays of the capacity the kernel has, so that an overflow is an out-of-bounds write the address sanitizer reports.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "tsp_gravity_tree_layout.h"

using namespace tsp::tree;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

static void check_levels(int64_t nv) {
    const Levels lv = levels_of(nv);
    CHECK(lv.n_levels >= 1 && lv.n_levels <= MAX_LEVELS);
    CHECK((int64_t)lv.count[0] == (nv + LEAF - 1) / LEAF);
    CHECK(lv.count[lv.n_levels - 1] == 1);
    int64_t first = 0;
    for (int l = 0; l < lv.n_levels; ++l) {
        CHECK(lv.first[l] == first);
        if (l) CHECK(lv.count[l] == (lv.count[l - 1] + FANOUT - 1) / FANOUT && lv.count[l - 1] > 1);
        first += lv.count[l];
    }
    CHECK(lv.n_nodes == first);
}

static void check_carve(int64_t n_src, int64_t nv, int64_t n_tgt, bool self) {
    const Levels lv = levels_of(nv);
    const Carve c = carve(n_src, nv, lv.n_nodes, n_tgt, self);
    const size_t nn = (size_t)lv.n_nodes;
    // every region starts 16-byte aligned, regions do not overlap, and the last one ends inside the buffer
    const size_t h_off[] = {c.h_mass, c.h_eps, c.h_sorted4, c.h_sorted_e2, c.h_bytes};
    const size_t h_len[] = {(size_t)n_src * 4, (size_t)n_src * 4, (size_t)c.padded * 16, (size_t)c.padded * 4};
    for (int k = 0; k < 4; ++k) CHECK(h_off[k] % 16 == 0 && h_off[k] + h_len[k] <= h_off[k + 1]);
    const size_t a_off[] = {c.a_node_cm, c.a_node_rule, c.a_node_q0, c.a_node_q1, c.a_node_sums, c.a_node_box, c.a_node_e2range,
                            c.a_walk, c.a_out, c.a_targets, c.a_counters, c.a_bytes};
    const size_t a_len[] = {nn * 16, nn * 8, nn * 16, nn * 16, nn * NODE_SUMS * 8, nn * 32, nn * 8, self ? (size_t)nv * 32 : 0,
                            (size_t)n_tgt * 32, self ? 0 : 3 * align16((size_t)n_tgt * 4), N_COUNTERS * 8};
    for (int k = 0; k < 11; ++k) CHECK(a_off[k] % 16 == 0 && a_off[k] + a_len[k] <= a_off[k + 1]);
    CHECK(c.padded % LEAF == 0 && c.padded >= nv && c.padded - nv < LEAF);
}

// the walk's discipline with every node opened: the largest any pending list gets, and the steps taken
static int replay_walk(int64_t nv) {
    const Levels lv = levels_of(nv);
    std::vector<std::vector<uint32_t>> pend(PENDING_LEVELS, std::vector<uint32_t>(PENDING_PER_LEVEL));      // exact capacity
    std::vector<uint32_t> leaves(LIST_SLOTS);
    uint64_t packed = 0;
    int nl = 0, worst = 0;
    int64_t leaves_seen = 0;
    const int top = lv.n_levels - 1;
    if (top == 0) return 0;
    pend[top - 1][0] = 0;
    packed += 1ull << (PENDING_COUNT_BITS * (top - 1));
    while (true) {
        if (nl > LIST_SLOTS - WAVE) leaves_seen += nl, nl = 0;
        if (!packed) break;
        const int level = __builtin_ctzll(packed) / PENDING_COUNT_BITS + 1;
        const int shift = PENDING_COUNT_BITS * (level - 1);
        const int have = (int)((packed >> shift) & 127);
        const int take = have < WAVE / FANOUT ? have : WAVE / FANOUT;
        packed -= (uint64_t)take << shift;
        int opened = 0;
        for (int lane = 0; lane < WAVE; ++lane) {
            const int slot = lane / FANOUT;
            if (slot >= take) continue;
            const uint32_t child = pend[level - 1][have - take + slot] * FANOUT + lane % FANOUT;
            if (child >= lv.count[level - 1]) continue;
            if (level - 1 == 0) {
                leaves[nl + opened] = child;      // (the address sanitizer watches the bound)
            } else {
                const int below = (int)((packed >> (PENDING_COUNT_BITS * (level - 2))) & 127);
                CHECK(below + opened < PENDING_PER_LEVEL);
                pend[level - 2][below + opened] = child;
            }
            ++opened;
        }
        if (level - 1 == 0) {
            nl += opened;
        } else {
            packed += (uint64_t)opened << (PENDING_COUNT_BITS * (level - 2));
            const int now = (int)((packed >> (PENDING_COUNT_BITS * (level - 2))) & 127);
            worst = now > worst ? now : worst;
        }
    }
    leaves_seen += nl;
    CHECK(leaves_seen == (int64_t)lv.count[0]);      // every leaf is reached exactly once
    return worst;
}

int main() {
    const int64_t sizes[] = {1, 31, 32, 33, 255, 256, 257, 2048, 2049, 2055, 16384, 65536, 1000003, (1ll << 24) + 1,
                             (1ll << 31) - 33, (1ll << 31) - 32, (1ll << 31) - 1};
    for (int64_t nv : sizes) {
        check_levels(nv);
        check_carve(nv + 5, nv, 129, false);
        check_carve(nv, nv, nv, true);
    }
    CHECK(levels_of((1ll << 31) - 1).n_levels == MAX_LEVELS && levels_of(0).n_levels == 0 && levels_of(32).n_levels == 1 &&
          levels_of(33).n_levels == 2);
    int worst = 0;
    for (int64_t nv : {(int64_t)1, (int64_t)33, (int64_t)2055, (int64_t)65536, (int64_t)1000003, ((int64_t)1 << 22) + 77}) {
        const int w = replay_walk(nv);
        worst = w > worst ? w : worst;
    }
    CHECK(worst <= PENDING_PER_LEVEL);
    printf("gravity tree layout: levels, carving and pending lists hold (largest pending list %d of %d)\n", worst, PENDING_PER_LEVEL);
    return 0;
}
