// tsp_hist2d_layout.h -- the host arithmetic of tsp_histogram_2d that needs no device: the bits of a cell index, the blocks of
// sorted entries and the levels its reduction takes, and the offsets at which the call carves its two scratch buffers.  Plain C++
// (no HIP), so that a stand-alone host program can exercise it under the address and undefined-behaviour sanitizers, and a test can
// drive it on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace tsp {
namespace hist2d {

constexpr int MAX_BINS = 1024;      // per axis
constexpr int BLOCK = 256;          // sorted entries a workgroup of the reduction takes: one per thread, 64 per wave
constexpr int MAX_LEVELS = 8;       // (2^31 entries need 5: every level leaves 2 records per block, 1 / 128 of its entries)

// the bits of a key: cells 0 .. cells - 1 and one value above them for the particles in no cell -- ceil(log2(cells + 1)), 1 .. 21
inline int key_bits(int64_t cells) {
    int b = 1;
    while ((1ll << b) < cells + 1) ++b;
    return b;
}

inline int64_t blocks_of(int64_t entries) { return (entries + BLOCK - 1) / BLOCK; }

// The reduction's levels: level 0 takes the n sorted particles, level k + 1 the two records every block of level k left (the run
// that reaches its left end and the one that reaches its right end); a level of one block leaves none and is the last.
struct Levels {
    int count;
    int64_t entries[MAX_LEVELS], blocks[MAX_LEVELS];
};

inline Levels levels_of(int64_t n) {
    Levels l = {};
    int64_t m = n < 1 ? 1 : n;
    while (l.count < MAX_LEVELS) {
        l.entries[l.count] = m;
        l.blocks[l.count] = blocks_of(m);
        ++l.count;
        if (blocks_of(m) == 1) break;
        m = 2 * blocks_of(m);
    }
    return l;
}

inline size_t align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

struct Region {
    size_t offset, bytes;       // bytes: what the call uses (the next region starts at the next multiple of 256)
};

// The two buffers of the call (the sites of gather_scratch()).
//   h: the caller's arrays: [x: n floats][y][w (none without weights)][v (none without values)]
//   a: [counts: cells int64][sums: (has_v ? 3 : 1) * cells float64][edges: nx + 1, then ny + 1 float64][counters: n_valid, n_binned]
//      [keys: n uint32 -- the cell of every particle, all ones for none: bin_out is a copy of it][keys sorted][indices][indices
//      sorted][records A: what levels 0, 2, .. leave][records B: what levels 1, 3, .. leave][temporary storage of the sort]
//   A record is (key uint32, count uint32, has_v ? 3 : 1 float64 sums), kept as one array per field: records_a / records_b are
//   the numbers of records, at 4 + 4 + 8 * planes bytes each.
struct Carve {
    Region h_x, h_y, h_w, h_v;
    size_t h_bytes;
    Region a_count, a_sums, a_edges, a_counters, a_keys, a_keys_sorted, a_index, a_index_sorted, a_records_a, a_records_b, a_tmp;
    size_t a_bytes;
    int64_t records_a, records_b;
    size_t bins_bytes;          // what goes back into bin_out: n int32, or nothing
};

inline size_t record_bytes(int64_t records, int planes) {      // key, count, then the planes: each array on a multiple of 256
    return records ? 2 * align256((size_t)records * 4) + (size_t)planes * align256((size_t)records * 8) : 0;
}

// 1 <= n < 2^31, 1 <= nx, ny <= MAX_BINS
inline Carve carve(int64_t n, int nx, int ny, bool has_w, bool has_v, bool want_bins, size_t tmp_bytes) {
    const size_t cells = (size_t)nx * (size_t)ny, planes = has_v ? 3 : 1, list = (size_t)n * 4;
    const Levels lv = levels_of(n);
    Carve c = {};
    c.records_a = lv.count > 1 ? lv.entries[1] : 0;
    c.records_b = lv.count > 2 ? lv.entries[2] : 0;
    c.bins_bytes = want_bins ? list : 0;
    size_t o = 0;
    auto take = [&o](Region &r, size_t bytes) { r.offset = o, r.bytes = bytes, o += align256(bytes); };
    take(c.h_x, list);
    take(c.h_y, list);
    take(c.h_w, has_w ? list : 0);
    take(c.h_v, has_v ? list : 0);
    c.h_bytes = o;
    o = 0;
    take(c.a_count, cells * 8);
    take(c.a_sums, planes * cells * 8);
    take(c.a_edges, (size_t)(nx + ny + 2) * 8);
    take(c.a_counters, 16);
    take(c.a_keys, list);
    take(c.a_keys_sorted, list);
    take(c.a_index, list);
    take(c.a_index_sorted, list);
    take(c.a_records_a, record_bytes(c.records_a, (int)planes));
    take(c.a_records_b, record_bytes(c.records_b, (int)planes));
    take(c.a_tmp, tmp_bytes);
    c.a_bytes = o;
    return c;
}

}  // namespace hist2d
}  // namespace tsp
