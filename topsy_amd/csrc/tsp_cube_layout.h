// tsp_cube_layout.h -- the host arithmetic of tsp_spectral_cube that needs no device: the screen tiles and channel blocks, the
// slices the particles go through, the capacity of the (tile, block) lists and the offsets at which the call carves its two scratch
// buffers.  Plain C++ (no HIP), so that a stand-alone host program can exercise it under the address and undefined-behaviour
// sanitizers, and a test can drive it on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace tsp {
namespace cube {

constexpr int TILE = 16;                    // an image tile is TILE x TILE pixels: one pixel per thread of a 256-thread workgroup
constexpr int CHANNEL_BLOCK = 32;           // channels per block: TILE * TILE * CHANNEL_BLOCK float64 sums are 64 KB of LDS
constexpr int MAX_CHANNELS = 4096;
constexpr int64_t MAX_CELLS = 1ll << 31;    // n_channels * R * R at most
// The bound on list memory: a slice of particles emits at most LIST_CAPACITY (tile, block) pairs.  A particle emits at most one
// pair per bin (its footprint may cover every tile and its line every block), so a slice of LIST_CAPACITY / n_bins particles
// can never overflow the lists, whatever the data: the slice boundaries depend on (n, R, n_channels) and the option alone.
// A pair costs 16 bytes (key and index, each in and out of the sort): 2 GiB of lists at most.
constexpr int64_t LIST_CAPACITY = 1ll << 27;
// ... and on record memory: 48 bytes per particle of a slice (geometry 16, line 24, pair count and offset 8): 192 MiB at most.
constexpr int64_t MAX_SLICE_PARTICLES = 1ll << 22;
constexpr int RECORD_BYTES = 16 + 24;

struct Grid {
    int tiles;          // tiles per image side
    int blocks;         // channel blocks
    int64_t bins;       // tiles * tiles * blocks: bin = (ty * tiles + tx) * blocks + block
    int key_bits;       // bits of a bin index (what the sort compares), 1 at least
};

// 1 <= R, 1 <= n_channels <= MAX_CHANNELS, n_channels * R * R <= MAX_CELLS
inline Grid grid_of(int R, int n_channels) {
    Grid g = {};
    g.tiles = (R + TILE - 1) / TILE;
    g.blocks = (n_channels + CHANNEL_BLOCK - 1) / CHANNEL_BLOCK;
    g.bins = (int64_t)g.tiles * g.tiles * g.blocks;
    g.key_bits = 1;
    while (g.key_bits < 32 && (1ll << g.key_bits) < g.bins) ++g.key_bits;
    return g;
}

// Particles per slice: as many as can never overflow the lists, capped by the record bound and by n; option > 0 (tsp_set_option
// "cube_slice_particles") lowers it further.  At least 1 (n_bins <= 2^18 + ... < LIST_CAPACITY for every allowed R, n_channels).
inline int64_t slice_particles(int64_t n, int R, int n_channels, int64_t option) {
    const Grid g = grid_of(R, n_channels);
    int64_t s = LIST_CAPACITY / g.bins;
    if (s > MAX_SLICE_PARTICLES) s = MAX_SLICE_PARTICLES;
    if (option > 0 && option < s) s = option;
    if (s > n) s = n;
    if (s < 1) s = 1;
    return s;
}

inline int64_t slice_count(int64_t n, int64_t per_slice) { return n <= 0 ? 0 : (n + per_slice - 1) / per_slice; }

// slice k of slice_count(n, per_slice): the resident particles [first, first + count)
inline void slice_range(int64_t n, int64_t per_slice, int64_t k, int64_t *first, int64_t *count) {
    *first = k * per_slice;
    *count = n - *first < per_slice ? n - *first : per_slice;
    if (*count < 0) *count = 0;
}

// pairs a slice of `per_slice` particles can emit
inline int64_t list_capacity(int64_t per_slice, const Grid &g) {
    const int64_t worst = per_slice * g.bins;        // <= LIST_CAPACITY + bins by slice_particles(): no overflow
    return worst < LIST_CAPACITY ? worst : LIST_CAPACITY;
}

inline size_t align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// The two buffers of the call (the sites of gather_scratch()), as byte offsets.
//   h: [sigma in the caller's order: n floats (none when the call has no sigma)][geometry (pcx, pcy, P, w0): per_slice float4]
//      [line (s, u, c_lo, c_hi): per_slice x 24 bytes]
//   a: [the cube: n_channels * R * R floats][pairs per particle: per_slice + 1 uint32][first pair per particle: per_slice + 1]
//      [keys, keys sorted, indices, indices sorted: capacity uint32 each][first and end entry per bin: bins uint32 each]
//      [temporary storage of the scan and of the sort]
struct Carve {
    size_t h_sigma, h_geom, h_line, h_bytes;
    size_t a_cube, a_count, a_offset, a_keys, a_keys_sorted, a_index, a_index_sorted, a_bin_first, a_bin_end, a_tmp, a_bytes;
    int64_t capacity;       // pairs
};

inline Carve carve(int64_t n, int64_t per_slice, int R, int n_channels, bool has_sigma, size_t tmp_bytes) {
    const Grid g = grid_of(R, n_channels);
    Carve c = {};
    c.capacity = list_capacity(per_slice, g);
    size_t o = 0;
    c.h_sigma = o, o += has_sigma ? align256((size_t)n * 4) : 0;
    c.h_geom = o, o += align256((size_t)per_slice * 16);
    c.h_line = o, o += align256((size_t)per_slice * 24);
    c.h_bytes = o;
    o = 0;
    c.a_cube = o, o += align256((size_t)n_channels * R * R * 4);
    c.a_count = o, o += align256((size_t)(per_slice + 1) * 4);
    c.a_offset = o, o += align256((size_t)(per_slice + 1) * 4);
    const size_t list = align256((size_t)c.capacity * 4);
    c.a_keys = o, o += list;
    c.a_keys_sorted = o, o += list;
    c.a_index = o, o += list;
    c.a_index_sorted = o, o += list;
    c.a_bin_first = o, o += align256((size_t)g.bins * 4);
    c.a_bin_end = o, o += align256((size_t)g.bins * 4);
    c.a_tmp = o, o += align256(tmp_bytes);
    c.a_bytes = o;
    return c;
}

}  // namespace cube
}  // namespace tsp
