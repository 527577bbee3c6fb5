// Stand-alone host check of topsy_amd/csrc/tsp_hist2d_layout.h (no GPU, no HIP): the key bits, the levels of the reduction and
// the carving offsets of tsp_histogram_2d, meant to be built with the sanitizers and run on the CPU:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//         -I topsy_amd/csrc tools/hist2d_layout_check.cpp -o hist2d_layout_check && ./hist2d_layout_check
// (gcc's two -static-lib options put the runtimes into the program, as clang does by itself; tests/test_phase_cpu.py does this.)
// It also replays, level by level, the record slots the reduction's blocks write (2 b and 2 b + 1 of every block b of a level
// with more than one block) into arrays of exactly the capacity the call carves, so that a slot past a record buffer is an
// out-of-bounds write the address sanitizer reports.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "tsp_hist2d_layout.h"

using namespace tsp::hist2d;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

static void check_levels(int64_t n) {
    const Levels lv = levels_of(n);
    CHECK(lv.count >= 1 && lv.count <= MAX_LEVELS);
    CHECK(lv.entries[0] == n && lv.blocks[lv.count - 1] == 1);
    for (int k = 0; k < lv.count; ++k) {
        CHECK(lv.blocks[k] == (lv.entries[k] + BLOCK - 1) / BLOCK);
        if (k) CHECK(lv.entries[k] == 2 * lv.blocks[k - 1] && lv.blocks[k - 1] > 1 && lv.entries[k] < lv.entries[k - 1]);
    }
}

static void check_carve(int64_t n, int nx, int ny, bool has_w, bool has_v, bool want_bins, size_t tmp) {
    const Carve c = carve(n, nx, ny, has_w, has_v, want_bins, tmp);
    const Levels lv = levels_of(n);
    const size_t cells = (size_t)nx * ny, planes = has_v ? 3 : 1, list = (size_t)n * 4;
    const Region h[] = {c.h_x, c.h_y, c.h_w, c.h_v};
    const size_t h_len[] = {list, list, has_w ? list : 0, has_v ? list : 0};
    size_t end = 0;
    for (int k = 0; k < 4; ++k) {
        CHECK(h[k].offset % 16 == 0 && h[k].offset >= end && h[k].bytes == h_len[k]);
        end = h[k].offset + h[k].bytes;
    }
    CHECK(end <= c.h_bytes && c.h_bytes % 16 == 0);
    CHECK(c.records_a == (lv.count > 1 ? lv.entries[1] : 0) && c.records_b == (lv.count > 2 ? lv.entries[2] : 0));
    for (int k = 3; k < lv.count; ++k) CHECK(lv.entries[k] <= (k & 1 ? c.records_a : c.records_b));      // level k - 1 writes A if even
    const Region a[] = {c.a_count, c.a_sums, c.a_edges, c.a_counters, c.a_keys, c.a_keys_sorted, c.a_index, c.a_index_sorted,
                        c.a_records_a, c.a_records_b, c.a_tmp};
    const size_t a_len[] = {cells * 8, planes * cells * 8, (size_t)(nx + ny + 2) * 8, 16, list, list, list, list,
                            record_bytes(c.records_a, (int)planes), record_bytes(c.records_b, (int)planes), tmp};
    end = 0;
    for (int k = 0; k < 11; ++k) {
        CHECK(a[k].offset % 16 == 0 && a[k].offset >= end && a[k].bytes == a_len[k]);
        end = a[k].offset + a[k].bytes;
    }
    CHECK(end <= c.a_bytes && c.a_bytes % 16 == 0);
    // the five arrays of a record buffer lie inside it
    for (int64_t records : {c.records_a, c.records_b})
        CHECK(record_bytes(records, (int)planes) >= (size_t)records * (8 + 8 * planes));
    CHECK(c.bins_bytes == (want_bins ? list : 0));
    CHECK(key_bits((int64_t)cells) >= 1 && (1ll << key_bits((int64_t)cells)) >= (int64_t)cells + 1 &&
          (key_bits((int64_t)cells) == 1 || (1ll << (key_bits((int64_t)cells) - 1)) < (int64_t)cells + 1));
}

// every block of a level with more than one block writes its two records; level k writes buffer k & 1
static int64_t replay_records(int64_t n) {
    const Levels lv = levels_of(n);
    const Carve c = carve(n, 1, 1, false, false, false, 0);
    std::vector<unsigned char> buffer[2] = {std::vector<unsigned char>((size_t)c.records_a), std::vector<unsigned char>((size_t)c.records_b)};
    int64_t written = 0;
    for (int k = 0; k + 1 < lv.count; ++k) {
        std::vector<unsigned char> &out = buffer[k & 1];
        for (int64_t b = 0; b < lv.blocks[k]; ++b) {
            out.data()[2 * b] = 1, out.data()[2 * b + 1] = 1;       // (the address sanitizer watches the bound)
            written += 2;
        }
        for (int64_t e = 0; e < lv.entries[k + 1]; ++e) CHECK(out[(size_t)e] == 1);     // what the next level reads was written
        for (int64_t e = 0; e < lv.entries[k + 1]; ++e) out[(size_t)e] = 0;
    }
    return written;
}

int main() {
    const int64_t sizes[] = {1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 65536, 65537, 1000003, 10000000, (1ll << 24) + 1,
                             (1ll << 31) - 257, (1ll << 31) - 256, (1ll << 31) - 1};
    const int shapes[][2] = {{1, 1}, {1, 1024}, {1024, 1}, {3, 5}, {256, 256}, {1024, 1024}};
    for (int64_t n : sizes) {
        check_levels(n);
        for (const auto &s : shapes)
            for (int flags = 0; flags < 8; ++flags) check_carve(n, s[0], s[1], flags & 1, flags & 2, flags & 4, flags == 7 ? 12345 : 0);
    }
    CHECK(levels_of(256).count == 1 && levels_of(257).count == 2 && levels_of(1).count == 1 && levels_of((1ll << 31) - 1).count == 5);
    CHECK(key_bits(1) == 1 && key_bits(3) == 2 && key_bits(4) == 3 && key_bits(1024 * 1024) == 21);
    int64_t written = 0;
    for (int64_t n : {(int64_t)1, (int64_t)257, (int64_t)65537, (int64_t)1000003, ((int64_t)1 << 26) + 77}) written += replay_records(n);
    printf("hist2d layout: levels, carving and record slots hold (%lld record slots replayed)\n", (long long)written);
    return 0;
}
