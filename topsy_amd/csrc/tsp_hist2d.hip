// tsp_hist2d.hip -- phase diagrams (tsp_histogram_2d, include/topsy_splat.h "Weighted 2-D histograms"): per cell of an nx x ny table
// the number of particles whose (x, y) fall into it and the float64 sums of w, w v and (w v) v.
//
// A table of up to 1024 x 1024 cells of four 8-byte words fits no LDS, and most of a snapshot sits on one ridge of it, so the
// particles are sorted by cell and the sorted list is reduced by a tree whose shape depends on n alone -- no atomics on floating-
// point values, no walk along a cell's members:
//   1. key pass: per particle its cell (the edges in LDS, a binary search on the float64 edges as passed) or all ones, and its index;
//   2. one stable radix sort of (key, index) over the ceil(log2(cells + 1)) low bits of the key;
//   3. reduction, level 0: a workgroup takes BLOCK = 256 consecutive sorted entries, one per lane.  Each wave runs a segmented
//      inclusive scan over its 64 entries (runs of equal keys; DPP row shifts and row broadcasts on the halves of the float64s, the
//      terms of another run replaced by nothing).  A run that touches neither end of the wave is complete: its last lane writes the
//      cell.  The run at the wave's left end and the one at its right end go to LDS, two records per wave in wave order, and wave 0
//      scans those eight records the same way.  A run of records that touches neither end of the block (or the list's end) is
//      written to its cell; the two that do are the block's output records;
//   4. levels 1, 2, ..: the same kernel over the records of the level before (1 / 128 of its entries), until one block is left.
// A cell is written exactly once, by the level at which its run stops touching a block's end; a cell with a third of the particles
// is reduced by n / 3 / 256 workgroups at level 0, n / 3 / 32768 at level 1, and so on.  Every addition has a fixed place.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <vector>

#include "tsp_hist2d_layout.h"
#include "tsp_internal.h"

namespace tsp {
namespace {

using namespace hist2d;

constexpr uint32_t NO_CELL = 0xffffffffu;       // the key of a particle in no cell: above every cell in the sorted bits, -1 in bin_out

// the bin of x among the nb + 1 ascending edges e: the number of edges <= x, less one: -1 (below e[0]) .. nb (at or above e[nb])
__device__ __forceinline__ int bin_of(const double *e, int nb, double x) {
    int lo = 0, hi = nb + 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

// A fixed grid strides over the particles, so that the edges are staged once per workgroup and not once per 256 particles.
__global__ __launch_bounds__(256) void hist2d_key_kernel(int64_t n, const float *__restrict__ x, const float *__restrict__ y,
                                                         const float *__restrict__ w, const float *__restrict__ v,
                                                         const double *__restrict__ edges, int nx, int ny,
                                                         uint32_t *__restrict__ keys, uint32_t *__restrict__ index,
                                                         unsigned long long *__restrict__ counters) {
    __shared__ double s_edges[2 * (MAX_BINS + 1)];
    for (int k = threadIdx.x; k < nx + ny + 2; k += 256) s_edges[k] = edges[k];
    __syncthreads();
    const double *ex = s_edges, *ey = s_edges + nx + 1;
    unsigned n_valid = 0, n_binned = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float xf = x[i], yf = y[i];
        bool valid = finite_f32(xf) && finite_f32(yf);
        if (w) valid = valid && finite_f32(w[i]);
        if (v) valid = valid && finite_f32(v[i]);
        uint32_t key = NO_CELL;
        if (valid) {
            const int ix = bin_of(ex, nx, (double)xf), iy = bin_of(ey, ny, (double)yf);
            if (ix >= 0 && ix < nx && iy >= 0 && iy < ny) key = (uint32_t)(iy * nx + ix);
        }
        keys[i] = key;
        index[i] = (uint32_t)i;
        n_valid += valid ? 1u : 0u;
        n_binned += key != NO_CELL ? 1u : 0u;
    }
    for (int off = 32; off; off >>= 1) {
        n_valid += (unsigned)__shfl_xor((int)n_valid, off);
        n_binned += (unsigned)__shfl_xor((int)n_binned, off);
    }
    if ((threadIdx.x & 63) == 0) {      // (integer counts: the order of these adds changes nothing)
        atomicAdd(counters, (unsigned long long)n_valid);
        atomicAdd(counters + 1, (unsigned long long)n_binned);
    }
}

struct Rec {
    uint32_t key, cnt;
    double s0, s1, s2;      // sum w, sum w v, sum (w v) v
};

struct Records {            // one array per field; s1 and s2 only with values
    uint32_t *key, *cnt;
    double *s0, *s1, *s2;
};

// The DPP move of a 32-bit value: lanes that have no source (the first lanes of a row under row_shr, the rows outside ROW_MASK
// under row_bcast) receive 0 -- as both halves of a float64, +0.0.
template <int CTRL, int ROW_MASK> __device__ __forceinline__ int dpp_or_zero(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xf, false);
}
template <int CTRL, int ROW_MASK> __device__ __forceinline__ double dpp_f64(double v) {
    return __hiloint2double(dpp_or_zero<CTRL, ROW_MASK>(__double2hiint(v)), dpp_or_zero<CTRL, ROW_MASK>(__double2loint(v)));
}
template <int CTRL, int ROW_MASK, bool HAS_V> __device__ __forceinline__ void scan_step(Rec &r, bool take) {
    const uint32_t c = (uint32_t)dpp_or_zero<CTRL, ROW_MASK>((int)r.cnt);
    const double a0 = dpp_f64<CTRL, ROW_MASK>(r.s0);
    r.cnt = take ? r.cnt + c : r.cnt;
    r.s0 = take ? r.s0 + a0 : r.s0;
    if (HAS_V) {
        const double a1 = dpp_f64<CTRL, ROW_MASK>(r.s1), a2 = dpp_f64<CTRL, ROW_MASK>(r.s2);
        r.s1 = take ? r.s1 + a1 : r.s1;
        r.s2 = take ? r.s2 + a2 : r.s2;
    }
}

// The segmented inclusive scan of a wave: `head` marks the first lane of every run (lane 0 always is one).  Afterwards the last lane
// of a run (is_end) holds the run's count and sums; start is the run's first lane.  Inside a row of 16 lanes the steps 1, 2, 4, 8 take
// the lane that far below if it belongs to the run; then row 1 takes lane 15 and row 3 lane 47 (row_bcast:15), and rows 2 and 3 take
// lane 31 (row_bcast:31), each where the run began before that lane's row ends.  Every lane executes every step.
template <bool HAS_V> __device__ __forceinline__ void segmented_scan(Rec &r, bool head, int lane, int &start, bool &is_end) {
    const unsigned long long heads = __ballot(head);
    start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
    is_end = lane == 63 || ((heads >> ((lane + 1) & 63)) & 1ull) != 0;
    const int in_row = lane & 15, row0 = lane & ~15;
    scan_step<0x111, 0xf, HAS_V>(r, in_row >= 1 && lane - 1 >= start);       // row_shr:1
    scan_step<0x112, 0xf, HAS_V>(r, in_row >= 2 && lane - 2 >= start);       // row_shr:2
    scan_step<0x114, 0xf, HAS_V>(r, in_row >= 4 && lane - 4 >= start);       // row_shr:4
    scan_step<0x118, 0xf, HAS_V>(r, in_row >= 8 && lane - 8 >= start);       // row_shr:8
    scan_step<0x142, 0xa, HAS_V>(r, (lane & 16) != 0 && start < row0);       // row_bcast:15 into rows 1 and 3
    scan_step<0x143, 0xc, HAS_V>(r, lane >= 32 && start < 32);               // row_bcast:31 into rows 2 and 3
}

// a finished run: its cell's count and sums, each sum started at +0.0 (a lone -0.0 term gives +0.0); keys at or above `cells` (the
// particles in no cell) are dropped here
template <bool HAS_V> __device__ __forceinline__ void write_cell(const Rec &r, uint32_t cells, int64_t *__restrict__ count,
                                                                 double *__restrict__ sums) {
    if (r.key >= cells) return;
    count[r.key] = (int64_t)r.cnt;
    sums[r.key] = 0.0 + r.s0;
    if (HAS_V) {
        sums[(size_t)cells + r.key] = 0.0 + r.s1;
        sums[2 * (size_t)cells + r.key] = 0.0 + r.s2;
    }
}

template <bool HAS_V> __device__ __forceinline__ void put_record(const Records &out, int64_t slot, uint32_t key, uint32_t cnt, double s0,
                                                                 double s1, double s2) {
    out.key[slot] = key, out.cnt[slot] = cnt, out.s0[slot] = s0;
    if (HAS_V) out.s1[slot] = s1, out.s2[slot] = s2;
}

// One workgroup per block of BLOCK entries.  FIRST: the entries are the sorted (key, particle index) pairs, and their terms are
// formed here; otherwise they are the records `in` of the level before.  A block of a level with more than one block leaves the
// records 2 b and 2 b + 1 in `out`; where one run reaches both ends, or the block is the first or the last of its level, the record
// that has no run of its own repeats its neighbour's key with a count of 0 and sums of +0.0, so that the next level's keys ascend.
template <bool FIRST, bool HAS_V>
__global__ __launch_bounds__(256) void hist2d_reduce_kernel(int64_t m, uint32_t cells, const uint32_t *__restrict__ keys_in,
                                                            const uint32_t *__restrict__ index_in, const float *__restrict__ w,
                                                            const float *__restrict__ v, Records in, Records out,
                                                            int64_t *__restrict__ count, double *__restrict__ sums) {
    __shared__ uint32_t s_key[8], s_cnt[8];
    __shared__ double s_s0[8], s_s1[8], s_s2[8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b = blockIdx.x, nb = gridDim.x, e = b * BLOCK + threadIdx.x;

    Rec r = {NO_CELL, 0u, 0.0, 0.0, 0.0};       // (past the list's end: a key that is never written)
    if (e < m) {
        if (FIRST) {
            r.key = keys_in[e];
            if (r.key < cells) {
                const uint32_t i = index_in[e];
                const double wd = w ? (double)w[i] : 1.0;
                r.cnt = 1u, r.s0 = wd;
                if (HAS_V) {
                    const double vd = (double)v[i];
                    r.s1 = wd * vd;
                    r.s2 = r.s1 * vd;
                }
            }
        } else {
            r.key = in.key[e], r.cnt = in.cnt[e], r.s0 = in.s0[e];
            if (HAS_V) r.s1 = in.s1[e], r.s2 = in.s2[e];
        }
    }
    int start;
    bool is_end;
    const uint32_t below = (uint32_t)__shfl_up((int)r.key, 1);
    segmented_scan<HAS_V>(r, lane == 0 || below != r.key, lane, start, is_end);
    if (is_end) {
        if (start != 0 && lane != 63) {
            write_cell<HAS_V>(r, cells, count, sums);
        } else {
            const int slot = 2 * wave + (start == 0 ? 0 : 1);
            s_key[slot] = r.key, s_cnt[slot] = r.cnt, s_s0[slot] = r.s0, s_s1[slot] = r.s1, s_s2[slot] = r.s2;
            if (start == 0 && lane == 63) s_key[slot + 1] = r.key, s_cnt[slot + 1] = 0u, s_s0[slot + 1] = 0.0, s_s1[slot + 1] = 0.0, s_s2[slot + 1] = 0.0;
        }
    }
    __syncthreads();
    if (wave != 0) return;

    Rec q = {NO_CELL, 0u, 0.0, 0.0, 0.0};
    if (lane < 8) q.key = s_key[lane], q.cnt = s_cnt[lane], q.s0 = s_s0[lane], q.s1 = s_s1[lane], q.s2 = s_s2[lane];
    const uint32_t below_q = (uint32_t)__shfl_up((int)q.key, 1);
    segmented_scan<HAS_V>(q, lane == 0 || lane == 8 || below_q != q.key, lane, start, is_end);
    if (!is_end || lane >= 8) return;
    const bool left = start == 0 && b > 0, right = lane == 7 && b + 1 < nb;
    if (!left && !right) {
        write_cell<HAS_V>(q, cells, count, sums);
    } else if (left) {
        put_record<HAS_V>(out, 2 * b, q.key, q.cnt, q.s0, q.s1, q.s2);
        if (lane == 7 || b + 1 == nb) put_record<HAS_V>(out, 2 * b + 1, q.key, 0u, 0.0, 0.0, 0.0);
    } else {
        put_record<HAS_V>(out, 2 * b + 1, q.key, q.cnt, q.s0, q.s1, q.s2);
        if (b == 0) put_record<HAS_V>(out, 0, q.key, 0u, 0.0, 0.0, 0.0);
    }
}

Records records_at(char *base, int64_t records, int planes) {
    Records r = {};
    if (!records) return r;
    const size_t w4 = align256((size_t)records * 4), w8 = align256((size_t)records * 8);
    r.key = reinterpret_cast<uint32_t *>(base);
    r.cnt = reinterpret_cast<uint32_t *>(base + w4);
    r.s0 = reinterpret_cast<double *>(base + 2 * w4);
    if (planes == 3) {
        r.s1 = reinterpret_cast<double *>(base + 2 * w4 + w8);
        r.s2 = reinterpret_cast<double *>(base + 2 * w4 + 2 * w8);
    }
    return r;
}

}  // namespace

// The host side of tsp_histogram_2d (the arguments are checked by the entry point).  Device memory through the two sites of the
// gather calls, carved by tsp_hist2d_layout.h; nothing of the context changes.
int histogram_2d(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *w, const float *v,
                 const tsp_hist2d_spec *spec, int64_t *count_out, double *sums_out, int32_t *bin_out, tsp_hist2d_info *info_out) {
    hipStream_t st = ctx->stream;
    // measurement aid: TOPSY_HIST2D_STATS=1 reports the time of the upload, of the three device stages and of the whole call
    const char *env = getenv("TOPSY_HIST2D_STATS");
    const bool stats = env && env[0] == '1';
    const auto t_call = std::chrono::steady_clock::now();
    auto ms_since = [](std::chrono::steady_clock::time_point t0) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    };
    const int nx = spec->nx, ny = spec->ny, planes = v ? 3 : 1;
    const int64_t cells = (int64_t)nx * ny;
    const int bits = key_bits(cells);
    const Levels lv = levels_of(n);

    size_t sort_bytes = 0;
    TSP_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr,
                                               (uint32_t *)nullptr, (int)n, 0, bits, st));
    const Carve c = carve(n, nx, ny, w != nullptr, v != nullptr, bin_out != nullptr, sort_bytes);
    DeviceScratch dh, da;
    const int rc_scratch = gather_scratch(ctx, dh, c.h_bytes, da, c.a_bytes);
    if (rc_scratch != TSP_OK) return rc_scratch;
    char *hb = dh.as<char>(), *ab = da.as<char>();
    float *d_x = reinterpret_cast<float *>(hb + c.h_x.offset), *d_y = reinterpret_cast<float *>(hb + c.h_y.offset);
    float *d_w = w ? reinterpret_cast<float *>(hb + c.h_w.offset) : nullptr, *d_v = v ? reinterpret_cast<float *>(hb + c.h_v.offset) : nullptr;
    int64_t *d_count = reinterpret_cast<int64_t *>(ab + c.a_count.offset);
    double *d_sums = reinterpret_cast<double *>(ab + c.a_sums.offset), *d_edges = reinterpret_cast<double *>(ab + c.a_edges.offset);
    unsigned long long *d_counters = reinterpret_cast<unsigned long long *>(ab + c.a_counters.offset);
    uint32_t *d_keys = reinterpret_cast<uint32_t *>(ab + c.a_keys.offset), *d_keys_sorted = reinterpret_cast<uint32_t *>(ab + c.a_keys_sorted.offset);
    uint32_t *d_index = reinterpret_cast<uint32_t *>(ab + c.a_index.offset), *d_index_sorted = reinterpret_cast<uint32_t *>(ab + c.a_index_sorted.offset);
    const Records rec[2] = {records_at(ab + c.a_records_a.offset, c.records_a, planes), records_at(ab + c.a_records_b.offset, c.records_b, planes)};
    void *d_tmp = ab + c.a_tmp.offset;

    std::vector<double> edges((size_t)nx + ny + 2);
    std::copy(spec->edges_x, spec->edges_x + nx + 1, edges.begin());
    std::copy(spec->edges_y, spec->edges_y + ny + 1, edges.begin() + nx + 1);
    const size_t fbytes = (size_t)n * sizeof(float);
    auto t0 = std::chrono::steady_clock::now();
    TSP_HIP(hipMemcpyAsync(d_x, x, fbytes, hipMemcpyHostToDevice, st));
    TSP_HIP(hipMemcpyAsync(d_y, y, fbytes, hipMemcpyHostToDevice, st));
    if (w) TSP_HIP(hipMemcpyAsync(d_w, w, fbytes, hipMemcpyHostToDevice, st));
    if (v) TSP_HIP(hipMemcpyAsync(d_v, v, fbytes, hipMemcpyHostToDevice, st));
    TSP_HIP(hipMemcpyAsync(d_edges, edges.data(), edges.size() * sizeof(double), hipMemcpyHostToDevice, st));
    // the table is the call's: whatever the scratch held, an empty cell is count 0 and +0.0
    TSP_HIP(hipMemsetAsync(d_count, 0, c.a_count.bytes, st));
    TSP_HIP(hipMemsetAsync(d_sums, 0, c.a_sums.bytes, st));
    TSP_HIP(hipMemsetAsync(d_counters, 0, c.a_counters.bytes, st));
    TSP_HIP(hipStreamSynchronize(st));          // (edges is pageable host memory of this function)
    const double ms_upload = ms_since(t0);

    if (stats) TSP_HIP(hipEventRecord(ctx->ev[EV_T0], st));
    const int key_grid = (int)std::min<int64_t>(blocks_of(n), (int64_t)ctx->cu_count * 8);
    hipLaunchKernelGGL(hist2d_key_kernel, dim3(key_grid), dim3(256), 0, st, n, d_x, d_y, d_w, d_v, d_edges, nx, ny, d_keys, d_index,
                       d_counters);
    TSP_HIP(hipGetLastError());
    if (stats) TSP_HIP(hipEventRecord(ctx->ev[EV_T1], st));
    TSP_HIP(hipcub::DeviceRadixSort::SortPairs(d_tmp, sort_bytes, d_keys, d_keys_sorted, d_index, d_index_sorted, (int)n, 0, bits, st));
    if (stats) TSP_HIP(hipEventRecord(ctx->ev[EV_T2], st));
    for (int k = 0; k < lv.count; ++k) {
        const Records none = {};
        const Records &in = k == 0 ? none : rec[(k - 1) & 1], &out = k + 1 < lv.count ? rec[k & 1] : none;
        auto kernel = k == 0 ? (v ? hist2d_reduce_kernel<true, true> : hist2d_reduce_kernel<true, false>)
                             : (v ? hist2d_reduce_kernel<false, true> : hist2d_reduce_kernel<false, false>);
        hipLaunchKernelGGL(kernel, dim3((unsigned)lv.blocks[k]), dim3(BLOCK), 0, st, lv.entries[k], (uint32_t)cells, d_keys_sorted,
                           d_index_sorted, d_w, d_v, in, out, d_count, d_sums);
        TSP_HIP(hipGetLastError());
    }
    if (stats) TSP_HIP(hipEventRecord(ctx->ev[EV_T3], st));

    unsigned long long counters[2] = {0, 0};
    TSP_HIP(hipMemcpyAsync(counters, d_counters, sizeof(counters), hipMemcpyDeviceToHost, st));
    TSP_HIP(hipMemcpyAsync(count_out, d_count, c.a_count.bytes, hipMemcpyDeviceToHost, st));
    TSP_HIP(hipMemcpyAsync(sums_out, d_sums, c.a_sums.bytes, hipMemcpyDeviceToHost, st));
    if (bin_out) TSP_HIP(hipMemcpyAsync(bin_out, d_keys, c.bins_bytes, hipMemcpyDeviceToHost, st));       // (all ones is -1)
    TSP_HIP(hipStreamSynchronize(st));
    if (info_out) info_out->n_valid = (int64_t)counters[0], info_out->n_binned = (int64_t)counters[1];
    if (stats) {
        float key_ms = 0.0f, sort_ms = 0.0f, reduce_ms = 0.0f;
        TSP_HIP(hipEventElapsedTime(&key_ms, ctx->ev[EV_T0], ctx->ev[EV_T1]));
        TSP_HIP(hipEventElapsedTime(&sort_ms, ctx->ev[EV_T1], ctx->ev[EV_T2]));
        TSP_HIP(hipEventElapsedTime(&reduce_ms, ctx->ev[EV_T2], ctx->ev[EV_T3]));
        fprintf(stderr, "tsp_histogram_2d: n=%lld nx=%d ny=%d planes=%d key_bits=%d levels=%d valid=%lld binned=%lld upload_ms=%.3f "
                        "key_ms=%.4f sort_ms=%.4f reduce_ms=%.4f call_ms=%.3f\n",
                (long long)n, nx, ny, planes, bits, lv.count, (long long)counters[0], (long long)counters[1], ms_upload, key_ms,
                sort_ms, reduce_ms, ms_since(t_call));
    }
    return TSP_OK;
}

}  // namespace tsp
