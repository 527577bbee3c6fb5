// tsp_gravity.hip -- softened direct-sum gravity (tsp_gravity_direct): the potential and the acceleration at every target from
// every source, Plummer-softened with the source's length, G = 1 -- pynbody's gravity.calc direct sum (the 'phi' of a snapshot, the
// midplane rotation curve and potential of a disc profile).  n_src * n_tgt pairs: no tree, no periodic images.
//
// Contract (include/topsy_splat.h): d = t_i - s_j per component, r2 = d . d + eps_j^2, pot_i = -sum m_j r2^(-1/2),
// acc_i = -sum m_j r2^(-3/2) d; pair terms in float32, per-target sums in float64 over float32 runs of RUN consecutive sources.
//
// The passes:
//   1. gravity_prepare_kernel, in place on the uploaded source planes (x, y, z, m, eps): a source with a non-finite field becomes
//      the padding source (m = 0 at the origin with eps^2 = 1: every term it forms is an exact zero), a valid one keeps its fields
//      and gets eps^2 (one float32 rounding) in the eps plane; the valid count is an integer atomic.
//   2. gravity_pairs_kernel<TPL, ACC>: 256 lanes, each owning TPL = 1, 2 or 4 targets in registers (target local = slot * 256 + lane
//      of the workgroup's 256 TPL targets), so that one fetch of a source serves TPL pairs per lane.  The sources come in tiles of
//      TILE = 512 through LDS as (x, y, z, m) float4 plus eps^2: every lane of a wave reads the same address (a broadcast: one
//      ds_read_b128 and one ds_read_b32 per source and wave, no bank conflict), the next tile's global loads are in flight while a
//      tile is summed.  Past the end of the sources a tile is filled with padding sources, so the inner loop has no bounds test.
//      grid = (splits, target blocks): workgroup (s, b) sums tiles [n_tiles s / splits, n_tiles (s + 1) / splits) for the targets of
//      block b and stores float64 partials.  Per pair 3 subtractions, 3 FMAs for r2, v_rsq_f32 (1 ulp), 1 multiply and 1 add for the
//      potential and, with ACC, 2 multiplies and 3 FMAs for the acceleration.  The tests "r2 is no normal number" (a pair at
//      distance 0 with eps = 0 contributes nothing) and "source index == target index" (targets = sources) cost a compare and a
//      select per pair; they run only in the tiles that need them -- one with an eps^2 below 2^-100, or one whose index range meets
//      the block's own targets -- chosen per tile for the whole workgroup (CHECK).  Both forms give the same bits for every pair
//      that counts.
//   3. gravity_reduce_kernel: one lane per target and component adds its partials in split order (eight loads in flight), changes
//      the sign, writes NaN for a target with a non-finite coordinate and counts the others.
// Few targets, many sources (a rotation curve: some hundred probes, 1e7 - 1e8 sources): one or two target blocks, TPL by the count,
// and splits = 4 workgroups per CU over the source range.  Many targets ('phi' of every particle): target blocks of 1024, launched
// in chunks of 2^18 targets so that the partials stay bounded (chunk_targets * splits * 32 bytes <= 32 MB on 256 CUs).
// Determinism: no floating-point atomics; TPL, the blocks and the splits are functions of n_src, the chunk's target count and
// ctx->cu_count; a target's sums do not depend on TPL, on CHECK or on which other targets share its block.
//
// Rounding (u = 2^-24), against the float64 evaluation on the float32 inputs: d within u; eps^2 within u; r2 = fma(dx, dx,
// fma(dy, dy, fma(dz, dz, eps^2))) within 2u + 3u; r2^(-1/2) within 2.5u + 2u (v_rsq_f32: 1 ulp <= 2u) -- 5u; the potential term
// m inv within 6u; inv^2 within 11u, w = (m inv) inv^2 within 18u, the acceleration term fma(w, d, .) within 19u before the sum's own
// rounding; a float32 run of RUN = 16 terms adds 15u; the float64 additions (n_src / 16 + splits of them) stay below 2^-22 = 4u for
// n_src < 2^31.  6u + 15u + 4u = 25u and 19u + 15u + 4u = 38u: TSP_GRAVITY_ERROR_K = 64 holds with room.
//
// Resources as built (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage) and measured rates: DESIGN.md section 4.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "tsp_internal.h"

namespace tsp {
namespace {

constexpr int TILE = TSP_GRAVITY_SOURCE_TILE;                    // sources per LDS tile
constexpr int LANES = 256;                                       // lanes of a workgroup
constexpr int MAX_TPL = TSP_GRAVITY_TARGETS_PER_WORKGROUP / LANES;   // targets per lane at most
constexpr int RUN = 16;                                          // consecutive sources summed in float32
constexpr int PER_LANE = TILE / LANES;                           // sources a lane stages per tile
constexpr int64_t CHUNK_TARGETS = 1ll << 18;                     // targets per launch
constexpr float R2_NORMAL = 1.17549435e-38f;                     // 2^-126: below it a pair contributes nothing
constexpr float E2_UNCHECKED = 7.88860905e-31f;                  // 2^-100: a tile whose eps^2 all reach it needs no r2 test
constexpr unsigned NO_INDEX = 0xffffffffu;                       // the source index no target has
static_assert(TILE % LANES == 0 && TILE % RUN == 0 && MAX_TPL == 4, "tile and target block shapes");

__global__ __launch_bounds__(256) void gravity_prepare_kernel(float *__restrict__ x, float *__restrict__ y, float *__restrict__ z,
                                                              float *__restrict__ m, float *__restrict__ e, int64_t n, int has_eps,
                                                              float eps_all, unsigned long long *__restrict__ n_valid) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool valid = false;
    if (i < n) {
        const float eps = has_eps ? e[i] : eps_all;
        valid = isfinite(x[i]) && isfinite(y[i]) && isfinite(z[i]) && isfinite(m[i]) && isfinite(eps);
        if (valid) {
            e[i] = eps * eps;
        } else {
            x[i] = y[i] = z[i] = m[i] = 0.0f;
            e[i] = 1.0f;
        }
    }
    const unsigned long long mask = __ballot(valid);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd(n_valid, (unsigned long long)__popcll(mask));
}

// The pairs of one tile in LDS with the TPL targets of a lane: float32 runs of RUN sources, added to the float64 sums.
template <int TPL, bool ACC, bool CHECK>
__device__ __forceinline__ void gravity_tile(const float4 *__restrict__ s4, const float *__restrict__ se2, unsigned tile_base,
                                             const unsigned (&ti)[TPL], const float (&px)[TPL], const float (&py)[TPL],
                                             const float (&pz)[TPL], double (&sum)[TPL][ACC ? 4 : 1]) {
    constexpr int NC = ACC ? 4 : 1;
    for (int k0 = 0; k0 < TILE; k0 += RUN) {
        float f[TPL][NC];
#pragma unroll
        for (int t = 0; t < TPL; ++t)
#pragma unroll
            for (int c = 0; c < NC; ++c) f[t][c] = 0.0f;
#pragma unroll
        for (int kk = 0; kk < RUN; ++kk) {
            const float4 s = s4[k0 + kk];
            const float e2 = se2[k0 + kk];
#pragma unroll
            for (int t = 0; t < TPL; ++t) {
                const float dx = px[t] - s.x, dy = py[t] - s.y, dz = pz[t] - s.z;
                const float r2 = __builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, __builtin_fmaf(dz, dz, e2)));
                float inv = __builtin_amdgcn_rsqf(r2);
                if (CHECK) inv = (r2 >= R2_NORMAL && ti[t] != tile_base + (unsigned)(k0 + kk)) ? inv : 0.0f;
                const float p = s.w * inv;
                f[t][0] += p;
                if (ACC) {
                    const float w = p * (inv * inv);
                    f[t][1] = __builtin_fmaf(w, dx, f[t][1]);
                    f[t][2] = __builtin_fmaf(w, dy, f[t][2]);
                    f[t][3] = __builtin_fmaf(w, dz, f[t][3]);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < TPL; ++t)
#pragma unroll
            for (int c = 0; c < NC; ++c) sum[t][c] += (double)f[t][c];
    }
}

// n_tgt targets at tx / ty / tz (this launch's chunk); self_index0: the source index of the chunk's first target when the targets
// are the sources, else NO_INDEX.  partials[((block * splits + split) * NC + c) * (256 TPL) + local], c = 0 the potential sum,
// 1 .. 3 the acceleration sums (signs not yet changed).
template <int TPL, bool ACC>
__global__ __launch_bounds__(256) void gravity_pairs_kernel(const float *__restrict__ sx, const float *__restrict__ sy,
                                                            const float *__restrict__ sz, const float *__restrict__ sm,
                                                            const float *__restrict__ se2, int64_t n_src, int n_tiles,
                                                            const float *__restrict__ tx, const float *__restrict__ ty,
                                                            const float *__restrict__ tz, int n_tgt, unsigned self_index0,
                                                            double *__restrict__ partials) {
    constexpr int NC = ACC ? 4 : 1;
    constexpr int BL = LANES * TPL;
    __shared__ float4 s4[TILE];
    __shared__ float se2s[TILE];
    const int lane = threadIdx.x;
    const int split = blockIdx.x, splits = gridDim.x, block = blockIdx.y;
    const int tile_lo = (int)((int64_t)n_tiles * split / splits), tile_hi = (int)((int64_t)n_tiles * (split + 1) / splits);
    const bool self = self_index0 != NO_INDEX;
    const unsigned own_lo = self_index0 + (unsigned)block * BL, own_hi = own_lo + BL;     // the block's targets as source indices

    float px[TPL], py[TPL], pz[TPL];
    unsigned ti[TPL];
    double sum[TPL][NC];
#pragma unroll
    for (int t = 0; t < TPL; ++t) {
        const int i = block * BL + t * LANES + lane;
        const bool in = i < n_tgt;
        px[t] = in ? tx[i] : 0.0f;
        py[t] = in ? ty[i] : 0.0f;
        pz[t] = in ? tz[i] : 0.0f;
        ti[t] = self && in ? self_index0 + (unsigned)i : NO_INDEX;
#pragma unroll
        for (int c = 0; c < NC; ++c) sum[t][c] = 0.0;
    }

    float4 r4[PER_LANE];
    float re2[PER_LANE];
    auto fetch = [&](int tile) {
#pragma unroll
        for (int q = 0; q < PER_LANE; ++q) {
            const int64_t j = (int64_t)tile * TILE + q * LANES + lane;
            const bool in = j < n_src;
            r4[q] = in ? make_float4(sx[j], sy[j], sz[j], sm[j]) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            re2[q] = in ? se2[j] : 1.0f;
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
            tiny |= !(re2[q] >= E2_UNCHECKED);
        }
        const unsigned tile_base = (unsigned)tile * TILE;
        const bool own = self && tile_base < own_hi && tile_base + TILE > own_lo;
        const bool check = __syncthreads_or(tiny) || own;
        if (tile + 1 < tile_hi) fetch(tile + 1);
        if (check)
            gravity_tile<TPL, ACC, true>(s4, se2s, tile_base, ti, px, py, pz, sum);
        else
            gravity_tile<TPL, ACC, false>(s4, se2s, tile_base, ti, px, py, pz, sum);
    }
    double *out = partials + ((size_t)block * splits + split) * NC * BL;
#pragma unroll
    for (int t = 0; t < TPL; ++t)
#pragma unroll
        for (int c = 0; c < NC; ++c) out[(size_t)c * BL + t * LANES + lane] = sum[t][c];
}

__global__ __launch_bounds__(256) void gravity_reduce_kernel(const double *__restrict__ partials, int splits, int bl, int nc,
                                                             const float *__restrict__ tx, const float *__restrict__ ty,
                                                             const float *__restrict__ tz, int n_tgt, double *__restrict__ pot,
                                                             double *__restrict__ acc, unsigned long long *__restrict__ n_valid) {
    const int i = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y;      // a lane per target and component
    bool valid = false;
    if (i < n_tgt) {
        valid = isfinite(tx[i]) && isfinite(ty[i]) && isfinite(tz[i]);
        const int block = i / bl, local = i % bl;
        const double *p = partials + ((size_t)block * splits * nc + c) * bl + local;
        const size_t stride = (size_t)nc * bl;
        double s = 0.0;
        int k = 0;
        for (; k + 8 <= splits; k += 8) {      // eight loads in flight, added in index order
            double v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = p[(size_t)(k + q) * stride];
#pragma unroll
            for (int q = 0; q < 8; ++q) s += v[q];
        }
        for (; k < splits; ++k) s += p[(size_t)k * stride];
        const double v = valid ? 0.0 - s : (double)NAN;
        if (c == 0)
            pot[i] = v;
        else
            acc[(size_t)3 * i + (c - 1)] = v;
    }
    const unsigned long long mask = __ballot(valid && c == 0);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd(n_valid, (unsigned long long)__popcll(mask));
}

// The shape of one launch: targets per lane, target blocks and source splits, from the chunk's targets, the tiles and the CUs.
struct GravityPlan {
    int tpl, blocks, splits;
    size_t partial_doubles(int nc) const { return (size_t)blocks * splits * nc * LANES * tpl; }
};
GravityPlan gravity_plan(int64_t n_chunk, int n_tiles, int cu_count) {
    GravityPlan p;
    p.tpl = n_chunk <= LANES ? 1 : n_chunk <= 2 * LANES ? 2 : MAX_TPL;
    const int bl = LANES * p.tpl;
    p.blocks = (int)((n_chunk + bl - 1) / bl);
    p.splits = std::max(1, std::min(n_tiles, (4 * std::max(cu_count, 1) + p.blocks - 1) / p.blocks));
    return p;
}

template <bool ACC>
void launch_pairs(const GravityPlan &plan, hipStream_t st, const float *sx, const float *sy, const float *sz, const float *sm,
                  const float *se2, int64_t n_src, int n_tiles, const float *tx, const float *ty, const float *tz, int n_tgt,
                  unsigned self_index0, double *partials) {
    const dim3 grid((unsigned)plan.splits, (unsigned)plan.blocks);
    auto kernel = plan.tpl == 1 ? gravity_pairs_kernel<1, ACC> : plan.tpl == 2 ? gravity_pairs_kernel<2, ACC> : gravity_pairs_kernel<4, ACC>;
    hipLaunchKernelGGL(kernel, grid, dim3(LANES), 0, st, sx, sy, sz, sm, se2, n_src, n_tiles, tx, ty, tz, n_tgt, self_index0, partials);
}

size_t align16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

}  // namespace

// The host side of tsp_gravity_direct (the arguments are checked by the entry point).  Device memory, through the two sites of
// the gather calls:
//   "sph_sum_h": [the source planes x, y, z, m, eps (-> eps^2): 5 n_src floats]
//   "sph_sum_a": [pot: n_tgt doubles][acc: 3 n_tgt doubles][the partials of one launch][the two valid counts][the target planes
//                x, y, z: 3 n_tgt floats]
int gravity_direct(tsp_context *ctx, int64_t n_src, const float *sx, const float *sy, const float *sz, const float *mass,
                   const float *eps, float eps_all, int64_t n_tgt, const float *tx, const float *ty, const float *tz, double *pot_out,
                   double *acc_out, tsp_gravity_info *info_out) {
    hipStream_t st = ctx->stream;
    // measurement aid: TOPSY_GRAVITY_STATS=1 reports the launch shapes and the time of the pair and reduce kernels
    const char *env = getenv("TOPSY_GRAVITY_STATS");
    const bool stats = env && env[0] == '1';
    const bool self = tx == nullptr;
    const bool want_acc = acc_out != nullptr;
    const int nc = want_acc ? 4 : 1;
    const int n_tiles = (int)((n_src + TILE - 1) / TILE);
    const size_t src_bytes = (size_t)n_src * sizeof(float), tgt_bytes = (size_t)n_tgt * sizeof(float);

    size_t partial_doubles = 0;
    for (int64_t first = 0; first < n_tgt; first += CHUNK_TARGETS)
        partial_doubles = std::max(partial_doubles,
                                   gravity_plan(std::min(CHUNK_TARGETS, n_tgt - first), n_tiles, ctx->cu_count).partial_doubles(nc));
    const size_t off_acc = (size_t)n_tgt * sizeof(double), off_partials = off_acc + (size_t)3 * n_tgt * sizeof(double);
    const size_t off_counts = off_partials + partial_doubles * sizeof(double);
    const size_t off_targets = off_counts + 2 * sizeof(unsigned long long);
    const size_t b_bytes = off_targets + 3 * align16(tgt_bytes);

    DeviceScratch dsrc, db;
    const int rc_scratch = gather_scratch(ctx, dsrc, 5 * align16(src_bytes), db, b_bytes);
    if (rc_scratch != TSP_OK) return rc_scratch;
    float *plane[5];
    for (int a = 0; a < 5; ++a) plane[a] = reinterpret_cast<float *>(dsrc.as<char>() + a * align16(src_bytes));
    char *b = db.as<char>();
    double *d_pot = reinterpret_cast<double *>(b), *d_acc = reinterpret_cast<double *>(b + off_acc);
    double *d_partials = reinterpret_cast<double *>(b + off_partials);
    unsigned long long *d_counts = reinterpret_cast<unsigned long long *>(b + off_counts);     // [0] valid sources, [1] valid targets
    float *tplane[3];
    for (int a = 0; a < 3; ++a) tplane[a] = reinterpret_cast<float *>(b + off_targets + a * align16(tgt_bytes));

    const float *host_src[5] = {sx, sy, sz, mass, eps};
    for (int a = 0; a < (eps ? 5 : 4); ++a) TSP_HIP(hipMemcpyAsync(plane[a], host_src[a], src_bytes, hipMemcpyHostToDevice, st));
    const float *host_tgt[3] = {tx, ty, tz};
    for (int a = 0; a < 3; ++a) {      // (targets = sources: the raw planes, before the preparation replaces the invalid sources)
        if (self)
            TSP_HIP(hipMemcpyAsync(tplane[a], plane[a], tgt_bytes, hipMemcpyDeviceToDevice, st));
        else
            TSP_HIP(hipMemcpyAsync(tplane[a], host_tgt[a], tgt_bytes, hipMemcpyHostToDevice, st));
    }
    TSP_HIP(hipMemsetAsync(d_counts, 0, 2 * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(gravity_prepare_kernel, dim3((unsigned)((n_src + 255) / 256)), dim3(256), 0, st, plane[0], plane[1], plane[2],
                       plane[3], plane[4], n_src, eps ? 1 : 0, eps_all, d_counts);
    TSP_HIP(hipGetLastError());
    unsigned long long counts[2] = {0, 0};
    TSP_HIP(hipMemcpyAsync(counts, d_counts, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    TSP_HIP(hipStreamSynchronize(st));      // (the host arrays are pageable: they are not read after this)
    TSP_REQUIRE(counts[0] > 0, TSP_EINVAL, "tsp_gravity_direct: no source has finite coordinates, mass and softening length");

    if (stats) TSP_HIP(hipEventRecord(ctx->ev[EV_T0], st));
    for (int64_t first = 0; first < n_tgt; first += CHUNK_TARGETS) {
        const int n_chunk = (int)std::min(CHUNK_TARGETS, n_tgt - first);
        const GravityPlan plan = gravity_plan(n_chunk, n_tiles, ctx->cu_count);
        const unsigned self_index0 = self ? (unsigned)first : NO_INDEX;
        const float *cx = tplane[0] + first, *cy = tplane[1] + first, *cz = tplane[2] + first;
        if (want_acc)
            launch_pairs<true>(plan, st, plane[0], plane[1], plane[2], plane[3], plane[4], n_src, n_tiles, cx, cy, cz, n_chunk,
                               self_index0, d_partials);
        else
            launch_pairs<false>(plan, st, plane[0], plane[1], plane[2], plane[3], plane[4], n_src, n_tiles, cx, cy, cz, n_chunk,
                                self_index0, d_partials);
        TSP_HIP(hipGetLastError());
        hipLaunchKernelGGL(gravity_reduce_kernel, dim3((unsigned)((n_chunk + 255) / 256), (unsigned)nc), dim3(256), 0, st, d_partials, plan.splits,
                           LANES * plan.tpl, nc, cx, cy, cz, n_chunk, d_pot + first, d_acc + 3 * first, d_counts + 1);
        TSP_HIP(hipGetLastError());
        if (stats)
            fprintf(stderr, "tsp_gravity_direct: chunk first=%lld targets=%d per_lane=%d blocks=%d splits=%d tiles=%d\n",
                    (long long)first, n_chunk, plan.tpl, plan.blocks, plan.splits, n_tiles);
    }
    if (stats) TSP_HIP(hipEventRecord(ctx->ev[EV_T1], st));
    std::vector<double> result((size_t)n_tgt * (want_acc ? 4 : 1));
    TSP_HIP(hipMemcpyAsync(result.data(), d_pot, result.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    TSP_HIP(hipMemcpyAsync(counts, d_counts, sizeof(counts), hipMemcpyDeviceToHost, st));
    TSP_HIP(hipStreamSynchronize(st));
    float kernel_ms = 0.0f;
    if (stats) TSP_HIP(hipEventElapsedTime(&kernel_ms, ctx->ev[EV_T0], ctx->ev[EV_T1]));

    if (pot_out) memcpy(pot_out, result.data(), (size_t)n_tgt * sizeof(double));
    if (acc_out) memcpy(acc_out, result.data() + n_tgt, (size_t)3 * n_tgt * sizeof(double));
    if (info_out) {
        info_out->n_valid_sources = (int64_t)counts[0];
        info_out->n_valid_targets = (int64_t)counts[1];
    }
    if (stats)
        fprintf(stderr, "tsp_gravity_direct: n_src=%lld valid=%llu n_tgt=%lld valid=%llu acc=%d kernel_ms=%.4f pairs_per_s=%.4g\n",
                (long long)n_src, counts[0], (long long)n_tgt, counts[1], (int)want_acc, kernel_ms,
                kernel_ms > 0.0f ? (double)n_src * (double)n_tgt / (1e-3 * kernel_ms) : 0.0);
    return TSP_OK;
}

}  // namespace tsp
