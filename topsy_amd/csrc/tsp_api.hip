// tsp_api.hip -- the extern "C" boundary of libtopsy_splat (see include/topsy_splat.h).
//
// Each entry point cites the reference interface it replaces in the header.  Everything here is
// host-side plumbing: argument validation, HBM allocation, uploads, kernel dispatch, hipEvent
// timing (the TimeGpuOperation hook of reference src/topsy/util.py:76-115) and read-back.
#include <stdarg.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "tsp_cube_layout.h"
#include "tsp_hist2d_layout.h"
#include "tsp_internal.h"
#include "tsp_morton.h"

namespace tsp {

static thread_local char g_err[1024] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int alloc_group(tsp_context *ctx, std::initializer_list<DeviceBuffer> bufs, std::initializer_list<Capacity> caps) {
    for (const Capacity &c : caps) c.set(0);
    hipError_t freed = hipSuccess;
    for (const DeviceBuffer &b : bufs) {
        if (*b.p) {
            const hipError_t e = hipFree(*b.p);
            if (freed == hipSuccess) freed = e;
        }
        *b.p = nullptr;
    }
    if (freed != hipSuccess) {
        set_error("hipFree failed before allocating %s: %s", bufs.begin()->site, hipGetErrorString(freed));
        return TSP_EHIP;
    }
    for (const DeviceBuffer &b : bufs) {
        int rc = TSP_OK;
        if (ctx->debug_fail_alloc > 0 && --ctx->debug_fail_alloc == 0) {
            set_error("injected allocation failure at %s (debug_fail_alloc)", b.site);
            rc = TSP_ENOMEM;
        } else {
            const hipError_t e = hipMalloc(b.p, b.bytes);
            if (e != hipSuccess) {
                (void)hipGetLastError();     // (a later launch check must not report this allocation)
                *b.p = nullptr;
                set_error("hipMalloc of %zu bytes failed at %s: %s", b.bytes, b.site, hipGetErrorString(e));
                rc = e == hipErrorOutOfMemory ? TSP_ENOMEM : TSP_EHIP;
            }
        }
        if (rc != TSP_OK) {      // the group is all or nothing
            for (const DeviceBuffer &q : bufs) {
                if (*q.p) (void)hipFree(*q.p);
                *q.p = nullptr;
            }
            return rc;
        }
    }
    for (const Capacity &c : caps) c.set(c.value);
    return TSP_OK;
}

int scratch_alloc(tsp_context *ctx, const char *site, DeviceScratch &buf, size_t bytes) {
    TSP_REQUIRE(!buf.p, TSP_ESTATE, "scratch buffer of site %s is allocated twice", site);
    if (ctx->debug_fail_alloc > 0 && --ctx->debug_fail_alloc == 0) {
        set_error("injected allocation failure at %s (debug_fail_alloc)", site);
        return TSP_ENOMEM;
    }
    const hipError_t e = hipMalloc(&buf.p, bytes ? bytes : 16);
    if (e != hipSuccess) {
        (void)hipGetLastError();     // (a later launch check must not report this allocation)
        buf.p = nullptr;
        set_error("hipMalloc of %zu bytes failed at %s: %s", bytes, site, hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? TSP_ENOMEM : TSP_EHIP;
    }
    return TSP_OK;
}

int gather_scratch(tsp_context *ctx, DeviceScratch &dh, size_t h_bytes, DeviceScratch &da, size_t a_bytes) {
    TSP_SCRATCH_ALLOC(ctx, SITE("sph_sum_h"), dh, h_bytes);
    TSP_SCRATCH_ALLOC(ctx, SITE("sph_sum_a"), da, a_bytes);
    return TSP_OK;
}

int check_workspace(const tsp_context *ctx) {
    const Workspace &ws = ctx->ws;
    struct Pair { int64_t cap; const void *p; const char *name; } pairs[] = {
        {ws.mid_capacity, ws.mid_geom, "mid_geom"}, {ws.mid_capacity, ws.mid_w, "mid_w"},
        {ws.huge_capacity, ws.huge_geom, "huge_geom"}, {ws.huge_capacity, ws.huge_w, "huge_w"},
        {ws.hband_stride, ws.hband_geom, "hband_geom"}, {ws.hband_stride, ws.hband_w, "hband_w"}, {ws.hband_stride, ws.hband_count, "hband_count"},
        {ws.hband_bands, ws.hband_geom, "hband_geom"},
        {ws.mband_capacity, ws.mband_geom, "mband_geom"}, {ws.mband_capacity, ws.mband_w, "mband_w"},
        {ws.mitem_capacity, ws.mitem_tile, "mitem_tile"},
        {ws.mtile_capacity, ws.mband_count, "mband_count"}, {ws.mtile_capacity, ws.mband_base, "mband_base"},
        {ws.mtile_capacity, ws.mitem_base, "mitem_base"},
        {ws.chunk_capacity, ws.alive_list, "alive_list"},
        {ws.bounds_capacity, ws.block_bounds, "block_bounds"},
        {ws.range_capacity, ws.range_prefix, "range_prefix"},
        {ws.count_R, ws.count_diff, "count_diff"}, {ws.count_R, ws.count_band, "count_band"},
    };
    for (const Pair &q : pairs)
        TSP_REQUIRE(q.cap <= 0 || q.p, TSP_ESTATE, "workspace invariant broken: %s is null with capacity %lld", q.name, (long long)q.cap);
    return TSP_OK;
}

__global__ void image_to_float_kernel(const double *__restrict__ src, float *__restrict__ dst, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = (float)src[i];
}
__global__ void image_to_double_kernel(const float *__restrict__ src, double *__restrict__ dst, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = (double)src[i];
}

int launch_image_convert(tsp_context *ctx, bool to_float) {
    const int64_t n = (int64_t)ctx->R * ctx->R * ctx->C;
    const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, (int64_t)ctx->cu_count * 8);
    if (to_float) hipLaunchKernelGGL(image_to_float_kernel, dim3(grid), dim3(256), 0, ctx->stream, ctx->image64, ctx->image, n);
    else hipLaunchKernelGGL(image_to_double_kernel, dim3(grid), dim3(256), 0, ctx->stream, ctx->image, ctx->image64, n);
    TSP_HIP(hipGetLastError());
    return TSP_OK;
}

__global__ void gather_kernel(const float *__restrict__ src, const uint32_t *__restrict__ perm, float *__restrict__ dst,
                              int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = src[perm[i]];
}

// One attribute upload (tsp_upload_quantity / _rgb / _velocities): `count` caller-ordered host arrays src[] into the resident
// arrays *dst[], through the load-time permutation if one is active.  Everything the call needs is allocated before the first
// copy, kernel or change of state, so that a call that returns TSP_ENOMEM has changed nothing (include/topsy_splat.h): the
// staging buffer of the permutation (one serves every array of the call) and, when the attribute is not resident yet, its
// arrays as one group (`missing`; alloc_group frees what its pointers hold, so arrays that are resident are never handed to
// it).  `changed` runs once the memory is there, before the first copy: what the context forgets because the attribute changes.
template <typename F>
static int upload_attributes(tsp_context *ctx, const char *staging_site, float **const *dst, const float *const *src, int count,
                             bool resident, std::initializer_list<DeviceBuffer> missing, F changed) {
    const int64_t n = ctx->p.n;
    const size_t bytes = (size_t)n * sizeof(float);
    DeviceScratch tmp;
    if (ctx->p.perm) {
        const int rc = scratch_alloc(ctx, staging_site, tmp, bytes);
        if (rc) return rc;
    }
    if (!resident) {
        const int rc = alloc_group(ctx, missing, {});
        if (rc) return rc;
    }
    changed();
    for (int k = 0; k < count; ++k) {
        if (!ctx->p.perm) {
            TSP_HIP(hipMemcpyAsync(*dst[k], src[k], bytes, hipMemcpyHostToDevice, ctx->stream));
            continue;
        }
        TSP_HIP(hipMemcpyAsync(tmp.p, src[k], bytes, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(gather_kernel, dim3(2048), dim3(256), 0, ctx->stream, tmp.as<float>(), ctx->p.perm, *dst[k], n);
        TSP_HIP(hipGetLastError());
        TSP_HIP(hipStreamSynchronize(ctx->stream));      // (tmp takes the next array)
    }
    TSP_HIP(hipStreamSynchronize(ctx->stream));
    return TSP_OK;
}

static void free_particles(tsp_context *ctx) {
    Particles &p = ctx->p;
    float **arrs[] = {&p.x, &p.y, &p.z, &p.h, &p.m, &p.q, &p.r, &p.g, &p.b, &p.vx, &p.vy, &p.vz};
    for (float **a : arrs) {
        if (*a) (void)hipFree(*a);
        *a = nullptr;
    }
    float **derived[] = {&p.wm, &p.wr, &p.wg, &p.wb};
    for (float **a : derived) {
        if (*a) (void)hipFree(*a);
        *a = nullptr;
    }
    p.wm_valid = false;
    p.wrgb_source = W_NONE;
    if (p.perm) (void)hipFree(p.perm);
    p.perm = nullptr;
    p.n = 0;
    ctx->ws.bounds_valid = false;
    ctx->surface_keys = false;         // the keys name particles that are gone: a surface block must start with clear = 1
    ctx->forget_render_undo();
    ctx->strata_offsets.clear();
    ctx->cell_offsets.clear();
    ctx->cell_bits = 0;
}

// clips the ranges (starts, lens) of a render call to [0, n) and drops the empty ones (an indirect draw with instance_count 0
// draws nothing); no ranges = every particle.  Returns the particles they hold in *total.
static int clip_ranges(const tsp_context *ctx, const int64_t *starts, const int64_t *lens, int n_ranges, std::vector<int64_t> &s,
                       std::vector<int64_t> &l, int64_t *total) {
    if (!starts) {
        if (ctx->p.n > 0) { s.push_back(0); l.push_back(ctx->p.n); }
    } else {
        for (int i = 0; i < n_ranges; ++i) {
            TSP_REQUIRE(lens[i] >= 0, TSP_EINVAL, "range %d has negative length %lld", i, (long long)lens[i]);
            // clip without forming starts + lens (a caller may pass INT64_MAX for "to the end")
            int64_t b = starts[i], len = lens[i];
            if (b < 0) {
                len = (len > -b) ? len + b : 0;      // b > INT64_MIN + len, no overflow
                b = 0;
            }
            if (b >= ctx->p.n || len == 0) continue;
            if (len > ctx->p.n - b) len = ctx->p.n - b;
            s.push_back(b);
            l.push_back(len);
        }
    }
    *total = 0;
    for (int64_t v : l) *total += v;
    return TSP_OK;
}

static Camera make_camera(const tsp_context *ctx, const float *M, float scale_factor) {
    Camera cam;
    for (int i = 0; i < 12; ++i) cam.m[i] = M[i];
    cam.sf = scale_factor;
    cam.R = ctx->R;
    cam.Rf = (float)ctx->R;
    cam.halfR = 0.5f * cam.Rf;
    return cam;
}

}  // namespace tsp

using namespace tsp;

extern "C" {

const char *tsp_last_error(void) { return g_err; }
int tsp_version(void) { return 128; }     // 128: tsp_project_perspective and the struct tsp_perspective (perspective camera: the transformed snapshot into a second context); 127: tsp_histogram_2d and tsp_histogram_2d_layout and the structs tsp_hist2d_spec / tsp_hist2d_info (weighted 2-D histograms: phase diagrams); 126: tsp_spectral_cube and tsp_spectral_cube_layout (position-position-velocity cubes of the resident particles), option "cube_slice_particles"; 125: tsp_group_potential and tsp_halo_properties (halo properties); 124: tsp_gravity_tree and the struct tsp_gravity_tree_info (Barnes-Hut tree gravity over the Morton order); 123: tsp_gravity_direct and the struct tsp_gravity_info (softened direct-sum gravity: potential, accelerations); 122: tsp_sph_sample_lattice and the struct tsp_lattice (SPH sums at the points of a lattice); 121: a failed upload is atomic (attributes: nothing changed; particles / synthetic: no particles left; groups: every member emptied); 120: tsp_sph_velocity_gradient; 119: tsp_moment_sort, TSP_PRESENT_MOMENT_MEAN / _SIGMA (the kinematic maps as the base of tsp_present / tsp_present_yuv420); 118: tsp_render_undo, tsp_group_render all-or-nothing across the members; 117: kinematic maps (tsp_upload_velocities, tsp_set_line_of_sight, TSP_MODE_KINEMATIC, tsp_velocity_moments, tsp_colormap_moment); 116: tsp_radial_profile; 115: tsp_sphere_moments; 114: tsp_fof_groups; 113: tsp_shrink_sphere_center; 112: tsp_present_surface, tsp_present_surface_yuv420; 111: tsp_content_neg_inf; 110: tsp_sph_sum; 109: tsp_present_yuv420; 108: tsp_present; 107: surface rendering; 106: tsp_smoothing_lengths; 101: tsp_stats gained ms_mega, n_mega (16 bytes); 102: the per-kernel fragment counts (32 bytes); 103: n_chunk_culled (8 bytes); 104: matrix-core / kernel-I options removed; 105: kernel M's options removed (kernel G draws the mid footprints)
int tsp_stats_size(void) { return (int)sizeof(tsp_stats); }

int tsp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        set_error("hipGetDeviceCount failed");
        return TSP_ENODEV;
    }
    return n;
}

static int create_resources(tsp_context *ctx, int device_id, int resolution, int n_channels) {
    hipDeviceProp_t prop;
    TSP_HIP(hipGetDeviceProperties(&prop, device_id));
    ctx->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    TSP_HIP(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    TSP_HIP(hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking));
    for (auto &e : ctx->ev) TSP_HIP(hipEventCreate(&e));
    const size_t npx = (size_t)resolution * resolution;
    TSP_HIP(hipMalloc((void **)&ctx->image, npx * n_channels * sizeof(float)));
    TSP_HIP(hipMemsetAsync(ctx->image, 0, npx * n_channels * sizeof(float), ctx->stream));
    TSP_HIP(hipMalloc((void **)&ctx->image64, npx * n_channels * sizeof(double)));
    TSP_HIP(hipMemsetAsync(ctx->image64, 0, npx * n_channels * sizeof(double), ctx->stream));
    TSP_HIP(hipMalloc((void **)&ctx->mips, 2 * MIP_TOTAL * sizeof(float)));   // SPH kernel mips, then the sphere mips
    TSP_HIP(hipMalloc((void **)&ctx->counters, sizeof(Counters)));
    TSP_HIP(hipMemsetAsync(ctx->counters, 0, sizeof(Counters), ctx->stream));
    TSP_HIP(hipMalloc((void **)&ctx->out8, npx * 4));
    TSP_HIP(hipStreamSynchronize(ctx->stream));
    return TSP_OK;
}

int tsp_create(int device_id, int resolution, int n_channels, tsp_context **out) {
    TSP_REQUIRE(out != nullptr, TSP_EINVAL, "out is NULL");
    *out = nullptr;
    TSP_REQUIRE(resolution > 0 && resolution <= 16384, TSP_EINVAL, "resolution %d out of range", resolution);
    TSP_REQUIRE(n_channels == 2 || n_channels == 4, TSP_EINVAL, "n_channels must be 2 (SPH) or 4 (RGBSPH), got %d",
                n_channels);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("no HIP device available");
        return TSP_ENODEV;
    }
    TSP_REQUIRE(device_id >= 0 && device_id < ndev, TSP_ENODEV, "device %d not present (%d devices)", device_id, ndev);
    TSP_HIP(hipSetDevice(device_id));
    tsp_context *ctx = new tsp_context();
    ctx->device = device_id;
    ctx->R = resolution;
    ctx->C = n_channels;
    ctx->Ccap = n_channels;
    // a failed allocation (the float64 master image is R*R*C*8 bytes: 8.6 GB at 16384^2 x 4) must not leak the
    // streams, events and buffers created before it: tsp_destroy releases whatever exists (the error text stays)
    const int rc = create_resources(ctx, device_id, resolution, n_channels);
    if (rc != TSP_OK) {
        tsp_destroy(ctx);
        return rc;
    }
    *out = ctx;
    return TSP_OK;
}

void tsp_destroy(tsp_context *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    tsp_comm_destroy(ctx);
    free_particles(ctx);
    void *ptrs[] = {ctx->image, ctx->image64, ctx->image64_entry, ctx->mips, ctx->counters, ctx->out8, ctx->outf, ctx->lut, ctx->lut2d, ctx->scratch,
                    ctx->ws.mid_geom, ctx->ws.mid_w, ctx->ws.huge_geom, ctx->ws.huge_w, ctx->ws.hband_geom, ctx->ws.hband_w, ctx->ws.hband_count, ctx->ws.mband_geom, ctx->ws.mband_w, ctx->ws.mband_count, ctx->ws.mband_base, ctx->ws.mitem_tile, ctx->ws.mitem_base, 
                    ctx->ws.block_bounds, ctx->ws.alive_list, ctx->ws.cull_info, ctx->ws.range_prefix, ctx->ws.count_diff, ctx->ws.count_band, ctx->sort_keys, ctx->sort_keys_alt, ctx->sort_tmp};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    for (auto &e : ctx->ev)
        if (e) (void)hipEventDestroy(e);
    if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int tsp_set_kernel_mips(tsp_context *ctx, const float *lut, int n0, int n_levels) {
    TSP_REQUIRE(ctx && lut, TSP_EINVAL, "NULL argument");
    TSP_REQUIRE(n0 == 64 && n_levels == 4, TSP_EINVAL,
                "kernel texture must be 64^2 with 4 mip levels (reference sph.py:396), got n0=%d levels=%d", n0, n_levels);
    TSP_HIP(hipSetDevice(ctx->device));
    TSP_HIP(hipMemcpy(ctx->mips, lut, MIP_TOTAL * sizeof(float), hipMemcpyHostToDevice));
    ctx->have_mips = true;
    // does the kernel vanish outside the inscribed disc, on every mip level?  level l has n = 64 >> l
    // texels per side, texel (j, i) centre = -2 + (k + 0.5) * 4 / n
    bool zero = true;
    for (int l = 0, off = 0; l < 4 && zero; off += (64 >> l) * (64 >> l), ++l) {
        const int n = 64 >> l;
        for (int j = 0; j < n && zero; ++j)
            for (int i = 0; i < n; ++i) {
                const double x = -2.0 + (i + 0.5) * 4.0 / n, y = -2.0 + (j + 0.5) * 4.0 / n;
                if (x * x + y * y >= 4.0 && lut[off + j * n + i] != 0.0f) { zero = false; break; }
            }
    }
    ctx->lut_zero_outside_disc = zero;
    // mirror symmetry, bit for bit (kernel G then keeps one quadrant of every level in LDS)
    bool sym = true;
    for (int l = 0, off = 0; l < 4 && sym; off += (64 >> l) * (64 >> l), ++l) {
        const int n = 64 >> l;
        for (int j = 0; j < n && sym; ++j)
            for (int i = 0; i < n; ++i)
                if (memcmp(&lut[off + j * n + i], &lut[off + j * n + (n - 1 - i)], 4) || memcmp(&lut[off + j * n + i], &lut[off + (n - 1 - j) * n + i], 4)) { sym = false; break; }
    }
    ctx->lut_mirror_symmetric = sym;
    return TSP_OK;
}

int tsp_upload_particles(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, const float *h,
                         const float *mass) {
    TSP_REQUIRE(ctx, TSP_EINVAL, "NULL context");
    TSP_REQUIRE(n >= 0 && n < ((int64_t)1 << 32), TSP_EINVAL, "particle count %lld out of range", (long long)n);
    TSP_REQUIRE(n == 0 || (x && y && z && h), TSP_EINVAL, "NULL position/smoothing array");
    TSP_HIP(hipSetDevice(ctx->device));
    // The old snapshot goes first (keeping it would double the peak memory of a large one), so a call that fails leaves the
    // context with no particles at all, as after n = 0: p.n is set only once every array exists and holds its data
    free_particles(ctx);
    if (n == 0) return TSP_OK;
    Particles &p = ctx->p;
    const size_t bytes = (size_t)n * sizeof(float);
    int rc = alloc_group(ctx, {{"particles_x", (void **)&p.x, bytes}, {"particles_y", (void **)&p.y, bytes},
                               {"particles_z", (void **)&p.z, bytes}, {"particles_h", (void **)&p.h, bytes}}, {});
    if (!rc && mass) rc = alloc_group(ctx, {{"particles_mass", (void **)&p.m, bytes}}, {});
    if (!rc) {
        rc = [&]() -> int {
            float *const dst[] = {p.x, p.y, p.z, p.h, p.m};
            const float *const src[] = {x, y, z, h, mass};
            for (int k = 0; k < (mass ? 5 : 4); ++k) TSP_HIP(hipMemcpyAsync(dst[k], src[k], bytes, hipMemcpyHostToDevice, ctx->stream));
            TSP_HIP(hipStreamSynchronize(ctx->stream));
            return TSP_OK;
        }();
    }
    if (rc) {
        free_particles(ctx);         // (allocates nothing and leaves tsp_last_error alone)
        return rc;
    }
    p.n = n;
    return TSP_OK;
}

int tsp_upload_quantity(tsp_context *ctx, const float *q) {
    TSP_REQUIRE(ctx, TSP_EINVAL, "NULL context");
    TSP_REQUIRE(!q || ctx->p.n > 0, TSP_ESTATE, "upload particles before the quantity");
    TSP_HIP(hipSetDevice(ctx->device));
    Particles &p = ctx->p;
    if (!q) {
        ctx->forget_render_undo();                       // (an upload ends the validity of tsp_render_undo: topsy_splat.h)
        if (p.q) TSP_HIP(hipFree(p.q));
        p.q = nullptr;
        return TSP_OK;
    }
    float **const dst[] = {&p.q};
    const float *const src[] = {q};
    return upload_attributes(ctx, SITE("quantity_staging"), dst, src, 1, p.q != nullptr,
                             {{"quantity_q", (void **)&p.q, (size_t)p.n * sizeof(float)}}, [&]() { ctx->forget_render_undo(); });
}

int tsp_upload_rgb(tsp_context *ctx, const float *r, const float *g, const float *b) {
    TSP_REQUIRE(ctx && r && g && b, TSP_EINVAL, "NULL argument");
    TSP_REQUIRE(ctx->p.n > 0, TSP_ESTATE, "upload particles before rgb");
    TSP_HIP(hipSetDevice(ctx->device));
    Particles &p = ctx->p;
    const size_t bytes = (size_t)p.n * sizeof(float);
    float **const dst[] = {&p.r, &p.g, &p.b};
    const float *const src[] = {r, g, b};
    return upload_attributes(ctx, SITE("rgb_staging"), dst, src, 3, p.r && p.g && p.b,
                             {{"rgb_r", (void **)&p.r, bytes}, {"rgb_g", (void **)&p.g, bytes}, {"rgb_b", (void **)&p.b, bytes}}, [&]() {
                                 ctx->forget_render_undo();
                                 p.wrgb_source = W_NONE;      // (the cached weights were formed from the colours that go)
                             });
}

int tsp_upload_velocities(tsp_context *ctx, const float *vx, const float *vy, const float *vz) {
    TSP_REQUIRE(ctx, TSP_EINVAL, "NULL context");
    TSP_REQUIRE((vx && vy && vz) || (!vx && !vy && !vz), TSP_EINVAL, "vx, vy and vz must be given together or not at all");
    Particles &p = ctx->p;
    TSP_REQUIRE(!vx || p.n > 0, TSP_ESTATE, "upload particles before the velocities");
    TSP_HIP(hipSetDevice(ctx->device));
    const auto changed = [&]() {
        ctx->forget_render_undo();
        if (p.wrgb_source == W_KINEMATIC) p.wrgb_source = W_NONE;     // (the weights were formed from the velocities that go)
    };
    if (!vx) {
        changed();
        float **arrs[] = {&p.vx, &p.vy, &p.vz};
        for (float **a : arrs) {
            if (*a) TSP_HIP(hipFree(*a));
            *a = nullptr;
        }
        return TSP_OK;
    }
    const size_t bytes = (size_t)p.n * sizeof(float);
    float **const dst[] = {&p.vx, &p.vy, &p.vz};
    const float *const src[] = {vx, vy, vz};
    return upload_attributes(ctx, SITE("velocities_staging"), dst, src, 3, p.vx && p.vy && p.vz,
                             {{"velocities_x", (void **)&p.vx, bytes}, {"velocities_y", (void **)&p.vy, bytes},
                              {"velocities_z", (void **)&p.vz, bytes}}, changed);
}

int tsp_set_line_of_sight(tsp_context *ctx, const float axis[3], const float v_ref[3]) {
    TSP_REQUIRE(ctx && axis && v_ref, TSP_EINVAL, "NULL argument");
    double norm2 = 0.0;
    for (int k = 0; k < 3; ++k) {
        TSP_REQUIRE(std::isfinite(axis[k]) && std::isfinite(v_ref[k]), TSP_EINVAL, "axis and v_ref must be finite");
        norm2 += (double)axis[k] * (double)axis[k];
    }
    TSP_REQUIRE(std::fabs(std::sqrt(norm2) - 1.0) <= 1e-5, TSP_EINVAL, "axis must have unit length to 1e-5, not %.9g", std::sqrt(norm2));
    for (int k = 0; k < 3; ++k) {
        ctx->los[k] = axis[k] == 0.0f ? 0.0f : axis[k];                // (-0 and +0 are one line of sight)
        ctx->los[3 + k] = v_ref[k] == 0.0f ? 0.0f : v_ref[k];
    }
    ctx->have_los = true;
    return TSP_OK;
}

// one lane per particle; the magnitudes are read in the caller's order (through the load-time permutation, if any)
__global__ __launch_bounds__(256) void band_contraction_kernel(const double *__restrict__ mags, const double *__restrict__ weights,
                                                               int n_bands, int64_t n, const uint32_t *__restrict__ perm,
                                                               float *__restrict__ r, float *__restrict__ g, float *__restrict__ b) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t src = perm ? (int64_t)perm[i] : i;
        double acc[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < n_bands; ++k) {
            const double lum = pow(10.0, -0.4 * mags[(int64_t)k * n + src]);      // _effective_mass_for_band (loader.py:112-113)
            for (int c = 0; c < 3; ++c) {
                const double w = weights[c * n_bands + k];
                if (w != 0.0) acc[c] += w * lum;
            }
        }
        const float fr = (float)acc[0], fg = (float)acc[1], fb = (float)acc[2];
        r[i] = (fr != fr) ? 0.0f : fr;                                            // rgb[np.isnan(rgb)] = 0 (loader.py:120)
        g[i] = (fg != fg) ? 0.0f : fg;
        b[i] = (fb != fb) ? 0.0f : fb;
    }
}

int tsp_upload_band_magnitudes(tsp_context *ctx, int n_bands, const double *mags, const double *weights) {
    TSP_REQUIRE(ctx && mags && weights, TSP_EINVAL, "NULL argument");
    TSP_REQUIRE(n_bands >= 1 && n_bands <= 64, TSP_EINVAL, "n_bands %d out of range", n_bands);
    TSP_REQUIRE(ctx->p.n > 0, TSP_ESTATE, "upload particles before the band magnitudes");
    TSP_HIP(hipSetDevice(ctx->device));
    Particles &p = ctx->p;
    const int64_t n = p.n;
    // every allocation first, as in upload_attributes: resident colour arrays are written in place (n cannot have changed)
    DeviceScratch d_mags, d_w;
    TSP_SCRATCH_ALLOC(ctx, SITE("band_magnitudes"), d_mags, (size_t)n_bands * n * sizeof(double));
    TSP_SCRATCH_ALLOC(ctx, SITE("band_weights"), d_w, (size_t)3 * n_bands * sizeof(double));
    if (!(p.r && p.g && p.b)) {
        const size_t bytes = (size_t)n * sizeof(float);
        const int rc = alloc_group(ctx, {{"band_r", (void **)&p.r, bytes}, {"band_g", (void **)&p.g, bytes}, {"band_b", (void **)&p.b, bytes}}, {});
        if (rc) return rc;
    }
    ctx->forget_render_undo();
    p.wrgb_source = W_NONE;
    TSP_HIP(hipMemcpyAsync(d_mags.p, mags, (size_t)n_bands * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    TSP_HIP(hipMemcpyAsync(d_w.p, weights, (size_t)3 * n_bands * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, (int64_t)ctx->cu_count * 16);
    hipLaunchKernelGGL(band_contraction_kernel, dim3(grid), dim3(256), 0, ctx->stream, d_mags.as<double>(), d_w.as<double>(), n_bands, n,
                       p.perm, p.r, p.g, p.b);
    TSP_HIP(hipGetLastError());
    TSP_HIP(hipStreamSynchronize(ctx->stream));
    return TSP_OK;
}

int tsp_generate_synthetic(tsp_context *ctx, int64_t n_total, int64_t first, int64_t count, uint64_t seed, float h_cap,
                           int with_quantity, int with_rgb) {
    TSP_REQUIRE(ctx, TSP_EINVAL, "NULL context");
    TSP_REQUIRE(n_total > 0 && first >= 0 && count >= 0 && first + count <= n_total, TSP_EINVAL,
                "bad shard [%lld, +%lld) of %lld", (long long)first, (long long)count, (long long)n_total);
    TSP_REQUIRE(count < ((int64_t)1 << 32), TSP_EINVAL, "shard too large");
    TSP_HIP(hipSetDevice(ctx->device));
    free_particles(ctx);
    const int rc = generate_synthetic(ctx, n_total, first, count, seed, h_cap, with_quantity, with_rgb);
    if (rc) free_particles(ctx);     // as tsp_upload_particles: a failed call leaves no particles (tsp_last_error stays)
    return rc;
}

int tsp_get_strata_offsets(tsp_context *ctx, int64_t *offsets_out, int capacity) {
    if (!ctx || !offsets_out || capacity <= 0) return 0;
    const int n = (int)std::min<size_t>(ctx->strata_offsets.size(), (size_t)capacity);
    for (int i = 0; i < n; ++i) offsets_out[i] = ctx->strata_offsets[(size_t)i];
    return n;
}

int tsp_get_cell_layout(tsp_context *ctx, int *n_strata_out, int *cells_per_axis_out, float *box_lo_out, float *cell_width_out) {
    TSP_REQUIRE(ctx && n_strata_out && cells_per_axis_out && box_lo_out && cell_width_out, TSP_EINVAL, "NULL argument");
    TSP_REQUIRE(!ctx->cell_offsets.empty(), TSP_ESTATE, "the particles were never reordered (tsp_reorder_spatial)");
    *n_strata_out = (int)ctx->strata_offsets.size() - 1;
    *cells_per_axis_out = 1 << ctx->cell_bits;
    for (int a = 0; a < 3; ++a) {
        box_lo_out[a] = ctx->cell_lo[a];
        cell_width_out[a] = ctx->cell_width[a];
    }
    return TSP_OK;
}

int64_t tsp_get_cell_offsets(tsp_context *ctx, int64_t *offsets_out, int64_t capacity) {
    if (!ctx || !offsets_out || capacity <= 0) return 0;
    const int64_t n = std::min<int64_t>((int64_t)ctx->cell_offsets.size(), capacity);
    for (int64_t i = 0; i < n; ++i) offsets_out[i] = ctx->cell_offsets[(size_t)i];
    return n;
}

int tsp_reorder_spatial(tsp_context *ctx, int n_strata, uint64_t seed, int64_t *perm_out) {
    TSP_REQUIRE(ctx, TSP_EINVAL, "NULL context");
    TSP_REQUIRE(n_strata >= 1 && n_strata <= 4096, TSP_EINVAL, "n_strata %d out of range", n_strata);
    TSP_REQUIRE(ctx->p.n > 0, TSP_ESTATE, "no particles resident");
    TSP_HIP(hipSetDevice(ctx->device));
    return reorder_spatial(ctx, n_strata, seed, perm_out);
}

int64_t tsp_num_particles(tsp_context *ctx) { return ctx ? ctx->p.n : 0; }

int tsp_download_particles(tsp_context *ctx, float *x, float *y, float *z, float *h, float *mass, float *q, float *r,
                           float *g, float *b) {
    TSP_REQUIRE(ctx, TSP_EINVAL, "NULL context");
    TSP_HIP(hipSetDevice(ctx->device));
    const Particles &p = ctx->p;
    struct { float *dst; const float *src; const char *name; } items[] = {
        {x, p.x, "x"}, {y, p.y, "y"}, {z, p.z, "z"}, {h, p.h, "h"}, {mass, p.m, "mass"},
        {q, p.q, "q"}, {r, p.r, "r"}, {g, p.g, "g"}, {b, p.b, "b"}};
    for (auto &it : items) {
        if (!it.dst) continue;
        TSP_REQUIRE(it.src, TSP_ESTATE, "array '%s' is not resident", it.name);
        TSP_HIP(hipMemcpy(it.dst, it.src, (size_t)p.n * sizeof(float), hipMemcpyDeviceToHost));
    }
    return TSP_OK;
}

static int render_block(tsp_context *ctx, const float *M, float scale_factor, const int64_t *starts, const int64_t *lens,
                        int n_ranges, int clear, int mode, int flags, double *gpu_ms_out);

// A block draws whole or not at all (the reference's render loop, sph.py:306-332, cannot fail half-way): the float64 accumulator is
// copied aside on entry (one device-to-device copy of the image: ~10 us at 1024^2) and a block that fails after its first kernel
// has added to it -- an allocation for its record lists or bins, an injected test failure -- puts accumulator, channel layout and
// statistics back as the call found them; the float32 presentation image is only written by the last step of a successful block.
int tsp_render(tsp_context *ctx, const float *M, float scale_factor, const int64_t *starts, const int64_t *lens,
               int n_ranges, int clear, int mode, int flags, double *gpu_ms_out) {
    TSP_REQUIRE(ctx && M, TSP_EINVAL, "NULL argument");
    ctx->forget_render_undo();                           // (image64_entry is about to be overwritten)
    TSP_REQUIRE(clear || !ctx->surface_keys, TSP_ESTATE, "the accumulator holds the keys of tsp_render_surface: start with clear = 1");
    TSP_HIP(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)ctx->R * ctx->R * ctx->Ccap * sizeof(double);
    if (!ctx->image64_entry) {
        const int rc = alloc_group(ctx, {{"image64_entry", (void **)&ctx->image64_entry, bytes}}, {});
        if (rc) {
            if (!ctx->surface_keys) ctx->undo.kind = 2;      // (nothing was touched)
            return rc;
        }
    }
    TSP_HIP(hipMemcpyAsync(ctx->image64_entry, ctx->image64, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    const int C_entry = ctx->C;
    const tsp_stats stats_entry = ctx->stats;
    const int64_t culled_entry = ctx->chunk_culled_particles;
    const int source_entry = ctx->image_source;
    float los_entry[6];
    memcpy(los_entry, ctx->image_los, sizeof(los_entry));
    const int rc = render_block(ctx, M, scale_factor, starts, lens, n_ranges, clear, mode, flags, gpu_ms_out);
    if (rc != TSP_OK) {
        const std::string why = tsp_last_error();        // (the restore below must not replace the reason of the failure)
        ctx->C = C_entry; ctx->stats = stats_entry; ctx->chunk_culled_particles = culled_entry;
        // (option overlap_mid_huge: kernels N / G may still be adding into image64 on stream2 -- they finish before the copy)
        const hipError_t e0 = ctx->stream2 ? hipStreamSynchronize(ctx->stream2) : hipSuccess;
        const hipError_t e1 = hipMemcpyAsync(ctx->image64, ctx->image64_entry, bytes, hipMemcpyDeviceToDevice, ctx->stream);
        const hipError_t e2 = hipStreamSynchronize(ctx->stream);
        const hipError_t e = e0 != hipSuccess ? e0 : (e1 != hipSuccess ? e1 : e2);
        if (e != hipSuccess) set_error("%s; and the accumulator could not be restored (%s)", why.c_str(), hipGetErrorString(e));
        else set_error("%s", why.c_str());
        if (e == hipSuccess && !ctx->surface_keys) ctx->undo.kind = 2;
    } else {
        // what tsp_render_undo puts back (not over a surface image: its keys cannot be re-formed into the presentation image)
        if (!ctx->surface_keys) {
            ctx->undo.kind = 1;
            ctx->undo.C = C_entry; ctx->undo.stats = stats_entry; ctx->undo.chunk_culled_particles = culled_entry;
            ctx->undo.image_source = source_entry;
            memcpy(ctx->undo.image_los, los_entry, sizeof(los_entry));
        }
        ctx->surface_keys = false;
    }
    return rc;
}

// Takes back the last tsp_render: valid while no other call has changed the image since.  After a block that drew, the
// accumulator (image64_entry still holds it), the channel layout, the statistics and the image tags are put back as that call
// found them; after a block that failed, tsp_render has done so itself.  Either way the float32 presentation image is formed
// again from the accumulator and the context is marked not reduced: the state in which a device group sums its members again.
// Allocates nothing.
int tsp_render_undo(tsp_context *ctx) {
    TSP_REQUIRE(ctx, TSP_EINVAL, "NULL context");
    TSP_REQUIRE(ctx->undo.kind != 0, TSP_ESTATE, "nothing to undo: the last call that changed the image was not tsp_render");
    TSP_HIP(hipSetDevice(ctx->device));
    if (ctx->undo.kind == 1) {
        const size_t bytes = (size_t)ctx->R * ctx->R * ctx->Ccap * sizeof(double);
        if (ctx->stream2) TSP_HIP(hipStreamSynchronize(ctx->stream2));
        TSP_HIP(hipMemcpyAsync(ctx->image64, ctx->image64_entry, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        ctx->C = ctx->undo.C; ctx->stats = ctx->undo.stats; ctx->chunk_culled_particles = ctx->undo.chunk_culled_particles;
        ctx->image_source = ctx->undo.image_source;
        memcpy(ctx->image_los, ctx->undo.image_los, sizeof(ctx->image_los));
    }
    ctx->forget_render_undo();
    const int rc = launch_image_convert(ctx, true);
    if (rc) return rc;
    ctx->image_is_reduced = false;
    TSP_HIP(hipStreamSynchronize(ctx->stream));
    return TSP_OK;
}

static int render_block(tsp_context *ctx, const float *M, float scale_factor, const int64_t *starts, const int64_t *lens,
                        int n_ranges, int clear, int mode, int flags, double *gpu_ms_out) {
    TSP_REQUIRE(ctx && M, TSP_EINVAL, "NULL argument");
    TSP_REQUIRE(ctx->have_mips, TSP_ESTATE, "tsp_set_kernel_mips must be called before tsp_render");
    TSP_REQUIRE(mode == TSP_MODE_WEIGHTED || mode == TSP_MODE_DEPTH || mode == TSP_MODE_RGB || mode == TSP_MODE_KINEMATIC, TSP_EINVAL,
                "bad mode %d", mode);
    const bool kinematic = mode == TSP_MODE_KINEMATIC;
    // (no upload leaves n > 0 without these four: the check keeps a half-made context from ever reaching a kernel)
    TSP_REQUIRE(ctx->p.n == 0 || (ctx->p.x && ctx->p.y && ctx->p.z && ctx->p.h), TSP_ESTATE, "position / smoothing-length arrays not resident");
    if (kinematic) {
        TSP_REQUIRE(ctx->Ccap == 4, TSP_EINVAL, "TSP_MODE_KINEMATIC needs a 4-channel context");
        TSP_REQUIRE(!(flags & (TSP_PIPE_GENERIC | TSP_SAMPLE_BILINEAR_MIP0 | TSP_SAMPLE_BILINEAR_MIP)), TSP_EINVAL,
                    "TSP_MODE_KINEMATIC draws with the three-class pipeline only (flags must be TSP_PIPE_DEFAULT)");
        TSP_REQUIRE(ctx->p.n == 0 || ctx->p.m, TSP_ESTATE, "mass array not uploaded");
        TSP_REQUIRE(ctx->p.n == 0 || (ctx->p.vx && ctx->p.vy && ctx->p.vz), TSP_ESTATE, "velocities not uploaded (tsp_upload_velocities)");
        TSP_REQUIRE(ctx->have_los, TSP_ESTATE, "no line of sight set (tsp_set_line_of_sight)");
    } else if (mode == TSP_MODE_RGB) {
        TSP_REQUIRE(ctx->Ccap == 4, TSP_EINVAL, "TSP_MODE_RGB needs a 4-channel context");
        TSP_REQUIRE(ctx->p.n == 0 || (ctx->p.r && ctx->p.g && ctx->p.b), TSP_ESTATE, "rgb arrays not uploaded");
    } else {
        TSP_REQUIRE(ctx->p.n == 0 || ctx->p.m, TSP_ESTATE, "mass array not uploaded");
    }
    // the active channel count follows the mode (a 4-channel context can also hold 2-channel renders);
    // a block that does not clear must continue in the layout of the image it adds to
    const int newC = (mode == TSP_MODE_RGB || kinematic) ? 4 : 2;
    TSP_REQUIRE(clear || newC == ctx->C, TSP_ESTATE, "cannot accumulate a %d-channel block onto a %d-channel image",
                newC, ctx->C);
    // ... and, of the two 4-channel modes, in the one that started it, along the same line of sight
    const int source = newC == 4 ? (kinematic ? W_KINEMATIC : W_RGB) : W_NONE;
    if (!clear && newC == 4 && ctx->image_source != W_NONE) {
        TSP_REQUIRE(ctx->image_source == source, TSP_ESTATE, "cannot accumulate %s block onto %s image: start with clear = 1",
                    kinematic ? "a kinematic" : "an rgb", kinematic ? "an rgb" : "a kinematic");
        TSP_REQUIRE(!kinematic || !memcmp(ctx->image_los, ctx->los, sizeof(ctx->los)), TSP_ESTATE,
                    "the kinematic image was started along another line of sight (axis or v_ref): start with clear = 1");
    }
    ctx->C = newC;
    TSP_REQUIRE(n_ranges >= 0 && (n_ranges == 0 || (starts && lens) || (!starts && !lens)), TSP_EINVAL, "bad ranges");
    TSP_HIP(hipSetDevice(ctx->device));

    std::vector<int64_t> s, l;
    int64_t total = 0;
    if (int rc = clip_ranges(ctx, starts, lens, n_ranges, s, l, &total)) return rc;
    const int nr = (int)s.size();
    const Camera cam = make_camera(ctx, M, scale_factor);

    TSP_HIP(hipEventRecord(ctx->ev[EV_RENDER_BEGIN], ctx->stream));
    if (clear)
        TSP_HIP(hipMemsetAsync(ctx->image64, 0, (size_t)ctx->R * ctx->R * ctx->C * sizeof(double), ctx->stream));
    TSP_HIP(hipMemsetAsync(ctx->counters, 0, sizeof(Counters), ctx->stream));
    ctx->stats = tsp_stats{};
    ctx->stats.n_particles = total;
    ctx->chunk_culled_particles = 0;
    int rc = TSP_OK;
    if (total > 0) {
        const int rule = (flags & TSP_SAMPLE_BILINEAR_MIP0) ? 1 : ((flags & TSP_SAMPLE_BILINEAR_MIP) ? 2 : 0);
        if ((flags & TSP_PIPE_GENERIC) || rule != 0) {     // the alternative sampling rules exist in the generic kernel only
            // device copy of the ranges: starts | lens | prefix
            std::vector<int64_t> pack(3 * (size_t)nr + 1);
            int64_t acc = 0;
            for (int i = 0; i < nr; ++i) {
                pack[i] = s[i];
                pack[nr + i] = l[i];
                pack[2 * nr + i] = acc;
                acc += l[i];
            }
            pack[3 * nr] = acc;
            if (ctx->ws.range_capacity < (int64_t)pack.size()) {
                const int64_t cap = (int64_t)pack.size() * 2 + 64;
                if ((rc = alloc_group(ctx, {{"range_prefix_generic", (void **)&ctx->ws.range_prefix, (size_t)cap * sizeof(int64_t)}},
                                      {{&ctx->ws.range_capacity, cap}})))
                    return rc;
            }
            TSP_HIP(hipMemcpyAsync(ctx->ws.range_prefix, pack.data(), pack.size() * sizeof(int64_t),
                                   hipMemcpyHostToDevice, ctx->stream));
            rc = launch_generic(ctx, cam, ctx->ws.range_prefix, nr, total, mode, rule);
            // pack must outlive the async copy
            TSP_HIP(hipStreamSynchronize(ctx->stream));
        } else {
            ctx->kinematic_block = kinematic;      // (the rgb instantiation, fed the kinematic weights: ensure_weights)
            rc = launch_pipeline(ctx, cam, s.data(), l.data(), nr, total, kinematic ? (int)TSP_MODE_RGB : mode);
            ctx->kinematic_block = false;
        }
    }
    if (rc) return rc;
    if ((rc = launch_image_convert(ctx, true))) return rc;     // round the float64 master image once
    ctx->image_is_reduced = false;                             // `image` is this rank's partial image again
    ctx->image_source = source;
    if (kinematic) memcpy(ctx->image_los, ctx->los, sizeof(ctx->los));
    TSP_HIP(hipEventRecord(ctx->ev[EV_RENDER_END], ctx->stream));
    TSP_HIP(hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    TSP_HIP(hipEventElapsedTime(&ms, ctx->ev[EV_RENDER_BEGIN], ctx->ev[EV_RENDER_END]));
    ctx->stats.ms_total = ms;
    Counters hc;
    TSP_HIP(hipMemcpy(&hc, ctx->counters, sizeof(hc), hipMemcpyDeviceToHost));
    ctx->stats.n_small = (int64_t)hc.n_small;
    ctx->stats.n_mid = (int64_t)hc.n_mid;
    ctx->stats.n_huge = (int64_t)hc.n_huge;
    ctx->stats.n_mega = 0;
    ctx->stats.n_culled = (int64_t)hc.n_culled + ctx->chunk_culled_particles;
    ctx->stats.n_chunk_culled = ctx->chunk_culled_particles;
    ctx->stats.n_fragments = (int64_t)hc.n_fragments;
    ctx->stats.n_fragments_stream = (int64_t)hc.n_frag_class[0];
    ctx->stats.n_fragments_mid = (int64_t)hc.n_frag_class[1];
    ctx->stats.n_fragments_huge = (int64_t)hc.n_frag_class[2];
    ctx->stats.n_fragments_mega = (int64_t)hc.n_frag_class[3];      // (0 in the product build; the TSP_H2_DEBUG analysis build counts here)
    if (gpu_ms_out) *gpu_ms_out = ms;
    return TSP_OK;
}

int tsp_read_image(tsp_context *ctx, float *out) {
    TSP_REQUIRE(ctx && out, TSP_EINVAL, "NULL argument");
    TSP_HIP(hipSetDevice(ctx->device));
    TSP_HIP(hipMemcpy(out, ctx->image, (size_t)ctx->R * ctx->R * ctx->C * sizeof(float), hipMemcpyDeviceToHost));
    return TSP_OK;
}

int tsp_write_image(tsp_context *ctx, const float *in) {
    TSP_REQUIRE(ctx && in, TSP_EINVAL, "NULL argument");
    TSP_HIP(hipSetDevice(ctx->device));
    TSP_HIP(hipMemcpy(ctx->image, in, (size_t)ctx->R * ctx->R * ctx->C * sizeof(float), hipMemcpyHostToDevice));
    int rc = launch_image_convert(ctx, false);                 // keep the master copy consistent
    if (rc) return rc;
    ctx->forget_render_undo();
    ctx->image_is_reduced = false;
    ctx->surface_keys = false;
    TSP_HIP(hipStreamSynchronize(ctx->stream));
    return TSP_OK;
}

// The cross-shard SUM becomes this context's float32 presentation image (what read-back, colormap and autorange see); the
// float64 accumulator keeps the context's own partial sums, as after an in-place RCCL reduce (tsp_comm_reduce_image)
int tsp_set_reduced_image(tsp_context *ctx, const float *sum) {
    TSP_REQUIRE(ctx && sum, TSP_EINVAL, "NULL argument");
    TSP_REQUIRE(!ctx->image_is_reduced, TSP_ESTATE, "the render target was already reduced for this frame (call tsp_render before reducing again)");
    TSP_HIP(hipSetDevice(ctx->device));
    TSP_HIP(hipMemcpy(ctx->image, sum, (size_t)ctx->R * ctx->R * ctx->C * sizeof(float), hipMemcpyHostToDevice));
    ctx->forget_render_undo();
    ctx->image_is_reduced = true;
    return TSP_OK;
}

static int ensure_lut(tsp_context *ctx, const float *lut_rgba, int n_lut) {
    TSP_REQUIRE(lut_rgba && n_lut >= 2 && n_lut <= 65536, TSP_EINVAL, "bad colormap LUT (n=%d)", n_lut);
    if (ctx->lut_capacity < n_lut) {
        const int rc = alloc_group(ctx, {{"lut", (void **)&ctx->lut, (size_t)n_lut * 4 * sizeof(float)}}, {{&ctx->lut_capacity, n_lut}});
        if (rc) return rc;
    }
    TSP_HIP(hipMemcpyAsync(ctx->lut, lut_rgba, (size_t)n_lut * 4 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    return TSP_OK;
}

int tsp_colormap_scalar(tsp_context *ctx, const float *lut_rgba, int n_lut, float vmin, float vmax, int log_scale,
                        int weighted, uint8_t *out_rgba) {
    TSP_REQUIRE(ctx && out_rgba, TSP_EINVAL, "NULL argument");
    TSP_HIP(hipSetDevice(ctx->device));
    int rc = ensure_lut(ctx, lut_rgba, n_lut);
    if (rc) return rc;
    const int64_t npix = (int64_t)ctx->R * ctx->R;
    rc = launch_colormap_scalar(ctx, ctx->image, npix, ctx->C, ctx->lut, n_lut, vmin, vmax, log_scale, weighted, ctx->out8);
    if (rc) return rc;
    TSP_HIP(hipMemcpyAsync(out_rgba, ctx->out8, (size_t)npix * 4, hipMemcpyDeviceToHost, ctx->stream));
    TSP_HIP(hipStreamSynchronize(ctx->stream));
    return TSP_OK;
}

// the R * R * 4 float staging that the HDR rgb map and the moment maps share
static int ensure_outf(tsp_context *ctx) {
    if (ctx->outf) return TSP_OK;
    return alloc_group(ctx, {{"outf", (void **)&ctx->outf, (size_t)ctx->R * ctx->R * 4 * sizeof(float)}}, {});
}

// the moment maps of the kinematic presentation image into ctx->outf (on ctx->stream)
static int moment_maps(tsp_context *ctx) {
    TSP_REQUIRE(ctx->image_source == W_KINEMATIC && ctx->C == 4, TSP_ESTATE,
                "the image is not a kinematic one (render with TSP_MODE_KINEMATIC first)");
    TSP_HIP(hipSetDevice(ctx->device));
    if (int rc = ensure_outf(ctx)) return rc;
    return launch_velocity_moments(ctx, ctx->image, (int64_t)ctx->R * ctx->R, ctx->outf);
}

int tsp_velocity_moments(tsp_context *ctx, float *maps_out) {
    TSP_REQUIRE(ctx && maps_out, TSP_EINVAL, "NULL argument");
    if (int rc = moment_maps(ctx)) return rc;
    TSP_HIP(hipMemcpyAsync(maps_out, ctx->outf, (size_t)ctx->R * ctx->R * 4 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    TSP_HIP(hipStreamSynchronize(ctx->stream));
    return TSP_OK;
}

int tsp_colormap_moment(tsp_context *ctx, int which, const float *lut_rgba, int n_lut, float vmin, float vmax, int log_scale,
                        uint8_t *out_rgba8) {
    TSP_REQUIRE(ctx && out_rgba8, TSP_EINVAL, "NULL argument");
    TSP_REQUIRE(which == 1 || which == 2, TSP_EINVAL, "which must be 1 (mean) or 2 (sigma), not %d", which);
    TSP_REQUIRE(lut_rgba && n_lut >= 2 && n_lut <= 65536, TSP_EINVAL, "bad colormap LUT (n=%d)", n_lut);
    int rc = moment_maps(ctx);
    if (rc) return rc;
    if ((rc = ensure_lut(ctx, lut_rgba, n_lut))) return rc;
    const int64_t npix = (int64_t)ctx->R * ctx->R;
    // the scalar map, unweighted, reads the first float of every 4-float pixel: the maps shifted by `which` put the moment there
    if ((rc = launch_colormap_scalar(ctx, ctx->outf + which, npix, 4, ctx->lut, n_lut, vmin, vmax, log_scale, 0, ctx->out8))) return rc;
    TSP_HIP(hipMemcpyAsync(out_rgba8, ctx->out8, (size_t)npix * 4, hipMemcpyDeviceToHost, ctx->stream));
    TSP_HIP(hipStreamSynchronize(ctx->stream));
    return TSP_OK;
}

int tsp_colormap_rgb(tsp_context *ctx, float vmin, float vmax, float gamma, uint8_t *out_rgba8, float *out_rgba_f32) {
    TSP_REQUIRE(ctx && (out_rgba8 || out_rgba_f32), TSP_EINVAL, "NULL argument");
    TSP_REQUIRE(ctx->C == 4, TSP_EINVAL, "rgb colormap needs a 4-channel image");
    TSP_HIP(hipSetDevice(ctx->device));
    const int64_t npix = (int64_t)ctx->R * ctx->R;
    int rc;
    if (out_rgba_f32 && (rc = ensure_outf(ctx))) return rc;
    rc = launch_colormap_rgb(ctx, ctx->image, npix, ctx->C, vmin, vmax, gamma, out_rgba8 ? ctx->out8 : nullptr,
                                 out_rgba_f32 ? ctx->outf : nullptr);
    if (rc) return rc;
    if (out_rgba8) TSP_HIP(hipMemcpyAsync(out_rgba8, ctx->out8, (size_t)npix * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (out_rgba_f32)
        TSP_HIP(hipMemcpyAsync(out_rgba_f32, ctx->outf, (size_t)npix * 16, hipMemcpyDeviceToHost, ctx->stream));
    TSP_HIP(hipStreamSynchronize(ctx->stream));
    return TSP_OK;
}

int tsp_colormap_set_lut2d(tsp_context *ctx, const float *lut_rgba, int n) {
    TSP_REQUIRE(ctx && lut_rgba && n >= 2 && n <= 4096, TSP_EINVAL, "bad 2-D colormap LUT (n=%d)", n);
    TSP_HIP(hipSetDevice(ctx->device));
    if (ctx->lut2d_n != n || !ctx->lut2d) {      // (a failed allocation leaves "no LUT")
        const int rc = alloc_group(ctx, {{"lut2d", (void **)&ctx->lut2d, (size_t)n * n * 4 * sizeof(float)}}, {{&ctx->lut2d_n, n}});
        if (rc) return rc;
    }
    TSP_HIP(hipMemcpy(ctx->lut2d, lut_rgba, (size_t)n * n * 4 * sizeof(float), hipMemcpyHostToDevice));
    return TSP_OK;
}

int tsp_colormap_bivariate(tsp_context *ctx, float vmin, float vmax, float density_vmin, float density_vmax, int log_scale,
                           int weighted, uint8_t *out_rgba) {
    TSP_REQUIRE(ctx && out_rgba, TSP_EINVAL, "NULL argument");
    TSP_REQUIRE(ctx->lut2d, TSP_ESTATE, "tsp_colormap_set_lut2d must be called first");
    TSP_HIP(hipSetDevice(ctx->device));
    const int64_t npix = (int64_t)ctx->R * ctx->R;
    int rc = launch_colormap_bivariate(ctx, ctx->image, npix, ctx->C, vmin, vmax, density_vmin, density_vmax, log_scale, weighted,
                                       ctx->out8);
    if (rc) return rc;
    TSP_HIP(hipMemcpyAsync(out_rgba, ctx->out8, (size_t)npix * 4, hipMemcpyDeviceToHost, ctx->stream));
    TSP_HIP(hipStreamSynchronize(ctx->stream));
    return TSP_OK;
}

// Host-image colormaps: the context's scratch holds the input and up to two outputs behind it, each at a 256-byte boundary.
struct HostStage { float *in; uint8_t *out8; float *outf; };
static int stage_host_image(tsp_context *ctx, size_t in_bytes, size_t out8_bytes, size_t outf_bytes, HostStage &hs) {
    const size_t a_in = (in_bytes + 255) & ~(size_t)255, a_o8 = (out8_bytes + 255) & ~(size_t)255, bytes = a_in + a_o8 + outf_bytes;
    if (ctx->scratch_bytes < bytes)
        if (int rc = alloc_group(ctx, {{"colormap_scratch", &ctx->scratch, bytes}}, {{&ctx->scratch_bytes, (int64_t)bytes}})) return rc;
    hs.in = (float *)ctx->scratch;
    hs.out8 = (uint8_t *)ctx->scratch + a_in;
    hs.outf = (float *)(hs.out8 + a_o8);
    return TSP_OK;
}
// the outputs the caller asked for back to the host, then the stream is drained
static int unstage_host_image(tsp_context *ctx, const HostStage &hs, uint8_t *out8, size_t out8_bytes, float *outf, size_t outf_bytes) {
    if (out8) TSP_HIP(hipMemcpyAsync(out8, hs.out8, out8_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (outf) TSP_HIP(hipMemcpyAsync(outf, hs.outf, outf_bytes, hipMemcpyDeviceToHost, ctx->stream));
    TSP_HIP(hipStreamSynchronize(ctx->stream));
    return TSP_OK;
}

int tsp_colormap_scalar_host(tsp_context *ctx, const float *img, int H, int W, int C, const float *lut_rgba, int n_lut,
                             float vmin, float vmax, int log_scale, int weighted, uint8_t *out_rgba) {
    TSP_REQUIRE(ctx && img && out_rgba, TSP_EINVAL, "NULL argument");
    TSP_REQUIRE(H > 0 && W > 0 && C >= 2, TSP_EINVAL, "bad image shape %dx%dx%d", H, W, C);
    TSP_HIP(hipSetDevice(ctx->device));
    const int64_t npix = (int64_t)H * W;
    const size_t in_bytes = (size_t)npix * C * sizeof(float), out_bytes = (size_t)npix * 4;
    HostStage hs;
    int rc = stage_host_image(ctx, in_bytes, out_bytes, 0, hs);
    if (rc) return rc;
    if ((rc = ensure_lut(ctx, lut_rgba, n_lut))) return rc;
    TSP_HIP(hipMemcpyAsync(hs.in, img, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = launch_colormap_scalar(ctx, hs.in, npix, C, ctx->lut, n_lut, vmin, vmax, log_scale, weighted, hs.out8)))
        return rc;
    return unstage_host_image(ctx, hs, out_rgba, out_bytes, nullptr, 0);
}

int tsp_colormap_bivariate_host(tsp_context *ctx, const float *img, int H, int W, int C, float vmin, float vmax,
                                float density_vmin, float density_vmax, int log_scale, int weighted, uint8_t *out_rgba) {
    TSP_REQUIRE(ctx && img && out_rgba, TSP_EINVAL, "NULL argument");
    TSP_REQUIRE(H > 0 && W > 0 && C >= 2, TSP_EINVAL, "bad image shape %dx%dx%d", H, W, C);
    TSP_REQUIRE(ctx->lut2d, TSP_ESTATE, "tsp_colormap_set_lut2d must be called first");
    TSP_HIP(hipSetDevice(ctx->device));
    const int64_t npix = (int64_t)H * W;
    const size_t in_bytes = (size_t)npix * C * sizeof(float), out_bytes = (size_t)npix * 4;
    HostStage hs;
    int rc = stage_host_image(ctx, in_bytes, out_bytes, 0, hs);
    if (rc) return rc;
    TSP_HIP(hipMemcpyAsync(hs.in, img, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = launch_colormap_bivariate(ctx, hs.in, npix, C, vmin, vmax, density_vmin, density_vmax, log_scale, weighted, hs.out8)))
        return rc;
    return unstage_host_image(ctx, hs, out_rgba, out_bytes, nullptr, 0);
}

int tsp_colormap_rgb_host(tsp_context *ctx, const float *img, int H, int W, int C, float vmin, float vmax, float gamma,
                          uint8_t *out_rgba8, float *out_rgba_f32) {
    TSP_REQUIRE(ctx && img && (out_rgba8 || out_rgba_f32), TSP_EINVAL, "NULL argument");
    TSP_REQUIRE(H > 0 && W > 0 && C >= 3, TSP_EINVAL, "bad image shape %dx%dx%d", H, W, C);
    TSP_HIP(hipSetDevice(ctx->device));
    const int64_t npix = (int64_t)H * W;
    const size_t in_bytes = (size_t)npix * C * sizeof(float), o8 = (size_t)npix * 4, of = (size_t)npix * 16;
    HostStage hs;
    int rc = stage_host_image(ctx, in_bytes, o8, of, hs);
    if (rc) return rc;
    TSP_HIP(hipMemcpyAsync(hs.in, img, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = launch_colormap_rgb(ctx, hs.in, npix, C, vmin, vmax, gamma, out_rgba8 ? hs.out8 : nullptr,
                                  out_rgba_f32 ? hs.outf : nullptr)))
        return rc;
    return unstage_host_image(ctx, hs, out_rgba8, o8, out_rgba_f32, of);
}

// what a k-nearest-neighbour search accepts (tsp_smoothing_lengths, tsp_sph_sample_lattice)
static int check_neighbour_search(int64_t n, int n_neighbours, float period) {
    TSP_REQUIRE(n >= 1 && n < (1ll << 31), TSP_EINVAL, "n = %lld outside [1, 2^31)", (long long)n);
    TSP_REQUIRE(n_neighbours >= 2 && n_neighbours <= 64, TSP_EINVAL, "n_neighbours = %d outside [2, 64]", n_neighbours);
    TSP_REQUIRE(period == 0.0f || (std::isfinite(period) && period > 0.0f), TSP_EINVAL,
                "period must be 0 (open box) or finite and > 0, not %g", (double)period);
    TSP_REQUIRE(n >= n_neighbours, TSP_EINVAL, "%lld particles, n_neighbours = %d", (long long)n, n_neighbours);
    return TSP_OK;
}

int tsp_smoothing_lengths(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, int n_neighbours,
                          float period, float *h_out) {
    TSP_REQUIRE(ctx && x && y && z && h_out, TSP_EINVAL, "NULL argument");
    if (const int rc = check_neighbour_search(n, n_neighbours, period)) return rc;
    TSP_HIP(hipSetDevice(ctx->device));
    return smoothing_lengths(ctx, n, x, y, z, n_neighbours, period == 0.0f ? 0.0f : period, h_out);
}

int tsp_sph_sum(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, const float *h, const float *a,
                float period, float *out) {
    TSP_REQUIRE(ctx && x && y && z && h && a && out, TSP_EINVAL, "NULL argument");
    TSP_REQUIRE(n >= 1 && n < (1ll << 31), TSP_EINVAL, "n = %lld outside [1, 2^31)", (long long)n);
    TSP_REQUIRE(period == 0.0f || (std::isfinite(period) && period > 0.0f), TSP_EINVAL,
                "period must be 0 (open box) or finite and > 0, not %g", (double)period);
    TSP_HIP(hipSetDevice(ctx->device));
    const float *fields[1] = {a};
    float *outs[1] = {out};
    return sph_sum(ctx, n, x, y, z, h, SPH_GATHER_SUM, fields, 1, period == 0.0f ? 0.0f : period, outs, 1);
}

int tsp_sph_velocity_gradient(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, const float *h,
                              const float *mass, const float *rho, const float *vx, const float *vy, const float *vz, float period,
                              float *div_out, float *curl_x_out, float *curl_y_out, float *curl_z_out) {
    TSP_REQUIRE(ctx && x && y && z && h && mass && rho && vx && vy && vz && div_out && curl_x_out && curl_y_out && curl_z_out,
                TSP_EINVAL, "NULL argument");
    TSP_REQUIRE(n >= 1 && n < (1ll << 31), TSP_EINVAL, "n = %lld outside [1, 2^31)", (long long)n);
    TSP_REQUIRE(period == 0.0f || (std::isfinite(period) && period > 0.0f), TSP_EINVAL,
                "period must be 0 (open box) or finite and > 0, not %g", (double)period);
    TSP_HIP(hipSetDevice(ctx->device));
    const float *fields[5] = {mass, rho, vx, vy, vz};
    float *outs[4] = {div_out, curl_x_out, curl_y_out, curl_z_out};
    return sph_sum(ctx, n, x, y, z, h, SPH_GATHER_VELOCITY_GRADIENT, fields, 5, period == 0.0f ? 0.0f : period, outs, 4);
}

int tsp_sph_sample_lattice(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, int n_fields,
                           const float *const *fields, int n_neighbours, float period, const tsp_lattice *lattice, float *h_out,
                           float *const *outs) {
    TSP_REQUIRE(ctx && x && y && z && fields && lattice && outs, TSP_EINVAL, "NULL argument");
    TSP_REQUIRE(n_fields >= 1 && n_fields <= 4, TSP_EINVAL, "n_fields = %d outside [1, 4]", n_fields);
    for (int f = 0; f < n_fields; ++f) TSP_REQUIRE(fields[f] && outs[f], TSP_EINVAL, "NULL field or output %d", f);
    if (const int rc = check_neighbour_search(n, n_neighbours, period)) return rc;
    const tsp_lattice &lat = *lattice;
    TSP_REQUIRE(lat.nu >= 1 && lat.nv >= 1 && lat.nw >= 1, TSP_EINVAL, "lattice of %d x %d x %d points", lat.nu, lat.nv, lat.nw);
    TSP_REQUIRE((int64_t)lat.nu * lat.nv < (1ll << 31) && (int64_t)lat.nu * lat.nv * lat.nw < (1ll << 31), TSP_EINVAL,
                "lattice of %d x %d x %d points: 2^31 or more", lat.nu, lat.nv, lat.nw);
    for (int a = 0; a < 3; ++a)
        TSP_REQUIRE(std::isfinite(lat.origin[a]) && std::isfinite(lat.du[a]) && std::isfinite(lat.dv[a]) && std::isfinite(lat.dw[a]),
                    TSP_EINVAL, "the lattice has a non-finite number on axis %d", a);
    // every coordinate is affine in (i, j, k), and so is every partial sum of the rule: the extremes are at the corners
    for (int corner = 0; corner < 8; ++corner) {
        float p[3];
        lattice_point(lat, corner & 1 ? lat.nu - 1 : 0, corner & 2 ? lat.nv - 1 : 0, corner & 4 ? lat.nw - 1 : 0, p[0], p[1], p[2]);
        TSP_REQUIRE(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]), TSP_EINVAL,
                    "a corner of the lattice, (%g, %g, %g), is not a finite float32", (double)p[0], (double)p[1], (double)p[2]);
    }
    TSP_HIP(hipSetDevice(ctx->device));
    return sph_sample_lattice(ctx, n, x, y, z, n_fields, fields, n_neighbours, period == 0.0f ? 0.0f : period, lattice, h_out, outs);
}

int tsp_shrink_sphere_center(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, const float *mass,
                             float mass_cut_factor, double r_start, double shrink_factor, int64_t min_particles,
                             int max_iterations, double center_out[3], tsp_center_info *info_out) {
    TSP_REQUIRE(ctx && x && y && z && mass && center_out, TSP_EINVAL, "NULL argument");
    TSP_REQUIRE(n >= 1 && n < (1ll << 31), TSP_EINVAL, "n = %lld outside [1, 2^31)", (long long)n);
    TSP_REQUIRE(shrink_factor > 0.0 && shrink_factor < 1.0, TSP_EINVAL, "shrink_factor = %g outside (0, 1)", shrink_factor);
    TSP_REQUIRE(min_particles >= 1, TSP_EINVAL, "min_particles = %lld below 1", (long long)min_particles);
    TSP_REQUIRE(max_iterations >= 0 && max_iterations <= 256, TSP_EINVAL, "max_iterations = %d outside [0, 256]", max_iterations);
    TSP_REQUIRE(std::isfinite(r_start) && r_start >= 0.0, TSP_EINVAL, "r_start must be 0 (estimated) or finite and > 0, not %g", r_start);
    TSP_REQUIRE(mass_cut_factor == 0.0f || (std::isfinite(mass_cut_factor) && mass_cut_factor > 1.0f), TSP_EINVAL,
                "mass_cut_factor must be 0 (no selection) or finite and > 1, not %g", (double)mass_cut_factor);
    TSP_HIP(hipSetDevice(ctx->device));
    return shrink_sphere_center(ctx, n, x, y, z, mass, mass_cut_factor == 0.0f ? 0.0f : mass_cut_factor, r_start == 0.0 ? 0.0 : r_start,
                                shrink_factor, min_particles, max_iterations, center_out, info_out);
}

int tsp_fof_groups(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, float linking_length, float period,
                   int64_t min_members, int32_t *group_out, tsp_fof_info *info_out) {
    TSP_REQUIRE(ctx && x && y && z && group_out, TSP_EINVAL, "NULL argument");
    TSP_REQUIRE(n >= 1 && n < (1ll << 31), TSP_EINVAL, "n = %lld outside [1, 2^31)", (long long)n);
    TSP_REQUIRE(std::isfinite(linking_length) && linking_length > 0.0f, TSP_EINVAL, "linking_length must be finite and > 0, not %g",
                (double)linking_length);
    TSP_REQUIRE(period == 0.0f || (std::isfinite(period) && period > 0.0f), TSP_EINVAL,
                "period must be 0 (open box) or finite and > 0, not %g", (double)period);
    TSP_REQUIRE(period == 0.0f || linking_length < 0.5f * period, TSP_EINVAL, "linking_length = %g must be below period / 2 = %g",
                (double)linking_length, 0.5 * (double)period);
    TSP_REQUIRE(min_members >= 1, TSP_EINVAL, "min_members = %lld below 1", (long long)min_members);
    TSP_HIP(hipSetDevice(ctx->device));
    return fof_groups(ctx, n, x, y, z, linking_length, period == 0.0f ? 0.0f : period, min_members, group_out, info_out);
}

int tsp_sphere_moments(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, const float *mass,
                       const float *vx, const float *vy, const float *vz, const double center[3], double r, double r_vel,
                       tsp_moments *out) {
    TSP_REQUIRE(ctx && x && y && z && mass && center && out, TSP_EINVAL, "NULL argument");
    TSP_REQUIRE((vx && vy && vz) || (!vx && !vy && !vz), TSP_EINVAL, "vx, vy and vz must be given together or not at all");
    TSP_REQUIRE(n >= 1 && n < (1ll << 31), TSP_EINVAL, "n = %lld outside [1, 2^31)", (long long)n);
    TSP_REQUIRE(std::isfinite(center[0]) && std::isfinite(center[1]) && std::isfinite(center[2]), TSP_EINVAL,
                "center = (%g, %g, %g) is not finite", center[0], center[1], center[2]);
    TSP_REQUIRE(std::isfinite(r) && r > 0.0, TSP_EINVAL, "r must be finite and > 0, not %g", r);
    if (vx)
        TSP_REQUIRE(std::isfinite(r_vel) && r_vel > 0.0 && r_vel <= r, TSP_EINVAL,
                    "with velocities r_vel must be finite with 0 < r_vel <= r = %g, not %g", r, r_vel);
    else
        TSP_REQUIRE(r_vel == 0.0, TSP_EINVAL, "without velocities r_vel must be 0, not %g", r_vel);
    TSP_HIP(hipSetDevice(ctx->device));
    return sphere_moments(ctx, n, x, y, z, mass, vx, vy, vz, center, r, r_vel == 0.0 ? 0.0 : r_vel, out);
}

int tsp_radial_profile(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, const float *mass,
                       const float *vx, const float *vy, const float *vz, const tsp_profile_spec *spec, int64_t *count_out,
                       double *sums_out, tsp_profile_info *info_out) {
    TSP_REQUIRE(ctx && x && y && z && mass && spec && count_out && sums_out, TSP_EINVAL, "NULL argument");
    TSP_REQUIRE((vx && vy && vz) || (!vx && !vy && !vz), TSP_EINVAL, "vx, vy and vz must be given together or not at all");
    TSP_REQUIRE(n >= 1 && n < (1ll << 31), TSP_EINVAL, "n = %lld outside [1, 2^31)", (long long)n);
    TSP_REQUIRE(spec->geometry == 0 || spec->geometry == 1, TSP_EINVAL, "geometry = %d is neither 0 (shells) nor 1 (annuli)",
                (int)spec->geometry);
    TSP_REQUIRE(spec->n_bins >= 1 && spec->n_bins <= 512, TSP_EINVAL, "n_bins = %d outside [1, 512]", (int)spec->n_bins);
    TSP_REQUIRE(spec->edges, TSP_EINVAL, "NULL edges");
    TSP_REQUIRE(std::isfinite(spec->edges[0]) && spec->edges[0] >= 0.0, TSP_EINVAL, "edges[0] must be finite and >= 0, not %g",
                spec->edges[0]);
    for (int k = 1; k <= spec->n_bins; ++k)
        TSP_REQUIRE(std::isfinite(spec->edges[k]) && spec->edges[k] > spec->edges[k - 1], TSP_EINVAL,
                    "edges must be finite and strictly ascending: edges[%d] = %g after %g", k, spec->edges[k], spec->edges[k - 1]);
    TSP_REQUIRE(std::isfinite(spec->center[0]) && std::isfinite(spec->center[1]) && std::isfinite(spec->center[2]), TSP_EINVAL,
                "center = (%g, %g, %g) is not finite", spec->center[0], spec->center[1], spec->center[2]);
    if (vx)
        TSP_REQUIRE(std::isfinite(spec->v_cen[0]) && std::isfinite(spec->v_cen[1]) && std::isfinite(spec->v_cen[2]), TSP_EINVAL,
                    "v_cen = (%g, %g, %g) is not finite", spec->v_cen[0], spec->v_cen[1], spec->v_cen[2]);
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) {
            const double *a = spec->frame + 3 * i, *b = spec->frame + 3 * j;
            const double dot = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
            TSP_REQUIRE(std::fabs(dot - (i == j ? 1.0 : 0.0)) <= 1e-6, TSP_EINVAL,
                        "frame is not a rotation: rows %d and %d have the product %g", i, j, dot);      // (NaN fails too)
        }
    if (spec->geometry == 1)
        TSP_REQUIRE(spec->half_height > 0.0, TSP_EINVAL, "half_height must be > 0 or +inf, not %g", spec->half_height);
    TSP_HIP(hipSetDevice(ctx->device));
    return radial_profile(ctx, n, x, y, z, mass, vx, vy, vz, spec, count_out, sums_out, info_out);
}

int tsp_gravity_direct(tsp_context *ctx, int64_t n_src, const float *sx, const float *sy, const float *sz, const float *mass,
                       const float *eps, float eps_all, int64_t n_tgt, const float *tx, const float *ty, const float *tz,
                       double *pot_out, double *acc_out, tsp_gravity_info *info_out) {
    TSP_REQUIRE(ctx && sx && sy && sz && mass, TSP_EINVAL, "NULL argument");
    TSP_REQUIRE((tx && ty && tz) || (!tx && !ty && !tz), TSP_EINVAL, "tx, ty and tz must be given together or not at all");
    TSP_REQUIRE(pot_out || acc_out, TSP_EINVAL, "neither pot_out nor acc_out is given");
    TSP_REQUIRE(n_src >= 1 && n_src < (1ll << 31), TSP_EINVAL, "n_src = %lld outside [1, 2^31)", (long long)n_src);
    TSP_REQUIRE(n_tgt >= 1 && n_tgt < (1ll << 31), TSP_EINVAL, "n_tgt = %lld outside [1, 2^31)", (long long)n_tgt);
    TSP_REQUIRE(tx || n_tgt == n_src, TSP_EINVAL, "without targets n_tgt must be n_src = %lld, not %lld", (long long)n_src,
                (long long)n_tgt);
    if (!eps) TSP_REQUIRE(std::isfinite(eps_all) && eps_all >= 0.0f, TSP_EINVAL, "eps_all must be finite and >= 0, not %g", (double)eps_all);
    TSP_HIP(hipSetDevice(ctx->device));
    return gravity_direct(ctx, n_src, sx, sy, sz, mass, eps, eps_all, n_tgt, tx, ty, tz, pot_out, acc_out, info_out);
}

int tsp_gravity_tree(tsp_context *ctx, int64_t n_src, const float *sx, const float *sy, const float *sz, const float *mass,
                     const float *eps, float eps_all, int64_t n_tgt, const float *tx, const float *ty, const float *tz, float theta,
                     double *pot_out, double *acc_out, tsp_gravity_tree_info *info_out) {
    TSP_REQUIRE(ctx && sx && sy && sz && mass, TSP_EINVAL, "NULL argument");
    TSP_REQUIRE((tx && ty && tz) || (!tx && !ty && !tz), TSP_EINVAL, "tx, ty and tz must be given together or not at all");
    TSP_REQUIRE(pot_out || acc_out, TSP_EINVAL, "neither pot_out nor acc_out is given");
    TSP_REQUIRE(n_src >= 1 && n_src < (1ll << 31), TSP_EINVAL, "n_src = %lld outside [1, 2^31)", (long long)n_src);
    TSP_REQUIRE(n_tgt >= 1 && n_tgt < (1ll << 31), TSP_EINVAL, "n_tgt = %lld outside [1, 2^31)", (long long)n_tgt);
    TSP_REQUIRE(tx || n_tgt == n_src, TSP_EINVAL, "without targets n_tgt must be n_src = %lld, not %lld", (long long)n_src,
                (long long)n_tgt);
    if (!eps) TSP_REQUIRE(std::isfinite(eps_all) && eps_all >= 0.0f, TSP_EINVAL, "eps_all must be finite and >= 0, not %g", (double)eps_all);
    TSP_REQUIRE(std::isfinite(theta) && theta >= 0.0f && theta <= 1.0f, TSP_EINVAL, "theta = %g outside [0, 1]", (double)theta);
    for (int64_t j = 0; j < n_src; ++j)      // (NaN passes: that source is left out)
        TSP_REQUIRE(!(mass[j] < 0.0f), TSP_EINVAL, "mass[%lld] = %g is negative: a centre of mass needs masses >= 0", (long long)j,
                    (double)mass[j]);
    TSP_HIP(hipSetDevice(ctx->device));
    return gravity_tree(ctx, n_src, sx, sy, sz, mass, eps, eps_all, n_tgt, tx, ty, tz, theta, pot_out, acc_out, info_out);
}

int tsp_group_potential(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, const float *mass,
                        const float *eps, float eps_all, const int32_t *group, int64_t n_groups, double period, int64_t max_members,
                        double *phi_out, tsp_group_potential_info *info_out) {
    TSP_REQUIRE(ctx && x && y && z && mass && group && phi_out, TSP_EINVAL, "NULL argument");
    TSP_REQUIRE(n >= 1 && n < (1ll << 31), TSP_EINVAL, "n = %lld outside [1, 2^31)", (long long)n);
    TSP_REQUIRE(n_groups >= 1 && n_groups < (1ll << 31), TSP_EINVAL, "n_groups = %lld outside [1, 2^31)", (long long)n_groups);
    if (!eps) TSP_REQUIRE(std::isfinite(eps_all) && eps_all >= 0.0f, TSP_EINVAL, "eps_all must be finite and >= 0, not %g", (double)eps_all);
    TSP_REQUIRE(period == 0.0 || (std::isfinite(period) && period > 0.0), TSP_EINVAL,
                "period must be 0 (open box) or finite and > 0, not %g", period);
    TSP_REQUIRE(max_members >= 0, TSP_EINVAL, "max_members = %lld is negative (0: no limit)", (long long)max_members);
    for (int64_t i = 0; i < n; ++i)
        TSP_REQUIRE(group[i] <= n_groups, TSP_EINVAL, "group[%lld] = %d above n_groups = %lld", (long long)i, (int)group[i],
                    (long long)n_groups);
    TSP_HIP(hipSetDevice(ctx->device));
    return group_potential(ctx, n, x, y, z, mass, eps, eps_all, group, n_groups, period == 0.0 ? 0.0 : period, max_members, phi_out,
                           info_out);
}

int tsp_halo_properties(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, const float *mass,
                        const float *vx, const float *vy, const float *vz, const double *phi, const int32_t *group, int64_t n_groups,
                        double period, int64_t *count_out, int64_t *n_bound_out, int64_t *i_pot_out, double *props_out,
                        tsp_halo_info *info_out) {
    TSP_REQUIRE(ctx && x && y && z && mass && group && count_out && n_bound_out && i_pot_out && props_out, TSP_EINVAL, "NULL argument");
    TSP_REQUIRE((vx && vy && vz) || (!vx && !vy && !vz), TSP_EINVAL, "vx, vy and vz must be given together or not at all");
    TSP_REQUIRE(n >= 1 && n < (1ll << 31), TSP_EINVAL, "n = %lld outside [1, 2^31)", (long long)n);
    TSP_REQUIRE(n_groups >= 1 && n_groups < (1ll << 31), TSP_EINVAL, "n_groups = %lld outside [1, 2^31)", (long long)n_groups);
    TSP_REQUIRE(period == 0.0 || (std::isfinite(period) && period > 0.0), TSP_EINVAL,
                "period must be 0 (open box) or finite and > 0, not %g", period);
    for (int64_t i = 0; i < n; ++i)
        TSP_REQUIRE(group[i] <= n_groups, TSP_EINVAL, "group[%lld] = %d above n_groups = %lld", (long long)i, (int)group[i],
                    (long long)n_groups);
    TSP_HIP(hipSetDevice(ctx->device));
    return halo_properties(ctx, n, x, y, z, mass, vx, vy, vz, phi, group, n_groups, period == 0.0 ? 0.0 : period, count_out, n_bound_out,
                           i_pot_out, props_out, info_out);
}

static int check_cube_shape(int resolution, int n_channels) {
    TSP_REQUIRE(resolution >= 1, TSP_EINVAL, "resolution = %d must be at least 1", resolution);
    TSP_REQUIRE(n_channels >= 1 && n_channels <= cube::MAX_CHANNELS, TSP_EINVAL, "n_channels = %d outside [1, %d]", n_channels,
                cube::MAX_CHANNELS);
    TSP_REQUIRE((int64_t)n_channels * resolution * resolution <= cube::MAX_CELLS, TSP_EINVAL,
                "n_channels * R * R = %lld above 2^31", (long long)n_channels * resolution * resolution);
    return TSP_OK;
}

int tsp_spectral_cube(tsp_context *ctx, const float *M, float scale_factor, double v_min, double dv, int n_channels, float sigma_v,
                      const float *sigma, float *cube_out) {
    TSP_REQUIRE(ctx && M && cube_out, TSP_EINVAL, "NULL argument");
    TSP_REQUIRE(std::isfinite(v_min) && std::isfinite(dv) && std::isfinite(sigma_v), TSP_EINVAL, "v_min, dv and sigma_v must be finite");
    TSP_REQUIRE(dv > 0.0, TSP_EINVAL, "dv = %g must be > 0", dv);
    TSP_REQUIRE(sigma_v >= 0.0f, TSP_EINVAL, "sigma_v = %g must be >= 0", (double)sigma_v);
    if (int rc = check_cube_shape(ctx->R, n_channels)) return rc;
    const Particles &p = ctx->p;
    TSP_REQUIRE(ctx->have_mips, TSP_ESTATE, "tsp_set_kernel_mips must be called before tsp_spectral_cube");
    TSP_REQUIRE(p.n > 0 && p.x && p.y && p.z && p.h && p.m, TSP_ESTATE, "no particles with mass are resident");
    TSP_REQUIRE(p.vx && p.vy && p.vz, TSP_ESTATE, "velocities not uploaded (tsp_upload_velocities)");
    TSP_REQUIRE(ctx->have_los, TSP_ESTATE, "no line of sight set (tsp_set_line_of_sight)");
    TSP_REQUIRE(p.n < (1ll << 31), TSP_EINVAL, "n = %lld outside [1, 2^31)", (long long)p.n);
    TSP_HIP(hipSetDevice(ctx->device));
    return spectral_cube(ctx, make_camera(ctx, M, scale_factor), v_min, dv, n_channels, (double)sigma_v, sigma, cube_out);
}

int tsp_spectral_cube_layout(int64_t n, int resolution, int n_channels, int64_t slice_option, int has_sigma, int64_t *out) {
    TSP_REQUIRE(out, TSP_EINVAL, "NULL argument");
    TSP_REQUIRE(n >= 0 && n < (1ll << 31), TSP_EINVAL, "n = %lld outside [0, 2^31)", (long long)n);
    TSP_REQUIRE(slice_option >= 0, TSP_EINVAL, "slice_option = %lld must be >= 0", (long long)slice_option);
    if (int rc = check_cube_shape(resolution, n_channels)) return rc;
    const cube::Grid g = cube::grid_of(resolution, n_channels);
    const int64_t per_slice = cube::slice_particles(n, resolution, n_channels, slice_option);
    const cube::Carve c = cube::carve(n, per_slice, resolution, n_channels, has_sigma != 0, 0);
    const int64_t v[TSP_CUBE_LAYOUT_VALUES] = {
        g.tiles, g.blocks, g.bins, g.key_bits, per_slice, cube::slice_count(n, per_slice), c.capacity,
        (int64_t)c.h_sigma, (int64_t)c.h_geom, (int64_t)c.h_line, (int64_t)c.h_bytes,
        (int64_t)c.a_cube, (int64_t)c.a_count, (int64_t)c.a_offset, (int64_t)c.a_keys, (int64_t)c.a_keys_sorted, (int64_t)c.a_index,
        (int64_t)c.a_index_sorted, (int64_t)c.a_bin_first, (int64_t)c.a_bin_end, (int64_t)c.a_tmp, (int64_t)c.a_bytes};
    for (int k = 0; k < TSP_CUBE_LAYOUT_VALUES; ++k) out[k] = v[k];
    return TSP_OK;
}

static int check_hist2d_shape(int64_t n, int nx, int ny) {
    TSP_REQUIRE(n >= 1 && n < (1ll << 31), TSP_EINVAL, "n = %lld outside [1, 2^31)", (long long)n);
    TSP_REQUIRE(nx >= 1 && nx <= hist2d::MAX_BINS && ny >= 1 && ny <= hist2d::MAX_BINS, TSP_EINVAL, "nx = %d or ny = %d outside [1, %d]",
                nx, ny, hist2d::MAX_BINS);
    return TSP_OK;
}

int tsp_histogram_2d(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *w, const float *v,
                     const tsp_hist2d_spec *spec, int64_t *count_out, double *sums_out, int32_t *bin_out, tsp_hist2d_info *info_out) {
    TSP_REQUIRE(ctx && x && y && spec && count_out && sums_out, TSP_EINVAL, "NULL argument");
    TSP_REQUIRE(spec->edges_x && spec->edges_y, TSP_EINVAL, "NULL edges");
    if (int rc = check_hist2d_shape(n, spec->nx, spec->ny)) return rc;
    const double *axis[2] = {spec->edges_x, spec->edges_y};
    const int bins[2] = {spec->nx, spec->ny};
    for (int a = 0; a < 2; ++a) {
        TSP_REQUIRE(std::isfinite(axis[a][0]), TSP_EINVAL, "edges_%c[0] = %g is not finite", "xy"[a], axis[a][0]);
        for (int k = 1; k <= bins[a]; ++k)
            TSP_REQUIRE(std::isfinite(axis[a][k]) && axis[a][k] > axis[a][k - 1], TSP_EINVAL,
                        "edges must be finite and strictly ascending: edges_%c[%d] = %g after %g", "xy"[a], k, axis[a][k], axis[a][k - 1]);
    }
    TSP_HIP(hipSetDevice(ctx->device));
    return histogram_2d(ctx, n, x, y, w, v, spec, count_out, sums_out, bin_out, info_out);
}

int tsp_histogram_2d_layout(int64_t n, int nx, int ny, int has_w, int has_v, int want_bins, int64_t *out) {
    TSP_REQUIRE(out, TSP_EINVAL, "NULL argument");
    if (int rc = check_hist2d_shape(n, nx, ny)) return rc;
    const hist2d::Levels lv = hist2d::levels_of(n);
    const hist2d::Carve c = hist2d::carve(n, nx, ny, has_w != 0, has_v != 0, want_bins != 0, 0);
    const hist2d::Region h[4] = {c.h_x, c.h_y, c.h_w, c.h_v};
    const hist2d::Region a[11] = {c.a_count, c.a_sums, c.a_edges, c.a_counters, c.a_keys, c.a_keys_sorted, c.a_index, c.a_index_sorted,
                                  c.a_records_a, c.a_records_b, c.a_tmp};
    int k = 0;
    out[k++] = hist2d::key_bits((int64_t)nx * ny), out[k++] = hist2d::BLOCK, out[k++] = lv.count, out[k++] = lv.blocks[0];
    out[k++] = c.records_a, out[k++] = c.records_b;
    for (const hist2d::Region &r : h) out[k++] = (int64_t)r.offset, out[k++] = (int64_t)r.bytes;
    out[k++] = (int64_t)c.h_bytes;
    for (const hist2d::Region &r : a) out[k++] = (int64_t)r.offset, out[k++] = (int64_t)r.bytes;
    out[k++] = (int64_t)c.a_bytes;
    out[k++] = (int64_t)c.bins_bytes;
    static_assert(6 + 2 * 4 + 1 + 2 * 11 + 1 + 1 == TSP_HIST2D_LAYOUT_VALUES, "the header's count of layout values");
    return TSP_OK;
}

int tsp_present(tsp_context *ctx, int width, int height, const tsp_present_base *base, const tsp_present_layer *layers,
                int n_layers, void *out, double *gpu_ms_out) {
    TSP_REQUIRE(ctx && base && out, TSP_EINVAL, "NULL argument");
    return present(ctx, width, height, *base, layers, n_layers, out, gpu_ms_out, false);
}

int tsp_present_yuv420(tsp_context *ctx, int width, int height, const tsp_present_base *base, const tsp_present_layer *layers,
                       int n_layers, uint8_t *out, double *gpu_ms_out) {
    TSP_REQUIRE(ctx && base && out, TSP_EINVAL, "NULL argument");
    return present(ctx, width, height, *base, layers, n_layers, out, gpu_ms_out, true);
}

int tsp_tile_periodic(tsp_context *ctx, int n, const float *offsets_xy, const float *weights) {
    TSP_REQUIRE(ctx && n >= 0 && n <= 4096 && (n == 0 || (offsets_xy && weights)), TSP_EINVAL, "bad argument");
    TSP_REQUIRE(!ctx->surface_keys, TSP_ESTATE, "the accumulator holds surface keys: periodic tiling needs a density render");
    TSP_HIP(hipSetDevice(ctx->device));
    return tile_periodic(ctx, n, offsets_xy, weights);
}

int tsp_content_sort(tsp_context *ctx, int kind, float scale, int64_t *n_finite, int64_t *n_nonpositive) {
    TSP_REQUIRE(ctx && n_finite && n_nonpositive, TSP_EINVAL, "NULL argument");
    TSP_REQUIRE(kind >= 0 && kind <= 3, TSP_EINVAL, "bad content kind %d", kind);
    TSP_REQUIRE(kind != 2 || ctx->C == 4, TSP_EINVAL, "rgb content needs a 4-channel image");
    TSP_HIP(hipSetDevice(ctx->device));
    return content_sort(ctx, kind, scale, n_finite, n_nonpositive);
}

int tsp_moment_sort(tsp_context *ctx, int which, int absolute, int64_t *n_finite) {
    TSP_REQUIRE(ctx && n_finite, TSP_EINVAL, "NULL argument");
    TSP_REQUIRE(which == 1 || which == 2, TSP_EINVAL, "which must be 1 (mean) or 2 (sigma), not %d", which);
    TSP_REQUIRE(ctx->image_source == W_KINEMATIC && ctx->C == 4, TSP_ESTATE,
                "the image is not a kinematic one (render with TSP_MODE_KINEMATIC first)");
    TSP_HIP(hipSetDevice(ctx->device));
    return moment_sort(ctx, which, absolute, n_finite);
}

int tsp_content_values(tsp_context *ctx, const int64_t *ranks, int n_ranks, float *out) {
    TSP_REQUIRE(ctx && ranks && out && n_ranks >= 0, TSP_EINVAL, "bad argument");
    TSP_REQUIRE(ctx->sort_keys_alt, TSP_ESTATE, "tsp_content_sort / tsp_moment_sort has not been called");
    TSP_HIP(hipSetDevice(ctx->device));
    for (int i = 0; i < n_ranks; ++i) {
        TSP_REQUIRE(ranks[i] >= 0 && ranks[i] < ctx->sorted_count, TSP_EINVAL, "rank %lld outside [0, %lld)",
                    (long long)ranks[i], (long long)ctx->sorted_count);
        uint32_t key;
        TSP_HIP(hipMemcpy(&key, ctx->sort_keys_alt + ranks[i], 4, hipMemcpyDeviceToHost));
        const uint32_t bits = (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;   // inverse of the monotone map
        memcpy(&out[i], &bits, 4);
    }
    return TSP_OK;
}

int tsp_content_neg_inf(tsp_context *ctx, int64_t *n_neg_inf) {
    TSP_REQUIRE(ctx && n_neg_inf, TSP_EINVAL, "NULL argument");
    TSP_REQUIRE(ctx->sort_keys_alt, TSP_ESTATE, "tsp_content_sort / tsp_moment_sort has not been called");
    *n_neg_inf = ctx->sorted_neg_inf;
    return TSP_OK;
}

int tsp_set_sphere_mips(tsp_context *ctx, const float *lut, int n0, int n_levels) {
    TSP_REQUIRE(ctx && lut, TSP_EINVAL, "NULL argument");
    TSP_REQUIRE(n0 == 64 && n_levels == 4, TSP_EINVAL, "sphere texture must be 64^2 with 4 mip levels, got n0=%d levels=%d", n0,
                n_levels);
    TSP_HIP(hipSetDevice(ctx->device));
    TSP_HIP(hipMemcpy(ctx->mips + MIP_TOTAL, lut, MIP_TOTAL * sizeof(float), hipMemcpyHostToDevice));
    ctx->have_sphere_mips = true;
    return TSP_OK;
}

int tsp_density_order_stats(tsp_context *ctx, const int64_t *ranks, int n_ranks, float *values_out) {
    TSP_REQUIRE(ctx && n_ranks >= 0 && (n_ranks == 0 || (ranks && values_out)), TSP_EINVAL, "bad argument");
    TSP_REQUIRE(ctx->p.n > 0 && ctx->p.m, TSP_EINVAL, "the density cut needs resident particles with mass");
    for (int i = 0; i < n_ranks; ++i)
        TSP_REQUIRE(ranks[i] >= 0 && ranks[i] < ctx->p.n, TSP_EINVAL, "rank %lld outside [0, %lld)", (long long)ranks[i],
                    (long long)ctx->p.n);
    TSP_HIP(hipSetDevice(ctx->device));
    return density_order_stats(ctx, ranks, n_ranks, values_out);
}

int tsp_render_surface(tsp_context *ctx, const float *M, float scale_factor, float density_cut, const int64_t *starts,
                       const int64_t *lens, int n_ranges, int clear, double *gpu_ms_out) {
    TSP_REQUIRE(ctx && M, TSP_EINVAL, "NULL argument");
    TSP_REQUIRE(ctx->p.n == 0 || ctx->p.m, TSP_EINVAL, "the surface pass needs the mass array (density cut)");
    TSP_REQUIRE(ctx->p.n == 0 || (ctx->p.x && ctx->p.y && ctx->p.z && ctx->p.h), TSP_ESTATE, "position / smoothing-length arrays not resident");
    TSP_REQUIRE(ctx->p.n < ((int64_t)1 << 32), TSP_EINVAL, "the surface keys hold indices below 2^32");
    TSP_REQUIRE(n_ranges >= 0 && (n_ranges == 0 || (starts && lens) || (!starts && !lens)), TSP_EINVAL, "bad ranges");
    TSP_REQUIRE(ctx->have_sphere_mips, TSP_ESTATE, "tsp_set_sphere_mips must be called before tsp_render_surface");
    TSP_REQUIRE(clear || ctx->surface_keys, TSP_ESTATE, "clear = 0 continues a surface image; the accumulator holds none");
    ctx->forget_render_undo();
    TSP_HIP(hipSetDevice(ctx->device));
    std::vector<int64_t> s, l;
    int64_t total = 0;
    if (int rc = clip_ranges(ctx, starts, lens, n_ranges, s, l, &total)) return rc;
    const Camera cam = make_camera(ctx, M, scale_factor);
    double ms_draw = 0.0, ms_resolve = 0.0;
    const int rc = render_surface(ctx, cam, density_cut, s.data(), l.data(), (int)s.size(), total, clear, &ms_draw, &ms_resolve);
    if (rc) return rc;
    ctx->C = 2;
    ctx->image_source = W_NONE;
    ctx->surface_keys = true;
    ctx->image_is_reduced = false;
    ctx->stats.ms_stream = ms_draw;
    ctx->stats.ms_mid = ms_resolve;
    ctx->stats.ms_total = ms_draw + ms_resolve;
    if (gpu_ms_out) *gpu_ms_out = ms_draw + ms_resolve;
    return TSP_OK;
}

// what every surface presentation needs of the image and the parameters; `shading`: the LUT is read
static int check_surface_params(const tsp_context *ctx, const tsp_surface_params *params, bool shading) {
    TSP_REQUIRE(ctx->C == 2, TSP_EINVAL, "surface presentation needs a 2-channel (q, depth) image, the active one has %d", ctx->C);
    TSP_REQUIRE(std::isfinite(params->smoothing_scale), TSP_EINVAL, "smoothing_scale must be finite");
    TSP_REQUIRE(!shading || !params->weighted_average || (params->lut_rgba && params->n_lut >= 2 && params->n_lut <= 65536),
                TSP_EINVAL, "weighted_average needs a colormap LUT of 2 to 65536 entries");
    return TSP_OK;
}

int tsp_surface_present(tsp_context *ctx, const tsp_surface_params *params, float *content_out, uint8_t *rgba8_out,
                        double *ms_out) {
    TSP_REQUIRE(ctx && params, TSP_EINVAL, "NULL argument");
    if (int rc = check_surface_params(ctx, params, rgba8_out != nullptr)) return rc;
    TSP_HIP(hipSetDevice(ctx->device));
    return surface_present(ctx, *params, content_out, rgba8_out, ms_out);
}

// a composed surface frame also refuses a light or a material range that is not finite
static int check_surface_frame(const tsp_context *ctx, const tsp_surface_params *params) {
    if (int rc = check_surface_params(ctx, params, true)) return rc;
    bool ok = std::isfinite(params->depth_scale);
    for (int k = 0; k < 3; ++k)
        ok = ok && std::isfinite(params->light_direction[k]) && std::isfinite(params->light_color[k]) &&
             std::isfinite(params->ambient_color[k]);
    TSP_REQUIRE(ok, TSP_EINVAL, "depth_scale, light_direction, light_color and ambient_color must be finite");
    TSP_REQUIRE(!params->weighted_average || (std::isfinite(params->vmin) && std::isfinite(params->vmax)), TSP_EINVAL,
                "the material range [vmin, vmax] must be finite");
    return TSP_OK;
}

int tsp_present_surface(tsp_context *ctx, int width, int height, const tsp_surface_params *params, const tsp_present_layer *layers,
                        int n_layers, uint8_t *out_rgba8, double *ms_out) {
    TSP_REQUIRE(ctx && params && out_rgba8, TSP_EINVAL, "NULL argument");
    if (int rc = check_surface_frame(ctx, params)) return rc;
    return present_surface(ctx, width, height, *params, layers, n_layers, out_rgba8, ms_out, false);
}

int tsp_present_surface_yuv420(tsp_context *ctx, int width, int height, const tsp_surface_params *params,
                               const tsp_present_layer *layers, int n_layers, uint8_t *out, double *ms_out) {
    TSP_REQUIRE(ctx && params && out, TSP_EINVAL, "NULL argument");
    if (int rc = check_surface_frame(ctx, params)) return rc;
    return present_surface(ctx, width, height, *params, layers, n_layers, out, ms_out, true);
}

int tsp_get_stats(tsp_context *ctx, tsp_stats *out) {
    TSP_REQUIRE(ctx && out, TSP_EINVAL, "NULL argument");
    *out = ctx->stats;
    return TSP_OK;
}

int tsp_set_option(tsp_context *ctx, const char *name, int64_t value) {
    TSP_REQUIRE(ctx && name, TSP_EINVAL, "NULL argument");
    if (!strcmp(name, "count_fragments")) {
        ctx->count_fragments = value != 0;
        return TSP_OK;
    }
    if (!strcmp(name, "p_small_milli")) {     // class boundary small/mid in 1/1000 px (<= 16000: kernel S holds mips 2 and 3 and packs <= 16 texel columns)
        TSP_REQUIRE(value >= 0 && value <= 16000, TSP_EINVAL, "p_small out of range (kernel S packs <= 16 texel columns per footprint)");
        ctx->p_small = (float)value * 1e-3f;
        return TSP_OK;
    }
    if (!strcmp(name, "debug_no_raster")) {
        ctx->debug_no_raster = value != 0;
        return TSP_OK;
    }
    if (!strcmp(name, "huge_split") || !strcmp(name, "stream_blocks_per_cu")) {
        TSP_REQUIRE(value >= 0 && value <= 4096, TSP_EINVAL, "%s out of range", name);
        if (name[0] == 'h') ctx->huge_split = (int)value;
        else ctx->stream_blocks_per_cu = (int)value;      // 0 = as many as stay resident
        return TSP_OK;
    }
    if (!strcmp(name, "slice_records")) {     // deferred footprints per launch of kernels G / H2 (0 = default: 2^27 mid, 2^30 huge)
        TSP_REQUIRE(value == 0 || (value >= 64 && value <= (1ll << 27)), TSP_EINVAL, "%s: 0 or 64 .. 2^27", name);
        ctx->slice_records = value;
        return TSP_OK;
    }
    if (!strcmp(name, "cube_slice_particles")) {     // particles per slice of tsp_spectral_cube (0 = default: what the list bound allows); only lowers it
        TSP_REQUIRE(value >= 0 && value < (1ll << 31), TSP_EINVAL, "%s: 0 .. 2^31 - 1", name);
        ctx->cube_slice_particles = value;
        return TSP_OK;
    }
    if (!strcmp(name, "debug_fail_stage")) {   // test aid: the next tsp_render fails after kernel S (1) or after kernel G (2)
        TSP_REQUIRE(value >= 0 && value <= 2, TSP_EINVAL, "%s out of range", name);
        ctx->debug_fail_stage = (int)value;
        return TSP_OK;
    }
    if (!strcmp(name, "debug_fail_alloc")) {   // test aid: the k-th device allocation from now on fails once (alloc_group)
        TSP_REQUIRE(value >= 0, TSP_EINVAL, "%s out of range", name);
        ctx->debug_fail_alloc = value;
        return TSP_OK;
    }
    if (!strcmp(name, "debug_gather_full_lut")) { ctx->debug_gather_full_lut = value ? 1 : 0; return TSP_OK; }
    if (!strcmp(name, "mid_item_scale_milli")) {
        TSP_REQUIRE(value >= 1 && value <= 100000, TSP_EINVAL, "%s out of range", name);
        ctx->mid_item_scale = (double)value * 1e-3;
        return TSP_OK;
    }
    if (!strcmp(name, "mid_narrow_px_milli")) {    // mid footprints below this many 1/1000 px go to kernel N (0 = none)
        TSP_REQUIRE(value >= 0 && value <= 64000, TSP_EINVAL, "%s out of range", name);
        ctx->mid_narrow_px = (float)value * 1e-3f;
        return TSP_OK;
    }
    if (!strcmp(name, "mid_item_records")) {
        TSP_REQUIRE(value == 0 || (value >= 64 && value <= 8192 && (value & (value - 1)) == 0), TSP_EINVAL, "%s: 0 or a power of two from 64 to 8192", name);
        ctx->mid_item_records = (int)value;
        return TSP_OK;
    }
    if (!strcmp(name, "stream_batch_chunks")) {
        TSP_REQUIRE(value >= 4 && value <= 4096, TSP_EINVAL, "%s out of range", name);
        ctx->stream_batch_chunks = (int)value;
        return TSP_OK;
    }
    if (!strcmp(name, "huge_band_mib")) {     // memory the band bins of the huge records may take, MiB (0 = never bin: kernel H2 scans one list)
        TSP_REQUIRE(value >= 0 && value <= (1 << 20), TSP_EINVAL, "%s out of range", name);
        ctx->huge_band_budget = value << 20;
        return TSP_OK;
    }
    if (!strcmp(name, "huge_variant")) {
        // 1 = auto; 2, 4-7 force a strip shape / occupancy of kernel H2 (A/B and tests)
        TSP_REQUIRE(value >= 1 && value <= 7 && value != 3, TSP_EINVAL, "huge_variant out of range");
        ctx->huge_variant = (int)value;
        return TSP_OK;
    }
    if (!strcmp(name, "h2_walk")) {
        // kernel H2's row walk for the density strips (64x32 and 64x16 at 8 waves/SIMD): 1 = asm (default), 0 = C++ (A/B and parity)
        TSP_REQUIRE(value == 0 || value == 1, TSP_EINVAL, "%s out of range", name);
        ctx->h2_walk = (int)value;
        return TSP_OK;
    }
    if (!strcmp(name, "h2_chord")) {
        // kernel H2's row clip: 1 = a hit's rows outside the chord of the footprint's disc are not walked (default), 0 = the square's rows (A/B and parity)
        TSP_REQUIRE(value == 0 || value == 1, TSP_EINVAL, "%s out of range", name);
        ctx->h2_chord = (int)value;
        return TSP_OK;
    }
    if (!strcmp(name, "reorder_interleave")) {   // read by the next tsp_reorder_spatial
        TSP_REQUIRE(value >= 0 && value <= 2, TSP_EINVAL, "%s out of range", name);
        ctx->reorder_interleave = (int)value;      // 0: Morton order inside the blocks, 1: 64 x 8 transposition, 2: by descending h
        return TSP_OK;
    }
    if (!strcmp(name, "chunk_cull")) {        // 1 (default): kernel S skips the chunks whose bounds lie outside the view
        ctx->chunk_cull = value != 0;
        return TSP_OK;
    }
    if (!strcmp(name, "overlap_mid_huge")) {
        ctx->overlap_mid_huge = value != 0;
        return TSP_OK;
    }
    if (!strcmp(name, "use_quantity")) {      // 0: render density-only without dropping the resident q array
        ctx->use_quantity = value != 0;
        return TSP_OK;
    }
    if (!strcmp(name, "active_channels")) {   // layout tsp_write_image / the colormap calls assume
        TSP_REQUIRE((value == 2 || value == 4) && value <= ctx->Ccap, TSP_EINVAL, "bad channel count %lld", (long long)value);
        ctx->C = (int)value;
        ctx->forget_render_undo();
        return TSP_OK;
    }
    set_error("unknown option '%s'", name);
    return TSP_EINVAL;
}

int tsp_measure_read_bandwidth(tsp_context *ctx, int64_t bytes, int iters, double *gbps_out) {
    TSP_REQUIRE(ctx && gbps_out && bytes > 0 && iters > 0, TSP_EINVAL, "bad argument");
    TSP_HIP(hipSetDevice(ctx->device));
    return measure_read_bandwidth(ctx, bytes, iters, gbps_out);
}

}  // extern "C"
