// tsp_internal.h -- context layout and helpers shared by the translation units of libtopsy_splat.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>
#include <vector>
#include <stdio.h>
#include <string>

#include "../../include/topsy_splat.h"
#include "tsp_math.h"

namespace tsp {

void set_error(const char *fmt, ...);

#define TSP_HIP(call)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            tsp::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return TSP_EHIP;                                                                   \
        }                                                                                      \
    } while (0)

#define TSP_REQUIRE(cond, code, ...)       \
    do {                                   \
        if (!(cond)) {                     \
            tsp::set_error(__VA_ARGS__);   \
            return (code);                 \
        }                                  \
    } while (0)

// Resident particle data: struct-of-arrays float32 in HBM, one allocation per attribute so each
// streams as an independent fully-coalesced sequence (20 B/particle density, 24 B with q, 28 B rgb).
struct Particles {
    int64_t n = 0;
    float *x = nullptr, *y = nullptr, *z = nullptr, *h = nullptr, *m = nullptr;
    float *q = nullptr;                      // nullptr -> density render (q = 0)
    float *r = nullptr, *g = nullptr, *b = nullptr;
    float *vx = nullptr, *vy = nullptr, *vz = nullptr;   // velocities (tsp_upload_velocities): read by the kinematic weight pass only
    uint32_t *perm = nullptr;                // new -> old index after tsp_reorder_spatial (else nullptr)
    // camera-independent vertex weights (sph.wgsl:76-83 `mass / (h*h)`, :69-73 `rgb / (h*h)`), formed once per upload by
    // ensure_weights() with the float32 operations the shader performs per vertex and frame: what kernel S streams
    // instead of m (r, g, b) -- the same bytes per particle, no division per particle and frame
    float *wm = nullptr;
    float *wr = nullptr, *wg = nullptr, *wb = nullptr;
    bool wm_valid = false;                   // cleared whenever h / m change (upload, generate, reorder)
    // what wr / wg / wb hold: nothing valid, (r, g, b) / h^2, or the kinematic weights (m, m u, m u^2) / h^2 of the line of sight
    // tsp_context::w_los (tsp_kinematics.hip).  W_NONE whenever h / m / rgb / velocities change (upload, generate, reorder)
    int wrgb_source = 0;
};
enum { W_NONE = 0, W_RGB = 1, W_KINEMATIC = 2 };     // Particles::wrgb_source, tsp_context::image_source

// Bounds of every block of BOUNDS_BLOCK consecutive particles (view culling of whole chunks, kernel S): two float4 per block,
// (xmin, ymin, zmin, hmax) and (xmax, ymax, zmax, -).  NaN coordinates are ignored (such a particle draws nothing).
constexpr int BOUNDS_BLOCK = 512;            // = CHUNK of tsp_pipeline.hip (static_assert there)

// Deferred-footprint record written by the streaming kernel for the tile kernels (20 B).
struct Record {
    float pcx, pcy, P, w0, w1;
};
struct Record4 {   // rgb variant (24 B)
    float pcx, pcy, P, w0, w1, w2;
};

struct Counters {      // device-side, zeroed per render call
    unsigned long long n_small, n_mid, n_huge, n_culled, n_fragments, huge_count, next_chunk, mid_odd_weights;     // next_chunk: kernel S's batch counter; mid_odd_weights: the mid list holds a weight that is not finite (kernel N's fill pass)
    unsigned long long n_frag_class[4];   // n_fragments by the kernel that drew them: S, G, H2, (unused)
};

struct Workspace {     // per-context scratch of the three-class pipeline (grown on demand)
    void *mid_geom = nullptr, *mid_w = nullptr;     // deferred mid footprints: float4 geometry + weights
    int64_t mid_capacity = 0;
    void *huge_geom = nullptr, *huge_w = nullptr;   // deferred huge footprints
    int64_t huge_capacity = 0;
    void *hband_geom = nullptr, *hband_w = nullptr; // the huge records once more, binned by 64-row image band (n_bands regions of hband_stride records)
    int *hband_count = nullptr;                     // records per band
    int64_t hband_stride = 0; int hband_bands = 0;
    // the strip bins of the mid records (bin_mid_records, tsp_mid.hip): one set, refilled for each launch of kernel N (16-column strips)
    // and of kernel G (64-column strips); a "tile" in these names is one strip of the kernel being launched
    void *mband_geom = nullptr, *mband_w = nullptr; // the mid records copied into exact-size bins, one per strip
    int *mband_count = nullptr;                     // records per strip | fill cursors
    long long *mband_base = nullptr;                // first record of each strip's bin
    int64_t mband_capacity = 0;                     // records the bins can hold
    int mtile_capacity = 0;                         // strips the per-strip arrays can hold
    int64_t mitem_capacity = 0;                     // work items the item table can hold
    int *mitem_tile = nullptr, *mitem_base = nullptr; // work items of kernels N and G: item -> strip, strip -> first item
    int64_t chunk_capacity = 0;         // chunks alive_list can hold
    float4 *block_bounds = nullptr;     // chunk culling: bounds of every BOUNDS_BLOCK particles (valid while bounds_valid)
    int64_t bounds_capacity = 0;        // blocks
    bool bounds_valid = false;          // cleared whenever positions / smoothing lengths change (upload, generate, reorder)
    int *alive_list = nullptr;          // chunk culling: the chunks of this render call that may reach the view (seg_capacity entries)
    unsigned long long *cull_info = nullptr;   // [0] chunks alive, [1] particles in culled chunks
    int64_t *range_prefix = nullptr;    // device copy of the ranges of the current call
    int64_t range_capacity = 0;
    int *count_diff = nullptr;          // rgb: (R+1)^2 corner-difference image of the huge footprints' pixel rectangles
    int *count_band = nullptr;          // rgb: per (64-row band, column) sums of its row-scanned form
    int count_R = 0;                    // resolution count_diff / count_band are sized for (0: not allocated)
};

// The context's timing events by what they delimit.  A render block (run_pipeline, inside tsp_render's pair) marks its kernels;
// every other call that times itself uses the neutral EV_T* marks, which share the first events: such calls never run inside
// a render block.
enum {
    EV_RENDER_BEGIN, EV_RENDER_END,         // tsp_render: the whole call
    EV_S_BEGIN, EV_S_END,                   // kernel S (every attempt records them: the last one counts)
    EV_MID_BEGIN, EV_MID_END,               // kernels N and G, on their stream (EV_MID_END is also what `stream` waits for when they overlap H2)
    EV_BLOCK_END,                           // after the last launch of the block
    EV_CULL_BEGIN,                          // before the culling passes: kernel S's time starts here when they run
    EV_S_DONE,                              // overlap_mid_huge: what the second stream waits for
    EV_HUGE_BEGIN, EV_HUGE_END,             // kernel H2 (its launcher records EV_HUGE_END again after every launch)
    EV_COUNT,
    EV_T0 = 0, EV_T1, EV_T2, EV_T3, EV_T4, EV_T5      // call-local marks (tsp_surface / tsp_present / tsp_data / tsp_comm)
};
// bits of tsp_context::kernel_attr_done
constexpr uint32_t attr_bit_stream(int mode) { return 1u << mode; }          // kernel S of a mode
constexpr uint32_t attr_bit_bins(int nw) { return 1u << (8 + nw); }          // the strip-bin passes by weight floats per record

}  // namespace tsp

struct tsp_context {
    int device = 0;
    int R = 0, C = 0, Ccap = 0;       // C = active channels (2 or 4) <= Ccap
    bool use_quantity = true;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;    // option overlap_mid_huge: kernel G runs here, concurrently with kernel H2 on `stream`
    hipEvent_t ev[tsp::EV_COUNT] = {};    // indexed by the EV_* names above
    float *image = nullptr;           // R*R*C float32 render target (what read-back, colormap and reduce see)
    double *image64 = nullptr;        // float64 master copy every kernel accumulates into (rounded once per render)
    double *image64_entry = nullptr;  // image64 as tsp_render found it: what a failed block puts back (the call draws all of a block or none of it)
    float *mips = nullptr;            // 2 x 5440 floats: the SPH kernel mips, then the sphere mips of the surface pass
    bool have_mips = false;
    bool have_sphere_mips = false;    // tsp_set_sphere_mips was called
    bool surface_keys = false;        // image64 holds the 64-bit occlusion keys of tsp_render_surface, not float64 sums
    bool lut_mirror_symmetric = false;    // every mip level equals its left-right and top-bottom mirror images bit for bit
    bool lut_zero_outside_disc = false;   // on every mip level, each texel whose centre is >= 2h from the centre is exactly 0
    tsp::Particles p;
    tsp::Counters *counters = nullptr;
    tsp::Workspace ws;
    uint8_t *out8 = nullptr;          // R*R*4 staging for colormap output
    float *outf = nullptr;            // R*R*4 float staging (HDR)
    float *lut = nullptr;             // colormap LUT on device
    int lut_capacity = 0;
    float *lut2d = nullptr;           // bivariate colormap LUT, n x n x RGBA
    int lut2d_n = 0;
    void *scratch = nullptr;          // host-image colormap staging
    size_t scratch_bytes = 0;
    uint32_t *sort_keys = nullptr, *sort_keys_alt = nullptr;   // content order statistics (autorange)
    void *sort_tmp = nullptr;
    size_t sort_tmp_bytes = 0;
    int64_t sort_capacity = 0, sorted_count = 0;
    int64_t sorted_neg_inf = 0;       // content values equal to -inf that the last tsp_content_sort dropped
    tsp_stats stats = {};
    std::vector<int64_t> cell_offsets;     // first index of every (stratum, Morton cell) run of the last reorder_spatial, then n
    int cell_bits = 0;                     // the cells form a (2^cell_bits)^3 grid over the bounding box
    float cell_lo[3] = {0, 0, 0}, cell_width[3] = {0, 0, 0};
    std::vector<int64_t> strata_offsets;   // first index of every stratum of the last reorder_spatial, then n
    uint32_t kernel_attr_done = 0;   // bit per kernel family whose dynamic-LDS limit was raised on this context's device
    bool count_fragments = false;
    // pipeline tuning (tsp_set_option)
    float p_small = 16.0f;             // footprints narrower than this many pixels are splatted by kernel S (mips 3 and 2; <= 16: its texel columns are packed 16 x 4 bits)
    int64_t huge_band_budget = 6ll << 30;   // bytes the band bins of the huge records may take (n_bands x n_huge records); above it kernel H2 scans one list
    int huge_variant = 1;             // kernel H2's strip shape / occupancy: 1 = auto (density: 64x32 strips at 8 waves/SIMD from 7e5 records, 64x16 below; two channels 64x16 at 7; rgb at 5), 2 / 4-7 = A/B builds
    int h2_walk = 1;                  // kernel H2's row walk in the single-channel 8-waves/SIMD builds: 1 = hand-allocated asm (tsp_huge.hip), 0 = the C++ walk (A/B and parity)
    int h2_chord = 1;                 // kernel H2 walks a hit's pixel rows: 1 = those whose chord of the inscribed disc reaches the strip's columns (tsp_pipeline.h chord_limit), 0 = every row of the square (A/B and parity)
    int huge_split = 0;              // workgroups per image tile of kernel H2 (0 = auto)
    int reorder_interleave = 2;     // tsp_reorder_spatial's arrangement inside every 512-particle block: 0 Morton order, 1 transposed 64 x 8, 2 by descending smoothing length (tsp_data.hip)
    int stream_blocks_per_cu = 0;    // kernel S: persistent workgroups per CU (0 = what the occupancy query reports)
    int debug_gather_full_lut = 0;   // kernel G: 1 = the whole mip pyramid in LDS even when the kernel image is symmetric (measurement aid)
    double mid_item_scale = 0.35;    // kernel G: records per work item = this x sqrt(records), rounded to a power of two (option mid_item_scale_milli)
    float mid_narrow_px = 64.0f;     // mid footprints narrower than this are drawn by kernel N, four records per wave step (0: all by kernel G; option mid_narrow_px_milli)
    int mid_item_records = 0;        // kernel G: records per work item (0 = by list length; a power of two from 64 to 1024)
    int stream_batch_chunks = 8;     // kernel S: the largest batch of consecutive chunks a workgroup takes from the shared counter
    bool chunk_cull = true;           // chunks (512 consecutive particles) whose bounds lie outside the view are skipped by kernel S
                                      // unread: pays with a load-time spatial order (tsp_reorder_spatial); identical results
    int64_t chunk_culled_particles = 0;   // of the last render call
    bool overlap_mid_huge = false;    // option: kernels G and H2 on two streams (measured: no gain at 1.25e8, +6 % at 1e7)
    int64_t slice_records = 0;        // option: deferred records kernels G / H2 take per launch (0 = 2^27 mid / 2^30 huge); a block of any size draws in slices
    int64_t cube_slice_particles = 0; // option: particles per slice of tsp_spectral_cube (0 = what the list bound allows, tsp_cube_layout.h); only lowers it
    int debug_fail_stage = 0;        // test aid: the next render fails with TSP_ENOMEM after kernel S (1) / after kernel G (2); cleared by the failure
    int64_t debug_fail_alloc = 0;     // test aid: the k-th allocation of alloc_group() or scratch_alloc() from now on fails once, as hipMalloc would (0 = off)
    int stream_occ[3][2] = {};        // kernel S: workgroups resident per CU by [mode][one-channel window | all channels] (occupancy query, once per context)
    bool debug_no_raster = false;    // measurement aid: kernel S classifies and emits records but rasterises nothing (the image is then incomplete)
    int cu_count = 256;
    // RCCL
    void *comm = nullptr;
    int n_ranks = 1, rank = 0;
    bool image_is_reduced = false;    // `image` already holds the cross-rank sum of the current frame (tsp_comm_reduce_image)
    // kinematic maps (TSP_MODE_KINEMATIC, tsp_kinematics.hip).  A line of sight is six floats: the unit axis, then v_ref
    bool have_los = false;
    float los[6] = {};                // tsp_set_line_of_sight: what the next kinematic block draws along
    float w_los[6] = {};              // what p.wr / wg / wb were formed with (while p.wrgb_source == W_KINEMATIC)
    int image_source = tsp::W_NONE;   // which 4-channel mode started the image (W_NONE: a 2-channel render, or none yet)
    float image_los[6] = {};          // ... and, for W_KINEMATIC, along which line of sight
    bool kinematic_block = false;     // set by tsp_render around a kinematic block: the rgb pipeline then asks for the kinematic weights
    // tsp_render_undo: what the last tsp_render found, kept until another call changes the image (forget_render_undo)
    struct RenderUndo {
        int kind = 0;                 // 0: nothing to undo; 1: the block drew (image64_entry and the fields below put it back); 2: it failed (tsp_render restored everything itself)
        int C = 0;
        tsp_stats stats = {};
        int64_t chunk_culled_particles = 0;
        int image_source = tsp::W_NONE;
        float image_los[6] = {};
    } undo;
    void forget_render_undo() { undo.kind = 0; }
};

namespace tsp {
// Per-call device scratch that is released on every exit path.  It is allocated by scratch_alloc() alone (TSP_SCRATCH_ALLOC in
// an entry point), so that every allocation has a named site, counts against option debug_fail_alloc and fails one way.
struct DeviceScratch {
    void *p = nullptr;
    DeviceScratch() = default;
    DeviceScratch(const DeviceScratch &) = delete;
    DeviceScratch &operator=(const DeviceScratch &) = delete;
    ~DeviceScratch() { if (p) (void)hipFree(p); }
    template <typename T> T *as() const { return static_cast<T *>(p); }
    void *release() { void *q = p; p = nullptr; return q; }
    void reset(void *q) { if (p) (void)hipFree(p); p = q; }
};
// `bytes` (16 at least) of device memory into the empty `buf`.  A failure -- hipMalloc's, or the injected one of option
// debug_fail_alloc, which counts these allocations and those of alloc_group() alike -- leaves buf empty, puts the site's name
// into tsp_last_error, clears HIP's sticky last error (a later launch check must not report this allocation) and returns
// TSP_ENOMEM (TSP_EHIP for another runtime error).  Site names are unique and written as SITE("site"), like alloc_group()'s.
int scratch_alloc(tsp_context *ctx, const char *site, DeviceScratch &buf, size_t bytes);
// scratch_alloc() in an entry point: a failure returns its code from the caller.  Entry points allocate before they write to
// the caller's outputs or change the context, so that a failed call leaves both as they were.
#define TSP_SCRATCH_ALLOC(ctx, site, buf, bytes)                                     \
    do {                                                                             \
        const int rc_ = tsp::scratch_alloc((ctx), (site), (buf), (size_t)(bytes));   \
        if (rc_ != TSP_OK) return rc_;                                               \
    } while (0)

// The two scratch buffers that every gather call (tsp_smooth.hip), the gravity sums and the halo calls (tsp_halo.hip) take, in this
// order: the one place that owns their sites (tsp_api.hip).  Each caller partitions them by offsets of its own.
int gather_scratch(tsp_context *ctx, DeviceScratch &dh, size_t h_bytes, DeviceScratch &da, size_t a_bytes);

// Every device buffer that can be (re)allocated after tsp_create -- the resident particle arrays, the render workspace, the
// colormap and post-pass staging -- goes through alloc_group().  A group is the buffers that are only ever used together, with the capacity
// fields that describe them: the group is freed and its capacities zeroed first, then each buffer is allocated, and only once all
// of them exist are the capacities recorded.  A failed allocation (or the injected one of option debug_fail_alloc) leaves every
// pointer of the group null and its capacities 0, so the next call allocates again instead of trusting a stale size; it returns
// TSP_ENOMEM (TSP_EHIP for another runtime error) with the site's name in tsp_last_error.  Site names are unique (a CPU test
// scans the sources), written first so that they can be found: {"site", (void **)&ptr, bytes}, or SITE("site") where a name
// is passed on.
#define SITE(name) name
struct DeviceBuffer {
    const char *site;
    void **p;
    size_t bytes;
};
struct Capacity {      // a capacity field and the value it takes once its group is allocated
    int64_t *c64 = nullptr; int *c32 = nullptr; size_t *csz = nullptr;
    int64_t value = 0;
    Capacity(int64_t *c, int64_t v) : c64(c), value(v) {}
    Capacity(int *c, int64_t v) : c32(c), value(v) {}
    Capacity(size_t *c, int64_t v) : csz(c), value(v) {}
    void set(int64_t v) const {
        if (c64) *c64 = v;
        else if (c32) *c32 = (int)v;
        else *csz = (size_t)v;
    }
};
int alloc_group(tsp_context *ctx, std::initializer_list<DeviceBuffer> bufs, std::initializer_list<Capacity> caps);

// Host-side invariant of the workspace: a capacity above 0 means every buffer it describes exists.  Checked before the kernels
// that use the buffers are launched, so that a missed allocation site is an error (TSP_ESTATE) and never a write through null.
int check_workspace(const tsp_context *ctx);

// kernels / launchers implemented in the other translation units
int launch_generic(tsp_context *ctx, const Camera &cam, const int64_t *d_ranges, int n_ranges,
                   int64_t total, int mode, int rule);
int launch_pipeline(tsp_context *ctx, const Camera &cam, const int64_t *h_starts, const int64_t *h_lens,
                    int n_ranges, int64_t total, int mode);
int launch_colormap_scalar(tsp_context *ctx, const float *d_img, int64_t npix, int C, const float *d_lut,
                           int n_lut, float vmin, float vmax, int log_scale, int weighted, uint8_t *d_out);
int launch_colormap_rgb(tsp_context *ctx, const float *d_img, int64_t npix, int C, float vmin, float vmax,
                        float gamma, uint8_t *d_out8, float *d_outf);
int launch_colormap_bivariate(tsp_context *ctx, const float *d_img, int64_t npix, int C, float vmin, float vmax,
                             float dvmin, float dvmax, int log_scale, int weighted, uint8_t *d_out);
int generate_synthetic(tsp_context *ctx, int64_t n_total, int64_t first, int64_t count, uint64_t seed,
                       float h_cap, int with_quantity, int with_rgb);
int reorder_spatial(tsp_context *ctx, int n_strata, uint64_t seed, int64_t *perm_out);
// (re)computes p.wm or p.wr / wg / wb on ctx->stream when the particles changed; rgb: also when wr / wg / wb hold the weights of the
// other 4-channel mode (ctx->kinematic_block selects which are wanted) or of another line of sight
int ensure_weights(tsp_context *ctx, bool rgb);
// tsp_kinematics.hip: the kinematic weights into p.wr / wg / wb (on ctx->stream) and the per-pixel moment maps of a kinematic image
int launch_kinematic_weights(tsp_context *ctx);
int launch_velocity_moments(tsp_context *ctx, const float *d_img, int64_t npix, float *d_maps);
// tsp_hist2d.hip: weighted 2-D histograms of caller-ordered host arrays (tsp_histogram_2d); per-call DeviceScratch only, through the
// sites of gather_scratch(); no context state
int histogram_2d(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *w, const float *v,
                 const tsp_hist2d_spec *spec, int64_t *count_out, double *sums_out, int32_t *bin_out, tsp_hist2d_info *info_out);
// tsp_cube.hip: the position-position-velocity cube of every resident particle (tsp_spectral_cube); per-call DeviceScratch only,
// through the sites of gather_scratch(); no context state
int spectral_cube(tsp_context *ctx, const Camera &cam, double v_min, double dv, int n_channels, double sigma_v, const float *sigma,
                  float *cube_out);
int ensure_block_bounds(tsp_context *ctx);     // (re)computes ws.block_bounds on ctx->stream when the particles changed
int measure_read_bandwidth(tsp_context *ctx, int64_t bytes, int iters, double *gbps_out);
int launch_image_convert(tsp_context *ctx, bool to_float);
int tile_periodic(tsp_context *ctx, int n, const float *h_offsets, const float *h_weights);
int moment_sort(tsp_context *ctx, int which, int absolute, int64_t *n_finite);   // the same sort of a kinematic image's moment map
int content_sort(tsp_context *ctx, int kind, float scale, int64_t *n_finite, int64_t *n_nonpositive);   // image64 -> image (true) or image -> image64 (false)
int smoothing_lengths(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, int k, float period,
                      float *h_out);   // tsp_smooth.hip: per-call DeviceScratch only, no context state
// tsp_smooth.hip: the gather-form SPH sums on the same index (tsp_sph_sum, tsp_sph_velocity_gradient); per-call DeviceScratch only.
// SPH_GATHER_SUM: fields = {a}, outs = {out}.  SPH_GATHER_VELOCITY_GRADIENT: fields = {mass, rho, vx, vy, vz}, outs = {div,
// curl_x, curl_y, curl_z}.
enum { SPH_GATHER_SUM = 0, SPH_GATHER_VELOCITY_GRADIENT = 1 };
int sph_sum(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, const float *h, int mode,
            const float *const *fields, int n_fields, float period, float *const *outs, int n_outs);
// tsp_smooth.hip: the SPH sums of n_fields per-particle fields at the points of a lattice, with h taken at the point from its k
// nearest particles (tsp_sph_sample_lattice); per-call DeviceScratch only, through the sites of sph_sum().
int sph_sample_lattice(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, int n_fields,
                       const float *const *fields, int k, float period, const tsp_lattice *lattice, float *h_out,
                       float *const *outs);
// tsp_fof.hip: friends-of-friends groups over the index of tsp_morton.h; per-call DeviceScratch only, no context state
int fof_groups(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, float linking_length, float period,
               int64_t min_members, int32_t *group_out, tsp_fof_info *info_out);
// tsp_center.hip: the shrinking-sphere centre of caller-ordered host arrays; per-call DeviceScratch only, no context state
int shrink_sphere_center(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, const float *mass,
                         float mass_cut_factor, double r_start, double shrink_factor, int64_t min_particles, int max_iterations,
                         double center_out[3], tsp_center_info *info_out);
// tsp_orient.hip: the moments of the particles inside a sphere (mass, centre of mass, angular momentum, second moments) of
// caller-ordered host arrays; per-call DeviceScratch only, no context state
int sphere_moments(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, const float *mass, const float *vx,
                   const float *vy, const float *vz, const double center[3], double r, double r_vel, tsp_moments *out);
// tsp_profile.hip: binned shell / annulus sums of caller-ordered host arrays (radial profiles); per-call DeviceScratch only, no
// context state
int radial_profile(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, const float *mass, const float *vx,
                   const float *vy, const float *vz, const tsp_profile_spec *spec, int64_t *count_out, double *sums_out,
                   tsp_profile_info *info_out);
// tsp_gravity.hip: the softened direct sum of potential and acceleration at the targets (tsp_gravity_direct; tx == nullptr: the
// targets are the sources); per-call DeviceScratch only, through the sites of gather_scratch(); no context state
int gravity_direct(tsp_context *ctx, int64_t n_src, const float *sx, const float *sy, const float *sz, const float *mass,
                   const float *eps, float eps_all, int64_t n_tgt, const float *tx, const float *ty, const float *tz, double *pot_out,
                   double *acc_out, tsp_gravity_info *info_out);
// tsp_gravity_tree.hip: the same sums by a Barnes-Hut tree over the Morton order of the sources (tsp_gravity_tree); per-call
// DeviceScratch only, through the sites of build_morton_index() and gather_scratch(); no context state
int gravity_tree(tsp_context *ctx, int64_t n_src, const float *sx, const float *sy, const float *sz, const float *mass,
                 const float *eps, float eps_all, int64_t n_tgt, const float *tx, const float *ty, const float *tz, float theta,
                 double *pot_out, double *acc_out, tsp_gravity_tree_info *info_out);
// tsp_halo.hip: the self-potential of every halo of a catalogue by a direct sum confined to the halo (tsp_group_potential) and
// the per-halo reductions (tsp_halo_properties) over the members sorted by label; per-call DeviceScratch only, through the sites
// of gather_scratch(); no context state
int group_potential(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, const float *mass, const float *eps,
                    float eps_all, const int32_t *group, int64_t n_groups, double period, int64_t max_members, double *phi_out,
                    tsp_group_potential_info *info_out);
int halo_properties(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, const float *mass, const float *vx,
                    const float *vy, const float *vz, const double *phi, const int32_t *group, int64_t n_groups, double period,
                    int64_t *count_out, int64_t *n_bound_out, int64_t *i_pot_out, double *props_out, tsp_halo_info *info_out);
// tsp_surface.hip: the occlusion pass + resolve (keys in image64, (q, depth) in image), the rho order statistics and the
// filter + shading; per-call memory is DeviceScratch
int render_surface(tsp_context *ctx, const Camera &cam, float cut, const int64_t *h_starts, const int64_t *h_lens,
                   int n_ranges, int64_t total, int clear, double *ms_draw, double *ms_resolve);
int density_order_stats(tsp_context *ctx, const int64_t *ranks, int n_ranks, float *values_out);
int surface_present(tsp_context *ctx, const tsp_surface_params &prm, float *content_out, uint8_t *rgba8_out, double *ms_out);
// the two halves of it that the surface base of the frame composition shares: the bilateral filter of ctx->image into `filtered`
// (R * R float2, launched on ctx->stream) and the shading parameters for a normal whose z is 1 / width
int launch_bilateral(tsp_context *ctx, double smoothing_scale, float2 *filtered);
ShadeParams shade_params(const tsp_surface_params &prm, int width);
// tsp_present.hip: frame composition (base map + layers on a W x H canvas), optionally converted to I420 planes (yuv420);
// per-call memory is DeviceScratch.  present_surface: the same with the lit surface as the base (the filter, then the shading
// from five samples of the filtered image per canvas pixel); ms_out = [filter, composition (+ conversion)]
int present(tsp_context *ctx, int W, int H, const tsp_present_base &base, const tsp_present_layer *layers, int n_layers, void *out,
            double *gpu_ms_out, bool yuv420);
int present_surface(tsp_context *ctx, int W, int H, const tsp_surface_params &prm, const tsp_present_layer *layers, int n_layers,
                    void *out, double *ms_out, bool yuv420);
}  // namespace tsp
