/* topsy_splat.h -- C-ABI of the MI355X-native SPH particle-splatting backend for topsy.
 *
 * This is the drop-in boundary for ONE hot path of pynbody/topsy: per-particle smoothing-kernel
 * rasterisation into a float32 image (reference src/topsy/sph.py + shaders/sph.wgsl) and the
 * 1-D-LUT / log-scale colormap post-pass (reference src/topsy/colormap/implementation.py +
 * shaders/colormap.wgsl).  In the reference that path sits behind a Python object protocol
 * (Visualizer <-> SPH / ColormapHolder) whose device side is wgpu; here the device side is this
 * library (hand-written HIP for gfx950) and the Python side (topsy_amd/) binds it with ctypes.
 *
 * Conventions
 *   - plain C types only; every function returns 0 on success, a negative TSP_E* code on error;
 *     tsp_last_error() gives the text of the most recent failure on the calling thread.
 *   - the caller owns every host array; the library copies on upload and writes only into
 *     caller-allocated output buffers.  No callbacks, no exceptions cross the boundary.
 *   - one context = one GPU (one process per GPU for multi-GPU; see tsp_comm_*).  Calls on one
 *     context must be serialised by the caller.  All calls are synchronous (they return after
 *     the GPU work they issued has completed), mirroring the reference's
 *     submit + on_submitted_work_done_sync pairs (src/topsy/util.py:84-99).
 *   - images are row-major, row 0 = top (+y), channels interleaved: float32 [R][R][C].
 */
#ifndef TOPSY_SPLAT_H
#define TOPSY_SPLAT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tsp_context tsp_context;

enum {
    TSP_OK = 0,
    TSP_EINVAL = -1,   /* bad argument */
    TSP_EHIP = -2,     /* HIP runtime error (text in tsp_last_error) */
    TSP_ENODEV = -3,   /* no usable GPU */
    TSP_ESTATE = -4,   /* call order violated (e.g. render before upload / before kernel LUT) */
    TSP_ECOMM = -5,    /* RCCL error */
    TSP_ENOMEM = -6    /* a device allocation failed.  Every entry point that takes a context may return it (the render
                          workspace, the post-pass staging and the scratch of the per-call entry points are allocated on
                          demand): on that return the caller's outputs are untouched, the context -- image, accumulator,
                          statistics, resident particles, their order and its layout -- is as the call found it,
                          tsp_last_error names the allocation, and the context stays usable.  The one exception are the
                          calls that replace the whole snapshot, tsp_upload_particles and tsp_generate_synthetic: they
                          leave no particles resident ("Failed uploads" below) */
};

/* Render modes: which per-particle channels feed the image (reference SPH subclasses). */
enum {
    TSP_MODE_WEIGHTED = 0, /* SPH: ch0 += k*m/h^2, ch1 += k*m/h^2*q      (sph.wgsl:76-83,139-146)  C=2 */
    TSP_MODE_DEPTH = 1,    /* DepthSPH: ch1 weights by clip-space z       (sph.wgsl:86-91)          C=2 */
    TSP_MODE_RGB = 2,      /* RGBSPH: ch0..2 += k*(r,g,b)/h^2, ch3 += 1   (sph.wgsl:69-73,161-165)  C=4 */
    TSP_MODE_KINEMATIC = 3 /* line-of-sight velocity moments: ch0..2 += k*(m, m u, m u^2)/h^2, ch3 += 1 ("Kinematic maps" below)  C=4 */
};

/* Pipeline selection for tsp_render (flags argument). 0 = default (fast three-class pipeline). */
enum {
    TSP_PIPE_DEFAULT = 0,
    TSP_PIPE_GENERIC = 1,  /* single generic kernel, global atomics only (cross-check / debugging) */
    /* Kernel-texture sampling rule.  The default reproduces every golden vector of the
     * reference's tests: bilinear on mip 0 when the footprint is >= 64 px wide (LOD <= 0, mag filter linear,
     * src/topsy/sph.py:425-426), else the NEAREST texel of the mip the rounded LOD selects (min / mipmap filters
     * left at wgpu's default).  The two alternatives below are what a driver with other filter defaults would
     * do; they exist to diagnose such differences and run on the generic kernel only. */
    TSP_SAMPLE_BILINEAR_MIP0 = 0x10,  /* bilinear on mip 0 whatever the footprint width */
    TSP_SAMPLE_BILINEAR_MIP = 0x20    /* bilinear within the mip the rounded LOD selects */
};

const char *tsp_last_error(void);
/* ABI version.  100: first release.  101: tsp_stats grew by 16 bytes (ms_mega, n_mega appended) -- tsp_get_stats
 * writes sizeof(tsp_stats) bytes, so a client compiled against the version-100 header must not be run against a
 * version-101 library (check tsp_version() >= 101 and tsp_stats_size() == sizeof(tsp_stats) at start-up).  The same
 * release narrowed the option "p_small_milli" from <= 22627 to <= 16000 (kernel S packs at most 16 texel columns per
 * footprint; the default moved from 13.5 to 16 px): values 16001..22627 now return TSP_EINVAL.
 * 102: tsp_stats grew by 32 bytes (n_fragments_stream / _mid / _huge / _mega appended); same rule.
 * 103: tsp_stats grew by 8 bytes (n_chunk_culled appended); same rule.  Defaults changed without an ABI change: kernel H3
 * (matrix cores) is an option ("p_mega_px" / "p_mega2_px" default to 0), chunk culling ("chunk_cull") is on.
 * 104: the matrix-core kernels and the round-1 gather kernel are gone (no default rule selected them): the options
 * "p_mega_px", "p_mega2_px", "p_mega_rgb_px", "mega_variant", "rgb_mega_variant", "mega_split", "integrated_px" (kernel I, the
 * inexact option of round 3) and "huge_variant" = 0 / 3 now return TSP_EINVAL; tsp_stats keeps its layout (ms_mega, n_mega and
 * n_fragments_mega are reserved: always 0).  New entry points: tsp_set_reduced_image, tsp_group_shard_range,
 * tsp_group_upload_band_magnitudes.
 * 105: the LDS scatter kernel of the footprints below 64 px (kernel M) is gone -- kernel G, a register gather over per-strip bins of
 * the deferred records, draws them at every size: the options "mid_split" and "debug_extra_lds" return TSP_EINVAL; new options
 * "mid_item_records", "mid_item_scale_milli", "stream_batch_chunks", "debug_gather_full_lut"; "stream_blocks_per_cu" now counts the
 * persistent workgroups of kernel S per CU (0 = as many as stay resident).  No entry point or struct changed.
 * 106: new entry point tsp_smoothing_lengths (k-nearest-neighbour smoothing lengths); nothing else changed.
 * 107: surface rendering: tsp_set_sphere_mips, tsp_density_order_stats, tsp_render_surface, tsp_surface_present and the
 * struct tsp_surface_params; nothing else changed.
 * 108: frame composition: tsp_present and the structs tsp_present_base / tsp_present_layer; nothing else changed.
 * 109: movie frames: tsp_present_yuv420 (the tsp_present frame as I420 planes); nothing else changed.
 * 110: new entry point tsp_sph_sum (gather-form SPH sums: densities for snapshots that carry none); nothing else changed.
 * 111: new entry point tsp_content_neg_inf (how many content values of the last tsp_content_sort were -inf); nothing else changed.
 * 112: surface frames: tsp_present_surface and tsp_present_surface_yuv420 (the lit surface composed onto a canvas of any size under
 * the layers of tsp_present, and that frame as I420 planes); no struct changed, nothing else changed.
 * 113: new entry point tsp_shrink_sphere_center and the struct tsp_center_info (a snapshot's centre); nothing else changed.
 * 114: new entry point tsp_fof_groups and the struct tsp_fof_info (friends-of-friends groups: a halo catalogue for arrays);
 * nothing else changed.
 * 115: new entry point tsp_sphere_moments and the struct tsp_moments (the moments of the particles inside a sphere: what a
 * face-on or side-on orientation is taken from); nothing else changed.
 * 116: new entry point tsp_radial_profile and the structs tsp_profile_spec / tsp_profile_info (binned shell and annulus sums: radial
 * profiles, the virial radius); nothing else changed.
 * 117: kinematic maps: TSP_MODE_KINEMATIC and the entry points tsp_upload_velocities, tsp_set_line_of_sight, tsp_velocity_moments,
 * tsp_colormap_moment; no struct changed, nothing else changed.
 * 118: new entry point tsp_render_undo; tsp_group_render draws a block on every member or on none (it used to leave the block in
 * the accumulators of the members that had succeeded); no struct changed, nothing else changed.
 * 119: kinematic frames: the bases TSP_PRESENT_MOMENT_MEAN / TSP_PRESENT_MOMENT_SIGMA of tsp_present and tsp_present_yuv420 (values
 * that returned TSP_EINVAL before) and the new entry point tsp_moment_sort; no struct changed, nothing else changed.
 * 120: new entry point tsp_sph_velocity_gradient (velocity divergence and curl by SPH gather sums); nothing else changed.
 * 121: a failed upload leaves no half-made state ("Failed uploads" below; it used to leave some arrays new, some old or
 * missing); no entry point or struct changed.
 * 122: new entry point tsp_sph_sample_lattice and the struct tsp_lattice (SPH sums at the points of a lattice: 3-D grids, slices
 * and rays); nothing else changed.
 * 123: new entry point tsp_gravity_direct and the struct tsp_gravity_info (softened direct-sum gravity: the potential and the
 * accelerations at targets, for 'phi' and a disc's rotation curve); nothing else changed.
 * 124: new entry point tsp_gravity_tree and the struct tsp_gravity_tree_info (the same sums by a Barnes-Hut tree over the
 * Morton order, O(n log n)); nothing else changed.
 * 125: new entry points tsp_group_potential and tsp_halo_properties and the structs tsp_group_potential_info / tsp_halo_info (the
 * haloes of a catalogue in one call: self-potential, masses, centres, radii, spin, bound mass); nothing else changed.
 * 126: new entry points tsp_spectral_cube and tsp_spectral_cube_layout (position-position-velocity cubes of the resident
 * particles, "Spectral cubes" below) and the option "cube_slice_particles"; no struct changed, nothing else changed.
 * 127: new entry points tsp_histogram_2d and tsp_histogram_2d_layout and the structs tsp_hist2d_spec / tsp_hist2d_info (weighted 2-D
 * histograms of per-particle quantities: phase diagrams, "Weighted 2-D histograms" below); nothing else changed. */
int tsp_version(void);
int tsp_stats_size(void);

/* Number of visible GPUs (hipGetDeviceCount); <0 on error. Does not create a HIP context. */
int tsp_device_count(void);

/* Create a renderer for one GPU.  Mirrors SPH.__init__ (reference src/topsy/sph.py:50-88):
 * allocates the R x R x C float32 render target.  n_channels: 2 (SPH / DepthSPH, rg32float,
 * sph.py:23) or 4 (RGBSPH, rgba32float, sph.py:432-439). */
int tsp_create(int device_id, int resolution, int n_channels, tsp_context **out);
void tsp_destroy(tsp_context *ctx);

/* Kernel texture: n_levels mip levels of sizes n0, n0/2, ... concatenated, float32
 * (reference SPH._setup_kernel_texture, src/topsy/sph.py:396-426; n0 = 64, n_levels = 4).
 * Sampler semantics are fixed to the reference's: mag linear, min/mip nearest, clamp-to-edge. */
int tsp_set_kernel_mips(tsp_context *ctx, const float *lut, int n0, int n_levels);

/* Particle upload, SoA float32, caller's (global) index order is preserved.
 * Replaces ParticleBuffers.get_pos_smooth_buffers / get_mass_and_quantity_buffers /
 * get_rgb_buffers (reference src/topsy/particle_buffers.py:84-118).
 * mass may be NULL for a context that will only render TSP_MODE_RGB.
 *
 * Failed uploads.  Every device allocation of the uploads is made before the first copy, kernel or change of state.
 *   1. Attribute uploads (tsp_upload_quantity, tsp_upload_rgb, tsp_upload_velocities, tsp_upload_band_magnitudes): a call that returns TSP_ENOMEM has changed nothing -- the
 *      resident arrays (bit for bit), the cached vertex weights and what they were formed from, the validity of
 *      tsp_render_undo, the image and the statistics are as before the call, and what the call allocated is freed.  Arrays
 *      that are resident already are written in place, never freed and allocated again (n cannot change between two particle
 *      uploads), so a repeated upload of an attribute allocates only the staging of the load-time permutation, if any.
 *   2. Replace-all uploads (tsp_upload_particles, tsp_generate_synthetic) free the old snapshot FIRST -- keeping it would
 *      double the peak memory of a 1e9-particle snapshot -- so a call that fails (TSP_ENOMEM or TSP_EHIP) leaves the context
 *      holding no particles, exactly as after tsp_upload_particles(ctx, 0, ...): tsp_num_particles is 0, there is no
 *      per-particle array, permutation, strata or cell grid; the image, the statistics, the LUTs and the options are
 *      untouched.  Every attribute upload then returns TSP_ESTATE and tsp_render draws nothing.
 *   3. tsp_render and tsp_render_surface return TSP_ESTATE for a context with n > 0 whose x, y, z or h array is missing,
 *      next to their checks of the mass, rgb and velocity arrays: no half-made context reaches a kernel.
 *   4. Groups: see "Several GPUs of one node behind ONE handle" at the end of this file. */
int tsp_upload_particles(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z,
                         const float *h, const float *mass);
/* q == NULL selects the density render (reference uploads q = 0 then, particle_buffers.py:96-99;
 * quantity swap: src/topsy/visualizer.py:294-309). */
int tsp_upload_quantity(tsp_context *ctx, const float *q);
int tsp_upload_rgb(tsp_context *ctx, const float *r, const float *g, const float *b);
/* The same three channels computed ON the device from SSP band magnitudes -- the 3 x n_bands "band contraction" of the
 * rgb render mode: channel_c[i] = sum_b weights[c * n_bands + b] * 10^(-0.4 * mags[b * n + i]), NaN -> 0, evaluated in
 * float64 and rounded to float32 once.  With weights = diag(0.5, 1, 1) over the bands (I, V, U) this is the reference's
 * PynbodyDataInMemory.get_rgb_masses / _effective_mass_for_band (src/topsy/loader.py:112-121).  mags: n_bands arrays of n
 * float64 each, contiguous, caller's particle order.  An HBM-bound VALU kernel (8 n_bands bytes in, 12 bytes out and
 * 3 n_bands FMAs per particle): the matrix cores have nothing to gain here. */
int tsp_upload_band_magnitudes(tsp_context *ctx, int n_bands, const double *mags, const double *weights);

/* On-device synthetic snapshot = restatement of topsy.loader.TestDataLoader's distribution
 * (reference src/topsy/loader.py:241-332) with a counter-based generator, so that shard
 * [first, first+count) of an n_total-particle snapshot is reproducible on any GPU without
 * materialising n_total rows on the host.  h_cap > 0 caps the smoothing length (bandwidth-bound
 * variant of BASELINE.md section 3); with_quantity / with_rgb also fill q / rgb. */
int tsp_generate_synthetic(tsp_context *ctx, int64_t n_total, int64_t first, int64_t count,
                           uint64_t seed, float h_cap, int with_quantity, int with_rgb);

/* Load-time spatial ordering (the analogue of the reference's CellLayout sort at load,
 * src/topsy/loader.py:88-97): reorders the resident particles into n_strata uniform random
 * strata, each Morton-sorted, so that index prefixes remain unbiased samples (progressive
 * rendering) while consecutive indices are screen-coherent.  perm_out (optional, host, n
 * int64) receives new->old indices.  Later tsp_upload_quantity/rgb calls are given in the OLD
 * order and permuted by the library.  A second call sorts the particles as they lie then and
 * reports new->ORIGINAL indices.
 * The key of particle i is stratum << 48 | Morton code of its position quantised to 16 bits per
 * axis over the bounding box of the FINITE coordinates (float32: (x - lo) * (65535 / (max - min)),
 * truncated), stratum = splitmix64(seed ^ i) % n_strata.  The sort is stable: particles with
 * equal keys (equal positions, among others) keep their index order.  Non-finite coordinates are
 * outside the box: NaN and -inf quantise to the lowest step of their axis, +inf to the highest;
 * an axis without any finite value, or with a single one, has one step. */
int tsp_reorder_spatial(tsp_context *ctx, int n_strata, uint64_t seed, int64_t *perm_out);
/* First index of every stratum of the last tsp_reorder_spatial call, plus the particle count:
 * n_strata + 1 ascending int64 values.  A contiguous index range is an unbiased spatial sample only
 * when it is a union of whole strata, so the progressive renderer ends its blocks on these offsets
 * (the reference gets the same property from its per-cell random order, src/topsy/progressive_render.py:152-187).
 * Returns the number of values written (<= capacity), 0 when the particles were never reordered. */
int tsp_get_strata_offsets(tsp_context *ctx, int64_t *offsets_out, int capacity);

/* View culling on the library's own ordering (the role of the reference's CellLayout and
 * RenderProgressionWithCells._map_logical_range_to_actual_ranges, src/topsy/cell_layout.py:26-31,63-113,
 * src/topsy/progressive_render.py:152-187,207-220).  Inside a stratum the Morton order stores the particles of every cell
 * of a cells_per_axis^3 grid over the snapshot's bounding box as ONE contiguous run.  tsp_get_cell_layout reports the grid
 * (cells_per_axis = 2^k, the largest k <= 4 with >= 16 particles per (stratum, cell) on average; cell (cx, cy, cz) covers
 * box_lo + (cx, cy, cz) * cell_width ... + cell_width per axis), tsp_get_cell_offsets the first index of every run:
 * n_strata * cells_per_axis^3 + 1 ascending int64 values, entry s * cells^3 + code for stratum s and Morton cell code
 * (bit 3 j of the code = bit j of cx, bit 3 j + 1 = bit j of cy, bit 3 j + 2 = bit j of cz), the last entry = n.
 * The host selects the cells that meet the view sphere and hands tsp_render the (start, len) runs of those cells.
 * The grid is honest for every snapshot: a particle that is finite on all axes lies inside the box its run's cell is
 * reported to cover (to float32 rounding, far inside the one-cell-diagonal margin the host adds).  Where float32 gives
 * out the library goes on in another way instead of reporting cell_width = 0 for particles that differ: an axis whose
 * extent max - min overflows float32 (sentinel rows at +-3e38) is quantised in float64; its cell_width is finite (about
 * extent / cells_per_axis) except with cells_per_axis = 1, where 2^16 / inv overflows and cell_width = +inf is
 * reported -- a cell whose centre or diagonal is not finite must be selected; an
 * axis so narrow that 65535 / (max - min) overflows (a few denormals) is quantised with FLT_MAX steps per unit.
 * cell_width = 0 means that every finite coordinate of the axis is box_lo (0 when the axis has none).
 * tsp_get_cell_offsets returns the number of values written (<= capacity), 0 when the particles were never reordered. */
int tsp_get_cell_layout(tsp_context *ctx, int *n_strata_out, int *cells_per_axis_out, float *box_lo_out /*3*/,
                        float *cell_width_out /*3*/);
int64_t tsp_get_cell_offsets(tsp_context *ctx, int64_t *offsets_out, int64_t capacity);

/* Copy resident particle arrays back (testing / fixtures). Any pointer may be NULL. */
int tsp_download_particles(tsp_context *ctx, float *x, float *y, float *z, float *h, float *mass,
                           float *q, float *r, float *g, float *b);
int64_t tsp_num_particles(tsp_context *ctx);

/* One render block.  Replaces the body of SPH.render's loop (reference src/topsy/sph.py:318-326:
 * encode_render_pass(clear) + update_particle_ranges(starts, lens) + timed queue.submit).
 *   M             row-major 4x4, clip = M * (x,y,z,1)  (= transpose of the reference's uploaded
 *                 "transform", src/topsy/sph.py:268-289)
 *   scale_factor  1/scale (sph.wgsl:58)
 *   starts/lens   n_ranges particle index ranges (first_instance, instance_count of the
 *                 reference's indirect draws, particle_buffers.py:76-82); NULL = all particles
 *   clear         1 = clear the target first (load_op clear, sph.py:346)
 *   mode          TSP_MODE_*
 *   flags         TSP_PIPE_*
 *   gpu_ms_out    optional: GPU time of this block (hipEvent pair) -- the TimeGpuOperation hook
 * A block of any size draws (the deferred-footprint lists go through the tile kernels in slices), and it draws whole or not at
 * all: on any error return the accumulator, the image, the channel layout and tsp_stats are as the call found them. */
int tsp_render(tsp_context *ctx, const float *M, float scale_factor, const int64_t *starts,
               const int64_t *lens, int n_ranges, int clear, int mode, int flags, double *gpu_ms_out);

/* Takes the last tsp_render back: for a driver that runs one block on several contexts and must leave it drawn on all of them or
 * on none (tsp_group_render does this itself).  Valid only while tsp_render is the last call that changed this context's image
 * -- no tsp_write_image, tsp_set_reduced_image, tsp_comm_reduce_image, tsp_tile_periodic, tsp_render_surface, upload or reorder
 * since, and not when that tsp_render replaced a surface image; otherwise TSP_ESTATE, and nothing changes.
 *   - After a tsp_render that succeeded: the accumulator, the channel layout, tsp_stats and what the image remembers of its mode
 *     (rgb / kinematic, the line of sight) are as that call found them.
 *   - After a tsp_render that failed there is nothing to put back (it draws whole or not at all).
 * In both cases the float32 image is formed again from the accumulator and the context counts as not reduced, so the driver's
 * next reduce sums every member's partial image anew.  A second call returns TSP_ESTATE.  Allocates nothing. */
int tsp_render_undo(tsp_context *ctx);

/* Read the render target (R*R*C float32).  SPH._get_image_unscaled, src/topsy/sph.py:127-140. */
int tsp_read_image(tsp_context *ctx, float *out);
/* Overwrite the render target from the host (testing the colormap on a known buffer). */
int tsp_write_image(tsp_context *ctx, const float *in);

/* Colormap post-pass on the resident render target -> RGBA8 (R*R*4 bytes, RGBA order).
 * scalar: colormap.wgsl fragment_main non-bivariate branch (:113-127); lut = n_lut x RGBA float32
 * (Colormap._generate_mapping_rgba_f32, implementation.py:235-238); vmin/vmax are the
 * already-scaled shader parameters (Colormap._update_parameter_buffer, implementation.py:427-453). */
int tsp_colormap_scalar(tsp_context *ctx, const float *lut_rgba, int n_lut, float vmin, float vmax,
                        int log_scale, int weighted, uint8_t *out_rgba);
/* rgb: colormap.wgsl fragment_main_tri + gamma_map (:131-159).  out_rgba8 and/or out_rgba_f32
 * (unclamped, the HDR canvas value) may be NULL. */
int tsp_colormap_rgb(tsp_context *ctx, float vmin, float vmax, float gamma, uint8_t *out_rgba8,
                     float *out_rgba_f32);

/* Bivariate map: colormap.wgsl fragment_main BIVARIATE branch (:91-111) with
 * the 2-D LUT of BivariateColormap._generate_mapping_rgba_f32 (implementation.py:585-605), n x n x RGBA
 * float32, first axis = normalised (weighted) value, second axis = normalised log10 density.  The LUT
 * (16 MB at n = 1000) is uploaded once with tsp_colormap_set_lut2d and stays resident. */
int tsp_colormap_set_lut2d(tsp_context *ctx, const float *lut_rgba, int n);
int tsp_colormap_bivariate(tsp_context *ctx, float vmin, float vmax, float density_vmin, float density_vmax,
                           int log_scale, int weighted, uint8_t *out_rgba);
int tsp_colormap_bivariate_host(tsp_context *ctx, const float *img, int H, int W, int C, float vmin, float vmax,
                                float density_vmin, float density_vmax, int log_scale, int weighted,
                                uint8_t *out_rgba);

/* Same maps applied to an arbitrary host image (H x W x C float32), the entry
 * Colormap.sph_raw_output_to_image drives (implementation.py:132-201). */
int tsp_colormap_scalar_host(tsp_context *ctx, const float *img, int H, int W, int C,
                             const float *lut_rgba, int n_lut, float vmin, float vmax, int log_scale,
                             int weighted, uint8_t *out_rgba);
int tsp_colormap_rgb_host(tsp_context *ctx, const float *img, int H, int W, int C, float vmin,
                          float vmax, float gamma, uint8_t *out_rgba8, float *out_rgba_f32);

/* Periodic tiling post-pass: replaces the render target by the weighted sum
 * of n shifted copies of itself -- PeriodicSPH.render + PeriodicSPHAccumulationOverlay (reference
 * src/topsy/periodic_sph.py:36-88, shaders/overlay.wgsl:18-51): one full-viewport quad per instance
 * displaced by offsets_xy[k] (clip units, +y up), sampled with a linear filter and clamp-to-edge,
 * additively blended into a cleared target.  The float64 accumulator keeps the untiled render, so a
 * later tsp_render(clear = 0) continues from the raw image and the tiling is re-applied afterwards.  TSP_ESTATE, nothing changed,
 * while the accumulator holds the keys of tsp_render_surface (a surface image has no tiling). */
int tsp_tile_periodic(tsp_context *ctx, int n, const float *offsets_xy, const float *weights);

/* SPH smoothing lengths by k-nearest neighbours (the pynbody.sph.smooth call of reference loader.py:222-240).
 * Host arrays in and out; uses ctx's device and stream only: resident particles, image, accumulator and tsp_stats unchanged.
 * For a particle i with finite coordinates, h_out[i] = 0.5f * sqrtf(k-th smallest d2) over every j with finite coordinates
 * (j = i included, at distance 0; ties and duplicates count), where in float32 with these operations in this order
 *     dx = x[j] - x[i] (dy, dz alike);  period > 0 only: t = dx / period; t = rint(t); dx = dx - (period * t);
 *     d2 = (dx * dx + dy * dy) + dz * dz,
 * k = n_neighbours.  A particle with a non-finite coordinate gets NaN and is nobody's neighbour.  2 <= n_neighbours <= 64,
 * period = 0 (open box) or finite and > 0, 1 <= n < 2^31, at least n_neighbours particles with finite coordinates; anything
 * else returns TSP_EINVAL and writes nothing.  Device memory is allocated for the call only (about 48 bytes per particle);
 * a failed allocation returns TSP_ENOMEM. */
int tsp_smoothing_lengths(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z,
                          int n_neighbours, float period, float *h_out);

/* Gather-form SPH sum at the particles: with a = mass, the density pynbody derives as snapshot['rho'].
 * Host arrays in and out, caller's order; uses ctx's device and stream only: resident particles, image, accumulator and
 * tsp_stats unchanged.  Float32 unless said otherwise, with these operations in this order (no fused multiply-adds):
 *   - Particle i is valid iff x[i], y[i], z[i] are finite.  A query i is answerable iff it is valid and h[i] is finite and > 0.
 *     out[i] = NaN for a query that is not answerable.  Invalid particles are nobody's neighbour.  a[j] is used as given (a NaN
 *     or infinite a[j] propagates into the sums it takes part in).
 *   - For an answerable i, over every valid j (j = i included):
 *         dx, dy, dz, d2 exactly as tsp_smoothing_lengths defines them (nearest image when period > 0);
 *         u = sqrtf(d2) / h[i];  the term exists iff u < 2;
 *         u2 = u * u;  w = u < 1 ? (1 - 1.5f * u2) + 0.75f * (u2 * u) : 0.25f * ((t * t) * t) with t = 2 - u;
 *         term = a[j] * w;  S += (double)term  (float64 sum, any order);
 *     out[i] = (float)(S / (M_PI * (double)((h[i] * h[i]) * h[i]))).
 *     This is the M4 cubic spline with support 2h in gather form (the query's own h).  With a = mass and h from
 *     tsp_smoothing_lengths(k) the sum runs over the k - 1 nearest neighbours and the particle itself (the k-th sits at u = 2
 *     exactly and is excluded).
 *   - The order of the sum is free but fixed (no atomics in it): the same call on the same input and device returns the same
 *     bits; for a >= 0 any two orders agree to within one float32 ulp of out[i].
 * 1 <= n < 2^31, period = 0 (open box) or finite and > 0, no NULL array; anything else returns TSP_EINVAL and writes nothing.
 * There is no limit on the number of neighbours: the cost is proportional to the candidates scanned, so a caller's own very
 * large h is slow, not wrong.  Device memory is allocated for the call only (about 56 bytes per particle); a failed allocation
 * returns TSP_ENOMEM and writes nothing. */
int tsp_sph_sum(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, const float *h,
                const float *a, float period, float *out);

/* Divergence and curl of the velocity at the particles by SPH gather sums: what pynbody derives as 'v_div' and 'v_curl' (the
 * norm of the curl is its 'vorticity').  Host arrays in and out, caller's order; uses ctx's device and stream only: resident
 * particles, image, accumulator and tsp_stats unchanged.  Float32 unless said otherwise, with these operations in this order (no
 * fused multiply-adds):
 *   - Particle i is valid iff x[i], y[i], z[i] are finite.  A query i is answerable iff it is valid and h[i] is finite and > 0.
 *     The four outputs of a query that is not answerable are NaN.  Invalid particles are nobody's neighbour.  mass, rho, vx, vy,
 *     vz are used as given (a NaN or an infinity propagates into every sum it takes part in).
 *   - For an answerable i, over every valid j:
 *         dx, dy, dz, d2 exactly as tsp_smoothing_lengths defines them (x[j] - x[i], nearest image when period > 0);
 *         u = sqrtf(d2) / h[i];  the term exists iff d2 > 0 and u < 2 (the particle itself and exact duplicates contribute
 *         nothing);
 *         t = 2 - u;  f = u < 1 ? 3.0f - 2.25f * u : (0.75f * (t * t)) / u      (-w'(u) / u of the M4 spline w of tsp_sph_sum);
 *         c = mass[j] * f;  dvx = vx[j] - vx[i] (dvy, dvz alike);
 *         term_div = c * ((dvx * dx + dvy * dy) + dvz * dz);
 *         term_cx = c * (dy * dvz - dz * dvy);  term_cy = c * (dz * dvx - dx * dvz);  term_cz = c * (dx * dvy - dy * dvx);
 *         four float64 sums, S += (double)term.
 *     hd = (double)h[i];  den = M_PI * (((hd * hd) * (hd * hd)) * hd) * (double)rho[i];  each output is (float)(S / den).
 *   - The order of the sums is free but fixed (no atomics in them): the same call on the same input and device returns the same
 *     bits.  Two orders differ by the float64 rounding of the sums only: with T terms and A = sum |term| / |den|, by at most
 *     2 T 2^-53 A before the rounding to float32.
 * This is the usual difference-form estimate, pynbody's convention:
 *     div v_i = (1 / rho_i) sum_j m_j (v_j - v_i) . grad_i W(r_ij, h_i),   curl v_i = (1 / rho_i) sum_j m_j grad_i W x (v_j - v_i),
 * with rho from tsp_sph_sum(a = mass) on the same h.  It is exactly zero for a uniform velocity field.  It is not exact for a
 * linear one, and it is biased low on disordered particles, because rho_i contains the self term and the sums do not: for
 * v = A x it returns about 0.77 of trace(A) and of the antisymmetric part on Poisson points with 32 neighbours, 0.981 on a cubic
 * lattice with h = 1.2 spacings.  (A matrix-corrected, linear-exact estimator is a different sum.)
 * 1 <= n < 2^31, period = 0 (open box) or finite and > 0, no NULL array (the outputs included); anything else returns
 * TSP_EINVAL and writes nothing.  The cost is proportional to the candidates scanned, as for tsp_sph_sum.  Device memory is
 * allocated for the call only (about 88 bytes per particle: the index and h as for tsp_sph_sum, 20 for the five fields, 16 for
 * the (mass, velocity) records in Morton order; the results reuse what is free by then); a failed allocation returns TSP_ENOMEM and
 * writes nothing. */
int tsp_sph_velocity_gradient(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, const float *h,
                              const float *mass, const float *rho, const float *vx, const float *vy, const float *vz,
                              float period, float *div_out, float *curl_x_out, float *curl_y_out, float *curl_z_out);

/* SPH sums at the points of a lattice: "what is the density, or the temperature, at this point in space?" on a regular 3-D grid
 * (pynbody's to_3d_grid), a slice or a ray.  Host arrays in and out; uses ctx's device and stream only: resident particles, image,
 * accumulator and tsp_stats unchanged.  The estimator is gather-form with the smoothing length taken at the sample point (yt's
 * "gather" smoothing).  Float32 unless said otherwise, with these operations in this order (no fused multiply-adds):
 *   - The lattice.  nq = nu * nv * nw points; point (i, j, k), 0 <= i < nu, 0 <= j < nv, 0 <= k < nw, has on every axis the
 *     coordinate ((origin + (double)i * du) + (double)j * dv) + (double)k * dw in float64, rounded once to float32.  The
 *     outputs are C-ordered [k][j][i], i fastest.  The point is used as it is: in a periodic box it may lie outside [0, period),
 *     the wrap happens inside the distances only.
 *   - Particle j is valid iff x[j], y[j], z[j] are finite; invalid particles are nobody's neighbour and contribute nothing.
 *   - For a lattice point r, over every valid j: d2_j exactly as tsp_smoothing_lengths defines it, with dx = x[j] - r.x (nearest
 *     image when period > 0).  h(r) = 0.5f * sqrtf(the n_neighbours-th smallest d2_j): the rule of tsp_smoothing_lengths, except
 *     that no particle is the query itself (one that coincides with r counts like any other).  h_out[r] = h(r) as computed
 *     (h_out may be NULL).
 *   - For each of the n_fields fields a_f (1 <= n_fields <= 4), over every valid j:
 *         u = sqrtf(d2_j) / h(r);  the term exists iff u < 2 (the n_neighbours-th neighbour itself, at u == 2, contributes nothing);
 *         u2 = u * u;  w = u < 1 ? (1 - 1.5f * u2) + 0.75f * (u2 * u) : 0.25f * ((t * t) * t) with t = 2 - u   (tsp_sph_sum's w);
 *         term = a_f[j] * w;  S_f += (double)term  (float64 sum, any order);
 *     outs[f][r] = (float)(S_f / (M_PI * (double)((h * h) * h))) with h = h(r).
 *     Where h(r) is not finite or is 0 (n_neighbours particles sit exactly on the point) every field at that point is NaN.  a_f[j]
 *     is used as given: a NaN or an infinity propagates into the points whose sums it takes part in, and only those.
 *     With a = mass this is the density at r; with a_0 = mass * q and a_1 = mass, outs[0] / outs[1] is the kernel-weighted mean
 *     of q at r, and no per-particle rho is needed.
 *   - The order of the sums is free but fixed (no atomics in them): the same call on the same input and device returns the same
 *     bits; for a_f >= 0 any two orders agree to within one float32 ulp of the output.
 * TSP_EINVAL, and nothing written: a NULL argument (h_out aside); n_fields outside [1, 4]; n, n_neighbours or period that
 * tsp_smoothing_lengths refuses; fewer than n_neighbours valid particles; nu, nv or nw below 1 or nq >= 2^31; a lattice number
 * that is not finite, or a lattice point that rounds to a float32 that is not finite.  The cost is that of a k-NN search and a
 * range sum per lattice point.  Device memory is allocated for the call only (the index of tsp_smoothing_lengths, 4 n_fields
 * bytes per particle twice, and 4 (1 + n_fields) bytes per lattice point); a failed allocation returns TSP_ENOMEM and writes
 * nothing. */
typedef struct {
    double origin[3], du[3], dv[3], dw[3];
    int32_t nu, nv, nw;
} tsp_lattice;
int tsp_sph_sample_lattice(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, int n_fields,
                           const float *const *fields, int n_neighbours, float period, const tsp_lattice *lattice,
                           float *h_out /* nq floats, may be NULL */, float *const *outs /* n_fields pointers to nq floats */);

/* The shrinking-sphere centre of a snapshot (Power et al. 2003): what pynbody.analysis.halo.center computes by default and the
 * reference asks for when it centres a snapshot at load (PynbodyDataLoader._perform_centering, src/topsy/loader.py:201-217, with
 * center = "all" or "zoom").  Host arrays in, caller's order; uses ctx's device and stream only: resident particles, image,
 * accumulator and tsp_stats unchanged.  Float64 throughout unless said otherwise (no fused multiply-adds):
 *   - Valid particles.  Particle i is valid iff x[i], y[i], z[i], mass[i] are finite and mass[i] > 0.  With mass_cut_factor > 0 it
 *     must also satisfy (double)mass[i] < (double)mass_cut_factor * (double)m_min, where m_min is the smallest mass among the
 *     otherwise valid particles (the reference's "zoom" rule, mass < 1.01 * mass.min()); mass_cut_factor == 0: no selection.
 *   - Initial centre.  c = sum m p / sum m over the valid particles (m = (double)mass[i], p = the (double) coordinates).
 *   - Initial radius.  r = r_start if r_start > 0, else ((double)max x - (double)min x) / 2 over the valid particles (pynbody's
 *     rough estimate).
 *   - Loop, until max_iterations updates have been done:
 *       1. r_try = r * shrink_factor;
 *       2. the inside set: the valid i with d2 < r_try * r_try (strict), where dx = (double)x[i] - c[0] (dy, dz alike) and
 *          d2 = (dx * dx + dy * dy) + dz * dz;
 *       3. fewer than min_particles members: stop, c and r stay;
 *       4. else c += sum m (dx, dy, dz) / sum m over the set, r = r_try, one more iteration.
 *     The displacements are summed from the current centre, so the rounding error is proportional to r and not to |p|: a
 *     snapshot sitting at 1e4 with structure at 1e-2 is centred as well as one at the origin.
 *   - Outputs.  center_out = the final c.  info_out (optional): n_valid, iterations = the updates done, radius = the final r,
 *     n_inside and mass_inside = the count and sum m of the last accepted inside set -- of all valid particles when no update
 *     happened; reserved = 0.
 *   - The order of every sum is free but fixed (no floating-point atomics; per-wave and per-workgroup partial sums are combined in
 *     a fixed order): the same call on the same input and device returns the same bits.  Counts are integers.
 * 1 <= n < 2^31, no NULL array or center_out, 0 < shrink_factor < 1, min_particles >= 1, 0 <= max_iterations <= 256, r_start = 0
 * or finite and > 0, mass_cut_factor = 0 or finite and > 1, at least one valid particle; anything else returns TSP_EINVAL and
 * writes nothing.  pynbody's defaults: shrink_factor 0.7, min_particles 100.  Not provided: periodic wrapping of the displacements.
 * Device memory is allocated for the call only (about 16 bytes per particle); a failed allocation returns TSP_ENOMEM and writes
 * nothing.  The cost is one 16-byte-per-particle pass per iteration, less the blocks of 1024 consecutive particles whose bounding
 * box lies outside the sphere: those are not read (identical results; pays with a spatial order of the arrays). */
typedef struct {
    int64_t n_valid, n_inside;
    int32_t iterations, reserved;
    double radius, mass_inside;
} tsp_center_info;
int tsp_shrink_sphere_center(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, const float *mass,
                             float mass_cut_factor, double r_start, double shrink_factor, int64_t min_particles,
                             int max_iterations, double center_out[3], tsp_center_info *info_out);

/* Friends-of-friends groups: the halo catalogue that arrays do not carry, which the reference's center = "halo-N" takes from
 * pynbody (PynbodyDataLoader._perform_centering, src/topsy/loader.py:203-206).  Host arrays in and out, caller's order; uses
 * ctx's device and stream only: resident particles, image, accumulator and tsp_stats unchanged.
 *   - Valid particles.  Particle i is valid iff x[i], y[i], z[i] are finite.  An invalid particle gets group_out[i] = -1 and is
 *     nobody's friend, so it never bridges two groups.
 *   - Links.  Two valid particles i != j are linked iff d2 <= ll2, where d2 is exactly the float32 expression
 *     tsp_smoothing_lengths defines (period > 0: the nearest image by dx - period * rint(dx / period)) and
 *     ll2 = linking_length * linking_length in float32.  A pair at exactly ll2 is linked.  Every step of d2 is odd-symmetric in
 *     dx, so d2(i, j) and d2(j, i) are the same bits: the relation is symmetric.
 *   - Groups.  The connected components of that graph; the size of a group is its member count.  The groups with
 *     size >= min_members are ranked 1, 2, ... by size descending, ties by the smaller smallest member index (caller's order).
 *     group_out[i] = the rank of i's group, or 0 for a valid particle whose group is too small.
 *   - info_out (optional): n_valid; n_groups = the number of ranked groups; n_grouped = the particles with rank >= 1;
 *     largest = the size of group 1, or 0.
 *   - Determinism.  Everything is an integer and the partition is unique: the same input gives the same output whatever order
 *     the atomics of the union-find resolve in.
 * 1 <= n < 2^31, linking_length finite and > 0, period = 0 (open box) or finite and > 0 with linking_length < period / 2,
 * min_members >= 1, no NULL array; anything else returns TSP_EINVAL and writes nothing.  The cost is proportional to the
 * candidates tested: a linking length of the order of the box is slow, not wrong.  Device memory is allocated for the call only
 * (about 48 bytes per particle); a failed allocation returns TSP_ENOMEM and writes nothing. */
typedef struct {
    int64_t n_valid, n_groups, n_grouped, largest;
} tsp_fof_info;
int tsp_fof_groups(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, float linking_length,
                   float period, int64_t min_members, int32_t *group_out, tsp_fof_info *info_out);

/* The moments of the particles inside a sphere: what pynbody.analysis.angmom.faceon / sideon take a disc's orientation from (the
 * mean velocity of a small sphere, then the angular momentum of a larger one about it), and the second-moment tensor for
 * snapshots without velocities.  Host arrays in, caller's order; uses ctx's device and stream only: resident particles, image,
 * accumulator and tsp_stats unchanged.  Float64 throughout unless said otherwise (no fused multiply-adds):
 *   - Velocities.  vx, vy, vz are all given or all NULL.
 *   - Valid particles.  Particle i is valid iff x[i], y[i], z[i], mass[i] (and vx[i], vy[i], vz[i] when given) are finite and
 *     mass[i] > 0.  m = (double)mass[i].
 *   - Membership.  dx = (double)x[i] - center[0] (dy, dz alike), d2 = (dx * dx + dy * dy) + dz * dz, d = (dx, dy, dz).  A valid
 *     particle is inside the r sphere iff d2 < r * r (strict), inside the r_vel sphere iff d2 < r_vel * r_vel.
 *   - Pass A, only with velocities: n_inside_vel, mass_vel = sum m and sum m v over the r_vel sphere, v = the (double)
 *     velocities; v_cen = sum m v / mass_vel.  Without velocities n_inside_vel = 0, mass_vel = 0, v_cen = 0.
 *   - Pass B, over the r sphere: n_inside; mass = sum m; com = sum m d / mass (the offset of the centre of mass from center);
 *     S = sum m d_i d_j in the order xx, xy, xz, yy, yz, zz, each term (m * d_i) * d_j.  With velocities, u = v - v_cen:
 *       L_x = sum m * (dy * u_z - dz * u_y), L_y = sum m * (dz * u_x - dx * u_z), L_z = sum m * (dx * u_y - dy * u_x);
 *       A = sum (m * sqrt(d2)) * sqrt((u_x * u_x + u_y * u_y) + u_z * u_z): the scale of L's rounding, and |L| / A the degree of
 *       ordered rotation.  Without velocities L = 0 and A = 0.
 *     The displacements are formed in float64 before anything is multiplied, so the rounding error is proportional to r and not
 *     to |center|.
 *   - n_valid counts the valid particles, inside or not.
 *   - The order of every sum is free but fixed (no floating-point atomics; per-wave and per-workgroup partial sums are combined in
 *     a fixed order, the grid is a function of n and the device): the same call on the same input and device returns the same
 *     bits.  Counts are integers.
 * 1 <= n < 2^31; no NULL among x, y, z, mass, center, out; center finite; r finite and > 0; with velocities r_vel finite and
 * 0 < r_vel <= r, without r_vel = 0; at least one valid particle; anything else returns TSP_EINVAL and writes nothing.  So does an
 * r sphere or, with velocities, an r_vel sphere without a valid particle inside: tsp_last_error names the sphere.  Not provided:
 * periodic wrapping of the displacements.  Device memory is allocated for the call only (about 16 bytes per particle, 28 with
 * velocities); a failed allocation returns TSP_ENOMEM and writes nothing.  The cost is one pass per sphere over those bytes, less
 * the blocks of 1024 consecutive particles whose bounding box lies outside the sphere: those are not read (identical results; pays
 * with a spatial order of the arrays, and makes the r_vel pass almost free there). */
typedef struct {
    int64_t n_valid, n_inside, n_inside_vel;   /* valid particles; inside r; inside r_vel (0 without velocities) */
    double  mass, mass_vel;                    /* sum m inside r / inside r_vel */
    double  com[3];                            /* sum m d / mass        (offset of the centre of mass from center) */
    double  v_cen[3];                          /* sum m v / mass_vel over the r_vel sphere; zeros without velocities */
    double  L[3];                              /* sum m d x (v - v_cen) over the r sphere; zeros without velocities */
    double  S[6];                              /* sum m d_i d_j over the r sphere: xx, xy, xz, yy, yz, zz */
    double  A;                                 /* sum m |d| |v - v_cen| over the r sphere (the scale of L's rounding) */
} tsp_moments;
int tsp_sphere_moments(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, const float *mass,
                       const float *vx, const float *vy, const float *vz,      /* all three or none (NULL) */
                       const double center[3], double r, double r_vel, tsp_moments *out);

/* Radial profiles: per radial bin the count and eleven sums of the particles in it, in spherical shells or in the cylindrical
 * annuli of a disc -- what pynbody.analysis.profile.Profile (density, rotation curve, dispersions, specific angular momentum) and
 * pynbody.analysis.halo.virial_radius are built from.  Host arrays in, caller's order; uses ctx's device and stream only: resident
 * particles, image, accumulator and tsp_stats unchanged.  Float64 throughout (no fused multiply-adds), every expression in the
 * order written here:
 *   - Velocities.  vx, vy, vz are all given or all NULL.
 *   - Valid particles.  As tsp_sphere_moments: particle i is valid iff x[i], y[i], z[i], mass[i] (and vx[i], vy[i], vz[i] when
 *     given) are finite and mass[i] > 0.  m = (double)mass[i].  n_valid counts them, binned or not.
 *   - Displacements.  dx = (double)x[i] - center[0] (dy, dz alike), d = (dx, dy, dz), formed in float64 before anything is
 *     multiplied.  With F = frame (row-major, F[3 * r + c]):
 *       x' = (F[0] * dx + F[1] * dy) + F[2] * dz, y' = (F[3] * dx + F[4] * dy) + F[5] * dz, z' = (F[6] * dx + F[7] * dy) + F[8] * dz.
 *     With velocities u = ((double)vx[i] - v_cen[0], ...) and u' = F u formed in the same way (ux', uy', uz').
 *   - Bin coordinate.  R2 = x' * x' + y' * y'.  Geometry 0 (shells): s2 = (dx * dx + dy * dy) + dz * dz, from the unrotated d, so
 *     that membership does not depend on the frame.  Geometry 1 (annuli about the frame's third axis): s2 = R2, and the particle
 *     takes part only if fabs(z') <= half_height.
 *   - Bin.  E2[k] = edges[k] * edges[k], k = 0 .. n_bins.  A valid particle (geometry 1: that takes part) is in bin k iff
 *     E2[k] <= s2 < E2[k + 1]; with s2 < E2[0] it is counted in n_inner and its m in mass_inner; with s2 >= E2[n_bins] it is
 *     counted nowhere.  count_out[k] = the members of bin k; n_binned = their total.
 *   - Sums.  sums_out[k * 11 + j] over the members of bin k, each starting at +0.0, with s = sqrt(s2):
 *       j = 0: sum m;  j = 1: sum m * s;
 *       j = 2, 3, 4: sum m * c_0, m * c_1, m * c_2;  j = 5, 6, 7: sum (m * c_0) * c_0, (m * c_1) * c_1, (m * c_2) * c_2;
 *       j = 8, 9, 10: sum m * (dy * uz - dz * uy), m * (dz * ux - dx * uz), m * (dx * uy - dy * ux): the angular momentum about
 *       center and v_cen in the caller's frame, formed as L of tsp_sphere_moments.
 *     Without velocities j = 2 .. 10 are +0.0.
 *   - Components c.  R = sqrt(R2);  eRx = x' / R and eRy = y' / R if R > 0, else eRx = 1 and eRy = 0 (so e_R = (eRx, eRy, 0) and
 *     e_phi = (-eRy, eRx, 0), on the axis (1, 0, 0) and (0, 1, 0)).
 *       c_1 = eRx * uy' - eRy * ux'                                             (u_phi, both geometries)
 *       Geometry 1, the cylindrical triad (u_R, u_phi, u_z):  c_0 = eRx * ux' + eRy * uy',  c_2 = uz'.
 *       Geometry 0, the spherical triad (u_r, u_phi, u_theta):  D = sqrt(R2 + z' * z');  erx = x' / D, ery = y' / D, erz = z' / D if
 *       D > 0, else (0, 0, 1);  c_0 = (erx * ux' + ery * uy') + erz * uz';  with e_theta = e_phi x e_r,
 *       c_2 = ((eRx * erz) * ux' + (eRy * erz) * uy') - (eRx * erx + eRy * ery) * uz'.
 *   - Determinism.  No floating-point atomics; the order of every sum is free but fixed (per-wave sums are added to a workgroup's
 *     table in wave order, the workgroups' tables in index order; the grid is a function of n, n_bins and the device): the same
 *     call on the same input and device returns the same bits.  Counts are integers.
 * 1 <= n < 2^31; no NULL among x, y, z, mass, spec, spec->edges, count_out, sums_out (info_out is optional); geometry 0 or 1;
 * 1 <= n_bins <= 512; the n_bins + 1 edges finite, edges[0] >= 0, strictly ascending; center finite; with velocities v_cen finite;
 * the rows of frame orthonormal to 1e-6 (|row_i . row_j - delta_ij| <= 1e-6); geometry 1: half_height > 0 or +inf; at least one
 * valid particle; anything else returns TSP_EINVAL and writes nothing.  A profile without a member is no error: zeros.  Not
 * provided: periodic wrapping of the displacements.  Device memory is allocated for the call only (about 16 bytes per particle, 28
 * with velocities, and at most 53 KB per workgroup of partial tables, 27 MB in all); a failed allocation returns TSP_ENOMEM and
 * writes nothing.  The cost is one pass over those bytes, less the blocks of 1024 consecutive particles whose bounding box lies at
 * a squared distance (formed as in tsp_sphere_moments) >= E2[n_bins] (geometry 0) or, with a finite half_height,
 * >= (E2[n_bins] + half_height * half_height) * (1 + 1e-5) (geometry 1: the sphere around the cylinder, widened by what the
 * frame's tolerance and rounding allow) from center: those are not read (identical results).  The pass is fast where a wave's 64
 * consecutive particles fall into a few bins (a spatial order of the arrays) and slow, not wrong, where they fall into many. */
typedef struct {
    int32_t geometry;        /* 0: spherical shells, 1: cylindrical annuli about the frame's third axis */
    int32_t n_bins;          /* 1 .. 512 */
    const double *edges;     /* n_bins + 1 radii, finite, edges[0] >= 0, strictly ascending */
    double center[3];
    double v_cen[3];         /* subtracted from the velocities; ignored without velocities */
    double frame[9];         /* row-major rotation: d' = frame * d, u' = frame * u (what topsy_amd.orientation returns) */
    double half_height;      /* geometry 1: members have |z'| <= half_height; > 0 or +inf.  geometry 0: ignored */
} tsp_profile_spec;
typedef struct {
    int64_t n_valid, n_inner, n_binned;        /* valid particles; those inside edges[0]; those in a bin */
    double  mass_inner;                        /* sum m inside edges[0] */
} tsp_profile_info;
int tsp_radial_profile(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, const float *mass,
                       const float *vx, const float *vy, const float *vz,      /* all three or none (NULL) */
                       const tsp_profile_spec *spec, int64_t *count_out /* n_bins */, double *sums_out /* n_bins * 11 */,
                       tsp_profile_info *info_out);

/* Weighted 2-D histograms: the phase diagram -- the mass in each cell of a (rho, T) plane, or any quantity against any other weighted
 * by a third (pynbody's plot.rho_T / plot.generic.hist2d).  Host arrays in, in the caller's order, as the other per-call analyses;
 * the call uses the context's device and stream only, is allowed in every state of the context, and leaves the resident particles,
 * the image, the accumulator and tsp_stats as they are.
 *
 * tsp_histogram_2d: n particles with the float32 coordinates x, y, the float32 weights w (NULL: every weight 1) and the float32
 * values v (NULL: no value), binned into nx columns and ny rows.
 *   - Valid.  A particle is valid iff x[i], y[i], w[i] (when given) and v[i] (when given) are all finite.  Any finite weight is
 *     allowed, negative and zero included.  n_valid = the number of valid particles.
 *   - Bin.  The float32 coordinate is widened to float64 (exact) and compared with the edges as passed: column i holds
 *     edges_x[i] <= x < edges_x[i + 1], row j holds edges_y[j] <= y < edges_y[j + 1].  A valid particle with both in range is a
 *     member of cell c = j * nx + i.  A value equal to an inner edge goes to the upper cell; a value equal to the LAST edge is
 *     outside -- the rule of tsp_radial_profile, not the closed last bin of numpy.histogram2d (move the last edge up by one ulp to
 *     bin a maximum).  The device evaluates no logarithm: logarithmic bins are logarithmic edges built by the caller, and the
 *     binning is exact against a float64 model.  n_binned = the number of members of all cells.
 *   - Outputs.  With S = nx * ny: count_out[c] = the members of cell c; sums_out[0 * S + c] = sum w; with v,
 *     sums_out[1 * S + c] = sum w * v and sums_out[2 * S + c] = sum (w * v) * v.  The terms are formed in float64 from the widened
 *     float32s; every sum starts at +0.0; a cell without members is count 0 and +0.0 whatever an earlier call left on the device.
 *     bin_out (n int32, or NULL): bin_out[p] = the cell of particle p, or -1 if it is invalid or outside.  info_out is optional.
 *     A histogram without members is zeros, not an error.
 *   - Determinism.  No floating-point atomics.  The particles are sorted by cell (a stable radix sort over the
 *     ceil(log2(S + 1)) bits of a cell index; particles in no cell sort last) and every cell's terms are added by a tree whose shape
 *     depends on n alone: a segmented scan over each wave's 64 sorted entries, then over the two boundary runs of each of a
 *     workgroup's four waves in wave order, then the same over the two boundary records of every block of TSP_HIST2D_BLOCK entries,
 *     level by level.  The order of a sum is therefore fixed but depends on where the cell's run lies in the sorted list: the same
 *     call on the same input and device returns the same bits; a permuted input may differ in the last bits of a sum.  Counts are
 *     integers.  For a cell of m members each sum lies within m * 2^-52 * sum |term| of the exact sum.
 *   - Cost.  A cell that holds a third of the particles is reduced by n / 3 / TSP_HIST2D_BLOCK workgroups in parallel: no
 *     workgroup walks a cell's members.
 *   - TSP_EINVAL: n < 1 or n >= 2^31; NULL among x, y, spec, spec->edges_x, spec->edges_y, count_out, sums_out; nx or ny outside
 *     [1, 1024]; an edge that is not finite, or edges that are not strictly ascending.  A refused call writes nothing.
 *   - Device memory is per call, through the two allocations of tsp_sph_sum (first the caller's arrays, 8 to 16 bytes per particle;
 *     then the table, the keys and indices in and out of the sort, 16 bytes per particle, the records of the reduction, about 0.25
 *     byte per particle, and the sort's temporary storage); a failed allocation returns TSP_ENOMEM and writes nothing.
 * tsp_histogram_2d_layout: the host arithmetic of the call without a device or a context -- for (n, nx, ny, has_w, has_v,
 * want_bins), out[TSP_HIST2D_LAYOUT_VALUES] receives: the bits of a key, TSP_HIST2D_BLOCK, the levels of the reduction, the
 * blocks of level 0, the records of the two record buffers; then (byte offset, bytes used) of x, y, w, v inside the first
 * allocation and its size; then (byte offset, bytes used) inside the second of the counts, the sums, the edges, the two counters,
 * the keys, the sorted keys, the indices, the sorted indices, the record buffers A and B, the sort's temporary storage (counted as
 * 0 bytes here) and its size; last the bytes copied into bin_out (the key array itself: all ones is -1; 0 without want_bins).
 * Every offset is a multiple of 256.  TSP_EINVAL for n outside [1, 2^31), nx or ny outside [1, 1024] or a NULL out. */
#define TSP_HIST2D_MAX_BINS 1024                    /* per axis */
#define TSP_HIST2D_BLOCK 256                        /* sorted entries per workgroup of the reduction */
#define TSP_HIST2D_LAYOUT_VALUES 39
typedef struct {
    int32_t nx, ny;            /* 1 .. 1024 each */
    const double *edges_x;     /* nx + 1, finite, strictly ascending */
    const double *edges_y;     /* ny + 1, finite, strictly ascending */
} tsp_hist2d_spec;
typedef struct { int64_t n_valid, n_binned; } tsp_hist2d_info;
int tsp_histogram_2d(tsp_context *ctx, int64_t n, const float *x, const float *y,
                     const float *w /* NULL: every weight 1 */, const float *v /* NULL: no value */,
                     const tsp_hist2d_spec *spec,
                     int64_t *count_out /* ny * nx */, double *sums_out /* (v ? 3 : 1) * ny * nx */,
                     int32_t *bin_out /* n, or NULL */, tsp_hist2d_info *info_out /* optional */);
int tsp_histogram_2d_layout(int64_t n, int nx, int ny, int has_w, int has_v, int want_bins,
                            int64_t *out /* TSP_HIST2D_LAYOUT_VALUES */);

/* Softened direct-sum gravity: the potential and the acceleration at every target from every source -- pynbody's gravity.calc
 * direct sum, from which a snapshot's 'phi' and a disc profile's midplane rotation curve and potential are taken.  Host arrays in,
 * caller's order; uses ctx's device and stream only, in every context state: resident particles, image, accumulator and tsp_stats
 * unchanged.  G = 1 (the caller multiplies).
 *   - Sums.  With d = t_i - s_j per component and r2 = d . d + eps_j^2 (Plummer softening with the source's length):
 *         pot_i = - sum_j m_j r2^(-1/2),        acc_i = - sum_j m_j r2^(-3/2) d.
 *     eps = NULL: every source has the softening length eps_all (the same bits as an array holding that value).
 *   - Sources.  Source j takes part iff sx[j], sy[j], sz[j], mass[j] and its softening length are finite; n_valid_sources counts
 *     those.  A source with mass 0 takes part (and adds zeros).
 *   - Pairs.  A pair with r2 == 0 (distance 0 and eps_j = 0) contributes nothing; so does one with r2 below 2^-126, and one whose
 *     r2 overflows float32.  Coincident distinct particles with eps > 0 are ordinary pairs.
 *   - Targets.  tx, ty, tz all NULL: the targets are the sources (n_tgt must equal n_src), and the pair i == j by index contributes
 *     nothing.  A target with a non-finite coordinate gets NaN in every output and is not counted in n_valid_targets; with NULL
 *     targets that is decided by the coordinates alone (a source left out for its mass is still a target).
 *   - Outputs.  pot_out[i], acc_out[3 i + (0, 1, 2)] = (ax, ay, az); either may be NULL, not both: what both forms of the call
 *     return is equal bit for bit.
 *   - Arithmetic.  Pair terms in float32: d by one subtraction each, eps_j^2 by one multiplication,
 *     r2 = fma(dx, dx, fma(dy, dy, fma(dz, dz, eps_j^2))), inv = the hardware reciprocal square root of r2 (1 ulp), the potential term
 *     p = m_j * inv, the acceleration terms fma(w, d, .) with w = p * (inv * inv).  Per target, runs of 16 consecutive sources
 *     (indices 16 k .. 16 k + 15) are added in float32 in index order, the runs in float64 in index order within a contiguous
 *     range of source tiles, and the ranges in index order.
 *   - Error bound.  Against the float64 evaluation of the formulae on the float32 inputs, per output component,
 *         |got - want| <= TSP_GRAVITY_ERROR_K * 2^-24 * sum_j |term_ij|,      TSP_GRAVITY_ERROR_K = 64.
 *     The account, u = 2^-24: each d within u; eps^2 within u; r2 within 2u + 3u; inv within 2.5u + 2u (1 ulp <= 2u): 5u; p within
 *     6u; inv * inv within 11u, w within 18u, an acceleration term within 19u; a float32 run of 16 terms adds 15u; the float64
 *     additions add less than n_src * 2^-53 <= 4u.  25u for the potential, 38u for an acceleration component.  It holds for pairs
 *     with 2^-80 <= r2 <= 2^80 whose m_j r2^(-3/2) is 0 or lies in float32's normal range [2^-126, 2^127], and for coordinates
 *     whose differences do not overflow float32; outside that range the float32 terms may flush, overflow or (a difference that is
 *     infinite) turn a target's acceleration into NaN.
 *   - Determinism.  No floating-point atomics; the order of every sum is a function of n_src, n_tgt and the device (the sources
 *     are cut into tiles of TSP_GRAVITY_SOURCE_TILE, the targets into launches of 2^18 and workgroups of up to
 *     TSP_GRAVITY_TARGETS_PER_WORKGROUP, the tiles into ranges by the launch's target count and the device's CU count): the same
 *     call returns the same bits, and a target's values do not depend on the other targets of a launch with the same number of
 *     target workgroups.
 * 1 <= n_src, n_tgt < 2^31; no NULL among sx, sy, sz, mass; eps_all finite and >= 0 when eps is NULL (ignored otherwise); the
 * targets all three NULL (then n_tgt == n_src) or none NULL; at least one of pot_out and acc_out; at least one valid source;
 * anything else returns TSP_EINVAL and writes nothing.  info_out is optional.  Not provided: periodic images (no Ewald sum), and
 * a tree -- the cost is n_src * n_tgt pairs, whatever the geometry (measured rates: DESIGN.md).  Device memory is allocated for the
 * call only (20 bytes per source, 44 per target, at most 32 MB of partial sums on 256 CUs); a failed allocation returns TSP_ENOMEM
 * and writes nothing. */
#define TSP_GRAVITY_SOURCE_TILE 512                 /* sources per tile of the pair kernel */
#define TSP_GRAVITY_TARGETS_PER_WORKGROUP 1024      /* targets of a workgroup at most (fewer than 513 targets: 256 or 512) */
#define TSP_GRAVITY_ERROR_K 64
typedef struct { int64_t n_valid_sources, n_valid_targets; } tsp_gravity_info;
int tsp_gravity_direct(tsp_context *ctx,
        int64_t n_src, const float *sx, const float *sy, const float *sz, const float *mass,
        const float *eps /* n_src softening lengths, or NULL: eps_all for every source */, float eps_all,
        int64_t n_tgt, const float *tx, const float *ty, const float *tz /* all three NULL: the targets are the sources */,
        double *pot_out /* n_tgt, or NULL */, double *acc_out /* n_tgt * 3, (ax, ay, az) per target, or NULL */,
        tsp_gravity_info *info_out /* optional */);

/* Barnes-Hut tree gravity: the sums of tsp_gravity_direct in O(n log n), by a tree that is implicit in the Morton order of the
 * sources (topsy_amd/csrc/tsp_gravity_tree.hip).  Host arrays in, caller's order; uses ctx's device and stream only, in every
 * context state: resident particles, image, accumulator and tsp_stats unchanged.  G = 1.  What is said of tsp_gravity_direct holds
 * here too -- the sums, the softening with the source's length, which sources, pairs and targets count, the self pair (left out by
 * the caller's index when the targets are the sources), the outputs and their order, "nothing is written on failure" -- except:
 *   - mass[j] < 0 returns TSP_EINVAL (a centre of mass needs masses >= 0; 0 is fine), and so does theta outside [0, 1] or not
 *     finite.
 *   - Tree.  The sources with finite coordinates are sorted along the 63-bit Morton curve of their bounding box (a source whose
 *     mass or softening length is not finite stays in the order with mass 0 and is not counted valid).  A leaf is
 *     TSP_GRAVITY_TREE_LEAF consecutive sorted particles, a node of level l + 1 is TSP_GRAVITY_TREE_FANOUT consecutive nodes of
 *     level l; the last node of a level may be partial; the top level has one node.  A node carries its mass M, its centre of
 *     mass c, the second moments Q_ab = sum m (x - c)_a (x - c)_b, the mass-weighted mean e2 of eps^2, and a radius b that is no
 *     smaller than the distance from c to the farthest corner of the members' bounding box.  Sums in float64, stored in float32.
 *   - Walk.  The targets are taken in groups of 64 (targets = sources: 64 consecutive particles of the Morton order; separate
 *     targets: 64 consecutive targets in the caller's order -- pass neighbours next to each other, the group's box decides what is
 *     opened).  With dmin the distance from the group's bounding box to c, a node with M > 0 is accepted iff
 *         dmin * theta > b      and      dmin^2 + e2_min >= 8 (e2_max - e2_min)
 *     (e2_min, e2_max over the members with mass; the second rule matters only where the softening varies inside the node, and
 *     keeps the mean e2 from being used at distances where the spread of eps^2 would show).  An accepted node adds, with
 *     d = t - c, r2 = d . d + e2, u = d r2^(-1/2), s = u . Q u, T = tr Q:
 *         pot -= r2^(-1/2) (M + (1.5 s - 0.5 T) / r2),
 *         acc -= ((M + (7.5 s - 1.5 T) / r2) u - 3 Q u / r2) / r2;
 *     a node that is not accepted is opened: its children are tested, and a leaf's particles are summed as tsp_gravity_direct
 *     sums pairs.  A node without mass adds nothing.  theta = 0 accepts nothing: the call is the direct sum with the sources in
 *     Morton order.  A node that holds a target of the group is never accepted (b >= |c - t| >= dmin), so the self pair only
 *     arises in a leaf.  A target's value may depend on which other targets share its group (they decide what is opened), not
 *     on anything else: the same call returns the same bits (no floating-point atomics).
 *   - Error.  Rounding, against the float64 evaluation of the same terms: TSP_GRAVITY_TREE_ERROR_K * 2^-24 * sum |term| per
 *     output component; with theta = 0 that is a bound against the direct sum itself.  A node whose mass is one particle's
 *     (every other member massless) gives that particle's pair term within 32 * 2^-24 relative.  The truncation (what the
 *     octupole and higher moments of the accepted nodes would add) is not bounded by the library; DESIGN.md has measured values
 *     (theta = 0.5: 99 % of the accelerations within 1e-2 relative in the scenes measured there).
 *   - info_out (optional): n_nodes, n_levels (the leaves' level included), pairs_direct = target-particle terms evaluated,
 *     pairs_node = target-node terms evaluated (integer counts over the valid targets).
 * 1 <= n_src, n_tgt < 2^31; arguments otherwise as tsp_gravity_direct; at least one source must be valid.  Device memory for the
 * call only (about 75 bytes per source, the neighbour index included, beside the sort's temporary storage; 44 bytes per separate
 * target, 64 per particle when the targets are the sources), through the allocation sites of the neighbour index and the gather
 * sums; a failed allocation returns TSP_ENOMEM and writes nothing. */
#define TSP_GRAVITY_TREE_LEAF 32                    /* sorted particles per leaf */
#define TSP_GRAVITY_TREE_FANOUT 8                   /* nodes of a level per node of the next */
#define TSP_GRAVITY_TREE_ERROR_K 64
typedef struct { int64_t n_valid_sources, n_valid_targets, n_nodes, n_levels, pairs_direct, pairs_node; } tsp_gravity_tree_info;
int tsp_gravity_tree(tsp_context *ctx,
        int64_t n_src, const float *sx, const float *sy, const float *sz, const float *mass,
        const float *eps /* n_src softening lengths, or NULL: eps_all for every source */, float eps_all,
        int64_t n_tgt, const float *tx, const float *ty, const float *tz /* all three NULL: the targets are the sources */,
        float theta, double *pot_out /* n_tgt, or NULL */, double *acc_out /* n_tgt * 3, or NULL */,
        tsp_gravity_tree_info *info_out /* optional */);

/* The haloes of a catalogue in one call: the self-potential of every halo (tsp_group_potential) and per-halo reductions
 * (tsp_halo_properties).  Host arrays in, caller's order; both use ctx's device and stream only, in every context state: resident
 * particles, image, accumulator and tsp_stats unchanged.  G = 1.  Shared by both:
 *   - Labels.  group[i] in 1 .. n_groups: particle i is a member of that halo; group[i] <= 0: of none (what tsp_fof_groups writes).
 *     A label above n_groups returns TSP_EINVAL.  A member is valid iff the fields named below are finite; an invalid member
 *     takes no part in its halo.
 *   - Order.  (label, index) pairs are sorted by label with a stable radix sort, everything that is no valid member under the
 *     key ~0: a halo's members are then contiguous and in the caller's index order.
 *   - Anchor and offsets.  The anchor a of a halo is the position of its valid member with the smallest index.  Per axis a member
 *     has the offset d = (double)x - (double)a and, with period > 0, d -= period * rint(d / period): float64, nothing fused, so
 *     that a numpy model forms the same bits.  That is the nearest image as long as every member lies within period / 2 of the
 *     anchor per axis, which is not checked: max_extent of the info struct is the largest |d| on any axis of any halo.
 *   - Determinism.  No floating-point atomics; the results are a function of the inputs alone (not of the device's CU count,
 *     not of timing): the same call returns the same bits.
 * 1 <= n < 2^31, 1 <= n_groups < 2^31; period 0 (open) or finite and > 0; no NULL among the required arrays; anything else
 * returns TSP_EINVAL and writes nothing.  Device memory is allocated for the call only, through the two allocation sites of the
 * gather sums (the radix sort's temporary storage included); a failed allocation returns TSP_ENOMEM and writes nothing.
 *
 * tsp_group_potential: phi_out[i] = - sum over the valid members j != i of i's halo of m_j / sqrt(|e_i - e_j|^2 + eps_j^2).
 *   - e = (float)d: the anchor-relative offset rounded once to float32, so that a halo far from the origin, or one that straddles
 *     a face of a periodic box, keeps its digits.
 *   - A valid member has finite x, y, z, mass and softening length (eps[i], or eps_all for every particle when eps is NULL).
 *     Non-members and invalid members get NaN.
 *   - Pair arithmetic, pairs that count (the own pair and r2 < 2^-126 contribute nothing) and the error bound are those of
 *     tsp_gravity_direct: |got - want| <= TSP_GRAVITY_ERROR_K * 2^-24 * sum |term| against the float64 evaluation on the float32
 *     e, m, eps.  The float32 runs of 16 are runs of 16 consecutive positions of the sorted order, aligned to that order (not to
 *     the halo's first member); a workgroup owns TSP_HALO_TARGET_BLOCK consecutive sorted targets and sums tiles of
 *     TSP_HALO_SOURCE_TILE sorted sources; a source range of more than 2 tiles is cut into up to 16 parts of at least 2 tiles, added in order.
 *   - max_members > 0: a halo with more valid members is skipped -- its members get NaN -- and counted in n_skipped_groups /
 *     n_skipped_members (the caller sends it to tsp_gravity_tree).  0: no limit.  Negative: TSP_EINVAL.
 *   - info_out (optional): n_members (valid members, those of skipped haloes included), n_groups_nonempty, pairs (ordered pairs
 *     i != j that count, skipped haloes left out), pair_slots (pairs the kernel evaluated, masked ones included), the two skip
 *     counts, max_extent.
 *
 * tsp_halo_properties: everything in float64.  A valid member has finite x, y, z, a finite mass > 0 and, when velocities are
 * given (all three or none), finite velocities.  Per halo, with M = sum m:
 *   - pass 1: count; M; com_off = sum m d / M; com = a + com_off, wrapped into [0, period) when periodic; v_com = sum m v / M.
 *   - pass 2, with e = d - com_off and w = v - v_com (w = 0 without velocities): S = sum m e_a e_b (xx, xy, xz, yy, yz, zz);
 *     L = sum m e x w; e_kin = 0.5 sum m |w|^2; sigma2 = 2 e_kin / (3 M); r_max = max |e|.  With phi (n float64, the caller's
 *     potential, G included): e_pot = 0.5 sum m phi; i_pot the member with the smallest phi (ties: the smaller index), pot_pos its
 *     position; n_bound, m_bound over the members with 0.5 |w|^2 + phi < 0.  A valid member with a non-finite phi gives its halo
 *     e_pot = NaN, i_pot = -1, n_bound = -1, m_bound = NaN, pot_pos = NaN.
 *   - pass 3: the members ordered by the key (float)|e|, ties by index; cum_k the running sum of m in that order; r_half = |e| of
 *     the first member with cum_k >= M / 2 (i_half its index); v2_max = the largest cum_k / |e_k| over the ranks k >= 10 (1-based)
 *     with |e_k| > 0, r_vmax that member's |e| (i_vmax its index; ties: the smaller rank).  Fewer than 10 members: v2_max, r_vmax
 *     and i_vmax are NaN.
 *   - A label without valid members: count = 0, mass = 0, every other column NaN, n_bound = -1, i_pot = -1.  Without velocities
 *     v_com, L, e_kin, sigma2 are NaN; without phi e_pot, m_bound, pot_pos are NaN, n_bound = -1 and i_pot = -1.
 *   - Sums.  Each sum is formed over slices of 256 consecutive sorted members (one partial per halo and slice, added in order),
 *     and a halo's partials are added in order in 64 chunks of consecutive partials, then the chunks in order: the association is
 *     a function of where the halo lies in the sorted order.  Against the exact sum each is within (n_h + 16) * 2^-53 * sum |term|.
 * Outputs: count_out, n_bound_out, i_pot_out int64[n_groups]; props_out[n_groups * TSP_HALO_NPROPS], row g = label g + 1, columns
 * TSP_HALO_*; info_out (optional): n_members, max_extent. */
#define TSP_HALO_SOURCE_TILE 512                    /* sorted sources per tile of the halo pair kernel */
#define TSP_HALO_TARGET_BLOCK 1024                  /* sorted targets of a workgroup */
#define TSP_HALO_MASS 0
#define TSP_HALO_COM 1                              /* 3 columns */
#define TSP_HALO_VCOM 4                             /* 3 */
#define TSP_HALO_S 7                                /* 6: xx, xy, xz, yy, yz, zz */
#define TSP_HALO_L 13                               /* 3 */
#define TSP_HALO_EKIN 16
#define TSP_HALO_SIGMA2 17
#define TSP_HALO_RMAX 18
#define TSP_HALO_RHALF 19
#define TSP_HALO_V2MAX 20
#define TSP_HALO_RVMAX 21
#define TSP_HALO_EPOT 22
#define TSP_HALO_MBOUND 23
#define TSP_HALO_POTPOS 24                          /* 3 */
#define TSP_HALO_IHALF 27                           /* the caller's index of the r_half member, as a double */
#define TSP_HALO_IVMAX 28                           /* ... of the r_vmax member */
#define TSP_HALO_NPROPS 29
typedef struct { int64_t n_members, n_groups_nonempty, pairs, pair_slots, n_skipped_groups, n_skipped_members; double max_extent; }
        tsp_group_potential_info;
typedef struct { int64_t n_members; double max_extent; } tsp_halo_info;
int tsp_group_potential(tsp_context *ctx,
        int64_t n, const float *x, const float *y, const float *z, const float *mass,
        const float *eps /* n softening lengths, or NULL: eps_all for every particle */, float eps_all,
        const int32_t *group, int64_t n_groups, double period, int64_t max_members /* 0: no limit */,
        double *phi_out /* n */, tsp_group_potential_info *info_out /* optional */);
int tsp_halo_properties(tsp_context *ctx,
        int64_t n, const float *x, const float *y, const float *z, const float *mass,
        const float *vx, const float *vy, const float *vz /* all three or none (NULL) */, const double *phi /* n, or NULL */,
        const int32_t *group, int64_t n_groups, double period,
        int64_t *count_out, int64_t *n_bound_out, int64_t *i_pot_out /* n_groups each */,
        double *props_out /* n_groups * TSP_HALO_NPROPS */, tsp_halo_info *info_out /* optional */);

/* Kinematic maps: the mass-weighted mean line-of-sight velocity and its dispersion per pixel, from resident velocities (what
 * pynbody's image(qty="vz", av_z=True) draws after analysis.angmom.sideon; the reference has no such mode).  The rgb kernels
 * accumulate three independent weighted sums and an exact fragment count; fed the "colours" (m, m u, m u^2) of a particle, u its
 * velocity along the line of sight, one splat pass leaves per pixel
 *     S = sum k m / h^2,   A = sum k m u / h^2,   B = sum k m u^2 / h^2,   n = the fragment count
 * (k the kernel value of the fragment), with the arithmetic, the tolerances and the count of TSP_MODE_RGB.
 *   - Velocities.  tsp_upload_velocities: float32, caller's order (permuted by the library after tsp_reorder_spatial, as
 *     tsp_upload_quantity); all three arrays, or all three NULL, which frees them; anything else TSP_EINVAL.  TSP_ESTATE before the
 *     particles are uploaded.  tsp_upload_particles and tsp_generate_synthetic drop them; tsp_download_particles does not return them.
 *   - Line of sight.  tsp_set_line_of_sight: axis finite with |sqrt(axis . axis) - 1| <= 1e-5 (formed in float64), v_ref finite;
 *     otherwise TSP_EINVAL and the line of sight set before stays.  For a camera with rotation matrix Q (clip = Q (x + offset) /
 *     scale) the axis is Q's third row.  -0 components are taken as +0.
 *   - Weights.  Per particle, once per change of the line of sight or of the particles (not per block, not for a change of pan or
 *     zoom), in float32 with these operations in this order, none fused:
 *         u = ((axis[0] * (vx - v_ref[0]) + axis[1] * (vy - v_ref[1])) + axis[2] * (vz - v_ref[2]))
 *         r = m;  g = m * u;  b = g * u;      m or u not finite: r = g = b = +0 (the particle's fragments are still counted)
 *         hh = h * h;  wr = r / hh;  wg = g / hh;  wb = b / hh
 *     A pure stream, 20 bytes read and 12 written per particle.  The weights live where TSP_MODE_RGB keeps its own (a render in
 *     either mode after the other recomputes them from the untouched r, g, b or m, velocities: 12 bytes per particle for both).
 *   - tsp_render(mode = TSP_MODE_KINEMATIC) needs a 4-channel context (TSP_EINVAL), flags = TSP_PIPE_DEFAULT (TSP_EINVAL: the
 *     generic kernel has no kinematic form), and mass, velocities and a line of sight (TSP_ESTATE).  A clear = 0 block continues an
 *     image only in the 4-channel mode that started it, and a kinematic one only along the same axis and v_ref (compared bit for
 *     bit): otherwise TSP_ESTATE.  As every refused render, it leaves image, accumulator and tsp_stats as they were.
 *   - tsp_velocity_moments: valid while the presentation image is a kinematic one -- the last successful tsp_render was kinematic;
 *     tsp_write_image, tsp_set_reduced_image, tsp_comm_reduce_image and tsp_tile_periodic keep that, tsp_render_surface and a render
 *     in another mode end it -- and has 4 active channels; otherwise TSP_ESTATE.  It reads the float32 presentation image (after a
 *     cross-rank reduce: the sum), and writes maps_out[R][R][4] = (S, (float)mean, (float)sigma, n) with, in float64, every
 *     operation correctly rounded and none fused:
 *         if S > 0 and S, A, B are finite:  mean = A / S;  var = B / S - mean * mean;  var < 0: var = 0;  sigma = sqrt(var)
 *         otherwise mean = sigma = NaN (0x7fc00000).
 *     B / S - mean^2 cancels: it loses about 6e-8 * (mean / sigma)^2 of relative accuracy in sigma^2 (the float32 rounding of the
 *     weights and channels against the size of mean^2).  That is what v_ref is for: subtract the bulk velocity (e.g. v_cen of
 *     tsp_sphere_moments) before the squares are formed, and add it back to mean if wanted.
 *   - tsp_colormap_moment: the scalar map of tsp_colormap_scalar, unweighted, of map `which` (1: mean, 2: sigma) -> RGBA8, bit for
 *     bit what that map gives on the image (value, 0).  Same conditions as tsp_velocity_moments; which or the LUT out of range:
 *     TSP_EINVAL.
 *   Neither of the two changes the image, the accumulator or tsp_stats.  Both form the maps in the staging buffer of
 *   tsp_colormap_rgb's float output (allocated on first use: TSP_ENOMEM).
 *   - Canvas-sized frames of the maps, under a colorbar and the other layers: the bases TSP_PRESENT_MOMENT_MEAN and
 *     TSP_PRESENT_MOMENT_SIGMA of tsp_present / tsp_present_yuv420 ("Frame composition" below).
 *   - tsp_moment_sort: the order statistics of a moment map, for its colour range -- tsp_content_sort's sort (below) of other
 *     values.  For every pixel of the kinematic presentation image the float32 moment `which` (1: mean, 2: sigma) is formed by the
 *     rule of tsp_velocity_moments directly from the image (no staging buffer), with absolute != 0 its fabsf is taken, and the finite
 *     values are sorted ascending into the buffers of tsp_content_sort (allocated on first use or growth: TSP_ENOMEM).  n_finite
 *     receives their number; tsp_content_values then returns the values at ranks in [0, n_finite) exactly as after a content sort,
 *     and tsp_content_neg_inf reports 0 (a moment is never -inf).  Same conditions as tsp_velocity_moments (TSP_ESTATE); which not
 *     1 or 2, or a NULL argument: TSP_EINVAL.  The image, the accumulator and tsp_stats are unchanged.
 * Not provided: velocities on a tsp_group or sharded over several contexts by the library (a caller that shards uploads each
 * shard's velocities itself; the reduced image is a valid input of tsp_velocity_moments and of the frames). */
int tsp_upload_velocities(tsp_context *ctx, const float *vx, const float *vy, const float *vz);
int tsp_set_line_of_sight(tsp_context *ctx, const float axis[3], const float v_ref[3]);
int tsp_velocity_moments(tsp_context *ctx, float *maps_out /* R * R * 4 */);
int tsp_colormap_moment(tsp_context *ctx, int which /* 1 mean, 2 sigma */, const float *lut_rgba, int n_lut, float vmin, float vmax,
                        int log_scale, uint8_t *out_rgba8);
int tsp_moment_sort(tsp_context *ctx, int which /* 1 mean, 2 sigma */, int absolute, int64_t *n_finite);

/* Spectral cubes: the whole line-of-sight velocity distribution per pixel, a position-position-velocity cube (channel maps, the
 * integrated line profile, position-velocity diagrams), where the kinematic maps above keep two numbers of it.  One call draws
 * every resident particle (no index ranges) at the camera M, scale_factor of tsp_render:
 *     cube_out[c][j][i] = sum over particles of (double)k * (double)w0 * g_c          float32 [n_channels][R][R], host
 *   - Geometry: the canonical rule of tsp_render -- projection, the draw test (0 <= cz <= 1; P, pcx, pcy finite; P > 0), coverage,
 *     mip level, nearest or bilinear sampling -- gives the float32 kernel value k of every covered pixel; w0 = m / (h * h) in float32.
 *   - Velocity: u, the float32 u of the kinematic weights above (same operations, same order, none fused), along the axis and about
 *     the v_ref of tsp_set_line_of_sight.
 *   - Channels: n_channels of them, with the edges e_k = v_min + k * dv formed in float64 for k = 0 .. n_channels (dv > 0).
 *   - Line width, per particle, in float64: s = sqrt(sigma_v^2 + sigma_p^2).  sigma_v >= 0 is the call's scalar (an instrumental or
 *     turbulent floor); sigma_p comes from `sigma`, n float32 in the caller's order (permuted by the library after
 *     tsp_reorder_spatial, as tsp_upload_quantity's array), or is 0 for every particle when sigma is NULL.
 *   - Channel response g_c: the Gaussian of width s about u INTEGRATED over the channel (not sampled at its centre: mass is
 *     conserved), in float64 without cancellation in the tails.  With a = (e_c - u) / s and b = (e_{c+1} - u) / s:
 *         a >= 0:     g_c = (erfc(a / sqrt 2) - erfc(b / sqrt 2)) / 2
 *         b <= 0:     g_c = (erfc(-b / sqrt 2) - erfc(-a / sqrt 2)) / 2
 *         otherwise:  g_c = (erf(b / sqrt 2) - erf(a / sqrt 2)) / 2
 *     s == 0: g_c = 1 for the one channel with e_c <= u < e_{c+1} (a u on an edge falls in the upper channel), 0 elsewhere; a u
 *     outside the band contributes nothing.  Channels that lie wholly more than 5 s from u are skipped: at most erfc(5 / sqrt 2) =
 *     5.8e-7 of a particle's mass.
 *   - Dead particles: m, u or sigma_p not finite, or sigma_p < 0: the particle contributes nothing.
 *   - Order: every cell is summed in float64 in ascending resident particle index, and rounded to float32 once per slice of
 *     particles (the float32 cube takes the slices' sums one after the other).  No floating-point atomics: two calls with the same
 *     arguments on the same context give the same bits.
 *   - Slices: the particles go through in slices of consecutive resident indices.  A slice holds
 *     min(2^27 / n_bins, 2^22, n) particles, n_bins = ceil(R / 16)^2 * ceil(n_channels / 32) -- a function of (n, R, n_channels)
 *     alone -- so that its (image tile, channel block) lists never exceed 2^27 entries whatever the data: 2 GiB of lists and
 *     192 MiB of records at most, next to the device copy of the cube.  Option "cube_slice_particles" > 0 lowers the slice further
 *     (a test aid: the many-slice path at small n); 0 restores the default.
 *   - The call is a read-only per-call entry point like the gather analyses: the image, the accumulator, tsp_stats and the
 *     context's state are untouched.  It is allowed wherever tsp_velocity_moments' inputs exist: particles with mass, velocities, a
 *     line of sight and the kernel mips (TSP_ESTATE otherwise).  Device memory is per call, through the two allocations of
 *     tsp_sph_sum (TSP_ENOMEM: nothing written).
 *   - TSP_EINVAL: M or cube_out NULL; v_min, dv or sigma_v not finite; dv <= 0; sigma_v < 0; n_channels outside [1, 4096];
 *     n_channels * R * R > 2^31.  A refused call leaves cube_out as it was.
 * tsp_spectral_cube_layout: the host arithmetic of the call without a device or a context -- for n particles, a resolution, a channel
 * count, the option's value (0: default) and has_sigma, out[TSP_CUBE_LAYOUT_VALUES] receives: tiles per image side, channel
 * blocks, bins, the bits of a bin index, particles per slice, slices, list entries per slice; then the byte offsets inside the
 * first allocation of sigma, the geometry records, the line records and its size; then inside the second of the cube, the pair
 * counts, the pair offsets, the keys, the sorted keys, the indices, the sorted indices, the bins' first entries, the bins' end
 * entries, the temporary storage of the scan and the sort (counted as 0 bytes here) and its size.  TSP_EINVAL as above, and for n
 * outside [0, 2^31) or a negative option. */
#define TSP_CUBE_TILE 16                            /* pixels per side of an image tile */
#define TSP_CUBE_CHANNEL_BLOCK 32                   /* channels per block */
#define TSP_CUBE_LAYOUT_VALUES 22
int tsp_spectral_cube(tsp_context *ctx, const float *M, float scale_factor, double v_min, double dv, int n_channels,
                      float sigma_v, const float *sigma /* n, caller's order, or NULL */, float *cube_out /* n_channels * R * R */);
int tsp_spectral_cube_layout(int64_t n, int resolution, int n_channels, int64_t slice_option, int has_sigma,
                             int64_t *out /* TSP_CUBE_LAYOUT_VALUES */);

/* Perspective view.  Every render call is orthographic.  To first order across each footprint, a perspective view of SPH particles
 * is the orthographic view of a transformed snapshot: a particle at distance d along the optical axis is seen as if it lay on the
 * reference plane at distance D -- position scaled by s = D / d, smoothing length h s, mass m s^2, so that the vertex weight
 * m' / h'^2 and with it the column density along the ray through the particle's centre are unchanged.  The small-angle statement:
 * a footprint is drawn as a disc, not as the conic the sphere projects to.  A pixel's ray that meets the particle's plane z = zv
 * at the distance b' from its centre has the kernel sampled at b' / h; the ray's true impact parameter is
 * b = b' sqrt(1 - sin^2(theta) cos^2(phi)) >= b' cos(theta), theta the ray's angle to the optical axis.  The sample is exact on the
 * ray through the centre and off by at most max|g'| (2 / cos(theta)) (1 - cos(theta)) elsewhere (g the projected kernel): small
 * while the footprint's rays stay near the axis (angular radius 2 h / d << 1 for a particle near it), second order in theta.
 *
 * tsp_project_perspective writes that snapshot of src's particles into dst, which the caller then renders with rotation =
 * identity, offset = 0 and any scale: tsp_render, tsp_render_surface and everything downstream are unchanged.
 *   Preconditions, checked before anything changes (a refused call leaves dst as it found it): src != dst, on one device
 *   (TSP_EINVAL); both hold n > 0 particles with x, y, z, h -- the caller uploaded the same snapshot into dst once, with the same
 *   tsp_reorder_spatial arguments where src was reordered, so that the resident orders agree index for index (TSP_ESTATE for a
 *   missing array, TSP_EINVAL for unequal n); dst holds mass iff src does and r, g, b iff src does (TSP_ESTATE); distance finite
 *   and > 0, near finite with 0 < near < distance, rot and offset finite (TSP_EINVAL).
 *   Per particle i in resident order, float32, in this order of operations:
 *     tx = x + offset[0]   ty = y + offset[1]   tz = z + offset[2]
 *     xv = (rot[0]*tx + rot[1]*ty) + rot[2]*tz     (yv with rot[3..5], zv with rot[6..8])
 *     d  = distance - zv          (the viewer sits at zv = +distance and looks down -z: greater z is nearer, as in the surface pass)
 *     visible = d >= near         (false for NaN)
 *     s  = distance / d           (IEEE division)
 *     x' = xv*s   y' = yv*s   z' = zv   h' = h*s   m' = m*(s*s)   r' = r*(s*s)   g' = g*(s*s)   b' = b*(s*s)
 *     not visible:  x' = y' = z' = NaN,  h' = 0,  m' = r' = g' = b' = 0     (a particle with NaN coordinates draws nothing)
 *   dst's q is not touched (it does not depend on the camera); src is only read.
 *   The same pass writes dst's vertex weights m' / (h' * h') and the bounds of every 512 transformed particles (chunk culling),
 *   so the next render forms neither.  Afterwards in dst: the rgb weights are re-formed by the next rgb block, the cell grid of
 *   tsp_get_cell_layout is gone (it described world coordinates: TSP_ESTATE), tsp_get_strata_offsets is unchanged, and
 *   tsp_render_undo has nothing to undo.  dst stays an ordinary context: any upload into it works as before.
 *   It allocates only what dst lacks of the weights and the bounds (once; TSP_ENOMEM leaves dst as it was) and runs on dst's
 *   stream after what src's stream holds; it returns when the pass has finished. */
typedef struct tsp_perspective {
    float rot[9];      /* row-major rotation, world -> view */
    float offset[3];   /* added to the position first */
    float distance;    /* D: from the viewer to the reference plane zv = 0 */
    float near;        /* particles with d < near are not drawn */
} tsp_perspective;
int tsp_project_perspective(tsp_context *src, tsp_context *dst, const tsp_perspective *cam);

/* Surface rendering: DepthSPHWithOcclusion + ColorAsSurfaceMap (reference src/topsy/sph.py:448-656, shaders/sph.wgsl:94-122,
 * 149-158, shaders/smooth.wgsl, shaders/surface.wgsl, colormap/surface.py).  Float32 throughout, operations in the order written.
 *
 * tsp_set_sphere_mips: the sphere texture (LocalSphereKernel, normalisation 1): 64^2 + 32^2 + 16^2 + 8^2 texel-centre samples of
 * sqrtf(4 - d^2) for d < 2, else -0.01; same layout and arguments as tsp_set_kernel_mips, stored next to the SPH mips.
 *
 * tsp_density_order_stats: the values at the given ascending ranks of rho = m / ((h * h) * h) over the n resident particles, sorted
 * as numpy sorts float32 (NaN last).  Device memory for the call only (about 12 bytes per particle); resident data, image and
 * accumulator are unchanged.  Needs mass (TSP_EINVAL otherwise) and 0 <= ranks[i] < n.
 *
 * tsp_render_surface: the occlusion pass.  A particle is drawn iff rho > density_cut and it passes the keep rule of tsp_render
 * (0 <= cz <= 1, finite P > 0, pcx, pcy).  Its covered pixels and texel rule are those of tsp_render; k is the sphere-texture
 * sample.  For a covered pixel: depth = cz + zs * k with zs = (h * scale_factor) * 0.5; the fragment is dropped if k < 0; it
 * competes with dc = min(depth, 1) if dc > 0.  Per pixel the fragment with the largest dc wins, on equal dc the lowest resident
 * index.  The float64 accumulator holds 64-bit keys (bits(dc) << 32) | (0xFFFFFFFF - index) while the context is in this state;
 * the presentation image becomes 2-channel (q_winner, depth_winner) with the unclamped depth, or (0, 0) where nothing won, q = 0
 * without an active quantity.  clear = 0 continues the keys of an earlier tsp_render_surface call (any split of the particles
 * into blocks gives the same image bit for bit); after a surface call tsp_render(clear = 0) returns TSP_ESTATE, clear = 1
 * renders as usual.  Needs a context with mass, fewer than 2^32 resident particles and tsp_set_sphere_mips (TSP_EINVAL /
 * TSP_ESTATE).  tsp_get_stats afterwards: n_particles, ms_total; ms_stream = the draw, ms_mid = the resolve. */
typedef struct tsp_surface_params {
    double smoothing_scale;      /* bilateral filter: sig = max(smoothing_scale, 1e-5), ss = (float)(sig * R), rs = (float)(sig * 2) */
    float depth_scale;           /* D = depth * depth_scale */
    float light_direction[3];
    float light_color[3];
    float ambient_color[3];
    float vmin, vmax;            /* material range (weighted_average only) */
    int weighted_average;        /* 0: material 1; 1: colormap LUT of q (log: of canon_log10f(q)) */
    int log_scale;
    const float *lut_rgba;       /* n_lut RGBA float32 entries (weighted_average only) */
    int n_lut;
} tsp_surface_params;

/* tsp_surface_present: the bilateral filter of the 2-channel image (q, depth), then optionally the lit shading.
 *   n = min((int)(ss * 4) + 1, 100), half = n / 2; for dy in [-half, half] (outer), dx in [-half, half] (inner), sample
 *   coordinates clamped to the image: ds = sqrtf((float)(dx*dx + dy*dy)); ws = exp(-(ds*ds) / ((2*ss)*ss));
 *   dd = |d - d_centre|; wr = exp(-(dd*dd) / ((2*rs)*rs)); w = ws*wr; sum += d*w; wsum += w.  Output (q_centre, sum / wsum);
 *   exp is the canonical expf of the colormap.  content_out: R*R*2 floats of it (or NULL).
 *   Shading per pixel of the filtered image F, neighbours clamped at the edges, D = F.depth * depth_scale:
 *   n = normalize(-(D_right - D_left) * 0.5, -(D_down - D_up) * 0.5, 1 / R) (row j+1 is down; length sqrtf((x*x + y*y) + z*z),
 *   each component divided by it); rgb = (light_color * max(n.L, 0) * mat + ambient_color * mat) * (clamp(D, 0, 0.5) * 2),
 *   n.L = (x*Lx + y*Ly) + z*Lz; alpha 1; mat as the scalar colormap's LUT lerp of clamp((v - vmin) / (vmax - vmin)), NaN -> 0.
 *   rgba8_out: R*R*4 bytes, floor(255 * clamp(c) + 0.5) (or NULL).  ms_out: [filter, shading] GPU milliseconds (or NULL).
 * Needs the active image to be 2-channel (TSP_EINVAL otherwise).  The image and accumulator are unchanged. */
int tsp_set_sphere_mips(tsp_context *ctx, const float *lut, int n0, int n_levels);
int tsp_density_order_stats(tsp_context *ctx, const int64_t *ranks, int n_ranks, float *values_out);
int tsp_render_surface(tsp_context *ctx, const float *M, float scale_factor, float density_cut, const int64_t *starts,
                       const int64_t *lens, int n_ranges, int clear, double *gpu_ms_out);
int tsp_surface_present(tsp_context *ctx, const tsp_surface_params *params, float *content_out, uint8_t *rgba8_out,
                        double *ms_out);

/* Frame composition: the W x H frame a user looks at, saves or records -- VisualizerBase.get_presentation_image / _encode_draw
 * (reference src/topsy/visualizer.py:367-384,480-491): the presentation image colormapped onto a canvas of any size, then an
 * ordered list of layers blended on top (colorbar, scale bar and its label, crosshairs, simulation cube, status line).  One call,
 * one kernel: every pixel computes its base colour and applies the layers in order.  Float32 throughout, the operations in
 * the order written, no fused multiply-adds; the rules below are restated in numpy by the tests (tests/present_ref.py).
 *
 * Canvas.  W, H in [1, 16384]; pixel (i, j), column i, row j from the top, has its centre at xc = i + 0.5f, yc = j + 0.5f.
 *
 * Base layer (colormap.wgsl:42-73 and the sampler of colormap/implementation.py:240-325).  The R x R float32 presentation image
 * of the context (what tsp_colormap_* read: periodic tiling and the mass-scale folding included) covers the square of side
 * S = max(W, H) centred on the canvas -- the aspect squash of colormap.wgsl:50-58; texture row 0 is the top (:60-65).  With
 *     k = (float)R / (float)S,  ox = 0.5f * (float)(W - S),  oy = 0.5f * (float)(H - S),
 *     ax = (xc - ox) * k,  ay = (yc - oy) * k,
 * the sample of every raw channel is
 *   - k <= 1 (magnification: mag_filter linear): tx = ax - 0.5f, x0 = floorf(tx), fx = tx - x0, i0 = clamp((int)x0, 0, R-1),
 *     i1 = clamp((int)x0 + 1, 0, R-1) (ty, y0, fy, j0, j1 alike);  lerp(a, b, f) = f == 0 ? a : a * (1 - f) + b * f;
 *     value = lerp(lerp(T[j0][i0], T[j0][i1], fx), lerp(T[j1][i0], T[j1][i1], fx), fy)
 *   - k > 1 (minification: min_filter nearest, no mips): T[clamp((int)floorf(ay), 0, R-1)][clamp((int)floorf(ax), 0, R-1)]
 * (clamp-to-edge).  At W = H = R, k = 1 and tx = i exactly, so the frame is tsp_colormap_*'s image bit for bit.  The raw channels
 * are sampled first and mapped afterwards (weighted maps divide the sampled g by the sampled r) by the maps of tsp_colormap_scalar,
 * tsp_colormap_bivariate (LUT of tsp_colormap_set_lut2d) and tsp_colormap_rgb (4-channel image).  TSP_PRESENT_RGB_HDR is the rgb
 * map on an rgba16float canvas: the unclamped float colour, alpha 1.
 *
 * Moment bases (TSP_PRESENT_MOMENT_MEAN, TSP_PRESENT_MOMENT_SIGMA): the kinematic maps ("Kinematic maps" above) on the canvas.  The
 * four raw channels (S, A, B, n) of the kinematic presentation image are sampled exactly as above (same k, ox, oy; the linear rule
 * with its f == 0 selection and clamp-to-edge for k <= 1, else nearest).  From the sampled S, A, B the moment is formed by the rule
 * of tsp_velocity_moments -- float64, every operation correctly rounded, none fused: S > 0 and S, A, B finite: mean = A / S,
 * var = B / S - mean * mean clamped at 0, sigma = sqrt(var); otherwise NaN -- and rounded to float32.  Sampling the sums and dividing
 * afterwards is the mass-weighted interpolation of the maps, the order in which the weighted scalar map works.  The moment is then
 * mapped by the scalar map, unweighted, on (value, 0) with lut_rgba, n_lut, vmin, vmax and log_scale of the base (weighted,
 * density_vmin, density_vmax and gamma are not read); a NaN takes the colour of vmin, as in tsp_colormap_moment.  At W = H = R
 * without layers the frame is tsp_colormap_moment's image bit for bit.  The image must be a 4-channel kinematic one, the condition
 * of tsp_velocity_moments (TSP_ESTATE otherwise); the LUT has 2..65536 entries (TSP_EINVAL); the canvas is rgba8unorm.
 *
 * Layers, in order; every instance of a textured quad and every segment of a line set is one primitive, drawn in turn.
 *   Textured quad (overlay.wgsl, overlay.py): texture_rgba = th rows (row 0 at the top) of tw RGBA float32 texels; clip_origin
 *   (x0, y0), clip_extent (w, h) > 0, tex_origin (u0, v0), tex_extent (du, dv); n_instances clip offsets (dx, dy) and weights.
 *   Instance k covers, in pixels,
 *       X0 = ((x0 + dx) + 1) * (0.5f * W),      X1 = (((x0 + dx) + w) + 1) * (0.5f * W),
 *       Y0 = (1 - ((y0 + dy) + h)) * (0.5f * H),  Y1 = (1 - (y0 + dy)) * (0.5f * H),
 *   a pixel iff X0 <= xc < X1 and Y0 <= yc < Y1; its colour is the texture sampled with a linear filter (mag and min), clamp-to-
 *   edge, at u = u0 + ((xc - X0) / (X1 - X0)) * du, v = v0 + ((yc - Y0) / (Y1 - Y0)) * dv: the base layer's linear rule with
 *   tx = u * tw - 0.5f, ty = v * th - 0.5f, times the weight (all four channels).
 *   Line set (line.wgsl, line.py:12-35): segments from starts[s] to ends[s] (xyzw each), row-major transform M (clip = M * p;
 *   px = ((M[0] * x + M[1] * y) + M[2] * z) + M[3] * w, py alike with M[4..7]), colour, width_px.  In float32:
 *       a = (px_s * W, py_s * H), b = (px_e * W, py_e * H), (dx, dy) = b - a, len = sqrtf(dx * dx + dy * dy),
 *       n = (-(dy / len), dx / len), o = ((n.x * width_px) * 0.5f, (n.y * width_px) * 0.5f),
 *       corners a - o, a + o, b + o, b - o, each divided by (W, H) (back to clip) and taken to pixels:
 *       X = (cx + 1) * (0.5f * W), Y = (1 - cy) * (0.5f * H).
 *   Coverage: twice the signed area A = sum over the edges P -> Q of (P.x * Q.y - Q.x * P.y), in corner order from 0; when A < 0
 *   the order is reversed, when A is 0 or not a number the segment covers nothing.  Per edge ex = Q.x - P.x, ey = Q.y - P.y,
 *   E = ex * (yc - P.y) - ey * (xc - P.x); a pixel is covered iff every edge has E > 0, or E == 0 on an edge with ey < 0 or
 *   (ey == 0 and ex > 0).  (This is the top-left rule: the left and top edges are closed, right and bottom open, as for the quads.)
 * Blending (overlay.py _blending, colour and alpha): out = src * src.a + dst * (1 - src.a), per channel, alpha included.  On the
 * rgba8unorm canvas dst is byte / 255.0f and every primitive's result is stored as floor(255 * clamp(c, 0, 1) + 0.5) (NaN -> 0)
 * before the next one; on the rgba16float canvas it is rounded to float16 (to nearest even, no clamp) after the base layer and
 * after every primitive.
 *
 * Limits (TSP_EINVAL otherwise, nothing written): 0 <= n_layers <= 1024, at most 65536 primitives in all; a quad has a texture of
 * 1..16384 texels per side, 1..128 instances, finite geometry with w, h > 0, |u0| + |du| and |v0| + |dv| <= 1024 and finite
 * offsets / weights; a line set 1..65536 segments, finite width >= 0.  The base layer needs a LUT of 2..65536 entries (scalar,
 * moments), tsp_colormap_set_lut2d (bivariate, TSP_ESTATE), a 4-channel image (rgb) or a kinematic image (moments, TSP_ESTATE).  out: H x W x 4 uint8, or H x W x 4 float16
 * (binary16 bits, uint16) for TSP_PRESENT_RGB_HDR.  Device memory for textures, primitive table and output staging is allocated
 * for the call only (TSP_ENOMEM on failure).  A failed call leaves the accumulator, the presentation image and `out` untouched.
 * gpu_ms_out (or NULL): GPU time of the composition kernel (hipEvents). */
enum { TSP_PRESENT_SCALAR = 0, TSP_PRESENT_BIVARIATE = 1, TSP_PRESENT_RGB = 2, TSP_PRESENT_RGB_HDR = 3, TSP_PRESENT_MOMENT_MEAN = 4,
       TSP_PRESENT_MOMENT_SIGMA = 5 };
enum { TSP_LAYER_QUAD = 0, TSP_LAYER_LINES = 1 };
typedef struct tsp_present_base {
    int map;                         /* TSP_PRESENT_* */
    float vmin, vmax;                /* the already-scaled shader parameters, as tsp_colormap_* take them */
    float density_vmin, density_vmax;    /* bivariate */
    float gamma;                     /* rgb */
    int log_scale, weighted;         /* scalar, bivariate; moments: log_scale */
    const float *lut_rgba;           /* scalar, moments: n_lut RGBA float32 entries */
    int n_lut;
} tsp_present_base;
typedef struct tsp_present_layer {
    int kind;                        /* TSP_LAYER_* */
    /* TSP_LAYER_QUAD */
    const float *texture_rgba;       /* tex_height x tex_width x 4 */
    int tex_width, tex_height;
    float clip_origin[2], clip_extent[2], tex_origin[2], tex_extent[2];
    int n_instances;
    const float *instance_offsets;   /* n_instances x 2 */
    const float *instance_weights;   /* n_instances */
    /* TSP_LAYER_LINES */
    int n_segments;
    const float *starts, *ends;      /* n_segments x 4 (xyzw) */
    float transform[16];             /* row-major */
    float color[4];
    float width_px;
} tsp_present_layer;
int tsp_present(tsp_context *ctx, int width, int height, const tsp_present_base *base, const tsp_present_layer *layers,
                int n_layers, void *out, double *gpu_ms_out);

/* tsp_present_yuv420: the frame tsp_present composes (same base, layers, rules and limits, bit for bit), converted on the device
 * to I420 ("yuv420p") -- what a movie encoder reads (reference recorder/__init__.py _replay draws this frame for every movie frame).
 * out: the W x H Y plane, then the (W/2) x (H/2) U plane, then the V plane (W * H * 3 / 2 bytes), all row-major, row 0 at the top.
 * Integer arithmetic only, `>>` an arithmetic shift (floor); alpha is ignored (the reference drops it, it does not composite).
 * With R, G, B the bytes of a pixel,
 *     Y = ((47 R + 157 G + 16 B + 128) >> 8) + 16                          (every pixel)
 * and for every 2 x 2 block, with the rounded means r = (R00 + R01 + R10 + R11 + 2) >> 2 (g, b alike),
 *     U = ((-26 r - 86 g + 112 b + 128) >> 8) + 128,   V = ((112 r - 102 g - 10 b + 128) >> 8) + 128.
 * These are the BT.709 limited-range ("tv") coefficients rounded so that every grey has U = V = 128 and white has Y = 235; for
 * every input Y lies in [16, 235] and U, V in [16, 240], so nothing is clamped.  Worked values (R, G, B -> Y, U, V): black -> 16,
 * 128, 128; white -> 235, 128, 128; (128, 128, 128) -> 126, 128, 128; red -> 63, 102, 240; green -> 172, 42, 26; blue -> 32, 240, 118.
 * TSP_EINVAL, nothing written, when W or H is odd or outside [2, 16384], when the map is TSP_PRESENT_RGB_HDR, and wherever
 * tsp_present refuses.  A failed call leaves the accumulator, the presentation image and `out` untouched.  Per-call device memory
 * as tsp_present, plus the planes.  gpu_ms_out (or NULL): GPU time of the composition and the conversion together. */
int tsp_present_yuv420(tsp_context *ctx, int width, int height, const tsp_present_base *base, const tsp_present_layer *layers,
                       int n_layers, uint8_t *out, double *gpu_ms_out);

/* tsp_present_surface: the surface map as the base of a composed frame -- what the reference draws in render_mode "surface", where
 * ColorAsSurfaceMap is one more colormap pass onto the canvas, under the same overlays (visualizer.py:367-384, 396;
 * colormap/surface.py:357-365; shaders/surface.wgsl:28-123).  The active image must be the 2-channel (q, depth) image of
 * tsp_render_surface.  Float32 throughout, the operations in the order written, no fused multiply-adds; restated in numpy by
 * tests/surface_present_ref.py.
 *
 * Filtered image.  F is the bilaterally filtered 2-channel image exactly as tsp_surface_present computes it (same ss, rs, kernel
 * size, bits), held in device memory for the call only.
 *
 * Canvas geometry.  S, k, ox, oy, xc, yc, ax, ay are those of "Frame composition".  sample(x, y) is that section's base-layer rule
 * applied to both channels of F at the texel-space coordinates (x, y): for k <= 1 the linear rule (tx = x - 0.5f, ty = y - 0.5f,
 * its lerp with the f == 0 case, clamp-to-edge), for k > 1 F[clamp((int)floorf(y), 0, R-1)][clamp((int)floorf(x), 0, R-1)].
 *
 * Sample spacing.  The reference's texelSize is (1 / W, 1 / H) of the canvas in texture coordinates, and one texture coordinate is
 * R texels, so with du = (float)R / (float)W and dv = (float)R / (float)H:
 *     c = sample(ax, ay),  l = sample(ax - du, ay),  r = sample(ax + du, ay),  u = sample(ax, ay - dv),  d = sample(ax, ay + dv),
 *     Dc = c.depth * depth_scale, and Dl, Dr, Du, Dd alike.
 *
 * Normal and lighting.  n = normalize(-((Dr - Dl) * 0.5f), -((Dd - Du) * 0.5f), 1.0f / (float)W); its length, the division of each
 * component by it, n.L, max(n.L, 0), the material from c.q (log scale, NaN -> 0, the LUT lerp), (diffuse + ambient) *
 * (clamp(Dc, 0, 0.5) * 2), alpha 1 and the rounding to bytes are exactly the shading of tsp_surface_present.
 *
 * Identity.  At W = H = R: k = 1, du = dv = 1, every tx and ty is an integer, the lerp returns the texel itself and clamp-to-edge
 * is the neighbour clamp of the shading, so without layers the frame is tsp_surface_present's rgba8_out bit for bit.
 *
 * Layers, blending, per-primitive quantisation and limits are those of tsp_present on the rgba8unorm canvas; out_rgba8 is
 * H x W x 4 uint8.  tsp_present_surface_yuv420 converts that frame as tsp_present_yuv420 does (even W, H in [2, 16384]); out is
 * W * H * 3 / 2 bytes.
 *
 * TSP_EINVAL, nothing written, wherever tsp_surface_present or tsp_present refuse -- the active image is not 2-channel,
 * smoothing_scale is not finite, weighted_average without a LUT of 2..65536 entries, the canvas or layer limits -- and when
 * depth_scale, a component of light_direction, light_color or ambient_color, or (with weighted_average) vmin or vmax is not
 * finite.  A failed call leaves the accumulator, the presentation image and `out` untouched; a successful one leaves the image
 * and the accumulator unchanged.  Per-call device memory as tsp_present, plus F (8 bytes per pixel of the image) and the LUT
 * (TSP_ENOMEM on failure).  ms_out (or NULL): two values, the GPU milliseconds of the filter and of the composition (for
 * tsp_present_surface_yuv420: the composition and the conversion together). */
int tsp_present_surface(tsp_context *ctx, int width, int height, const tsp_surface_params *params, const tsp_present_layer *layers,
                        int n_layers, uint8_t *out_rgba8, double *ms_out);
int tsp_present_surface_yuv420(tsp_context *ctx, int width, int height, const tsp_surface_params *params,
                               const tsp_present_layer *layers, int n_layers, uint8_t *out, double *ms_out);

/* On-device autorange support (replaces the image read-back + host
 * np.percentile of Colormap.autorange_vmin_vmax / _autorange_using_values, reference
 * src/topsy/colormap/implementation.py:381-425, and RGBColormap.autorange_vmin_vmax :512-531).
 * tsp_content_sort computes the logical content of the render target scaled by `scale` in the same
 * float32 arithmetic numpy uses on the host (kind 0: ch0*scale; 1: (ch1*scale)/(ch0*scale);
 * 2: the three colour channels of an rgb image, flattened; 3: every channel of the image, flattened --
 * what the reference's RGBColormap.autorange_vmin_vmax sees, since it ravel()s the raw 4-channel image
 * including the fragment-count channel), sorts the FINITE values on the device
 * and reports how many there are and how many of them are <= 0.  tsp_content_values then returns
 * the values at the given ranks of that ascending order (the host needs only a handful: min, max,
 * and the neighbours of each percentile's virtual index): TSP_EINVAL for a rank outside [0, n_finite),
 * TSP_ESTATE before the first sort; ranks are checked one by one.  -0.0 sorts before +0.0 and both count
 * as <= 0; denormal products are kept, not flushed.
 * What happens to the values that are not finite: NaN and +inf are dropped and counted nowhere (the host
 * rule ignores them too); -inf is dropped from the sort and from both counts as well, but the host rule
 * `use_log = not (vals < 0).any()` sees it as a negative value, so the sort counts the -inf values and
 * tsp_content_neg_inf reports that count for the last tsp_content_sort (TSP_ESTATE before the first). */
int tsp_content_sort(tsp_context *ctx, int kind, float scale, int64_t *n_finite, int64_t *n_nonpositive);
int tsp_content_values(tsp_context *ctx, const int64_t *ranks, int n_ranks, float *out);
int tsp_content_neg_inf(tsp_context *ctx, int64_t *n_neg_inf);

/* Counters of the last tsp_render call (measurement aid). */
typedef struct {
    int64_t n_particles;   /* particles visited (sum of range lengths) */
    int64_t n_small;       /* splatted by the streaming kernel */
    int64_t n_mid;         /* nearest-mip footprints deferred to kernel G (register gather over per-strip bins) */
    int64_t n_huge;        /* bilinear footprints (P >= 64 px) deferred to the tile-gather kernel */
    int64_t n_culled;      /* z-slab / off-screen / non-finite */
    int64_t n_fragments;   /* pixel updates (only counted when TSP_STATS is enabled) */
    double ms_stream, ms_mid, ms_huge, ms_total; /* per-kernel GPU time, hipEvents; ms_mid = kernel G + its binning passes; ms_huge = kernel H2 + its band fill */
    double ms_mega;        /* reserved (0): a second gather kernel existed in rounds 2-4 */
    int64_t n_mega;        /* reserved (0) */
    /* n_fragments by the kernel that drew them (counted like n_fragments; 0 on the generic pipeline): kernel S, kernel G,
     * kernel H2, reserved (0) -- what bench.py prices each kernel's fragment-rate roofline with */
    int64_t n_fragments_stream, n_fragments_mid, n_fragments_huge, n_fragments_mega;
    /* of n_culled: particles of chunks (512 consecutive particles) whose bounding box lay outside the view -- never read
     * (option "chunk_cull", on by default; needs >= 4096 chunks in the call, pays after tsp_reorder_spatial) */
    int64_t n_chunk_culled;
} tsp_stats;
int tsp_get_stats(tsp_context *ctx, tsp_stats *out);
/* Options by name.  "count_fragments" (0/1): fragment counting (adds atomics; off by default).  "use_quantity" (0/1): render
 * density-only without dropping the resident quantity.  "chunk_cull" (1/0), "reorder_interleave" (1/0, read by the next
 * tsp_reorder_spatial).  The remaining names are tuning and measurement aids of the pipeline ("p_small_milli", "huge_split",
 * "huge_variant", "h2_walk", "h2_chord", "huge_band_mib", "mid_item_records", "mid_item_scale_milli", "stream_blocks_per_cu", "stream_batch_chunks",
 * "overlap_mid_huge", "slice_records", "debug_*"; csrc/tsp_api.hip). */
int tsp_set_option(tsp_context *ctx, const char *name, int64_t value);

/* Streaming-read microbenchmark (float4 read-sum over `bytes` of device memory; best of a few launch shapes): returns GB/s.
 * The measured HBM peak BASELINE.md section 2 prices the roofline fraction against. */
int tsp_measure_read_bandwidth(tsp_context *ctx, int64_t bytes, int iters, double *gbps_out);

/* Multi-GPU: one process per GPU, particles sharded by index range, partial images summed
 * with ONE RCCL reduce over xGMI (the reference has no counterpart).
 * Rank 0 calls tsp_comm_unique_id and distributes the 128-byte id out-of-band. */
#define TSP_UNIQUE_ID_BYTES 128
int tsp_comm_unique_id(char *id_out);
int tsp_comm_init(tsp_context *ctx, int n_ranks, int rank, const char *id);
/* Sum-reduce the float32 render target to `root` (or to every rank when root < 0), in place.
 * Contract: every rank calls it exactly ONCE per frame, after the frame's last tsp_render.  The float64
 * accumulator stays rank-local; the reduced float32 image is a presentation copy (what tsp_read_image,
 * the colormap calls and autorange see), not an accumulator:
 *   - a second call without a tsp_render (or tsp_write_image) in between returns TSP_ESTATE instead of
 *     adding the other ranks' shares twice;
 *   - any later tsp_render -- including a REFINE block with clear = 0 -- rebuilds the float32 image from
 *     the rank's own accumulator, so the frame must be reduced again before it is presented.
 * On ranks other than `root` the image content after the call is unspecified (root >= 0). */
int tsp_comm_reduce_image(tsp_context *ctx, int root, double *gpu_ms_out);
int tsp_comm_destroy(tsp_context *ctx);
/* The same hand-over for a collective the CALLER performed (shards summed through the host: contexts that share a device,
 * which RCCL refuses, or no RCCL at all): `sum` (R * R * C float32) becomes the float32 presentation image of `ctx`; its
 * float64 accumulator keeps the context's own partial sums, so a later tsp_render with clear = 0 continues unrounded --
 * exactly the state tsp_comm_reduce_image leaves on the root.  Same once-per-frame rule (TSP_ESTATE on a second call). */
int tsp_set_reduced_image(tsp_context *ctx, const float *sum);

/* Several GPUs of one node behind ONE handle (SURVEY.md section 8b sketched `tsp_create(n_devices, device_ids, ...)`; the
 * reference has no counterpart -- its SplitBuffers, src/topsy/split_buffers.py:26-38,78-116, cuts one device's buffers the same
 * way).  A group is n_devices ordinary contexts plus the host-thread choreography: uploads are cut into the contiguous index
 * ranges [g N / G, (g + 1) N / G), tsp_group_render intersects the block's (start, len) ranges with every shard and runs the
 * G tsp_render calls concurrently (returns the slowest shard's GPU time), and tsp_group_end_frame is the frame's ONE sum-reduce
 * of the float32 image onto context 0 -- RCCL over xGMI when the device ids are distinct, a read-back / add of the float32
 * partial images through the host and tsp_set_reduced_image when two contexts share a device (RCCL refuses that; single-GPU test
 * boxes) or librccl cannot be loaded.  Everything that looks at the finished
 * frame (tsp_read_image, tsp_colormap_*, tsp_content_*, tsp_tile_periodic) is called on tsp_group_context(group, 0) after
 * tsp_group_end_frame; per-shard state can be inspected through tsp_group_context(group, g).  The reduce contract of
 * tsp_comm_reduce_image holds: end_frame reduces at most once per rendered frame, and a later tsp_group_render -- a REFINE
 * block with clear = 0 included -- continues from every shard's own float64 accumulator.  A block draws on every member or on
 * none: when one member's tsp_render fails, tsp_group_render puts the members that succeeded back as it found them
 * (tsp_render_undo) before it returns that member's error ("context g (device d): ..."), every member's float32 image is its
 * own partial image again, and the next tsp_group_end_frame sums them anew -- so a retried clear = 0 block is counted once.
 * Exceptions, both about a member touched through tsp_group_context: one whose tsp_render is refused before it touches
 * anything -- its accumulator holds the keys of tsp_render_surface and the block has clear = 0, or its device cannot be
 * selected -- has nothing to take back and is left as it is, reduced state included (if it is context 0 and still presents a
 * reduced frame, that frame stands and is not summed again); and one on which the block replaced a surface image keeps the
 * block, because tsp_render_undo does not restore surface keys.
 * Failed uploads ("Failed uploads" at tsp_upload_particles): a snapshot is resident on every member or on none -- when
 * tsp_upload_particles or tsp_generate_synthetic fails on one member, tsp_group_upload_particles /
 * tsp_group_generate_synthetic empty EVERY member, tsp_group_num_particles returns 0, and that member's code and message are
 * returned; a tsp_group_render then draws nothing.  The group's attribute uploads (quantity, rgb, band magnitudes) are NOT
 * transactional across the members: each member follows rule 1 on its own, so after a failure the failing member holds the
 * old attribute and every other member the old or the new one -- upload the attribute again before rendering.
 * Calls on one group must be
 * serialised by the caller.  tsp_group_get_stats: counters summed over the shards, times of the slowest shard. */
typedef struct tsp_group tsp_group;
int tsp_group_create(int n_devices, const int *device_ids, int resolution, int n_channels, tsp_group **out);
void tsp_group_destroy(tsp_group *group);
int tsp_group_size(tsp_group *group);
tsp_context *tsp_group_context(tsp_group *group, int index);
int tsp_group_uses_rccl(tsp_group *group);
int tsp_group_set_kernel_mips(tsp_group *group, const float *lut, int n0, int n_levels);
int tsp_group_upload_particles(tsp_group *group, int64_t n, const float *x, const float *y, const float *z, const float *h,
                               const float *mass);
int tsp_group_upload_quantity(tsp_group *group, const float *q);
int tsp_group_upload_rgb(tsp_group *group, const float *r, const float *g, const float *b);
int tsp_group_generate_synthetic(tsp_group *group, int64_t n_total, int64_t first, int64_t count, uint64_t seed, float h_cap,
                                 int with_quantity, int with_rgb);
int tsp_group_reorder_spatial(tsp_group *group, int n_strata, uint64_t seed);
int64_t tsp_group_num_particles(tsp_group *group);
int tsp_group_set_option(tsp_group *group, const char *name, int64_t value);
int tsp_group_render(tsp_group *group, const float *M, float scale_factor, const int64_t *starts, const int64_t *lens,
                     int n_ranges, int clear, int mode, int flags, double *gpu_ms_out);
int tsp_group_end_frame(tsp_group *group, double *ms_out);
int tsp_group_get_stats(tsp_group *group, tsp_stats *out);
/* Shard `index` owns the global indices [*first_out, *first_out + *count_out) of the last upload / generate. */
int tsp_group_shard_range(tsp_group *group, int index, int64_t *first_out, int64_t *count_out);
/* tsp_upload_band_magnitudes for the group: mags is [n_bands][N] over the whole snapshot, every shard takes its columns. */
int tsp_group_upload_band_magnitudes(tsp_group *group, int n_bands, const double *mags, const double *weights);

#ifdef __cplusplus
}
#endif
#endif /* TOPSY_SPLAT_H */
