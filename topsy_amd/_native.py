"""ctypes binding of libtopsy_splat.so -- the only route from the Python host layer to the GPU.

There is deliberately NO fallback: if the HIP library is missing or no GPU is present the
product raises `BackendUnavailable` (the CPU oracle under oracle/ is test infrastructure and is
never imported from here).
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TOPSY_SPLAT_LIB") or os.path.join(_HERE, "libtopsy_splat.so")    # TOPSY_SPLAT_LIB: an alternative build (A/B measurements)

MODE_WEIGHTED, MODE_DEPTH, MODE_RGB, MODE_KINEMATIC = 0, 1, 2, 3
PIPE_DEFAULT, PIPE_GENERIC = 0, 1
SAMPLE_BILINEAR_MIP0, SAMPLE_BILINEAR_MIP = 0x10, 0x20      # diagnostic sampling rules (generic kernel)
UNIQUE_ID_BYTES = 128
ABI_VERSION = 112            # the oldest tsp_version() whose structs this binding matches; entry points added since
                             # (113: tsp_shrink_sphere_center, 114: tsp_fof_groups, 115: tsp_sphere_moments,
                             # 116: tsp_radial_profile, 117: the kinematic maps, 119: tsp_moment_sort,
                             # 120: tsp_sph_velocity_gradient, 122: tsp_sph_sample_lattice, 123: tsp_gravity_direct,
                             # 124: tsp_gravity_tree, 125: tsp_group_potential, tsp_halo_properties, 126: tsp_spectral_cube,
                             # 127: tsp_histogram_2d, 128: tsp_project_perspective) are required by
                             # name in load_library()
PRESENT_SCALAR, PRESENT_BIVARIATE, PRESENT_RGB, PRESENT_RGB_HDR, PRESENT_MOMENT_MEAN, PRESENT_MOMENT_SIGMA = 0, 1, 2, 3, 4, 5
LAYER_QUAD, LAYER_LINES = 0, 1


class SurfaceParams(ctypes.Structure):
    """struct tsp_surface_params (include/topsy_splat.h)."""
    _fields_ = [("smoothing_scale", ctypes.c_double), ("depth_scale", ctypes.c_float),
                ("light_direction", ctypes.c_float * 3), ("light_color", ctypes.c_float * 3), ("ambient_color", ctypes.c_float * 3),
                ("vmin", ctypes.c_float), ("vmax", ctypes.c_float), ("weighted_average", ctypes.c_int), ("log_scale", ctypes.c_int),
                ("lut_rgba", ctypes.POINTER(ctypes.c_float)), ("n_lut", ctypes.c_int)]


class PresentBase(ctypes.Structure):
    """struct tsp_present_base (include/topsy_splat.h "Frame composition")."""
    _fields_ = [("map", ctypes.c_int), ("vmin", ctypes.c_float), ("vmax", ctypes.c_float), ("density_vmin", ctypes.c_float),
                ("density_vmax", ctypes.c_float), ("gamma", ctypes.c_float), ("log_scale", ctypes.c_int), ("weighted", ctypes.c_int),
                ("lut_rgba", ctypes.POINTER(ctypes.c_float)), ("n_lut", ctypes.c_int)]


class PresentLayer(ctypes.Structure):
    """struct tsp_present_layer."""
    _fields_ = [("kind", ctypes.c_int), ("texture_rgba", ctypes.POINTER(ctypes.c_float)), ("tex_width", ctypes.c_int),
                ("tex_height", ctypes.c_int), ("clip_origin", ctypes.c_float * 2), ("clip_extent", ctypes.c_float * 2),
                ("tex_origin", ctypes.c_float * 2), ("tex_extent", ctypes.c_float * 2), ("n_instances", ctypes.c_int),
                ("instance_offsets", ctypes.POINTER(ctypes.c_float)), ("instance_weights", ctypes.POINTER(ctypes.c_float)),
                ("n_segments", ctypes.c_int), ("starts", ctypes.POINTER(ctypes.c_float)), ("ends", ctypes.POINTER(ctypes.c_float)),
                ("transform", ctypes.c_float * 16), ("color", ctypes.c_float * 4), ("width_px", ctypes.c_float)]


class CenterInfo(ctypes.Structure):
    """struct tsp_center_info."""
    _fields_ = [("n_valid", ctypes.c_int64), ("n_inside", ctypes.c_int64), ("iterations", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("radius", ctypes.c_double), ("mass_inside", ctypes.c_double)]


class FofInfo(ctypes.Structure):
    """struct tsp_fof_info."""
    _fields_ = [("n_valid", ctypes.c_int64), ("n_groups", ctypes.c_int64), ("n_grouped", ctypes.c_int64),
                ("largest", ctypes.c_int64)]


class Moments(ctypes.Structure):
    """struct tsp_moments."""
    _fields_ = [("n_valid", ctypes.c_int64), ("n_inside", ctypes.c_int64), ("n_inside_vel", ctypes.c_int64),
                ("mass", ctypes.c_double), ("mass_vel", ctypes.c_double), ("com", ctypes.c_double * 3),
                ("v_cen", ctypes.c_double * 3), ("L", ctypes.c_double * 3), ("S", ctypes.c_double * 6), ("A", ctypes.c_double)]

    def as_dict(self):
        """Counts as int, sums as float, vectors as float64 arrays."""
        out = {}
        for name, kind in self._fields_:
            v = getattr(self, name)
            out[name] = int(v) if kind is ctypes.c_int64 else float(v) if kind is ctypes.c_double else np.array(v, dtype=np.float64)
        return out


class ProfileSpec(ctypes.Structure):
    """struct tsp_profile_spec."""
    _fields_ = [("geometry", ctypes.c_int32), ("n_bins", ctypes.c_int32), ("edges", ctypes.POINTER(ctypes.c_double)),
                ("center", ctypes.c_double * 3), ("v_cen", ctypes.c_double * 3), ("frame", ctypes.c_double * 9),
                ("half_height", ctypes.c_double)]


class ProfileInfo(ctypes.Structure):
    """struct tsp_profile_info."""
    _fields_ = [("n_valid", ctypes.c_int64), ("n_inner", ctypes.c_int64), ("n_binned", ctypes.c_int64),
                ("mass_inner", ctypes.c_double)]


class Hist2dSpec(ctypes.Structure):
    """struct tsp_hist2d_spec."""
    _fields_ = [("nx", ctypes.c_int32), ("ny", ctypes.c_int32), ("edges_x", ctypes.POINTER(ctypes.c_double)),
                ("edges_y", ctypes.POINTER(ctypes.c_double))]


class Hist2dInfo(ctypes.Structure):
    """struct tsp_hist2d_info."""
    _fields_ = [("n_valid", ctypes.c_int64), ("n_binned", ctypes.c_int64)]


class Perspective(ctypes.Structure):
    """struct tsp_perspective: view = rot @ (position + offset); the viewer sits at view z = +distance and looks down -z."""
    _fields_ = [("rot", ctypes.c_float * 9), ("offset", ctypes.c_float * 3), ("distance", ctypes.c_float), ("near", ctypes.c_float)]


class Lattice(ctypes.Structure):
    """struct tsp_lattice: point (i, j, k) is origin + i du + j dv + k dw."""
    _fields_ = [("origin", ctypes.c_double * 3), ("du", ctypes.c_double * 3), ("dv", ctypes.c_double * 3),
                ("dw", ctypes.c_double * 3), ("nu", ctypes.c_int32), ("nv", ctypes.c_int32), ("nw", ctypes.c_int32)]


class GravityInfo(ctypes.Structure):
    """struct tsp_gravity_info."""
    _fields_ = [("n_valid_sources", ctypes.c_int64), ("n_valid_targets", ctypes.c_int64)]


# tsp_gravity_direct (the header's TSP_GRAVITY_* constants): sources per tile of the pair kernel, targets of a workgroup at most,
# and K of its error bound |got - want| <= K * 2^-24 * sum |term|
GRAVITY_SOURCE_TILE = 512
GRAVITY_TARGETS_PER_WORKGROUP = 1024
GRAVITY_ERROR_K = 64


class GravityTreeInfo(ctypes.Structure):
    """struct tsp_gravity_tree_info."""
    _fields_ = [(name, ctypes.c_int64) for name in ("n_valid_sources", "n_valid_targets", "n_nodes", "n_levels", "pairs_direct",
                                                    "pairs_node")]


# tsp_gravity_tree (the header's TSP_GRAVITY_TREE_* constants): sorted particles per leaf, nodes of a level per node of the next,
# and K of its rounding bound
GRAVITY_TREE_LEAF = 32
GRAVITY_TREE_FANOUT = 8
GRAVITY_TREE_ERROR_K = 64


class GroupPotentialInfo(ctypes.Structure):
    """struct tsp_group_potential_info."""
    _fields_ = [(name, ctypes.c_int64) for name in ("n_members", "n_groups_nonempty", "pairs", "pair_slots", "n_skipped_groups",
                                                    "n_skipped_members")] + [("max_extent", ctypes.c_double)]


class HaloInfo(ctypes.Structure):
    """struct tsp_halo_info."""
    _fields_ = [("n_members", ctypes.c_int64), ("max_extent", ctypes.c_double)]


# tsp_group_potential / tsp_halo_properties (the header's TSP_HALO_* constants): the pair kernel's tile and target block, and the
# first column of every property in a row of props_out
HALO_SOURCE_TILE = 512
HALO_TARGET_BLOCK = 1024
HALO_COLUMNS = {"mass": 0, "com": 1, "v_com": 4, "S": 7, "L": 13, "e_kin": 16, "sigma2": 17, "r_max": 18, "r_half": 19, "v2_max": 20,
                "r_vmax": 21, "e_pot": 22, "m_bound": 23, "pot_pos": 24, "i_half": 27, "i_vmax": 28}
HALO_NPROPS = 29
LATTICE_MAX_FIELDS = 4       # fields per tsp_sph_sample_lattice call
CUBE_MAX_CHANNELS = 4096     # tsp_spectral_cube: n_channels at most
CUBE_MAX_CELLS = 1 << 31     # ... and n_channels * R * R
CUBE_LAYOUT_NAMES = ("tiles", "blocks", "bins", "key_bits", "slice_particles", "slices", "list_capacity",
                     "h_sigma", "h_geom", "h_line", "h_bytes", "a_cube", "a_count", "a_offset", "a_keys", "a_keys_sorted", "a_index",
                     "a_index_sorted", "a_bin_first", "a_bin_end", "a_tmp", "a_bytes")      # tsp_spectral_cube_layout's values
HIST2D_MAX_BINS = 1024      # tsp_histogram_2d: bins per axis at most
HIST2D_BLOCK = 256          # ... and the sorted entries a workgroup of its reduction takes (the header's TSP_HIST2D_BLOCK)
_HIST2D_REGIONS_H = ("h_x", "h_y", "h_w", "h_v")
_HIST2D_REGIONS_A = ("a_count", "a_sums", "a_edges", "a_counters", "a_keys", "a_keys_sorted", "a_index", "a_index_sorted",
                     "a_records_a", "a_records_b", "a_tmp")
HIST2D_LAYOUT_NAMES = (("key_bits", "block", "levels", "blocks", "records_a", "records_b")
                       + tuple(f"{r}{suffix}" for r in _HIST2D_REGIONS_H for suffix in ("", "_size")) + ("h_bytes",)
                       + tuple(f"{r}{suffix}" for r in _HIST2D_REGIONS_A for suffix in ("", "_size")) + ("a_bytes", "bins_bytes"))
                                                                                        # tsp_histogram_2d_layout's values
PROFILE_SUMS = 11           # doubles per bin of tsp_radial_profile's sums_out: mass, ms, mc (3), mc2 (3), mj (3)


class BackendUnavailable(RuntimeError):
    """libtopsy_splat.so could not be loaded, or no MI355X-class GPU is visible."""


class BackendError(RuntimeError):
    """A C-ABI call returned a negative status."""


class Stats(ctypes.Structure):
    _fields_ = [("n_particles", ctypes.c_int64), ("n_small", ctypes.c_int64), ("n_mid", ctypes.c_int64),
                ("n_huge", ctypes.c_int64), ("n_culled", ctypes.c_int64), ("n_fragments", ctypes.c_int64),
                ("ms_stream", ctypes.c_double), ("ms_mid", ctypes.c_double), ("ms_huge", ctypes.c_double),
                ("ms_total", ctypes.c_double), ("ms_mega", ctypes.c_double), ("n_mega", ctypes.c_int64),
                ("n_fragments_stream", ctypes.c_int64), ("n_fragments_mid", ctypes.c_int64),
                ("n_fragments_huge", ctypes.c_int64), ("n_fragments_mega", ctypes.c_int64), ("n_chunk_culled", ctypes.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_fp = ctypes.POINTER(ctypes.c_float)
_i64p = ctypes.POINTER(ctypes.c_int64)
_u8p = ctypes.POINTER(ctypes.c_uint8)
_ctx = ctypes.c_void_p

# name -> (restype, argtypes); every symbol declared in include/topsy_splat.h
SIGNATURES = {
    "tsp_last_error": (ctypes.c_char_p, []),
    "tsp_version": (ctypes.c_int, []),
    "tsp_stats_size": (ctypes.c_int, []),
    "tsp_device_count": (ctypes.c_int, []),
    "tsp_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_ctx)]),
    "tsp_destroy": (None, [_ctx]),
    "tsp_set_kernel_mips": (ctypes.c_int, [_ctx, _fp, ctypes.c_int, ctypes.c_int]),
    "tsp_upload_particles": (ctypes.c_int, [_ctx, ctypes.c_int64, _fp, _fp, _fp, _fp, _fp]),
    "tsp_upload_quantity": (ctypes.c_int, [_ctx, _fp]),
    "tsp_upload_rgb": (ctypes.c_int, [_ctx, _fp, _fp, _fp]),
    "tsp_upload_velocities": (ctypes.c_int, [_ctx, _fp, _fp, _fp]),
    "tsp_set_line_of_sight": (ctypes.c_int, [_ctx, _fp, _fp]),
    "tsp_velocity_moments": (ctypes.c_int, [_ctx, _fp]),
    "tsp_spectral_cube": (ctypes.c_int, [_ctx, _fp, ctypes.c_float, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_float,
                                         _fp, _fp]),
    "tsp_spectral_cube_layout": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int, _i64p]),
    "tsp_colormap_moment": (ctypes.c_int, [_ctx, ctypes.c_int, _fp, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_int, _u8p]),
    "tsp_upload_band_magnitudes": (ctypes.c_int, [_ctx, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "tsp_generate_synthetic": (ctypes.c_int, [_ctx, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_uint64,
                                              ctypes.c_float, ctypes.c_int, ctypes.c_int]),
    "tsp_reorder_spatial": (ctypes.c_int, [_ctx, ctypes.c_int, ctypes.c_uint64, _i64p]),
    "tsp_get_strata_offsets": (ctypes.c_int, [_ctx, _i64p, ctypes.c_int]),
    "tsp_get_cell_layout": (ctypes.c_int, [_ctx, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), _fp, _fp]),
    "tsp_get_cell_offsets": (ctypes.c_int64, [_ctx, _i64p, ctypes.c_int64]),
    "tsp_download_particles": (ctypes.c_int, [_ctx] + [_fp] * 9),
    "tsp_project_perspective": (ctypes.c_int, [_ctx, _ctx, ctypes.POINTER(Perspective)]),
    "tsp_num_particles": (ctypes.c_int64, [_ctx]),
    "tsp_render": (ctypes.c_int, [_ctx, _fp, ctypes.c_float, _i64p, _i64p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                  ctypes.c_int, ctypes.POINTER(ctypes.c_double)]),
    "tsp_render_undo": (ctypes.c_int, [_ctx]),
    "tsp_read_image": (ctypes.c_int, [_ctx, _fp]),
    "tsp_write_image": (ctypes.c_int, [_ctx, _fp]),
    "tsp_colormap_scalar": (ctypes.c_int, [_ctx, _fp, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_int,
                                           ctypes.c_int, _u8p]),
    "tsp_colormap_rgb": (ctypes.c_int, [_ctx, ctypes.c_float, ctypes.c_float, ctypes.c_float, _u8p, _fp]),
    "tsp_colormap_set_lut2d": (ctypes.c_int, [_ctx, _fp, ctypes.c_int]),
    "tsp_colormap_bivariate": (ctypes.c_int, [_ctx, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_int,
                                              ctypes.c_int, _u8p]),
    "tsp_colormap_bivariate_host": (ctypes.c_int, [_ctx, _fp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float,
                                                   ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_int, _u8p]),
    "tsp_colormap_scalar_host": (ctypes.c_int, [_ctx, _fp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _fp, ctypes.c_int,
                                                ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_int, _u8p]),
    "tsp_colormap_rgb_host": (ctypes.c_int, [_ctx, _fp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                             ctypes.c_float, ctypes.c_float, _u8p, _fp]),
    "tsp_tile_periodic": (ctypes.c_int, [_ctx, ctypes.c_int, _fp, _fp]),
    "tsp_smoothing_lengths": (ctypes.c_int, [_ctx, ctypes.c_int64, _fp, _fp, _fp, ctypes.c_int, ctypes.c_float, _fp]),
    "tsp_sph_sum": (ctypes.c_int, [_ctx, ctypes.c_int64, _fp, _fp, _fp, _fp, _fp, ctypes.c_float, _fp]),
    "tsp_sph_velocity_gradient": (ctypes.c_int, [_ctx, ctypes.c_int64] + [_fp] * 9 + [ctypes.c_float] + [_fp] * 4),
    "tsp_sph_sample_lattice": (ctypes.c_int, [_ctx, ctypes.c_int64, _fp, _fp, _fp, ctypes.c_int, ctypes.POINTER(_fp), ctypes.c_int,
                                              ctypes.c_float, ctypes.POINTER(Lattice), _fp, ctypes.POINTER(_fp)]),
    "tsp_shrink_sphere_center": (ctypes.c_int, [_ctx, ctypes.c_int64, _fp, _fp, _fp, _fp, ctypes.c_float, ctypes.c_double,
                                                ctypes.c_double, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                                ctypes.POINTER(CenterInfo)]),
    "tsp_fof_groups": (ctypes.c_int, [_ctx, ctypes.c_int64, _fp, _fp, _fp, ctypes.c_float, ctypes.c_float, ctypes.c_int64,
                                      ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(FofInfo)]),
    "tsp_sphere_moments": (ctypes.c_int, [_ctx, ctypes.c_int64, _fp, _fp, _fp, _fp, _fp, _fp, _fp, ctypes.POINTER(ctypes.c_double),
                                          ctypes.c_double, ctypes.c_double, ctypes.POINTER(Moments)]),
    "tsp_radial_profile": (ctypes.c_int, [_ctx, ctypes.c_int64, _fp, _fp, _fp, _fp, _fp, _fp, _fp, ctypes.POINTER(ProfileSpec), _i64p,
                                          ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ProfileInfo)]),
    "tsp_histogram_2d": (ctypes.c_int, [_ctx, ctypes.c_int64, _fp, _fp, _fp, _fp, ctypes.POINTER(Hist2dSpec), _i64p,
                                        ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(Hist2dInfo)]),
    "tsp_histogram_2d_layout": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _i64p]),
    "tsp_gravity_direct": (ctypes.c_int, [_ctx, ctypes.c_int64, _fp, _fp, _fp, _fp, _fp, ctypes.c_float, ctypes.c_int64, _fp, _fp, _fp,
                                          ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                          ctypes.POINTER(GravityInfo)]),
    "tsp_gravity_tree": (ctypes.c_int, [_ctx, ctypes.c_int64, _fp, _fp, _fp, _fp, _fp, ctypes.c_float, ctypes.c_int64, _fp, _fp, _fp,
                                        ctypes.c_float, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                        ctypes.POINTER(GravityTreeInfo)]),
    "tsp_group_potential": (ctypes.c_int, [_ctx, ctypes.c_int64, _fp, _fp, _fp, _fp, _fp, ctypes.c_float, ctypes.POINTER(ctypes.c_int32),
                                           ctypes.c_int64, ctypes.c_double, ctypes.c_int64, ctypes.POINTER(ctypes.c_double),
                                           ctypes.POINTER(GroupPotentialInfo)]),
    "tsp_halo_properties": (ctypes.c_int, [_ctx, ctypes.c_int64, _fp, _fp, _fp, _fp, _fp, _fp, _fp, ctypes.POINTER(ctypes.c_double),
                                           ctypes.POINTER(ctypes.c_int32), ctypes.c_int64, ctypes.c_double, _i64p, _i64p, _i64p,
                                           ctypes.POINTER(ctypes.c_double), ctypes.POINTER(HaloInfo)]),
    "tsp_set_sphere_mips": (ctypes.c_int, [_ctx, _fp, ctypes.c_int, ctypes.c_int]),
    "tsp_density_order_stats": (ctypes.c_int, [_ctx, _i64p, ctypes.c_int, _fp]),
    "tsp_render_surface": (ctypes.c_int, [_ctx, _fp, ctypes.c_float, ctypes.c_float, _i64p, _i64p, ctypes.c_int, ctypes.c_int,
                                          ctypes.POINTER(ctypes.c_double)]),
    "tsp_surface_present": (ctypes.c_int, [_ctx, ctypes.c_void_p, _fp, _u8p, ctypes.POINTER(ctypes.c_double)]),
    "tsp_present": (ctypes.c_int, [_ctx, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                   ctypes.POINTER(ctypes.c_double)]),
    "tsp_present_yuv420": (ctypes.c_int, [_ctx, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, _u8p,
                                          ctypes.POINTER(ctypes.c_double)]),
    "tsp_present_surface": (ctypes.c_int, [_ctx, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, _u8p,
                                           ctypes.POINTER(ctypes.c_double)]),
    "tsp_present_surface_yuv420": (ctypes.c_int, [_ctx, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                                  _u8p, ctypes.POINTER(ctypes.c_double)]),
    "tsp_content_sort": (ctypes.c_int, [_ctx, ctypes.c_int, ctypes.c_float, _i64p, _i64p]),
    "tsp_moment_sort": (ctypes.c_int, [_ctx, ctypes.c_int, ctypes.c_int, _i64p]),
    "tsp_content_values": (ctypes.c_int, [_ctx, _i64p, ctypes.c_int, _fp]),
    "tsp_content_neg_inf": (ctypes.c_int, [_ctx, _i64p]),
    "tsp_get_stats": (ctypes.c_int, [_ctx, ctypes.POINTER(Stats)]),
    "tsp_set_option": (ctypes.c_int, [_ctx, ctypes.c_char_p, ctypes.c_int64]),
    "tsp_measure_read_bandwidth": (ctypes.c_int, [_ctx, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]),
    "tsp_comm_unique_id": (ctypes.c_int, [ctypes.c_char_p]),
    "tsp_comm_init": (ctypes.c_int, [_ctx, ctypes.c_int, ctypes.c_int, ctypes.c_char_p]),
    "tsp_comm_reduce_image": (ctypes.c_int, [_ctx, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]),
    "tsp_comm_destroy": (ctypes.c_int, [_ctx]),
    "tsp_set_reduced_image": (ctypes.c_int, [_ctx, _fp]),
    # several GPUs behind one handle (C clients; the Python layer's own driver is multigpu.MultiGpuContext)
    "tsp_group_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int, ctypes.POINTER(_ctx)]),
    "tsp_group_destroy": (None, [_ctx]),
    "tsp_group_size": (ctypes.c_int, [_ctx]),
    "tsp_group_context": (_ctx, [_ctx, ctypes.c_int]),
    "tsp_group_uses_rccl": (ctypes.c_int, [_ctx]),
    "tsp_group_set_kernel_mips": (ctypes.c_int, [_ctx, _fp, ctypes.c_int, ctypes.c_int]),
    "tsp_group_upload_particles": (ctypes.c_int, [_ctx, ctypes.c_int64, _fp, _fp, _fp, _fp, _fp]),
    "tsp_group_upload_quantity": (ctypes.c_int, [_ctx, _fp]),
    "tsp_group_upload_rgb": (ctypes.c_int, [_ctx, _fp, _fp, _fp]),
    "tsp_group_generate_synthetic": (ctypes.c_int, [_ctx, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_uint64,
                                                    ctypes.c_float, ctypes.c_int, ctypes.c_int]),
    "tsp_group_reorder_spatial": (ctypes.c_int, [_ctx, ctypes.c_int, ctypes.c_uint64]),
    "tsp_group_num_particles": (ctypes.c_int64, [_ctx]),
    "tsp_group_set_option": (ctypes.c_int, [_ctx, ctypes.c_char_p, ctypes.c_int64]),
    "tsp_group_render": (ctypes.c_int, [_ctx, _fp, ctypes.c_float, _i64p, _i64p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_int, ctypes.POINTER(ctypes.c_double)]),
    "tsp_group_end_frame": (ctypes.c_int, [_ctx, ctypes.POINTER(ctypes.c_double)]),
    "tsp_group_get_stats": (ctypes.c_int, [_ctx, ctypes.POINTER(Stats)]),
    "tsp_group_shard_range": (ctypes.c_int, [_ctx, ctypes.c_int, _i64p, _i64p]),
    "tsp_group_upload_band_magnitudes": (ctypes.c_int, [_ctx, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
}

_lib = None


def load_library():
    """dlopen libtopsy_splat.so and declare every prototype. Raises BackendUnavailable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BackendUnavailable(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"or `make -C topsy_amd/csrc` (needs hipcc, --offload-arch=gfx950)")
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:
        raise BackendUnavailable(f"cannot load {LIB_PATH}: {e}") from e
    for name, (restype, argtypes) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise BackendUnavailable(f"{LIB_PATH} does not export {name}") from e
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.tsp_version() < ABI_VERSION or lib.tsp_stats_size() != ctypes.sizeof(Stats):
        raise BackendUnavailable(f"{LIB_PATH} has ABI version {lib.tsp_version()} / tsp_stats of {lib.tsp_stats_size()} bytes; "
                                 f"this binding needs version >= {ABI_VERSION} and {ctypes.sizeof(Stats)} bytes: rebuild the library")
    _lib = lib
    return lib


def lattice_struct(origin, du, dv, dw, shape):
    """The tsp_lattice of shape = (nu, nv, nw) points origin + i du + j dv + k dw.  Raises ValueError for a shape that is not
    three integers >= 1 with fewer than 2^31 points in all, or vectors that are not three finite numbers."""
    try:
        dims = [int(v) for v in shape]
        exact = all(not isinstance(v, bool) and int(v) == v for v in shape)
    except (TypeError, ValueError):
        dims, exact = [], False
    if len(dims) != 3 or not exact or min(dims) < 1 or dims[0] * dims[1] * dims[2] >= 2 ** 31:
        raise ValueError(f"shape must be three integers >= 1 with fewer than 2^31 points in all, not {shape!r}")
    lat = Lattice()
    for name, v in (("origin", origin), ("du", du), ("dv", dv), ("dw", dw)):
        try:
            a = np.asarray(v, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{name} must be three finite numbers, not {v!r}") from None
        if a.shape != (3,) or not np.isfinite(a).all():
            raise ValueError(f"{name} must be three finite numbers, not {v!r}")
        getattr(lat, name)[:] = a.tolist()
    lat.nu, lat.nv, lat.nw = dims
    return lat


def perspective_struct(rot, offset, distance, near):
    """The tsp_perspective of a (3, 3) rotation, a (3,) offset, the distance to the reference plane and the near distance, each
    rounded to float32.  Raises ValueError for a wrong shape, a value that is not finite, distance <= 0 or near outside
    (0, distance) -- what the library would refuse with TSP_EINVAL."""
    cam = Perspective()
    for name, v, shape in (("rot", rot, (3, 3)), ("offset", offset, (3,))):
        try:
            a = np.asarray(v, dtype=np.float32)
        except (TypeError, ValueError):
            raise ValueError(f"{name} must be {shape} finite numbers, not {v!r}") from None
        if a.shape != shape or not np.isfinite(a).all():
            raise ValueError(f"{name} must be {shape} finite numbers, not {v!r}")
        getattr(cam, name)[:] = a.ravel().tolist()
    try:
        d, nr = float(np.float32(distance)), float(np.float32(near))
    except (TypeError, ValueError):
        raise ValueError(f"distance and near must be numbers, not {distance!r} and {near!r}") from None
    if not (np.isfinite(d) and d > 0):
        raise ValueError(f"distance must be finite and > 0, not {distance!r}")
    if not (np.isfinite(nr) and 0 < nr < d):
        raise ValueError(f"near must be finite, > 0 and < distance, not {near!r}")
    cam.distance, cam.near = d, nr
    return cam


def _check(rc):
    if rc < 0:
        raise BackendError(f"libtopsy_splat error {rc}: {load_library().tsp_last_error().decode(errors='replace')}")
    return rc


def _f32(a, n=None, name="array"):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if n is not None and a.size != n:
        raise ValueError(f"{name} has {a.size} elements, expected {n}")
    return a


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_fp)


def device_count():
    return load_library().tsp_device_count()


def spectral_cube_layout(n, resolution, n_channels, slice_option=0, has_sigma=False):
    """The host arithmetic of tsp_spectral_cube as a dict (CUBE_LAYOUT_NAMES): tiles, channel blocks, bins, particles per slice,
    slices, list capacity and the byte offsets of its two device buffers (tsp_spectral_cube_layout; needs no GPU)."""
    out = np.zeros(len(CUBE_LAYOUT_NAMES), dtype=np.int64)
    _check(load_library().tsp_spectral_cube_layout(int(n), int(resolution), int(n_channels), int(slice_option), int(bool(has_sigma)),
                                                   out.ctypes.data_as(_i64p)))
    return dict(zip(CUBE_LAYOUT_NAMES, out.tolist()))


def histogram_2d_layout(n, nx, ny, has_w=False, has_v=False, want_bins=False):
    """The host arithmetic of tsp_histogram_2d as a dict (HIST2D_LAYOUT_NAMES): the bits of a key, the block of the reduction, its
    levels and blocks, the records of its two record buffers, and per region of the two device buffers the byte offset (`name`) and
    the bytes used (`name_size`) (tsp_histogram_2d_layout; needs no GPU)."""
    out = np.zeros(len(HIST2D_LAYOUT_NAMES), dtype=np.int64)
    _check(load_library().tsp_histogram_2d_layout(int(n), int(nx), int(ny), int(bool(has_w)), int(bool(has_v)), int(bool(want_bins)),
                                                  out.ctypes.data_as(_i64p)))
    return dict(zip(HIST2D_LAYOUT_NAMES, out.tolist()))


def _ranges(starts, lens):
    """(starts pointer, lens pointer, count, the arrays the pointers lend from) of a render call's ranges; None = no ranges."""
    if starts is None:
        return None, None, 0, None
    s = np.ascontiguousarray(starts, dtype=np.int64)
    l = np.ascontiguousarray(lens, dtype=np.int64)
    if s.shape != l.shape or s.ndim != 1:
        raise ValueError("starts and lens must be 1-D arrays of equal length")
    if len(s) == 0:
        # an empty selection (e.g. view culling picked no cell of this block) draws nothing: hand the library one
        # explicit zero-length range so that it can never be read as "no ranges given = all particles"
        s = np.zeros(1, dtype=np.int64)
        l = np.zeros(1, dtype=np.int64)
    return s.ctypes.data_as(_i64p), l.ctypes.data_as(_i64p), len(s), (s, l)


class Context:
    """One GPU renderer: R x R x C float32 target + resident SoA particles (include/topsy_splat.h)."""

    def __init__(self, resolution, n_channels, device_id=0):
        lib = load_library()
        ndev = lib.tsp_device_count()
        if ndev <= 0:
            raise BackendUnavailable("no HIP device visible: the topsy_amd render path needs an AMD GPU "
                                     "(there is no CPU fallback)")
        h = _ctx()
        _check(lib.tsp_create(int(device_id), int(resolution), int(n_channels), ctypes.byref(h)))
        self._h = h
        self._lib = lib
        self.resolution = int(resolution)
        self.n_channels = int(n_channels)          # capacity of the render target
        self.active_channels = int(n_channels)     # layout of the image currently held (2 or 4)
        self.device_id = int(device_id)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.tsp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- data -----------------------------------------------------------------------------
    def set_kernel_mips(self, mips, n0=64, n_levels=4):
        mips = _f32(mips, name="kernel mips")
        _check(self._lib.tsp_set_kernel_mips(self._h, _ptr(mips), n0, n_levels))

    def upload_particles(self, x, y, z, h, mass=None):
        n = len(x)
        arrs = [_f32(a, n, nm) for a, nm in ((x, "x"), (y, "y"), (z, "z"), (h, "h"))]
        m = None if mass is None else _f32(mass, n, "mass")
        _check(self._lib.tsp_upload_particles(self._h, n, *[_ptr(a) for a in arrs], _ptr(m)))

    def upload_quantity(self, q):
        q = None if q is None else _f32(q, self.num_particles, "quantity")
        _check(self._lib.tsp_upload_quantity(self._h, _ptr(q)))

    def upload_rgb(self, r, g, b):
        n = self.num_particles
        r, g, b = _f32(r, n, "r"), _f32(g, n, "g"), _f32(b, n, "b")
        _check(self._lib.tsp_upload_rgb(self._h, _ptr(r), _ptr(g), _ptr(b)))

    def upload_velocities(self, vx, vy=None, vz=None):
        """The resident velocities of MODE_KINEMATIC (tsp_upload_velocities): three float32 arrays in the caller's order, or
        upload_velocities(None), which frees them."""
        if vx is None and vy is None and vz is None:
            _check(self._lib.tsp_upload_velocities(self._h, None, None, None))
            return
        n = self.num_particles
        v = [None if a is None else _f32(a, n, name) for a, name in ((vx, "vx"), (vy, "vy"), (vz, "vz"))]
        _check(self._lib.tsp_upload_velocities(self._h, *[_ptr(a) for a in v]))

    def set_line_of_sight(self, axis, v_ref=(0.0, 0.0, 0.0)):
        """The unit axis the next MODE_KINEMATIC blocks take the velocities along, and the velocity subtracted first
        (tsp_set_line_of_sight); both are rounded to float32 here."""
        axis, v_ref = _f32(axis, 3, "axis"), _f32(v_ref, 3, "v_ref")
        _check(self._lib.tsp_set_line_of_sight(self._h, _ptr(axis), _ptr(v_ref)))

    def velocity_moments(self):
        """(R, R, 4) float32 (S, mean, sigma, n) of the kinematic image (tsp_velocity_moments): the surface-density sum, the
        mass-weighted mean line-of-sight velocity, its dispersion (NaN where S is not > 0) and the fragment count."""
        out = np.empty((self.resolution, self.resolution, 4), dtype=np.float32)
        _check(self._lib.tsp_velocity_moments(self._h, _ptr(out)))
        return out

    def spectral_cube(self, matrix, scale_factor, v_min, dv, n_channels, sigma_v=0.0, sigma=None):
        """(n_channels, R, R) float32: the position-position-velocity cube of every resident particle at the camera (matrix,
        scale_factor) along the line of sight set last (tsp_spectral_cube): channel c spans v_min + c * dv .. v_min + (c + 1) * dv;
        a particle's line is a Gaussian of width sqrt(sigma_v^2 + sigma[i]^2) integrated over each channel (sigma: per particle,
        the caller's order, or None)."""
        M = _f32(np.asarray(matrix, dtype=np.float32).reshape(16), 16, "matrix")
        s = None if sigma is None else _f32(sigma, self.num_particles, "sigma")
        shape = (int(n_channels), self.resolution, self.resolution)
        allowed = 0 < shape[0] <= CUBE_MAX_CHANNELS and shape[0] * shape[1] * shape[2] <= CUBE_MAX_CELLS
        out = np.empty(shape if allowed else (1,), dtype=np.float32)       # (the library refuses the others: TSP_EINVAL)
        _check(self._lib.tsp_spectral_cube(self._h, _ptr(M), float(scale_factor), float(v_min), float(dv), int(n_channels),
                                           float(np.float32(sigma_v)), _ptr(s), _ptr(out)))
        return out

    def histogram_2d(self, x, y, w=None, v=None, edges_x=(0.0, 1.0), edges_y=(0.0, 1.0), want_bins=False):
        """The weighted 2-D histogram of the caller-ordered float32 arrays (tsp_histogram_2d): column i holds
        edges_x[i] <= x < edges_x[i + 1], row j likewise from edges_y (the last edge is outside).  Returns a dict: "count"
        (ny, nx) int64, "sums" (1 or, with v, 3 planes of (ny, nx)) float64 -- sum w, sum w v, sum (w v) v; w None: weights of 1 --,
        "n_valid", "n_binned" and, with want_bins, "bin_index" (n int32: the cell j * nx + i of every particle, or -1)."""
        n = len(x)
        x, y = _f32(x, n, "x"), _f32(y, n, "y")
        w = None if w is None else _f32(w, n, "w")
        v = None if v is None else _f32(v, n, "v")
        ex, ey = (np.ascontiguousarray(e, dtype=np.float64).ravel() for e in (edges_x, edges_y))
        nx, ny = len(ex) - 1, len(ey) - 1
        allowed = 1 <= nx <= HIST2D_MAX_BINS and 1 <= ny <= HIST2D_MAX_BINS
        shape = (ny, nx) if allowed else (1, 1)                 # (the library refuses the others: TSP_EINVAL)
        dp = ctypes.POINTER(ctypes.c_double)
        spec = Hist2dSpec(nx, ny, ex.ctypes.data_as(dp), ey.ctypes.data_as(dp))
        count = np.empty(shape, dtype=np.int64)
        sums = np.empty((1 if v is None else 3,) + shape, dtype=np.float64)
        bins = np.empty(n, dtype=np.int32) if want_bins else None
        info = Hist2dInfo()
        _check(self._lib.tsp_histogram_2d(self._h, n, _ptr(x), _ptr(y), _ptr(w), _ptr(v), ctypes.byref(spec),
                                          count.ctypes.data_as(_i64p), sums.ctypes.data_as(dp),
                                          None if bins is None else bins.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                          ctypes.byref(info)))
        out = {"count": count, "sums": sums, "n_valid": int(info.n_valid), "n_binned": int(info.n_binned)}
        if want_bins:
            out["bin_index"] = bins
        return out

    def colormap_moment(self, which, lut_rgba, vmin, vmax, log=False):
        """(R, R, 4) uint8: the scalar map of moment `which` (1: mean, 2: sigma) of the kinematic image (tsp_colormap_moment)."""
        lut = _f32(lut_rgba, name="lut")
        out = np.empty((self.resolution, self.resolution, 4), dtype=np.uint8)
        _check(self._lib.tsp_colormap_moment(self._h, int(which), _ptr(lut), lut.size // 4, float(vmin), float(vmax), int(bool(log)),
                                             out.ctypes.data_as(_u8p)))
        return out

    def upload_band_magnitudes(self, mags, weights):
        """rgb channels from SSP band magnitudes on the device: channel_c = sum_b weights[c, b] * 10^(-0.4 * mags[b]).
        mags: (n_bands, n) float64; weights: (3, n_bands) float64 (reference loader.py:112-121: diag(0.5, 1, 1) over I, V, U)."""
        mags = np.ascontiguousarray(mags, dtype=np.float64)
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        if mags.ndim != 2 or mags.shape[1] != self.num_particles or weights.shape != (3, mags.shape[0]):
            raise ValueError("mags must be (n_bands, n_particles) and weights (3, n_bands)")
        dp = ctypes.POINTER(ctypes.c_double)
        _check(self._lib.tsp_upload_band_magnitudes(self._h, mags.shape[0], mags.ctypes.data_as(dp), weights.ctypes.data_as(dp)))

    def generate_synthetic(self, n_total, first=0, count=None, seed=1337, h_cap=0.0, with_quantity=False,
                           with_rgb=False):
        count = n_total - first if count is None else count
        _check(self._lib.tsp_generate_synthetic(self._h, n_total, first, count, seed, h_cap, int(with_quantity),
                                                int(with_rgb)))

    def reorder_spatial(self, n_strata=1, seed=1337, want_permutation=False):
        perm = np.empty(self.num_particles, dtype=np.int64) if want_permutation else None
        _check(self._lib.tsp_reorder_spatial(self._h, n_strata, seed,
                                             None if perm is None else perm.ctypes.data_as(_i64p)))
        return perm

    def strata_offsets(self):
        """First index of every stratum of the last reorder_spatial call, then n (empty if never reordered)."""
        buf = np.empty(4098, dtype=np.int64)
        k = int(self._lib.tsp_get_strata_offsets(self._h, buf.ctypes.data_as(_i64p), len(buf)))
        return buf[:k].copy()

    def cell_layout(self):
        """Cells of the library's load-time ordering (tsp_get_cell_layout / tsp_get_cell_offsets) or None when the
        particles were never reordered: dict(n_strata, cells_per_axis, box_lo (3,), cell_width (3,), offsets (n_strata *
        cells_per_axis^3 + 1,))."""
        ns, ca = ctypes.c_int(0), ctypes.c_int(0)
        lo, width = np.zeros(3, dtype=np.float32), np.zeros(3, dtype=np.float32)
        if self._lib.tsp_get_cell_layout(self._h, ctypes.byref(ns), ctypes.byref(ca), _ptr(lo), _ptr(width)) < 0:
            return None
        buf = np.empty(ns.value * ca.value ** 3 + 1, dtype=np.int64)
        k = int(self._lib.tsp_get_cell_offsets(self._h, buf.ctypes.data_as(_i64p), len(buf)))
        if k != len(buf):
            raise BackendError("tsp_get_cell_offsets returned an unexpected number of values")
        return {"n_strata": ns.value, "cells_per_axis": ca.value, "box_lo": lo.astype(np.float64),
                "cell_width": width.astype(np.float64), "offsets": buf}

    def cell_layouts(self):
        """[cell_layout()] or [] -- the list form that a multi-GPU context fills with one entry per shard."""
        lay = self.cell_layout()
        return [] if lay is None else [lay]

    def download_particles(self, names=("x", "y", "z", "h", "mass")):
        order = ("x", "y", "z", "h", "mass", "q", "r", "g", "b")
        n = self.num_particles
        out = {k: np.empty(n, dtype=np.float32) for k in names}
        _check(self._lib.tsp_download_particles(self._h, *[_ptr(out.get(k)) for k in order]))
        return out

    def project_perspective(self, dst, rot, offset, distance, near):
        """Write the perspective-transformed snapshot of this context's particles into the Context `dst`, which holds the same
        snapshot in the same resident order (tsp_project_perspective): view = rot @ (position + offset), a particle at
        d = distance - view z is scaled by s = distance / d about the optical axis (h by s, mass and rgb by s^2) and dropped (NaN
        position) when d < near; dst's vertex weights and chunk bounds are written by the same pass.  dst then renders with the
        identity rotation and no offset.  rot (3, 3), offset (3,), distance and near are rounded to float32 here."""
        if not isinstance(dst, Context):
            raise ValueError(f"dst must be a Context, not {type(dst).__name__}")
        cam = perspective_struct(rot, offset, distance, near)
        _check(self._lib.tsp_project_perspective(self._h, dst._h, ctypes.byref(cam)))

    @property
    def num_particles(self):
        return int(self._lib.tsp_num_particles(self._h))

    # ---- render ---------------------------------------------------------------------------
    def render(self, matrix, scale_factor, starts=None, lens=None, clear=True, mode=MODE_WEIGHTED, flags=PIPE_DEFAULT):
        """One synchronous render block; returns GPU milliseconds (hipEvent pair)."""
        M = _f32(np.asarray(matrix, dtype=np.float32).reshape(16), 16, "matrix")
        ms = ctypes.c_double(0.0)
        sp, lp, nr, _keep = _ranges(starts, lens)
        _check(self._lib.tsp_render(self._h, _ptr(M), float(scale_factor), sp, lp, nr, int(bool(clear)), int(mode),
                                    int(flags), ctypes.byref(ms)))
        self.active_channels = 4 if mode in (MODE_RGB, MODE_KINEMATIC) else 2
        return ms.value

    def render_undo(self):
        """Take the last render() back (tsp_render_undo): what a driver of several contexts calls on every member when a block
        failed on one of them.  The caller restores `active_channels` (the library's layout is the one before that render)."""
        _check(self._lib.tsp_render_undo(self._h))

    def read_image(self):
        out = np.empty((self.resolution, self.resolution, self.active_channels), dtype=np.float32)
        _check(self._lib.tsp_read_image(self._h, _ptr(out)))
        return out

    def write_image(self, img):
        """Overwrite the render target; the last axis (2 or 4) selects the active layout."""
        img = np.ascontiguousarray(img, dtype=np.float32)
        if img.shape[:2] != (self.resolution, self.resolution) or img.shape[2] not in (2, 4) or img.shape[2] > self.n_channels:
            raise ValueError(f"image shape {img.shape} does not fit the render target")
        self.set_option("active_channels", img.shape[2])
        self.active_channels = img.shape[2]
        _check(self._lib.tsp_write_image(self._h, _ptr(img)))

    def tile_periodic(self, offsets_xy, weights):
        """Replace the render target by the weighted sum of shifted copies of itself (clip-space offsets)."""
        off = _f32(offsets_xy, name="offsets")
        w = _f32(weights, name="weights")
        if off.size != 2 * w.size:
            raise ValueError("offsets must have shape (n, 2) for n weights")
        _check(self._lib.tsp_tile_periodic(self._h, w.size, _ptr(off), _ptr(w)))

    def smoothing_lengths(self, x, y, z, n_neighbours=32, period=None):
        """SPH smoothing lengths of caller-ordered float32 positions (tsp_smoothing_lengths): half the distance to the
        n_neighbours-th nearest particle, the particle itself included; NaN where a coordinate is not finite.  period: the
        side of a periodic box (None or 0: open).  Uses this context's device only; what is resident stays as it is."""
        n = len(x)
        x, y, z = _f32(x, n, "x"), _f32(y, n, "y"), _f32(z, n, "z")
        out = np.empty(n, dtype=np.float32)
        _check(self._lib.tsp_smoothing_lengths(self._h, n, _ptr(x), _ptr(y), _ptr(z), int(n_neighbours),
                                               float(np.float32(period or 0.0)), _ptr(out)))
        return out

    def sph_sum(self, x, y, z, h, a, period=None):
        """Gather-form SPH sum at caller-ordered float32 particles (tsp_sph_sum): sum_j a[j] W(|r_i - r_j|, h[i]) with the M4
        spline of support 2 h[i]; a = mass gives the density.  NaN where a coordinate is not finite or h is not finite and > 0.
        period: the side of a periodic box (None or 0: open).  Uses this context's device only; what is resident stays."""
        n = len(x)
        x, y, z, h, a = _f32(x, n, "x"), _f32(y, n, "y"), _f32(z, n, "z"), _f32(h, n, "h"), _f32(a, n, "a")
        out = np.empty(n, dtype=np.float32)
        _check(self._lib.tsp_sph_sum(self._h, n, _ptr(x), _ptr(y), _ptr(z), _ptr(h), _ptr(a), float(np.float32(period or 0.0)),
                                     _ptr(out)))
        return out

    def sph_velocity_gradient(self, x, y, z, h, mass, rho, vx, vy, vz, period=None):
        """Divergence and curl of the velocity at caller-ordered float32 particles by SPH gather sums
        (tsp_sph_velocity_gradient): (1 / rho_i) sum_j m_j (v_j - v_i) . grad_i W(r_ij, h_i) and the like cross product, with the
        M4 spline of support 2 h[i] -- pynbody's 'v_div' and 'v_curl'.  Returns (div (n,), curl (n, 3)) float32; NaN where a
        coordinate is not finite or h is not finite and > 0.  period: the side of a periodic box (None or 0: open).  Uses this
        context's device only; what is resident stays."""
        n = len(x)
        arrs = [_f32(a, n, name) for a, name in ((x, "x"), (y, "y"), (z, "z"), (h, "h"), (mass, "mass"), (rho, "rho"), (vx, "vx"),
                                                 (vy, "vy"), (vz, "vz"))]
        div = np.empty(n, dtype=np.float32)
        planes = np.empty((3, n), dtype=np.float32)
        _check(self._lib.tsp_sph_velocity_gradient(self._h, n, *[_ptr(a) for a in arrs], float(np.float32(period or 0.0)),
                                                   _ptr(div), _ptr(planes[0]), _ptr(planes[1]), _ptr(planes[2])))
        return div, np.ascontiguousarray(planes.T)

    def sph_sample_lattice(self, x, y, z, fields, k=32, period=None, origin=(0, 0, 0), du=(1, 0, 0), dv=(0, 1, 0), dw=(0, 0, 1),
                           shape=(1, 1, 1)):
        """SPH sums of 1 to 4 caller-ordered float32 per-particle `fields` at the points origin + i du + j dv + k dw of a
        lattice of shape = (nu, nv, nw) points (tsp_sph_sample_lattice): at every point the smoothing length h is half the
        distance to the k-th nearest particle and field f is sum_j fields[f][j] W(|r - r_j|, h) with the M4 spline of support
        2 h; fields = [mass] gives the density, [mass * q, mass] the two sums whose ratio is the kernel-weighted mean of q.
        Returns (h (nw, nv, nu), outs (len(fields), nw, nv, nu)) float32; the fields are NaN where h is 0 or not finite.
        period: the side of a periodic box (None or 0: open).  Uses this context's device only; what is resident stays."""
        n = len(x)
        x, y, z = _f32(x, n, "x"), _f32(y, n, "y"), _f32(z, n, "z")
        fields = [_f32(a, n, f"fields[{f}]") for f, a in enumerate(fields)]
        if not 1 <= len(fields) <= LATTICE_MAX_FIELDS:
            raise ValueError(f"1 to {LATTICE_MAX_FIELDS} fields per call, not {len(fields)}")
        lat = lattice_struct(origin, du, dv, dw, shape)
        nu, nv, nw = lat.nu, lat.nv, lat.nw
        h = np.empty((nw, nv, nu), dtype=np.float32)
        outs = np.empty((len(fields), nw, nv, nu), dtype=np.float32)
        field_ptrs = (_fp * len(fields))(*[_ptr(a) for a in fields])
        out_ptrs = (_fp * len(fields))(*[_ptr(outs[f]) for f in range(len(fields))])
        _check(self._lib.tsp_sph_sample_lattice(self._h, n, _ptr(x), _ptr(y), _ptr(z), len(fields), field_ptrs, int(k),
                                                float(np.float32(period or 0.0)), ctypes.byref(lat), _ptr(h), out_ptrs))
        return h, outs

    def shrink_sphere_center(self, x, y, z, mass, mass_cut_factor=0.0, r_start=0.0, shrink_factor=0.7, min_particles=100,
                             max_iterations=256):
        """Shrinking-sphere centre of caller-ordered float32 particles (tsp_shrink_sphere_center): from the centre of mass, the
        mass-weighted mean of the particles inside a sphere whose radius shrinks by shrink_factor per step, until fewer than
        min_particles are inside.  mass_cut_factor > 1 keeps the particles lighter than that many times the smallest mass;
        r_start = 0 starts from half the x extent.  Returns (center float64 (3,), dict(n_valid, n_inside, iterations, radius,
        mass_inside)).  Uses this context's device only; what is resident stays."""
        n = len(x)
        x, y, z, mass = _f32(x, n, "x"), _f32(y, n, "y"), _f32(z, n, "z"), _f32(mass, n, "mass")
        center = np.empty(3, dtype=np.float64)
        info = CenterInfo()
        _check(self._lib.tsp_shrink_sphere_center(self._h, n, _ptr(x), _ptr(y), _ptr(z), _ptr(mass), float(np.float32(mass_cut_factor)),
                                                  float(r_start), float(shrink_factor), int(min_particles), int(max_iterations),
                                                  center.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(info)))
        return center, {"n_valid": int(info.n_valid), "n_inside": int(info.n_inside), "iterations": int(info.iterations),
                        "radius": float(info.radius), "mass_inside": float(info.mass_inside)}

    def fof_groups(self, x, y, z, linking_length, period=0.0, min_members=20):
        """Friends-of-friends groups of caller-ordered float32 positions (tsp_fof_groups): particles closer than linking_length
        (nearest image in a periodic box of side `period`; None or 0: open) are friends, the groups are the connected
        components.  Returns (int32 (n,) labels, dict(n_valid, n_groups, n_grouped, largest)): label N >= 1 is the N-th largest
        group with at least min_members members, 0 a smaller one, -1 a particle with a non-finite coordinate.  Uses this
        context's device only; what is resident stays."""
        n = len(x)
        x, y, z = _f32(x, n, "x"), _f32(y, n, "y"), _f32(z, n, "z")
        out = np.empty(n, dtype=np.int32)
        info = FofInfo()
        _check(self._lib.tsp_fof_groups(self._h, n, _ptr(x), _ptr(y), _ptr(z), float(np.float32(linking_length)),
                                        float(np.float32(period or 0.0)), int(min_members),
                                        out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(info)))
        return out, {"n_valid": int(info.n_valid), "n_groups": int(info.n_groups), "n_grouped": int(info.n_grouped),
                     "largest": int(info.largest)}

    def sphere_moments(self, x, y, z, mass, vel=None, center=(0.0, 0.0, 0.0), r=1.0, r_vel=0.0):
        """Moments of the caller-ordered float32 particles inside the sphere of radius r around center (tsp_sphere_moments):
        mass, com (the offset of the centre of mass from center), the second moments S (xx, xy, xz, yy, yz, zz) and, with
        vel = (vx, vy, vz), the mean velocity v_cen of the sphere of radius r_vel, the angular momentum L about it and its
        scale A.  Returns a dict of the fields of struct tsp_moments (counts int, sums float, vectors float64 arrays).  Uses this
        context's device only; what is resident stays."""
        n = len(x)
        x, y, z, mass = _f32(x, n, "x"), _f32(y, n, "y"), _f32(z, n, "z"), _f32(mass, n, "mass")
        if vel is not None:
            if len(vel) != 3:
                raise ValueError("vel must be the three arrays (vx, vy, vz)")
            vel = [_f32(v, n, name) for v, name in zip(vel, ("vx", "vy", "vz"))]
        vx, vy, vz = vel if vel is not None else (None, None, None)
        center = np.ascontiguousarray(center, dtype=np.float64)
        if center.shape != (3,):
            raise ValueError(f"center must be three coordinates, not shape {center.shape}")
        out = Moments()
        _check(self._lib.tsp_sphere_moments(self._h, n, _ptr(x), _ptr(y), _ptr(z), _ptr(mass), _ptr(vx), _ptr(vy), _ptr(vz),
                                            center.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), float(r), float(r_vel),
                                            ctypes.byref(out)))
        return out.as_dict()

    def radial_profile(self, x, y, z, mass, vel=None, edges=(0.0, 1.0), geometry=0, center=(0.0, 0.0, 0.0), v_cen=(0.0, 0.0, 0.0),
                       frame=None, half_height=np.inf):
        """Binned sums of the caller-ordered float32 particles (tsp_radial_profile) in the spherical shells (geometry 0) or the
        cylindrical annuli about the third axis of `frame` with |z'| <= half_height (geometry 1) between the ascending radii
        `edges` around center; with vel = (vx, vy, vz) the velocity sums are taken about v_cen.  frame=None is the identity.
        Returns a dict: count int64 (n_bins,), sums float64 (n_bins, 11) (mass, ms, mc (3), mc2 (3), mj (3): the header's order),
        n_valid, n_inner, n_binned, mass_inner.  Uses this context's device only; what is resident stays."""
        n = len(x)
        x, y, z, mass = _f32(x, n, "x"), _f32(y, n, "y"), _f32(z, n, "z"), _f32(mass, n, "mass")
        if vel is not None:
            if len(vel) != 3:
                raise ValueError("vel must be the three arrays (vx, vy, vz)")
            vel = [_f32(v, n, name) for v, name in zip(vel, ("vx", "vy", "vz"))]
        vx, vy, vz = vel if vel is not None else (None, None, None)
        edges = np.ascontiguousarray(edges, dtype=np.float64)
        if edges.ndim != 1 or len(edges) < 2:
            raise ValueError(f"edges must be at least two radii, not shape {edges.shape}")
        spec = ProfileSpec()
        spec.geometry, spec.n_bins = int(geometry), len(edges) - 1
        spec.edges = edges.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        for name, value, shape in (("center", center, (3,)), ("v_cen", v_cen, (3,)),
                                   ("frame", np.eye(3) if frame is None else frame, (3, 3))):
            value = np.ascontiguousarray(value, dtype=np.float64)
            if value.shape != shape:
                raise ValueError(f"{name} must have shape {shape}, not {value.shape}")
            getattr(spec, name)[:] = value.ravel().tolist()
        spec.half_height = float(half_height)
        count = np.zeros(spec.n_bins, dtype=np.int64)
        sums = np.zeros((spec.n_bins, PROFILE_SUMS), dtype=np.float64)
        info = ProfileInfo()
        _check(self._lib.tsp_radial_profile(self._h, n, _ptr(x), _ptr(y), _ptr(z), _ptr(mass), _ptr(vx), _ptr(vy), _ptr(vz),
                                            ctypes.byref(spec), count.ctypes.data_as(_i64p),
                                            sums.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(info)))
        return {"count": count, "sums": sums, "n_valid": int(info.n_valid), "n_inner": int(info.n_inner),
                "n_binned": int(info.n_binned), "mass_inner": float(info.mass_inner)}

    def gravity_direct(self, sx, sy, sz, mass, eps, targets=None, want_pot=True, want_acc=True):
        """The softened direct sum (tsp_gravity_direct, G = 1) of the float32 sources at `targets` = (tx, ty, tz), or at the
        sources themselves (None: the pair of a particle with itself is left out).  eps: one softening length for every source or
        an array of them.  Returns (pot float64 (n_tgt,) or None, acc float64 (n_tgt, 3) or None, dict(n_valid_sources,
        n_valid_targets)); NaN at a target with a non-finite coordinate.  The cost is n_src * n_tgt pairs.  Uses this context's
        device only; what is resident stays."""
        return self._gravity(False, sx, sy, sz, mass, eps, targets, 0.0, want_pot, want_acc)

    def gravity_tree(self, sx, sy, sz, mass, eps, targets=None, theta=0.5, want_pot=True, want_acc=True):
        """The same sums by the Barnes-Hut tree over the Morton order of the sources (tsp_gravity_tree, G = 1): arguments and
        results as gravity_direct, with the opening angle theta in [0, 1] (0: nothing is accepted, the direct sum in Morton
        order) and masses >= 0.  The dict holds n_valid_sources, n_valid_targets, n_nodes, n_levels, pairs_direct and pairs_node
        (target-particle and target-node terms evaluated).  Separate targets are walked in groups of 64 in the order given:
        neighbours next to each other prune best."""
        return self._gravity(True, sx, sy, sz, mass, eps, targets, float(theta), want_pot, want_acc)

    def _gravity(self, tree, sx, sy, sz, mass, eps, targets, theta, want_pot, want_acc):
        n = len(sx)
        sx, sy, sz, mass = _f32(sx, n, "sx"), _f32(sy, n, "sy"), _f32(sz, n, "sz"), _f32(mass, n, "mass")
        if np.ndim(eps) == 0:
            eps_array, eps_all = None, float(np.float32(eps))
        else:
            eps_array, eps_all = _f32(eps, n, "eps"), 0.0
        if targets is None:
            n_tgt, (tx, ty, tz) = n, (None, None, None)
        else:
            if len(targets) != 3:
                raise ValueError("targets must be the three arrays (tx, ty, tz)")
            n_tgt = len(targets[0])
            tx, ty, tz = (_f32(t, n_tgt, name) for t, name in zip(targets, ("tx", "ty", "tz")))
        if not (want_pot or want_acc):
            raise ValueError("at least one of want_pot and want_acc must be set")
        pot = np.empty(n_tgt, dtype=np.float64) if want_pot else None
        acc = np.empty((n_tgt, 3), dtype=np.float64) if want_acc else None
        info = GravityTreeInfo() if tree else GravityInfo()
        dp = ctypes.POINTER(ctypes.c_double)
        sources = (self._h, n, _ptr(sx), _ptr(sy), _ptr(sz), _ptr(mass), _ptr(eps_array), eps_all, n_tgt, _ptr(tx), _ptr(ty), _ptr(tz))
        outputs = (None if pot is None else pot.ctypes.data_as(dp), None if acc is None else acc.ctypes.data_as(dp), ctypes.byref(info))
        if tree:
            _check(self._lib.tsp_gravity_tree(*sources, theta, *outputs))
        else:
            _check(self._lib.tsp_gravity_direct(*sources, *outputs))
        return pot, acc, {name: int(getattr(info, name)) for name, _ in info._fields_}

    def group_potential(self, x, y, z, mass, eps, group, n_groups, period=0.0, max_members=0):
        """The self-potential of every halo (tsp_group_potential, G = 1): for particle i with the label group[i] in 1..n_groups,
        the softened sum over the other valid members of its halo, on anchor-relative float32 offsets (nearest image in a box
        of side `period`; None or 0: open).  eps: one softening length or an array.  max_members > 0: haloes with more valid
        members are skipped.  Returns (float64 (n,), NaN for non-members, invalid members and skipped haloes; dict of
        struct tsp_group_potential_info).  Uses this context's device only; what is resident stays."""
        n = len(x)
        x, y, z, mass = _f32(x, n, "x"), _f32(y, n, "y"), _f32(z, n, "z"), _f32(mass, n, "mass")
        if np.ndim(eps) == 0:
            eps_array, eps_all = None, float(np.float32(eps))
        else:
            eps_array, eps_all = _f32(eps, n, "eps"), 0.0
        group = np.ascontiguousarray(group, dtype=np.int32)
        if group.size != n:
            raise ValueError(f"group has {group.size} elements, expected {n}")
        phi = np.empty(n, dtype=np.float64)
        info = GroupPotentialInfo()
        _check(self._lib.tsp_group_potential(self._h, n, _ptr(x), _ptr(y), _ptr(z), _ptr(mass), _ptr(eps_array), eps_all,
                                             group.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(n_groups), float(period or 0.0),
                                             int(max_members), phi.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(info)))
        return phi, {name: (float if kind is ctypes.c_double else int)(getattr(info, name)) for name, kind in info._fields_}

    def halo_properties(self, x, y, z, mass, group, n_groups, vel=None, phi=None, period=0.0):
        """The per-halo reductions of tsp_halo_properties over the labels group[i] in 1..n_groups; vel = (vx, vy, vz) or None,
        phi = float64 (n,) potential or None.  Returns a dict: count, n_bound, i_pot int64 (n_groups,), props float64 (n_groups,
        HALO_NPROPS) (columns: HALO_COLUMNS), n_members, max_extent.  Uses this context's device only; what is resident stays."""
        n = len(x)
        x, y, z, mass = _f32(x, n, "x"), _f32(y, n, "y"), _f32(z, n, "z"), _f32(mass, n, "mass")
        if vel is not None:
            if len(vel) != 3:
                raise ValueError("vel must be the three arrays (vx, vy, vz)")
            vel = [_f32(v, n, name) for v, name in zip(vel, ("vx", "vy", "vz"))]
        vx, vy, vz = vel if vel is not None else (None, None, None)
        if phi is not None:
            phi = np.ascontiguousarray(phi, dtype=np.float64)
            if phi.size != n:
                raise ValueError(f"phi has {phi.size} elements, expected {n}")
        group = np.ascontiguousarray(group, dtype=np.int32)
        if group.size != n:
            raise ValueError(f"group has {group.size} elements, expected {n}")
        n_groups = int(n_groups)
        count, n_bound, i_pot = (np.empty(max(n_groups, 0), dtype=np.int64) for _ in range(3))
        props = np.empty((max(n_groups, 0), HALO_NPROPS), dtype=np.float64)
        info = HaloInfo()
        dp = ctypes.POINTER(ctypes.c_double)
        _check(self._lib.tsp_halo_properties(self._h, n, _ptr(x), _ptr(y), _ptr(z), _ptr(mass), _ptr(vx), _ptr(vy), _ptr(vz),
                                             None if phi is None else phi.ctypes.data_as(dp),
                                             group.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n_groups, float(period or 0.0),
                                             count.ctypes.data_as(_i64p), n_bound.ctypes.data_as(_i64p), i_pot.ctypes.data_as(_i64p),
                                             props.ctypes.data_as(dp), ctypes.byref(info)))
        return {"count": count, "n_bound": n_bound, "i_pot": i_pot, "props": props, "n_members": int(info.n_members),
                "max_extent": float(info.max_extent)}

    # ---- surface (include/topsy_splat.h "Surface rendering") ---------------------------------
    def set_sphere_mips(self, mips, n0=64, n_levels=4):
        mips = _f32(mips, name="sphere mips")
        _check(self._lib.tsp_set_sphere_mips(self._h, _ptr(mips), n0, n_levels))

    def density_order_stats(self, ranks):
        """Values of rho = m / h^3 over the resident particles at the given ascending ranks (numpy's sort order, NaN last)."""
        r = np.ascontiguousarray(ranks, dtype=np.int64)
        out = np.empty(len(r), dtype=np.float32)
        _check(self._lib.tsp_density_order_stats(self._h, r.ctypes.data_as(_i64p), len(r), _ptr(out)))
        return out

    def render_surface(self, matrix, scale_factor, density_cut, starts=None, lens=None, clear=True):
        """The occlusion pass: (q, depth) of the front-most sphere per pixel becomes the 2-channel image; returns GPU ms."""
        M = _f32(np.asarray(matrix, dtype=np.float32).reshape(16), 16, "matrix")
        ms = ctypes.c_double(0.0)
        sp, lp, nr, _keep = _ranges(starts, lens)
        _check(self._lib.tsp_render_surface(self._h, _ptr(M), float(scale_factor), float(np.float32(density_cut)), sp, lp, nr,
                                            int(bool(clear)), ctypes.byref(ms)))
        self.active_channels = 2
        return ms.value

    @staticmethod
    def _surface_params(smoothing_scale=0.01, depth_scale=1.0, light_direction=(0.0, 0.0, 1.0), light_color=(1.0, 1.0, 1.0),
                        ambient_color=(0.2, 0.2, 0.2), vmin=0.0, vmax=1.0, weighted_average=False, log=False, lut_rgba=None):
        """struct tsp_surface_params of a surface presentation, and the LUT array it points into (kept alive by the caller)."""
        p = SurfaceParams()
        p.smoothing_scale = float(smoothing_scale)
        p.depth_scale = float(depth_scale)
        p.light_direction[:] = [float(np.float32(v)) for v in light_direction]
        p.light_color[:] = [float(np.float32(v)) for v in light_color]
        p.ambient_color[:] = [float(np.float32(v)) for v in ambient_color]
        p.vmin, p.vmax = float(np.float32(vmin)), float(np.float32(vmax))
        p.weighted_average, p.log_scale = int(bool(weighted_average)), int(bool(log))
        lut = None
        if weighted_average:
            lut = _f32(lut_rgba, name="lut")
            p.lut_rgba, p.n_lut = _ptr(lut), lut.size // 4
        return p, lut

    def surface_present(self, smoothing_scale=0.01, depth_scale=1.0, light_direction=(0.0, 0.0, 1.0), light_color=(1.0, 1.0, 1.0),
                        ambient_color=(0.2, 0.2, 0.2), vmin=0.0, vmax=1.0, weighted_average=False, log=False, lut_rgba=None,
                        content=True, rgba=True, timings=None):
        """Bilateral filter of the (q, depth) image, then the lit shading.  Returns (content (R, R, 2) float32 or None,
        rgba (R, R, 4) uint8 or None); `timings`, a list, receives [filter ms, shading ms]."""
        p, _lut = self._surface_params(smoothing_scale, depth_scale, light_direction, light_color, ambient_color, vmin, vmax,
                                       weighted_average, log, lut_rgba)
        R = self.resolution
        c = np.empty((R, R, 2), dtype=np.float32) if content else None
        o = np.empty((R, R, 4), dtype=np.uint8) if rgba else None
        ms = (ctypes.c_double * 2)()
        _check(self._lib.tsp_surface_present(self._h, ctypes.byref(p), _ptr(c), None if o is None else o.ctypes.data_as(_u8p), ms))
        if timings is not None:
            timings[:] = [ms[0], ms[1]]
        return c, o

    def present_surface(self, width, height, params=None, layers=(), timings=None):
        """Compose a (height, width, 4) uint8 frame with the lit surface as its base (tsp_present_surface): the (q, depth) image
        filtered, shaded from five samples per canvas pixel, then `layers` in order.  params: a dict of surface_present's
        keywords (smoothing_scale, depth_scale, light_direction, light_color, ambient_color, vmin, vmax, weighted_average, log,
        lut_rgba); layers as present takes them.  `timings`, a list, receives [filter ms, composition ms]."""
        p, _lut = self._surface_params(**(params or {}))
        arr, _keep = self._layer_args(layers)
        return self._compose(self._lib.tsp_present_surface, width, height, p, arr, len(layers), 2, timings)

    def present_surface_yuv420(self, width, height, params=None, layers=(), timings=None):
        """The frame of present_surface(width, height, params, layers) as I420 planes (tsp_present_surface_yuv420): uint8 arrays
        Y (height, width), U and V (height / 2, width / 2); width and height must be even.  `timings`, a list, receives
        [filter ms, composition + conversion ms]."""
        p, _lut = self._surface_params(**(params or {}))
        arr, _keep = self._layer_args(layers)
        return self._compose(self._lib.tsp_present_surface_yuv420, width, height, p, arr, len(layers), 2, timings, yuv420=True)

    def content_sort(self, kind, scale=1.0):
        """Sort the finite content values on the device; returns (n_finite, n_nonpositive)."""
        nf, nnp = ctypes.c_int64(0), ctypes.c_int64(0)
        _check(self._lib.tsp_content_sort(self._h, int(kind), float(np.float32(scale)), ctypes.byref(nf), ctypes.byref(nnp)))
        return nf.value, nnp.value

    def moment_sort(self, which, absolute=False):
        """Sort the finite values of a moment map of the kinematic image (which: 1 mean, 2 sigma; absolute: of its absolute
        value) on the device (tsp_moment_sort); returns n_finite.  content_values then reads the values at ranks below it."""
        nf = ctypes.c_int64(0)
        _check(self._lib.tsp_moment_sort(self._h, int(which), int(bool(absolute)), ctypes.byref(nf)))
        return nf.value

    def content_values(self, ranks):
        r = np.ascontiguousarray(ranks, dtype=np.int64)
        out = np.empty(len(r), dtype=np.float32)
        _check(self._lib.tsp_content_values(self._h, r.ctypes.data_as(_i64p), len(r), _ptr(out)))
        return out

    def content_neg_inf(self):
        """How many content values of the last content_sort were -inf (dropped from the sort, negative to the autorange)."""
        n = ctypes.c_int64(0)
        _check(self._lib.tsp_content_neg_inf(self._h, ctypes.byref(n)))
        return n.value

    def stats(self):
        s = Stats()
        _check(self._lib.tsp_get_stats(self._h, ctypes.byref(s)))
        return s.as_dict()

    def set_option(self, name, value):
        _check(self._lib.tsp_set_option(self._h, name.encode(), int(value)))

    def measure_read_bandwidth(self, nbytes=1 << 30, iters=10):
        g = ctypes.c_double(0.0)
        _check(self._lib.tsp_measure_read_bandwidth(self._h, nbytes, iters, ctypes.byref(g)))
        return g.value

    n_gpus = 1

    def end_frame(self, root=0):
        """Frame boundary of the render loop: nothing to exchange on one GPU (multigpu.MultiGpuContext sums the shards here)."""
        return 0.0

    # ---- colormap -------------------------------------------------------------------------
    def colormap_scalar(self, lut_rgba, vmin, vmax, log, weighted, out=None):
        """-> (R, R, 4) uint8.  `out`: a caller-owned array of that shape to write into (a display loop reuses one: a fresh
        4 MiB numpy array per frame costs its page faults inside the device-to-host copy, ~0.15 ms)."""
        lut = _f32(lut_rgba, name="lut")
        if out is None:
            out = np.empty((self.resolution, self.resolution, 4), dtype=np.uint8)
        elif out.shape != (self.resolution, self.resolution, 4) or out.dtype != np.uint8 or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous (R, R, 4) uint8 array")
        _check(self._lib.tsp_colormap_scalar(self._h, _ptr(lut), lut.size // 4, float(vmin), float(vmax), int(bool(log)),
                                             int(bool(weighted)), out.ctypes.data_as(_u8p)))
        return out

    def colormap_rgb(self, vmin, vmax, gamma, as_float=False):
        shape = (self.resolution, self.resolution, 4)
        if as_float:
            out = np.empty(shape, dtype=np.float32)
            _check(self._lib.tsp_colormap_rgb(self._h, float(vmin), float(vmax), float(gamma), None, _ptr(out)))
        else:
            out = np.empty(shape, dtype=np.uint8)
            _check(self._lib.tsp_colormap_rgb(self._h, float(vmin), float(vmax), float(gamma),
                                              out.ctypes.data_as(_u8p), None))
        return out

    def colormap_set_lut2d(self, lut_rgba):
        lut = np.ascontiguousarray(lut_rgba, dtype=np.float32)
        if lut.ndim != 3 or lut.shape[0] != lut.shape[1] or lut.shape[2] != 4:
            raise ValueError("2-D LUT must have shape (n, n, 4)")
        _check(self._lib.tsp_colormap_set_lut2d(self._h, _ptr(lut), lut.shape[0]))

    def colormap_bivariate(self, vmin, vmax, dvmin, dvmax, log, weighted):
        out = np.empty((self.resolution, self.resolution, 4), dtype=np.uint8)
        _check(self._lib.tsp_colormap_bivariate(self._h, float(vmin), float(vmax), float(dvmin), float(dvmax), int(bool(log)),
                                                int(bool(weighted)), out.ctypes.data_as(_u8p)))
        return out

    def colormap_bivariate_host(self, img, vmin, vmax, dvmin, dvmax, log, weighted):
        img = np.ascontiguousarray(img, dtype=np.float32)
        H, W, C = img.shape
        out = np.empty((H, W, 4), dtype=np.uint8)
        _check(self._lib.tsp_colormap_bivariate_host(self._h, _ptr(img), H, W, C, float(vmin), float(vmax), float(dvmin),
                                                     float(dvmax), int(bool(log)), int(bool(weighted)), out.ctypes.data_as(_u8p)))
        return out

    def colormap_scalar_host(self, img, lut_rgba, vmin, vmax, log, weighted):
        img = np.ascontiguousarray(img, dtype=np.float32)
        H, W, C = img.shape
        lut = _f32(lut_rgba, name="lut")
        out = np.empty((H, W, 4), dtype=np.uint8)
        _check(self._lib.tsp_colormap_scalar_host(self._h, _ptr(img), H, W, C, _ptr(lut), lut.size // 4, float(vmin),
                                                  float(vmax), int(bool(log)), int(bool(weighted)),
                                                  out.ctypes.data_as(_u8p)))
        return out

    def colormap_rgb_host(self, img, vmin, vmax, gamma, as_float=False):
        img = np.ascontiguousarray(img, dtype=np.float32)
        H, W, C = img.shape
        if as_float:
            out = np.empty((H, W, 4), dtype=np.float32)
            _check(self._lib.tsp_colormap_rgb_host(self._h, _ptr(img), H, W, C, float(vmin), float(vmax), float(gamma),
                                                   None, _ptr(out)))
        else:
            out = np.empty((H, W, 4), dtype=np.uint8)
            _check(self._lib.tsp_colormap_rgb_host(self._h, _ptr(img), H, W, C, float(vmin), float(vmax), float(gamma),
                                                   out.ctypes.data_as(_u8p), None))
        return out

    # ---- frame composition ----------------------------------------------------------------
    def present(self, width, height, base, layers=(), timings=None):
        """Compose a (height, width, 4) frame (tsp_present): the presentation image colormapped onto the canvas, then `layers`
        in order.  base: dict with "map" ("scalar" | "bivariate" | "rgb" | "rgb-hdr" | "moment-mean" | "moment-sigma", the last two
        the maps of a kinematic image), "vmin", "vmax" and as the map needs "lut" (scalar, moments: (n, 4) float32), "log",
        "weighted", "density_vmin", "density_vmax" (bivariate, after colormap_set_lut2d), "gamma" (rgb).  A layer is a dict with "kind" "quad" (texture (th, tw, 4) float32, clip (x0, y0, w, h), tex (u0, v0, du,
        dv), offsets (n, 2), weights (n,)) or "lines" (starts / ends (n, 4), transform (4, 4) row-major, color (4,), width).
        Returns uint8, or float16 for "rgb-hdr".  `timings`, a list, receives the composition kernel's GPU ms."""
        b, arr, keep = self._present_args(base, layers)
        return self._compose(self._lib.tsp_present, width, height, b, arr, len(layers), 1, timings,
                             dtype=np.float16 if b.map == PRESENT_RGB_HDR else np.uint8)

    def present_yuv420(self, width, height, base, layers=(), timings=None):
        """The frame of present(width, height, base, layers) as I420 planes (tsp_present_yuv420): uint8 arrays Y (height,
        width), U and V (height / 2, width / 2).  width and height must be even; the "rgb-hdr" map has no 8-bit frame.
        `timings`, a list, receives the GPU ms of the composition and the conversion together."""
        b, arr, keep = self._present_args(base, layers)
        return self._compose(self._lib.tsp_present_yuv420, width, height, b, arr, len(layers), 1, timings, yuv420=True)

    def _compose(self, entry, width, height, head, layer_array, n_layers, n_ms, timings, yuv420=False, dtype=np.uint8):
        """One call of a composition entry point (entry: the library function; head: its base or surface struct): the output sized
        for the (height, width, 4) frame of `dtype`, or (yuv420) for its I420 planes, which come back as the views Y, U, V; the
        n_ms GPU times the entry point reports go to `timings`."""
        W, H = int(width), int(height)
        n, c = max(W, 0) * max(H, 0), (max(W, 0) // 2) * (max(H, 0) // 2)
        out = np.empty(n + 2 * c, dtype=np.uint8) if yuv420 else np.empty((max(H, 0), max(W, 0), 4), dtype=dtype)
        ms = (ctypes.c_double * n_ms)()
        _check(entry(self._h, W, H, ctypes.byref(head), layer_array, n_layers, out.ctypes.data_as(entry.argtypes[6]), ms))
        if timings is not None:
            timings[:] = list(ms)
        if not yuv420:
            return out
        return out[:n].reshape(H, W), out[n:n + c].reshape(H // 2, W // 2), out[n + c:].reshape(H // 2, W // 2)

    @staticmethod
    def _present_args(base, layers):
        """The ctypes structs of tsp_present's base and layers, and the arrays they point into (kept alive by the caller)."""
        maps = {"scalar": PRESENT_SCALAR, "bivariate": PRESENT_BIVARIATE, "rgb": PRESENT_RGB, "rgb-hdr": PRESENT_RGB_HDR,
                "moment-mean": PRESENT_MOMENT_MEAN, "moment-sigma": PRESENT_MOMENT_SIGMA}
        b = PresentBase()
        b.map = maps[base["map"]]
        b.vmin, b.vmax = float(np.float32(base["vmin"])), float(np.float32(base["vmax"]))
        b.density_vmin = float(np.float32(base.get("density_vmin", 0.0)))
        b.density_vmax = float(np.float32(base.get("density_vmax", 1.0)))
        b.gamma = float(np.float32(base.get("gamma", 1.0)))
        b.log_scale, b.weighted = int(bool(base.get("log", False))), int(bool(base.get("weighted", False)))
        keep = []             # the arrays the structs point into stay alive for the call
        if b.map in (PRESENT_SCALAR, PRESENT_MOMENT_MEAN, PRESENT_MOMENT_SIGMA):
            lut = _f32(base["lut"], name="lut")
            keep.append(lut)
            b.lut_rgba, b.n_lut = _ptr(lut), lut.size // 4
        arr, layer_keep = Context._layer_args(layers)
        return b, arr, keep + layer_keep

    @staticmethod
    def _layer_args(layers):
        """The tsp_present_layer array of `layers`, and the arrays it points into (kept alive by the caller)."""
        keep = []
        arr = (PresentLayer * max(1, len(layers)))()
        for L, d in zip(arr, layers):
            if d["kind"] == "quad":
                tex = _f32(d["texture"], name="texture")
                if tex.ndim != 3 or tex.shape[2] != 4:
                    raise ValueError(f"a quad texture must have shape (h, w, 4), not {tex.shape}")
                off = _f32(d.get("offsets", [[0.0, 0.0]]), name="offsets").reshape(-1)
                w = _f32(d.get("weights", [1.0]), name="weights").reshape(-1)
                if off.size != 2 * w.size:
                    raise ValueError("offsets must have shape (n, 2) for n weights")
                keep += [tex, off, w]
                L.kind = LAYER_QUAD
                L.texture_rgba, L.tex_height, L.tex_width = _ptr(tex), tex.shape[0], tex.shape[1]
                x0, y0, cw, ch = (float(np.float32(v)) for v in d["clip"])
                u0, v0, du, dv = (float(np.float32(v)) for v in d.get("tex", (0.0, 0.0, 1.0, 1.0)))
                L.clip_origin[:], L.clip_extent[:], L.tex_origin[:], L.tex_extent[:] = [x0, y0], [cw, ch], [u0, v0], [du, dv]
                L.n_instances, L.instance_offsets, L.instance_weights = w.size, _ptr(off), _ptr(w)
            elif d["kind"] == "lines":
                st = _f32(d["starts"], name="starts").reshape(-1)
                en = _f32(d["ends"], name="ends").reshape(-1)
                if st.size != en.size or st.size % 4:
                    raise ValueError("starts and ends must both have shape (n, 4)")
                keep += [st, en]
                L.kind = LAYER_LINES
                L.n_segments, L.starts, L.ends = st.size // 4, _ptr(st), _ptr(en)
                L.transform[:] = [float(v) for v in _f32(d.get("transform", np.eye(4)), 16, "transform").reshape(16)]
                L.color[:] = [float(v) for v in _f32(d["color"], 4, "color")]
                L.width_px = float(np.float32(d["width"]))
            else:
                raise ValueError(f"unknown layer kind {d['kind']!r}")
        return arr, keep

    # ---- multi-GPU ------------------------------------------------------------------------
    @staticmethod
    def comm_unique_id():
        buf = ctypes.create_string_buffer(UNIQUE_ID_BYTES)
        _check(load_library().tsp_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, n_ranks, rank, unique_id):
        if len(unique_id) != UNIQUE_ID_BYTES:
            raise ValueError("unique id must be 128 bytes")
        _check(self._lib.tsp_comm_init(self._h, n_ranks, rank, unique_id))

    def comm_destroy(self):
        if getattr(self, "_h", None):
            _check(self._lib.tsp_comm_destroy(self._h))

    def set_reduced_image(self, total):
        """Hand over a sum the caller formed (host collective): presentation image only, the accumulator stays this shard's."""
        total = np.ascontiguousarray(total, dtype=np.float32)
        if total.shape != (self.resolution, self.resolution, self.active_channels):
            raise ValueError(f"image shape {total.shape} does not fit the render target")
        _check(self._lib.tsp_set_reduced_image(self._h, _ptr(total)))

    def comm_reduce_image(self, root=0):
        ms = ctypes.c_double(0.0)
        _check(self._lib.tsp_comm_reduce_image(self._h, root, ctypes.byref(ms)))
        return ms.value


class Group:
    """ctypes view of the C-level device group (tsp_group_*, include/topsy_splat.h): what a C client uses to put several
    GPUs behind one handle.  The product's own multi-GPU driver is multigpu.MultiGpuContext; this class exists so that the
    tests exercise the C entry points.  `root` is a borrowed Context over tsp_group_context(group, 0)."""

    def __init__(self, resolution, n_channels, device_ids):
        self._lib = load_library()
        ids = (ctypes.c_int * len(device_ids))(*[int(d) for d in device_ids])
        h = _ctx()
        _check(self._lib.tsp_group_create(len(device_ids), ids, int(resolution), int(n_channels), ctypes.byref(h)))
        self._g = h
        self.resolution, self.n_channels = int(resolution), int(n_channels)
        self.root = self.member(0)

    def member(self, index):
        h = self._lib.tsp_group_context(self._g, int(index))
        if not h:
            raise IndexError(index)
        c = Context.__new__(Context)
        c._lib = self._lib
        c._h = _ctx(h)
        c.close = lambda: None           # borrowed: the group destroys its contexts
        c.resolution, c.n_channels, c.device_id, c.active_channels = self.resolution, self.n_channels, -1, 2
        return c

    def close(self):
        if getattr(self, "_g", None):
            self.root._h = None
            self._lib.tsp_group_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def size(self):
        return self._lib.tsp_group_size(self._g)

    @property
    def uses_rccl(self):
        return bool(self._lib.tsp_group_uses_rccl(self._g))

    @property
    def num_particles(self):
        return self._lib.tsp_group_num_particles(self._g)

    def set_kernel_mips(self, mips, n0=64, n_levels=4):
        m = _f32(mips, None, "mips")
        _check(self._lib.tsp_group_set_kernel_mips(self._g, _ptr(m), n0, n_levels))

    def upload_particles(self, x, y, z, h, mass=None):
        n = len(x)
        arrs = [_f32(a, n, nm) for a, nm in ((x, "x"), (y, "y"), (z, "z"), (h, "h"))]
        m = None if mass is None else _f32(mass, n, "mass")
        _check(self._lib.tsp_group_upload_particles(self._g, n, *[_ptr(a) for a in arrs], None if m is None else _ptr(m)))

    def upload_quantity(self, q):
        qa = None if q is None else _f32(q, self.num_particles, "q")
        _check(self._lib.tsp_group_upload_quantity(self._g, None if qa is None else _ptr(qa)))

    def upload_rgb(self, r, g, b):
        n = self.num_particles
        arrs = [_f32(a, n, nm) for a, nm in ((r, "r"), (g, "g"), (b, "b"))]
        _check(self._lib.tsp_group_upload_rgb(self._g, *[_ptr(a) for a in arrs]))

    def upload_band_magnitudes(self, mags, weights):
        mags = np.ascontiguousarray(mags, dtype=np.float64)
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        if mags.ndim != 2 or mags.shape[1] != self.num_particles or weights.shape != (3, mags.shape[0]):
            raise ValueError("mags must be (n_bands, N) and weights (3, n_bands)")
        dp = ctypes.POINTER(ctypes.c_double)
        _check(self._lib.tsp_group_upload_band_magnitudes(self._g, mags.shape[0], mags.ctypes.data_as(dp), weights.ctypes.data_as(dp)))

    def shard_range(self, index):
        first, count = ctypes.c_int64(0), ctypes.c_int64(0)
        _check(self._lib.tsp_group_shard_range(self._g, int(index), ctypes.byref(first), ctypes.byref(count)))
        return first.value, count.value

    def generate_synthetic(self, n_total, first=0, count=None, seed=1337, h_cap=0.0, with_quantity=False, with_rgb=False):
        count = n_total - first if count is None else count
        _check(self._lib.tsp_group_generate_synthetic(self._g, int(n_total), int(first), int(count), int(seed), float(h_cap),
                                                      int(with_quantity), int(with_rgb)))

    def reorder_spatial(self, n_strata=1, seed=1337):
        _check(self._lib.tsp_group_reorder_spatial(self._g, int(n_strata), int(seed)))

    def set_option(self, name, value):
        _check(self._lib.tsp_group_set_option(self._g, name.encode(), int(value)))

    def render(self, matrix, scale_factor, starts=None, lens=None, clear=True, mode=MODE_WEIGHTED, flags=PIPE_DEFAULT):
        M = _f32(np.asarray(matrix, dtype=np.float32).reshape(16), 16, "matrix")
        ms = ctypes.c_double(0.0)
        sp, lp, nr, _keep = _ranges(starts, lens)
        _check(self._lib.tsp_group_render(self._g, _ptr(M), float(scale_factor), sp, lp, nr, int(bool(clear)), int(mode), int(flags),
                                          ctypes.byref(ms)))
        self.root.active_channels = 4 if mode == MODE_RGB else 2
        return ms.value

    def end_frame(self):
        ms = ctypes.c_double(0.0)
        _check(self._lib.tsp_group_end_frame(self._g, ctypes.byref(ms)))
        return ms.value

    def stats(self):
        st = Stats()
        _check(self._lib.tsp_group_get_stats(self._g, ctypes.byref(st)))
        return st.as_dict()
