"""Failed per-call scratch allocations leave the caller's outputs and the context as they were.

Every entry point outside tsp_render and the post-passes takes its device memory per call, through scratch_alloc()
(topsy_amd/csrc/tsp_internal.h), which counts against option debug_fail_alloc like alloc_group().  Each test below walks
k = 1, 2, ... over the allocations of one entry point (or one variant of it) on one context: the k-th allocation fails, the raw
ctypes call must return TSP_ENOMEM (-6) with the site's name in tsp_last_error, every output buffer and info struct must still hold
the sentinel bytes it was filled with, and the image, the counts and the resident particles of the context must be what they were
before the call.  At the k where nothing is left to fail the result is held to the CPU reference of the feature's own test at that
test's tolerance, and the sites reached must be exactly the set written out here: a new scratch site fails these tests, and the
source lint (test_alloc_sites.py), until it is covered.

Failures are injected only: nothing here allocates a large amount, and no real hipMalloc failure is provoked (the clearing of
HIP's sticky last error after a real failure is one line of the one helper)."""
import ctypes

import numpy as np
import pytest

from test_gpu_alloc_failure import INJECTED, MAX_K, check_image

pytestmark = pytest.mark.gpu

f32 = np.float32
SENTINEL = 0xA5
ENOMEM = -6

# ---- the sites every entry point and variant reaches ------------------------------------------------------------------------
INDEX_SITES = {"index_x", "index_y", "index_z", "index_bounds", "index_keys", "index_keys_sorted", "index_order",
               "index_order_sorted", "index_sort_tmp", "index_sorted_x", "index_sorted_y", "index_sorted_z"}     # build_morton_index
_MOMENTS = {"moments_x", "moments_y", "moments_z", "moments_mass", "moments_boxes", "moments_partials", "moments_valid_count"}
_PROFILE = {"profile_x", "profile_y", "profile_z", "profile_mass", "profile_boxes", "profile_partials", "profile_result",
            "profile_edges", "profile_counters"}
_PRESENT = {"present_frame", "present_prims", "present_textures"}
SCRATCH_SITES = {
    "smoothing_lengths": INDEX_SITES,
    "sph_sum": INDEX_SITES | {"sph_sum_h", "sph_sum_a"},
    "fof_groups": INDEX_SITES | {"fof_rank_keys", "fof_sort_tmp"},
    "shrink_sphere_center": {"center_x", "center_y", "center_z", "center_mass", "center_boxes", "center_partials", "center_min_mass"},
    ("sphere_moments", False): _MOMENTS,
    ("sphere_moments", True): _MOMENTS | {"moments_vx", "moments_vy", "moments_vz"},
    ("radial_profile", False): _PROFILE,
    ("radial_profile", True): _PROFILE | {"profile_vx", "profile_vy", "profile_vz"},
    # (entry point, the base or the surface has a 1-D LUT)
    ("present", True): _PRESENT | {"present_lut"},
    ("present", False): _PRESENT,
    ("present_yuv420", True): _PRESENT | {"present_lut", "present_yuv"},
    ("present_yuv420", False): _PRESENT | {"present_yuv"},
    ("present_surface", True): _PRESENT | {"present_filtered", "present_lut"},
    ("present_surface", False): _PRESENT | {"present_filtered"},
    ("present_surface_yuv420", True): _PRESENT | {"present_filtered", "present_lut", "present_yuv"},
    ("present_surface_yuv420", False): _PRESENT | {"present_filtered", "present_yuv"},
    ("surface_present", True): {"surface_filtered", "surface_lut"},
    ("surface_present", False): {"surface_filtered"},
    "render_surface": {"surface_ranges", "surface_drawn_count"},
    "density_order_stats": {"rho_keys", "rho_keys_sorted", "rho_sort_tmp", "rho_ranks", "rho_values"},
    "upload_band_magnitudes": {"band_magnitudes", "band_weights"},
    "measure_read_bandwidth": {"bandwidth_buffer", "bandwidth_sink"},
    "reorder_spatial": {"reorder_bounds", "reorder_keys", "reorder_keys_sorted", "reorder_index", "reorder_order", "reorder_sort_tmp",
                        "reorder_strata_offsets", "reorder_cell_offsets", "reorder_spare"},
}

_fp = ctypes.POINTER(ctypes.c_float)
_dp = ctypes.POINTER(ctypes.c_double)
_i64p = ctypes.POINTER(ctypes.c_int64)
_u8p = ctypes.POINTER(ctypes.c_uint8)


@pytest.fixture(scope="module")
def native():
    from topsy_amd import _native
    _native.load_library()
    return _native


def P(a, kind=_fp):
    return None if a is None else a.ctypes.data_as(kind)


def col(a):
    return None if a is None else [np.ascontiguousarray(a[:, k], dtype=f32) for k in range(3)]


class Outputs:
    """The output buffers (numpy arrays) and info structs (ctypes) of one raw call, filled with sentinel bytes before every call."""

    def __init__(self, **items):
        self.items = items
        for name, v in items.items():
            setattr(self, name, v)

    def fill(self):
        for v in self.items.values():
            if isinstance(v, np.ndarray):
                v.view(np.uint8).reshape(-1)[:] = SENTINEL
            else:
                ctypes.memset(ctypes.byref(v), SENTINEL, ctypes.sizeof(v))

    def written(self):
        """names of the outputs that no longer hold the sentinel bit for bit"""
        bad = []
        for name, v in self.items.items():
            raw = v.view(np.uint8) if isinstance(v, np.ndarray) else np.frombuffer(bytes(v), dtype=np.uint8)
            if not (raw == SENTINEL).all():
                bad.append(name)
        return bad


def snapshot(ctx):
    """image, counts and resident particles (test_neighbours_unchanged of test_gpu_fof.py)"""
    counts = {k: v for k, v in ctx.stats().items() if not k.startswith("ms_")}
    return ctx.read_image(), counts, ctx.download_particles() if ctx.num_particles else {}


def assert_same_state(before, after, what):
    assert before[0].shape == after[0].shape and np.array_equal(before[0].view(np.uint32), after[0].view(np.uint32)), \
        f"{what}: the image changed"
    assert before[1] == after[1], f"{what}: the statistics changed"
    for k in before[2]:
        assert np.array_equal(before[2][k].view(np.uint32), after[2][k].view(np.uint32)), f"{what}: resident array {k} changed"


def walk(native, ctx, call, outs, expected, after_failure=None):
    """k = 1, 2, ... on the one context until `call` (-> the entry point's return code) succeeds; then `outs` holds its result"""
    lib = native.load_library()
    reached = []
    for k in range(1, MAX_K + 1):
        before = snapshot(ctx)
        outs.fill()
        ctx.set_option("debug_fail_alloc", k)
        rc = call()
        err = lib.tsp_last_error().decode(errors="replace")
        ctx.set_option("debug_fail_alloc", 0)
        if rc == 0:
            break
        found = INJECTED.search(err)
        assert rc == ENOMEM and found, f"k={k}: return code {rc}, not the injected failure: {err}"
        reached.append(found.group(1))
        what = f"after a failure at {reached[-1]} (k={k})"
        assert not outs.written(), f"{what}: outputs written: {outs.written()}"
        assert_same_state(before, snapshot(ctx), what)
        if after_failure:
            after_failure(what)
    else:
        pytest.fail(f"the call still failed at k={MAX_K}")
    print(f"\nallocation sites reached: {reached}")
    assert len(set(reached)) == len(reached), f"a site failed twice: {reached}"
    assert set(reached) == expected, (f"sites reached but not expected: {sorted(set(reached) - expected)}; "
                                      f"expected but not reached: {sorted(expected - set(reached))}")
    return reached


@pytest.fixture(scope="module")
def frame_ctx(native, mips):
    """a context that holds resident particles and a rendered frame: the analysis calls must leave all of it alone"""
    from oracle import oracle_np
    ctx = native.Context(160, 2)
    ctx.set_kernel_mips(mips)
    g = np.arange(-70.0, 71.0, 20.0, dtype=f32)
    gx, gy = (v.ravel() for v in np.meshgrid(g, g))
    ctx.upload_particles(gx, gy, np.zeros(64, dtype=f32), np.full(64, 3.0, dtype=f32), np.ones(64, dtype=f32))
    M, sf = oracle_np.transform_matrix(np.eye(3), np.zeros(3), 90.0)
    ctx.render(M, sf)
    assert np.count_nonzero(ctx.read_image()[..., 0]) > 64 * 20
    yield ctx
    ctx.close()


# ---- the neighbour index and what is built on it -----------------------------------------------------------------------------
def index_points(periodic):
    """3000 points, clustered and uniform; periodic: in a box of side 25, some of them whole periods outside it"""
    rs = np.random.RandomState(41)
    L = 25.0 if periodic else 0.0
    pos = rs.uniform(0.0, 25.0, size=(3000, 3))
    pos[:800] = rs.uniform(0.0, 1.5, size=(800, 3)) + rs.randint(0, 2, size=(800, 3)) * 23.5      # clustered at the corners
    if periodic:
        pos += rs.randint(-2, 3, size=pos.shape) * L
    return pos.astype(f32), L


@pytest.mark.parametrize("periodic", [False, True])
def test_smoothing_lengths(native, frame_ctx, periodic):
    from test_smoothing_cpu import brute_force_smoothing
    lib = native.load_library()
    pos, L = index_points(periodic)
    x, y, z = col(pos)
    outs = Outputs(h=np.empty(len(pos), dtype=f32))
    walk(native, frame_ctx, lambda: lib.tsp_smoothing_lengths(frame_ctx._h, len(pos), P(x), P(y), P(z), 32, L, P(outs.h)), outs,
         SCRATCH_SITES["smoothing_lengths"])
    want = brute_force_smoothing(pos, 32, period=L)
    assert np.array_equal(outs.h.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("periodic", [False, True])
def test_sph_sum(native, frame_ctx, periodic):
    from test_density_cpu import brute_force_sph_sum, within_one_ulp
    from test_smoothing_cpu import brute_force_smoothing
    lib = native.load_library()
    pos, L = index_points(periodic)
    x, y, z = col(pos)
    h = brute_force_smoothing(pos, 32, period=L)
    a = np.random.RandomState(23).uniform(0.5, 2.0, len(pos)).astype(f32)
    outs = Outputs(rho=np.empty(len(pos), dtype=f32))
    walk(native, frame_ctx, lambda: lib.tsp_sph_sum(frame_ctx._h, len(pos), P(x), P(y), P(z), P(h), P(a), L, P(outs.rho)), outs,
         SCRATCH_SITES["sph_sum"])
    ok = within_one_ulp(outs.rho, brute_force_sph_sum(pos, h, a, period=L))
    assert ok.all(), f"{np.count_nonzero(~ok)} of {len(pos)} differ by more than one ulp"


def test_fof_groups(native, frame_ctx):
    from test_fof_cpu import clumps, fof_reference
    lib = native.load_library()
    pos = np.ascontiguousarray(clumps()[:5000])
    ll = float(f32(0.2 * len(pos) ** (-1.0 / 3.0)))          # the scene's rule at this count: 0.2 mean separations
    labels_ref, info_ref = fof_reference(pos, f32(ll), 1.0, 20)
    assert info_ref["n_groups"] >= 3 and info_ref["n_valid"] == len(pos)
    x, y, z = col(pos)
    outs = Outputs(labels=np.empty(len(pos), dtype=np.int32), info=native.FofInfo())
    walk(native, frame_ctx, lambda: lib.tsp_fof_groups(frame_ctx._h, len(pos), P(x), P(y), P(z), ll, 1.0, 20,
                                                       P(outs.labels, ctypes.POINTER(ctypes.c_int32)), ctypes.byref(outs.info)),
         outs, SCRATCH_SITES["fof_groups"])
    info = {k: int(getattr(outs.info, k)) for k in ("n_valid", "n_groups", "n_grouped", "largest")}
    assert info == info_ref and np.array_equal(outs.labels, labels_ref)


# ---- the sphere passes -------------------------------------------------------------------------------------------------------
def test_shrink_sphere_center(native, frame_ctx):
    from test_center_cpu import reference, scene
    from test_gpu_center import _accept
    lib = native.load_library()
    pos, mass, kw = scene("clump")
    c_ref, info_ref, _ = reference("clump")
    a = dict(mass_cut_factor=0.0, r_start=0.0, shrink_factor=0.7, min_particles=100, max_iterations=256) | kw
    x, y, z = col(pos)
    m = np.ascontiguousarray(mass, dtype=f32)
    outs = Outputs(center=np.empty(3, dtype=np.float64), info=native.CenterInfo())
    walk(native, frame_ctx,
         lambda: lib.tsp_shrink_sphere_center(frame_ctx._h, len(pos), P(x), P(y), P(z), P(m), float(f32(a["mass_cut_factor"])),
                                              float(a["r_start"]), float(a["shrink_factor"]), int(a["min_particles"]),
                                              int(a["max_iterations"]), P(outs.center, _dp), ctypes.byref(outs.info)),
         outs, SCRATCH_SITES["shrink_sphere_center"])
    info = {"n_valid": int(outs.info.n_valid), "n_inside": int(outs.info.n_inside), "iterations": int(outs.info.iterations),
            "radius": float(outs.info.radius), "mass_inside": float(outs.info.mass_inside)}
    _accept("clump", (outs.center, info), (c_ref, info_ref))


@pytest.mark.parametrize("with_vel", [False, True])
def test_sphere_moments(native, frame_ctx, with_vel):
    from test_gpu_orient import _accept
    from test_orient_cpu import reference, scene
    lib = native.load_library()
    name = "disc" if with_vel else "no_vel"
    pos, mass, vel, kw = scene(name)
    assert (vel is not None) == with_vel
    x, y, z = col(pos)
    vx, vy, vz = col(vel) or (None, None, None)
    m = np.ascontiguousarray(mass, dtype=f32)
    center = np.ascontiguousarray(kw["center"], dtype=np.float64)
    outs = Outputs(moments=native.Moments())
    walk(native, frame_ctx,
         lambda: lib.tsp_sphere_moments(frame_ctx._h, len(pos), P(x), P(y), P(z), P(m), P(vx), P(vy), P(vz), P(center, _dp),
                                        float(kw["r"]), float(kw["r_vel"]), ctypes.byref(outs.moments)),
         outs, SCRATCH_SITES[("sphere_moments", with_vel)])
    _accept(name, outs.moments.as_dict(), reference(name))


@pytest.mark.parametrize("n_bins", [100, 104])            # a table per wave | one per workgroup (the step is at 103 / 104)
@pytest.mark.parametrize("geometry", [0, 1])
@pytest.mark.parametrize("with_vel", [False, True])
def test_radial_profile(native, frame_ctx, with_vel, geometry, n_bins):
    from test_gpu_profile import _accept
    from test_profile_cpu import near_edge_margin, reference, scene, spec_of
    lib = native.load_library()
    name = "disc" if with_vel else "no_vel"
    pos, mass, vel, _ = scene(name)
    assert (vel is not None) == with_vel
    kw = spec_of(name, geometry, n_bins)
    assert near_edge_margin(pos, kw) > 1e-9
    edges = np.ascontiguousarray(kw["edges"], dtype=np.float64)
    spec = native.ProfileSpec()
    spec.geometry, spec.n_bins, spec.edges = geometry, n_bins, P(edges, _dp)
    spec.center[:] = np.asarray(kw["center"], dtype=np.float64).tolist()
    spec.v_cen[:] = np.asarray(kw.get("v_cen", (0.0, 0.0, 0.0)), dtype=np.float64).tolist()
    spec.frame[:] = np.asarray(kw["frame"], dtype=np.float64).ravel().tolist()
    spec.half_height = float(kw["half_height"])
    x, y, z = col(pos)
    vx, vy, vz = col(vel) or (None, None, None)
    m = np.ascontiguousarray(mass, dtype=f32)
    outs = Outputs(count=np.empty(n_bins, dtype=np.int64), sums=np.empty((n_bins, native.PROFILE_SUMS), dtype=np.float64),
                   info=native.ProfileInfo())
    walk(native, frame_ctx,
         lambda: lib.tsp_radial_profile(frame_ctx._h, len(pos), P(x), P(y), P(z), P(m), P(vx), P(vy), P(vz), ctypes.byref(spec),
                                        P(outs.count, _i64p), P(outs.sums, _dp), ctypes.byref(outs.info)),
         outs, SCRATCH_SITES[("radial_profile", with_vel)])
    got = {"count": outs.count, "sums": outs.sums, "n_valid": int(outs.info.n_valid), "n_inner": int(outs.info.n_inner),
           "n_binned": int(outs.info.n_binned), "mass_inner": float(outs.info.mass_inner)}
    _accept(f"{name}, geometry {geometry}, {n_bins} bins", got, reference(name, geometry, n_bins))


def test_measure_read_bandwidth(native, frame_ctx):
    lib = native.load_library()
    outs = Outputs(gbps=ctypes.c_double())
    walk(native, frame_ctx, lambda: lib.tsp_measure_read_bandwidth(frame_ctx._h, 1 << 20, 1, ctypes.byref(outs.gbps)), outs,
         SCRATCH_SITES["measure_read_bandwidth"])
    assert np.isfinite(outs.gbps.value) and outs.gbps.value > 0.0         # the call after the failures succeeds


# ---- frame composition -------------------------------------------------------------------------------------------------------
W, H = 64, 48


def frame_buffer(yuv420):
    return np.empty(W * H + 2 * ((W // 2) * (H // 2)), dtype=np.uint8) if yuv420 else np.empty((H, W, 4), dtype=np.uint8)


def assert_frame(got, want_rgba, yuv420):
    import yuv420_ref
    if not yuv420:
        assert got.dtype == want_rgba.dtype and np.array_equal(got, want_rgba)
        return
    n, c = W * H, (W // 2) * (H // 2)
    planes = got[:n].reshape(H, W), got[n:n + c].reshape(H // 2, W // 2), got[n + c:].reshape(H // 2, W // 2)
    for plane, want, name in zip(planes, yuv420_ref.to_yuv420(want_rgba), "YUV"):
        assert np.array_equal(plane, want), name


@pytest.mark.parametrize("yuv420", [False, True])
@pytest.mark.parametrize("map_name", ["scalar", "rgb"])           # a scalar base with a LUT; an rgb base without one
def test_present(native, map_name, yuv420):
    import present_ref
    from test_gpu_present import overlapping_layers
    lib = native.load_library()
    rs = np.random.RandomState(5)
    img = rs.uniform(0.0, 3.0, size=(96, 96, 4)).astype(f32)
    img[3, 5, 0] = np.nan
    layers = overlapping_layers(rs)
    lut = rs.uniform(0, 1, size=(50, 4)).astype(f32)
    base = ({"map": "scalar", "lut": lut, "vmin": 0.1, "vmax": 2.5, "log": False, "weighted": True} if map_name == "scalar"
            else {"map": "rgb", "vmin": -1.0, "vmax": 0.5, "gamma": 0.8})
    ctx = native.Context(96, 4)
    try:
        ctx.write_image(img)
        b, arr, _keep = native.Context._present_args(base, layers)
        entry = lib.tsp_present_yuv420 if yuv420 else lib.tsp_present
        outs = Outputs(frame=frame_buffer(yuv420), ms=ctypes.c_double())
        walk(native, ctx, lambda: entry(ctx._h, W, H, ctypes.byref(b), arr, len(layers), outs.frame.ctypes.data_as(entry.argtypes[6]),
                                        ctypes.byref(outs.ms)),
             outs, SCRATCH_SITES[("present_yuv420" if yuv420 else "present", map_name == "scalar")])
        assert_frame(outs.frame, present_ref.compose(img, W, H, base, layers), yuv420)
    finally:
        ctx.close()


def surface_context(native, R):
    from topsy_amd import kernel_lut
    ctx = native.Context(R, 2)
    ctx.set_kernel_mips(kernel_lut.kernel_mips())
    ctx.set_sphere_mips(kernel_lut.sphere_mips())
    return ctx


@pytest.mark.parametrize("yuv420", [False, True])
@pytest.mark.parametrize("weighted", [False, True])                # the material of the surface: constant | through a LUT
def test_present_surface(native, weighted, yuv420):
    import surface_present_ref
    from test_gpu_present import overlapping_layers
    from test_surface_present_cpu import SHADING_OPTIONS, shading_image, shading_params
    lib = native.load_library()
    img = shading_image()
    params = shading_params(SHADING_OPTIONS[1 if weighted else 0])
    assert bool(params.get("weighted_average", False)) == weighted
    layers = overlapping_layers(np.random.RandomState(5))
    ctx = surface_context(native, img.shape[0])
    try:
        ctx.write_image(img)
        p, _lut = native.Context._surface_params(**params)
        arr, _keep = native.Context._layer_args(layers)
        entry = lib.tsp_present_surface_yuv420 if yuv420 else lib.tsp_present_surface
        outs = Outputs(frame=frame_buffer(yuv420), ms=(ctypes.c_double * 2)())
        walk(native, ctx, lambda: entry(ctx._h, W, H, ctypes.byref(p), arr, len(layers), P(outs.frame, _u8p), outs.ms), outs,
             SCRATCH_SITES[("present_surface_yuv420" if yuv420 else "present_surface", weighted)])
        assert_frame(outs.frame, surface_present_ref.compose_surface(img, W, H, params, layers), yuv420)
    finally:
        ctx.close()


@pytest.mark.parametrize("weighted", [False, True])
def test_surface_present(native, weighted):
    import surface_ref
    from test_surface_present_cpu import SHADING_OPTIONS, shading_image, shading_params
    lib = native.load_library()
    img = shading_image()
    R = img.shape[0]
    params = shading_params(SHADING_OPTIONS[1 if weighted else 0])
    ctx = surface_context(native, R)
    try:
        ctx.write_image(img)
        p, _lut = native.Context._surface_params(**params)
        outs = Outputs(content=np.empty((R, R, 2), dtype=f32), rgba=np.empty((R, R, 4), dtype=np.uint8), ms=(ctypes.c_double * 2)())
        walk(native, ctx, lambda: lib.tsp_surface_present(ctx._h, ctypes.byref(p), P(outs.content), P(outs.rgba, _u8p), outs.ms), outs,
             SCRATCH_SITES[("surface_present", weighted)])
        want_f = surface_ref.bilateral(img, params["smoothing_scale"])
        assert np.array_equal(outs.content.view(np.uint32), want_f.view(np.uint32))
        shade_args = {k: v for k, v in params.items() if k not in ("smoothing_scale", "lut_rgba")}
        assert np.array_equal(outs.rgba, surface_ref.shade(want_f, lut=params["lut_rgba"], **shade_args))
    finally:
        ctx.close()


# ---- the occlusion pass and the density cut ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cloud_ctx(native):
    """4000 resident particles at R = 64"""
    from conftest import make_cloud
    pos, h, m, q, _ = make_cloud(4000, seed=0)
    ctx = surface_context(native, 64)
    ctx.upload_particles(pos[:, 0], pos[:, 1], pos[:, 2], h, m)
    ctx.upload_quantity(q)
    yield ctx, pos, h, m, q
    ctx.close()


def test_render_surface(native, cloud_ctx):
    """A failed call leaves the occlusion keys and the image of the frame before it: an empty block drawn with clear = 0 after the
    failure resolves the keys it finds, and must give that frame again."""
    import surface_ref
    from oracle import oracle_np
    lib = native.load_library()
    ctx, pos, h, m, q = cloud_ctx
    R = 64
    cut = surface_ref.cut_for_percentile(surface_ref.density_cuts(m, h), 50.0)
    M0, sf0 = oracle_np.transform_matrix(np.eye(3), np.zeros(3), 80.0)
    M, sf = oracle_np.transform_matrix(np.eye(3), np.zeros(3), 50.0)
    ctx.render_surface(M0, sf0, cut)
    frame0 = ctx.read_image()
    assert np.count_nonzero(frame0[..., 1]) > 50
    Mf = np.ascontiguousarray(np.asarray(M, dtype=f32).reshape(16))
    empty = (np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64))

    def keys_are_the_old_ones(what):
        ctx.render_surface(M0, sf0, cut, *empty, clear=False)
        assert np.array_equal(ctx.read_image().view(np.uint32), frame0.view(np.uint32)), f"{what}: the occlusion keys changed"

    outs = Outputs(ms=ctypes.c_double())
    walk(native, ctx, lambda: lib.tsp_render_surface(ctx._h, P(Mf), float(sf), float(f32(cut)), None, None, 0, 1, ctypes.byref(outs.ms)),
         outs, SCRATCH_SITES["render_surface"], after_failure=keys_are_the_old_ones)
    ps = np.column_stack([pos, h]).astype(f32)
    want, winner = surface_ref.occlusion(ps, m, q, M, sf, R, cut, surface_ref.sphere_mips())
    assert (winner >= 0).sum() > 50
    assert np.array_equal(ctx.read_image().view(np.uint32), want.view(np.uint32))


def test_density_order_stats(native, cloud_ctx):
    import surface_ref
    from topsy_amd.colormap.implementation import quantile_from_order_statistics
    lib = native.load_library()
    ctx, pos, h, m, q = cloud_ctx
    n = len(h)
    ranks = np.unique(np.linspace(0, n - 1, 77).astype(np.int64))
    outs = Outputs(values=np.empty(len(ranks), dtype=f32))
    walk(native, ctx, lambda: lib.tsp_density_order_stats(ctx._h, P(ranks, _i64p), len(ranks), P(outs.values)), outs,
         SCRATCH_SITES["density_order_stats"])
    rho = m / ((h * h) * h)
    assert np.array_equal(outs.values, np.sort(rho)[ranks])
    cuts = quantile_from_order_statistics(ctx.density_order_stats, n, np.linspace(0, 1, 101))
    assert np.array_equal(cuts, surface_ref.density_cuts(m, h))


# ---- uploads and the load-time ordering --------------------------------------------------------------------------------------
def test_upload_band_magnitudes(native, mips):
    """The two staging buffers.  After a failed call an rgb render still shows the colours of the upload before it."""
    from conftest import make_cloud
    from oracle import oracle_c, oracle_np
    lib = native.load_library()
    R, n = 128, 3000
    M, sf = oracle_np.transform_matrix(np.eye(3), np.zeros(3), 150.0)
    pos, h, m, _, _ = make_cloud(n, seed=9)
    x, y, z = col(pos)
    rs = np.random.RandomState(4)
    weights = np.ascontiguousarray(np.diag([0.5, 1.0, 1.0]))
    mags = [np.ascontiguousarray(rs.uniform(2.0, 14.0, size=(3, n))) for _ in range(2)]

    def oracle_image(mg):
        rgb = oracle_np.band_contraction(mg, weights).astype(f32)
        img, _ = oracle_c.splat(x, y, z, h, rgb[:, 0].copy(), rgb[:, 1].copy(), rgb[:, 2].copy(), mode=2, M=M, sf=float(sf), R=R, mips=mips)
        return img.astype(np.float64)

    want_old, want_new = oracle_image(mags[0]), oracle_image(mags[1])
    assert not np.array_equal(want_old, want_new)
    ctx = native.Context(R, 4)
    try:
        ctx.set_kernel_mips(mips)
        ctx.upload_particles(x, y, z, h, m)
        ctx.upload_band_magnitudes(mags[0], weights)

        def shows(want, what):
            ctx.render(M, sf, mode=native.MODE_RGB)
            check_image("rgb", ctx.read_image(), want, None, what)

        shows(want_old, "before the walk")
        walk(native, ctx, lambda: lib.tsp_upload_band_magnitudes(ctx._h, 3, P(mags[1], _dp), P(weights, _dp)), Outputs(),
             SCRATCH_SITES["upload_band_magnitudes"], after_failure=lambda what: shows(want_old, what + ", the colours before it"))
        shows(want_new, "after the upload")
    finally:
        ctx.close()


def assert_same_layout(ctx, before, what):
    """the comparisons of test_refused_calls_change_nothing (test_gpu_reorder.py)"""
    from test_gpu_reorder import bits
    assert np.array_equal(ctx.strata_offsets(), before[0]), f"{what}: layout changed (the strata offsets)"
    lay = ctx.cell_layout()
    assert (lay is None) == (before[1] is None), f"{what}: layout changed (a cell layout where there was none)"
    if lay is not None:
        assert lay["n_strata"] == before[1]["n_strata"] and lay["cells_per_axis"] == before[1]["cells_per_axis"] and \
            np.array_equal(lay["offsets"], before[1]["offsets"]), f"{what}: layout changed (the cell offsets)"
        assert all(np.array_equal(bits(lay[k]), bits(before[1][k])) for k in ("box_lo", "cell_width")), f"{what}: layout changed (the grid)"


@pytest.mark.parametrize("reordered", [False, True])              # a never-reordered context | one that already is
@pytest.mark.parametrize("interleave", [0, 1, 2])
def test_reorder_spatial(native, mips, interleave, reordered):
    """All or nothing: after a failed call the particles lie in their old order, the layout describes that order, and a render
    is the oracle's."""
    import reorder_ref as ref
    from oracle import oracle_c
    from test_gpu_reorder import attributes, check_layout, check_resident, load, smoothing, view
    lib = native.load_library()
    R, n = 64, 1023
    pos = ref.scene_nonfinite(n, 6)
    (M, sf), _ = view(pos)
    h = smoothing(0, n, 1) * f32(4.0)                          # distinct (arrangement 2 is one permutation), 1.4 to 7 pixels wide
    d = attributes(pos, h, 3)
    rs = np.random.RandomState(12)
    d["mass"], d["q"] = rs.uniform(0.5, 2.0, n).astype(f32), rs.uniform(0.5, 1.5, n).astype(f32)
    want, _ = oracle_c.splat(d["x"], d["y"], d["z"], h, d["mass"], d["q"], mode=0, M=M, sf=float(sf), R=R, mips=mips)
    want = want.astype(np.float64)
    assert np.count_nonzero(want[..., 0]) > R * R // 4

    ctx = native.Context(R, 4)
    try:
        ctx.set_kernel_mips(mips)
        load(ctx, d)
        ctx.set_option("reorder_interleave", interleave)
        perm0 = ctx.reorder_spatial(8, 2, want_permutation=True) if reordered else np.arange(n)
        layout0 = (ctx.strata_offsets(), ctx.cell_layout())
        assert (layout0[1] is not None) == reordered

        def renders(what):
            ctx.render(M, sf)
            check_image("weighted", ctx.read_image(), want, want[..., 1], what)       # (q > 0: the terms are their magnitudes)

        def nothing_changed(what):
            check_resident(ctx, d, perm0)
            assert_same_layout(ctx, layout0, what)
            renders(what)

        renders("before the walk")
        outs = Outputs(perm=np.empty(n, dtype=np.int64))
        walk(native, ctx, lambda: lib.tsp_reorder_spatial(ctx._h, 3, 5, P(outs.perm, _i64p)), outs, SCRATCH_SITES["reorder_spatial"],
             after_failure=nothing_changed)
        # the call sorts the particles as they lie and reports new -> original indices (test_a_second_reorder_composes)
        m = ref.reorder(pos[perm0], h[perm0], 3, 5, interleave)
        perm = perm0[m["perm_by_h" if interleave == 2 else "perm"]]
        assert np.array_equal(outs.perm, perm)
        check_layout(ctx, m, n)
        check_resident(ctx, d, perm)
        renders("after the reorder")
    finally:
        ctx.close()
