"""Spectral cubes on the GPU (tsp_spectral_cube, topsy_amd.spectral_cube, VelocityView.get_cube) against the float64 model of
spectral_cube_ref.py and against the proven kernels.  The scene is all_class_scene(128) with the velocities of
test_gpu_kinematics.py: 1500 particles of every footprint class, partly off-screen, some on pixel corners, masses positive.

Per cell: |got - want| <= 1e-5 * want + 1e-6 * S_pixel, S_pixel the model's sum over all velocities at the pixel: 1e-5 is the
project's density tolerance, 1e-6 covers the 5 s truncation the kernel is allowed (5.8e-7 of a particle's mass)."""
import ctypes

import numpy as np
import pytest

import kinematics_ref
import parity_scenes as ps
import spectral_cube_ref as ref

pytestmark = pytest.mark.gpu
R = 128
SCALE = 100.0
f32 = np.float32
V_BULK = np.array([50.0, -30.0, 20.0], dtype=f32)
TILT = ps._rot(0.15, -0.1) @ ps.roll(0.9)
BAND = dict(v_min=-400.0, dv=20.0, n_channels=40)           # two channel blocks
EINVAL, ESTATE, ENOMEM = -1, -4, -6


@pytest.fixture(scope="module")
def native():
    from topsy_amd import _native
    _native.load_library()
    return _native


def with_velocities(sc, seed=11):
    rs = np.random.RandomState(seed)
    sc["vel"] = (rs.normal(0.0, 100.0, size=sc["pos"].shape) + np.array([50.0, -30.0, 20.0])).astype(f32)
    return sc


@pytest.fixture(scope="module")
def scene():
    sc = with_velocities(ps.all_class_scene(R))
    for a in sc.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return sc


def camera(rotation=None, scale=SCALE):
    from oracle import oracle_np
    rotation = np.eye(3) if rotation is None else rotation
    M, sf = oracle_np.transform_matrix(rotation, np.zeros(3), scale)
    axis = rotation[2] / np.sqrt(rotation[2] @ rotation[2])
    return M, sf, axis.astype(f32)


def new_context(native, mips, sc, resolution=R, vel=None, los=None):
    ctx = native.Context(resolution, 4)
    ctx.set_kernel_mips(mips)
    p = sc["pos"]
    ctx.upload_particles(p[:, 0], p[:, 1], p[:, 2], sc["h"], sc["m"])
    vel = sc["vel"] if vel is None else vel
    ctx.upload_velocities(*(np.ascontiguousarray(vel[:, k]) for k in range(3)))
    if los is not None:
        ctx.set_line_of_sight(*los)
    return ctx


_models = {}


def model(sc, mips, M, sf, axis, v_ref, resolution=R, vel=None, sigma_v=0.0, sigma=None, **band):
    """the float64 model, computed once per configuration and left unchanged"""
    vel = sc["vel"] if vel is None else vel
    key = ps._key(sc["pos"], sc["h"], sc["m"], vel, np.asarray(M, dtype=f32), f32(sf), np.asarray(axis, dtype=f32),
                  np.asarray(v_ref, dtype=f32), np.asarray([band["v_min"], band["dv"], band["n_channels"], sigma_v, resolution]),
                  np.zeros(0) if sigma is None else np.asarray(sigma, dtype=f32))
    if key not in _models:
        want, S = ref.cube(sc["pos"], sc["h"], sc["m"], vel, M, sf, resolution, axis, v_ref, band["v_min"], band["dv"],
                           band["n_channels"], sigma_v, sigma, mips)
        want.setflags(write=False)
        S.setflags(write=False)
        _models[key] = (want, S)
    return _models[key]


def check(got, want, S, label):
    assert got.dtype == f32 and got.shape == want.shape, label
    ok, worst = ref.within(got, want, S)
    print(f"{label}: worst |got - want| / bound = {worst:.3g}; cells above 0: {np.count_nonzero(got)} of {got.size}")
    assert ok, (label, worst)


@pytest.fixture(scope="module")
def plain(native, mips, scene):
    """the context of case 1 (untilted, v_ref = 0), its camera, its cube and the model"""
    M, sf, axis = camera()
    ctx = new_context(native, mips, scene, los=(axis, np.zeros(3)))
    got = ctx.spectral_cube(M, sf, sigma_v=30.0, **BAND)
    want, S = model(scene, mips, M, sf, axis, np.zeros(3), sigma_v=30.0, **BAND)
    yield ctx, (M, sf, axis), got, want, S
    ctx.close()


# ---- 1. against the model ------------------------------------------------------------------------------------------------------
def test_cube_matches_the_model(plain):
    _, _, got, want, S = plain
    assert np.count_nonzero(want.sum(axis=(1, 2))) == BAND["n_channels"] and (S > 0).sum() > R * R // 2
    check(got, want, S, "untilted, v_ref = 0")


def test_tilted_cube_about_the_bulk_velocity_matches_the_model(native, mips, scene):
    M, sf, axis = camera(TILT)
    ctx = new_context(native, mips, scene, los=(axis, V_BULK))
    got = ctx.spectral_cube(M, sf, sigma_v=30.0, **BAND)
    ctx.close()
    check(got, *model(scene, mips, M, sf, axis, V_BULK, sigma_v=30.0, **BAND), "tilted, v_ref = bulk")


# ---- 2. zero width: a particle's mass lands in exactly one channel or none -------------------------------------------------------
def test_zero_width_lines_on_edges_and_outside_the_band(native, mips, scene):
    M, sf, axis = camera()
    vel = scene["vel"].copy()
    vel[:, :2] = 0.0
    on_edges = np.array([-400.0, -380.0, 0.0, 20.0, 380.0, -20.0], dtype=f32)
    outside = np.array([400.0, -400.5, 1e6, -1e6, 400.001], dtype=f32)             # the upper end of the band is outside it
    n = len(vel)
    vel[0::40, 2] = np.resize(on_edges, len(range(0, n, 40)))
    vel[5::40, 2] = np.resize(outside, len(range(5, n, 40)))
    ctx = new_context(native, mips, scene, vel=vel, los=(axis, np.zeros(3)))
    got = ctx.spectral_cube(M, sf, sigma_v=0.0, **BAND)
    ctx.close()
    want, S = model(scene, mips, M, sf, axis, np.zeros(3), vel=vel, sigma_v=0.0, **BAND)
    assert (want.sum(axis=0) < S * (1 - 1e-9)).any()          # some mass is outside the band
    check(got, want, S, "sigma_v = 0")


# ---- 3. per-particle widths, and their permutation -----------------------------------------------------------------------------
@pytest.mark.parametrize("reorder", [False, True])
def test_per_particle_sigma_in_the_callers_order(native, mips, scene, reorder):
    M, sf, axis = camera()
    n = len(scene["h"])
    sigma = np.random.RandomState(3).uniform(5.0, 60.0, n).astype(f32)
    sigma[::9] = 0.0
    sigma[4::50] = np.nan
    sigma[5::50] = np.inf
    sigma[6::50] = -1.0
    ctx = new_context(native, mips, scene, los=(axis, np.zeros(3)))
    if reorder:
        perm = ctx.reorder_spatial(4, 7, want_permutation=True)
        assert not np.array_equal(perm, np.arange(n))
    got = ctx.spectral_cube(M, sf, sigma_v=0.0, sigma=sigma, **BAND)
    ctx.close()
    want, S = model(scene, mips, M, sf, axis, np.zeros(3), sigma_v=0.0, sigma=sigma, **BAND)
    s, dead = ref.line_widths(n, 0.0, sigma)
    assert dead.sum() == 90 and (s[~dead] == 0).sum() > 100   # the model leaves the dead particles out
    check(got, want, S, f"per-particle sigma, reorder = {reorder}")


# ---- 4. against the proven kernels ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rotation", [None, TILT], ids=["untilted", "tilted"])
def test_channel_sum_is_the_kinematic_surface_density(native, mips, scene, rotation):
    M, sf, axis = camera(rotation)
    u = kinematics_ref.kinematic_colours(scene["m"], scene["vel"], axis, np.zeros(3))[3].astype(np.float64)
    sigma_v = 25.0
    lo, hi = u.min() - 6 * sigma_v, u.max() + 6 * sigma_v
    n_channels = 48
    ctx = new_context(native, mips, scene, los=(axis, np.zeros(3)))
    got = ctx.spectral_cube(M, sf, lo, (hi - lo) / n_channels, n_channels, sigma_v=sigma_v)
    one = ctx.spectral_cube(M, sf, u.min() - 1.0, (u.max() - u.min()) + 2.0, 1, sigma_v=0.0)
    ctx.render(M, sf, mode=native.MODE_KINEMATIC)
    S = ctx.read_image()[..., 0].astype(np.float64)
    ctx.close()
    total = got.astype(np.float64).sum(axis=0)
    assert (S > 0).sum() > R * R // 2
    err = np.abs(total - S)
    print(f"sum of channels against S: worst {np.max(err / np.maximum(S, 1e-300)):.3g} relative")
    assert (err <= 2e-5 * S + 1e-6 * S).all()
    err1 = np.abs(one[0].astype(np.float64) - S)
    print(f"one channel against S: worst {np.max(err1 / np.maximum(S, 1e-300)):.3g} relative")
    assert one.shape == (1, R, R) and (err1 <= 2e-5 * S).all()


# ---- 5. reproducibility and isolation ------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_two_calls_give_the_same_bits_and_change_nothing_else(native, plain):
    ctx, (M, sf, axis), got, _, _ = plain
    ctx.render(M, sf, mode=native.MODE_KINEMATIC)
    image, stats, maps = ctx.read_image(), ctx.stats(), ctx.velocity_moments()
    again = ctx.spectral_cube(M, sf, sigma_v=30.0, **BAND)
    assert np.array_equal(bits(again), bits(got))
    assert np.array_equal(bits(ctx.read_image()), bits(image)) and ctx.stats() == stats
    assert np.array_equal(bits(ctx.velocity_moments()), bits(maps))
    assert ctx.active_channels == 4


# ---- 6. slices -----------------------------------------------------------------------------------------------------------------
def test_forced_slices_stay_within_the_tolerance_and_the_default_returns(native, plain):
    ctx, (M, sf, axis), got, want, S = plain
    assert native.spectral_cube_layout(1500, R, BAND["n_channels"], 256)["slices"] == 6
    ctx.set_option("cube_slice_particles", 256)
    try:
        sliced = ctx.spectral_cube(M, sf, sigma_v=30.0, **BAND)
    finally:
        ctx.set_option("cube_slice_particles", 0)
    check(sliced, want, S, "slices of 256 particles")
    assert not np.array_equal(bits(sliced), bits(got))        # (a float32 rounding per slice: other last bits)
    assert np.array_equal(bits(ctx.spectral_cube(M, sf, sigma_v=30.0, **BAND)), bits(got))


# ---- 7. shapes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resolution", [100, 8])          # not a multiple of the tile; smaller than one tile
def test_resolutions_off_the_tile_grid(native, mips, resolution):
    sc = with_velocities(ps.all_class_scene(resolution, n=400))
    M, sf, axis = camera()
    band = dict(v_min=-300.0, dv=25.0, n_channels=33)
    ctx = new_context(native, mips, sc, resolution=resolution, los=(axis, V_BULK))
    got = ctx.spectral_cube(M, sf, sigma_v=25.0, **band)
    ctx.close()
    want, S = model(sc, mips, M, sf, axis, V_BULK, resolution=resolution, sigma_v=25.0, **band)
    assert (S > 0).all()
    check(got, want, S, f"R = {resolution}")


def small_scene(P, vel):
    """footprints of widths P (px at R = 128) at the centre of the view"""
    n = len(P)
    sc = ps.make_scene(np.zeros((n, 3)) + 0.3, np.asarray(P) * SCALE / (2.0 * R), np.full(n, 1.5), np.zeros(n), np.zeros((n, 3)),
                       P=np.asarray(P), scale=SCALE)
    sc["vel"] = np.asarray(vel, dtype=f32).reshape(n, 3)
    return sc


def test_one_footprint_that_covers_everything(native, mips):
    sc = small_scene([4000.0], [[0.0, 0.0, 37.0]])
    M, sf, axis = camera()
    ctx = new_context(native, mips, sc, los=(axis, np.zeros(3)))
    got = ctx.spectral_cube(M, sf, sigma_v=30.0, **BAND)
    ctx.close()
    want, S = model(sc, mips, M, sf, axis, np.zeros(3), sigma_v=30.0, **BAND)
    assert (S > 0).all()
    check(got, want, S, "one footprint of 4000 px")


def test_one_particle_and_an_empty_band(native, mips):
    sc = small_scene([9.0], [[0.0, 0.0, -123.0]])
    M, sf, axis = camera()
    ctx = new_context(native, mips, sc, los=(axis, np.zeros(3)))
    got = ctx.spectral_cube(M, sf, sigma_v=0.0, **BAND)
    empty = ctx.spectral_cube(M, sf, 200.0, 10.0, 40, sigma_v=3.0)         # the line ends 5 s = 15 above -123
    ctx.close()
    want, S = model(sc, mips, M, sf, axis, np.zeros(3), sigma_v=0.0, **BAND)
    check(got, want, S, "n = 1")
    c = int(np.floor((-123.0 + 400.0) / 20.0))
    assert np.count_nonzero(got[c]) == np.count_nonzero(S) > 20 and np.count_nonzero(got) == np.count_nonzero(got[c])
    assert empty.shape == (40, R, R) and not empty.any()


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------
def raw_call(native, ctx, M, sf, out, v_min=-400.0, dv=20.0, n_channels=40, sigma_v=30.0, sigma=None, null_M=False, null_out=False):
    lib = native.load_library()
    fp = ctypes.POINTER(ctypes.c_float)
    Mf = np.ascontiguousarray(np.asarray(M, dtype=f32).reshape(16))
    return lib.tsp_spectral_cube(ctx._h, None if null_M else Mf.ctypes.data_as(fp), float(sf), v_min, dv, n_channels, sigma_v,
                                 None if sigma is None else sigma.ctypes.data_as(fp), None if null_out else out.ctypes.data_as(fp))


def test_refused_calls_leave_the_output_and_the_context_alone(native, mips, scene, plain):
    from test_gpu_scratch_alloc_failure import assert_same_state, snapshot
    ctx, (M, sf, axis), _, _, _ = plain
    out = np.full((40, R, R), 7.25, dtype=f32)
    before = snapshot(ctx)
    invalid = [dict(null_M=True), dict(null_out=True), dict(v_min=np.nan), dict(v_min=np.inf), dict(dv=np.nan), dict(dv=np.inf),
               dict(sigma_v=np.nan), dict(sigma_v=np.inf), dict(dv=0.0), dict(dv=-1.0), dict(sigma_v=-1.0), dict(n_channels=0),
               dict(n_channels=-3), dict(n_channels=4097)]
    for kw in invalid:
        assert raw_call(native, ctx, M, sf, out, **kw) == EINVAL, kw
        assert (out == 7.25).all(), kw
    assert_same_state(before, snapshot(ctx), "after the invalid calls")
    big = native.Context(1024, 4)                             # 2049 * 1024^2 > 2^31: refused before anything is read or allocated
    try:
        assert raw_call(native, big, M, sf, out, n_channels=2049) == EINVAL and (out == 7.25).all()
    finally:
        big.close()

    p = scene["pos"]
    stages = [("nothing", lambda c: None),
              ("mips only", lambda c: c.set_kernel_mips(mips)),
              ("particles without mass", lambda c: c.upload_particles(p[:, 0], p[:, 1], p[:, 2], scene["h"])),
              ("mass, no velocities", lambda c: c.upload_particles(p[:, 0], p[:, 1], p[:, 2], scene["h"], scene["m"])),
              ("velocities, no line of sight", lambda c: c.upload_velocities(*(scene["vel"][:, k].copy() for k in range(3))))]
    def state_of(c):        # snapshot() of a context that may hold no mass yet
        counts = {k: v for k, v in c.stats().items() if not k.startswith("ms_")}
        return c.read_image(), counts, c.download_particles(("x", "y", "z", "h")) if c.num_particles else {}

    ctx2 = native.Context(R, 4)
    try:
        for name, step in stages:
            step(ctx2)
            state = state_of(ctx2)
            assert raw_call(native, ctx2, M, sf, out) == ESTATE, name
            assert (out == 7.25).all(), name
            assert_same_state(state, state_of(ctx2), name)
        ctx2.set_line_of_sight(axis, np.zeros(3))
        assert raw_call(native, ctx2, M, sf, out) == 0 and np.array_equal(bits(out), bits(plain[2]))
    finally:
        ctx2.close()


# ---- 9. allocation failure -----------------------------------------------------------------------------------------------------
def test_failed_scratch_allocations(native, plain):
    from test_gpu_scratch_alloc_failure import SCRATCH_SITES, Outputs, walk
    ctx, (M, sf, axis), got, _, _ = plain
    sites = SCRATCH_SITES["sph_sum"] - set(s for s in SCRATCH_SITES["sph_sum"] if s.startswith("index_"))
    assert sites == {"sph_sum_h", "sph_sum_a"}
    outs = Outputs(cube=np.empty((40, R, R), dtype=f32))
    reached = walk(native, ctx, lambda: raw_call(native, ctx, M, sf, outs.cube), outs, sites)
    assert reached == ["sph_sum_h", "sph_sum_a"]
    assert np.array_equal(bits(outs.cube), bits(got))         # the call after the failures, on the same context


# ---- 10. Python ----------------------------------------------------------------------------------------------------------------
def test_spectral_cube_of_arrays_is_the_contexts(native, mips, scene):
    import topsy_amd
    from topsy_amd import particle_buffers
    M, sf, axis = camera(TILT)
    n = len(scene["h"])
    sigma = np.random.RandomState(5).uniform(0.0, 40.0, n).astype(f32)
    kw = dict(n_channels=40, sigma_v=10.0, sigma=sigma)
    cube = topsy_amd.spectral_cube(scene["pos"], scene["h"], scene["m"], scene["vel"], v_range=(-400.0, 400.0), rotation=TILT,
                                   scale=SCALE, resolution=R, v_ref=V_BULK, **kw)
    ctx = new_context(native, mips, scene, los=(axis, V_BULK))
    ctx.reorder_spatial(particle_buffers.ParticleBuffers._num_strata(n), 1337)
    want = ctx.spectral_cube(M, sf, -400.0, 20.0, **kw)
    ctx.close()
    assert isinstance(cube, topsy_amd.SpectralCube) and cube.dv == 20.0 and np.array_equal(cube.v_edges, ref.edges(-400.0, 20.0, 40))
    assert np.array_equal(bits(cube.data), bits(want))
    # the default band: wide enough for every line
    auto = topsy_amd.spectral_cube(scene["pos"], scene["h"], scene["m"], scene["vel"], rotation=TILT, scale=SCALE, resolution=R,
                                   v_ref=V_BULK, n_channels=16, sigma_v=10.0)
    u = kinematics_ref.kinematic_colours(scene["m"], scene["vel"], axis, V_BULK)[3].astype(np.float64)
    assert auto.v_edges[-1] == pytest.approx(np.abs(u).max() + 50.0, rel=1e-6) and auto.v_edges[0] == -auto.v_edges[-1]


def test_view_cube_at_the_visualizers_camera(native, mips, scene):
    """VelocityView.get_cube after vis.orient("sideon", r): the cube is the model's at the visualizer's camera and the view's v_ref,
    and its first moment is the view's v_los map.  The two MODELS (spectral_cube_ref on 64 channels of width 15.3 <= s = 30, and
    kinematics_ref's moments of the oracle's kinematic image) differ on this scene by at most 2.96e-5 in v_los, computed here on the
    CPU (float32 sums of the oracle's image against the cube's float64, and the aliasing of the channels); the bound is that gap,
    formed by the test itself from the two models, plus 1e-5 of the band's width (981.4: 9.8e-3).  Measured: the GPU's cube and
    map differ by 4.95e-5."""
    import topsy_amd
    from kinematic_compare import oracle_kinematic
    from oracle import oracle_np
    vis = topsy_amd.from_arrays(scene["pos"], scene["h"], scene["m"], vel=scene["vel"], render_resolution=R)
    try:
        vis.scale = SCALE
        vis.orient("sideon", 80.0)
        view = topsy_amd.VelocityView(vis, v_ref=V_BULK)
        cube = view.get_cube(sigma_v=30.0)
        maps = view.get_maps()
        rotation = np.asarray(vis.rotation_matrix, dtype=np.float64)
        assert not np.allclose(rotation, np.eye(3))
        M, sf = oracle_np.transform_matrix(rotation, np.asarray(vis.position_offset, dtype=np.float64), vis.scale)
        axis = (rotation[2] / np.sqrt(rotation[2] @ rotation[2])).astype(f32)
        u = kinematics_ref.kinematic_colours(scene["m"], scene["vel"], axis, V_BULK)[3].astype(np.float64)
        V = np.abs(u).max() + 5 * 30.0
        assert cube.n_channels == 64 and cube.v_edges[0] == pytest.approx(-V, rel=1e-6) and cube.v_edges[-1] == pytest.approx(V, rel=1e-6)
        band = dict(v_min=cube.v_min, dv=cube.dv, n_channels=64)
        want, S = model(scene, mips, M, sf, axis, V_BULK, sigma_v=30.0, **band)
        check(cube.data, want, S, "the view's cube")
        # the models' gap in v_los, then the GPU's two answers
        image = oracle_kinematic(scene, mips, M, sf, axis, V_BULK)[0]
        v_model = kinematics_ref.velocity_moments(image)[..., 1].astype(np.float64)
        m1_model = topsy_amd.SpectralCube(want, cube.v_min, cube.dv).moment(1)
        seen = np.isfinite(v_model) & np.isfinite(m1_model)
        assert seen.sum() > R * R // 2 and np.array_equal(np.isfinite(v_model), np.isfinite(m1_model))
        gap = float(np.abs(v_model - m1_model)[seen].max())
        width = cube.v_edges[-1] - cube.v_edges[0]
        m1 = cube.moment(1)
        got_gap = float(np.abs(m1 - maps["v_los"].astype(np.float64))[seen].max())
        print(f"v_los: the models differ by {gap:.3g}, the GPU's cube and map by {got_gap:.3g}; band width {width:.4g}")
        assert np.array_equal(np.isfinite(m1), np.isfinite(maps["v_los"]))
        assert got_gap <= gap + 1e-5 * width
    finally:
        vis.close()
