"""tsp_sphere_moments on the GPU against sphere_moments_reference (test_orient_cpu.py), on that file's scenes, and the orientation
of the view built on it.

Acceptance per scene: n_valid, n_inside and n_inside_vel equal the reference's exactly (membership is bit-determined by the
contract, and test_orient_cpu.py shows that no particle lies within a relative 1e-9 of either sphere's surface); mass and mass_vel
agree to n * 2^-52 relative (sums of positive terms); every component of L within 1e-9 * A_ref, every component of S and of
mass * com within 1e-9 * sum m d2, v_cen within 1e-9 * max |v - v_cen|.  Where the tolerances come from: reordering a float64 sum
of n terms errs by at most about n * 2^-53 of the sum of their magnitudes, 1e-12 at these sizes, whatever the order; one particle
wrongly in or out moves a sum by about 1 / n of it, 1e-4.  So 1e-9 passes every summation order and catches every flip.

On the integer lattice every output but A is exact, so equal to the reference bit for bit in any order.  A is left out of that
claim because it cannot be exact: its terms are products of two square roots, irrational for most lattice points, so each is
rounded and their float64 sum depends on the order; it is a sum of positive terms and is held to n * 2^-52 relative there."""
import ctypes
import re

import numpy as np
import pytest

from test_orient_cpu import (AT, AXIS, R_SPHERE, R_VEL, SCENES, angle_between, blocks_read, lattice_scene, near_tie_margin, reference,
                             scene, sphere_moments_reference)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from topsy_amd import _native
    c = _native.Context(64, 2)
    yield c
    c.close()


def _columns(a):
    return None if a is None else tuple(np.ascontiguousarray(a[:, k]) for k in range(3))


def _call(ctx, pos, mass, vel, **kw):
    return ctx.sphere_moments(pos[:, 0], pos[:, 1], pos[:, 2], mass, vel=_columns(vel), **kw)


def _bits(mo):
    return {k: (np.asarray(v, dtype=np.float64).view(np.uint64).tolist() if not isinstance(v, int) else v) for k, v in mo.items()}


def _accept(label, got, ref):
    n = ref["n_inside"]
    tol_L, tol_S = 1e-9 * ref["A"], 1e-9 * ref["sum_md2"]
    tol_v = 1e-9 * ref["max_u_vel"]
    err_L = np.abs(got["L"] - ref["L"]).max()
    err_S = np.abs(got["S"] - ref["S"]).max()
    err_com = np.abs(got["mass"] * got["com"] - ref["mass"] * ref["com"]).max()
    err_v = np.abs(got["v_cen"] - ref["v_cen"]).max()
    print(f"{label}: valid {got['n_valid']} / {ref['n_valid']}, inside {got['n_inside']} / {ref['n_inside']}, inside r_vel "
          f"{got['n_inside_vel']} / {ref['n_inside_vel']}, |dL| = {err_L:.3g} (tolerance {tol_L:.3g}), |dS| = {err_S:.3g} and "
          f"|d(mass com)| = {err_com:.3g} (tolerance {tol_S:.3g}), |dv_cen| = {err_v:.3g} (tolerance {tol_v:.3g}), "
          f"mass {got['mass']!r} / {ref['mass']!r}, A {got['A']!r} / {ref['A']!r}")
    assert sorted(got) == sorted(k for k in ref if k not in ("sum_md2", "max_u_vel")), label
    for k in ("com", "v_cen", "L"):
        assert got[k].shape == (3,) and got[k].dtype == np.float64
    assert got["S"].shape == (6,)
    assert (got["n_valid"], got["n_inside"], got["n_inside_vel"]) == (ref["n_valid"], ref["n_inside"], ref["n_inside_vel"]), label
    # sums of positive terms: any two orders agree to n * 2^-52 relative
    assert abs(got["mass"] - ref["mass"]) <= n * 2.0 ** -52 * ref["mass"], label
    assert abs(got["mass_vel"] - ref["mass_vel"]) <= max(ref["n_inside_vel"], 1) * 2.0 ** -52 * ref["mass_vel"], label
    assert abs(got["A"] - ref["A"]) <= 1e-9 * ref["A"], label
    assert err_L <= tol_L and err_S <= tol_S and err_com <= tol_S and err_v <= tol_v, label


@pytest.mark.parametrize("name", SCENES)
def test_scene_against_the_reference(ctx, name):
    pos, mass, vel, kw = scene(name)
    assert near_tie_margin(pos, kw["center"], kw["r"], kw["r_vel"]) > 1e-9
    got = _call(ctx, pos, mass, vel, **kw)
    _accept(name, got, reference(name))
    # repeatability: the same call, the same bits
    assert _bits(got) == _bits(_call(ctx, pos, mass, vel, **kw))
    if name == "no_vel":
        assert got["n_inside_vel"] == 0 and got["mass_vel"] == 0.0 and got["A"] == 0.0
        assert not got["L"].any() and not got["v_cen"].any()


@pytest.mark.parametrize("name", ["disc", "disc_sorted", "invalid"])
def test_blocks_outside_a_sphere_are_not_read(ctx, name, monkeypatch, capfd):
    """TOPSY_ORIENT_STATS=1 reports the blocks each pass read: exactly those whose box reaches into the sphere, so in the sorted
    scene fewer than there are, and the sums are the shuffled scene's."""
    pos, mass, vel, kw = scene(name)
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(pos).all(axis=1) & np.isfinite(vel).all(axis=1) & np.isfinite(mass) & (mass > 0)
    monkeypatch.setenv("TOPSY_ORIENT_STATS", "1")
    capfd.readouterr()
    got = _call(ctx, pos, mass, vel, **kw)
    err = capfd.readouterr().err
    print(err)
    nblocks = int(re.search(r" blocks=(\d+) ", err).group(1))
    read = {m.group(1): int(m.group(2)) for m in re.finditer(r"pass=([AB]) kernel_ms=\S+ blocks_read=(\d+)", err)}
    assert nblocks == -(-len(pos) // 1024) == 7 and sorted(read) == ["A", "B"]
    assert re.search(r"upload_ms=\S+ prepare_ms=\S+", err)
    assert read["A"] == blocks_read(pos, valid, kw["center"], kw["r_vel"])
    assert read["B"] == blocks_read(pos, valid, kw["center"], kw["r"])
    if name == "disc_sorted":
        assert read["A"] < nblocks
    else:
        assert read["A"] == read["B"] == nblocks
    _accept(name, got, reference(name))


@pytest.mark.parametrize("order", ["shuffled", "sorted"])
def test_exact_on_the_integer_lattice(ctx, order):
    """Every output except A equals the reference bit for bit (exact sums: the module docstring), and the lattice points at
    distance exactly r or r_vel -- on the face of a block's box when the block is skipped -- are outside."""
    pos, mass, vel, kw = lattice_scene(order)
    ref = sphere_moments_reference(pos, mass, vel, **kw)
    got = _call(ctx, pos, mass, vel, **kw)
    print(f"lattice {order}: inside {got['n_inside']}, inside r_vel {got['n_inside_vel']}, L {got['L']}, A {got['A']!r} / {ref['A']!r}")
    d2 = ((pos.astype(np.float64) - np.asarray(kw["center"])) ** 2).sum(axis=1)
    assert got["n_inside"] == int((d2 < 25).sum()) < int((d2 <= 25).sum())
    assert got["n_inside_vel"] == int((d2 < 9).sum()) < int((d2 <= 9).sum())
    for k in ("n_valid", "n_inside", "n_inside_vel", "mass", "mass_vel"):
        assert got[k] == ref[k], k
    for k in ("com", "v_cen", "L", "S"):
        assert np.array_equal(got[k].view(np.uint64), np.asarray(ref[k], dtype=np.float64).view(np.uint64)), k
    assert abs(got["A"] - ref["A"]) <= ref["n_inside"] * 2.0 ** -52 * ref["A"]
    assert _bits(got) == _bits(_call(ctx, pos, mass, vel, **kw))


def test_python_entries(ctx):
    import topsy_amd
    from topsy_amd import loader
    pos, mass, vel, kw = scene("disc")
    ref = reference("disc")
    got = topsy_amd.sphere_moments(pos, mass, vel, center=AT, radius=R_SPHERE, vel_radius=R_VEL)
    _accept("topsy_amd.sphere_moments", got, ref)
    assert _bits(got) == _bits(_call(ctx, pos, mass, vel, **kw))
    # vel_radius=None: a fifth of the radius (here the same 0.8, formed as 0.2 * 4)
    default = topsy_amd.sphere_moments(pos, mass, vel, center=AT, radius=R_SPHERE)
    _accept("vel_radius=None", default, sphere_moments_reference(pos, mass, vel, center=AT, r=R_SPHERE, r_vel=0.2 * R_SPHERE))
    for orient in ("faceon", "sideon"):
        R, mo = topsy_amd.orientation(pos, mass, vel, center=AT, radius=R_SPHERE, vel_radius=R_VEL, orient=orient)
        _accept(f"topsy_amd.orientation {orient}", mo, ref)
        assert np.abs(R - loader.orientation_matrix(ref, orient, "angmom")).max() <= 1e-9
        axis = R.T @ ([0.0, 0.0, 1.0] if orient == "faceon" else [0.0, 1.0, 0.0])
        assert angle_between(axis, ref["L"]) <= 1e-9 and np.degrees(angle_between(axis, AXIS)) < 0.5
    # without velocities: the shape
    R, mo = topsy_amd.orientation(pos, mass, center=AT, radius=R_SPHERE)
    _accept("topsy_amd.orientation, shape", mo, reference("no_vel"))
    axis = R.T @ [0.0, 0.0, 1.0]
    assert angle_between(axis, loader.orientation_axis(reference("no_vel"), "shape")) <= 1e-9
    assert np.degrees(min(angle_between(axis, AXIS), angle_between(-axis, AXIS))) < 2.0
    R2, _ = topsy_amd.orientation(pos, mass, vel, center=AT, radius=R_SPHERE, method="shape")
    assert np.abs(R2 - R).max() <= 1e-9


def test_works_on_the_multi_gpu_context(ctx):
    from topsy_amd import multigpu
    pos, mass, vel, kw = scene("invalid")
    want = _call(ctx, pos, mass, vel, **kw)
    mg = multigpu.MultiGpuContext(16, 2, [0, 0])
    got = mg.sphere_moments(pos[:, 0], pos[:, 1], pos[:, 2], mass, vel=_columns(vel), **kw)
    mg.close()
    assert _bits(got) == _bits(want)


# ---- errors: TSP_EINVAL, and nothing changes --------------------------------------------------------------------------------
def test_invalid_arguments_change_nothing():
    """The resident scene is 64 particles whose footprints do not overlap, so that two renders of it are the same bit for bit
    (test_gpu_density.py): so must be the renders before and after the refused calls and a good one."""
    from oracle import oracle_np
    from topsy_amd import _native, kernel_lut
    lib = _native.load_library()
    fp = ctypes.POINTER(ctypes.c_float)
    ctx = _native.Context(160, 2)
    ctx.set_kernel_mips(kernel_lut.kernel_mips())
    g = np.arange(-70.0, 71.0, 20.0, dtype=np.float32)
    gx, gy = (v.ravel() for v in np.meshgrid(g, g))
    ctx.upload_particles(gx, gy, np.zeros(64, dtype=np.float32), np.full(64, 3.0, dtype=np.float32), np.ones(64, dtype=np.float32))
    M, sf = oracle_np.transform_matrix(np.eye(3), np.zeros(3), 90.0)

    def render_state():
        ctx.render(M, sf)
        counts = {k: v for k, v in ctx.stats().items() if not k.startswith("ms_")}
        return ctx.read_image(), counts, ctx.download_particles()
    img0, counts0, parts0 = render_state()
    assert np.count_nonzero(img0[..., 0]) > 64 * 20

    pos, mass, vel, kw = scene("one_block")
    n = len(pos)
    x, y, z = _columns(pos)
    vx, vy, vz = _columns(vel)
    m = np.ascontiguousarray(mass)
    P = lambda v: v.ctypes.data_as(fp)                                              # noqa: E731
    D = lambda v: v.ctypes.data_as(ctypes.POINTER(ctypes.c_double))                 # noqa: E731
    center = np.array(kw["center"], dtype=np.float64)
    out = _native.Moments()
    sentinel = bytes([0xA5]) * ctypes.sizeof(out)

    def reset():
        ctypes.memmove(ctypes.byref(out), sentinel, len(sentinel))

    def untouched():
        return bytes(out) == sentinel
    reset()
    good = [n, P(x), P(y), P(z), P(m), P(vx), P(vy), P(vz), D(center), kw["r"], kw["r_vel"], ctypes.byref(out)]

    def but(changes):
        args = list(good)
        for i, v in changes.items():
            args[i] = v
        return tuple(args)
    nan, inf = float("nan"), float("inf")
    zeros = np.zeros(n, dtype=np.float32)
    nans = np.full(n, np.nan, dtype=np.float32)
    far = np.array([1e6, 0.0, 0.0])
    no_vel = {5: None, 6: None, 7: None, 10: 0.0}
    cases = [but({0: 0}), but({0: -5}), but({0: 1 << 31}),
             but({1: None}), but({2: None}), but({3: None}), but({4: None}), but({8: None}), but({11: None}),
             # one or two of the three velocity arrays
             but({5: None}), but({6: None}), but({7: None}), but({5: None, 6: None}), but({5: None, 7: None}), but({6: None, 7: None}),
             but({9: 0.0}), but({9: -1.0}), but({9: nan}), but({9: inf}), but({9: -inf}),
             but({10: kw["r"] * 1.5}), but({10: 0.0}), but({10: -0.5}), but({10: nan}), but({10: inf}),
             # without velocities r_vel must be 0
             but({**no_vel, 10: 0.8}), but({**no_vel, 10: nan}),
             but({8: D(np.array([nan, 0.0, 0.0]))}), but({8: D(np.array([0.0, inf, 0.0]))}), but({8: D(np.array([0.0, 0.0, -inf]))}),
             # no valid particle
             but({4: P(zeros)}), but({1: P(nans)}), but({6: P(nans)}), but({**no_vel, 4: P(nans)})]
    for args in cases:
        assert lib.tsp_sphere_moments(ctx._h, *args) == -1, args            # TSP_EINVAL
        assert args[11] is None or untouched(), args
        assert lib.tsp_last_error()
    assert lib.tsp_sphere_moments(None, *good) == -1 and untouched()
    # an empty sphere: the message names it
    assert lib.tsp_sphere_moments(ctx._h, *but({8: D(far)})) == -1 and untouched()
    assert b"r_vel sphere" in lib.tsp_last_error()
    assert lib.tsp_sphere_moments(ctx._h, *but({**no_vel, 8: D(far)})) == -1 and untouched()
    assert b"the r sphere" in lib.tsp_last_error()
    assert near_tie_margin(pos, center, 1e-4) > 1e-9 and not (((pos.astype(np.float64) - center) ** 2).sum(axis=1) < 1e-8).any()
    assert lib.tsp_sphere_moments(ctx._h, *but({10: 1e-4})) == -1 and untouched()
    assert b"r_vel sphere" in lib.tsp_last_error()

    # the good call on the same context: the reference's answer, r_vel = r allowed, and the resident scene as it was
    assert lib.tsp_sphere_moments(ctx._h, *good) == 0
    _accept("one_block, C call", out.as_dict(), reference("one_block"))
    reset()
    assert lib.tsp_sphere_moments(ctx._h, *but({10: kw["r"]})) == 0
    _accept("one_block, r_vel = r", out.as_dict(), sphere_moments_reference(pos, mass, vel, center=center, r=kw["r"], r_vel=kw["r"]))
    reset()
    assert lib.tsp_sphere_moments(ctx._h, *but(no_vel)) == 0
    _accept("one_block, no velocities", out.as_dict(), sphere_moments_reference(pos, mass, None, center=center, r=kw["r"]))
    reset()
    assert lib.tsp_sphere_moments(ctx._h, *but({0: 1, 8: D(pos[0].astype(np.float64)), 10: 1.0, 9: 1.0})) == 0
    assert (out.n_valid, out.n_inside, out.n_inside_vel, out.mass, out.A) == (1, 1, 1, float(mass[0]), 0.0)
    assert list(out.v_cen) == [float(np.float64(mass[0]) * np.float64(v) / np.float64(mass[0])) for v in vel[0]]
    assert not any(out.L) and not any(out.S) and not any(out.com)
    img1, counts1, parts1 = render_state()
    assert np.array_equal(img0.view(np.uint32), img1.view(np.uint32))
    assert counts0 == counts1
    for k in parts0:
        assert np.array_equal(parts0[k], parts1[k]), k
    ctx.close()


# ---- the product path -----------------------------------------------------------------------------------------------------
SMOOTH, VIEW_SCALE, RES = 0.1, 4.0, 128


def _variant_kwargs(variant):
    kw = dict(render_resolution=RES, with_cells=variant == "with_cells")
    if variant == "two_contexts":
        kw["device_ids"] = [0, 0]
    return kw


def _count_calls(monkeypatch):
    from topsy_amd import _native
    calls = []
    real = _native.Context.sphere_moments
    monkeypatch.setattr(_native.Context, "sphere_moments", lambda self, *a, **k: calls.append(1) or real(self, *a, **k))
    return calls


def _reference_matrix(ld, orient, method="angmom", center=AT, r=R_SPHERE):
    """orientation_matrix of the reference's moments of the loader's own (with cells: reordered) arrays."""
    from topsy_amd import loader
    vel = ld.get_velocities()
    assert near_tie_margin(ld.get_positions(), center, r, 0.2 * r if vel is not None else 0.0) > 1e-9
    mo = sphere_moments_reference(ld.get_positions(), ld.get_mass(), vel, center=center, r=r, r_vel=0.2 * r if vel is not None else 0.0)
    return loader.orientation_matrix(mo, orient, method)


def _moment_ratio(vis):
    """Iyy / Ixx of the rendered density about the image centre (rows are y, columns x)."""
    from topsy_amd.drawreason import DrawReason
    vis.render_sph(DrawReason.EXPORT)
    img = np.asarray(vis.get_sph_image(), dtype=np.float64)
    assert img.shape == (RES, RES) and np.isfinite(img).all() and img.sum() > 0
    c = (np.arange(RES) + 0.5) - RES / 2
    return float((img * c[:, None] ** 2).sum() / (img * c[None, :] ** 2).sum())


@pytest.mark.parametrize("variant", ["plain", "with_cells", "two_contexts"])
def test_from_arrays_opens_face_on(variant, monkeypatch):
    import topsy_amd
    from topsy_amd import loader, visualizer
    pos, mass, vel, _ = scene("disc")
    h = np.full(len(pos), SMOOTH, dtype=np.float32)
    kw = _variant_kwargs(variant)
    calls = _count_calls(monkeypatch)
    vis = topsy_amd.from_arrays(pos, h, mass, vel=vel, center=AT, orient="faceon", orient_radius=R_SPHERE, **kw)
    cached = None
    try:
        ld = vis.data_loader
        R = ld.get_initial_rotation()
        assert len(calls) == 1 and R is ld.get_initial_rotation() and R.dtype == np.float64
        assert np.abs(np.asarray(vis.rotation_matrix) - _reference_matrix(ld, "faceon")).max() <= 1e-9
        assert np.array_equal(vis.rotation_matrix, R) and np.array_equal(vis.position_offset, -AT)
        assert np.degrees(angle_between(R.T @ [0.0, 0.0, 1.0], AXIS)) < 0.5
        assert ld.orient_moments["n_inside"] == reference("disc")["n_inside"]
        # face-on the disc is round
        vis.scale = VIEW_SCALE
        assert 0.8 < _moment_ratio(vis) < 1.25 and len(calls) == 1
        assert np.array_equal(vis.rotation_matrix, R)

        # a rotation from the caller's cache: nothing is computed, the same view
        class Cached(loader.ArrayDataLoader):
            def __init__(self, device, **kwargs):
                super().__init__(device, **kwargs)
                self.set_initial_rotation(R)
        cached = visualizer.Visualizer(data_loader_class=Cached, render_resolution=RES, device_ids=kw.get("device_ids"),
                                       data_loader_kwargs=dict(pos=pos, smooth=h, mass=mass, vel=vel, center=AT, orient="faceon",
                                                               orient_radius=R_SPHERE, with_cells=kw["with_cells"]))
        assert np.array_equal(cached.rotation_matrix, R) and len(calls) == 1
    finally:
        for v in (vis, cached):
            if v is not None:
                v.close()


@pytest.mark.parametrize("variant", ["plain", "with_cells", "two_contexts"])
def test_side_on_flattens_the_image(variant, monkeypatch):
    """The mass-weighted second moments of the rendered density about the image centre: edge-on the disc lies along x, so
    Iyy / Ixx < 0.3; unoriented it is above 0.6.  The CPU oracle's render of this scene (128 px, smooth 0.1, scale 4) gives 0.125
    and 0.877; the particle positions alone inside the window 0.133 and 0.873.  The bounds sit between, about the midpoint."""
    import topsy_amd
    pos, mass, vel, _ = scene("disc")
    h = np.full(len(pos), SMOOTH, dtype=np.float32)
    kw = _variant_kwargs(variant)
    calls = _count_calls(monkeypatch)
    side = topsy_amd.from_arrays(pos, h, mass, vel=vel, center=AT, orient="sideon", orient_radius=R_SPHERE, **kw)
    plain = None
    try:
        assert np.abs(np.asarray(side.rotation_matrix) - _reference_matrix(side.data_loader, "sideon")).max() <= 1e-9
        assert np.degrees(angle_between(np.asarray(side.rotation_matrix).T @ [0.0, 1.0, 0.0], AXIS)) < 0.5
        side.scale = VIEW_SCALE
        ratio_side = _moment_ratio(side)
        assert len(calls) == 1
        plain = topsy_amd.from_arrays(pos, h, mass, vel=vel, center=AT, orient="none", **kw)
        assert np.array_equal(plain.rotation_matrix, np.eye(3)) and len(calls) == 1
        plain.scale = VIEW_SCALE
        ratio_plain = _moment_ratio(plain)
        print(f"{variant}: Iyy / Ixx side-on {ratio_side:.4f}, unoriented {ratio_plain:.4f}")
        assert ratio_side < 0.3 and ratio_plain > 0.6
    finally:
        for v in (side, plain):
            if v is not None:
                v.close()


def test_vis_orient(monkeypatch):
    import topsy_amd
    from topsy_amd import _native
    pos, mass, vel, _ = scene("disc")
    h = np.full(len(pos), SMOOTH, dtype=np.float32)
    calls = _count_calls(monkeypatch)
    vis = topsy_amd.from_arrays(pos, h, mass, vel=vel, center=AT, render_resolution=RES)
    nov = other = None
    try:
        assert np.array_equal(vis.rotation_matrix, np.eye(3)) and not calls
        # the same matrix as the load-time path (the same call: the same bits)
        R = vis.orient("faceon", R_SPHERE)
        assert len(calls) == 1 and np.array_equal(vis.rotation_matrix, R)
        assert np.abs(R - _reference_matrix(vis.data_loader, "faceon")).max() <= 1e-9
        load_time = topsy_amd.from_arrays(pos, h, mass, vel=vel, center=AT, orient="faceon", orient_radius=R_SPHERE,
                                          render_resolution=RES)
        try:
            assert np.array_equal(load_time.rotation_matrix, R)
        finally:
            load_time.close()
        vis.scale = VIEW_SCALE
        assert 0.8 < _moment_ratio(vis) < 1.25
        # side-on, through the surface view, about an explicit centre: the visualizer's camera
        view = topsy_amd.SurfaceView(vis)
        S = view.orient("sideon", R_SPHERE, center=AT)
        assert np.array_equal(vis.rotation_matrix, S) and np.array_equal(S, vis.orient("sideon", R_SPHERE))
        assert np.abs(S - _reference_matrix(vis.data_loader, "sideon")).max() <= 1e-9
        assert _moment_ratio(vis) < 0.3
        # center=None follows the view: away from the disc the sphere is empty, back on it the matrix returns
        vis.position_offset = -(AT + [50.0, 0.0, 0.0])
        with pytest.raises(_native.BackendError, match="sphere"):
            vis.orient("faceon", 1.0)
        assert np.array_equal(vis.rotation_matrix, S)
        vis.position_offset = -AT
        assert np.array_equal(vis.orient("faceon", R_SPHERE), R)
        with pytest.raises(ValueError, match="upward"):
            vis.orient("upward", R_SPHERE)
        with pytest.raises(ValueError, match="radius"):
            vis.orient("faceon", -1.0)

        # the shape method on a snapshot without velocities; angmom is refused there
        nov = topsy_amd.from_arrays(pos, h, mass, center=AT, render_resolution=RES)
        with pytest.raises(ValueError, match="angmom"):
            nov.orient("faceon", R_SPHERE, method="angmom")
        Rs = nov.orient("faceon", R_SPHERE, method="shape")
        axis = Rs.T @ [0.0, 0.0, 1.0]
        assert np.degrees(min(angle_between(axis, AXIS), angle_between(-axis, AXIS))) < 2.0
        assert np.abs(Rs - _reference_matrix(nov.data_loader, "faceon", "shape")).max() <= 1e-9
        assert np.array_equal(nov.orient("faceon", R_SPHERE), Rs)          # without vel the default is the shape
        # another loader has no host arrays to orient by
        other = topsy_amd.test(1000, render_resolution=64)
        with pytest.raises(ValueError, match="TestDataLoader"):
            other.orient("faceon", 10.0)
        assert np.array_equal(other.rotation_matrix, np.eye(3))
    finally:
        for v in (vis, nov, other):
            if v is not None:
                v.close()


def test_orients_on_a_halo_centre():
    """The orientation is taken about whatever center= produced: here the shrinking-sphere centre of the largest
    friends-of-friends halo, which is the disc."""
    import topsy_amd
    pos, mass, vel, _ = scene("disc")
    h = np.full(len(pos), SMOOTH, dtype=np.float32)
    vis = topsy_amd.from_arrays(pos, h, mass, vel=vel, halos={"linking_length": 0.25}, center="halo-1", orient="faceon",
                                orient_radius=R_SPHERE, render_resolution=64)
    try:
        centre = vis.data_loader.get_initial_center()
        assert np.linalg.norm(centre - AT) < 0.3 and np.array_equal(vis.position_offset, -centre)
        want = _reference_matrix(vis.data_loader, "faceon", center=centre)
        assert np.abs(np.asarray(vis.rotation_matrix) - want).max() <= 1e-9
        assert np.degrees(angle_between(np.asarray(vis.rotation_matrix).T @ [0.0, 0.0, 1.0], AXIS)) < 1.0
    finally:
        vis.close()
