"""tsp_shrink_sphere_center on the GPU against shrink_sphere_reference (test_center_cpu.py), on that file's scenes.

Acceptance: iterations, n_valid and n_inside equal the reference's exactly and |c_gpu - c_ref| <= 1e-9 * radius_final per axis.
The float64 summation error is at most N * 2^-53 * r (1e-11 r at these sizes) whatever the order of the sums, and a single
particle changing sides moves the centre by at least r / N (1e-5 r): 1e-9 passes every summation order and catches every flip.
test_center_cpu.py shows that no particle of these scenes lies within a relative 1e-9 of any trial radius, so the rounding of
the centre cannot flip a membership either.  Then: the trace step by step, the exact lattice, repeatability, argument errors
that change nothing, the product path (from_arrays(center=...)) and centre_on_pixel."""
import ctypes

import numpy as np
import pytest

from test_center_cpu import (CLUMP_AT, SCENES, ZOOM_CUT, lattice_scene, near_tie_margin, reference, scene,
                             shrink_sphere_reference)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from topsy_amd import _native
    c = _native.Context(64, 2)
    yield c
    c.close()


def _call(ctx, pos, mass, **kw):
    return ctx.shrink_sphere_center(pos[:, 0], pos[:, 1], pos[:, 2], mass, **kw)


def _accept(label, got, want):
    (c, info), (c_ref, info_ref) = got, want
    tol = 1e-9 * info_ref["radius"]
    err = np.abs(c - c_ref)
    print(f"{label}: iterations {info['iterations']} / {info_ref['iterations']}, inside {info['n_inside']} / {info_ref['n_inside']}, "
          f"valid {info['n_valid']} / {info_ref['n_valid']}, |dc| = {err.max():.3g} (tolerance {tol:.3g}), "
          f"radius {info['radius']!r} / {info_ref['radius']!r}")
    assert c.dtype == np.float64 and c.shape == (3,)
    assert info["iterations"] == info_ref["iterations"], label
    assert info["n_valid"] == info_ref["n_valid"] and info["n_inside"] == info_ref["n_inside"], label
    assert info["radius"] == info_ref["radius"], label            # the same products of the same two numbers
    assert (err <= tol).all(), (label, c, c_ref)
    # a sum of n positive terms: any two orders agree to n * 2^-52 relative
    assert abs(info["mass_inside"] - info_ref["mass_inside"]) <= info_ref["n_inside"] * 2.0 ** -52 * info_ref["mass_inside"], label


@pytest.mark.parametrize("name", SCENES)
def test_scene_against_the_reference(ctx, name):
    pos, mass, kw = scene(name)
    c_ref, info_ref, trace = reference(name)
    assert near_tie_margin(pos, mass, trace, kw.get("mass_cut_factor", 0.0)) > 1e-9
    got = _call(ctx, pos, mass, **kw)
    _accept(name, got, (c_ref, info_ref))
    # repeatability: the same call, the same bits
    again = _call(ctx, pos, mass, **kw)
    assert np.array_equal(got[0].view(np.uint64), again[0].view(np.uint64)) and got[1] == again[1]
    if name == "duplicates":
        assert got[1]["iterations"] == 256 and np.array_equal(got[0], np.float64([0.5078125, 0.49609375, 0.50390625]))
    if name == "too_few":
        assert got[1]["iterations"] == 0 and got[1]["n_inside"] == got[1]["n_valid"] == 60
    if name == "zoom":
        assert np.linalg.norm(got[0] - [0.25, 0.62, 0.4]) < 0.005
    if name == "zoom_all":
        assert np.linalg.norm(got[0] - CLUMP_AT) < 0.005


@pytest.mark.parametrize("name", ["clump_sorted", "invalid"])
def test_trace_step_by_step(ctx, name):
    pos, mass, kw = scene(name)
    _, info_full, trace = reference(name)
    assert near_tie_margin(pos, mass, trace, kw.get("mass_cut_factor", 0.0)) > 1e-9
    for k in range(0, info_full["iterations"] + 2):
        want = shrink_sphere_reference(pos, mass, max_iterations=k, **kw)
        assert want[1]["iterations"] == min(k, info_full["iterations"])
        assert np.array_equal(want[0], trace[min(k, len(trace) - 1)][0])
        _accept(f"{name}, max_iterations = {k}", _call(ctx, pos, mass, max_iterations=k, **kw), want[:2])


@pytest.mark.parametrize("order", ["shuffled", "sorted"])
def test_exact_boundary_on_the_integer_lattice(ctx, order):
    """Every sum is exact, so the centre stays (0, 0, 0) bit for bit, and the points at distance exactly r_try (on the face of a
    block's box when the block is skipped) are outside."""
    pos, mass = lattice_scene(order)
    p2 = (pos.astype(np.float64) ** 2).sum(axis=1)
    for k, bound in ((1, 16), (2, 4), (3, 1)):
        c, info = _call(ctx, pos, mass, r_start=8.0, shrink_factor=0.5, min_particles=1, max_iterations=k)
        print(f"lattice {order}, {k} iterations: inside {info['n_inside']}, centre {c}")
        assert np.array_equal(c, np.zeros(3)), c
        assert info["iterations"] == k and info["radius"] == 8.0 * 0.5 ** k and info["n_valid"] == 13 ** 3
        assert info["n_inside"] == int((p2 < bound).sum()) and info["mass_inside"] == float(info["n_inside"])
    assert int((p2 < 16).sum()) < int((p2 <= 16).sum())


def test_r_start_and_the_python_entry(ctx):
    import topsy_amd
    pos, mass, _ = scene("offset")
    want = shrink_sphere_reference(pos, mass, r_start=0.3, shrink_factor=0.8, min_particles=200)
    _accept("offset, r_start", _call(ctx, pos, mass, r_start=0.3, shrink_factor=0.8, min_particles=200), want[:2])
    got = topsy_amd.shrink_sphere_center(pos, mass, r_start=0.3, shrink_factor=0.8, min_particles=200)
    _accept("offset, topsy_amd.shrink_sphere_center", got, want[:2])
    pos, mass, _ = scene("zoom")
    got = topsy_amd.shrink_sphere_center(pos, mass, select="zoom")
    _accept("zoom, topsy_amd.shrink_sphere_center", got, reference("zoom")[:2])
    assert got[1] == _call(ctx, pos, mass, mass_cut_factor=ZOOM_CUT)[1]


def test_works_on_the_multi_gpu_context(ctx):
    from topsy_amd import multigpu
    pos, mass, kw = scene("zoom")
    want = _call(ctx, pos, mass, **kw)
    mg = multigpu.MultiGpuContext(16, 2, [0, 0])
    got = mg.shrink_sphere_center(pos[:, 0], pos[:, 1], pos[:, 2], mass, **kw)
    mg.close()
    assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)) and got[1] == want[1]


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

    pos, mass, _ = scene("offset")
    n = len(pos)
    x, y, z = (np.ascontiguousarray(pos[:, a]) for a in range(3))
    m = np.ascontiguousarray(mass)
    center = np.full(3, 7.0)
    info = _native.CenterInfo(-1, -2, -3, -4, -5.0, -6.0)
    P = lambda v: v.ctypes.data_as(fp)                                              # noqa: E731
    C = center.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    good = [n, P(x), P(y), P(z), P(m), 0.0, 0.0, 0.7, 100, 256, C, ctypes.byref(info)]

    def untouched():
        return ((center == 7.0).all() and (info.n_valid, info.n_inside, info.iterations, info.reserved, info.radius,
                                           info.mass_inside) == (-1, -2, -3, -4, -5.0, -6.0))

    def but(i, v):
        args = list(good)
        args[i] = v
        return tuple(args)
    nan, inf = float("nan"), float("inf")
    bad_mass = np.zeros(n, dtype=np.float32)
    bad_x = np.full(n, np.nan, dtype=np.float32)
    cases = [but(0, 0), but(0, -5), but(0, 1 << 31), but(1, None), but(2, None), but(3, None), but(4, None), but(10, None),
             but(7, 0.0), but(7, 1.0), but(7, -0.5), but(7, 1.5), but(7, nan), but(8, 0), but(8, -3), but(9, -1), but(9, 257),
             but(6, -1.0), but(6, nan), but(6, inf), but(6, -inf), but(5, 1.0), but(5, 0.5), but(5, -2.0), but(5, nan), but(5, inf),
             but(4, P(bad_mass)), but(1, P(bad_x)), but(5, 1.01)[:4] + (P(bad_mass),) + but(5, 1.01)[5:]]
    for args in cases:
        assert lib.tsp_shrink_sphere_center(ctx._h, *args) == -1, args          # TSP_EINVAL
        assert untouched(), args
        assert lib.tsp_last_error()
    assert lib.tsp_shrink_sphere_center(None, *good) == -1 and untouched()

    # the good call on the same context: the reference's answer, an optional info, and the resident scene as it was
    assert lib.tsp_shrink_sphere_center(ctx._h, *good) == 0
    c_ref, info_ref, _ = reference("offset")
    assert info.iterations == info_ref["iterations"] and info.n_inside == info_ref["n_inside"] and info.reserved == 0
    assert (np.abs(center - c_ref) <= 1e-9 * info_ref["radius"]).all()
    first = center.copy()
    center[:] = 7.0
    assert lib.tsp_shrink_sphere_center(ctx._h, *but(11, None)) == 0 and np.array_equal(center, first)
    assert lib.tsp_shrink_sphere_center(ctx._h, *but(0, 1)) == 0 and np.array_equal(center, pos[0].astype(np.float64))
    img1, counts1, parts1 = render_state()
    assert np.array_equal(img0.view(np.uint32), img1.view(np.uint32))
    assert counts0 == counts1
    for k in parts0:
        assert np.array_equal(parts0[k], parts1[k]), k
    ctx.close()


# ---- the product path -----------------------------------------------------------------------------------------------------
def _blob_snapshot():
    """A compact blob far from the origin of a thin uniform box: the blob is the brightest pixel wherever it is drawn."""
    rs = np.random.RandomState(31)
    at = np.array([6.0, -4.0, 3.0])
    pos = np.concatenate([rs.uniform(-10.0, 10.0, size=(3000, 3)), at + rs.normal(scale=0.05, size=(3 * 1024 + 17, 3))])
    pos = pos[rs.permutation(len(pos))].astype(np.float32)
    return pos, np.full(len(pos), 0.15, dtype=np.float32), np.ones(len(pos), dtype=np.float32), at


def _brightest(vis):
    from topsy_amd.drawreason import DrawReason
    vis.render_sph(DrawReason.EXPORT)
    img = np.asarray(vis.get_sph_image())
    return np.unravel_index(int(np.argmax(img)), img.shape)


def _near_image_centre(pixel, res):
    """Within one pixel of the image centre (the corner shared by the four middle pixels of an even image)."""
    return all(abs(p + 0.5 - res / 2) <= 1.0 for p in pixel)


@pytest.mark.parametrize("variant", ["plain", "with_cells", "two_contexts"])
def test_from_arrays_opens_on_the_centre(variant, monkeypatch):
    import topsy_amd
    from topsy_amd import _native
    pos, h, mass, at = _blob_snapshot()
    res = 128
    kw = dict(render_resolution=res, with_cells=variant == "with_cells")
    if variant == "two_contexts":
        kw["device_ids"] = [0, 0]
    calls = []
    real = _native.Context.shrink_sphere_center
    monkeypatch.setattr(_native.Context, "shrink_sphere_center", lambda self, *a, **k: calls.append(1) or real(self, *a, **k))
    vis = topsy_amd.from_arrays(pos, h, mass, center="all", **kw)
    plain = cached = None
    try:
        ld = vis.data_loader
        centre = ld.get_initial_center()
        assert len(calls) == 1 and centre is ld.get_initial_center() and centre.dtype == np.float64
        # the centre of the loader's own (with cells: reordered) arrays, which is the caller's up to rounding
        want = shrink_sphere_reference(ld.get_positions(), ld.get_mass())
        assert near_tie_margin(ld.get_positions(), ld.get_mass(), want[2]) > 1e-9
        assert (np.abs(centre - want[0]) <= 1e-9 * want[1]["radius"]).all() and ld.center_info["iterations"] == want[1]["iterations"]
        assert np.allclose(centre, shrink_sphere_reference(pos, mass)[0], rtol=0, atol=1e-9)
        assert np.linalg.norm(centre - at) < 0.05
        assert np.array_equal(vis.position_offset, -centre)
        vis.scale = 10.0
        assert _near_image_centre(_brightest(vis), res)
        assert np.array_equal(vis.position_offset, -centre) and len(calls) == 1

        plain = topsy_amd.from_arrays(pos, h, mass, center="none", **kw)
        assert np.array_equal(plain.position_offset, np.zeros(3)) and len(calls) == 1
        plain.scale = 10.0
        row, col = _brightest(plain)
        assert not _near_image_centre((row, col), res)
        assert abs(col + 0.5 - (at[0] / 10.0 + 1.0) * res / 2) <= 1.0 and abs(row + 0.5 - (1.0 - at[1] / 10.0) * res / 2) <= 1.0

        # a centre from the caller's cache: nothing is computed, the same view
        loader_kwargs = dict(pos=pos, smooth=h, mass=mass, center="all", with_cells=variant == "with_cells")
        from topsy_amd import loader, visualizer

        class Cached(loader.ArrayDataLoader):
            def __init__(self, device, **kwargs):
                super().__init__(device, **kwargs)
                self.set_initial_center(centre)
        cached = visualizer.Visualizer(data_loader_class=Cached, data_loader_kwargs=loader_kwargs, render_resolution=res,
                                       device_ids=kw.get("device_ids"))
        assert np.array_equal(cached.position_offset, -centre) and len(calls) == 1
    finally:
        for v in (vis, plain, cached):
            if v is not None:
                v.close()


def test_from_arrays_zoom(monkeypatch):
    import topsy_amd
    pos, mass, _ = scene("zoom")
    h = np.full(len(pos), 0.01, dtype=np.float32)
    vis = topsy_amd.from_arrays(pos, h, mass, center="zoom", render_resolution=64)
    try:
        c_ref, info_ref, _ = reference("zoom")
        assert (np.abs(vis.data_loader.get_initial_center() - c_ref) <= 1e-9 * info_ref["radius"]).all()
        assert np.array_equal(vis.position_offset, -vis.data_loader.get_initial_center())
    finally:
        vis.close()


@pytest.mark.parametrize("view", ["visualizer", "surface"])
def test_centre_on_pixel(view):
    import topsy_amd
    rs = np.random.RandomState(41)
    at = np.array([3.0, -2.0, 1.5])
    smooth = 0.2
    pos = (at + rs.normal(scale=0.02, size=(500, 3))).astype(np.float32)
    res = 128
    vis = topsy_amd.from_arrays(pos, np.full(len(pos), smooth, dtype=np.float32), np.ones(len(pos), dtype=np.float32),
                                render_resolution=res)
    try:
        vis.scale = 8.0
        pixel_width = 2 * 8.0 / res
        target = topsy_amd.SurfaceView(vis) if view == "surface" else vis
        row, col = _brightest(vis)
        assert not _near_image_centre((row, col), res)
        offset = target.centre_on_pixel(row, col)
        assert np.array_equal(offset, vis.position_offset)
        print(f"{view}: pixel ({row}, {col}) -> offset {offset}")
        assert abs(offset[0] + at[0]) <= pixel_width and abs(offset[1] + at[1]) <= pixel_width
        assert abs(offset[2] + at[2]) <= smooth
        assert _near_image_centre(_brightest(vis), res)
        # an empty pixel has no depth: x and y move, z stays
        depth = vis.get_depth_image()
        assert np.isnan(depth[3, 5]) and np.isfinite(depth[res // 2, res // 2])
        before = np.array(vis.position_offset, copy=True)
        after = target.centre_on_pixel(3, 5)
        shift = after - before
        assert shift[2] == 0.0
        assert abs(shift[0] + ((5 + 0.5) * 2 / res - 1) * 8.0) < 1e-12 and abs(shift[1] + (1 - (3 + 0.5) * 2 / res) * 8.0) < 1e-12
        # a rotated view: the clicked point still comes to the centre
        vis.position_offset = -at + np.array([1.0, 2.0, 0.5])
        vis.rotate(0.4, -0.3)
        row, col = _brightest(vis)
        assert not _near_image_centre((row, col), res)
        offset = target.centre_on_pixel(row, col)
        assert _near_image_centre(_brightest(vis), res)
        assert np.linalg.norm(offset + at) <= np.hypot(smooth, 2 * pixel_width)
        with pytest.raises(ValueError, match="128"):
            target.centre_on_pixel(res, 0)
    finally:
        vis.close()
