"""SPH fields on a lattice (no GPU): the brute force of lattice_ref.py, which the GPU tests (test_gpu_lattice.py) hold
tsp_sph_sample_lattice to, pinned against the particle brute forces and a lattice sum, and the host layer: the lattices of
sph_grid / sph_slice / sph_ray / get_slice_image, their argument checks, and a restatement of the library's brick order."""
import ctypes
import types

import numpy as np
import pytest

import lattice_ref
from test_smoothing_cpu import _cloud, _no_gpu, brute_force_smoothing

f32 = np.float32
EPS = 2.0 ** -24           # half a float32 ulp, relative: the rounding of one float32 operation


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


# ---- the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("period", [0.0, 12.0])
@pytest.mark.parametrize("k", [8, 33])
def test_h_at_points_that_are_particles_is_the_particles_h(k, period):
    """A lattice point that coincides with a particle sees the distances that particle sees (itself at 0 included), so h there
    is tsp_smoothing_lengths' h of the particle, bit for bit.  Integer coordinates: the lattice points are exact."""
    rs = np.random.RandomState(3)
    cells = rs.choice(12 ** 3, 500, replace=False)
    pos = np.stack([cells % 12, (cells // 12) % 12, cells // 144], axis=1).astype(f32)
    h, _ = lattice_ref.sample_lattice(pos, [np.ones(len(pos), dtype=f32)], k, period, (0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1),
                                      (12, 12, 12))
    want = brute_force_smoothing(pos, k, period=period)
    i, j, kk = (pos[:, a].astype(int) for a in range(3))
    assert np.array_equal(_bits(h[kk, j, i]), _bits(want))
    assert np.isfinite(h).all() and (h > 0).all()


def test_points_follow_the_float64_then_float32_rule():
    o, du, dv, dw = (0.1, -3.0, 1e-3), (1.0 / 3.0, 0.0, 1e-9), (0.0, 0.7, 0.0), (1e-5, 0.0, 2.0)
    pts = lattice_ref.lattice_points(o, du, dv, dw, (5, 3, 2))
    assert pts.shape == (2, 3, 5, 3) and pts.dtype == f32
    for (i, j, k) in [(0, 0, 0), (4, 2, 1), (3, 1, 0)]:
        want = [f32(((o[a] + float(i) * du[a]) + float(j) * dv[a]) + float(k) * dw[a]) for a in range(3)]
        assert np.array_equal(_bits(pts[k, j, i]), _bits(want))


def _epstein_zeta5(G=40):
    """sum over the non-zero integer vectors g of |g|^-5, from above: the terms with every |g_a| <= G and a bound of the rest."""
    g = np.arange(-G, G + 1, dtype=np.float64)
    r2 = g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2
    r2[G, G, G] = np.inf
    head = (r2 ** -2.5).sum()
    # a vector g outside has |g| >= G + 1, and every x of its unit cube has |x| <= |g| + c, c = sqrt(3) / 2, and |x| >= R = G + 0.5:
    # |g|^-5 <= (|x| - c)^-5, r^2 <= (R / (R - c))^2 (r - c)^2 for r >= R, so the rest is below the integral
    # 4 pi (R / (R - c))^2 int_R^inf (r - c)^-3 dr = 4 pi (R / (R - c))^2 / (2 (R - c)^2)
    R, c = G + 0.5, np.sqrt(3.0) / 2.0
    return head + 4.0 * np.pi * (R / (R - c)) ** 2 / (2.0 * (R - c) ** 2)


@pytest.mark.parametrize("k", [33, 64])
def test_density_of_a_cubic_lattice_is_one_within_the_discreteness_bound(k):
    """Unit masses on the integer points of a periodic box: the density at a cell centre is sum_n f(n + s), f = W(|x| / h) /
    (pi h^3), whose integral is 1.  By Poisson's formula the sum is 1 + sum_{g != 0} fhat(g) e^(2 pi i g s) with
    fhat(g) = (4 / kappa) int_0^2 G(u) sin(kappa u) du, G(u) = u w(u), kappa = 2 pi |g| h.  G, G' and G'' are continuous and
    vanish at 0 and 2 where the parts need it (G(0) = G(2) = 0, G'(2) = 0, sin(0) = 0, G''(0) = G''(2) = 0), so three
    integrations by parts leave -(1 / kappa^3) int G''' cos, and one more bounds that by (jumps of G''' + int |G''''|) / kappa^4:
    G''' = -9 + 18 u on [0, 1) and 9 - 6 u on [1, 2), so the jump terms are |9 - 3| + |-3| = 9 and int |G''''| = 18 + 6 = 24.
    Hence |fhat(g)| <= 4 * 33 / kappa^5 and |rho - 1| <= 132 Z / (2 pi h)^5 with Z = sum_{g != 0} |g|^-5 (about 10.4).
    h follows from the geometry: the particles lie at distances sqrt(3)/2 (8 of them), sqrt(11)/2 (24), sqrt(19)/2 (24) and
    sqrt(27)/2 (32) from a cell centre, so the 33rd is at sqrt(19)/2 and the 64th at sqrt(27)/2.  The bound is 9.1 % at
    k = 33 and 3.8 % at k = 64 (the values are 1.0058 and 1.0044); the float32 rounding of the terms is 1e-7 of that."""
    n = 12
    g = np.arange(n, dtype=f32)
    pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    h, outs = lattice_ref.sample_lattice(pos, [np.ones(len(pos), dtype=f32)], k, float(n), (0.5, 0.5, 0.5), (3, 0, 0), (0, 4, 0),
                                         (0, 0, 5), (4, 3, 2))
    h_geometry = 0.5 * np.sqrt({33: 19.0, 64: 27.0}[k]) / 2.0
    assert np.allclose(h, h_geometry, rtol=2 * EPS, atol=0)
    bound = 132.0 * _epstein_zeta5() / (2.0 * np.pi * h_geometry) ** 5
    print(f"k={k}: h={h_geometry:.4f} rho in [{outs.min():.6f}, {outs.max():.6f}], bound {bound:.4f}")
    assert 0.03 < bound < 0.1
    assert (np.abs(outs[0].astype(np.float64) - 1.0) <= bound + 1e-5).all()


def test_mean_of_a_constant_is_the_constant():
    """mean = S0 / S1 with the float32 terms (m c) w and m w, all positive: a term of S0 is c times the term of S1 to three
    roundings (m c, its product with w, m w), the float64 sums add nothing at this level, each sum is rounded to float32 once
    and so is the quotient: |mean / c - 1| <= 6 * 2^-24 (and the second order of that)."""
    from topsy_amd import lattice
    pos = _cloud(1500, 11)
    mass = np.random.RandomState(2).uniform(0.5, 2.0, len(pos)).astype(f32)
    c = f32(37.25)
    spec, _ = lattice.box_lattice((5, 4, 3), (0.1, 0.0, -0.2), 1.5)
    out = lattice.sample(lattice_ref.ReferenceContext(), pos, mass, np.full(len(pos), c, dtype=f32), 16, 0.0, spec)
    assert out["mean"].shape == out["rho"].shape == out["smooth"].shape == (3, 4, 5) and out["mean"].dtype == f32
    assert (out["rho"] > 0).all()
    assert (np.abs(out["mean"].astype(np.float64) / float(c) - 1.0) <= 6.5 * EPS).all()


def test_mean_is_nan_where_rho_is_zero_or_nan():
    from topsy_amd import lattice
    pos = np.zeros((40, 3), dtype=f32)
    pos[32:] = np.arange(1, 9, dtype=f32)[:, None]
    spec = {"origin": (0, 0, 0), "du": (0.5, 0.5, 0.5), "dv": (0, 0, 0), "dw": (0, 0, 0), "shape": (3, 1, 1)}
    out = lattice.sample(lattice_ref.ReferenceContext(), pos, np.ones(40, dtype=f32), np.ones(40, dtype=f32), 32, 0.0, spec)
    assert out["smooth"][0, 0, 0] == 0 and np.isnan(out["rho"][0, 0, 0]) and np.isnan(out["mean"][0, 0, 0])
    # the second point is equally far from the 32 particles at the origin and from the one at (1, 1, 1): all 33 sit at u = 2
    assert out["smooth"][0, 0, 1] > 0 and out["rho"][0, 0, 1] == 0 and np.isnan(out["mean"][0, 0, 1])
    assert out["rho"][0, 0, 2] > 0 and out["mean"][0, 0, 2] == 1


# ---- the brick order ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 3, 2), (1, 1, 1), (9, 1, 1), (70, 1, 1), (17, 13, 1), (8, 8, 8), (1, 5, 7), (3, 1, 2)])
def test_brick_order_is_a_bijection(shape):
    """lattice_ref.brick_order restates lattice_slot() of tsp_smooth.hip: every lattice point has exactly one unmasked slot."""
    ijk, inside = lattice_ref.brick_order(shape)
    nu, nv, nw = shape
    assert len(ijk) % 64 == 0 and inside.sum() == nu * nv * nw and (ijk >= 0).all()
    lin = (ijk[inside, 2] * nv + ijk[inside, 1]) * nu + ijk[inside, 0]
    assert np.array_equal(np.sort(lin), np.arange(nu * nv * nw))
    bu, bv, bw = lattice_ref.brick_shape(shape)
    assert bu * bv * bw == 64 and (bu, bv, bw) == ((64, 1, 1) if nv == nw == 1 else (8, 8, 1) if nw == 1 else (4, 4, 4))
    # the 64 slots of a brick are neighbours in space: they span at most the brick
    for b in range(len(ijk) // 64):
        span = ijk[64 * b:64 * b + 64].max(axis=0) - ijk[64 * b:64 * b + 64].min(axis=0)
        assert (span == np.array([bu, bv, bw]) - 1).all()


# ---- the lattices of the host layer ------------------------------------------------------------------------------------------
def test_box_lattice_samples_cell_centres():
    from topsy_amd import lattice
    rot = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    spec, (u, v, w) = lattice.box_lattice((4, 2, 1), (10.0, 20.0, 30.0), (8.0, 2.0, 6.0), rot)
    assert np.allclose(u, [-3, -1, 1, 3]) and np.allclose(v, [-0.5, 0.5]) and np.allclose(w, [0.0])
    pts = lattice_ref.lattice_points(**spec)
    assert pts.shape == (1, 2, 4, 3)
    want = np.array([10.0, 20.0, 30.0]) + u[3] * rot[0] + v[1] * rot[1] + w[0] * rot[2]
    assert np.allclose(pts[0, 1, 3], want)
    spec1, offs = lattice.box_lattice((3, 3, 3), (0, 0, 0), 3.0)
    assert all(np.allclose(o, [-1, 0, 1]) for o in offs) and np.allclose(spec1["origin"], [-1, -1, -1])


def test_slice_lattice_is_centre_on_pixels_convention():
    """Pixel (row, col) of the slice is the point the view would be centred on after centre_on_pixel(row, col) at zero depth:
    minus the new position_offset, by the arithmetic of Visualizer.centre_on_pixel."""
    from topsy_amd import lattice
    a, b = 0.4, -0.7
    rot = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) @ \
        np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    offset, scale, res = np.array([1.5, -2.0, 0.25]), 7.0, 32
    spec = lattice.slice_lattice(rot, offset, scale, res)
    assert spec["shape"] == (res, res, 1)
    pts = lattice_ref.lattice_points(**spec)[0].astype(np.float64)
    for row, col in [(0, 0), (31, 31), (5, 20), (16, 15)]:
        view = np.array([((col + 0.5) * 2.0 / res - 1.0) * scale, (1.0 - (row + 0.5) * 2.0 / res) * scale, 0.0])
        new_offset = offset - rot.T @ view
        assert np.allclose(pts[row, col], -new_offset, rtol=0, atol=1e-5)


# ---- the host layer refuses bad arguments before any GPU call ----------------------------------------------------------------
def _particles(n=200):
    return _cloud(n, 1), np.ones(n, dtype=f32)


@pytest.mark.parametrize("kw, match", [
    (dict(size=None), "size"), (dict(size=0.0), "size"), (dict(size=np.nan), "size"), (dict(size=(1.0, 2.0)), "size"),
    (dict(size=(1.0, -2.0, 1.0)), "size"), (dict(size="big"), "size"),
    (dict(shape=(4, 4)), "shape"), (dict(shape=(4, 0, 4)), "shape"), (dict(shape=(4, 2.5, 4)), "shape"), (dict(shape=5), "shape"),
    (dict(shape=(2048, 2048, 2048)), "shape"), (dict(shape=(True, 2, 2)), "shape"),
    (dict(center=(0, 0)), "center"), (dict(center=(0, np.inf, 0)), "center"), (dict(center="origin"), "center"),
    (dict(rotation=np.eye(2)), "rotation"), (dict(rotation=2 * np.eye(3)), "orthonormal"),
    (dict(n_smooth=1), "n_smooth"), (dict(n_smooth=65), "n_smooth"), (dict(n_smooth=201), "n_smooth"),
    (dict(periodicity_scale=-1.0), "periodicity_scale"), (dict(values=np.ones(7)), "same length"),
])
def test_sph_grid_refuses_bad_arguments_on_the_host(monkeypatch, kw, match):
    import topsy_amd
    _no_gpu(monkeypatch)
    pos, mass = _particles()
    args = dict(shape=(4, 4, 4), size=1.0) | kw
    if kw.get("n_smooth") == 201:
        args["n_smooth"], match = 64, "finite coordinates"
        pos, mass = pos[:50], mass[:50]
    with pytest.raises(ValueError, match=match):
        topsy_amd.sph_grid(pos, mass, **args)


def test_sph_grid_refuses_bad_arrays_on_the_host(monkeypatch):
    import topsy_amd
    _no_gpu(monkeypatch)
    pos, mass = _particles()
    with pytest.raises(ValueError, match="shape"):
        topsy_amd.sph_grid(pos[:, :2], mass, size=1.0)
    with pytest.raises(ValueError, match="same length"):
        topsy_amd.sph_grid(pos, mass[:-1], size=1.0)
    with pytest.raises(ValueError, match="mass"):
        topsy_amd.sph_grid(pos, None, size=1.0)
    with pytest.raises(ValueError, match="at least one"):
        topsy_amd.sph_grid(np.empty((0, 3)), np.empty(0), size=1.0)
    bad = pos.copy()
    bad[10:] = np.nan
    with pytest.raises(ValueError, match="finite coordinates"):
        topsy_amd.sph_grid(bad, mass, size=1.0)


@pytest.mark.parametrize("kw, match", [
    (dict(resolution=0), "resolution"), (dict(resolution=2.5), "resolution"), (dict(resolution=True), "resolution"),
    (dict(size=None), "size"), (dict(size=(1.0, 2.0, 3.0)), "size"), (dict(size=(1.0, 0.0)), "size"),
    (dict(center=(1, 2)), "center"), (dict(n_smooth=0), "n_smooth"),
])
def test_sph_slice_refuses_bad_arguments_on_the_host(monkeypatch, kw, match):
    import topsy_amd
    _no_gpu(monkeypatch)
    pos, mass = _particles()
    with pytest.raises(ValueError, match=match):
        topsy_amd.sph_slice(pos, mass, **(dict(resolution=8, size=1.0) | kw))


@pytest.mark.parametrize("kw, match", [
    (dict(start=None), "start"), (dict(end=None), "end"), (dict(start=(0, 0)), "start"), (dict(end=(0, 0, np.nan)), "end"),
    (dict(n_samples=0), "n_samples"), (dict(n_samples=1.5), "n_samples"), (dict(n_samples=2 ** 31), "n_samples"),
    (dict(n_smooth=1), "n_smooth"), (dict(values=np.ones(3)), "same length"),
])
def test_sph_ray_refuses_bad_arguments_on_the_host(monkeypatch, kw, match):
    import topsy_amd
    _no_gpu(monkeypatch)
    pos, mass = _particles()
    with pytest.raises(ValueError, match=match):
        topsy_amd.sph_ray(pos, mass, **(dict(start=(0, 0, 0), end=(1, 1, 1), n_samples=5) | kw))


def _stub_visualizer(data_loader):
    """A Visualizer that was never given a GPU: get_slice_image reads the view and the loader only."""
    from topsy_amd import visualizer
    vis = object.__new__(visualizer.Visualizer)
    vis._sph = types.SimpleNamespace(rotation_matrix=np.eye(3), position_offset=np.zeros(3), scale=1.0)
    vis._render_resolution = 16
    vis.data_loader = data_loader
    return vis


def test_get_slice_image_refuses_bad_arguments_on_the_host(monkeypatch):
    from topsy_amd import loader
    _no_gpu(monkeypatch)
    pos, mass = _particles()
    ld = loader.ArrayDataLoader(pos=pos, smooth=None, mass=mass, quantities={"temp": np.ones(len(pos), dtype=f32)})
    vis = _stub_visualizer(ld)
    for res in (0, -4, 2.5, "32", True):
        with pytest.raises(ValueError, match="resolution"):
            vis.get_slice_image(resolution=res)
    with pytest.raises(KeyError, match="pressure"):
        vis.get_slice_image("pressure")
    with pytest.raises(ValueError, match="from_arrays"):
        _stub_visualizer(loader.TestDataLoader(100)).get_slice_image()
    few = loader.ArrayDataLoader(pos=pos[:10], smooth=np.ones(10, dtype=f32), mass=mass[:10])
    with pytest.raises(ValueError, match="finite coordinates"):
        _stub_visualizer(few).get_slice_image()


def test_context_binding_refuses_bad_lattices_on_the_host():
    from topsy_amd import _native
    ok = dict(origin=(0, 0, 0), du=(1, 0, 0), dv=(0, 1, 0), dw=(0, 0, 1), shape=(2, 3, 4))
    lat = _native.lattice_struct(**ok)
    assert (lat.nu, lat.nv, lat.nw) == (2, 3, 4) and list(lat.dv) == [0.0, 1.0, 0.0]
    assert ctypes.sizeof(_native.Lattice) == 4 * 24 + 16
    for bad in (dict(shape=(2, 3)), dict(shape=(0, 1, 1)), dict(shape=(1 << 11, 1 << 10, 1 << 10)), dict(shape=(1.5, 1, 1)),
                dict(origin=(0, 0)), dict(du=(np.nan, 0, 0)), dict(dw="up")):
        with pytest.raises(ValueError):
            _native.lattice_struct(**(ok | bad))


# ---- no GPU: the product raises, it never falls back to the reference ----------------------------------------------------------
def test_without_a_gpu_the_public_functions_raise():
    import topsy_amd
    from topsy_amd import _native, loader
    if _native.device_count() > 0:
        pytest.skip("a GPU is present")
    pos, mass = _particles()
    with pytest.raises(_native.BackendUnavailable):
        topsy_amd.sph_grid(pos, mass, shape=(2, 2, 2), size=1.0)
    with pytest.raises(_native.BackendUnavailable):
        topsy_amd.sph_slice(pos, mass, resolution=4, size=1.0)
    with pytest.raises(_native.BackendUnavailable):
        topsy_amd.sph_ray(pos, mass, start=(0, 0, 0), end=(1, 0, 0), n_samples=4)
    with pytest.raises(_native.BackendUnavailable):
        _stub_visualizer(loader.ArrayDataLoader(pos=pos, smooth=None, mass=mass)).get_slice_image()


def test_the_call_is_declared_bound_and_exported():
    import os
    from topsy_amd import _native, multigpu, visualizer
    import topsy_amd
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "topsy_splat.h")).read()
    assert "int tsp_sph_sample_lattice(" in text and "} tsp_lattice;" in text and " * 122: new entry point tsp_sph_sample_lattice" in text
    restype, argtypes = _native.SIGNATURES["tsp_sph_sample_lattice"]
    assert restype is ctypes.c_int and len(argtypes) == 12
    assert _native.ABI_VERSION == 112 and _native.load_library().tsp_version() >= 122
    assert hasattr(_native.Context, "sph_sample_lattice") and hasattr(multigpu.MultiGpuContext, "sph_sample_lattice")
    assert hasattr(visualizer.Visualizer, "get_slice_image")
    assert all(callable(getattr(topsy_amd, name)) for name in ("sph_grid", "sph_slice", "sph_ray"))
