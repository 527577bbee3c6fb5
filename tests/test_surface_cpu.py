"""Surface rendering without a GPU: the numpy restatement (tests/surface_ref.py) meets the reference's known answers
(tests/test_render_output.py::test_surface_render, in tests/golden/surface_kats.npz) at the reference's tolerances; the sphere
texture, the density-cut interpolation and the filter parameters of the product equal their definitions."""
import numpy as np
import pytest

import surface_ref
from oracle import oracle_np
from topsy_amd import kernel_lut, loader
from topsy_amd.colormap.implementation import _lut_from_matplotlib, quantile_from_order_statistics
from topsy_amd.colormap.surface import ColorAsSurfaceMap
from topsy_amd import config

R = 200


def _rotation(x_angle, y_angle):
    cx, sx, cy, sy = np.cos(x_angle), np.sin(x_angle), np.cos(y_angle), np.sin(y_angle)
    rot_y = np.array([[cx, 0, sx], [0, 1, 0], [-sx, 0, cx]])        # VisualizerBase._x_rotation_matrix
    rot_x = np.array([[1, 0, 0], [0, cy, -sy], [0, sy, cy]])        # VisualizerBase._y_rotation_matrix
    return rot_y @ rot_x


@pytest.fixture(scope="module")
def kat_scene():
    """The scene of the reference's test_surface_render: 1e5 test particles, 200^2, scale 30, rotate(0, 1), test-quantity."""
    ld = loader.TestDataLoader(None, int(1e5))
    ps = ld.get_pos_smooth()
    m = np.asarray(ld.get_mass(), dtype=np.float32)
    q = np.asarray(ld.get_named_quantity("test-quantity"), dtype=np.float32)
    M, sf = oracle_np.transform_matrix(_rotation(0.0, 1.0), -np.asarray(ld.get_initial_center()), 30.0)
    cut = surface_ref.cut_for_percentile(surface_ref.density_cuts(m, ps[:, 3]), 50.0)
    raw, _ = surface_ref.occlusion(ps, m, q, M, sf, R, cut)
    return raw


def test_restatement_meets_the_reference_kats(kat_scene, golden):
    kats = golden["surface_kats.npz"]
    raw = kat_scene
    filtered = surface_ref.bilateral(raw, 0.01)
    keep = np.ones(100, dtype=bool)
    keep[67] = False                           # the reference's test skips pixel 67 of the quantity
    np.testing.assert_allclose(filtered[::20, ::20, 0].ravel()[keep], kats["quantity"][keep], rtol=1e-3)
    np.testing.assert_allclose(filtered[::20, ::20, 1].ravel(), kats["depth"], rtol=1e-3)
    vmin, vmax, log = surface_ref.autorange(raw)
    lut = _lut_from_matplotlib(config.DEFAULT_COLORMAP, config.COLORMAP_NUM_SAMPLES)
    rgba = surface_ref.shade(filtered, weighted_average=True, log=log, vmin=vmin, vmax=vmax, lut=lut)
    np.testing.assert_allclose(rgba[::20, ::20].ravel().astype(int), kats["presentation"].astype(int), atol=30)


def test_sphere_mips_match_their_formula():
    got = kernel_lut.sphere_mips()
    assert got.dtype == np.float32 and got.shape == (5440,)
    assert np.array_equal(got, surface_ref.sphere_mips())
    lvl0 = got[:4096].reshape(64, 64)
    assert lvl0[0, 0] == np.float32(-0.01) and lvl0[31, 31] == np.float32(np.sqrt(4.0 - 2 * (2.0 / 64) ** 2))
    assert np.array_equal(lvl0, lvl0[::-1]) and np.array_equal(lvl0, lvl0[:, ::-1])


@pytest.mark.parametrize("case", ["testdata", "nonfinite", "tiny"])
def test_order_statistic_interpolation_equals_np_quantile(case):
    if case == "testdata":
        ld = loader.TestDataLoader(None, 20000)
        m, h = np.asarray(ld.get_mass(), np.float32), ld.get_pos_smooth()[:, 3]
    elif case == "nonfinite":
        rs = np.random.RandomState(3)
        m = rs.uniform(-1, 2, 5000).astype(np.float32)
        h = rs.uniform(0.0, 1.0, 5000).astype(np.float32)
        h[::97] = 0.0                       # rho = +-inf (and 0 / 0 = NaN where m is 0)
        m[::501] = np.nan
        m[::13] = np.inf
    else:
        m, h = np.array([2.0], np.float32), np.array([1.0], np.float32)
    with np.errstate(all="ignore"):
        rho = m / ((h * h) * h)
    srt = np.sort(rho)
    q = np.linspace(0, 1, 101)
    with np.errstate(all="ignore"):
        want = surface_ref.density_cuts(m, h)
        got = quantile_from_order_statistics(lambda r: srt[np.asarray(r)], len(rho), q)
    assert got.dtype == want.dtype
    assert np.array_equal(got, want, equal_nan=True)
    if case == "nonfinite":
        assert np.isnan(got).all()
        finite = rho[~np.isnan(rho)]
        srt = np.sort(finite)
        with np.errstate(all="ignore"):
            assert np.array_equal(quantile_from_order_statistics(lambda r: srt[np.asarray(r)], len(finite), q),
                                  np.quantile(finite, q), equal_nan=True)


@pytest.mark.parametrize("scale,R,want", [(0.01, 200, (2.0, 0.02, 9)), (0.01, 1024, (10.24, 0.02, 41)),
                                          (1e-7, 1024, (1e-5 * 1024, 2e-5, 1)), (0.1, 1024, (102.4, 0.2, 100)),
                                          (0.5, 4096, (2048.0, 1.0, 100))])
def test_filter_parameters(scale, R, want):
    ss, rs, n = surface_ref.filter_parameters(scale, R)
    assert (ss, rs, n) == (np.float32(want[0]), np.float32(want[1]), want[2])
    cm = ColorAsSurfaceMap(None, None, "rgba8unorm", {"smoothing_scale": scale})
    assert cm.filter_parameters(R) == (ss, rs, n)


def test_surface_map_is_not_selectable_by_the_holder():
    from topsy_amd.colormap import ColormapHolder
    with pytest.raises(ValueError):
        ColormapHolder.instance_from_parameters({"type": "surface"}, None, None, "rgba8unorm")
    cm = ColorAsSurfaceMap(None, None, "rgba8unorm", {})
    assert cm.get_parameter("smoothing_scale") == 0.01 and cm.get_parameter("ambient_color") == [0.0, 0.0, 0.2]
    with pytest.raises(ValueError):
        cm.update_parameters({"type": "density"})


def test_surface_view_refuses_a_multi_gpu_visualizer():
    import types
    from topsy_amd.surface import SurfaceView
    vis = types.SimpleNamespace(particle_buffers=types.SimpleNamespace(context=types.SimpleNamespace(n_gpus=2)),
                                _periodic_tiling=False)
    with pytest.raises(NotImplementedError):
        SurfaceView(vis)


@pytest.mark.parametrize("n", [1, 2, 7, 1000, 54321])
def test_density_quantiles_sort_once_and_equal_np_quantile(n):
    from topsy_amd.sph import density_quantiles
    rs = np.random.RandomState(n)
    m = rs.uniform(0, 2, n).astype(np.float32)
    h = rs.lognormal(size=n).astype(np.float32)

    class FakeContext:
        num_particles = n
        calls = 0

        def density_order_stats(self, ranks):
            FakeContext.calls += 1
            return np.sort(m / ((h * h) * h))[np.asarray(ranks)]
    got = density_quantiles(FakeContext())
    assert FakeContext.calls == 1
    assert got.dtype == np.float64 and np.array_equal(got, surface_ref.density_cuts(m, h))
