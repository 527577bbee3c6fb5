"""Velocity divergence and vorticity (no GPU): the float32 brute force that the GPU tests (test_gpu_velocity_gradient.py) hold
tsp_sph_velocity_gradient to, pinned against exact results (a uniform field, a linear field on a lattice), against a float64
evaluation over scipy's kd-tree and at its edge cases, and the host layer ('v_div' and 'vorticity' as quantities of an
ArrayDataLoader with velocities, the argument checks of sph_velocity_gradient)."""
import numpy as np
import pytest

from test_density_cpu import _w64, brute_force_sph_sum, lattice
from test_smoothing_cpu import _cloud, _no_gpu, brute_force_smoothing
from velocity_gradient_ref import brute_force_velocity_gradient, velocity_field, within_bound


def _masses(n, seed=17):
    return np.random.RandomState(seed).uniform(0.5, 2.0, size=n).astype(np.float32)


def test_uniform_velocity_gives_exact_zeros():
    """every dv is exactly 0, so every term is +-0 whatever the masses and distances are"""
    pos = _cloud(1500, 3)
    n = len(pos)
    h = brute_force_smoothing(pos, 32)
    h[[4, 5]] = [0.0, np.nan]
    mass = _masses(n)
    rho = brute_force_sph_sum(pos, h, mass)
    vel = np.tile(np.array([3.25, -1.5, 0.125], dtype=np.float32), (n, 1))
    value, A, T = brute_force_velocity_gradient(pos, h, mass, rho, vel)
    answerable = np.isfinite(h) & (h > 0)
    assert (value[answerable] == 0).all() and (A[answerable] == 0).all() and (T[answerable] >= 29).all()
    assert np.isnan(value[~answerable]).all() and (T[~answerable] == 0).all()


def _f64(u):
    """-w'(u) / u of the M4 spline in float64: 3 - 2.25 u below 1, 0.75 (2 - u)^2 / u up to 2"""
    u = np.asarray(u, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(u < 1, 3 - 2.25 * u, np.where(u < 2, 0.75 * (2 - u) ** 2 / u, 0.0))


def lattice_kappa(h=1.2):
    """What the estimator returns for a unit gradient on the unit lattice, in float64: the sum over the lattice offsets r of
    f(|r| / h) r_x^2 / (pi h^5), divided by the lattice density, the sum of w(|r| / h) / (pi h^3)."""
    h = float(np.float32(h))
    m = int(np.ceil(2 * h)) + 1
    o = np.arange(-m, m + 1, dtype=np.float64)
    ox, oy, oz = o[:, None, None], o[None, :, None], o[None, None, :]
    r = np.sqrt(ox ** 2 + oy ** 2 + oz ** 2)
    f = np.where(r > 0, _f64(r / h), 0.0)
    return float((f * ox ** 2).sum() / (np.pi * h ** 5) / (_w64(r / h).sum() / (np.pi * h ** 3)))


def test_linear_field_on_a_lattice():
    """v = A x on lattice(10), open box, h = 1.2, unit masses: at the interior points (coordinates 3..6, whose neighbourhood is
    whole) the lattice's symmetry leaves div = kappa trace(A) and curl = kappa (A_zy - A_yz, A_xz - A_zx, A_yx - A_xy), with
    kappa = 0.98089449 the float64 lattice sum.  Measured when the check was set: the largest relative deviation of the brute
    force from that is 1.39e-7, the float32 rounding of the terms and of rho.  rtol = 6e-7 is 4 x that, rounded up; a wrong sign,
    factor or normalisation is off by percents."""
    pos = lattice(10)
    n = len(pos)
    h = np.full(n, 1.2, dtype=np.float32)
    mass = np.ones(n, dtype=np.float32)
    rho = brute_force_sph_sum(pos, h, mass)
    Amat = np.array([[0.5, -0.25, 0.75], [1.25, -1.0, 0.375], [-0.625, 0.875, 1.5]])
    vel = (pos.astype(np.float64) @ Amat.T).astype(np.float32)
    assert np.array_equal(vel.astype(np.float64), pos.astype(np.float64) @ Amat.T)      # (exact in float32)
    value, _, T = brute_force_velocity_gradient(pos, h, mass, rho, vel)
    interior = ((pos >= 3) & (pos <= 6)).all(axis=1)
    assert interior.sum() == 64 and (T[interior] == 56).all()          # the offsets with 0 < |r|^2 <= 5 < (2 h)^2 = 5.76
    kappa = lattice_kappa()
    assert abs(kappa - 0.98089449) < 5e-9, kappa
    want = kappa * np.array([np.trace(Amat), Amat[2, 1] - Amat[1, 2], Amat[0, 2] - Amat[2, 0], Amat[1, 0] - Amat[0, 1]])
    dev = float(np.max(np.abs(value[interior].astype(np.float64) / want - 1)))
    print(f"lattice: kappa {kappa:.9g}, largest relative deviation {dev:.3g}")
    np.testing.assert_allclose(value[interior], np.tile(want, (64, 1)), rtol=6e-7)


def kdtree_velocity_gradient(pos, h, mass, rho, vel, workers=16):
    """The same four sums in float64 over scipy's cKDTree.query_ball_point (radius 2 h); returns float64 (n, 4)."""
    from scipy.spatial import cKDTree
    p = np.asarray(pos, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    m = np.asarray(mass, dtype=np.float64)
    rho = np.asarray(rho, dtype=np.float64)
    v = np.asarray(vel, dtype=np.float64)
    lists = cKDTree(p).query_ball_point(p, 2.0 * h, workers=workers)
    out = np.empty((len(p), 4))
    for i, js in enumerate(lists):
        js = np.asarray(js, dtype=np.int64)
        d = p[js] - p[i]
        r = np.sqrt((d ** 2).sum(axis=1))
        c = np.where(r > 0, m[js] * _f64(r / h[i]), 0.0)
        dv = v[js] - v[i]
        den = np.pi * h[i] ** 5 * rho[i]
        out[i, 0] = (c * (dv * d).sum(axis=1)).sum() / den
        out[i, 1:] = (c[:, None] * np.cross(d, dv)).sum(axis=0) / den
    return out


KDTREE_C = 7e-6      # 4 x the largest |bf - kd| / A measured below


@pytest.mark.parametrize("k", [8, 32, 64])
def test_brute_force_agrees_with_kdtree(k):
    """|brute force - kd-tree| <= c A, A = sum |term| / |den| (a relative error is ill-defined where the sums cancel).  Measured
    when the check was set: the largest |bf - kd| / A is 1.75e-6, 3.95e-7, 2.61e-7 for k = 8, 32, 64 -- the float32 rounding of
    the displacement, u, f, the velocity differences and the products, which inside one term is relative to the partial products
    dvx dx, ..., not to the term (they cancel where dv is nearly perpendicular to d; with the 6 or 7 terms of k = 8 one such term
    weighs most).  c = 7e-6 is 4 x the largest: room for another libm, not for a wrong kernel (a wrong sign or a missing factor
    is off by order 1 in these units).  The float64 sums summed forwards and backwards stay inside within_bound."""
    pos = _cloud(3000, 5)
    n = len(pos)
    mass = _masses(n)
    h = brute_force_smoothing(pos, k)
    rho = brute_force_sph_sum(pos, h, mass)
    vel = velocity_field(pos, 29)
    got, A, T = brute_force_velocity_gradient(pos, h, mass, rho, vel)
    want = kdtree_velocity_gradient(pos, h, mass, rho, vel)
    assert (T >= k - 3).all() and (A > 0).all() and np.isfinite(got).all()
    c = float(np.max(np.abs(got.astype(np.float64) - want) / A))
    print(f"k={k}: largest |brute force - kd-tree| / A = {c:.3g}")
    assert c <= KDTREE_C, c
    # the size of the estimate: biased low by the self term of rho, about 0.77 at 32 neighbours on the uniform half
    if k == 32:
        med = np.median(got[n // 2:, 0]) / (3 * 0.7)
        print(f"k=32: median divergence on the uniform half / (3 x 0.7) = {med:.3f}")
        assert 0.6 < med < 0.95
    for order in ("forward", "backward"):
        other = brute_force_velocity_gradient(pos, h, mass, rho, vel, order=order)[0]
        assert within_bound(other, got, A, T).all()


def test_unanswerable_queries_and_non_finite_inputs():
    rs = np.random.RandomState(2)
    pos = rs.uniform(-1, 1, size=(400, 3)).astype(np.float32)
    h = np.full(400, 0.3, dtype=np.float32)
    mass = np.ones(400, dtype=np.float32)
    vel = velocity_field(pos, 3)
    pos[5, 1] = np.nan
    pos[12, 0] = np.inf
    h[[6, 7, 8, 9]] = [0.0, -1.0, np.nan, np.inf]
    vel[10] = np.nan
    rho = brute_force_sph_sum(pos, h, mass)
    rho[~np.isfinite(rho)] = 1.0
    value, A, T = brute_force_velocity_gradient(pos, h, mass, rho, vel)
    assert np.isnan(value[[5, 12, 6, 7, 8, 9]]).all()
    d10 = np.linalg.norm(pos - pos[10], axis=1)
    answerable = np.isfinite(pos).all(axis=1) & np.isfinite(h) & (h > 0)
    sees_nan = (d10 < 0.55) & answerable
    far = (d10 > 0.65) & answerable
    assert sees_nan[10] and sees_nan.sum() > 3 and np.isnan(value[sees_nan]).all()
    assert far.sum() > 100 and np.isfinite(value[far]).all()
    # the invalid particles are nobody's neighbour: removing one changes nothing else
    keep = np.arange(400) != 5
    again = brute_force_velocity_gradient(pos[keep], h[keep], mass[keep], rho[keep], vel[keep])
    for a, b in zip(again, (value[keep], A[keep], T[keep])):
        np.testing.assert_array_equal(a, b)


def test_exact_duplicates_contribute_nothing():
    """copies of a particle with other velocities and huge masses sit at d2 = 0 of the original: no term, at either"""
    rs = np.random.RandomState(8)
    pos = rs.uniform(-1, 1, size=(300, 3)).astype(np.float32)
    h = np.full(300, 0.4, dtype=np.float32)
    mass = _masses(300)
    vel = velocity_field(pos, 4)
    rho = brute_force_sph_sum(pos, h, mass)
    base = brute_force_velocity_gradient(pos, h, mass, rho, vel)
    pos2 = np.concatenate([pos, pos[[20, 20, 20]]])
    vel2 = np.concatenate([vel, rs.normal(size=(3, 3)).astype(np.float32) * 50])
    mass2 = np.concatenate([mass, np.full(3, 1e6, dtype=np.float32)])
    h2, rho2 = np.concatenate([h, h[[20] * 3]]), np.concatenate([rho, rho[[20] * 3]])
    value, A, T = brute_force_velocity_gradient(pos2, h2, mass2, rho2, vel2)
    assert np.array_equal(value[20], base[0][20]) and T[20] == base[2][20]
    assert (T[300:] == T[20]).all() and not np.array_equal(value[300], value[20])     # (their own v_i differs)
    # the copies are ordinary neighbours of everyone else
    d = np.linalg.norm(pos.astype(np.float64) - pos[20], axis=1)
    sure = np.abs(d - 0.8) > 1e-4
    sure[20] = False
    assert np.array_equal((T[:300] - base[2])[sure], np.where(d < 0.8, 3, 0)[sure]) and (d[sure] < 0.8).sum() > 10


# ---- the host layer ---------------------------------------------------------------------------------------------------------
def test_quantity_names_with_and_without_velocities(monkeypatch):
    from topsy_amd import loader
    _no_gpu(monkeypatch)
    pos = _cloud(100, 1)
    vel = velocity_field(pos, 1)
    ld = loader.ArrayDataLoader(pos=pos, smooth=np.ones(100), mass=np.ones(100), vel=vel)
    assert ld.get_quantity_names() == ["rho", "v_div", "vorticity"]
    ld = loader.ArrayDataLoader(pos=pos, smooth=None, mass=np.ones(100), quantities={"temp": np.ones(100)}, vel=vel)
    assert ld.get_quantity_names() == ["temp", "rho", "v_div", "vorticity"]
    ld = loader.ArrayDataLoader(pos=pos, smooth=None, mass=np.ones(100), quantities={"rho": np.ones(100), "temp": np.ones(100)}, vel=vel)
    assert ld.get_quantity_names() == ["rho", "temp", "v_div", "vorticity"]
    # without velocities nothing changes, and the names are unknown quantities
    ld = loader.ArrayDataLoader(pos=pos, smooth=None, mass=np.ones(100), quantities={"temp": np.ones(100)})
    assert ld.get_quantity_names() == ["temp", "rho"]
    for name in ("v_div", "vorticity"):
        with pytest.raises(KeyError):
            ld.get_named_quantity(name)
    with pytest.raises(KeyError):
        ld.get_velocity_gradient()


def test_supplied_v_div_is_returned_untouched(monkeypatch):
    from topsy_amd import loader
    _no_gpu(monkeypatch)
    pos = _cloud(100, 1)
    mine = np.random.RandomState(0).normal(size=100).astype(np.float32)
    ld = loader.ArrayDataLoader(pos=pos, smooth=np.ones(100), mass=np.ones(100), vel=velocity_field(pos, 1),
                                quantities={"v_div": mine, "vorticity": mine * 2})
    assert ld.get_quantity_names() == ["v_div", "vorticity", "rho"]
    np.testing.assert_array_equal(ld.get_named_quantity("v_div"), mine)            # (any GPU call would have raised)
    np.testing.assert_array_equal(ld.get_named_quantity("vorticity"), mine * 2)
    ld = loader.ArrayDataLoader(pos=pos, smooth=np.ones(100), mass=np.ones(100), vel=velocity_field(pos, 1), quantities={"v_div": mine})
    assert ld.get_quantity_names() == ["v_div", "rho", "vorticity"]
    # and without velocities a supplied one is an ordinary quantity
    ld = loader.ArrayDataLoader(pos=pos, smooth=np.ones(100), mass=np.ones(100), quantities={"v_div": mine})
    assert ld.get_quantity_names() == ["v_div", "rho"]
    np.testing.assert_array_equal(ld.get_named_quantity("v_div"), mine)


def test_set_velocity_gradient_hands_a_cache_back(monkeypatch):
    from topsy_amd import loader
    _no_gpu(monkeypatch)
    pos = _cloud(500, 2)
    vel = velocity_field(pos, 2)
    ld = loader.ArrayDataLoader(pos=pos, smooth=None, mass=np.ones(500), quantities={"i": np.arange(500)}, with_cells=True, vel=vel)
    order = ld.get_named_quantity("i").astype(np.int64)
    np.testing.assert_array_equal(ld.get_velocities(), vel[order])                 # permuted with the other arrays
    rs = np.random.RandomState(6)
    div = rs.normal(size=500).astype(np.float32)[order]                            # the caller's cache, in the loader's order
    curl = rs.normal(size=(500, 3)).astype(np.float32)[order]
    curl[7] = np.nan
    with pytest.raises(ValueError, match="shape"):
        ld.set_velocity_gradient(div[:-1], curl)
    with pytest.raises(ValueError, match="shape"):
        ld.set_velocity_gradient(div, curl[:, :2])
    with pytest.raises(ValueError, match="shape"):
        ld.set_velocity_gradient(div, curl.T)
    ld.set_velocity_gradient(div, curl)
    got_div, got_curl = ld.get_velocity_gradient()
    np.testing.assert_array_equal(got_div, div)
    np.testing.assert_array_equal(got_curl, curl)
    assert ld.get_named_quantity("v_div") is ld.get_named_quantity("v_div")
    np.testing.assert_array_equal(ld.get_named_quantity("v_div"), div)
    vort = ld.get_named_quantity("vorticity")
    cx, cy, cz = curl[:, 0], curl[:, 1], curl[:, 2]
    assert vort.dtype == np.float32 and vort is ld.get_named_quantity("vorticity")
    np.testing.assert_array_equal(vort, np.sqrt((cx * cx + cy * cy) + cz * cz))
    assert np.isnan(vort[7]) and np.isfinite(np.delete(vort, 7)).all()
    # a second cache replaces the first, the vorticity with it
    ld.set_velocity_gradient(div * 2, curl * 2)
    np.testing.assert_array_equal(ld.get_named_quantity("vorticity"), np.sqrt((4 * cx * cx + 4 * cy * cy) + 4 * cz * cz))
    with pytest.raises(ValueError, match="velocities"):
        loader.ArrayDataLoader(pos=pos, smooth=None, mass=np.ones(500)).set_velocity_gradient(div, curl)


def test_sph_velocity_gradient_argument_errors(monkeypatch):
    import topsy_amd
    _no_gpu(monkeypatch)
    pos = _cloud(100, 1)
    m = np.ones(100, dtype=np.float32)
    vel = velocity_field(pos, 1)
    for bad in (None, vel[:, :2], vel[:, 0], vel.T):
        with pytest.raises(ValueError, match="vel must have shape"):
            topsy_amd.sph_velocity_gradient(pos, m, bad)
    with pytest.raises(ValueError, match="same length"):
        topsy_amd.sph_velocity_gradient(pos, m, vel[:99])
    with pytest.raises(ValueError, match="same length"):
        topsy_amd.sph_velocity_gradient(pos, m[:99], vel)
    with pytest.raises(ValueError, match="same length"):
        topsy_amd.sph_velocity_gradient(pos, m, vel, smooth=np.ones(101))
    with pytest.raises(ValueError, match="same length"):
        topsy_amd.sph_velocity_gradient(pos, m, vel, smooth=m, rho=np.ones((100, 1)))
    with pytest.raises(ValueError, match="shape"):
        topsy_amd.sph_velocity_gradient(pos[:, :2], m, vel)
    for bad in (0, 1, 65, 2.5, "32", True):
        with pytest.raises(ValueError, match="n_smooth"):
            topsy_amd.sph_velocity_gradient(pos, m, vel, n_smooth=bad)
    for bad in (-1.0, 0.0, np.nan, np.inf, 1e39, "big"):
        with pytest.raises(ValueError, match="periodicity_scale"):
            topsy_amd.sph_velocity_gradient(pos, m, vel, periodicity_scale=bad)
    with pytest.raises(ValueError, match="at least one"):
        topsy_amd.sph_velocity_gradient(np.zeros((0, 3)), np.zeros(0), np.zeros((0, 3)), smooth=np.zeros(0))
    few = pos.copy()
    few[3:, 0] = np.nan
    with pytest.raises(ValueError, match="finite"):
        topsy_amd.sph_velocity_gradient(few, m, vel, n_smooth=4)


def test_binding_declares_the_entry_point():
    from topsy_amd import _native, multigpu
    assert _native.ABI_VERSION == 112 and "tsp_sph_velocity_gradient" in _native.SIGNATURES
    assert len(_native.SIGNATURES["tsp_sph_velocity_gradient"][1]) == 16
    assert hasattr(_native.Context, "sph_velocity_gradient") and hasattr(multigpu.MultiGpuContext, "sph_velocity_gradient")
    assert _native.load_library().tsp_version() >= 120
