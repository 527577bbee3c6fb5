"""SPH densities for snapshots without them (no GPU): the float32 brute force that the GPU tests (test_gpu_density.py) hold
tsp_sph_sum to, pinned against a float64 evaluation over scipy's kd-tree and against a lattice sum, and the host layer
('rho' as a quantity of every ArrayDataLoader, the argument checks of sph_density / sph_mean)."""
import numpy as np
import pytest

from test_smoothing_cpu import _cloud, _no_gpu, brute_force_smoothing


def brute_force_sph_sum(pos, h, a, period=0.0, block=256, order="pairwise", queries=None, with_negative=False):
    """The contract of tsp_sph_sum in numpy float32 with its operation order and a float64 row sum: for every answerable
    query i (finite coordinates, h[i] finite and > 0), over every j with finite coordinates,
    u = sqrtf(d2) / h[i], the term a[j] * w(u) exists iff u < 2, w = (1 - 1.5 u2) + 0.75 (u2 u) below 1 and
    0.25 ((t t) t), t = 2 - u, above; out[i] = (float)(S / (pi * (double)((h h) h))); NaN elsewhere.  d2 as in
    brute_force_smoothing.  order: how the float64 row sum runs ("pairwise": numpy's own; "forward" / "backward": one term
    after the other).  queries: only these indices are evaluated (the others stay NaN).  with_negative: also return, per
    particle, whether a term with a[j] < 0 took part."""
    pos = np.asarray(pos, dtype=np.float32)
    h = np.asarray(h, dtype=np.float32)
    a = np.asarray(a, dtype=np.float32)
    valid = np.isfinite(pos).all(axis=1)
    P, A = pos[valid], a[valid]
    L = np.float32(period)
    one, two = np.float32(1.0), np.float32(2.0)
    out = np.full(len(pos), np.nan, dtype=np.float32)
    negative = np.zeros(len(pos), dtype=bool)
    with np.errstate(all="ignore"):
        answerable = valid & np.isfinite(h) & (h > 0)
    if queries is not None:
        chosen = np.zeros(len(pos), dtype=bool)
        chosen[np.asarray(queries)] = True
        answerable &= chosen
    todo = np.flatnonzero(answerable)
    with np.errstate(all="ignore"):
        for b in range(0, len(todo), block):
            idx = todo[b:b + block]
            q, hq = pos[idx], h[idx]
            d = []
            for ax in range(3):
                dx = P[None, :, ax] - q[:, None, ax]
                if period:
                    t = dx / L
                    t = np.rint(t)
                    dx = dx - L * t
                d.append(dx)
            d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            u = np.sqrt(d2) / hq[:, None]
            inside = u < two
            u2 = u * u
            t = two - u
            w = np.where(u < one, (one - np.float32(1.5) * u2) + np.float32(0.75) * (u2 * u), np.float32(0.25) * ((t * t) * t))
            term = A[None, :] * w
            assert term.dtype == np.float32
            term64 = np.where(inside, term.astype(np.float64), 0.0)
            if order == "pairwise":
                S = term64.sum(axis=1)
            elif order == "forward":
                S = np.cumsum(term64, axis=1)[:, -1]
            else:
                S = np.cumsum(term64[:, ::-1], axis=1)[:, -1]
            out[idx] = (S / (np.pi * ((hq * hq) * hq).astype(np.float64))).astype(np.float32)
            negative[idx] = (inside & (A[None, :] < 0)).any(axis=1)
    return (out, negative) if with_negative else out


def within_one_ulp(got, want):
    """Per element: equal bits, both NaN, or finite and no farther apart than one float32 ulp (of the larger magnitude)."""
    got = np.asarray(got, dtype=np.float32)
    want = np.asarray(want, dtype=np.float32)
    with np.errstate(all="ignore"):
        same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)) | (got == want)
        both = np.isfinite(got) & np.isfinite(want)
        ulp = np.maximum(np.spacing(np.abs(got)), np.spacing(np.abs(want))).astype(np.float64)
        near = both & (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp)
    return same | near


def _w64(u):
    """The M4 spline in float64 (support 2, value 1 at 0): what topsy_amd/kernel_lut.py::_w3 integrates."""
    u = np.asarray(u, dtype=np.float64)
    return np.where(u < 1, 1 - 1.5 * u ** 2 + 0.75 * u ** 3, np.where(u < 2, 0.25 * (2 - u) ** 3, 0.0))


def kdtree_sph_sum(pos, h, a, workers=16):
    """The same sum in float64 over scipy's cKDTree.query_ball_point (radius 2 h)."""
    from scipy.spatial import cKDTree
    p = np.asarray(pos, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    a = np.asarray(a, dtype=np.float64)
    tree = cKDTree(p)
    lists = tree.query_ball_point(p, 2.0 * h, workers=workers)
    out = np.empty(len(p))
    for i, js in enumerate(lists):
        js = np.asarray(js, dtype=np.int64)
        u = np.sqrt(((p[js] - p[i]) ** 2).sum(axis=1)) / h[i]
        out[i] = (a[js] * _w64(u)).sum() / (np.pi * h[i] ** 3)
    return out


@pytest.mark.parametrize("k", [8, 32, 64])
def test_brute_force_agrees_with_kdtree(k):
    """Measured when the check was set: the largest relative deviation is 2.2e-7 (2.0e-7, 2.1e-7, 1.8e-7 for k = 8, 32, 64;
    with the masses drawn here 2.4e-7, 2.1e-7, 1.6e-7), the float32 rounding of d2, u, w and of the result.  rtol = 1e-6 is
    4 x that, rounded up: room for another libm, not for a wrong kernel (a wrong normalisation or a missing self term is off by
    percents).  More than 2.5e-7 here means that this restatement differs from the contract."""
    pos = _cloud(3000, 5)
    mass = np.random.RandomState(17).uniform(0.5, 2.0, size=len(pos)).astype(np.float32)
    h = brute_force_smoothing(pos, k)
    got = brute_force_sph_sum(pos, h, mass)
    want = kdtree_sph_sum(pos, h, mass)
    dev = float(np.max(np.abs(got.astype(np.float64) - want) / want))
    print(f"k={k}: largest relative deviation from the kd-tree {dev:.3g}")
    assert (want > 0).all()
    np.testing.assert_allclose(got, want, rtol=1e-6)
    assert dev <= 2.5e-7, dev
    # the sum order does not matter beyond one ulp when every term is >= 0
    for order in ("forward", "backward"):
        assert within_one_ulp(brute_force_sph_sum(pos, h, mass, order=order), got).all()


def lattice(n=12):
    g = np.arange(n, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def lattice_density(h=1.2):
    """sum over the lattice offsets r of w(|r| / h) / (pi h^3), in float64"""
    h = float(np.float32(h))
    m = int(np.ceil(2 * h)) + 1
    o = np.arange(-m, m + 1, dtype=np.float64)
    r = np.sqrt(o[:, None, None] ** 2 + o[None, :, None] ** 2 + o[None, None, :] ** 2)
    return float(_w64(r / h).sum() / (np.pi * h ** 3))


def test_periodic_lattice_normalisation():
    """Every particle of a periodic unit lattice sees the same neighbourhood: one density everywhere (measured: the ratio of
    the largest to the smallest is exactly 1, every value 1.0008096), equal to the float64 lattice sum."""
    pos = lattice(12)
    n = len(pos)
    rho = brute_force_sph_sum(pos, np.full(n, 1.2, dtype=np.float32), np.ones(n, dtype=np.float32), period=12.0)
    print(f"lattice: rho in [{rho.min():.9g}, {rho.max():.9g}], lattice sum {lattice_density():.9g}")
    assert rho.max() / rho.min() - 1 <= 1e-6
    np.testing.assert_allclose(rho, lattice_density(), rtol=1e-6)
    # without the wrap the faces see fewer neighbours
    open_box = brute_force_sph_sum(pos, np.full(n, 1.2, dtype=np.float32), np.ones(n, dtype=np.float32))
    assert open_box.min() < 0.7 * rho.min() and np.isclose(open_box.max(), rho.max(), rtol=1e-6)


def test_brute_force_unanswerable_queries_and_non_finite_weights():
    rs = np.random.RandomState(2)
    pos = rs.uniform(-1, 1, size=(400, 3)).astype(np.float32)
    h = np.full(400, 0.3, dtype=np.float32)
    a = np.ones(400, dtype=np.float32)
    pos[5, 1] = np.nan
    h[[6, 7, 8, 9]] = [0.0, -1.0, np.nan, np.inf]
    a[10] = np.nan
    a[11] = np.inf
    rho = brute_force_sph_sum(pos, h, a)
    assert np.isnan(rho[[5, 6, 7, 8, 9]]).all()
    d10 = np.linalg.norm(pos - pos[10], axis=1)
    d11 = np.linalg.norm(pos - pos[11], axis=1)
    sees_nan = (d10 < 0.55) & np.isfinite(h) & (h > 0) & np.isfinite(d10)
    far = (d10 > 0.65) & (d11 > 0.65) & np.isfinite(h) & (h > 0)
    assert np.isnan(rho[sees_nan]).all() and sees_nan.sum() > 3
    assert np.isfinite(rho[far]).all() and (rho[far] > 0).all() and far.sum() > 100
    assert np.isinf(rho[11])
    # the invalid particle is nobody's neighbour: removing it changes nothing else
    keep = np.arange(400) != 5
    np.testing.assert_array_equal(brute_force_sph_sum(pos[keep], h[keep], a[keep]), rho[keep])


# ---- the host layer ---------------------------------------------------------------------------------------------------------
def test_array_loader_always_has_rho(monkeypatch):
    from topsy_amd import loader
    _no_gpu(monkeypatch)
    pos = _cloud(100, 1)
    ld = loader.ArrayDataLoader(pos=pos, smooth=np.ones(100), mass=np.ones(100))
    assert ld.get_quantity_names() == ["rho"]
    assert ld.get_quantity_label("rho") == "rho" and ld.get_quantity_label(None) == "density"
    ld = loader.ArrayDataLoader(pos=pos, smooth=None, mass=np.ones(100), quantities={"temp": np.ones(100)})
    assert ld.get_quantity_names() == ["temp", "rho"]
    with pytest.raises(KeyError):
        ld.get_named_quantity("entropy")


def test_supplied_rho_is_returned_untouched(monkeypatch):
    from topsy_amd import loader
    _no_gpu(monkeypatch)
    pos = _cloud(100, 1)
    rho = np.random.RandomState(0).uniform(size=100).astype(np.float32)
    ld = loader.ArrayDataLoader(pos=pos, smooth=np.ones(100), mass=np.ones(100), quantities={"rho": rho, "temp": np.ones(100)})
    assert ld.get_quantity_names() == ["rho", "temp"]
    np.testing.assert_array_equal(ld.get_named_quantity("rho"), rho)     # (any GPU call would have raised)
    with pytest.raises(ValueError):
        ld.set_density(rho)


def test_set_density_hands_a_cached_density_back(monkeypatch):
    from topsy_amd import loader
    _no_gpu(monkeypatch)
    pos = _cloud(500, 2)
    ld = loader.ArrayDataLoader(pos=pos, smooth=None, mass=np.ones(500), quantities={"i": np.arange(500)}, with_cells=True)
    order = ld.get_named_quantity("i").astype(np.int64)
    rho = np.arange(500, dtype=np.float32)[order] * 2       # the caller's cache, in the loader's order
    with pytest.raises(ValueError, match="shape"):
        ld.set_density(rho[:-1])
    ld.set_density(rho)
    assert ld.get_named_quantity("rho") is ld.get_named_quantity("rho")
    np.testing.assert_array_equal(ld.get_named_quantity("rho"), rho)
    # a supplied rho is reordered with the other arrays
    ld = loader.ArrayDataLoader(pos=pos, smooth=None, mass=np.ones(500), with_cells=True,
                                quantities={"i": np.arange(500), "rho": np.arange(500) * 3})
    np.testing.assert_array_equal(ld.get_named_quantity("rho"), ld.get_named_quantity("i") * 3)


def test_sph_density_and_mean_argument_errors(monkeypatch):
    import topsy_amd
    _no_gpu(monkeypatch)
    pos = _cloud(100, 1)
    m = np.ones(100, dtype=np.float32)
    for bad in (0, 1, 65, 2.5, "32", True):
        with pytest.raises(ValueError, match="n_smooth"):
            topsy_amd.sph_density(pos, m, n_smooth=bad)
        with pytest.raises(ValueError, match="n_smooth"):
            topsy_amd.sph_mean(pos, m, m, m, n_smooth=bad)
    for bad in (-1.0, 0.0, np.nan, np.inf, 1e39, "big"):
        with pytest.raises(ValueError, match="periodicity_scale"):
            topsy_amd.sph_density(pos, m, periodicity_scale=bad)
        with pytest.raises(ValueError, match="periodicity_scale"):
            topsy_amd.sph_mean(pos, m, m, m, periodicity_scale=bad)
    with pytest.raises(ValueError, match="shape"):
        topsy_amd.sph_density(pos[:, :2], m)
    with pytest.raises(ValueError, match="same length"):
        topsy_amd.sph_density(pos, m[:99])
    with pytest.raises(ValueError, match="same length"):
        topsy_amd.sph_density(pos, m, smooth=np.ones(101))
    with pytest.raises(ValueError, match="same length"):
        topsy_amd.sph_density(pos, m, smooth=np.ones((100, 1)))
    with pytest.raises(ValueError, match="same length"):
        topsy_amd.sph_mean(pos, m, m, m[:50])
    with pytest.raises(ValueError, match="same length"):
        topsy_amd.sph_mean(pos, m, m, m, rho=m[:50])
    with pytest.raises(ValueError, match="values"):
        topsy_amd.sph_mean(pos, m, m, None)
    with pytest.raises(ValueError, match="at least one"):
        topsy_amd.sph_density(np.zeros((0, 3)), np.zeros(0), smooth=np.zeros(0))
    few = pos.copy()
    few[3:, 0] = np.nan
    with pytest.raises(ValueError, match="finite"):
        topsy_amd.sph_density(few, m, n_smooth=4)


def test_binding_declares_the_entry_point():
    from topsy_amd import _native, multigpu
    assert _native.ABI_VERSION >= 110 and "tsp_sph_sum" in _native.SIGNATURES
    assert hasattr(_native.Context, "sph_sum") and hasattr(multigpu.MultiGpuContext, "sph_sum")
