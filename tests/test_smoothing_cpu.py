"""Smoothing lengths for snapshots without them (no GPU): the argument checks of the host layer, and the float32 brute force
that the GPU tests (test_gpu_smoothing.py) hold tsp_smoothing_lengths to, pinned against scipy's kd-tree."""
import numpy as np
import pytest


def brute_force_smoothing(pos, ks, period=0.0, block=256):
    """The contract of tsp_smoothing_lengths in numpy float32 with its operation order: for every particle with finite
    coordinates, 0.5f * sqrtf(k-th smallest d2) over every particle with finite coordinates (itself included), with
    d2 = (dx*dx + dy*dy) + dz*dz and, in a periodic box, dx = dx - L * rint(dx / L); NaN elsewhere.  ks: one k or several;
    returns {k: h}."""
    single = np.isscalar(ks)
    ks = [int(ks)] if single else [int(k) for k in ks]
    pos = np.asarray(pos, dtype=np.float32)
    valid = np.isfinite(pos).all(axis=1)
    P = pos[valid]
    L = np.float32(period)
    out = {k: np.full(len(pos), np.nan, dtype=np.float32) for k in ks}
    res = {k: np.empty(len(P), dtype=np.float32) for k in ks}
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(0, len(P), block):
            q = P[a:a + block]
            d = []
            for ax in range(3):
                dx = P[None, :, ax] - q[:, None, ax]
                if period:
                    t = dx / L
                    t = np.rint(t)
                    dx = dx - L * t
                d.append(dx)
            d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            part = np.partition(d2, [k - 1 for k in ks], axis=1)
            for k in ks:
                res[k][a:a + block] = np.float32(0.5) * np.sqrt(part[:, k - 1])
    for k in ks:
        out[k][valid] = res[k]
    return out[ks[0]] if single else out


def kdtree_smoothing(pos, k, period=None, workers=16):
    """The same definition in float64 by scipy's cKDTree (positions must lie in [0, period) for a periodic box)."""
    from scipy.spatial import cKDTree
    p = np.asarray(pos, dtype=np.float64)
    tree = cKDTree(p, boxsize=period)
    d, _ = tree.query(p, k=k, workers=workers)
    return 0.5 * d[:, -1]


def _cloud(n, seed):
    rs = np.random.RandomState(seed)
    core = rs.normal(size=(n // 2, 3)) * 0.05 + rs.uniform(-1, 1, size=(1, 3))
    rest = rs.uniform(-1, 1, size=(n - n // 2, 3))
    return np.concatenate([core, rest]).astype(np.float32)


@pytest.mark.parametrize("k", [2, 8, 32, 64])
def test_brute_force_agrees_with_kdtree(k):
    pos = _cloud(3000, 5)
    h = brute_force_smoothing(pos, k)
    np.testing.assert_allclose(h, kdtree_smoothing(pos, k), rtol=1e-6)


@pytest.mark.parametrize("k", [8, 32])
def test_brute_force_agrees_with_kdtree_periodic(k):
    L = 10.0
    rs = np.random.RandomState(3)
    pos = rs.uniform(0, L, size=(3000, 3)).astype(np.float32)
    pos[pos >= np.float32(L)] = 0.0
    h = brute_force_smoothing(pos, k, period=L)
    np.testing.assert_allclose(h, kdtree_smoothing(pos, k, period=L), rtol=1e-6)
    # a point near a face has neighbours across it: the open-box answer is larger there
    assert (brute_force_smoothing(pos, k) >= h).all() and (brute_force_smoothing(pos, k) > h).any()


def test_brute_force_non_finite_and_duplicates():
    pos = np.zeros((50, 3), dtype=np.float32)
    pos[40:] = np.arange(10, dtype=np.float32)[:, None] + 1.0
    pos[45, 1] = np.nan
    pos[46, 2] = np.inf
    h = brute_force_smoothing(pos, [40, 41])
    assert np.isnan(h[40][[45, 46]]).all() and np.isfinite(np.delete(h[40], [45, 46])).all()
    assert (h[40][:40] == 0).all() and (h[41][:40] > 0).all()


# ---- the host layer refuses bad arguments before any GPU call ------------------------------------------------------------
def _no_gpu(monkeypatch):
    """Make any attempt to reach the library fail loudly, so that a ValueError can only come from the host checks."""
    from topsy_amd import _native

    def refuse(*a, **k):
        raise AssertionError("the GPU was touched")
    monkeypatch.setattr(_native, "load_library", refuse)
    monkeypatch.setattr(_native.Context, "__init__", refuse)


def test_array_loader_accepts_no_smoothing_lengths():
    from topsy_amd import config, loader
    pos = _cloud(100, 1)
    ld = loader.ArrayDataLoader(pos=pos, smooth=None, mass=np.ones(100))
    assert ld.needs_smoothing and ld.n_smooth == config.SMOOTH_NEIGHBOURS == 32
    with pytest.raises(RuntimeError):
        ld.get_smooth()
    h = np.arange(100, dtype=np.float32)
    ld.set_smooth(h)
    np.testing.assert_array_equal(ld.get_pos_smooth()[:, 3], h)
    ld = loader.ArrayDataLoader(pos=pos, smooth=np.ones(100), mass=np.ones(100))
    assert not ld.needs_smoothing


def test_array_loader_with_cells_keeps_its_order_without_smoothing_lengths():
    from topsy_amd import loader
    pos = _cloud(500, 2)
    q = np.arange(500, dtype=np.float32)
    ld = loader.ArrayDataLoader(pos=pos, smooth=None, mass=np.ones(500), quantities={"q": q}, with_cells=True,
                                n_smooth=16)
    order = ld.get_named_quantity("q").astype(np.int64)
    np.testing.assert_array_equal(ld.get_positions(), pos[order])
    assert ld.needs_smoothing and ld.n_smooth == 16 and hasattr(ld, "_cell_layout")


@pytest.mark.parametrize("n_smooth", [0, 1, 65, 2.5, "32", True])
def test_bad_n_smooth_is_refused_on_the_host(monkeypatch, n_smooth):
    import topsy_amd
    from topsy_amd import loader
    _no_gpu(monkeypatch)
    pos = _cloud(100, 1)
    with pytest.raises(ValueError, match="n_smooth"):
        loader.ArrayDataLoader(pos=pos, smooth=None, mass=np.ones(100), n_smooth=n_smooth)
    with pytest.raises(ValueError, match="n_smooth"):
        topsy_amd.from_arrays(pos, None, np.ones(100), n_smooth=n_smooth, render_resolution=64)
    with pytest.raises(ValueError, match="n_smooth"):
        topsy_amd.smoothing_lengths(pos, n_smooth=n_smooth)


@pytest.mark.parametrize("period", [-1.0, 0.0, np.nan, np.inf, -np.inf, 1e39, "big"])
def test_bad_period_is_refused_on_the_host(monkeypatch, period):
    import topsy_amd
    from topsy_amd import loader
    _no_gpu(monkeypatch)
    pos = _cloud(100, 1)
    with pytest.raises(ValueError, match="periodicity_scale"):
        loader.ArrayDataLoader(pos=pos, smooth=None, mass=np.ones(100), periodicity_scale=period)
    with pytest.raises(ValueError, match="periodicity_scale"):
        topsy_amd.from_arrays(pos, None, np.ones(100), periodicity_scale=period, render_resolution=64)
    with pytest.raises(ValueError, match="periodicity_scale"):
        topsy_amd.smoothing_lengths(pos, periodicity_scale=period)


def test_bad_shapes_are_refused_on_the_host(monkeypatch):
    import topsy_amd
    from topsy_amd import loader
    _no_gpu(monkeypatch)
    pos = _cloud(100, 1)
    with pytest.raises(ValueError, match="same length"):
        loader.ArrayDataLoader(pos=pos, smooth=None, mass=np.ones(99))
    with pytest.raises(ValueError, match="same length"):
        topsy_amd.from_arrays(pos, None, np.ones(101), render_resolution=64)
    with pytest.raises(ValueError, match="shape"):
        topsy_amd.from_arrays(pos[:, :2], None, np.ones(100), render_resolution=64)
    with pytest.raises(ValueError, match="shape"):
        topsy_amd.smoothing_lengths(pos[:, :2])
    bad = pos.copy()
    bad[3:, 0] = np.nan
    with pytest.raises(ValueError, match="finite"):
        topsy_amd.smoothing_lengths(bad, n_smooth=4)


def test_binding_declares_the_entry_point():
    from topsy_amd import _native
    assert _native.ABI_VERSION >= 106 and "tsp_smoothing_lengths" in _native.SIGNATURES
