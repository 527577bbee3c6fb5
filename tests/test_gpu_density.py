"""tsp_sph_sum on the GPU: within one float32 ulp of the float32 brute force of test_density_cpu.py (the sum order is free, so
for weights >= 0 that is what the contract promises) on the scenes that test_gpu_smoothing.py built to break a spatial search,
with k-NN radii and with a caller's own h, with non-finite and negative weights, at 1e6 particles; argument errors that change
nothing; and the product path: 'rho' as a quantity of a snapshot that carries none."""
import ctypes

import numpy as np
import pytest

from test_density_cpu import brute_force_sph_sum, lattice, lattice_density, within_one_ulp
from test_gpu_smoothing import SCENES, _clustered, _snapshot
from test_smoothing_cpu import brute_force_smoothing

pytestmark = pytest.mark.gpu
KS = (8, 32)


@pytest.fixture(scope="module")
def ctx():
    from topsy_amd import _native
    c = _native.Context(64, 2)
    yield c
    c.close()


def _masses(n, seed=23):
    return np.random.RandomState(seed).uniform(0.5, 2.0, size=n).astype(np.float32)


def _compare(label, got, want, h, pos):
    """Every query takes part: NaN exactly where the query is not answerable, one ulp elsewhere.  Prints the bit-equal share."""
    assert got.dtype == np.float32 and got.shape == want.shape
    with np.errstate(invalid="ignore"):
        answerable = np.isfinite(pos).all(axis=1) & np.isfinite(h) & (h > 0)
    assert np.isnan(got[~answerable]).all() and np.isnan(want[~answerable]).all(), label
    ok = within_one_ulp(got, want)
    equal = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    print(f"{label}: {equal.mean() * 100:.2f} % bit-equal, {np.count_nonzero(~answerable)} not answerable")
    assert ok.all(), (f"{label}: {np.count_nonzero(~ok)} of {len(got)} farther than one ulp, e.g. index {np.flatnonzero(~ok)[:5]}: "
                      f"{got[~ok][:5]} vs {want[~ok][:5]}")
    return answerable


@pytest.mark.parametrize("name", list(SCENES))
def test_one_ulp_against_brute_force(ctx, name):
    pos, L = SCENES[name]
    a = _masses(len(pos))
    hs = brute_force_smoothing(pos, KS, period=L)
    for k in KS:
        h = hs[k]
        got = ctx.sph_sum(pos[:, 0], pos[:, 1], pos[:, 2], h, a, L)
        want = brute_force_sph_sum(pos, h, a, period=L)
        answerable = _compare(f"{name}, k={k}", got, want, h, pos)
        assert np.isfinite(got[answerable]).all() and (got[answerable] > 0).all()
        if name == "duplicates" and k <= 32:
            assert (h[100:140] == 0).all() and np.isnan(got[100:140]).all() and np.isnan(got[7])
        if name == "non_finite":
            assert np.count_nonzero(~answerable) == 100


@pytest.mark.parametrize("name", list(SCENES))
def test_one_ulp_with_the_callers_own_h(ctx, name):
    """h that is no k-NN radius: scaled by a factor from [0.3, 3] per particle, and one particle whose h spans the whole box."""
    pos, L = SCENES[name]
    rs = np.random.RandomState(31)
    a = _masses(len(pos))
    h = brute_force_smoothing(pos, 32, period=L) * rs.uniform(0.3, 3.0, size=len(pos)).astype(np.float32)
    valid = np.isfinite(pos).all(axis=1)
    big = int(np.flatnonzero(valid)[len(pos) // 3])
    extent = float(L) if L else float(np.ptp(pos[valid], axis=0).max())
    h[big] = np.float32(2.0 * extent)
    got = ctx.sph_sum(pos[:, 0], pos[:, 1], pos[:, 2], h, a, L)
    want = brute_force_sph_sum(pos, h, a, period=L)
    _compare(f"{name}, own h", got, want, h, pos)
    # every valid particle is a neighbour of the big one
    d = np.linalg.norm(pos[valid].astype(np.float64) - pos[big], axis=1)
    assert L or d.max() < 2 * h[big]
    assert np.isfinite(got[big]) and got[big] > 0


def test_non_finite_and_negative_weights(ctx):
    """NaN, +inf and negative a[j] on the uniform scene.  Queries with no such neighbour: one ulp.  A NaN in the neighbourhood:
    NaN.  Infinite results equal the brute force's (or both NaN, where +inf meets a negative or NaN term).  A negative term
    voids the one-ulp derivation (the sum can cancel): those queries are held to a relative bound taken from the reference
    alone -- 4 x the largest relative difference, on the CPU, between the brute force summed forwards and summed backwards over
    these queries, at least one ulp.  Measured when the test was written: on the 1551 such queries with a finite result,
    forwards and backwards give the same float32 bits (relative difference 0; the float64 sum of some 33 terms is off by
    about 1e-14 of the largest term, far below a float32 ulp even where the result is 2000 x smaller than the median), so the
    bound that holds is its floor: one ulp."""
    pos, L = SCENES["uniform"]
    n = len(pos)
    rs = np.random.RandomState(41)
    a = _masses(n)
    special = rs.choice(n, 100, replace=False)
    a[special[:20]] = np.nan
    a[special[20:40]] = np.inf
    a[special[40:]] = -a[special[40:]] * np.float32(3.0)
    h = brute_force_smoothing(pos, 32)
    got = ctx.sph_sum(pos[:, 0], pos[:, 1], pos[:, 2], h, a)
    want, negative = brute_force_sph_sum(pos, h, a, with_negative=True)
    fwd = brute_force_sph_sum(pos, h, a, order="forward")
    bwd = brute_force_sph_sum(pos, h, a, order="backward")
    finite = np.isfinite(want)
    clean = finite & ~negative
    assert clean.sum() > n // 2 and negative.sum() > 100 and np.isnan(want).sum() >= 20 and np.isinf(want).sum() >= 10
    # non-finite results: NaN where the brute force is NaN, the same infinity where it is infinite
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got[np.isinf(want)], want[np.isinf(want)])
    # no special neighbour: one ulp
    ok = within_one_ulp(got[clean], want[clean])
    assert ok.all(), np.flatnonzero(clean)[~ok][:5]
    # a negative term: the reference's own order dependence, times 4, floor one ulp
    sel = finite & negative
    scale = np.abs(want[sel]).astype(np.float64)
    order_spread = float(np.max(np.abs(fwd[sel].astype(np.float64) - bwd[sel]) / scale))
    diff = np.abs(got[sel].astype(np.float64) - want[sel])
    bound = np.maximum(4.0 * order_spread * scale, np.spacing(want[sel]).astype(np.float64))
    print(f"negative terms: {sel.sum()} queries, forwards vs backwards {order_spread:.3g} relative, "
          f"largest GPU difference {float(np.max(diff / scale)):.3g} relative")
    assert (diff <= bound).all(), np.flatnonzero(sel)[diff > bound][:5]


@pytest.mark.parametrize("periodic", [False, True])
def test_million_points(ctx, periodic):
    L = 40.0 if periodic else None
    pos = _clustered(1_000_000, 11, L)
    a = _masses(len(pos))
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    h = ctx.smoothing_lengths(x, y, z, 32, L)
    got = ctx.sph_sum(x, y, z, h, a, L)
    assert np.array_equal(np.isnan(got), ~(h > 0))
    assert np.isfinite(got[h > 0]).all() and (got[h > 0] > 0).all()
    queries = np.random.RandomState(5).choice(len(pos), 2000, replace=False)
    want = brute_force_sph_sum(pos, h, a, period=L or 0.0, block=16, queries=queries)
    ok = within_one_ulp(got[queries], want[queries])
    equal = got[queries].view(np.uint32) == want[queries].view(np.uint32)
    print(f"1e6 particles, periodic={periodic}: {equal.mean() * 100:.2f} % of 2000 queries bit-equal")
    assert ok.all(), (queries[~ok][:5], got[queries][~ok][:5], want[queries][~ok][:5])
    # the same call again: the same bits (the order of the sum is fixed)
    again = ctx.sph_sum(x, y, z, h, a, L)
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32))


# ---- errors: TSP_EINVAL, and nothing changes ----------------------------------------------------------------------------
def _render_state(ctx, M, sf):
    ctx.render(M, sf)
    st = ctx.stats()
    counts = {k: v for k, v in st.items() if not k.startswith("ms_")}
    return ctx.read_image(), counts, ctx.download_particles()


def test_invalid_arguments_change_nothing(mips):
    """The resident scene is 64 particles whose footprints do not overlap: every pixel then holds at most one fragment, so two
    renders of it are the same bit for bit (where footprints overlap, the order of the splat's float atomics is free and two
    renders agree to 1e-5 only), and so must be the renders before and after the calls."""
    from oracle import oracle_np
    from topsy_amd import _native
    lib = _native.load_library()
    fp = ctypes.POINTER(ctypes.c_float)
    ctx = _native.Context(160, 2)
    ctx.set_kernel_mips(mips)
    g = np.arange(-70.0, 71.0, 20.0, dtype=np.float32)              # 8 x 8 particles 17.8 px apart, footprints of radius 5.3 px
    gx, gy = (v.ravel() for v in np.meshgrid(g, g))
    rs = np.random.RandomState(9)
    ctx.upload_particles(gx, gy, np.zeros(64, dtype=np.float32), np.full(64, 3.0, dtype=np.float32), _masses(64))
    ctx.upload_quantity(rs.normal(size=64).astype(np.float32))
    ctx.set_option("count_fragments", 1)
    M, sf = oracle_np.transform_matrix(np.eye(3), np.zeros(3), 90.0)
    img0, counts0, parts0 = _render_state(ctx, M, sf)
    assert np.count_nonzero(img0[..., 0]) > 64 * 20

    n = 1000
    rs = np.random.RandomState(1)
    x, y, z = (np.ascontiguousarray(rs.uniform(0, 1, n), dtype=np.float32) for _ in range(3))
    hh = np.full(n, 0.1, dtype=np.float32)
    a = _masses(n)
    out = np.full(n, 7.0, dtype=np.float32)
    P = lambda v: v.ctypes.data_as(fp)                                              # noqa: E731
    good = [n, P(x), P(y), P(z), P(hh), P(a), 0.0, P(out)]

    def but(i, v):
        args = list(good)
        args[i] = v
        return tuple(args)
    cases = [but(0, 0), but(0, -5), but(0, 1 << 31), but(6, -1.0), but(6, float("nan")), but(6, float("inf")),
             but(6, float("-inf")), but(1, None), but(2, None), but(3, None), but(4, None), but(5, None), but(7, None)]
    for args in cases:
        assert lib.tsp_sph_sum(ctx._h, *args) == -1, args          # TSP_EINVAL
        assert (out == 7.0).all(), args
    assert lib.tsp_sph_sum(None, *good) == -1 and (out == 7.0).all()

    got = ctx.sph_sum(x, y, z, hh, a)
    assert within_one_ulp(got, brute_force_sph_sum(np.stack([x, y, z], 1), hh, a)).all()
    # no valid particle at all: every output NaN, still no error
    assert np.isnan(ctx.sph_sum(np.full(n, np.nan, dtype=np.float32), y, z, hh, a)).all()
    assert lib.tsp_sph_sum(ctx._h, 1, P(x), P(y), P(z), P(hh), P(a), 0.0, P(out)) == 0 and out[0] > 0 and (out[1:] == 7.0).all()
    img1, counts1, parts1 = _render_state(ctx, M, sf)
    assert np.array_equal(img0.view(np.uint32), img1.view(np.uint32))
    assert counts0 == counts1 and counts0["n_fragments"] > 0
    for k in parts0:
        assert np.array_equal(parts0[k], parts1[k]), k
    ctx.close()


def test_works_on_the_multi_gpu_context():
    from topsy_amd import _native, multigpu
    pos, _ = SCENES["lattice"]
    a = _masses(len(pos))
    h = brute_force_smoothing(pos, 16)
    ctx = _native.Context(16, 2)
    want = ctx.sph_sum(pos[:, 0], pos[:, 1], pos[:, 2], h, a)
    ctx.close()
    mg = multigpu.MultiGpuContext(16, 2, [0, 0])
    got = mg.sph_sum(pos[:, 0], pos[:, 1], pos[:, 2], h, a)
    mg.close()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- the product path ---------------------------------------------------------------------------------------------------
def _image(vis):
    from topsy_amd.drawreason import DrawReason
    vis.scale = 20.0
    vis.rotate(0.3, 0.2)
    vis.quantity_name = "rho"
    vis.render_sph(DrawReason.EXPORT)
    return np.array(vis.get_sph_image(), copy=True)


@pytest.mark.parametrize("variant", ["plain", "with_cells", "periodic", "two_contexts"])
def test_rho_of_a_snapshot_without_one(variant, monkeypatch):
    import topsy_amd
    from topsy_amd import _native
    L = 30.0 if variant == "periodic" else None
    pos, mass, quantities = _snapshot(L=L)
    kw = dict(render_resolution=128, with_cells=variant == "with_cells", periodicity_scale=L, render_mode="bivariate")
    if variant == "two_contexts":
        kw["device_ids"] = [0, 0]
    vis = topsy_amd.from_arrays(pos, None, mass, quantities=quantities, **kw)
    ref = None
    try:
        ld = vis.data_loader
        assert ld.get_quantity_names() == ["temp", "rho"]
        img = _image(vis)                                   # on the parent commit the setter raises ValueError here
        assert vis.quantity_name == "rho"
        rho = ld.get_named_quantity("rho")
        assert rho.dtype == np.float32 and rho.shape == (len(pos),) and rho is ld.get_named_quantity("rho")
        # the determinism clause: the same sum on another context of the same device gives the same bits
        want = topsy_amd.sph_density(ld.get_positions(), ld.get_mass(), periodicity_scale=L)
        assert np.array_equal(rho.view(np.uint32), want.view(np.uint32))
        assert within_one_ulp(rho, brute_force_sph_sum(ld.get_positions(), ld.get_smooth(), ld.get_mass(), period=L or 0.0)).all()
        if variant == "plain":
            assert np.array_equal(rho.view(np.uint32), topsy_amd.sph_density(pos, mass).view(np.uint32))

        # a second visualizer that is given this density and these smoothing lengths: the same image, and no SPH sum at all
        calls = []
        real = _native.Context.sph_sum
        monkeypatch.setattr(_native.Context, "sph_sum", lambda self, *a, **k: calls.append(1) or real(self, *a, **k))
        ref = topsy_amd.from_arrays(ld.get_positions(), ld.get_smooth(), ld.get_mass(), quantities={"rho": rho},
                                    **dict(kw, with_cells=False))
        ref_img = _image(ref)
        np.testing.assert_allclose(img, ref_img, rtol=1e-5)
        assert np.array_equal(ref.data_loader.get_named_quantity("rho"), rho) and not calls
        assert np.nanmax(img[..., 0]) > 0
    finally:
        vis.close()
        if ref is not None:
            ref.close()


def test_set_density_restores_a_cached_density(monkeypatch):
    import topsy_amd
    from topsy_amd import _native
    pos, mass, _ = _snapshot(n=3000)
    rho = topsy_amd.sph_density(pos, mass, n_smooth=16)
    h = topsy_amd.smoothing_lengths(pos, n_smooth=16)
    assert within_one_ulp(rho, brute_force_sph_sum(pos, h, mass)).all()
    assert np.array_equal(rho, topsy_amd.sph_density(pos, mass, smooth=h))

    def refuse(*a, **k):
        raise AssertionError("the density was computed again")
    monkeypatch.setattr(_native.Context, "sph_sum", refuse)
    vis = topsy_amd.from_arrays(pos, h, mass, render_resolution=64)
    try:
        vis.data_loader.set_density(rho)
        vis.quantity_name = "rho"
        assert vis.data_loader.get_named_quantity("rho") is not None
        assert np.array_equal(vis.data_loader.get_named_quantity("rho"), rho)
    finally:
        vis.close()


def test_sph_mean():
    import topsy_amd
    pos, _ = SCENES["uniform"]
    n = len(pos)
    mass = _masses(n)
    values = np.random.RandomState(3).uniform(1.0, 2.0, size=n).astype(np.float32)
    h = brute_force_smoothing(pos, 32)
    rho = topsy_amd.sph_density(pos, mass, smooth=h)
    got = topsy_amd.sph_mean(pos, mass, h, values, rho=rho)
    a = mass * values / rho
    assert a.dtype == np.float32
    assert within_one_ulp(got, brute_force_sph_sum(pos, h, a)).all()
    # rho and smooth computed by the wrapper itself: the same composition
    assert np.array_equal(topsy_amd.sph_mean(pos, mass, None, values), got)
    # the periodic lattice: every rho[j] is the same number, so a constant field comes back as that constant
    lat = lattice(12)
    ones = np.ones(len(lat), dtype=np.float32)
    hl = np.full(len(lat), 1.2, dtype=np.float32)
    rho_l = topsy_amd.sph_density(lat, ones, smooth=hl, periodicity_scale=12.0)
    np.testing.assert_allclose(rho_l, lattice_density(), rtol=1e-6)
    assert rho_l.max() / rho_l.min() - 1 <= 1e-6
    const = topsy_amd.sph_mean(lat, ones, hl, np.full(len(lat), 3.7, dtype=np.float32), periodicity_scale=12.0)
    np.testing.assert_allclose(const, 3.7, rtol=1e-6)
