"""tsp_sph_velocity_gradient on the GPU: inside the derived bound of velocity_gradient_ref.within_bound around the float32 brute
force (the order of the four float64 sums is free, so that is what the contract promises) on the scenes that test_gpu_smoothing.py
built to break a spatial search, with k-NN radii and with a caller's own h, exact zeros for a uniform velocity, non-finite inputs,
determinism, argument errors and failed allocations that change nothing, and the product path: 'v_div' and 'vorticity' as
quantities of a snapshot that carries velocities."""
import ctypes

import numpy as np
import pytest

from test_density_cpu import brute_force_sph_sum
from test_gpu_smoothing import SCENES, _snapshot
from test_smoothing_cpu import brute_force_smoothing
from velocity_gradient_ref import OUTPUTS, brute_force_velocity_gradient, velocity_field, within_bound

pytestmark = pytest.mark.gpu
KS = (8, 32)
_H = {}


def _smoothing(name):
    """{k: h} of a scene for k in KS, computed once"""
    if name not in _H:
        pos, L = SCENES[name]
        _H[name] = brute_force_smoothing(pos, KS, period=L)
    return _H[name]


@pytest.fixture(scope="module")
def ctx():
    from topsy_amd import _native
    c = _native.Context(64, 2)
    yield c
    c.close()


def _masses(n, seed=23):
    return np.random.RandomState(seed).uniform(0.5, 2.0, size=n).astype(np.float32)


def _gpu(ctx, pos, h, mass, rho, vel, L=None):
    """(n, 4) float32 in the order of OUTPUTS"""
    div, curl = ctx.sph_velocity_gradient(pos[:, 0], pos[:, 1], pos[:, 2], h, mass, rho, vel[:, 0], vel[:, 1], vel[:, 2], L)
    assert div.dtype == curl.dtype == np.float32 and div.shape == (len(pos),) and curl.shape == (len(pos), 3)
    return np.column_stack([div, curl])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _compare(label, got, ref, h, pos):
    """Every query takes part: NaN exactly where the query is not answerable, the bound elsewhere.  Prints the bit-equal share."""
    want, A, T = ref
    assert got.dtype == np.float32 and got.shape == want.shape
    with np.errstate(invalid="ignore"):
        answerable = np.isfinite(pos).all(axis=1) & np.isfinite(h) & (h > 0)
    assert np.isnan(got[~answerable]).all() and np.isnan(want[~answerable]).all(), label
    assert not np.isnan(got[answerable]).any() and not np.isnan(want[answerable]).any(), label
    ok = within_bound(got, want, A, T)
    equal = (_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))
    print(f"{label}: {equal.mean() * 100:.2f} % bit-equal, {np.count_nonzero(~answerable)} not answerable, "
          f"up to {int(T.max())} terms")
    bad = np.argwhere(~ok)
    assert ok.all(), (f"{label}: {len(bad)} of {got.size} outside the bound, e.g. (query, output) {bad[:5].tolist()}: "
                      f"{got[~ok][:5]} vs {want[~ok][:5]}")
    return answerable


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", list(SCENES))
def test_within_the_bound_of_the_brute_force(ctx, name, k):
    pos, L = SCENES[name]
    mass = _masses(len(pos))
    h = _smoothing(name)[k]
    rho = brute_force_sph_sum(pos, h, mass, period=L)
    vel = velocity_field(pos, 37)
    got = _gpu(ctx, pos, h, mass, rho, vel, L)
    answerable = _compare(f"{name}, k={k}", got, brute_force_velocity_gradient(pos, h, mass, rho, vel, period=L), h, pos)
    assert np.isfinite(got[answerable]).all()
    if name == "duplicates":
        assert (h[100:140] == 0).all() and np.isnan(got[100:140]).all() and np.isnan(got[7]).all()
    if name == "non_finite":
        assert np.count_nonzero(~answerable) == 100


@pytest.mark.parametrize("name", list(SCENES))
def test_within_the_bound_with_the_callers_own_h(ctx, name):
    """h that is no k-NN radius: scaled by a factor from [0.3, 3] per particle, one particle whose h spans the whole box, and
    on the scene that has outliers one of them with a small h, whose neighbourhood is empty: exact zeros."""
    pos, L = SCENES[name]
    rs = np.random.RandomState(31)
    mass = _masses(len(pos))
    h = _smoothing(name)[32] * rs.uniform(0.3, 3.0, size=len(pos)).astype(np.float32)
    valid = np.isfinite(pos).all(axis=1)
    big = int(np.flatnonzero(valid)[len(pos) // 3])
    extent = float(L) if L else float(np.ptp(pos[valid], axis=0).max())
    h[big] = np.float32(2.0 * extent)
    if name == "clustered_outliers":
        lonely = len(pos) - 1                                    # an outlier 1e4 x farther away than the cloud is wide
        h[lonely] = np.float32(0.5)
    rho = brute_force_sph_sum(pos, h, mass, period=L)
    vel = velocity_field(pos, 41)
    got = _gpu(ctx, pos, h, mass, rho, vel, L)
    ref = brute_force_velocity_gradient(pos, h, mass, rho, vel, period=L)
    _compare(f"{name}, own h", got, ref, h, pos)
    # every valid particle that is no copy of the big one is its neighbour
    assert np.isfinite(got[big]).all() and ref[2][big] >= np.count_nonzero(valid) - 50
    if name == "clustered_outliers":
        assert ref[2][lonely] == 0 and rho[lonely] > 0 and (got[lonely] == 0).all()


def test_one_particle(ctx):
    one = np.array([[0.25, -1.0, 3.0]], dtype=np.float32)
    got = _gpu(ctx, one, np.array([0.5], dtype=np.float32), np.ones(1, dtype=np.float32), np.array([2.0], dtype=np.float32),
               np.array([[1.0, 2.0, 3.0]], dtype=np.float32))
    assert got.shape == (1, 4) and (got == 0).all()


@pytest.mark.parametrize("name", ["periodic", "clustered_outliers"])
def test_uniform_velocity_gives_exact_zeros(ctx, name):
    pos, L = SCENES[name]
    mass = _masses(len(pos))
    h = _smoothing(name)[32]
    rho = brute_force_sph_sum(pos, h, mass, period=L)
    vel = np.tile(np.array([3.25, -1.5, 0.125], dtype=np.float32), (len(pos), 1))
    got = _gpu(ctx, pos, h, mass, rho, vel, L)
    answerable = np.isfinite(pos).all(axis=1) & np.isfinite(h) & (h > 0)
    assert answerable.sum() > len(pos) // 2 and (got[answerable] == 0).all() and np.isnan(got[~answerable]).all()


def test_non_finite_inputs(ctx):
    """NaN and infinities in vel, mass and rho at 60 particles of the uniform scene: the NaN pattern and the infinities are the
    brute force's, the rest is inside the bound.  rho > 0 elsewhere and the infinite masses are +inf with finite velocities, so an
    infinite sum gets its sign from one term (or is NaN in the brute force as well: inf - inf, inf x 0)."""
    pos, L = SCENES["uniform"]
    n = len(pos)
    rs = np.random.RandomState(43)
    mass = _masses(n)
    h = _smoothing("uniform")[32]
    rho = brute_force_sph_sum(pos, h, mass)
    assert (rho > 0).all()
    vel = velocity_field(pos, 47)
    special = rs.choice(n, 60, replace=False)
    vel[special[:10], rs.randint(0, 3, size=10)] = np.nan
    vel[special[10:20], rs.randint(0, 3, size=10)] = np.array([np.inf, -np.inf], dtype=np.float32)[rs.randint(0, 2, size=10)]
    mass[special[20:30]] = np.nan
    mass[special[30:40]] = np.inf
    rho[special[40:50]] = np.nan
    rho[special[50:60]] = np.inf
    got = _gpu(ctx, pos, h, mass, rho, vel)
    want, A, T = brute_force_velocity_gradient(pos, h, mass, rho, vel)
    assert np.isnan(want).any(axis=1).sum() >= 200 and np.isinf(want).sum() >= 10 and (want[special[50:60]] == 0).any()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got[np.isinf(want)], want[np.isinf(want)])
    finite = np.isfinite(want)
    assert finite.all(axis=1).sum() > n // 2
    ok = within_bound(got, want, A, T) | ~finite
    assert ok.all(), np.argwhere(~ok)[:5].tolist()


def test_the_same_bits_again_and_on_another_context(ctx):
    from topsy_amd import _native
    pos, L = SCENES["periodic"]
    mass = _masses(len(pos))
    h = _smoothing("periodic")[32]
    rho = ctx.sph_sum(pos[:, 0], pos[:, 1], pos[:, 2], h, mass, L)
    vel = velocity_field(pos, 53)
    first = _gpu(ctx, pos, h, mass, rho, vel, L)
    assert np.array_equal(_bits(_gpu(ctx, pos, h, mass, rho, vel, L)), _bits(first))
    other = _native.Context(16, 2)
    try:
        assert np.array_equal(_bits(_gpu(other, pos, h, mass, rho, vel, L)), _bits(first))
    finally:
        other.close()


# ---- errors: TSP_EINVAL and TSP_ENOMEM, and nothing changes ----------------------------------------------------------------
def _render_state(ctx, M, sf):
    ctx.render(M, sf)
    counts = {k: v for k, v in ctx.stats().items() if not k.startswith("ms_")}
    return ctx.read_image(), counts, ctx.download_particles()


def _resident_scene(mips, fragments=False):
    """64 resident particles whose footprints do not overlap (test_gpu_density.py::test_invalid_arguments_change_nothing): every
    pixel holds at most one fragment, so two renders of it are the same bit for bit"""
    from oracle import oracle_np
    from topsy_amd import _native
    ctx = _native.Context(160, 2)
    ctx.set_kernel_mips(mips)
    g = np.arange(-70.0, 71.0, 20.0, dtype=np.float32)
    gx, gy = (v.ravel() for v in np.meshgrid(g, g))
    ctx.upload_particles(gx, gy, np.zeros(64, dtype=np.float32), np.full(64, 3.0, dtype=np.float32), _masses(64))
    ctx.upload_quantity(np.random.RandomState(9).normal(size=64).astype(np.float32))
    if fragments:
        ctx.set_option("count_fragments", 1)
    return ctx, oracle_np.transform_matrix(np.eye(3), np.zeros(3), 90.0)


def test_invalid_arguments_change_nothing(mips):
    from topsy_amd import _native
    lib = _native.load_library()
    fp = ctypes.POINTER(ctypes.c_float)
    ctx, (M, sf) = _resident_scene(mips, fragments=True)
    try:
        img0, counts0, parts0 = _render_state(ctx, M, sf)
        assert np.count_nonzero(img0[..., 0]) > 64 * 20

        n = 1000
        rs = np.random.RandomState(1)
        x, y, z = (np.ascontiguousarray(rs.uniform(0, 1, n), dtype=np.float32) for _ in range(3))
        pos = np.stack([x, y, z], 1)
        hh = np.full(n, 0.1, dtype=np.float32)
        mass = _masses(n)
        rho = brute_force_sph_sum(pos, hh, mass)
        vel = velocity_field(pos, 3)
        vx, vy, vz = (np.ascontiguousarray(vel[:, a]) for a in range(3))
        outs = [np.full(n, 7.0, dtype=np.float32) for _ in range(4)]
        P = lambda v: v.ctypes.data_as(fp)                                              # noqa: E731
        good = [n, P(x), P(y), P(z), P(hh), P(mass), P(rho), P(vx), P(vy), P(vz), 0.0] + [P(o) for o in outs]

        def but(i, v):
            args = list(good)
            args[i] = v
            return tuple(args)
        cases = [but(0, 0), but(0, -5), but(0, 1 << 31), but(10, -1.0), but(10, float("nan")), but(10, float("inf")),
                 but(10, float("-inf"))] + [but(i, None) for i in list(range(1, 10)) + [11, 12, 13, 14]]
        assert len(cases) == 7 + 9 + 4
        for args in cases:
            assert lib.tsp_sph_velocity_gradient(ctx._h, *args) == -1, args          # TSP_EINVAL
            assert all((o == 7.0).all() for o in outs), args
        assert lib.tsp_sph_velocity_gradient(None, *good) == -1 and all((o == 7.0).all() for o in outs)

        got = _gpu(ctx, pos, hh, mass, rho, vel)
        want, A, T = brute_force_velocity_gradient(pos, hh, mass, rho, vel)
        assert within_bound(got, want, A, T).all() and np.isfinite(got).all()
        # no valid particle at all: every output NaN, still no error
        assert np.isnan(_gpu(ctx, np.full((n, 3), np.nan, dtype=np.float32), hh, mass, rho, vel)).all()
        assert lib.tsp_sph_velocity_gradient(ctx._h, 1, *good[1:]) == 0
        assert all(o[0] == 0 and (o[1:] == 7.0).all() for o in outs)
        img1, counts1, parts1 = _render_state(ctx, M, sf)
        assert np.array_equal(img0.view(np.uint32), img1.view(np.uint32))
        assert counts0 == counts1 and counts0["n_fragments"] > 0
        for k in parts0:
            assert np.array_equal(parts0[k], parts1[k]), k
    finally:
        ctx.close()


@pytest.mark.parametrize("periodic", [False, True])
def test_failed_allocations_change_nothing(mips, periodic):
    """The k-th allocation of the call fails for k = 1, 2, ...: TSP_ENOMEM, the four outputs keep their sentinel, the context its
    image, counts and particles; the sites are those of tsp_sph_sum (the call adds none); the call after the failures is right."""
    from test_gpu_scratch_alloc_failure import SCRATCH_SITES, Outputs, P, col, index_points, walk
    from topsy_amd import _native
    lib = _native.load_library()
    ctx, (M, sf) = _resident_scene(mips)
    try:
        ctx.render(M, sf)
        pos, L = index_points(periodic)
        n = len(pos)
        x, y, z = col(pos)
        h = brute_force_smoothing(pos, 32, period=L)
        mass = _masses(n)
        rho = brute_force_sph_sum(pos, h, mass, period=L)
        vel = velocity_field(pos, 5)
        vx, vy, vz = col(vel)
        outs = Outputs(**{name: np.empty(n, dtype=np.float32) for name in OUTPUTS})
        walk(_native, ctx,
             lambda: lib.tsp_sph_velocity_gradient(ctx._h, n, P(x), P(y), P(z), P(h), P(mass), P(rho), P(vx), P(vy), P(vz), L,
                                                   *[P(getattr(outs, name)) for name in OUTPUTS]),
             outs, SCRATCH_SITES["sph_sum"])
        got = np.column_stack([getattr(outs, name) for name in OUTPUTS])
        want, A, T = brute_force_velocity_gradient(pos, h, mass, rho, vel, period=L)
        ok = within_bound(got, want, A, T)
        assert ok.all() and np.isfinite(got).all(), f"{np.count_nonzero(~ok)} of {got.size} outside the bound"
    finally:
        ctx.close()


def test_works_on_the_multi_gpu_context():
    from topsy_amd import _native, multigpu
    pos, _ = SCENES["lattice"]
    mass = _masses(len(pos))
    h = brute_force_smoothing(pos, 16)
    vel = velocity_field(pos, 59)
    ctx = _native.Context(16, 2)
    rho = ctx.sph_sum(pos[:, 0], pos[:, 1], pos[:, 2], h, mass)
    want = _gpu(ctx, pos, h, mass, rho, vel)
    ctx.close()
    mg = multigpu.MultiGpuContext(16, 2, [0, 0])
    got = _gpu(mg, pos, h, mass, rho, vel)
    mg.close()
    assert np.array_equal(_bits(got), _bits(want)) and np.isfinite(got[np.isfinite(h) & (h > 0)]).all()


# ---- the product path ---------------------------------------------------------------------------------------------------
def _image(vis, quantity):
    from topsy_amd.drawreason import DrawReason
    vis.scale = 20.0
    vis.rotate(0.3, 0.2)
    vis.quantity_name = quantity
    vis.render_sph(DrawReason.EXPORT)
    return np.array(vis.get_sph_image(), copy=True)


@pytest.mark.parametrize("variant", ["plain", "with_cells", "periodic"])
def test_v_div_and_vorticity_of_a_snapshot_with_velocities(variant, monkeypatch):
    import topsy_amd
    from topsy_amd import _native
    L = 30.0 if variant == "periodic" else None
    pos, mass, _ = _snapshot(n=3000, L=L)
    # periodic: the field of the nearest image of the origin, so that it is continuous across the faces the view is centred on
    vel = velocity_field(pos - np.float32(L) * np.rint(pos / np.float32(L)) if L else pos, 61, noise=0.02)
    kw = dict(render_resolution=64, with_cells=variant == "with_cells", periodicity_scale=L)
    vis = topsy_amd.from_arrays(pos, None, mass, vel=vel, **kw)
    ref = None
    try:
        ld = vis.data_loader
        assert ld.get_quantity_names()[-3:] == ["rho", "v_div", "vorticity"]
        img = _image(vis, "v_div")                          # on the parent commit the setter raises ValueError here
        assert vis.quantity_name == "v_div"
        div, curl = ld.get_velocity_gradient()
        assert div.dtype == curl.dtype == np.float32 and div.shape == (len(pos),) and curl.shape == (len(pos), 3)
        assert div is ld.get_named_quantity("v_div") and div is ld.get_velocity_gradient()[0]
        # the determinism clause: the same sums on another context of the same device give the same bits
        want_div, want_curl = topsy_amd.sph_velocity_gradient(ld.get_positions(), ld.get_mass(), ld.get_velocities(), periodicity_scale=L)
        assert np.array_equal(_bits(div), _bits(want_div)) and np.array_equal(_bits(curl), _bits(want_curl))
        smooth, rho = ld.get_smooth(), ld.get_named_quantity("rho")
        again = topsy_amd.sph_velocity_gradient(ld.get_positions(), ld.get_mass(), ld.get_velocities(), smooth=smooth, rho=rho,
                                                periodicity_scale=L)
        assert np.array_equal(_bits(div), _bits(again[0])) and np.array_equal(_bits(curl), _bits(again[1]))
        bf, A, T = brute_force_velocity_gradient(ld.get_positions(), smooth, ld.get_mass(), rho, ld.get_velocities(), period=L or 0.0)
        assert within_bound(np.column_stack([div, curl]), bf, A, T).all() and np.isfinite(div).all()
        cx, cy, cz = curl[:, 0], curl[:, 1], curl[:, 2]
        vort = ld.get_named_quantity("vorticity")
        assert vort.dtype == np.float32 and np.array_equal(_bits(vort), _bits(np.sqrt((cx * cx + cy * cy) + cz * cz)))
        # the field is 0.7 r + Omega x r + noise: the estimates have its signs and, biased low, its size
        assert 0.5 * 2.1 < np.median(div) < 2.1 and 0.5 * 2 * 0.8 < np.median(cz) < 2 * 0.8
        img_vort = _image(vis, "vorticity")
        assert img_vort.shape == img.shape and (img_vort[np.isfinite(img_vort)] >= 0).all() and np.nanmax(img_vort) > 0

        # a second visualizer that is given these arrays: the same image, and no gradient call at all
        calls = []
        real = _native.Context.sph_velocity_gradient
        monkeypatch.setattr(_native.Context, "sph_velocity_gradient", lambda self, *a, **k: calls.append(1) or real(self, *a, **k))
        ref = topsy_amd.from_arrays(ld.get_positions(), smooth, ld.get_mass(), quantities={"v_div": div, "rho": rho},
                                    vel=ld.get_velocities(), **dict(kw, with_cells=False))
        ref_img = _image(ref, "v_div")
        with np.errstate(all="ignore"):
            print(f"{variant}: largest relative difference of the two images {np.nanmax(np.abs(img - ref_img) / np.abs(ref_img)):.3g}")
        np.testing.assert_allclose(img, ref_img, rtol=1e-5)
        assert np.array_equal(ref.data_loader.get_named_quantity("v_div"), div) and not calls
        assert np.nanmax(np.abs(img)) > 0
    finally:
        vis.close()
        if ref is not None:
            ref.close()


def test_set_velocity_gradient_restores_a_cache(monkeypatch):
    import topsy_amd
    from topsy_amd import _native
    pos, mass, _ = _snapshot(n=3000)
    vel = velocity_field(pos, 67, noise=0.2)
    h = topsy_amd.smoothing_lengths(pos, n_smooth=16)
    div, curl = topsy_amd.sph_velocity_gradient(pos, mass, vel, n_smooth=16)
    rho = topsy_amd.sph_density(pos, mass, smooth=h)
    bf, A, T = brute_force_velocity_gradient(pos, h, mass, rho, vel)
    assert within_bound(np.column_stack([div, curl]), bf, A, T).all()

    def refuse(*a, **k):
        raise AssertionError("the velocity gradient was computed again")
    monkeypatch.setattr(_native.Context, "sph_velocity_gradient", refuse)
    vis = topsy_amd.from_arrays(pos, h, mass, vel=vel, render_resolution=64)
    try:
        vis.data_loader.set_velocity_gradient(div, curl)
        vis.quantity_name = "vorticity"
        assert np.array_equal(vis.data_loader.get_named_quantity("v_div"), div)
        assert np.array_equal(vis.data_loader.get_velocity_gradient()[1], curl)
    finally:
        vis.close()
