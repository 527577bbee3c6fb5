"""tsp_sph_sample_lattice on the GPU against the brute force of lattice_ref.py: h bit for bit and every (positive) field within
one float32 ulp -- the criterion test_gpu_density.py applies to tsp_sph_sum -- at every lattice point, on lattices that reach every
brick shape and their partial bricks, points outside the particles' bounding box and whole periods outside a periodic box,
every KP instantiation of the search and every payload width of the sums; then non-finite inputs, duplicates, a signed field
against its derived bound, determinism, errors and failed allocations that change nothing, and the product path (sph_grid,
sph_slice, sph_ray, Visualizer.get_slice_image)."""
import ctypes

import numpy as np
import pytest

import lattice_ref
from test_density_cpu import within_one_ulp
from test_gpu_scratch_alloc_failure import (INDEX_SITES, Outputs, P, assert_same_state, col, frame_ctx, index_points,  # noqa: F401
                                            native, snapshot, walk)

pytestmark = pytest.mark.gpu
f32 = np.float32
EINVAL = -1
SHAPES = [(5, 3, 2), (1, 1, 1), (9, 1, 1), (70, 1, 1), (17, 13, 1), (8, 8, 8)]
_fp = ctypes.POINTER(ctypes.c_float)


@pytest.fixture(scope="module")
def ctx():
    from topsy_amd import _native
    c = _native.Context(64, 2)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _fields(n, count, seed=23):
    """strictly positive fields: the order of the float64 sums cannot cost more than the final rounding"""
    rs = np.random.RandomState(seed)
    return [rs.uniform(0.5, 2.0, size=n).astype(f32) for _ in range(count)]


def _spanning(shape, lo, hi, skew=0.013):
    """A lattice of `shape` whose points run from lo to hi on every axis (a single point along an axis sits at lo), slightly
    skewed so that no axis of it is an axis of the particles' grid."""
    step = [(hi - lo) / (m - 1) if m > 1 else 1.0 for m in shape]
    return dict(origin=(lo + 0.37, lo + 0.11, lo + 0.73), du=(step[0], skew * step[0], 0.0), dv=(0.0, step[1], -skew * step[1]),
                dw=(skew * step[2], 0.0, step[2]), shape=shape)


def _check(label, ctx, pos, fields, k, L, lat):
    """The GPU's (h, outs) of the lattice, held to the brute force at every point: h bit-equal, every field within one ulp."""
    h, outs = ctx.sph_sample_lattice(pos[:, 0], pos[:, 1], pos[:, 2], fields, k, L, **lat)
    nu, nv, nw = lat["shape"]
    assert h.dtype == outs.dtype == f32 and h.shape == (nw, nv, nu) and outs.shape == (len(fields), nw, nv, nu)
    want_h, want = lattice_ref.sample_lattice(pos, fields, k, L or 0.0, **lat)
    assert np.array_equal(_bits(h), _bits(want_h)), f"{label}: h differs at {np.argwhere(_bits(h) != _bits(want_h))[:5].tolist()}"
    ok = within_one_ulp(outs, want)
    equal = (_bits(outs) == _bits(want)) | (np.isnan(outs) & np.isnan(want))
    print(f"{label}: {h.size} points, fields {equal.mean() * 100:.2f} % bit-equal")
    assert ok.all(), (f"{label}: {np.count_nonzero(~ok)} of {outs.size} farther than one ulp, e.g. {np.argwhere(~ok)[:5].tolist()}: "
                      f"{outs[~ok][:5]} vs {want[~ok][:5]}")
    return h, outs, want_h, want


# ---- every brick shape, open and periodic ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("periodic", [False, True])
def test_matches_the_brute_force(ctx, periodic, shape):
    """Open: the lattice spans the particles' box.  Periodic (L = 25): the positions lie up to two periods outside the box and
    the lattice runs from -30 to 45, so most of its points lie outside it too."""
    pos, L = index_points(periodic)
    lat = _spanning(shape, -30.0, 45.0) if periodic else _spanning(shape, 0.5, 24.0)
    h, outs, _, _ = _check(f"periodic={periodic} {shape}", ctx, pos, _fields(len(pos), 2), 32, L, lat)
    assert np.isfinite(h).all() and (h > 0).all() and np.isfinite(outs).all() and (outs > 0).all()


def test_points_far_outside_the_bounding_box(ctx):
    """The particles fill [0, 25]^3; the lattice runs from -60 to 85 on every axis: most queries clamp into edge cells."""
    pos, L = index_points(False)
    lat = _spanning((6, 5, 4), -60.0, 85.0)
    pts = lattice_ref.lattice_points(**lat)
    assert ((pts < 0) | (pts > 25)).any(axis=-1).mean() > 0.9
    h, outs, _, _ = _check("outside", ctx, pos, _fields(len(pos), 1), 32, L, lat)
    assert np.isfinite(outs).all() and h.max() > 25.0


def test_rotated_lattice(ctx):
    a, b = 0.6, -1.1
    rot = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) @ \
        np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    for periodic in (False, True):
        pos, L = index_points(periodic)
        lat = dict(origin=np.array([12.0, 13.0, 11.0]) - 9.0 * rot.sum(axis=0), du=3.0 * rot[0], dv=3.6 * rot[1], dw=9.0 * rot[2],
                   shape=(7, 6, 3))
        _check(f"rotated, periodic={periodic}", ctx, pos, _fields(len(pos), 2), 16, L, lat)


# ---- every instantiation: KP of the search, W of the sums ----------------------------------------------------------------------
@pytest.mark.parametrize("k", [7, 8, 9, 32, 33, 64])
def test_every_neighbour_count(ctx, k):
    pos, L = index_points(False)
    _check(f"k={k}", ctx, pos, _fields(len(pos), 1), k, L, _spanning((5, 3, 2), -3.0, 27.0))


@pytest.mark.parametrize("n", [7, 32, 64])
def test_as_many_particles_as_neighbours(ctx, n):
    pos = index_points(False)[0][400:400 + n * 40:40]
    assert len(pos) == n
    h, outs, _, _ = _check(f"n=k={n}", ctx, pos, _fields(n, 2), n, 0.0, _spanning((5, 3, 2), -3.0, 27.0))
    assert np.isfinite(outs).all()


@pytest.mark.parametrize("n_fields", [1, 2, 3, 4])
def test_every_number_of_fields(ctx, n_fields):
    pos, L = index_points(True)
    fields = _fields(len(pos), n_fields)
    lat = _spanning((9, 6, 5), -30.0, 45.0)
    _, outs, _, _ = _check(f"{n_fields} fields", ctx, pos, fields, 32, L, lat)
    # a field's sum does not depend on the fields it travels with
    _, alone = ctx.sph_sample_lattice(pos[:, 0], pos[:, 1], pos[:, 2], fields[-1:], 32, L, **lat)
    assert np.array_equal(_bits(alone[0]), _bits(outs[-1]))


# ---- special inputs ------------------------------------------------------------------------------------------------------------
def test_duplicates_at_a_lattice_point(ctx):
    """40 particles on one lattice point, k = 32: h = 0 there and the fields are NaN; the points around it are finite and exact."""
    pos, L = index_points(False)
    pos = pos.copy()
    lat = dict(origin=(10.0, 10.0, 10.0), du=(0.5, 0, 0), dv=(0, 0.5, 0), dw=(0, 0, 0.5), shape=(5, 4, 3))
    pos[1000:1040] = (11.0, 10.5, 10.5)                     # lattice point (2, 1, 1)
    h, outs, _, _ = _check("duplicates", ctx, pos, _fields(len(pos), 2), 32, L, lat)
    assert h[1, 1, 2] == 0 and np.isnan(outs[:, 1, 1, 2]).all()
    rest = np.ones(h.shape, dtype=bool)
    rest[1, 1, 2] = False
    assert (h[rest] > 0).all() and np.isfinite(outs[:, rest]).all()


def test_particles_with_non_finite_coordinates_are_ignored(ctx):
    pos, L = index_points(True)
    fields = _fields(len(pos), 2)
    bad = np.array([5, 700, 1500, 2999, 17, 2000])
    keep = np.setdiff1d(np.arange(len(pos)), bad)
    dirty = pos.copy()
    dirty[bad[:2], 0] = np.nan
    dirty[bad[2:4], 1] = np.inf
    dirty[bad[4:], 2] = -np.inf
    lat = _spanning((9, 7, 3), -30.0, 45.0)
    h, outs, _, _ = _check("non-finite coordinates", ctx, dirty, fields, 32, L, lat)
    h_clean, outs_clean = ctx.sph_sample_lattice(pos[keep, 0], pos[keep, 1], pos[keep, 2], [a[keep] for a in fields], 32, L, **lat)
    assert np.array_equal(_bits(h), _bits(h_clean)) and np.array_equal(_bits(outs), _bits(outs_clean))
    assert np.isfinite(outs).all()


def test_a_nan_in_a_field_reaches_only_its_neighbourhood(ctx):
    pos, L = index_points(False)
    fields = _fields(len(pos), 2)
    fields[0][[100, 2200]] = np.nan
    fields[1][1700] = np.inf
    h, outs, _, want = _check("non-finite field values", ctx, pos, fields, 32, L, _spanning((8, 8, 8), 0.5, 24.0))
    assert np.array_equal(np.isnan(outs), np.isnan(want)) and np.array_equal(np.isinf(outs), np.isinf(want))
    assert 0 < np.isnan(outs[0]).sum() < outs[0].size // 4 and not np.isnan(outs[1]).any() and np.isinf(outs[1]).any()


def test_h_at_integer_particle_positions_is_the_particles_h(ctx):
    """Lattice points on particles: h_out is tsp_smoothing_lengths' h of those particles, bit for bit."""
    rs = np.random.RandomState(3)
    cells = rs.choice(12 ** 3, 700, replace=False)
    pos = np.stack([cells % 12, (cells // 12) % 12, cells // 144], axis=1).astype(f32)
    i, j, k = (pos[:, a].astype(int) for a in range(3))
    for L in (0.0, 12.0):
        h, _ = ctx.sph_sample_lattice(pos[:, 0], pos[:, 1], pos[:, 2], [np.ones(len(pos), dtype=f32)], 16, L, origin=(0, 0, 0),
                                      du=(1, 0, 0), dv=(0, 1, 0), dw=(0, 0, 1), shape=(12, 12, 12))
        own = ctx.smoothing_lengths(pos[:, 0], pos[:, 1], pos[:, 2], 16, L)
        assert np.array_equal(_bits(h[k, j, i]), _bits(own))


def test_signed_field_within_its_bound(ctx):
    """With terms of both signs the order of the float64 sum shows: two orders of T terms differ by at most 2 T 2^-53 A before
    the rounding to float32, A = sum |term| / (pi h^3) (the clause of tsp_sph_velocity_gradient's contract).  T < 2^27 here, so
    that is below 2^-24 A; the rounding to float32 adds one ulp of the result."""
    pos, L = index_points(True)
    rs = np.random.RandomState(7)
    fields = [rs.normal(size=len(pos)).astype(f32), rs.uniform(-1.0, 1.0, size=len(pos)).astype(f32)]
    lat = _spanning((9, 8, 5), -30.0, 45.0)
    h, outs = ctx.sph_sample_lattice(pos[:, 0], pos[:, 1], pos[:, 2], fields, 32, L, **lat)
    want_h, want, A, T = lattice_ref.sample_lattice(pos, fields, 32, L, with_bound=True, **lat)
    assert np.array_equal(_bits(h), _bits(want_h)) and T.max() < 2 ** 27 and np.isfinite(want).all()
    ulp = np.maximum(np.spacing(np.abs(outs)), np.spacing(np.abs(want))).astype(np.float64)
    err = np.abs(outs.astype(np.float64) - want.astype(np.float64))
    print(f"signed: largest error {np.max(err / (2.0 ** -24 * A + ulp)):.3f} of the bound, "
          f"{(_bits(outs) == _bits(want)).mean() * 100:.2f} % bit-equal")
    assert (err <= 2.0 ** -24 * A + ulp).all()
    assert (np.abs(want) < 0.1 * A).any()                    # cancellation does occur


def test_the_same_bits_again_and_on_another_context(ctx):
    from topsy_amd import _native
    pos, L = index_points(True)
    fields = _fields(len(pos), 3)
    lat = _spanning((17, 13, 1), -30.0, 45.0)
    args = (pos[:, 0], pos[:, 1], pos[:, 2], fields, 32, L)
    h, outs = ctx.sph_sample_lattice(*args, **lat)
    again = ctx.sph_sample_lattice(*args, **lat)
    assert np.array_equal(_bits(h), _bits(again[0])) and np.array_equal(_bits(outs), _bits(again[1]))
    other = _native.Context(16, 2)
    try:
        there = other.sph_sample_lattice(*args, **lat)
    finally:
        other.close()
    assert np.array_equal(_bits(h), _bits(there[0])) and np.array_equal(_bits(outs), _bits(there[1]))


def test_works_on_the_multi_gpu_context(ctx):
    from topsy_amd import multigpu
    pos, L = index_points(False)
    fields = _fields(len(pos), 2)
    lat = _spanning((5, 3, 2), 0.5, 24.0)
    want = ctx.sph_sample_lattice(pos[:, 0], pos[:, 1], pos[:, 2], fields, 32, L, **lat)
    mg = multigpu.MultiGpuContext(16, 2, [0, 0])
    try:
        got = mg.sph_sample_lattice(pos[:, 0], pos[:, 1], pos[:, 2], fields, 32, L, **lat)
    finally:
        mg.close()
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1]))


# ---- errors and resident state -------------------------------------------------------------------------------------------------
def _raw_call(native, lib, handle, pos, fields, k, L, lat, h_out, outs, n=None, n_fields=None):
    x, y, z = col(pos)
    keep = [x, y, z] + list(fields)
    nf = len(fields) if n_fields is None else n_fields
    fptr = (_fp * max(len(fields), 1))(*[P(a) for a in fields])
    optr = (_fp * max(len(outs), 1))(*[P(a) for a in outs])
    struct = lat if lat is None or isinstance(lat, native.Lattice) else native.lattice_struct(**lat)
    rc = lib.tsp_sph_sample_lattice(handle, len(pos) if n is None else n, P(x), P(y), P(z), nf, fptr, k, L,
                                    None if struct is None else ctypes.byref(struct), P(h_out), optr)
    del keep
    return rc


def test_invalid_arguments_change_nothing(native, frame_ctx):
    lib = native.load_library()
    pos, L = index_points(False)
    fields = _fields(len(pos), 2)
    good = dict(origin=(1, 2, 3), du=(2, 0, 0), dv=(0, 2, 0), dw=(0, 0, 2), shape=(5, 3, 2))
    outs = Outputs(h=np.empty(30, dtype=f32), a=np.empty(30, dtype=f32), b=np.empty(30, dtype=f32))
    before = snapshot(frame_ctx)

    def lattice(**changes):
        lat = native.lattice_struct(**good)
        for name, v in changes.items():
            if name in ("nu", "nv", "nw"):
                setattr(lat, name, v)
            else:
                getattr(lat, name)[:] = v
        return lat

    def call(pos=pos, fields=fields, k=32, period=L, lat=None, handle=frame_ctx._h, **kw):
        return _raw_call(native, lib, handle, pos, fields, k, period, lattice() if lat is None else lat, outs.h, [outs.a, outs.b], **kw)

    few_valid = pos[:40].copy()
    few_valid[10:, 0] = np.nan                                 # 10 particles with finite coordinates, k = 32
    cases = {
        "nu = 0": lambda: call(lat=lattice(nu=0)), "nv = -1": lambda: call(lat=lattice(nv=-1)), "nw = 0": lambda: call(lat=lattice(nw=0)),
        "2^31 points": lambda: call(lat=lattice(nu=2048, nv=1024, nw=1024)),
        "2^32 points": lambda: call(lat=lattice(nu=65536, nv=65536, nw=1)),
        "nan in du": lambda: call(lat=lattice(du=[np.nan, 0, 0])), "inf in origin": lambda: call(lat=lattice(origin=[0, np.inf, 0])),
        "-inf in dw": lambda: call(lat=lattice(dw=[0, 0, -np.inf])), "nan in dv": lambda: call(lat=lattice(dv=[0, np.nan, 0])),
        "a point beyond float32": lambda: call(lat=lattice(origin=[3.0e38, 0, 0], du=[2.0e37, 0, 0])),
        "a point beyond float32, last corner": lambda: call(lat=lattice(dw=[0, -3.3e38, 0], dv=[0, -1e37, 0])),
        "no field": lambda: call(n_fields=0), "five fields": lambda: call(n_fields=5), "k = 1": lambda: call(k=1),
        "k = 65": lambda: call(k=65), "k > n": lambda: call(pos=pos[:20], fields=[a[:20] for a in fields]),
        "fewer finite particles than k": lambda: call(pos=few_valid, fields=[a[:40] for a in fields]),
        "n = 0": lambda: call(n=0), "n = 2^31": lambda: call(n=1 << 31), "period < 0": lambda: call(period=-1.0),
        "period nan": lambda: call(period=float("nan")), "no context": lambda: call(handle=None),
        "no lattice": lambda: _raw_call(native, lib, frame_ctx._h, pos, fields, 32, L, None, outs.h, [outs.a, outs.b]),
        "a NULL field": lambda: _raw_call(native, lib, frame_ctx._h, pos, [fields[0], None], 32, L, good, outs.h, [outs.a, outs.b]),
        "a NULL output": lambda: _raw_call(native, lib, frame_ctx._h, pos, fields, 32, L, good, outs.h, [outs.a, None]),
    }
    for name, case in cases.items():
        outs.fill()
        assert case() == EINVAL, name
        assert not outs.written(), f"{name}: outputs written: {outs.written()}"
    assert_same_state(before, snapshot(frame_ctx), "after the refused calls")
    # the context is usable: the good call is right, with and without h_out
    outs.fill()
    assert call() == 0
    want_h, want = lattice_ref.sample_lattice(pos, fields, 32, L, **good)
    assert np.array_equal(_bits(outs.h), _bits(want_h.ravel()))
    assert within_one_ulp(outs.a, want[0].ravel()).all() and within_one_ulp(outs.b, want[1].ravel()).all()
    first = outs.a.copy()
    outs.fill()
    assert _raw_call(native, lib, frame_ctx._h, pos, fields, 32, L, good, None, [outs.a, outs.b]) == 0
    assert np.array_equal(_bits(outs.a), _bits(first)) and outs.written() == ["a", "b"]
    assert_same_state(before, snapshot(frame_ctx), "after the good calls")


@pytest.mark.parametrize("periodic", [False, True])
def test_failed_allocations_change_nothing(native, frame_ctx, periodic):
    """The k-th allocation of the call fails for k = 1, 2, ...: TSP_ENOMEM with the site's name, the outputs keep their sentinel,
    the context its image, counts and particles (walk() of test_gpu_scratch_alloc_failure.py).  The call adds no site: it
    reaches those of the index and the two of tsp_sph_sum."""
    lib = native.load_library()
    pos, L = index_points(periodic)
    fields = _fields(len(pos), 3)
    lat = _spanning((5, 3, 2), -30.0, 45.0)
    outs = Outputs(h=np.empty(30, dtype=f32), **{f"f{c}": np.empty(30, dtype=f32) for c in range(3)})
    expected = {"index_x", "index_y", "index_z", "index_bounds", "index_keys", "index_keys_sorted", "index_order",
                "index_order_sorted", "index_sort_tmp", "index_sorted_x", "index_sorted_y", "index_sorted_z", "sph_sum_h", "sph_sum_a"}
    assert expected <= INDEX_SITES | {"sph_sum_h", "sph_sum_a"}
    walk(native, frame_ctx,
         lambda: _raw_call(native, lib, frame_ctx._h, pos, fields, 32, L, lat, outs.h, [outs.f0, outs.f1, outs.f2]), outs, expected)
    want_h, want = lattice_ref.sample_lattice(pos, fields, 32, L, **lat)
    assert np.array_equal(_bits(outs.h), _bits(want_h.ravel()))
    assert all(within_one_ulp(getattr(outs, f"f{c}"), want[c].ravel()).all() for c in range(3))


# ---- the product path ----------------------------------------------------------------------------------------------------------
def _cloud2000():
    rs = np.random.RandomState(12)
    pos = np.concatenate([rs.normal(size=(1000, 3)) * 2.0, rs.uniform(-10, 10, size=(1000, 3))]).astype(f32)
    return pos, rs.uniform(0.5, 2.0, size=2000).astype(f32), rs.lognormal(size=2000).astype(f32)


def _mean_close(got, rho_got, want_outs):
    """mean = outs[0] / outs[1]: each sum within one ulp (2^-23) of the brute force's, the quotient rounded once on each side:
    3 x 2^-23 and the second order of that"""
    with np.errstate(all="ignore"):
        want = np.where(want_outs[1] == 0, np.nan, want_outs[0] / want_outs[1])
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = np.isnan(want) | (np.abs(got.astype(np.float64) - want) <= 3.5 * 2.0 ** -23 * np.abs(want))
    assert ok.all() and within_one_ulp(rho_got, want_outs[1]).all()


def test_sph_grid_slice_and_ray_agree_with_the_brute_force():
    import topsy_amd
    from topsy_amd import lattice
    pos, mass, temp = _cloud2000()
    a = 0.5
    rot = np.array([[np.cos(a), np.sin(a), 0], [-np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    fields = [mass * temp, mass]

    grid = topsy_amd.sph_grid(pos, mass, temp, shape=(6, 5, 4), center=(0.5, 0.0, -0.5), size=(8.0, 6.0, 4.0), rotation=rot, n_smooth=16)
    spec, offsets = lattice.box_lattice((6, 5, 4), (0.5, 0.0, -0.5), (8.0, 6.0, 4.0), rot)
    want_h, want = lattice_ref.sample_lattice(pos, fields, 16, 0.0, **spec)
    assert grid["rho"].shape == (4, 5, 6) and np.array_equal(_bits(grid["smooth"]), _bits(want_h))
    _mean_close(grid["mean"], grid["rho"], want)
    assert all(np.array_equal(p, o) for p, o in zip(grid["points"], offsets))
    only_rho = topsy_amd.sph_grid(pos, mass, shape=(6, 5, 4), center=(0.5, 0.0, -0.5), size=(8.0, 6.0, 4.0), rotation=rot, n_smooth=16)
    assert set(only_rho) == {"rho", "smooth", "points"} and np.array_equal(_bits(only_rho["rho"]), _bits(grid["rho"]))

    sl = topsy_amd.sph_slice(pos, mass, temp, resolution=9, center=(0, 0, 1.0), size=(12.0, 6.0), rotation=rot, n_smooth=16,
                             periodicity_scale=25.0)
    spec, _ = lattice.box_lattice((9, 9, 1), (0, 0, 1.0), (12.0, 6.0, 1.0), rot)
    want_h, want = lattice_ref.sample_lattice(pos, fields, 16, 25.0, **spec)
    assert sl["rho"].shape == (9, 9) and len(sl["points"]) == 2 and np.array_equal(_bits(sl["smooth"]), _bits(want_h[0]))
    _mean_close(sl["mean"], sl["rho"], want[:, 0])

    ray = topsy_amd.sph_ray(pos, mass, temp, start=(-12.0, 1.0, 0.5), end=(12.0, -2.0, 0.0), n_samples=70, n_smooth=16)
    step = (np.array([12.0, -2.0, 0.0]) - np.array([-12.0, 1.0, 0.5])) / 69
    want_h, want = lattice_ref.sample_lattice(pos, fields, 16, 0.0, (-12.0, 1.0, 0.5), step, (0, 0, 0), (0, 0, 0), (70, 1, 1))
    assert ray["rho"].shape == (70,) and ray["points"].shape == (70, 3) and np.array_equal(_bits(ray["smooth"]), _bits(want_h[0, 0]))
    _mean_close(ray["mean"], ray["rho"], want[:, 0, 0])
    assert np.allclose(ray["points"][-1], (12.0, -2.0, 0.0))


def test_get_slice_image_of_a_visualizer():
    """The slice of a rotated, offset view equals the brute force on the lattice of centre_on_pixel's convention (pinned by
    test_lattice_cpu.py), and the resident frame is what it was."""
    import topsy_amd
    from topsy_amd import lattice
    from topsy_amd.drawreason import DrawReason
    pos, mass, temp = _cloud2000()
    vis = topsy_amd.from_arrays(pos, None, mass, quantities={"temp": temp}, render_resolution=32, n_smooth=16)
    try:
        vis.scale = 8.0
        vis.rotate(0.3, 0.2)
        vis.position_offset = np.array([0.7, -0.4, 0.2])
        vis.render_sph(DrawReason.EXPORT)
        frame = np.array(vis.get_sph_image(), copy=True)
        assert np.count_nonzero(frame) > 100

        rho = vis.get_slice_image()
        mean = vis.get_slice_image("temp")
        small = vis.get_slice_image(resolution=8)
        ld = vis.data_loader
        fields = [ld.get_mass() * ld.get_named_quantity("temp"), ld.get_mass()]
        spec = lattice.slice_lattice(vis.rotation_matrix, vis.position_offset, vis.scale, 32)
        _, want = lattice_ref.sample_lattice(ld.get_positions(), fields, 16, 0.0, **spec)
        assert rho.shape == mean.shape == (32, 32) and rho.dtype == mean.dtype == f32 and small.shape == (8, 8)
        assert within_one_ulp(rho, want[1, 0]).all() and (rho > 0).all()
        _mean_close(mean, rho, want[:, 0])
        with pytest.raises(KeyError):
            vis.get_slice_image("pressure")
        after = np.array(vis.get_sph_image(), copy=True)
        assert np.array_equal(_bits(frame), _bits(after))

        # pixel (row, col) is the point centre_on_pixel(row, col) centres on, up to the depth it adds along the view axis
        pts = lattice_ref.lattice_points(**spec)[0].astype(np.float64)
        rot = np.asarray(vis.rotation_matrix, dtype=np.float64)
        centred = -np.asarray(vis.centre_on_pixel(5, 20), dtype=np.float64)
        across = rot[:2] @ (centred - pts[5, 20])
        assert np.abs(across).max() <= 1e-5 * vis.scale
    finally:
        vis.close()
