"""tsp_radial_profile on the GPU against radial_profile_reference (test_profile_cpu.py), on that file's scenes, and the Python
entries built on it.

Acceptance per scene, geometry and bin count: count_out, n_valid, n_inner and n_binned equal the reference's exactly (membership
is bit-determined by the contract, and test_profile_cpu.py shows that no particle lies within a relative 1e-9 of a bin edge or of
the disc's half height); mass and ms of a bin agree to n_bin * 2^-52 relative, n_bin the bin's member count (sums of positive
terms: any two orders agree to that); every mc and mj within 1e-9 * sum m |term| of that bin, every mc2 within 1e-9 relative.  Where
the tolerances come from (the derivation of test_gpu_orient.py's docstring): reordering a float64 sum of n terms errs by at most
about n * 2^-53 of the sum of their magnitudes, below 1e-12 at these sizes, whatever the order; a particle in the wrong bin moves
that bin's sums by about 1 / n_bin of them, 1e-4 and more.  So 1e-9 passes every summation order and catches every misbinned
particle.

On the integer lattice the counts, mass, mj and -- in the bins that hold one integer radius -- ms are exact, so equal to the
reference bit for bit in any order; the velocity components go through square roots and divisions and are held to the tolerances
above."""
import ctypes
import re

import numpy as np
import pytest

from test_profile_cpu import (AT, BIN_COUNTS, GEOMETRIES, HALF_HEIGHT, LATTICE_EDGES, LATTICE_OMEGA, LATTICE_THIN, MC, MC2, MJ, MS, MASS,
                              R_MAX, R_MIN, SCENES, TABLE_BIN_COUNTS, VIRIAL_SCENES, lattice_profile_scene, near_edge_margin, profile_blocks_read,
                              radial_profile_reference, reference, reference_shell_masses, scene, spec_of)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from topsy_amd import _native
    c = _native.Context(64, 2)
    yield c
    c.close()


def _columns(a):
    return None if a is None else tuple(np.ascontiguousarray(a[:, k]) for k in range(3))


def _call(ctx, pos, mass, vel, **spec):
    return ctx.radial_profile(pos[:, 0], pos[:, 1], pos[:, 2], mass, vel=_columns(vel), **spec)


def _bits(out):
    """Every output as integers: the floats by their bit patterns."""
    return {k: v if isinstance(v, int) else np.asarray(v).view(np.uint64).tolist() if np.asarray(v).dtype == np.float64 else v.tolist()
            for k, v in out.items()}


def _accept(label, got, ref):
    n_bin = ref["count"].astype(np.float64)
    err = np.abs(got["sums"] - ref["sums"])
    positive = n_bin[:, None] * 2.0 ** -52 * ref["sums"][:, :2]
    signed = 1e-9 * ref["scale"]
    print(f"{label}: valid {got['n_valid']} / {ref['n_valid']}, inner {got['n_inner']} / {ref['n_inner']}, binned {got['n_binned']} / "
          f"{ref['n_binned']}, worst |d mass, ms| / tolerance {np.max(err[:, :2] / np.maximum(positive, 1e-300)):.3g}, worst |d mc| / scale "
          f"{np.max(err[:, MC] / np.maximum(ref['scale'][:, MC], 1e-300)):.3g}, |d mc2| / mc2 {np.max(err[:, MC2] / np.maximum(ref['sums'][:, MC2], 1e-300)):.3g}, "
          f"|d mj| / scale {np.max(err[:, MJ] / np.maximum(ref['scale'][:, MJ], 1e-300)):.3g} (tolerance 1e-9)")
    assert sorted(got) == sorted(k for k in ref if k != "scale"), label
    assert got["count"].dtype == np.int64 and got["sums"].dtype == np.float64 and got["sums"].shape == (len(n_bin), 11)
    assert np.array_equal(got["count"], ref["count"]), label
    assert (got["n_valid"], got["n_inner"], got["n_binned"]) == (ref["n_valid"], ref["n_inner"], ref["n_binned"]), label
    assert abs(got["mass_inner"] - ref["mass_inner"]) <= max(ref["n_inner"], 1) * 2.0 ** -52 * ref["mass_inner"], label
    assert (err[:, :2] <= positive).all(), label
    assert (err[:, MC] <= signed[:, MC]).all() and (err[:, MJ] <= signed[:, MJ]).all(), label
    assert (err[:, MC2] <= 1e-9 * ref["sums"][:, MC2]).all(), label
    assert not np.signbit(got["sums"][ref["count"] == 0]).any() and not got["sums"][ref["count"] == 0].any(), label


@pytest.mark.parametrize("n_bins", BIN_COUNTS)
@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("name", SCENES)
def test_scene_against_the_reference(ctx, name, geometry, n_bins):
    pos, mass, vel, _ = scene(name)
    spec = spec_of(name, geometry, n_bins)
    assert near_edge_margin(pos, spec) > 1e-9
    got = _call(ctx, pos, mass, vel, **spec)
    _accept(f"{name}, geometry {geometry}, {n_bins} bins", got, reference(name, geometry, n_bins))
    # repeatability: the same call, the same bits
    assert _bits(got) == _bits(_call(ctx, pos, mass, vel, **spec))
    if vel is None:
        assert not got["sums"][:, 2:].any() and not np.signbit(got["sums"]).any()


@pytest.mark.parametrize("n_bins", TABLE_BIN_COUNTS)
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_either_side_of_the_table_threshold(ctx, geometry, n_bins, monkeypatch, capfd):
    """Up to 103 bins every wave of a workgroup has a table of its own, above they share one: both sides of the step."""
    pos, mass, vel, _ = scene("disc")
    spec = spec_of("disc", geometry, n_bins)
    assert near_edge_margin(pos, spec) > 1e-9
    monkeypatch.setenv("TOPSY_PROFILE_STATS", "1")
    capfd.readouterr()
    got = _call(ctx, pos, mass, vel, **spec)
    assert int(re.search(r" tables=(\d+) ", capfd.readouterr().err).group(1)) == (4 if n_bins == 103 else 1)
    _accept(f"disc, geometry {geometry}, {n_bins} bins", got, reference("disc", geometry, n_bins))
    assert _bits(got) == _bits(_call(ctx, pos, mass, vel, **spec))


@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("order", ["shuffled", "sorted"])
def test_exact_on_the_integer_lattice(ctx, order, geometry):
    """Counts, mass, mj and, in the bins of one integer radius, ms equal the reference bit for bit (exact sums: the module
    docstring); the lattice points exactly on an edge are in the bin that starts there, those on the half height take part, and
    the particles on the axis and at the centre take the fallback triads."""
    pos, mass, vel, spec = lattice_profile_scene(order)
    spec = dict(spec, geometry=geometry, half_height=2.0 if geometry else np.inf)
    ref = radial_profile_reference(pos, mass, vel, **spec)
    got = _call(ctx, pos, mass, vel, **spec)
    _accept(f"lattice {order}, geometry {geometry}", got, ref)
    for k in ("n_valid", "n_inner", "n_binned", "mass_inner"):
        assert got[k] == ref[k], k
    same = lambda a, b: np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))   # noqa: E731
    assert np.array_equal(got["count"], ref["count"]) and same(got["sums"][:, MASS], ref["sums"][:, MASS])
    assert same(got["sums"][:, MJ], ref["sums"][:, MJ])
    assert same(got["sums"][LATTICE_THIN, MS], ref["sums"][LATTICE_THIN, MS])
    assert same(got["sums"][LATTICE_THIN, MS], LATTICE_EDGES[LATTICE_THIN] * ref["sums"][LATTICE_THIN, MASS])
    # the edge radius 5 ((3, 4, 0) and its like) is in the bin [5, 5.05), not in [4.05, 5)
    d = pos.astype(np.float64) - np.asarray(spec["center"])
    dp = d @ np.asarray(spec["frame"]).T
    s2 = (d * d).sum(axis=1) if geometry == 0 else dp[:, 0] ** 2 + dp[:, 1] ** 2
    part = np.ones(len(d), dtype=bool) if geometry == 0 else np.abs(dp[:, 2]) <= 2.0
    assert got["count"][10] == (part & (s2 == 25.0)).sum() > 0
    assert got["count"][9] == (part & (s2 >= 4.05 ** 2) & (s2 < 25.0)).sum()
    assert _bits(got) == _bits(_call(ctx, pos, mass, vel, **spec))


def test_solid_body_rotation_on_the_lattice(ctx):
    from topsy_amd import loader
    pos, mass, vel, spec = lattice_profile_scene("shuffled", "solid")
    got = _call(ctx, pos, mass, vel, geometry=1, half_height=2.0, **spec)
    p = loader.Profile(spec["edges"], got["count"], got["sums"], got, "disc")
    for k in LATTICE_THIN:
        assert p.v_phi[k] == LATTICE_OMEGA * LATTICE_EDGES[k] and p.sigma_phi[k] == 0.0 and p.v_R[k] == 0.0 and p.v_z[k] == 0.0, k


@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("name", ["disc", "disc_sorted", "invalid"])
def test_blocks_outside_the_profile_are_not_read(ctx, name, geometry, monkeypatch, capfd):
    """TOPSY_PROFILE_STATS=1 reports the blocks the pass read: exactly those whose box reaches into the sphere of the last edge
    (the sphere around the cylinder), so in the sorted scene fewer than there are, and the sums are the shuffled scene's."""
    pos, mass, vel, _ = scene(name)
    spec = spec_of(name, geometry, 8)
    spec["edges"] = spec["edges"][:3].copy()            # R_MIN .. about 1: the outer slabs of the sorted scene lie outside
    assert near_edge_margin(pos, spec) > 1e-9
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(pos).all(axis=1) & np.isfinite(vel).all(axis=1) & np.isfinite(mass) & (mass > 0)
    monkeypatch.setenv("TOPSY_PROFILE_STATS", "1")
    capfd.readouterr()
    got = _call(ctx, pos, mass, vel, **spec)
    err = capfd.readouterr().err
    print(err)
    nblocks = int(re.search(r" blocks=(\d+) ", err).group(1))
    read = int(re.search(r"kernel_ms=\S+ blocks_read=(\d+)", err).group(1))
    assert nblocks == -(-len(pos) // 1024) == 7
    assert re.search(r"upload_ms=\S+ prepare_ms=\S+", err)
    assert read == profile_blocks_read(pos, valid, spec)
    if name == "disc_sorted":
        assert read < nblocks
    else:
        assert read == nblocks
    ref = radial_profile_reference(pos, mass, vel, **spec)
    _accept(f"{name}, geometry {geometry}", got, ref)
    if name == "disc_sorted":
        pos0, mass0, vel0, _ = scene("disc")
        _accept("sorted against shuffled", got, radial_profile_reference(pos0, mass0, vel0, **spec))
    if geometry == 1 and name == "disc_sorted":
        # an infinite height skips nothing
        monkeypatch.setenv("TOPSY_PROFILE_STATS", "1")
        tall = dict(spec, half_height=np.inf)
        got = _call(ctx, pos, mass, vel, **tall)
        err = capfd.readouterr().err
        assert int(re.search(r"blocks_read=(\d+)", err).group(1)) == nblocks
        _accept("infinite height", got, radial_profile_reference(pos, mass, vel, **tall))


def test_works_on_the_multi_gpu_context(ctx):
    from topsy_amd import multigpu
    pos, mass, vel, _ = scene("invalid")
    spec = spec_of("invalid", 1, 8)
    want = _call(ctx, pos, mass, vel, **spec)
    mg = multigpu.MultiGpuContext(16, 2, [0, 0])
    got = mg.radial_profile(pos[:, 0], pos[:, 1], pos[:, 2], mass, vel=_columns(vel), **spec)
    mg.close()
    assert _bits(got) == _bits(want)


# ---- errors: TSP_EINVAL, and nothing is written ---------------------------------------------------------------------------------
def test_invalid_arguments_write_nothing(ctx):
    from topsy_amd import _native
    lib = _native.load_library()
    assert lib.tsp_version() >= 116
    fp = ctypes.POINTER(ctypes.c_float)
    dp = ctypes.POINTER(ctypes.c_double)
    pos, mass, vel, _ = scene("disc")
    pos, mass, vel = pos[:700], mass[:700], vel[:700]
    n = len(pos)
    x, y, z = _columns(pos)
    vx, vy, vz = _columns(vel)
    m = np.ascontiguousarray(mass)
    P = lambda v: v.ctypes.data_as(fp)                                              # noqa: E731
    base = spec_of("disc", 1, 8)
    keep = []

    def make_spec(**changes):
        s = _native.ProfileSpec()
        v = dict(base, v_cen=(30.0, -12.0, 5.0), n_bins=None)
        v.update(changes)
        edges = np.ascontiguousarray(v["edges"], dtype=np.float64)
        keep.append(edges)
        s.geometry = v["geometry"]
        s.n_bins = len(edges) - 1 if v["n_bins"] is None else v["n_bins"]
        s.edges = edges.ctypes.data_as(dp) if v.get("edges_null") is None else None
        s.center[:] = list(v["center"])
        s.v_cen[:] = list(v["v_cen"])
        s.frame[:] = np.asarray(v["frame"], dtype=np.float64).ravel().tolist()
        s.half_height = v["half_height"]
        return s
    count = np.full(512, -7, dtype=np.int64)
    sums = np.full((512, 11), -7.0)
    info = _native.ProfileInfo()
    sentinel = bytes([0xA5]) * ctypes.sizeof(info)

    def reset():
        ctypes.memmove(ctypes.byref(info), sentinel, len(sentinel))
        count[:] = -7
        sums[:] = -7.0

    def untouched():
        return bytes(info) == sentinel and (count == -7).all() and (sums == -7.0).all()

    def call(s, **changes):
        a = dict(ctx=ctx._h, n=n, x=P(x), y=P(y), z=P(z), m=P(m), vx=P(vx), vy=P(vy), vz=P(vz),
                 spec=ctypes.byref(s), count=count.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                 sums=sums.ctypes.data_as(dp), info=ctypes.byref(info))
        a.update(changes)
        return lib.tsp_radial_profile(*a.values())
    reset()
    nan, inf = float("nan"), float("inf")
    e = base["edges"]
    skew = np.array([[1.0, 1e-3, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    bad_specs = [
        dict(edges=[0.0, 2.0, 1.0, 3.0]), dict(edges=[0.0, 1.0, 1.0]), dict(edges=[1.0, 0.5]),           # non-ascending
        dict(edges=[-0.5, 1.0]), dict(edges=[0.0, nan]), dict(edges=[0.0, inf]), dict(edges=[nan, 1.0]), dict(edges_null=True),
        dict(n_bins=0), dict(n_bins=513, edges=np.arange(514.0)), dict(n_bins=-3),
        dict(geometry=2), dict(geometry=-1),
        dict(center=(nan, 0.0, 0.0)), dict(center=(0.0, inf, 0.0)), dict(center=(0.0, 0.0, -inf)),           # a non-finite centre
        dict(v_cen=(nan, 0.0, 0.0)), dict(v_cen=(0.0, 0.0, inf)),
        dict(frame=np.eye(3) * 1.001), dict(frame=skew), dict(frame=np.zeros((3, 3))), dict(frame=np.full((3, 3), nan)),
        dict(half_height=0.0), dict(half_height=-1.0), dict(half_height=nan), dict(half_height=-inf),
    ]
    for changes in bad_specs:
        assert call(make_spec(**changes)) == -1 and untouched(), changes             # TSP_EINVAL
        assert lib.tsp_last_error()
    good = make_spec()
    zeros = np.zeros(n, dtype=np.float32)
    nans = np.full(n, np.nan, dtype=np.float32)
    bad_calls = [dict(ctx=None), dict(n=0), dict(n=-5), dict(n=1 << 31), dict(x=None), dict(y=None), dict(z=None), dict(m=None),
                 dict(spec=None), dict(count=None), dict(sums=None),
                 # only one or two of the three velocity arrays
                 dict(vx=None), dict(vy=None), dict(vz=None), dict(vx=None, vy=None), dict(vx=None, vz=None), dict(vy=None, vz=None),
                 # no valid particle
                 dict(m=P(zeros)), dict(x=P(nans)), dict(vy=P(nans)), dict(m=P(nans), vx=None, vy=None, vz=None)]
    for changes in bad_calls:
        assert call(good, **changes) == -1, changes
        assert untouched() or changes.keys() & {"count", "sums"}, changes
        assert lib.tsp_last_error()

    # the good call on the same context: the reference's answer; info_out is optional; geometry 0 ignores the half height, and
    # without velocities v_cen
    ref = radial_profile_reference(pos, mass, vel, **dict(base, v_cen=(30.0, -12.0, 5.0)))
    assert call(good) == 0
    got = {"count": count[:8].copy(), "sums": sums[:8].copy(), "n_valid": info.n_valid, "n_inner": info.n_inner,
           "n_binned": info.n_binned, "mass_inner": info.mass_inner}
    _accept("one block, C call", got, ref)
    assert (count[8:] == -7).all() and (sums[8:] == -7.0).all()
    reset()
    assert call(good, info=None) == 0 and np.array_equal(count[:8], ref["count"]) and bytes(info) == sentinel
    reset()
    assert call(make_spec(geometry=0, half_height=nan)) == 0
    assert np.array_equal(count[:8], radial_profile_reference(pos, mass, vel, **dict(base, geometry=0, v_cen=(30.0, -12.0, 5.0)))["count"])
    reset()
    assert call(make_spec(v_cen=(nan, nan, nan)), vx=None, vy=None, vz=None) == 0
    assert np.array_equal(count[:8], radial_profile_reference(pos, mass, None, **base)["count"]) and not sums[:8, 2:].any()
    # a profile without a member is no error
    reset()
    assert call(make_spec(center=(1e6, 0.0, 0.0))) == 0
    assert not count[:8].any() and not sums[:8].any() and (info.n_valid, info.n_inner, info.n_binned, info.mass_inner) == (n, 0, 0, 0.0)
    # one particle, one bin that starts at its radius, 0
    reset()
    assert call(make_spec(center=tuple(pos[0].astype(np.float64)), edges=[0.0, 1.0], geometry=0), n=1) == 0
    assert count[0] == 1 and sums[0, 0] == float(mass[0]) and sums[0, 1] == 0.0 and (info.n_valid, info.n_binned) == (1, 1)


# ---- the Python entries ---------------------------------------------------------------------------------------------------------
SMOOTH, RES = 0.1, 64


def _profile_matches(label, p, ref):
    _accept(label, {"count": p.count, "sums": p.sums, **{k: p.info[k] for k in ("n_valid", "n_inner", "n_binned", "mass_inner")}}, ref)


def test_python_entries(ctx):
    import topsy_amd
    from topsy_amd import loader
    from test_orient_cpu import sphere_moments_reference
    pos, mass, vel, base = scene("disc")
    # explicit everything: the reference's sums, and the same bits as the context call
    p = topsy_amd.radial_profile(pos, mass, vel, center=AT, r_max=R_MAX, r_min=R_MIN, n_bins=8, geometry="disc", frame=base["frame"],
                                 half_height=HALF_HEIGHT, v_cen=base["v_cen"], G=2.0)
    ref = reference("disc", 1, 8)
    _profile_matches("topsy_amd.radial_profile, disc", p, ref)
    assert isinstance(p, topsy_amd.Profile) and p.geometry == "disc" and len(p) == 8
    assert np.array_equal(p.sums.view(np.uint64), _call(ctx, pos, mass, vel, **spec_of("disc", 1, 8))["sums"].view(np.uint64))
    want = loader.Profile(p.edges, ref["count"], ref["sums"], ref, "disc", G=2.0)
    for name in ("mass", "mass_enc", "density", "r_mean", "v_R", "v_phi", "v_z", "sigma_R", "sigma_phi", "sigma_z", "v_circ"):
        assert np.allclose(getattr(p, name), getattr(want, name), rtol=1e-9, atol=1e-9), name
    assert np.abs(p.v_phi[1:6] - 1.0).max() < 0.1          # the disc's flat rotation curve
    # the defaults: shells in the identity frame about the velocity of the inner fifth; log bins
    p = topsy_amd.radial_profile(pos, mass, vel, center=AT, r_max=R_MAX, r_min=R_MIN, n_bins=8, bins="log")
    v_cen = sphere_moments_reference(pos, mass, vel, center=AT, r=R_MAX, r_vel=0.2 * R_MAX)["v_cen"]
    assert np.abs(p.info["v_cen"] - v_cen).max() <= 1e-9
    edges = loader.profile_edges("log", 8, R_MIN, R_MAX)
    assert near_edge_margin(pos, dict(edges=edges, geometry=0, center=AT)) > 1e-9
    _profile_matches("topsy_amd.radial_profile, defaults", p,
                     radial_profile_reference(pos, mass, vel, edges=edges, geometry=0, center=AT, v_cen=p.info["v_cen"]))
    assert p.geometry == "sphere" and p.v_circ is None and p.v_theta is not None
    # without velocities
    p = topsy_amd.radial_profile(pos, mass, center=AT, bins=[0.5, 1.0, 3.0])
    assert p.v_r is None and p.j is None and np.array_equal(p.n, radial_profile_reference(pos, mass, None, edges=[0.5, 1.0, 3.0], center=AT)["count"])


@pytest.mark.parametrize("name", sorted(VIRIAL_SCENES))
def test_virial_radius(name):
    """The same rule on the GPU's shell masses and on the reference's: the brackets agree (a mass differs in its last bits, a
    bracket only where the density is within that of the threshold at an edge) and the radii to the interpolation's rounding."""
    import topsy_amd
    from topsy_amd import loader
    pos, mass, threshold, r_max = VIRIAL_SCENES[name]
    want, (lower, upper) = loader.find_virial_radius(reference_shell_masses(pos, mass, AT), threshold, r_max, 3)
    got = topsy_amd.virial_radius(pos, mass, AT, threshold, r_max)
    print(f"{name}: r_vir {got!r}, reference {want!r}, last bracket [{lower!r}, {upper!r}]")
    assert lower <= got <= upper and abs(got - want) <= upper - lower
    coarse = topsy_amd.virial_radius(pos, mass, AT, threshold, r_max, refinements=0)
    assert abs(coarse - got) <= r_max * (1024.0 ** (1.0 / 256.0) - 1.0)
    with pytest.raises(ValueError, match="never falls"):
        topsy_amd.virial_radius(pos, mass, AT, threshold * 1e9, r_max)


def test_vis_profile_and_scale_to_virial():
    import topsy_amd
    from topsy_amd import loader
    pos, mass, vel, base = scene("disc")
    h = np.full(len(pos), SMOOTH, dtype=np.float32)
    vis = topsy_amd.from_arrays(pos, h, mass, vel=vel, center=AT, render_resolution=RES)
    other = None
    try:
        # the profile of what the view shows: about -position_offset, in the view's frame
        R = vis.orient("faceon", R_MAX)
        p = vis.profile(R_MAX, r_min=R_MIN, n_bins=8, geometry="disc", half_height=HALF_HEIGHT)
        ld = vis.data_loader
        spec = dict(edges=loader.profile_edges("lin", 8, R_MIN, R_MAX), geometry=1, center=AT, frame=R, half_height=HALF_HEIGHT,
                    v_cen=p.info["v_cen"])
        assert near_edge_margin(ld.get_positions(), spec) > 1e-9
        ref = radial_profile_reference(ld.get_positions(), ld.get_mass(), ld.get_velocities(), **spec)
        _profile_matches("vis.profile, face-on disc", p, ref)
        want = loader.Profile(spec["edges"], ref["count"], ref["sums"], ref, "disc")
        assert np.allclose(p.v_phi, want.v_phi, rtol=0, atol=1e-9) and np.abs(p.v_phi[1:6] - 1.0).max() < 0.1
        assert np.abs(p.v_R[:6]).max() < 0.05
        # unoriented the same call bins about the z axis of the data: no rotation curve
        vis.rotation_matrix = np.eye(3)
        tilted = vis.profile(R_MAX, r_min=R_MIN, n_bins=8, geometry="disc", half_height=HALF_HEIGHT)
        assert np.abs(tilted.v_phi[1:6] - p.v_phi[1:6]).max() > 0.1
        # explicit centre and frame; the surface view forwards
        view = topsy_amd.SurfaceView(vis)
        q = view.profile(R_MAX, r_min=R_MIN, n_bins=8, geometry="disc", half_height=HALF_HEIGHT, frame=R, center=AT)
        assert np.array_equal(q.sums.view(np.uint64), p.sums.view(np.uint64))
        # away from everything the profile is empty, not an error
        vis.position_offset = -(AT + [500.0, 0.0, 0.0])
        empty = vis.profile(1.0, v_cen=(0.0, 0.0, 0.0))
        assert empty.info["n_binned"] == 0 and np.isnan(empty.v_r).all() and not empty.mass.any()
        with pytest.raises(ValueError, match="ring"):
            vis.profile(R_MAX, geometry="ring")

        # the virial radius of what the view is centred on sets the scale
        vis.position_offset = -AT
        d = np.sqrt(((pos.astype(np.float64) - AT) ** 2).sum(axis=1))
        threshold = 3.0 * mass[d < 3.0].astype(np.float64).sum() / (4.0 * np.pi * 27.0)
        want, bracket = loader.find_virial_radius(reference_shell_masses(ld.get_positions(), ld.get_mass(), AT), threshold, 6.0, 3)
        before = vis.scale
        assert vis.scale_to_virial(threshold, 6.0) == vis.scale != before
        assert bracket[0] <= vis.scale <= bracket[1] and abs(vis.scale - want) <= bracket[1] - bracket[0]
        assert view.scale_to_virial(threshold, 6.0, factor=2.0) == vis.scale and abs(vis.scale - 2.0 * want) <= 2.0 * (bracket[1] - bracket[0])
        with pytest.raises(ValueError, match="factor"):
            vis.scale_to_virial(threshold, 6.0, factor=0.0)
        with pytest.raises(ValueError, match="never falls"):
            vis.scale_to_virial(threshold * 1e9, 6.0)
        assert abs(vis.scale - 2.0 * want) <= 2.0 * (bracket[1] - bracket[0])
        # another loader has no host arrays
        other = topsy_amd.test(1000, render_resolution=RES)
        before = other.scale
        with pytest.raises(ValueError, match="TestDataLoader"):
            other.profile(10.0)
        with pytest.raises(ValueError, match="TestDataLoader"):
            other.scale_to_virial(1.0, 10.0)
        with pytest.raises(ValueError, match="TestDataLoader"):
            topsy_amd.SurfaceView(other).profile(10.0)
        assert other.scale == before
    finally:
        for v in (vis, other):
            if v is not None:
                v.close()
