"""The orientation of a view on the CPU: sphere_moments_reference, the NumPy float64 restatement of the contract of
tsp_sphere_moments (include/topsy_splat.h) that test_gpu_orient.py holds the GPU to; the scenes both files use, with the property
of the inputs that the GPU comparison relies on (no particle within a relative 1e-9 of either sphere's surface) established here
by the reference alone; orientation_matrix against pynbody's formula; and the loader's logic with a context stubbed by the
reference, which needs no GPU."""
import functools

import numpy as np
import pytest

AXIS = np.array([0.48, -0.6, 0.64])             # the disc's unit axis
AT = np.array([120.5, -63.25, 40.0])            # where the scene sits: displacements must be formed in float64
BOOST = np.array([30.0, -12.0, 5.0])
R_SPHERE, R_VEL = 4.0, 0.8


def sphere_moments_reference(pos, mass, vel=None, center=(0.0, 0.0, 0.0), r=1.0, r_vel=0.0):
    """The contract in float64 (numpy's pairwise sums; no fused multiply-adds).  Returns the fields of struct tsp_moments as a
    dict, and for the tolerances of the GPU comparison "sum_md2" = sum m d2 over the r sphere and "max_u_vel" = max |v - v_cen|
    over the r_vel sphere (0 without velocities).  ValueError where the library returns TSP_EINVAL for the data."""
    pos = np.asarray(pos, dtype=np.float32)
    mass = np.asarray(mass, dtype=np.float32)
    c = np.asarray(center, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        valid = np.isfinite(pos).all(axis=1) & np.isfinite(mass) & (mass > 0)
        if vel is not None:
            vel = np.asarray(vel, dtype=np.float32)
            valid &= np.isfinite(vel).all(axis=1)
        if not valid.any():
            raise ValueError("no valid particle")
        d = pos.astype(np.float64) - c
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        inside = valid & (d2 < r * r)
        inside_vel = valid & (d2 < r_vel * r_vel)
    out = {"n_valid": int(valid.sum()), "n_inside": int(inside.sum()), "n_inside_vel": 0, "mass_vel": 0.0,
           "v_cen": np.zeros(3), "L": np.zeros(3), "A": 0.0, "max_u_vel": 0.0}
    if vel is not None:
        if not inside_vel.any():
            raise ValueError("the r_vel sphere is empty")
        mv = mass[inside_vel].astype(np.float64)
        vv = vel[inside_vel].astype(np.float64)
        out["n_inside_vel"] = int(inside_vel.sum())
        out["mass_vel"] = float(mv.sum())
        out["v_cen"] = (mv[:, None] * vv).sum(axis=0) / mv.sum()
        out["max_u_vel"] = float(np.sqrt(((vv - out["v_cen"]) ** 2).sum(axis=1)).max())
    if not inside.any():
        raise ValueError("the r sphere is empty")
    m = mass[inside].astype(np.float64)
    dx, dy, dz = d[inside, 0], d[inside, 1], d[inside, 2]
    out["mass"] = float(m.sum())
    out["com"] = np.array([(m * dx).sum(), (m * dy).sum(), (m * dz).sum()]) / m.sum()
    out["S"] = np.array([((m * dx) * dx).sum(), ((m * dx) * dy).sum(), ((m * dx) * dz).sum(), ((m * dy) * dy).sum(),
                         ((m * dy) * dz).sum(), ((m * dz) * dz).sum()])
    out["sum_md2"] = float((m * d2[inside]).sum())
    if vel is not None:
        u = vel[inside].astype(np.float64) - out["v_cen"]
        ux, uy, uz = u[:, 0], u[:, 1], u[:, 2]
        out["L"] = np.array([(m * (dy * uz - dz * uy)).sum(), (m * (dz * ux - dx * uz)).sum(), (m * (dx * uy - dy * ux)).sum()])
        out["A"] = float(((m * np.sqrt(d2[inside])) * np.sqrt((ux * ux + uy * uy) + uz * uz)).sum())
    return out


def near_tie_margin(pos, center, r, r_vel=0.0):
    """min | d2 / s^2 - 1 | over the particles with finite coordinates and s = r and, if > 0, r_vel: how far the inputs are from
    a membership that a rounding difference could flip."""
    pos = np.asarray(pos, dtype=np.float32)
    p = pos[np.isfinite(pos).all(axis=1)].astype(np.float64) - np.asarray(center, dtype=np.float64)
    d2 = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
    return min(float(np.abs(d2 / (s * s) - 1.0).min()) for s in (r, r_vel) if s > 0)


def angle_between(a, b):
    """The angle in radians between two vectors, well-conditioned near 0 (atan2 of |a x b| and a . b)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.arctan2(np.linalg.norm(np.cross(a, b)), np.dot(a, b)))


# ---- scenes ---------------------------------------------------------------------------------------------------------------
def disc_snapshot(seed=7, n_disc=6000, n_halo=600):
    """A thin rotating disc about AXIS (R ~ Gamma(2, 1), thickness sigma 0.05, circular speed 1, velocity noise sigma 0.1) in a
    hot halo (uniform in a ball of radius 6, velocity sigma 0.7), at AT, moving with BOOST, shuffled.  float32 (n, 3) pos and vel,
    unit-scale masses."""
    rs = np.random.RandomState(seed)
    e1 = np.cross(AXIS, [0.0, 0.0, 1.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(AXIS, e1)                     # e1 x e2 = AXIS: the rotation is right-handed about AXIS
    radius = rs.gamma(2.0, 1.0, size=n_disc)
    phi = rs.uniform(0.0, 2 * np.pi, size=n_disc)
    height = rs.normal(scale=0.05, size=n_disc)
    disc = (radius * np.cos(phi))[:, None] * e1 + (radius * np.sin(phi))[:, None] * e2 + height[:, None] * AXIS
    disc_v = (-np.sin(phi))[:, None] * e1 + np.cos(phi)[:, None] * e2 + rs.normal(scale=0.1, size=(n_disc, 3))
    halo = rs.normal(size=(n_halo, 3))
    halo *= (6.0 * rs.uniform(size=n_halo) ** (1.0 / 3.0) / np.linalg.norm(halo, axis=1))[:, None]
    halo_v = rs.normal(scale=0.7, size=(n_halo, 3))
    order = rs.permutation(n_disc + n_halo)
    pos = (np.concatenate([disc, halo]) + AT)[order].astype(np.float32)
    vel = (np.concatenate([disc_v, halo_v]) + BOOST)[order].astype(np.float32)
    mass = rs.uniform(0.5, 1.5, size=len(pos)).astype(np.float32)
    return pos, vel, mass


def blocks_read(pos, valid, center, s, block=1024):
    """How many blocks of `block` consecutive particles a pass over the sphere of radius s reads: those whose valid members'
    float32 bounding box lies at a squared distance < s^2 from the centre, the distance formed like d2 (an empty block: none)."""
    c = np.asarray(center, dtype=np.float64)
    count = 0
    for start in range(0, len(pos), block):
        p = pos[start:start + block][valid[start:start + block]].astype(np.float64)
        if len(p) == 0:
            continue
        g = np.maximum(np.maximum(p.min(axis=0) - c, c - p.max(axis=0)), 0.0)
        count += bool((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2] < s * s)
    return count


@functools.lru_cache(maxsize=None)
def scene(name):
    """(pos float32 (n, 3), mass float32 (n,), vel float32 (n, 3) or None, keyword arguments center, r, r_vel of the call)."""
    pos, vel, mass = disc_snapshot()
    kw = dict(center=tuple(AT), r=R_SPHERE, r_vel=R_VEL)
    if name == "disc":
        pass
    elif name == "disc_sorted":
        order = np.argsort(pos[:, 0], kind="stable")
        pos, vel, mass = pos[order], vel[order], mass[order]
    elif name == "invalid":
        rs = np.random.RandomState(10)
        n = len(pos)
        for array in (pos, vel):
            bad = rs.choice(n, n // 60, replace=False)
            array[bad, rs.randint(0, 3, size=len(bad))] = rs.choice([np.nan, np.inf, -np.inf], size=len(bad))
        for value in (0.0, -1.0, np.nan, np.inf, -0.0, -np.inf):
            mass[rs.choice(n, 40, replace=False)] = value
    elif name == "no_vel":
        vel = None
        kw["r_vel"] = 0.0
    elif name == "one_block":
        pos, vel, mass = pos[:700].copy(), vel[:700].copy(), mass[:700].copy()
    else:
        raise KeyError(name)
    for a in (pos, vel, mass):
        if a is not None:
            a.setflags(write=False)
    return pos, mass, vel, kw


SCENES = ("disc", "disc_sorted", "invalid", "no_vel", "one_block")


@functools.lru_cache(maxsize=None)
def reference(name):
    pos, mass, vel, kw = scene(name)
    return sphere_moments_reference(pos, mass, vel, **kw)


LATTICE_AT = np.array([3.0, -2.0, 1.0])
LATTICE_BOOST = np.array([2.0, -1.0, 3.0])
LATTICE_SPIN = np.array([1.0, 2.0, 3.0])


def lattice_scene(order="shuffled"):
    """The integer lattice {-6..6}^3 about LATTICE_AT with unit masses and the integer velocities LATTICE_SPIN x d +
    LATTICE_BOOST: every product and every sum of the contract except A's square roots is an integer far below 2^53, so exact in
    any order.  r = 5 and r_vel = 3 both have lattice points exactly on the sphere ((3, 4, 0), (3, 0, 0), (2, 2, 1)), which are
    outside; it is therefore kept apart from SCENES, whose margin test it cannot pass."""
    g = np.arange(-6, 7, dtype=np.float64)
    d = np.stack([v.ravel() for v in np.meshgrid(g, g, g, indexing="ij")], axis=1)
    if order == "shuffled":
        d = d[np.random.RandomState(21).permutation(len(d))]
    pos = (d + LATTICE_AT).astype(np.float32)
    vel = (np.cross(LATTICE_SPIN, d) + LATTICE_BOOST).astype(np.float32)
    return pos, np.ones(len(pos), dtype=np.float32), vel, dict(center=tuple(LATTICE_AT), r=5.0, r_vel=3.0)


# ---- the reference and the inputs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_scenes_have_no_near_ties(name):
    pos, mass, vel, kw = scene(name)
    ref = reference(name)
    margin = near_tie_margin(pos, kw["center"], kw["r"], kw["r_vel"])
    print(f"{name}: n = {len(pos)}, valid {ref['n_valid']}, inside r {ref['n_inside']}, inside r_vel {ref['n_inside_vel']}, "
          f"nearest tie {margin:.3g}, |L| / A = {np.linalg.norm(ref['L']) / ref['A'] if ref['A'] else 0:.3g}")
    assert margin > 1e-9
    assert ref["n_inside"] > 100 and (vel is None or ref["n_inside_vel"] > 50)


def test_scene_properties():
    """What each scene is for, shown by the reference."""
    pos, mass, vel, kw = scene("disc")
    ref = reference("disc")
    # several blocks of 1024 with a ragged last one; both spheres hold a good part of the disc, the small one far fewer
    assert len(pos) == 6600 and len(pos) % 1024 != 0 and ref["n_valid"] == 6600
    assert 5000 < ref["n_inside"] < 6600 and 500 < ref["n_inside_vel"] < ref["n_inside"] / 3
    # L points along the disc's axis (the halo is hot and isotropic: it tilts L by its shot noise only), the rotation is ordered
    assert np.degrees(angle_between(ref["L"], AXIS)) < 0.5
    assert np.linalg.norm(ref["L"]) / ref["A"] > 0.85
    assert np.linalg.norm(ref["v_cen"] - BOOST) < 0.1 and np.linalg.norm(ref["com"]) < 0.1
    # the offset is the point: float32 displacements would be wrong by their spacing at |AT|, far above the tolerance
    assert np.spacing(np.float32(120.5)) * ref["mass"] > 1e2 * 1e-9 * ref["sum_md2"]
    # sorted: the same sums up to their order
    srt = reference("disc_sorted")
    assert (srt["n_inside"], srt["n_inside_vel"]) == (ref["n_inside"], ref["n_inside_vel"])
    assert np.allclose(srt["L"], ref["L"], rtol=0, atol=1e-11 * ref["A"])
    # sorted along x the 7 blocks are slabs, and the outer ones lie wholly outside the small sphere; shuffled, every block
    # reaches into both spheres
    everyone = np.ones(len(pos), dtype=bool)
    assert blocks_read(scene("disc_sorted")[0], everyone, AT, R_VEL) <= 4 and blocks_read(pos, everyone, AT, R_VEL) == 7
    assert blocks_read(pos, everyone, AT, R_SPHERE) == 7
    # invalid data: the valid count is what the rule says, and all three kinds of bad value occur
    pos, mass, vel, _ = scene("invalid")
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(pos).all(axis=1) & np.isfinite(vel).all(axis=1) & np.isfinite(mass) & (mass > 0)
    inv = reference("invalid")
    assert inv["n_valid"] == int(ok.sum()) < len(pos) - 300
    assert (~np.isfinite(pos).all(axis=1)).sum() > 50 and (~np.isfinite(vel).all(axis=1)).sum() > 50
    assert inv["n_inside"] < ref["n_inside"] and np.isfinite(inv["L"]).all() and np.isfinite(inv["S"]).all()
    # no velocities: zeros where the contract says so, and the minor axis of the shape is the disc's axis
    nov = reference("no_vel")
    assert nov["n_inside_vel"] == 0 and nov["mass_vel"] == 0 and nov["A"] == 0 and not nov["L"].any() and not nov["v_cen"].any()
    assert np.array_equal(nov["S"], ref["S"]) and nov["mass"] == ref["mass"]
    from topsy_amd import loader
    axis = loader.orientation_axis(nov, "shape")
    assert np.degrees(min(angle_between(axis, AXIS), angle_between(-axis, AXIS))) < 2.0
    # one block: a single ragged block
    assert len(scene("one_block")[0]) == 700


def test_lattice_reference_is_exact():
    for order in ("shuffled", "sorted"):
        pos, mass, vel, kw = lattice_scene(order)
        assert len(pos) == 13 ** 3 and len(pos) % 1024 != 0
        ref = sphere_moments_reference(pos, mass, vel, **kw)
        d = pos.astype(np.float64) - LATTICE_AT
        d2 = (d ** 2).sum(axis=1)
        assert ref["n_inside"] == int((d2 < 25).sum()) < int((d2 <= 25).sum())
        assert ref["n_inside_vel"] == int((d2 < 9).sum()) < int((d2 <= 9).sum())
        assert ref["mass"] == ref["n_inside"] and ref["mass_vel"] == ref["n_inside_vel"]
        assert np.array_equal(ref["v_cen"], LATTICE_BOOST) and np.array_equal(ref["com"], np.zeros(3))
        # L = sum d x (w x d) = sum (w d2 - d (d . w)): by the cubic symmetry of the set, w * (2 / 3) sum d2
        inside = d2 < 25
        assert np.array_equal(ref["L"], LATTICE_SPIN * (2.0 * d2[inside].sum() / 3.0))
        third = d2[inside].sum() / 3.0
        assert np.array_equal(ref["S"], [third, 0.0, 0.0, third, 0.0, third])


# ---- orientation_matrix -----------------------------------------------------------------------------------------------------
def pynbody_calc_faceon_matrix(angmom_vec, up=[0.0, 1.0, 0.0]):
    """pynbody.analysis.angmom.calc_faceon_matrix, transcribed."""
    vec_in = np.asarray(angmom_vec)
    vec_in = vec_in / np.sum(vec_in ** 2).sum() ** 0.5
    vec_p1 = np.cross(up, vec_in)
    vec_p1 = vec_p1 / np.sum(vec_p1 ** 2).sum() ** 0.5
    vec_p2 = np.cross(vec_in, vec_p1)
    matr = np.concatenate((vec_p1, vec_p2, vec_in)).reshape((3, 3))
    return matr


def _moments_with(L=(0.0, 0.0, 1.0), A=1.0, S=(1.0, 0.0, 0.0, 1.0, 0.0, 0.5), com=(0.0, 0.0, 0.0), mass=1.0):
    return {"L": np.asarray(L, dtype=np.float64), "A": float(A), "S": np.asarray(S, dtype=np.float64),
            "com": np.asarray(com, dtype=np.float64), "mass": float(mass)}


def _is_rotation(R):
    return np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(R) - 1.0) <= 1e-12


def test_faceon_matrix_is_pynbodys():
    from topsy_amd import loader
    rs = np.random.RandomState(3)
    for L in rs.normal(size=(50, 3)) * 10.0 ** rs.uniform(-3, 8, size=(50, 1)):
        R = loader.orientation_matrix(_moments_with(L=L, A=np.linalg.norm(L) * 2), "faceon", "angmom")
        assert R.shape == (3, 3) and R.dtype == np.float64
        assert np.abs(R - pynbody_calc_faceon_matrix(L)).max() <= 1e-15
        a = L / np.linalg.norm(L)
        assert np.abs(R @ a - [0.0, 0.0, 1.0]).max() <= 1e-12 and _is_rotation(R)
        side = loader.orientation_matrix(_moments_with(L=L, A=np.linalg.norm(L) * 2), "sideon", "angmom")
        assert np.abs(side @ a - [0.0, 1.0, 0.0]).max() <= 1e-12 and _is_rotation(side)
        # the disc plane's first direction stays along x
        assert np.abs(side[0] - R[0]).max() == 0.0
        up = rs.normal(size=3)
        assert np.abs(loader.orientation_matrix(_moments_with(L=L, A=1.0), "faceon", "angmom", up=up)
                      - pynbody_calc_faceon_matrix(L, up)).max() <= 1e-14


def test_up_parallel_to_the_axis_takes_the_fallback():
    from topsy_amd import loader
    for L in ((0.0, 3.0, 0.0), (0.0, -2.0, 0.0), (1e-8, 5.0, 0.0)):
        R = loader.orientation_matrix(_moments_with(L=L, A=10.0), "faceon", "angmom")
        a = np.asarray(L) / np.linalg.norm(L)
        assert np.isfinite(R).all() and _is_rotation(R) and np.abs(R @ a - [0.0, 0.0, 1.0]).max() <= 1e-12
        assert np.abs(R - pynbody_calc_faceon_matrix(L, [1.0, 0.0, 0.0])).max() <= 1e-15
    R = loader.orientation_matrix(_moments_with(L=(2.0, 0.0, 0.0), A=10.0), "faceon", "angmom", up=(7.0, 0.0, 0.0))
    assert _is_rotation(R) and np.abs(R @ [1.0, 0.0, 0.0] - [0.0, 0.0, 1.0]).max() <= 1e-12


def test_shape_method_finds_the_short_axis():
    """The second moments of a Gaussian of mass M with covariance Q diag(4, 3, 1/4) Q^T about a centre of mass at com are
    M (C + com com^T): the minor axis is Q's third column, whatever com."""
    from topsy_amd import loader
    rs = np.random.RandomState(5)
    for _ in range(20):
        Q, _r = np.linalg.qr(rs.normal(size=(3, 3)))
        C = Q @ np.diag([4.0, 3.0, 0.25]) @ Q.T
        com = rs.normal(size=3)
        M = 7.5
        T = M * (C + np.outer(com, com))
        mo = _moments_with(S=(T[0, 0], T[0, 1], T[0, 2], T[1, 1], T[1, 2], T[2, 2]), com=com, mass=M)
        a = loader.orientation_axis(mo, "shape")
        short = Q[:, 2]
        assert min(angle_between(a, short), angle_between(-a, short)) <= 1e-9
        # the sign rule: the largest-magnitude component is positive
        assert a[np.argmax(np.abs(a))] > 0 and abs(np.linalg.norm(a) - 1.0) <= 1e-12
        R = loader.orientation_matrix(mo, "faceon", "shape")
        assert _is_rotation(R) and np.abs(R @ a - [0.0, 0.0, 1.0]).max() <= 1e-12
    flat_z = _moments_with(S=(2.0, 0.0, 0.0, 3.0, 0.0, 0.5))
    assert np.array_equal(np.abs(loader.orientation_axis(flat_z, "shape")), [0.0, 0.0, 1.0])
    assert loader.orientation_axis(flat_z, "shape")[2] == 1.0


def test_no_axis_raises():
    from topsy_amd import loader
    with pytest.raises(ValueError, match="no net rotation"):
        loader.orientation_matrix(_moments_with(L=(0.0, 0.0, 0.0), A=5.0), "faceon", "angmom")
    with pytest.raises(ValueError, match="no net rotation"):
        loader.orientation_matrix(_moments_with(L=(3e-13, 0.0, 4e-13), A=1.0), "faceon", "angmom")
    loader.orientation_matrix(_moments_with(L=(3e-12, 0.0, 4e-12), A=1.0), "faceon", "angmom")
    with pytest.raises(ValueError, match="no net rotation"):       # no velocities: L = 0 and A = 0
        loader.orientation_matrix(_moments_with(L=(0.0, 0.0, 0.0), A=0.0), "faceon", "angmom")
    with pytest.raises(ValueError, match="minor axis"):             # prolate: the two smallest eigenvalues agree
        loader.orientation_matrix(_moments_with(S=(1.0, 0.0, 0.0, 1.0, 0.0, 4.0)), "faceon", "shape")
    with pytest.raises(ValueError, match="minor axis"):
        loader.orientation_matrix(_moments_with(S=(1.0, 0.0, 0.0, 1.0 + 5e-7, 0.0, 4.0)), "faceon", "shape")
    loader.orientation_matrix(_moments_with(S=(1.0, 0.0, 0.0, 1.0 + 1e-5, 0.0, 4.0)), "faceon", "shape")
    with pytest.raises(ValueError, match="minor axis"):             # a single point: every eigenvalue is 0
        loader.orientation_matrix(_moments_with(S=(0.0,) * 6), "sideon", "shape")
    with pytest.raises(ValueError, match="upside"):
        loader.orientation_matrix(_moments_with(), "upside", "angmom")
    with pytest.raises(ValueError, match="inertia"):
        loader.orientation_matrix(_moments_with(), "faceon", "inertia")


# ---- the loader, with a context stubbed by the reference ----------------------------------------------------------------------
class StubContext:
    """What ArrayDataLoader asks of a context for an orientation, answered by the reference."""

    def __init__(self):
        self.calls = []

    def sphere_moments(self, x, y, z, mass, vel=None, center=(0.0, 0.0, 0.0), r=1.0, r_vel=0.0):
        self.calls.append(dict(center=np.array(center), r=r, r_vel=r_vel, vel=vel is not None))
        return sphere_moments_reference(np.stack([x, y, z], axis=1), mass, None if vel is None else np.stack(vel, axis=1),
                                        center, r, r_vel)


def _no_context(monkeypatch):
    from topsy_amd import _native

    def refuse(*a, **k):
        raise AssertionError("a context was created before the arguments were checked")
    monkeypatch.setattr(_native, "Context", refuse)


def _loader(name="disc", **kwargs):
    from topsy_amd import loader
    pos, mass, vel, kw = scene(name)
    kwargs.setdefault("center", kw["center"])
    ld = loader.ArrayDataLoader(pos=pos, smooth=np.full(len(pos), 0.1, dtype=np.float32), mass=mass, vel=vel, **kwargs)
    stub = StubContext()
    ld.set_density_context(stub)
    return ld, stub


def test_loader_orients_once_and_caches(monkeypatch):
    from topsy_amd import loader
    _no_context(monkeypatch)
    ld, stub = _loader(orient="faceon", orient_radius=R_SPHERE)
    R = ld.get_initial_rotation()
    assert R is ld.get_initial_rotation() and len(stub.calls) == 1
    assert stub.calls[0]["r"] == R_SPHERE and stub.calls[0]["r_vel"] == 0.2 * R_SPHERE and stub.calls[0]["vel"]
    assert np.array_equal(stub.calls[0]["center"], AT)
    assert np.abs(R - loader.orientation_matrix(reference("disc"), "faceon", "angmom")).max() <= 1e-12
    assert np.degrees(angle_between(R.T @ [0.0, 0.0, 1.0], AXIS)) < 0.5 and _is_rotation(R)
    assert ld.orient_moments["n_inside"] == reference("disc")["n_inside"]
    # side-on, by the shape, without velocities
    ld, stub = _loader("no_vel", orient="sideon", orient_radius=R_SPHERE)
    R = ld.get_initial_rotation()
    assert len(stub.calls) == 1 and not stub.calls[0]["vel"] and stub.calls[0]["r_vel"] == 0.0
    up_screen = R.T @ [0.0, 1.0, 0.0]
    assert np.degrees(min(angle_between(up_screen, AXIS), angle_between(-up_screen, AXIS))) < 2.0
    # orient="none" and every other loader: the identity, nothing computed
    ld, stub = _loader()
    assert np.array_equal(ld.get_initial_rotation(), np.eye(3)) and not stub.calls
    assert np.array_equal(loader.TestDataLoader(n_particles=10).get_initial_rotation(), np.eye(3))
    # a rotation from the caller's cache: nothing is computed
    ld, stub = _loader(orient="faceon", orient_radius=R_SPHERE)
    ld.set_initial_rotation(R)
    assert np.array_equal(ld.get_initial_rotation(), R) and not stub.calls
    ld, stub = _loader()
    ld.set_initial_rotation(R.astype(np.float32))
    assert np.allclose(ld.get_initial_rotation(), R, atol=1e-7) and ld.get_initial_rotation().dtype == np.float64


def test_vel_is_permuted_with_the_cells(monkeypatch):
    from topsy_amd import loader
    _no_context(monkeypatch)
    pos, mass, vel, kw = scene("disc")
    tag = np.arange(len(pos), dtype=np.float32)
    ld = loader.ArrayDataLoader(pos=pos, smooth=np.ones(len(pos), dtype=np.float32), mass=mass, vel=vel, with_cells=True,
                                quantities={"tag": tag}, center=kw["center"], orient="faceon", orient_radius=R_SPHERE)
    order = ld.get_named_quantity("tag").astype(np.int64)
    assert not np.array_equal(order, np.arange(len(pos)))
    assert np.array_equal(ld.get_positions(), pos[order]) and np.array_equal(ld.get_velocities(), vel[order])
    assert ld.get_velocities().dtype == np.float32
    stub = StubContext()
    ld.set_density_context(stub)
    want = loader.orientation_matrix(sphere_moments_reference(pos[order], mass[order], vel[order], **kw), "faceon", "angmom")
    assert np.array_equal(ld.get_initial_rotation(), want)
    assert np.abs(want - loader.orientation_matrix(reference("disc"), "faceon", "angmom")).max() <= 1e-12


def test_loader_checks_its_orientation_arguments(monkeypatch):
    from topsy_amd import loader
    import topsy_amd
    _no_context(monkeypatch)
    pos, mass, vel, kw = scene("disc")
    h = np.ones(len(pos), dtype=np.float32)
    for make in (lambda **k: loader.ArrayDataLoader(pos=pos, smooth=h, mass=mass, **k), lambda **k: topsy_amd.from_arrays(pos, h, mass, **k)):
        with pytest.raises(ValueError, match="5 kpc"):
            make(vel=vel, orient="faceon")
        with pytest.raises(ValueError, match="orient_radius"):
            make(orient="sideon")
        for radius in (0.0, -1.0, np.nan, np.inf, "wide", True):
            with pytest.raises(ValueError, match="orient_radius"):
                make(vel=vel, orient="faceon", orient_radius=radius)
        with pytest.raises(ValueError, match="edgeon"):
            make(vel=vel, orient="edgeon", orient_radius=4.0)
        with pytest.raises(ValueError, match="inertia"):
            make(vel=vel, orient="faceon", orient_radius=4.0, orient_method="inertia")
        with pytest.raises(ValueError, match="angmom"):
            make(orient="faceon", orient_radius=4.0, orient_method="angmom")
        for bad in (vel[:-1], vel[:, :2], vel.ravel(), np.zeros((len(pos), 3, 1))):
            with pytest.raises(ValueError, match="vel"):
                make(vel=bad)
    ld = loader.ArrayDataLoader(pos=pos, smooth=h, mass=mass, vel=vel)
    for bad in (np.eye(3)[:2], np.eye(4), np.eye(3) * 1.001, np.array([[1.0, 1e-3, 0], [0, 1, 0], [0, 0, 1]]), np.full((3, 3), np.nan),
                "faceon"):
        with pytest.raises(ValueError):
            ld.set_initial_rotation(bad)
    ld.set_initial_rotation(np.eye(3) + 1e-8)
    with pytest.raises(ValueError, match="angmom"):
        loader.ArrayDataLoader(pos=pos, smooth=h, mass=mass).orientation("faceon", 4.0, method="angmom")


def test_python_entries_check_their_arguments_first(monkeypatch):
    import topsy_amd
    _no_context(monkeypatch)
    pos = np.zeros((10, 3), dtype=np.float32)
    mass = np.ones(10, dtype=np.float32)
    vel = np.ones((10, 3), dtype=np.float32)
    bad = [
        (dict(pos=np.zeros((10, 2)), mass=mass, radius=1.0), r"\(10, 2\)"),
        (dict(pos=pos, mass=np.ones(9), radius=1.0), r"\(9,\)"),
        (dict(pos=pos, mass=mass, vel=np.ones((10, 2)), radius=1.0), r"\(10, 2\)"),
        (dict(pos=pos, mass=mass, vel=np.ones(30), radius=1.0), r"\(30,\)"),
        (dict(pos=np.zeros((0, 3)), mass=np.ones(0), radius=1.0), "at least one"),
        (dict(pos=pos, mass=mass), "radius is required"),
        (dict(pos=pos, mass=mass, radius=0.0), "0.0"),
        (dict(pos=pos, mass=mass, radius=-2.0), "-2.0"),
        (dict(pos=pos, mass=mass, radius=np.nan), "nan"),
        (dict(pos=pos, mass=mass, radius=np.inf), "inf"),
        (dict(pos=pos, mass=mass, radius="wide"), "wide"),
        (dict(pos=pos, mass=mass, radius=1.0, center=(0.0, 1.0)), "center"),
        (dict(pos=pos, mass=mass, radius=1.0, center=(0.0, np.nan, 0.0)), "nan"),
        (dict(pos=pos, mass=mass, radius=1.0, vel_radius=0.5), "needs velocities"),
        (dict(pos=pos, mass=mass, vel=vel, radius=1.0, vel_radius=2.0), "exceed"),
        (dict(pos=pos, mass=mass, vel=vel, radius=1.0, vel_radius=0.0), "vel_radius"),
        (dict(pos=pos, mass=mass, vel=vel, radius=1.0, vel_radius=np.nan), "vel_radius"),
        (dict(pos=pos, mass=np.zeros(10), radius=1.0), "no particle"),
        (dict(pos=pos, mass=mass, vel=np.full((10, 3), np.inf), radius=1.0), "no particle"),
    ]
    for kwargs, match in bad:
        with pytest.raises(ValueError, match=match):
            topsy_amd.sphere_moments(**kwargs)
        with pytest.raises(ValueError, match=match):
            topsy_amd.orientation(**kwargs)
    with pytest.raises(ValueError, match="angmom"):
        topsy_amd.orientation(pos, mass, radius=1.0, method="angmom")
    with pytest.raises(ValueError, match="topdown"):
        topsy_amd.orientation(pos, mass, vel, radius=1.0, orient="topdown")


def test_binding_matches_the_header():
    import ctypes
    import os
    import re
    from topsy_amd import _native, multigpu
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "topsy_splat.h")).read()
    assert " * 115: new entry point tsp_sphere_moments" in text
    struct = re.search(r"typedef struct \{([^}]*)\} tsp_moments;", text).group(1)
    fields = re.findall(r"\b(int64_t|double)\s+([^;]*);", re.sub(r"/\*.*?\*/", "", struct))
    declared = [(t, name.strip()) for t, names in fields for name in names.split(",")]
    assert declared == [("int64_t", "n_valid"), ("int64_t", "n_inside"), ("int64_t", "n_inside_vel"), ("double", "mass"),
                        ("double", "mass_vel"), ("double", "com[3]"), ("double", "v_cen[3]"), ("double", "L[3]"), ("double", "S[6]"),
                        ("double", "A")]
    assert [name for name, _ in _native.Moments._fields_] == [name.split("[")[0] for _, name in declared]
    assert ctypes.sizeof(_native.Moments) == 8 * (3 + 2 + 3 + 3 + 3 + 6 + 1)
    restype, argtypes = _native.SIGNATURES["tsp_sphere_moments"]
    assert restype is ctypes.c_int and len(argtypes) == 13
    assert _native.load_library().tsp_version() >= 115
    assert hasattr(_native.Context, "sphere_moments") and hasattr(multigpu.MultiGpuContext, "sphere_moments")
    contract = text[text.index("/* The moments of the particles inside a sphere"):text.index("} tsp_moments;")]
    assert "Not provided:" in contract and "periodic wrapping of the displacements" in contract.replace("\n *", "")
