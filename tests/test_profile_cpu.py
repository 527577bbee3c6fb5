"""Radial profiles on the CPU: radial_profile_reference, the NumPy float64 restatement of the contract of tsp_radial_profile
(include/topsy_splat.h) that test_gpu_profile.py holds the GPU to; the scenes both files use, with the property of the inputs that
the GPU comparison relies on (no particle within a relative 1e-9 of a bin edge or of the disc's half height) established here by
the reference alone; Profile's arithmetic from hand-made sums; the edge builders; every argument error; and virial_radius's
bracketing rule run on the reference against the brute-force crossing of the sorted radii.  None of it needs a GPU."""
import functools

import numpy as np
import pytest

from test_orient_cpu import AT, AXIS, BOOST, LATTICE_AT, LATTICE_BOOST, lattice_scene
from test_orient_cpu import scene as orient_scene

R_MAX, R_MIN, HALF_HEIGHT = 4.0, 0.05, 0.2
BIN_COUNTS = (1, 8, 512)
TABLE_BIN_COUNTS = (103, 104)       # the last bin count with a table per wave and the first with one per workgroup (tsp_profile.hip)
GEOMETRIES = (0, 1)
MASS, MS, MC, MC2, MJ = 0, 1, slice(2, 5), slice(5, 8), slice(8, 11)


def radial_profile_reference(pos, mass, vel=None, edges=(0.0, 1.0), geometry=0, center=(0.0, 0.0, 0.0), v_cen=(0.0, 0.0, 0.0),
                             frame=None, half_height=np.inf):
    """The contract in float64, every expression in the header's order (no fused multiply-adds; each sum starts at +0.0 and runs in
    index order).  Returns count int64 (n_bins,), sums float64 (n_bins, 11), n_valid, n_inner, n_binned, mass_inner and, for the
    tolerances of the GPU comparison, "scale" (n_bins, 11): the sum of the magnitudes of each sum's terms."""
    pos = np.asarray(pos, dtype=np.float32)
    mass = np.asarray(mass, dtype=np.float32)
    edges = np.asarray(edges, dtype=np.float64)
    n_bins = len(edges) - 1
    c = np.asarray(center, dtype=np.float64)
    F = (np.eye(3) if frame is None else np.asarray(frame, dtype=np.float64)).ravel()
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        valid = np.isfinite(pos).all(axis=1) & np.isfinite(mass) & (mass > 0)
        if vel is not None:
            vel = np.asarray(vel, dtype=np.float32)
            valid &= np.isfinite(vel).all(axis=1)
        if not valid.any():
            raise ValueError("no valid particle")
        dx, dy, dz = (pos[:, k].astype(np.float64) - c[k] for k in range(3))
        xp = (F[0] * dx + F[1] * dy) + F[2] * dz
        yp = (F[3] * dx + F[4] * dy) + F[5] * dz
        zp = (F[6] * dx + F[7] * dy) + F[8] * dz
        R2 = xp * xp + yp * yp
        if geometry == 0:
            s2 = (dx * dx + dy * dy) + dz * dz
            takes_part = valid
        else:
            s2 = R2
            takes_part = valid & (np.abs(zp) <= half_height)
        E2 = edges * edges
        row = np.searchsorted(E2, s2, side="right")         # the number of squared edges <= s2
        row[~takes_part | np.isnan(s2)] = n_bins + 1
        m = mass.astype(np.float64)
        terms = np.zeros((len(pos), 11))
        terms[:, 0] = m
        terms[:, 1] = m * np.sqrt(s2)
        if vel is not None:
            o = np.asarray(v_cen, dtype=np.float64)
            ux, uy, uz = (vel[:, k].astype(np.float64) - o[k] for k in range(3))
            upx = (F[0] * ux + F[1] * uy) + F[2] * uz
            upy = (F[3] * ux + F[4] * uy) + F[5] * uz
            upz = (F[6] * ux + F[7] * uy) + F[8] * uz
            R = np.sqrt(R2)
            eRx = np.where(R > 0, xp / R, 1.0)
            eRy = np.where(R > 0, yp / R, 0.0)
            c1 = eRx * upy - eRy * upx
            if geometry == 0:
                D = np.sqrt(R2 + zp * zp)
                erx = np.where(D > 0, xp / D, 0.0)
                ery = np.where(D > 0, yp / D, 0.0)
                erz = np.where(D > 0, zp / D, 1.0)
                c0 = (erx * upx + ery * upy) + erz * upz
                c2 = ((eRx * erz) * upx + (eRy * erz) * upy) - (eRx * erx + eRy * ery) * upz
            else:
                c0 = eRx * upx + eRy * upy
                c2 = upz
            for k, comp in enumerate((c0, c1, c2)):
                terms[:, 2 + k] = m * comp
                terms[:, 5 + k] = (m * comp) * comp
            terms[:, 8] = m * (dy * uz - dz * uy)
            terms[:, 9] = m * (dz * ux - dx * uz)
            terms[:, 10] = m * (dx * uy - dy * ux)
    member = row <= n_bins
    rows, terms = row[member], terms[member]
    count = np.bincount(rows, minlength=n_bins + 1).astype(np.int64)
    sums = np.stack([np.bincount(rows, weights=terms[:, j], minlength=n_bins + 1) for j in range(11)], axis=1)
    scale = np.stack([np.bincount(rows, weights=np.abs(terms[:, j]), minlength=n_bins + 1) for j in range(11)], axis=1)
    return {"count": count[1:], "sums": sums[1:], "scale": scale[1:], "n_valid": int(valid.sum()), "n_inner": int(count[0]),
            "n_binned": int(count[1:].sum()), "mass_inner": float(sums[0, 0])}


def near_edge_margin(pos, spec):
    """min | s2 / E2[k] - 1 | over the particles with finite coordinates and the edges > 0 and, in a disc of finite half height,
    min | |z'| / half_height - 1 |: how far the inputs are from a membership that a rounding difference could flip."""
    pos = np.asarray(pos, dtype=np.float32)
    d = pos[np.isfinite(pos).all(axis=1)].astype(np.float64) - np.asarray(spec["center"], dtype=np.float64)
    F = np.eye(3) if spec.get("frame") is None else np.asarray(spec["frame"], dtype=np.float64)
    dp = d @ F.T
    s2 = (d * d).sum(axis=1) if spec["geometry"] == 0 else dp[:, 0] ** 2 + dp[:, 1] ** 2
    E2 = np.asarray(spec["edges"], dtype=np.float64) ** 2
    E2 = E2[E2 > 0]
    s2 = np.sort(s2)
    at = np.clip(np.searchsorted(s2, E2), 1, len(s2) - 1)
    margin = float(np.minimum(np.abs(s2[at] / E2 - 1.0), np.abs(s2[at - 1] / E2 - 1.0)).min())
    hh = spec.get("half_height", np.inf)
    if spec["geometry"] == 1 and np.isfinite(hh):
        margin = min(margin, float(np.abs(np.abs(dp[:, 2]) / hh - 1.0).min()))
    return margin


def profile_blocks_read(pos, valid, spec, block=1024):
    """How many blocks of `block` consecutive particles the pass reads: those whose valid members' float32 bounding box lies at a
    squared distance (formed like d2) below E2[n_bins] (shells) or (E2[n_bins] + half_height^2) * (1 + 1e-5) (annuli of finite
    height); with an infinite height every block with a valid member."""
    c = np.asarray(spec["center"], dtype=np.float64)
    e = float(spec["edges"][-1])
    hh = spec.get("half_height", np.inf)
    limit = e * e if spec["geometry"] == 0 else (e * e + hh * hh) * (1.0 + 1e-5)
    count = 0
    for start in range(0, len(pos), block):
        p = pos[start:start + block][valid[start:start + block]].astype(np.float64)
        if len(p) == 0:
            continue
        g = np.maximum(np.maximum(p.min(axis=0) - c, c - p.max(axis=0)), 0.0)
        count += bool((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2] < limit)
    return count


# ---- scenes ---------------------------------------------------------------------------------------------------------------
def faceon_frame():
    from topsy_amd import loader
    return loader.orientation_matrix({"L": AXIS, "A": 1.0}, "faceon", "angmom")


OFFSET_AT = np.array([1.0e4, -1.0e4, 1.0e4]) + np.array([0.00137, -0.00211, 0.00309])
OFFSET_R_MAX = 0.03


@functools.lru_cache(maxsize=None)
def scene(name):
    """(pos float32 (n, 3), mass float32 (n,), vel float32 (n, 3) or None, dict(center, v_cen, frame, r_min, r_max, half_height)):
    the rotating exponential disc of test_orient_cpu.py in its hot halo, at AT, moving with BOOST, profiled in the frame that
    shows it face-on -- shuffled ("disc"), sorted along x ("disc_sorted"), with NaN / inf / non-positive-mass rows ("invalid"),
    without velocities ("no_vel") -- and "offset": structure of size 1e-2 at 1e4 from the origin, where the spacing of float32 is
    1e-3: displacements formed in float32, or after a multiplication, would be wrong by a tenth of the structure."""
    base = dict(center=tuple(AT), v_cen=tuple(BOOST), frame=faceon_frame(), r_min=R_MIN, r_max=R_MAX, half_height=HALF_HEIGHT)
    if name == "offset":
        rs = np.random.RandomState(31)
        n = 7000
        d = rs.normal(scale=1e-2, size=(n, 3))
        pos = (d + OFFSET_AT).astype(np.float32)
        vel = (np.cross([0.0, 0.0, 3.0], d) / 1e-2 + rs.normal(scale=0.2, size=(n, 3))).astype(np.float32)
        mass = rs.uniform(0.5, 1.5, size=n).astype(np.float32)
        base = dict(center=tuple(OFFSET_AT), v_cen=(0.0, 0.0, 0.0), frame=None, r_min=1e-3, r_max=OFFSET_R_MAX, half_height=8e-3)
    else:
        pos, mass, vel, _ = orient_scene(name)
    return pos, mass, vel, base


SCENES = ("disc", "disc_sorted", "invalid", "no_vel", "offset")


def spec_of(name, geometry, n_bins):
    """The keyword arguments of radial_profile_reference / Context.radial_profile besides the arrays: n_bins linear bins between
    the scene's r_min and r_max."""
    from topsy_amd import loader
    _, _, vel, base = scene(name)
    spec = dict(edges=loader.profile_edges("lin", n_bins, base["r_min"], base["r_max"]), geometry=geometry, center=base["center"],
                frame=base["frame"], half_height=base["half_height"] if geometry == 1 else np.inf)
    if vel is not None:
        spec["v_cen"] = base["v_cen"]
    return spec


@functools.lru_cache(maxsize=None)
def reference(name, geometry, n_bins):
    pos, mass, vel, _ = scene(name)
    return radial_profile_reference(pos, mass, vel, **spec_of(name, geometry, n_bins))


LATTICE_EDGES = np.array([0.0, 0.5, 1.0, 1.05, 2.0, 2.05, 3.0, 3.05, 4.0, 4.05, 5.0, 5.05, 6.0, 6.05, 7.0, 9.0])
LATTICE_THIN = np.arange(2, 14, 2)              # the bins [k, k + 0.05), k = 1 .. 6: their members have s2 = k * k exactly
LATTICE_FRAME = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])       # x' = y, y' = z, z' = x: exact
LATTICE_OMEGA = 2.0


def lattice_profile_scene(order="shuffled", rotation="spin"):
    """The integer lattice {-6..6}^3 about LATTICE_AT with the integer masses 1, 2, 3 and integer velocities: every product and
    sum of the contract that involves no square root or division is an integer far below 2^53, so exact in any order.  The edges
    1 .. 7 pass exactly through lattice radii ((3, 4, 0) has s = 5): such a particle belongs to the bin that starts there.  The
    bins [k, k + 0.05) hold the radius k alone.  (0, 0, z') is on the axis and (0, 0, 0) at the centre: the fallback triads.
    rotation "spin": the velocities of test_orient_cpu.py's lattice; "solid": LATTICE_OMEGA e x d + LATTICE_BOOST with e the
    third axis of LATTICE_FRAME, a solid-body rotation about the disc's axis."""
    pos, _, vel, _ = lattice_scene(order)
    d = pos.astype(np.float64) - LATTICE_AT
    mass = (1.0 + (np.abs(d).sum(axis=1) % 3)).astype(np.float32)
    if rotation == "solid":
        vel = (np.cross(LATTICE_OMEGA * LATTICE_FRAME[2], d) + LATTICE_BOOST).astype(np.float32)
    spec = dict(edges=LATTICE_EDGES, center=tuple(LATTICE_AT), v_cen=tuple(LATTICE_BOOST), frame=LATTICE_FRAME)
    return pos, mass, vel, spec


# ---- the reference and the inputs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_scenes_have_no_near_edges(name):
    pos, mass, vel, base = scene(name)
    assert 6500 <= len(pos) <= 7168 and -(-len(pos) // 1024) == 7 and len(pos) % 1024 != 0
    for geometry in GEOMETRIES:
        for n_bins in BIN_COUNTS + (TABLE_BIN_COUNTS if name == "disc" else ()):
            spec = spec_of(name, geometry, n_bins)
            margin = near_edge_margin(pos, spec)
            ref = reference(name, geometry, n_bins)
            print(f"{name} geometry {geometry} bins {n_bins}: valid {ref['n_valid']}, inner {ref['n_inner']}, binned {ref['n_binned']}, "
                  f"fullest bin {ref['count'].max()}, empty bins {(ref['count'] == 0).sum()}, nearest edge {margin:.3g}")
            assert margin > 1e-9
            assert ref["n_binned"] > 1000 and ref["n_inner"] > 0 and ref["n_binned"] + ref["n_inner"] < ref["n_valid"]


def test_scene_properties():
    """What each scene is for, shown by the reference."""
    from topsy_amd import loader
    pos, mass, vel, base = scene("disc")
    sphere, disc = reference("disc", 0, 8), reference("disc", 1, 8)
    # the disc rotates about the frame's third axis at speed 1: a flat rotation curve, little radial or vertical motion
    p = loader.Profile(spec_of("disc", 1, 8)["edges"], disc["count"], disc["sums"], disc, "disc")
    assert np.abs(p.v_phi[1:6] - 1.0).max() < 0.1 and np.abs(p.v_R[:6]).max() < 0.05 and np.abs(p.v_z[:6]).max() < 0.05
    assert np.abs(p.sigma_phi[:6] - 0.1).max() < 0.03
    # j points along the disc's axis in the caller's frame
    j = p.j[2]
    assert np.dot(j, AXIS) / np.linalg.norm(j) > 0.999
    # the shells hold the halo too, the thin disc does not: fewer members, and membership in shells ignores the frame
    assert disc["n_binned"] < sphere["n_binned"]
    turned = radial_profile_reference(pos, mass, vel, **{**spec_of("disc", 0, 8), "frame": None})
    assert np.array_equal(turned["count"], sphere["count"]) and np.array_equal(turned["sums"][:, :2], sphere["sums"][:, :2])
    assert np.array_equal(turned["sums"][:, MJ], sphere["sums"][:, MJ])
    assert not np.allclose(turned["sums"][:, MC], sphere["sums"][:, MC], rtol=1e-3, atol=0)
    # sorted: the same sums up to their order; sorted along x the outer blocks lie outside the profile
    srt = reference("disc_sorted", 0, 8)
    assert np.array_equal(srt["count"], sphere["count"])
    assert np.abs(srt["sums"] - sphere["sums"]).max() <= 1e-11 * sphere["scale"].max()
    everyone = np.ones(len(pos), dtype=bool)
    small = {**spec_of("disc", 0, 8), "edges": np.array([0.0, 0.4, 0.8])}
    assert profile_blocks_read(scene("disc_sorted")[0], everyone, small) < 7 == profile_blocks_read(pos, everyone, small)
    thin = {**spec_of("disc", 1, 8), "edges": np.array([0.0, 0.4, 0.8])}
    assert profile_blocks_read(scene("disc_sorted")[0], everyone, thin) < 7 == profile_blocks_read(pos, everyone, thin)
    assert profile_blocks_read(scene("disc_sorted")[0], everyone, {**thin, "half_height": np.inf}) == 7
    # invalid rows take no part
    inv = reference("invalid", 0, 8)
    ipos, imass, ivel, _ = scene("invalid")
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(ipos).all(axis=1) & np.isfinite(ivel).all(axis=1) & np.isfinite(imass) & (imass > 0)
    assert inv["n_valid"] == int(ok.sum()) < len(ipos) - 300 and np.isfinite(inv["sums"]).all()
    assert inv["n_binned"] < sphere["n_binned"]
    # no velocities: the nine velocity sums are +0.0, the others those of the disc
    nov = reference("no_vel", 0, 8)
    assert not nov["sums"][:, 2:].any() and not np.signbit(nov["sums"]).any()
    assert np.array_equal(nov["sums"][:, :2], sphere["sums"][:, :2]) and np.array_equal(nov["count"], sphere["count"])
    # offset: displacements rounded to float32 (or a float32 centre) would move the bins' masses far beyond the tolerance
    opos, omass, ovel, obase = scene("offset")
    off = reference("offset", 0, 8)
    coarse = radial_profile_reference(opos, omass, ovel, **{**spec_of("offset", 0, 8),
                                                             "center": tuple(np.float32(OFFSET_AT).astype(np.float64))})
    assert np.abs(coarse["sums"][:, MASS] - off["sums"][:, MASS]).max() > 1e-3 * off["sums"][:, MASS].max()
    assert np.spacing(np.float32(1e4)) > 0.03 * OFFSET_R_MAX


def test_lattice_reference_is_exact():
    for order in ("shuffled", "sorted"):
        pos, mass, vel, spec = lattice_profile_scene(order)
        d = pos.astype(np.float64) - LATTICE_AT
        dp = d @ LATTICE_FRAME.T
        for geometry, s2, part in ((0, (d * d).sum(axis=1), np.ones(len(d), dtype=bool)),
                                   (1, dp[:, 0] ** 2 + dp[:, 1] ** 2, np.abs(dp[:, 2]) <= 2.0)):
            ref = radial_profile_reference(pos, mass, vel, geometry=geometry, half_height=2.0 if geometry else np.inf, **spec)
            E2 = LATTICE_EDGES ** 2
            for k in range(len(LATTICE_EDGES) - 1):
                inside = part & (s2 >= E2[k]) & (s2 < E2[k + 1])
                assert ref["count"][k] == inside.sum() and ref["sums"][k, MASS] == mass[inside].astype(np.float64).sum()
                assert np.array_equal(ref["sums"][k, MJ], (mass[inside, None] * np.cross(d[inside], vel[inside] - LATTICE_BOOST)).sum(axis=0))
            # a particle exactly on an edge is in the bin that starts there; on the half height it takes part
            on_edge = part & (s2 == 25.0)
            assert on_edge.sum() > 0 and ref["count"][10] == on_edge.sum()
            for k in LATTICE_THIN:
                radius = LATTICE_EDGES[k]
                assert ref["count"][k] > 0 and ref["sums"][k, MS] == radius * ref["sums"][k, MASS]
            if geometry == 1:
                assert (np.abs(dp[part, 2]) == 2.0).any()
                assert ref["n_binned"] == part.sum()          # the last edge, 9, is beyond the lattice's corner in the plane
            assert ref["n_inner"] == 0 and ref["count"][0] == (1 if geometry == 0 else 5)


def test_fallback_triads_on_the_axis_and_at_the_centre():
    """One particle each: at the centre (e_r = z', e_phi = y', e_theta = x'), on the axis above and below (e_R = x', e_phi = y',
    e_r = +-z', e_theta = +-x') and off the axis, against the triads written out."""
    F = LATTICE_FRAME
    u = np.array([3.0, -5.0, 7.0])          # u' = F u = (-5, 7, 3)
    up = F @ u
    cases = [((0.0, 0.0, 0.0), 0, (up[2], up[1], up[0])), ((0.0, 0.0, 0.0), 1, (up[0], up[1], up[2])),
             ((0.0, 0.0, 2.0), 0, (up[2], up[1], up[0])), ((0.0, 0.0, -2.0), 0, (-up[2], up[1], -up[0])),
             ((0.0, 0.0, 2.0), 1, (up[0], up[1], up[2])),
             ((3.0, 0.0, 0.0), 0, (up[0], up[1], -up[2])), ((0.0, 3.0, 0.0), 1, (up[1], -up[0], up[2]))]
    for dprime, geometry, want in cases:
        d = F.T @ np.array(dprime)
        ref = radial_profile_reference([d], [2.0], [u], edges=(0.0, 10.0), geometry=geometry, frame=F)
        assert ref["count"][0] == 1 and np.array_equal(ref["sums"][0, MC], 2.0 * np.array(want)), (dprime, geometry)
        assert np.array_equal(ref["sums"][0, MC2], 2.0 * np.array(want) ** 2)
    # a general point: the spherical triad is orthonormal and right-handed (e_r x e_phi = -e_theta ... e_theta = e_phi x e_r)
    rs = np.random.RandomState(2)
    for _ in range(20):
        d, u = rs.normal(size=3), rs.normal(size=3)
        r = np.linalg.norm(d)
        e_r = d / r
        e_phi = np.array([-d[1], d[0], 0.0]) / np.hypot(d[0], d[1])
        e_theta = np.cross(e_phi, e_r)
        ref = radial_profile_reference([d.astype(np.float32)], [1.0], [u.astype(np.float32)], edges=(0.0, 10.0))
        d32, u32 = d.astype(np.float32).astype(np.float64), u.astype(np.float32).astype(np.float64)
        assert np.abs(ref["sums"][0, MC] - [u32 @ e_r, u32 @ e_phi, u32 @ e_theta]).max() < 1e-6
        assert abs(ref["sums"][0, MC2].sum() - u32 @ u32) < 1e-12 * (u32 @ u32) + 1e-12
        assert np.abs(ref["sums"][0, MJ] - np.cross(d32, u32)).max() < 1e-12


# ---- Profile ----------------------------------------------------------------------------------------------------------------
def _sums(n_bins, **columns):
    sums = np.zeros((n_bins, 11))
    for name, values in columns.items():
        sums[:, {"mass": 0, "ms": 1, "mc0": 2, "mc1": 3, "mc2": 4, "mcc0": 5, "mcc1": 6, "mcc2": 7}[name]] = values
    return sums


def test_profile_of_a_uniform_sphere_is_flat():
    from topsy_amd import loader
    edges = loader.profile_edges("log", 12, 0.5, 40.0)
    rho = 2.5
    shell = 4.0 / 3.0 * np.pi * (edges[1:] ** 3 - edges[:-1] ** 3)
    inner = rho * 4.0 / 3.0 * np.pi * edges[0] ** 3
    p = loader.Profile(edges, np.full(12, 10), _sums(12, mass=rho * shell, ms=rho * shell * 0.5 * (edges[1:] + edges[:-1])),
                       {"mass_inner": inner, "n_inner": 3, "n_valid": 123, "n_binned": 120}, "sphere", G=4.3e-6, with_velocities=False)
    assert np.abs(p.density / rho - 1.0).max() <= 4e-16 and len(p) == 12
    assert np.array_equal(p.rbins, 0.5 * (edges[1:] + edges[:-1])) and np.abs(p.r_mean / p.rbins - 1.0).max() <= 4e-16
    # mass_enc is at the outer edges and includes what lies inside edges[0]
    assert np.abs(p.mass_enc / (rho * 4.0 / 3.0 * np.pi * edges[1:] ** 3) - 1.0).max() <= 1e-14
    assert p.mass_enc[0] == inner + p.mass[0]
    assert np.abs(p.v_circ / np.sqrt(4.3e-6 * rho * 4.0 / 3.0 * np.pi * edges[1:] ** 2) - 1.0).max() <= 1e-14
    assert p.v_r is None and p.sigma_theta is None and p.j is None and p.info["n_inner"] == 3
    assert loader.Profile(edges, np.full(12, 10), _sums(12, mass=1.0), {}, "sphere").v_circ is None
    # a disc: surface density
    q = loader.Profile(edges, np.full(12, 10), _sums(12, mass=rho * np.pi * (edges[1:] ** 2 - edges[:-1] ** 2)), {}, "disc")
    assert np.abs(q.density / rho - 1.0).max() <= 4e-16 and q.mass_enc[0] == q.mass[0]
    assert hasattr(q, "v_R") and hasattr(q, "sigma_z") and not hasattr(q, "v_r")
    import topsy_amd
    assert topsy_amd.Profile is loader.Profile


def test_profile_means_dispersions_and_empty_bins():
    from topsy_amd import loader
    mass = np.array([2.0, 0.0, 4.0])
    sums = _sums(3, mass=mass, ms=[3.0, 0.0, 10.0], mc1=[6.0, 0.0, -8.0], mcc1=[20.0, 0.0, 16.0], mc0=[2.0, 0.0, 0.0],
                 mcc0=[1.9999999, 0.0, 4.0])
    sums[:, 8:11] = [[2.0, 4.0, 6.0], [0.0, 0.0, 0.0], [4.0, 0.0, -4.0]]
    p = loader.Profile([0.0, 1.0, 2.0, 3.0], [2, 0, 3], sums, {"mass_inner": 0.0}, "sphere")
    assert np.array_equal(p.v_phi[[0, 2]], [3.0, -2.0]) and np.array_equal(p.sigma_phi[[0, 2]], [1.0, 0.0])
    # a variance below zero by rounding is a dispersion of 0, not NaN
    assert p.v_r[0] == 1.0 and p.sigma_r[0] == 0.0 and p.sigma_r[2] == 1.0
    assert np.array_equal(p.j[[0, 2]], [[1.0, 2.0, 3.0], [1.0, 0.0, -1.0]]) and np.array_equal(p.r_mean[[0, 2]], [1.5, 2.5])
    # the empty bin: zero mass and density, NaN means
    assert p.mass[1] == 0.0 and p.density[1] == 0.0 and p.n[1] == 0
    for a in (p.r_mean, p.v_r, p.v_phi, p.v_theta, p.sigma_r, p.sigma_phi, p.sigma_theta, p.j[:, 0], p.j[:, 2]):
        assert np.isnan(a[1]) and np.isfinite(a[[0, 2]]).all()
    assert np.array_equal(p.mass_enc, [2.0, 2.0, 6.0])
    with pytest.raises(ValueError, match="ring"):
        loader.Profile([0.0, 1.0], [1], _sums(1), {}, "ring")
    with pytest.raises(ValueError, match="sums"):
        loader.Profile([0.0, 1.0, 2.0], [1], _sums(2), {}, "sphere")


def test_solid_body_rotation_on_the_lattice():
    """In the annuli that hold one integer radius R the components of Omega e x d along e_phi are Omega * R exactly (x' / R and
    y' / R are rounded, but their products with the integer velocities sum to the integer Omega * R within half an ulp), so
    v_phi = Omega * R and sigma_phi = 0 exactly; v_R = v_z = 0."""
    from topsy_amd import loader
    pos, mass, vel, spec = lattice_profile_scene("shuffled", "solid")
    ref = radial_profile_reference(pos, mass, vel, geometry=1, half_height=2.0, **spec)
    p = loader.Profile(spec["edges"], ref["count"], ref["sums"], ref, "disc")
    for k in LATTICE_THIN:
        radius = LATTICE_EDGES[k]
        assert p.n[k] >= 4 * 5 and p.v_phi[k] == LATTICE_OMEGA * radius and p.sigma_phi[k] == 0.0, k
        assert p.v_R[k] == 0.0 and p.v_z[k] == 0.0 and p.sigma_z[k] == 0.0 and p.r_mean[k] == radius
    # everywhere else to rounding
    full = (p.n > 0) & (p.r_mean > 0)
    assert np.abs(p.v_phi[full] / (LATTICE_OMEGA * p.r_mean[full]) - 1.0).max() < 0.05
    assert np.array_equal(p.j[full] @ LATTICE_FRAME[0], np.zeros(full.sum()))


# ---- the edges and the arguments ----------------------------------------------------------------------------------------------
def test_edge_builders():
    from topsy_amd import loader
    lin = loader.profile_edges("lin", 8, 0.0, 4.0)
    assert lin.dtype == np.float64 and np.array_equal(lin, np.arange(9) * 0.5)
    log = loader.profile_edges("log", 4, 1.0, 16.0)
    assert np.array_equal(log, [1.0, 2.0, 4.0, 8.0, 16.0])
    for bins, r_min, r_max, n in (("lin", 0.05, 4.0, 512), ("log", 0.3, 7.7, 512), ("log", 1e-3, 1e3, 100), ("lin", 0.1, 0.7, 1)):
        e = loader.profile_edges(bins, n, r_min, r_max)
        assert e.shape == (n + 1,) and e[0] == r_min and e[-1] == r_max and (np.diff(e) > 0).all()
        steps = np.diff(np.log(e)) if bins == "log" else np.diff(e)
        assert np.abs(steps / steps.mean() - 1.0).max() < 1e-9
    own = loader.profile_edges([0.5, 1.0, 3.0])
    assert own.dtype == np.float64 and np.array_equal(own, [0.5, 1.0, 3.0])
    given = np.array([1.0, 2.0])
    assert loader.profile_edges(given) is not given
    bad = [(dict(bins="cubic", r_max=1.0), "cubic"), (dict(r_max=None), "r_max is required"), (dict(r_max=0.0), "r_max"),
           (dict(r_max=np.inf), "r_max"), (dict(r_max="far"), "r_max"), (dict(r_max=1.0, r_min=1.0), "r_min"),
           (dict(r_max=1.0, r_min=-0.1), "r_min"), (dict(r_max=1.0, r_min=np.nan), "r_min"), (dict(r_max=1.0, r_min="0"), "r_min"),
           (dict(r_max=1.0, bins="log"), "r_min > 0"), (dict(r_max=1.0, n_bins=0), "n_bins"), (dict(r_max=1.0, n_bins=513), "n_bins"),
           (dict(r_max=1.0, n_bins=2.5), "n_bins"), (dict(r_max=1.0, n_bins=True), "n_bins"),
           (dict(r_max=1.0 + 1e-15, r_min=1.0, n_bins=100), "not distinct"),
           (dict(bins=[1.0]), "2 to 513"), (dict(bins=np.arange(515.0)), "2 to 513"), (dict(bins=[[0.0, 1.0]]), "2 to 513"),
           (dict(bins=[0.0, 1.0, 1.0]), "ascending"), (dict(bins=[0.0, 2.0, 1.0]), "ascending"), (dict(bins=[-1.0, 1.0]), "ascending"),
           (dict(bins=[0.0, np.nan]), "ascending"), (dict(bins=[0.0, np.inf]), "ascending"), (dict(bins=["a", "b"]), "bins must be")]
    for kwargs, match in bad:
        with pytest.raises(ValueError, match=match):
            loader.profile_edges(**kwargs)


def _no_context(monkeypatch):
    from topsy_amd import _native

    def refuse(*a, **k):
        raise AssertionError("a context was created before the arguments were checked")
    monkeypatch.setattr(_native, "Context", refuse)


def test_python_entries_check_their_arguments_first(monkeypatch):
    import topsy_amd
    from topsy_amd import loader
    _no_context(monkeypatch)
    pos = np.zeros((10, 3), dtype=np.float32)
    mass = np.ones(10, dtype=np.float32)
    vel = np.ones((10, 3), dtype=np.float32)
    bad = [
        (dict(pos=np.zeros((10, 2)), mass=mass, r_max=1.0), r"\(10, 2\)"),
        (dict(pos=pos, mass=np.ones(9), r_max=1.0), r"\(9,\)"),
        (dict(pos=pos, mass=mass, vel=np.ones((10, 2)), r_max=1.0), r"\(10, 2\)"),
        (dict(pos=np.zeros((0, 3)), mass=np.ones(0), r_max=1.0), "at least one"),
        (dict(pos=pos, mass=np.zeros(10), r_max=1.0), "no particle"),
        (dict(pos=pos, mass=mass), "r_max is required"),
        (dict(pos=pos, mass=mass, r_max=-2.0), "-2.0"),
        (dict(pos=pos, mass=mass, r_max=1.0, bins="log"), "r_min > 0"),
        (dict(pos=pos, mass=mass, r_max=1.0, n_bins=600), "600"),
        (dict(pos=pos, mass=mass, bins=[2.0, 1.0]), "ascending"),
        (dict(pos=pos, mass=mass, r_max=1.0, center=(0.0, 1.0)), "center"),
        (dict(pos=pos, mass=mass, r_max=1.0, center=(0.0, np.nan, 0.0)), "nan"),
        (dict(pos=pos, mass=mass, r_max=1.0, geometry="ring"), "ring"),
        (dict(pos=pos, mass=mass, r_max=1.0, geometry=1), "geometry"),
        (dict(pos=pos, mass=mass, r_max=1.0, frame=np.eye(4)), r"\(4, 4\)"),
        (dict(pos=pos, mass=mass, r_max=1.0, frame=np.eye(3) * 1.01), "orthonormal"),
        (dict(pos=pos, mass=mass, r_max=1.0, half_height=0.1), "needs geometry='disc'"),
        (dict(pos=pos, mass=mass, r_max=1.0, geometry="disc", half_height=0.0), "half_height"),
        (dict(pos=pos, mass=mass, r_max=1.0, geometry="disc", half_height=-1.0), "half_height"),
        (dict(pos=pos, mass=mass, r_max=1.0, geometry="disc", half_height=np.nan), "half_height"),
        (dict(pos=pos, mass=mass, r_max=1.0, geometry="disc", half_height="thin"), "half_height"),
        (dict(pos=pos, mass=mass, r_max=1.0, v_cen=(0.0, 0.0, 0.0)), "needs velocities"),
        (dict(pos=pos, mass=mass, vel=vel, r_max=1.0, v_cen=(0.0, 0.0)), "v_cen"),
        (dict(pos=pos, mass=mass, vel=vel, r_max=1.0, v_cen=(0.0, np.inf, 0.0)), "v_cen"),
        (dict(pos=pos, mass=mass, r_max=1.0, G=0.0), "G"),
        (dict(pos=pos, mass=mass, r_max=1.0, G=np.nan), "G"),
    ]
    for kwargs, match in bad:
        with pytest.raises(ValueError, match=match):
            topsy_amd.radial_profile(**kwargs)
    ld = loader.ArrayDataLoader(pos=pos, smooth=np.ones(10, dtype=np.float32), mass=mass, vel=vel)
    for kwargs, match in ((dict(), "r_max is required"), (dict(r_max=1.0, geometry="ring"), "ring"),
                          (dict(r_max=1.0, half_height=1.0), "disc"), (dict(r_max=1.0, center=(1.0,)), "center")):
        with pytest.raises(ValueError, match=match):
            ld.profile(**kwargs)
    good = dict(pos=pos, mass=mass, center=(0.0, 0.0, 0.0), rho_threshold=1.0, r_max=1.0)
    for change, match in ((dict(pos=np.zeros((10, 2))), r"\(10, 2\)"), (dict(mass=np.ones(9)), r"\(9,\)"), (dict(mass=np.zeros(10)), "no particle"),
                          (dict(center=(0.0, 1.0)), "center"), (dict(center=(np.inf, 0.0, 0.0)), "center"),
                          (dict(rho_threshold=0.0), "rho_threshold"), (dict(rho_threshold=np.nan), "rho_threshold"),
                          (dict(rho_threshold="200c"), "rho_threshold"), (dict(r_max=0.0), "r_max"), (dict(r_max=np.inf), "r_max"),
                          (dict(refinements=-1), "refinements"), (dict(refinements=9), "refinements"), (dict(refinements=1.5), "refinements"),
                          (dict(refinements=True), "refinements")):
        with pytest.raises(ValueError, match=match):
            topsy_amd.virial_radius(**{**good, **change})
    for kwargs, match in ((dict(rho_threshold=-1.0, r_max=1.0), "rho_threshold"), (dict(rho_threshold=1.0, r_max=-1.0), "r_max")):
        with pytest.raises(ValueError, match=match):
            ld.virial_radius(**kwargs)


# ---- the loader, with a context stubbed by the reference ----------------------------------------------------------------------
class StubContext:
    """What ArrayDataLoader asks of a context for a profile, answered by the references."""

    def __init__(self):
        self.calls = []

    def sphere_moments(self, x, y, z, mass, vel=None, center=(0.0, 0.0, 0.0), r=1.0, r_vel=0.0):
        from test_orient_cpu import sphere_moments_reference
        self.calls.append(("moments", r, r_vel))
        return sphere_moments_reference(np.stack([x, y, z], axis=1), mass, None if vel is None else np.stack(vel, axis=1), center, r, r_vel)

    def radial_profile(self, x, y, z, mass, vel=None, **spec):
        self.calls.append(("profile", spec))
        return radial_profile_reference(np.stack([x, y, z], axis=1), mass, None if vel is None else np.stack(vel, axis=1), **spec)


def _loader(name="disc", **kwargs):
    from topsy_amd import loader
    pos, mass, vel, base = scene(name)
    ld = loader.ArrayDataLoader(pos=pos, smooth=np.full(len(pos), 0.1, dtype=np.float32), mass=mass, vel=vel, center=base["center"], **kwargs)
    stub = StubContext()
    ld.set_density_context(stub)
    return ld, stub


def test_loader_profile(monkeypatch):
    from test_orient_cpu import sphere_moments_reference
    _no_context(monkeypatch)
    pos, mass, vel, base = scene("disc")
    ld, stub = _loader()
    p = ld.profile(R_MAX, r_min=R_MIN, n_bins=8, geometry="disc", frame=base["frame"], half_height=HALF_HEIGHT, v_cen=base["v_cen"], G=2.0)
    ref = reference("disc", 1, 8)
    assert [c[0] for c in stub.calls] == ["profile"] and stub.calls[0][1]["geometry"] == 1
    assert np.array_equal(p.sums, ref["sums"]) and np.array_equal(p.n, ref["count"]) and p.geometry == "disc"
    assert p.info["n_inner"] == ref["n_inner"] and p.info["mass_inner"] == ref["mass_inner"] and p.info["n_valid"] == ref["n_valid"]
    assert np.array_equal(p.v_circ, np.sqrt(2.0 * p.mass_enc / p.edges[1:]))
    # the defaults: the initial centre, the identity, any height, and the velocity centre of the inner fifth
    ld, stub = _loader()
    p = ld.profile(R_MAX, n_bins=8)
    assert [c[0] for c in stub.calls] == ["moments", "profile"] and stub.calls[0][1:] == (R_MAX, 0.2 * R_MAX)
    spec = stub.calls[1][1]
    v_cen = sphere_moments_reference(pos, mass, vel, center=AT, r=R_MAX, r_vel=0.2 * R_MAX)["v_cen"]
    assert np.array_equal(spec["center"], AT) and np.array_equal(spec["frame"], np.eye(3)) and spec["half_height"] == np.inf
    assert np.array_equal(spec["v_cen"], v_cen) and np.array_equal(p.info["v_cen"], v_cen) and spec["geometry"] == 0
    assert np.array_equal(spec["edges"], np.arange(9) * 0.5) and p.info["n_inner"] == 0
    # explicit edges: the sphere of the outermost edge gives v_cen
    ld, stub = _loader()
    ld.profile(bins=[0.5, 1.0, 3.0])
    assert stub.calls[0][1:] == (3.0, 0.2 * 3.0) and np.array_equal(stub.calls[1][1]["edges"], [0.5, 1.0, 3.0])
    # without velocities nothing asks for a velocity centre, and the profile carries none
    ld, stub = _loader("no_vel")
    p = ld.profile(R_MAX, n_bins=8)
    assert [c[0] for c in stub.calls] == ["profile"] and p.v_r is None and p.j is None
    assert p.mass.sum() == pytest.approx(radial_profile_reference(pos, mass, None, edges=[0.0, R_MAX], center=AT)["sums"][0, 0], rel=1e-12)


# ---- the virial radius --------------------------------------------------------------------------------------------------------
def downward_crossings(pos, mass, center, threshold, r_lo, r_hi):
    """Every radius in [r_lo, r_hi] at which the mean enclosed density 3 M(<r) / (4 pi r^3) of the sorted radii falls through
    `threshold`: between two particles M is constant and the density falls as r^-3, so there is at most one per gap."""
    d = np.asarray(pos, dtype=np.float64) - np.asarray(center, dtype=np.float64)
    r = np.sqrt((d * d).sum(axis=1))
    order = np.argsort(r, kind="stable")
    r = np.append(r[order], np.inf)
    enclosed = np.cumsum(np.asarray(mass, dtype=np.float64)[order])
    at = np.cbrt(3.0 * enclosed / (4.0 * np.pi * threshold))
    hit = (at >= r[:-1]) & (at < r[1:]) & (at >= r_lo) & (at <= r_hi)
    return at[hit]


def _virial_scenes():
    rs = np.random.RandomState(17)
    # a dense ball of radius 1, nothing out to 6, a thin cloud beyond: one clean crossing inside the gap
    n = 5000
    ball = rs.normal(size=(n, 3))
    ball *= (rs.uniform(size=n) ** (1.0 / 3.0) / np.linalg.norm(ball, axis=1))[:, None]
    cloud = rs.normal(size=(2000, 3))
    cloud *= (rs.uniform(6.0, 8.0, size=2000) / np.linalg.norm(cloud, axis=1))[:, None]
    gap_pos = (np.concatenate([ball, cloud]) + AT).astype(np.float32)
    gap_mass = rs.uniform(0.5, 1.5, size=len(gap_pos)).astype(np.float32)
    gap_threshold = 3.0 * gap_mass[:n].astype(np.float64).sum() / (4.0 * np.pi * 3.7 ** 3)
    # a Hernquist-like halo (scale radius 1): the density falls smoothly through the threshold among the particles
    u = rs.uniform(0.0, 0.96, size=7000)
    radius = np.sqrt(u) / (1.0 - np.sqrt(u))
    halo = rs.normal(size=(7000, 3))
    halo_pos = (halo * (radius / np.linalg.norm(halo, axis=1))[:, None] + AT).astype(np.float32)
    halo_mass = np.ones(7000, dtype=np.float32)
    halo_threshold = 3.0 * 7000 * 0.25 / (4.0 * np.pi * 1.0 ** 3) / 8.0       # about the mean density inside r = 2.4
    return {"gap": (gap_pos, gap_mass, gap_threshold, 8.0), "halo": (halo_pos, halo_mass, halo_threshold, 30.0)}


VIRIAL_SCENES = _virial_scenes()


def reference_shell_masses(pos, mass, center):
    def shell_masses(edges):
        ref = radial_profile_reference(pos, mass, None, edges=edges, geometry=0, center=center)
        return ref["sums"][:, 0], ref["mass_inner"]
    return shell_masses


@pytest.mark.parametrize("name", sorted(VIRIAL_SCENES))
@pytest.mark.parametrize("refinements", [0, 1, 3])
def test_virial_radius_against_the_sorted_radii(name, refinements):
    """The bracketing rule on the reference's shell masses against the crossings of the sorted radii: the last bracket holds a
    crossing, so the two agree to within its width -- which is what the rule computed, r_max-independent after three refinements
    (256^-3 of a level-0 bin).  In the "gap" scene the crossing is the only one; in the "halo" scene the density ripples through
    the threshold from particle to particle, and the rule's answer is held to the crossing nearest to it and, by the level-0
    rule, to the first level-0 bin whose ends straddle the threshold."""
    from topsy_amd import loader
    pos, mass, threshold, r_max = VIRIAL_SCENES[name]
    r_vir, (lower, upper) = loader.find_virial_radius(reference_shell_masses(pos, mass, AT), threshold, r_max, refinements)
    level0 = loader.profile_edges("log", 256, r_max / 1024.0, r_max)
    k = np.searchsorted(level0, r_vir, side="right")
    width = (level0[k] - level0[k - 1]) / 256.0 ** refinements
    crossings = downward_crossings(pos, mass, AT, threshold, r_max / 1024.0, r_max)
    print(f"{name}, {refinements} refinements: r_vir = {r_vir!r} in [{lower!r}, {upper!r}] (width {upper - lower:.3g}, expected {width:.3g}), "
          f"{len(crossings)} crossing(s) of the sorted radii, the first at {crossings[0]!r}, the nearest {np.abs(crossings - r_vir).min():.3g} away")
    assert lower <= r_vir <= upper and upper - lower <= width + 4 * np.spacing(r_max)       # (the edges are rounded)
    assert np.abs(crossings - r_vir).min() <= upper - lower
    assert ((crossings >= lower) & (crossings <= upper)).any()
    # the density at the bracket's ends, from the sorted radii
    d = np.sqrt(((pos.astype(np.float64) - AT) ** 2).sum(axis=1))
    rho = lambda r: 3.0 * mass[d < r].astype(np.float64).sum() / (4.0 * np.pi * r ** 3)       # noqa: E731
    assert rho(lower) >= threshold > rho(upper)
    if name == "gap":
        assert len(crossings) == 1 and 3.6 < r_vir < 3.8
    else:
        # level 0: no earlier bin falls from above to below
        rho0 = np.array([rho(e) for e in level0])
        first = np.flatnonzero((rho0[:-1] >= threshold) & (rho0[1:] < threshold))[0]
        assert level0[first] <= r_vir <= level0[first + 1]


def test_virial_radius_without_a_crossing():
    from topsy_amd import loader
    pos, mass, threshold, r_max = VIRIAL_SCENES["gap"]
    shell_masses = reference_shell_masses(pos, mass, AT)
    with pytest.raises(ValueError, match="never falls"):          # always above
        loader.find_virial_radius(shell_masses, threshold * 1e-6, r_max)
    with pytest.raises(ValueError, match="never falls"):          # always below
        loader.find_virial_radius(shell_masses, threshold * 1e9, r_max)
    with pytest.raises(ValueError, match="never falls"):          # r_max inside the ball: still above at r_max
        loader.find_virial_radius(shell_masses, threshold, 0.9)


def test_loader_virial_radius(monkeypatch):
    from topsy_amd import loader
    _no_context(monkeypatch)
    pos, mass, threshold, r_max = VIRIAL_SCENES["gap"]
    ld = loader.ArrayDataLoader(pos=pos, smooth=np.ones(len(pos), dtype=np.float32), mass=mass, center=tuple(AT))
    stub = StubContext()
    ld.set_density_context(stub)
    want, _ = loader.find_virial_radius(reference_shell_masses(pos, mass, AT), threshold, r_max, 3)
    assert ld.virial_radius(threshold, r_max) == want
    assert len(stub.calls) == 4 and all(len(c[1]["edges"]) == 257 and c[1]["geometry"] == 0 for c in stub.calls)
    assert np.array_equal(stub.calls[0][1]["edges"], loader.profile_edges("log", 256, r_max / 1024.0, r_max))
    assert ld.virial_radius(threshold, r_max, center=AT, refinements=0) == loader.find_virial_radius(
        reference_shell_masses(pos, mass, AT), threshold, r_max, 0)[0]


def test_binding_matches_the_header():
    import ctypes
    import os
    import re
    from topsy_amd import _native, multigpu, surface, visualizer
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "topsy_splat.h")).read()
    assert " * 116: new entry point tsp_radial_profile" in text
    for struct_name, cls in (("tsp_profile_spec", _native.ProfileSpec), ("tsp_profile_info", _native.ProfileInfo)):
        struct = re.search(r"typedef struct \{([^}]*)\} " + struct_name + ";", text).group(1)
        fields = re.findall(r"\b(int32_t|int64_t|const double|double)\s+([^;]*);", re.sub(r"/\*.*?\*/", "", struct))
        declared = [name.strip().lstrip("*").split("[")[0] for _, names in fields for name in names.split(",")]
        assert declared == [name for name, _ in cls._fields_], struct_name
    assert ctypes.sizeof(_native.ProfileSpec) == 8 + 8 + 8 * (3 + 3 + 9 + 1) and ctypes.sizeof(_native.ProfileInfo) == 32
    restype, argtypes = _native.SIGNATURES["tsp_radial_profile"]
    assert restype is ctypes.c_int and len(argtypes) == 13
    assert _native.ABI_VERSION == 112 and _native.load_library().tsp_version() >= 116
    assert hasattr(_native.Context, "radial_profile") and hasattr(multigpu.MultiGpuContext, "radial_profile")
    for cls in (visualizer.Visualizer, surface.SurfaceView):
        assert hasattr(cls, "profile") and hasattr(cls, "scale_to_virial")
    contract = text[text.index("/* Radial profiles: per radial bin"):text.index("} tsp_profile_spec;")]
    assert "Not\n * provided: periodic wrapping" in contract or "Not provided: periodic wrapping" in contract.replace("\n *", "")
    srcs = open(os.path.join(root, "topsy_amd", "csrc", "Makefile")).read()
    assert "tsp_profile.hip" in srcs
