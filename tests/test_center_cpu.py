"""The shrinking-sphere centre on the CPU: shrink_sphere_reference, the NumPy float64 restatement of the contract of
tsp_shrink_sphere_center (include/topsy_splat.h) that test_gpu_center.py holds the GPU to; the scenes both files use, with the
properties of the inputs that the GPU comparison relies on (no particle within a relative 1e-9 of any trial radius) established
here by the reference alone; and the host-side argument checks, which raise before any context is needed."""
import functools

import numpy as np
import pytest

ZOOM_CUT = 1.01
SIGMA = 0.01
CLUMP_AT = np.array([0.71, 0.33, 0.58])
OFFSET = np.array([1e4, -2e4, 3e4])


def shrink_sphere_reference(pos, mass, mass_cut_factor=0.0, r_start=0.0, shrink_factor=0.7, min_particles=100, max_iterations=256):
    """The contract in float64 (numpy's pairwise sums; no fused multiply-adds).  Returns (centre (3,), info dict, trace): the
    trace holds, for every trial radius, (c before the trial, r_try, number inside) -- the last entry is the trial that was
    refused, unless max_iterations ended the loop; trace[k][0] is therefore the centre after k updates."""
    pos = np.asarray(pos, dtype=np.float32)
    mass = np.asarray(mass, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(pos).all(axis=1) & np.isfinite(mass) & (mass > 0)
        if mass_cut_factor > 0:
            m_min = mass[valid].min()
            valid &= mass.astype(np.float64) < np.float64(np.float32(mass_cut_factor)) * np.float64(m_min)
    p = pos[valid].astype(np.float64)
    m = mass[valid].astype(np.float64)
    if len(p) == 0:
        raise ValueError("no valid particle")
    c = (m[:, None] * p).sum(axis=0) / m.sum()
    r = float(r_start) if r_start > 0 else (p[:, 0].max() - p[:, 0].min()) / 2.0
    info = {"n_valid": len(p), "n_inside": len(p), "iterations": 0, "radius": r, "mass_inside": float(m.sum())}
    trace = []
    while info["iterations"] < max_iterations:
        r_try = r * shrink_factor
        d = p - c
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        inside = d2 < r_try * r_try
        count = int(inside.sum())
        trace.append((c.copy(), r_try, count))
        if count < min_particles:
            break
        mi = m[inside]
        c = c + (mi[:, None] * d[inside]).sum(axis=0) / mi.sum()
        r = r_try
        info.update(iterations=info["iterations"] + 1, n_inside=count, radius=r, mass_inside=float(mi.sum()))
    return c, info, trace


def near_tie_margin(pos, mass, trace, mass_cut_factor=0.0):
    """The smallest | |p - c| / r_try - 1 | over every valid particle and every trial of the trace: how far the inputs are from a
    membership that a rounding difference could flip."""
    pos = np.asarray(pos, dtype=np.float32)
    mass = np.asarray(mass, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(pos).all(axis=1) & np.isfinite(mass) & (mass > 0)
        if mass_cut_factor > 0:
            valid &= mass.astype(np.float64) < np.float64(np.float32(mass_cut_factor)) * np.float64(mass[valid].min())
    p = pos[valid].astype(np.float64)
    margin = np.inf
    for c, r_try, _ in trace:
        if r_try == 0.0:
            continue
        dist = np.sqrt(((p - c) ** 2).sum(axis=1))
        margin = min(margin, float(np.abs(dist / r_try - 1.0).min()))
    return margin


# ---- scenes ---------------------------------------------------------------------------------------------------------------
def clump_in_box(n, seed, clump_fraction=0.2, at=CLUMP_AT, sigma=SIGMA):
    """A uniform unit box with a compact Gaussian clump (equal masses, so the clump holds clump_fraction of the mass)."""
    rs = np.random.RandomState(seed)
    n_clump = int(round(n * clump_fraction))
    pos = rs.uniform(0.0, 1.0, size=(n, 3))
    pos[:n_clump] = at + rs.normal(scale=sigma, size=(n_clump, 3))
    pos = pos[rs.permutation(n)]
    return pos.astype(np.float32), np.ones(n, dtype=np.float32), n_clump


@functools.lru_cache(maxsize=None)
def scene(name):
    """(pos float32 (n, 3), mass float32 (n,), keyword arguments of the call).  Every n leaves a ragged last block of 1024."""
    kw = {}
    if name in ("clump", "clump_sorted"):
        pos, mass, n_clump = clump_in_box(20 * 1024 + 17, 3)
        kw["min_particles"] = n_clump // 2      # (why: test_reference_finds_the_clump_and_the_mean_does_not)
        if name == "clump_sorted":
            order = np.argsort(pos[:, 0], kind="stable")
            pos, mass = pos[order], mass[order]
    elif name == "offset":
        # float32 coordinates near 3e4 are 2e-3 apart: the clump is a few steps wide and many of its members coincide
        pos, mass, _ = clump_in_box(3 * 1024 + 17, 5)
        pos = (pos.astype(np.float64) + OFFSET).astype(np.float32)
    elif name == "mass_range":
        pos, mass, _ = clump_in_box(196 * 1024 + 17, 7)
        mass = (10.0 ** np.random.RandomState(8).uniform(-6, 6, size=len(pos))).astype(np.float32)
    elif name == "invalid":
        pos, mass, _ = clump_in_box(40 * 1024 + 17, 9)
        rs = np.random.RandomState(10)
        n = len(pos)
        bad = rs.choice(n, n // 100, replace=False)
        pos[bad, rs.randint(0, 3, size=len(bad))] = rs.choice([np.nan, np.inf, -np.inf], size=len(bad))
        for value in (0.0, -1.0, np.nan, np.inf, -0.0, -np.inf):
            mass[rs.choice(n, 50, replace=False)] = value
    elif name == "duplicates":
        pos, mass, _ = clump_in_box(3 * 1024 + 17, 11, clump_fraction=0.0)
        pos[np.random.RandomState(12).choice(len(pos), 150, replace=False)] = np.float32([0.5078125, 0.49609375, 0.50390625])
    elif name == "too_few":
        pos, mass, _ = clump_in_box(3 * 1024 + 17, 13)
        keep = np.random.RandomState(14).choice(len(pos), 60, replace=False)
        light = np.zeros(len(pos), dtype=np.float32)
        light[keep] = 1.0 + np.arange(60, dtype=np.float32)
        mass = light
    elif name in ("zoom", "zoom_all"):
        # heavy species (mass 8): a box with its own clump at CLUMP_AT; light species (mass 1): a clump elsewhere and a few strays
        heavy, _, _ = clump_in_box(10 * 1024, 15, clump_fraction=0.3)
        light, _, _ = clump_in_box(4 * 1024 + 17, 16, clump_fraction=0.8, at=np.array([0.25, 0.62, 0.4]))
        pos = np.concatenate([heavy, light])
        mass = np.concatenate([np.full(len(heavy), 8.0), np.ones(len(light))]).astype(np.float32)
        order = np.random.RandomState(17).permutation(len(pos))
        pos, mass = pos[order], mass[order]
        if name == "zoom":
            kw["mass_cut_factor"] = ZOOM_CUT
    else:
        raise KeyError(name)
    pos.setflags(write=False)
    mass.setflags(write=False)
    return pos, mass, kw


SCENES = ("clump", "clump_sorted", "offset", "mass_range", "invalid", "duplicates", "too_few", "zoom", "zoom_all")


@functools.lru_cache(maxsize=None)
def reference(name):
    pos, mass, kw = scene(name)
    return shrink_sphere_reference(pos, mass, **kw)


def lattice_scene(order):
    """The integer lattice {-6..6}^3 with equal masses: every sum of the contract is exact in float64."""
    g = np.arange(-6, 7, dtype=np.float32)
    pos = np.stack([v.ravel() for v in np.meshgrid(g, g, g, indexing="ij")], axis=1)
    if order == "shuffled":
        pos = pos[np.random.RandomState(21).permutation(len(pos))]
    else:
        pos = pos[np.argsort(pos[:, 0], kind="stable")]
    return np.ascontiguousarray(pos), np.ones(len(pos), dtype=np.float32)


# ---- the reference and the inputs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_reference_finds_the_clump_and_the_mean_does_not(seed):
    """The final centre is the mean of the n_inside particles of the last sphere, so its error is about the spread of those
    particles over sqrt(n_inside): it can meet 3 sigma / sqrt(N_clump) only when the last sphere still holds a good part of the
    clump.  Stopping at half the clump (a sphere of about 1.5 sigma: the expected error is 1.5 sigma / sqrt(N_clump), and the
    uniform background puts less than one particle inside) does; pynbody's default of 100 particles is for haloes whose centre is
    a cusp, and misses this bound on a Gaussian clump of 4000 more often than not."""
    pos, mass, n_clump = clump_in_box(20 * 1024 + 17, seed)
    c, info, trace = shrink_sphere_reference(pos, mass, min_particles=n_clump // 2)
    bound = 3 * SIGMA / np.sqrt(n_clump)
    err = float(np.linalg.norm(c - CLUMP_AT))
    mean = (mass[:, None].astype(np.float64) * pos).sum(axis=0) / mass.sum(dtype=np.float64)
    print(f"seed {seed}: |c - clump| = {err:.3g} (bound {bound:.3g}), |mean - clump| = {np.linalg.norm(mean - CLUMP_AT):.3g}, "
          f"{info['iterations']} iterations, r = {info['radius']:.3g}, {info['n_inside']} inside")
    assert err <= bound
    assert np.linalg.norm(mean - CLUMP_AT) > 100 * bound
    assert n_clump // 2 <= info["n_inside"] and trace[-1][2] < n_clump // 2 and info["iterations"] == len(trace) - 1
    assert np.array_equal(trace[0][0], mean) or np.allclose(trace[0][0], mean, rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", SCENES)
def test_scenes_have_no_near_ties(name):
    pos, mass, kw = scene(name)
    c, info, trace = reference(name)
    margin = near_tie_margin(pos, mass, trace, kw.get("mass_cut_factor", 0.0))
    print(f"{name}: n = {len(pos)}, valid {info['n_valid']}, {info['iterations']} iterations, r = {info['radius']:.3g}, "
          f"{info['n_inside']} inside, nearest tie {margin:.3g}")
    assert len(pos) % 1024 != 0 and 3 * 1024 + 17 <= len(pos) <= 201_000
    assert margin > 1e-9
    assert np.isfinite(c).all()


def test_scene_properties():
    """What each scene is for, shown by the reference."""
    _, info, _ = reference("clump")
    c_sorted, info_sorted, _ = reference("clump_sorted")
    assert info_sorted["iterations"] == info["iterations"] and info_sorted["n_inside"] == info["n_inside"]
    assert np.allclose(c_sorted, reference("clump")[0], rtol=0, atol=1e-12)
    # offset: the centre sits at OFFSET + the clump, and the final radius is far above the spacing of float64 there
    c, info, _ = reference("offset")
    assert np.linalg.norm(c - OFFSET - CLUMP_AT) < 0.01
    assert 1e-9 * info["radius"] > 2 * np.spacing(3e4)
    # invalid data: the valid count is what the rule says
    pos, mass, _ = scene("invalid")
    with np.errstate(invalid="ignore"):
        assert reference("invalid")[1]["n_valid"] == int((np.isfinite(pos).all(axis=1) & np.isfinite(mass) & (mass > 0)).sum())
    assert reference("invalid")[1]["n_valid"] < len(pos) - 500
    # duplicates: the loop ends at the cap, on the point, with the 150 copies inside
    c, info, trace = reference("duplicates")
    assert info["iterations"] == 256 and info["n_inside"] == 150 and len(trace) == 256
    assert np.array_equal(c, np.float64([0.5078125, 0.49609375, 0.50390625]))
    # too few: no update, the centre of mass
    pos, mass, _ = scene("too_few")
    c, info, trace = reference("too_few")
    assert info["iterations"] == 0 and info["n_valid"] == info["n_inside"] == 60 and len(trace) == 1
    sel = mass > 0
    assert np.allclose(c, (mass[sel, None].astype(np.float64) * pos[sel]).sum(axis=0) / mass[sel].sum(dtype=np.float64), atol=1e-12)
    # zoom: the light species' clump with the cut, the heavy one's without
    c_zoom, info_zoom, _ = reference("zoom")
    c_all, info_all, _ = reference("zoom_all")
    assert info_zoom["n_valid"] == 4 * 1024 + 17 and info_all["n_valid"] == 14 * 1024 + 17
    assert np.linalg.norm(c_zoom - [0.25, 0.62, 0.4]) < 0.005 and np.linalg.norm(c_all - CLUMP_AT) < 0.005


def test_lattice_reference_is_exact():
    for order in ("shuffled", "sorted"):
        pos, mass = lattice_scene(order)
        p2 = (pos.astype(np.float64) ** 2).sum(axis=1)
        for k, bound in ((1, 16), (2, 4), (3, 1)):
            c, info, _ = shrink_sphere_reference(pos, mass, r_start=8.0, shrink_factor=0.5, min_particles=1, max_iterations=k)
            assert np.array_equal(c, np.zeros(3)) and info["iterations"] == k
            assert info["n_inside"] == int((p2 < bound).sum()) and info["radius"] == 8.0 * 0.5 ** k
        assert int((p2 == 16).sum()) > 0 and int((p2 == 4).sum()) == 6 and int((p2 == 1).sum()) == 6


def test_reference_argument_semantics():
    pos, mass, _ = scene("clump")
    c0, info0, _ = shrink_sphere_reference(pos, mass, max_iterations=0)
    assert info0["iterations"] == 0 and info0["n_inside"] == len(pos)
    assert info0["radius"] == (np.float64(pos[:, 0].max()) - np.float64(pos[:, 0].min())) / 2
    c3, info3, trace3 = shrink_sphere_reference(pos, mass, max_iterations=3)
    full = shrink_sphere_reference(pos, mass)[2]
    assert info3["iterations"] == 3 and len(trace3) == 3 and np.array_equal(c3, full[3][0])
    assert shrink_sphere_reference(pos, mass, r_start=0.05)[2][0][1] == 0.05 * 0.7


# ---- the host layer: checked before a context is needed -------------------------------------------------------------------
def _no_context(monkeypatch):
    from topsy_amd import _native

    def refuse(*a, **k):
        raise AssertionError("a context was created before the arguments were checked")
    monkeypatch.setattr(_native, "Context", refuse)


def test_shrink_sphere_center_checks_its_arguments_first(monkeypatch):
    import topsy_amd
    _no_context(monkeypatch)
    pos = np.zeros((10, 3), dtype=np.float32)
    mass = np.ones(10, dtype=np.float32)
    bad = [
        (dict(pos=np.zeros((10, 2)), mass=mass), r"\(10, 2\)"),
        (dict(pos=np.zeros(30), mass=mass), r"\(30,\)"),
        (dict(pos=pos, mass=np.ones(9)), r"\(9,\)"),
        (dict(pos=pos, mass=np.ones((10, 1))), r"\(10, 1\)"),
        (dict(pos=np.zeros((0, 3)), mass=np.ones(0)), "at least one"),
        (dict(pos=pos, mass=mass, select="halo-1"), "halo-1"),
        (dict(pos=pos, mass=mass, select=None), "None"),
        (dict(pos=pos, mass=mass, r_start=0.0), "0.0"),
        (dict(pos=pos, mass=mass, r_start=-1.0), "-1.0"),
        (dict(pos=pos, mass=mass, r_start=np.inf), "inf"),
        (dict(pos=pos, mass=mass, r_start="wide"), "wide"),
        (dict(pos=pos, mass=mass, shrink_factor=1.0), "1.0"),
        (dict(pos=pos, mass=mass, shrink_factor=0.0), "0.0"),
        (dict(pos=pos, mass=mass, shrink_factor=np.nan), "nan"),
        (dict(pos=pos, mass=mass, min_particles=0), "0"),
        (dict(pos=pos, mass=mass, min_particles=2.5), "2.5"),
        (dict(pos=pos, mass=mass, min_particles=True), "True"),
        (dict(pos=pos, mass=np.zeros(10)), "no particle"),
        (dict(pos=np.full((10, 3), np.nan), mass=mass), "no particle"),
    ]
    for kwargs, match in bad:
        with pytest.raises(ValueError, match=match):
            topsy_amd.shrink_sphere_center(**kwargs)


def test_from_arrays_checks_center_first(monkeypatch):
    import topsy_amd
    from topsy_amd import loader
    _no_context(monkeypatch)
    pos = np.zeros((10, 3), dtype=np.float32)
    h = np.ones(10, dtype=np.float32)
    for center, match in (("halo-3", "halo-3"), ("centre", "centre"), ((1.0, 2.0), "1.0, 2.0"), (np.zeros((3, 1)), "center"),
                          ((0.0, np.nan, 0.0), "nan"), (None, "None"), (7, "7")):
        with pytest.raises(ValueError, match=match):
            topsy_amd.from_arrays(pos, h, h, center=center)
        with pytest.raises(ValueError, match=match):
            loader.ArrayDataLoader(pos=pos, smooth=h, mass=h, center=center)
    with pytest.raises(ValueError, match=r"\(10, 2\)"):
        loader.ArrayDataLoader(pos=np.zeros((10, 2)), smooth=h, mass=h, center="all")
    with pytest.raises(ValueError, match="-2"):
        loader.ArrayDataLoader(pos=pos, smooth=h, mass=h, center="zoom").set_initial_center([0.0, -2])


def test_center_none_and_explicit_centres_need_no_gpu(monkeypatch):
    from topsy_amd import loader
    _no_context(monkeypatch)
    pos = np.random.RandomState(0).uniform(size=(10, 3)).astype(np.float32)
    h = np.ones(10, dtype=np.float32)
    ld = loader.ArrayDataLoader(pos=pos, smooth=h, mass=h)
    assert np.array_equal(ld.get_initial_center(), np.zeros(3)) and ld.get_initial_center().dtype == np.float32
    ld = loader.ArrayDataLoader(pos=pos, smooth=h, mass=h, center="none")
    assert np.array_equal(ld.get_initial_center(), np.zeros(3))
    ld = loader.ArrayDataLoader(pos=pos, smooth=h, mass=h, center=(1.5, -2.0, 1e4), with_cells=True)
    assert np.array_equal(ld.get_initial_center(), [1.5, -2.0, 1e4]) and ld.get_initial_center().dtype == np.float64
    # a centre from the caller's cache: nothing is computed
    ld = loader.ArrayDataLoader(pos=pos, smooth=h, mass=h, center="all")
    ld.set_initial_center([0.25, 0.5, 0.75])
    assert np.array_equal(ld.get_initial_center(), [0.25, 0.5, 0.75])
    ld = loader.ArrayDataLoader(pos=pos, smooth=h, mass=h)
    ld.set_initial_center(np.float32([1, 2, 3]))
    assert np.array_equal(ld.get_initial_center(), [1.0, 2.0, 3.0])


def test_binding_matches_the_header():
    import ctypes
    import os
    import re
    from topsy_amd import _native, multigpu
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "topsy_splat.h")).read()
    assert " * 113: new entry point tsp_shrink_sphere_center" in text
    assert re.search(r"int64_t n_valid, n_inside;\s*int32_t iterations, reserved;\s*double radius, mass_inside;\s*\} tsp_center_info;", text)
    assert ("int tsp_shrink_sphere_center(tsp_context *ctx, int64_t n, const float *x, const float *y, const float *z, "
            "const float *mass,") in text
    assert ctypes.sizeof(_native.CenterInfo) == 40
    restype, argtypes = _native.SIGNATURES["tsp_shrink_sphere_center"]
    assert restype is ctypes.c_int and len(argtypes) == 13
    assert _native.load_library().tsp_version() >= 113
    assert hasattr(_native.Context, "shrink_sphere_center") and hasattr(multigpu.MultiGpuContext, "shrink_sphere_center")
