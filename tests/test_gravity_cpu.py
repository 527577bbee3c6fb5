"""Direct-sum gravity without a GPU: the float64 model (gravity_ref.py) against closed forms, the host layer of
topsy_amd.gravity_direct / rotation_curve / from_arrays(eps=...), and the header against the binding."""
import os
import re

import numpy as np
import pytest

import gravity_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


# ---- the model against closed forms ---------------------------------------------------------------------------------------------
def test_model_two_bodies():
    src = np.array([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0]])
    mass = np.array([2.0, 5.0])
    eps = np.array([0.5, 0.25])
    ref = gravity_ref.direct_sum(src, mass, eps)
    r2_0 = 25.0 + 0.25 ** 2           # body 0 feels body 1, softened with body 1's length
    r2_1 = 25.0 + 0.5 ** 2
    assert ref["pot"] == pytest.approx([-5.0 / np.sqrt(r2_0), -2.0 / np.sqrt(r2_1)], rel=1e-15)
    assert ref["acc"][0] == pytest.approx(5.0 * r2_0 ** -1.5 * np.array([3.0, 4.0, 0.0]), rel=1e-15)      # toward body 1
    assert ref["acc"][1] == pytest.approx(-2.0 * r2_1 ** -1.5 * np.array([3.0, 4.0, 0.0]), rel=1e-15)
    assert ref["pot_scale"] == pytest.approx(-ref["pot"]) and ref["n_valid_sources"] == 2 and ref["n_valid_targets"] == 2
    # explicit targets: the same particles see themselves too (distance 0, eps > 0: an ordinary pair)
    both = gravity_ref.direct_sum(src, mass, eps, targets=src)
    assert both["pot"] == pytest.approx(ref["pot"] - mass / eps, rel=1e-15)
    assert both["acc"] == pytest.approx(ref["acc"], rel=1e-15)


def test_model_validity_rules():
    src = np.array([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [2, 0, 0], [3, 0, 0], [1, 0, 0]], dtype=f32)
    mass = np.array([1, 1, 1, np.inf, 1, 0], dtype=f32)
    eps = np.array([0, 0, 0.1, 0.1, np.nan, 0], dtype=f32)
    ref = gravity_ref.direct_sum(src, mass, eps)
    assert ref["n_valid_sources"] == 3 and ref["n_valid_targets"] == 5          # sources 0, 1, 5; every target but 2
    assert np.isnan(ref["pot"][2]) and np.isnan(ref["acc"][2]).all()
    # target 1 coincides with the massless source 5 at eps 0: r2 == 0, nothing; it feels source 0 alone
    assert ref["pot"][1] == -1.0 and np.array_equal(ref["acc"][1], [-1.0, 0.0, 0.0])
    # target 3 (left out as a source for its mass) is still a target
    assert ref["pot"][3] == pytest.approx(-(1 / 2 + 1 / 1))


def test_model_plummer_point_mass_rotation_curve():
    """a softened point mass: rotation_curve's rule applied to the model's accelerations gives v^2 = G M R^2 / (R^2 + eps^2)^1.5"""
    from topsy_amd import gravity
    M, eps, G = 3.0, 0.7, 4.3e-6
    radii = np.array([0.1, 0.5, 1.0, 2.0, 8.0])
    frame = np.array([[0.6, 0.8, 0.0], [-0.8, 0.6, 0.0], [0.0, 0.0, 1.0]])
    probes = gravity.rotation_probes(radii, frame).reshape(-1, 3).astype(f32)
    ref = gravity_ref.direct_sum(np.zeros((1, 3)), [M], eps, targets=probes)
    curve = gravity.RotationCurve(radii, probes, ref["pot"], ref["acc"], G)
    e2 = float(f32(eps)) ** 2
    assert curve.v_circ == pytest.approx(np.sqrt(G * M * radii ** 2 / (radii ** 2 + e2) ** 1.5), rel=1e-6)     # (float32 probes)
    assert curve.pot == pytest.approx(-G * M / np.sqrt(radii ** 2 + e2), rel=1e-6)
    assert curve.acc.shape == (5, 4, 3) and len(curve) == 5


def test_model_lattice_centre_is_force_free():
    g = np.arange(-3, 4, dtype=np.float64)
    src = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    ref = gravity_ref.direct_sum(src, np.ones(len(src)), 0.05, targets=np.zeros((1, 3)))
    # the terms cancel in pairs: what is left is the rounding of a float64 sum of 343 terms
    assert np.abs(ref["acc"][0]).max() <= 343 * 2.0 ** -52 * ref["acc_scale"][0].max()
    assert ref["pot"][0] < 0 and ref["acc_scale"][0].min() > 1.0


# ---- the host layer ---------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    import topsy_amd
    from topsy_amd import gravity
    pos, mass = np.zeros((4, 3)), np.ones(4)
    for bad in ({"pos": np.zeros((4, 2))}, {"pos": np.zeros((0, 3)), "mass": np.ones(0)}, {"mass": np.ones(3)}, {"eps": None},
                {"eps": -1.0}, {"eps": np.nan}, {"eps": np.ones(3)}, {"eps": "soft"}):
        args = {"pos": pos, "mass": mass, "eps": 0.1} | bad
        with pytest.raises(ValueError):
            gravity.check_arrays(args["pos"], args["mass"], args["eps"])
    assert gravity.check_arrays(pos, mass, 0.25)[2] == 0.25
    assert gravity.check_arrays(pos, mass, [0.1, 0.2, np.nan, 0.4])[2].dtype == f32      # a non-finite entry: that source is left out
    for bad in (0.0, -1.0, np.inf, "g"):
        with pytest.raises(ValueError):
            gravity.check_G(bad)
    for bad in ([], [1.0, -2.0], [0.0], [np.nan], [[1.0, 2.0]]):
        with pytest.raises(ValueError):
            gravity.check_radii(bad)
    assert np.array_equal(gravity.check_radii(2.0), [2.0])
    for bad in ((0, 0), (0, 0, np.inf)):
        with pytest.raises(ValueError):
            gravity.check_center(bad)
    with pytest.raises(ValueError):
        gravity.check_frame(np.ones((3, 3)))
    with pytest.raises(ValueError):
        gravity.check_targets(np.zeros((3, 2)))
    # the public calls check before they look for a GPU
    with pytest.raises(ValueError):
        topsy_amd.gravity_direct(pos, mass, -1.0)
    with pytest.raises(ValueError):
        topsy_amd.rotation_curve(pos, mass, 0.1, radii=[-1.0])
    with pytest.raises(ValueError):
        topsy_amd.rotation_curve(pos, mass, 0.1, radii=[1.0], frame=2 * np.eye(3))
    assert topsy_amd.RotationCurve is gravity.RotationCurve


def test_probe_placement_in_a_rotated_frame():
    from topsy_amd import gravity
    from topsy_amd.loader import orientation_matrix
    a = np.array([1.0, 2.0, 2.0]) / 3.0
    frame = orientation_matrix({"L": a, "mass_vel": 1.0, "A": 1.0, "n_inside_vel": 10}, "faceon", "angmom")
    radii = np.array([0.5, 2.0])
    p = gravity.rotation_probes(radii, frame)
    assert p.shape == (2, 4, 3)
    assert np.allclose(p @ a, 0.0, atol=1e-15)                       # in the plane normal to the axis
    assert np.allclose(np.linalg.norm(p, axis=2), radii[:, None], rtol=1e-15)
    assert np.allclose(p[:, 0], -p[:, 1]) and np.allclose(p[:, 2], -p[:, 3])
    assert np.allclose((p[:, 0] * p[:, 2]).sum(axis=1), 0.0, atol=1e-15)      # the two diameters are perpendicular
    assert np.allclose(p[1, 0], 2.0 * frame[0]) and np.allclose(p[1, 2], 2.0 * frame[1])


def test_centre_is_subtracted_in_float64():
    from topsy_amd import gravity
    center = np.array([50000.0, -50000.0, 12345.678])
    offsets = np.array([[1e-3, 2e-3, -3e-3], [0.125, 0.25, 0.5]])
    pos = center[None, :] + offsets                                     # float64 positions far from the origin
    got = gravity.centred_positions(pos, center)
    assert got.dtype == f32
    assert np.allclose(got, offsets, rtol=1e-6, atol=1e-11)             # (float64 rounding of the sum, then one float32 rounding)
    lost = pos.astype(f32) - center.astype(f32)[None, :]                # what a float32 subtraction would leave
    assert np.abs(lost[0] - offsets[0]).max() > 1e-4


def _loader(**kw):
    from topsy_amd.loader import ArrayDataLoader
    rs = np.random.RandomState(5)
    n = 50
    kw = {"quantities": {"temp": np.ones(n)}} | kw
    return ArrayDataLoader(pos=rs.normal(size=(n, 3)), smooth=np.full(n, 0.1), mass=np.ones(n), **kw)


def test_phi_is_a_quantity_only_with_eps():
    without = _loader()
    assert without.get_quantity_names() == ["temp", "rho"] and without.get_softening() is None
    with pytest.raises(KeyError):
        without.get_named_quantity("phi")
    with pytest.raises(ValueError, match="softening"):
        without.rotation_curve([1.0])
    with_eps = _loader(eps=0.05, vel=np.zeros((50, 3)))
    assert with_eps.get_quantity_names() == ["temp", "rho", "v_div", "vorticity", "phi"]
    assert with_eps.get_softening() == pytest.approx(0.05)
    per_particle = _loader(eps=np.linspace(0.01, 0.1, 50), with_cells=True)
    assert per_particle.get_quantity_names()[-1] == "phi" and per_particle.get_softening().shape == (50,)
    assert sorted(per_particle.get_softening()) == pytest.approx(np.linspace(0.01, 0.1, 50), rel=1e-6)
    supplied = _loader(eps=0.05, quantities={"phi": np.arange(50.0)})
    assert supplied.get_quantity_names() == ["phi", "rho"] and supplied.get_named_quantity("phi")[7] == 7.0
    with pytest.raises(ValueError):
        _loader(eps=-1.0)
    with pytest.raises(ValueError):
        _loader(eps=np.ones(49))


def test_pair_cap_raises_before_any_gpu_work(monkeypatch):
    from topsy_amd import config
    assert config.GRAVITY_DIRECT_MAX_PAIRS >= 1e11
    monkeypatch.setattr(config, "GRAVITY_DIRECT_MAX_PAIRS", 2499)
    ld = _loader(eps=0.05)
    with pytest.raises(ValueError, match=r"50 x 50 = 2.5e\+03 pairs.*GRAVITY_DIRECT_MAX_PAIRS = 2.5e\+03"):
        ld.get_named_quantity("phi")


# ---- header and binding -----------------------------------------------------------------------------------------------------------
def test_header_and_binding():
    from topsy_amd import _native
    header = open(os.path.join(ROOT, "include", "topsy_splat.h")).read()
    assert re.search(r"\bint tsp_gravity_direct\(tsp_context \*ctx,", header)
    assert "typedef struct { int64_t n_valid_sources, n_valid_targets; } tsp_gravity_info;" in header
    assert re.search(r"^ \* 123: new entry point tsp_gravity_direct", header, flags=re.M)
    assert "tsp_gravity_direct" in _native.SIGNATURES and len(_native.SIGNATURES["tsp_gravity_direct"][1]) == 15
    assert _native.ABI_VERSION == 112
    assert [name for name, _ in _native.GravityInfo._fields_] == ["n_valid_sources", "n_valid_targets"]
    for macro, value in (("TSP_GRAVITY_SOURCE_TILE", _native.GRAVITY_SOURCE_TILE),
                         ("TSP_GRAVITY_TARGETS_PER_WORKGROUP", _native.GRAVITY_TARGETS_PER_WORKGROUP),
                         ("TSP_GRAVITY_ERROR_K", _native.GRAVITY_ERROR_K)):
        assert int(re.search(rf"^#define {macro} (\d+)", header, flags=re.M).group(1)) == value
    assert _native.GRAVITY_ERROR_K <= 168          # 168 * 2^-24 = 1e-5, the project's parity tolerance
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert _native.load_library().tsp_version() >= 123


def test_design_lists_the_call_as_stateless():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "tsp_gravity_direct" in design
