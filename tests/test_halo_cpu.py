"""Halo properties without a GPU: the numpy model (halo_ref.py) against closed forms, the argument checks of topsy_amd.halos, the
exported symbols, and the conditions under which the GPU tests (test_gpu_halo.py) may hold the library to the model."""
import ctypes
import os

import numpy as np
import pytest

import halo_ref as ref

f32 = np.float32


def two_bodies(period=0.0, shift=(0.0, 0.0, 0.0)):
    pos = (np.array([[0.25, 0.5, 0.5], [0.75, 0.5, 0.5]]) * 0.1 + 0.3 + np.asarray(shift)).astype(f32)
    return dict(pos=pos, vel=np.array([[0, 1, 0], [0, -3, 0]], dtype=f32), mass=np.array([3.0, 1.0], dtype=f32),
                eps=np.array([0.03, 0.04], dtype=f32), labels=np.array([1, 1], dtype=np.int32), n_groups=1, period=period)


def test_two_bodies_potential():
    s = two_bodies()
    got = ref.potential_model(s)
    d = float(s["pos"][1, 0]) - float(s["pos"][0, 0])
    d = float(f32(d))
    e2 = [float(f32(e) * f32(e)) for e in s["eps"]]
    want = [-1.0 / np.sqrt(d * d + e2[1]), -3.0 / np.sqrt(d * d + e2[0])]
    assert np.allclose(got["phi"], want, rtol=1e-15, atol=0)
    assert np.allclose(got["scale"], np.abs(want), rtol=1e-15, atol=0)
    assert got["info"] == dict(n_members=2, n_groups_nonempty=1, pairs=2, n_skipped_groups=0, n_skipped_members=0,
                               max_extent=abs(float(s["pos"][1, 0]) - float(s["pos"][0, 0])))


def test_two_bodies_properties():
    s = two_bodies()
    phi = np.array([-5.0, -1.0])
    p = ref.properties_model(s, phi=phi)
    x = s["pos"].astype(np.float64)
    sep = x[1, 0] - x[0, 0]
    assert p["count"][0] == 2 and p["mass"][0] == 4.0
    assert np.allclose(p["com"][0], (3 * x[0] + x[1]) / 4, rtol=1e-15)
    assert np.allclose(p["v_com"][0], [0, 0, 0]) and np.allclose(p["L"][0], [0, 0, -3 * 0.25 * sep - 0.75 * sep * 3], rtol=1e-14)
    assert np.allclose(p["S"][0], [3 * (sep / 4) ** 2 + (3 * sep / 4) ** 2, 0, 0, 0, 0, 0], rtol=1e-14, atol=1e-30)
    assert np.isclose(p["e_kin"][0], 0.5 * (3 * 1 + 1 * 9)) and np.isclose(p["sigma2"][0], 12.0 / 12.0)
    assert np.isclose(p["r_max"][0], 0.75 * sep, rtol=1e-14)
    # the radial order: the heavy body first (|e| = sep / 4), and it alone reaches half the mass
    assert p["i_half"][0] == 0 and np.isclose(p["r_half"][0], 0.25 * sep, rtol=1e-14)
    assert np.isnan(p["v2_max"][0]) and np.isnan(p["r_vmax"][0]) and p["i_vmax"][0] == -1          # fewer than 10 members
    assert np.isclose(p["e_pot"][0], 0.5 * (3 * -5.0 + 1 * -1.0)) and p["i_pot"][0] == 0 and np.array_equal(p["pot_pos"][0], x[0])
    # 0.5 |w|^2 + phi: 0.5 - 5 < 0 bound, 4.5 - 1 > 0 not
    assert p["n_bound"][0] == 1 and p["m_bound"][0] == 3.0


def test_member_free_label():
    s = two_bodies()
    s["n_groups"] = 3
    s["labels"] = np.array([3, 0], dtype=np.int32)
    p = ref.properties_model(s, phi=np.array([-1.0, -1.0]))
    assert list(p["count"]) == [0, 0, 1] and list(p["mass"][:2]) == [0.0, 0.0] and list(p["i_pot"]) == [-1, -1, 0]
    for k in ("com", "v_com", "S", "L", "e_kin", "r_max", "r_half", "v2_max", "e_pot", "m_bound", "pot_pos"):
        assert np.isnan(p[k][:2]).all(), k
    assert p["r_max"][2] == 0.0 and p["r_half"][2] == 0.0 and p["n_bound"][2] == 1
    pot = ref.potential_model(s)
    assert pot["phi"][0] == 0.0 and np.isnan(pot["phi"][1]) and pot["info"]["n_groups_nonempty"] == 1


def test_a_clump_and_its_image_across_a_face():
    """the same clump well inside the periodic box and straddling a face: the same properties, up to the wrap of com"""
    rs = np.random.RandomState(2)
    n = 300
    # offsets on a grid of 2^-12 around centres that are multiples of 2^-10: both copies are exact in float32
    off = np.round(rs.normal(size=(n, 3)) * 0.01 * 4096) / 4096
    base = dict(vel=rs.normal(size=(n, 3)).astype(f32), mass=rs.uniform(0.5, 1.5, n).astype(f32), eps=np.full(n, 1e-3, dtype=f32),
                labels=np.ones(n, dtype=np.int32), n_groups=1, period=1.0)
    inside = dict(base, pos=(np.array([0.5, 0.5, 0.5]) + off).astype(f32))
    across = (np.array([0.0, 0.5, 0.5]) + off)
    across = dict(base, pos=(across - np.floor(across)).astype(f32))
    assert (across["pos"][:, 0] > 0.9).any() and (across["pos"][:, 0] < 0.1).any()
    pa, pb = ref.potential_model(inside), ref.potential_model(across)
    assert np.array_equal(pa["phi"], pb["phi"])
    a, b = ref.properties_model(inside, phi=pa["phi"]), ref.properties_model(across, phi=pb["phi"])
    for k in ("count", "mass", "v_com", "S", "L", "e_kin", "r_max", "r_half", "v2_max", "r_vmax", "e_pot", "n_bound", "m_bound", "i_pot",
              "i_half", "i_vmax"):
        assert np.array_equal(a[k], b[k]), k
    shift = a["com"][0] - b["com"][0]
    want = np.array([0.5, 0.0, 0.0])                        # the copies lie half a box apart in x; com is wrapped into [0, 1)
    assert np.allclose((shift - want) - np.rint(shift - want), 0.0, atol=1e-14)
    assert (b["com"][0] >= 0).all() and (b["com"][0] < 1).all()


def test_ordered_sums_are_sums():
    rs = np.random.RandomState(1)
    for k, start in ((1, 0), (255, 1), (256, 0), (257, 255), (20000, 77)):
        t = rs.normal(size=(k, 2))
        assert np.allclose(ref.ordered_sum(t, start), t.sum(axis=0), rtol=0, atol=1e-12 * np.abs(t).sum())
        m = rs.uniform(0.5, 1.5, k)
        assert np.allclose(ref.ordered_cumsum(m, start), np.cumsum(m), rtol=1e-13)


# ---- the conditions of the GPU tests, on the model alone -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["clumps", "periodic"])
def test_scene_conditions(name):
    scene, pot, props = ref.reference(name)
    members = props["n_members"]
    assert members == sum(ref.CLUMP_SIZES) == 8610 and len(scene["pos"]) == members + ref.N_BACKGROUND
    assert props["n_energy_ambiguous"] <= 0.01 * members, "members whose binding energy float32 cannot decide"
    two = props["count"] >= 2
    assert props["pot_ambiguous"][two].sum() <= 0.1 * two.sum(), "haloes whose potential minimum float32 cannot decide"
    assert props["n_key_ambiguous"] == 0, "members whose radial key could round either way"
    big = props["count"] >= 19
    frac = props["n_bound"][big] / props["count"][big]
    print(f"\n{name}: energy-ambiguous {props['n_energy_ambiguous']}, bound fractions {frac.min():.3f} .. {frac.max():.3f}")
    assert (frac > 0.5).all() and (frac < 1.0).any(), "n_bound would test nothing"
    assert props["max_extent"] < 0.25 and pot["info"]["max_extent"] == props["max_extent"]


def test_crumbs_and_nonfinite_conditions():
    scene, pot, props = ref.reference("crumbs")
    assert (props["count"][-5:] == 0).all() and (props["count"][:3000] >= 1).all() and props["count"].max() == 3
    assert props["n_key_ambiguous"] == 0
    scene, pot, props = ref.reference("nonfinite")
    clean = ref.reference("clumps")[2]
    # x, y, z, mass (properties and potential), eps (potential only), vx, vy, vz (properties only): one member each
    assert props["n_members"] == clean["n_members"] - 7 and pot["info"]["n_members"] == clean["n_members"] - 5
    assert props["n_key_ambiguous"] == 0
    assert (props["n_bound"] == -1).sum() == 1 and np.isnan(props["e_pot"]).sum() == 1      # the halo whose member has no eps: NaN phi


# ---- the argument checks ----------------------------------------------------------------------------------------------------------
def test_argument_checks():
    import topsy_amd
    from topsy_amd import halos
    from topsy_amd.loader import FofCatalogue
    pos, mass, lab = np.zeros((4, 3)), np.ones(4), np.array([1, 1, 0, 2])
    for bad in (np.zeros((4, 2)), np.zeros(4), np.zeros((0, 3)), np.array([["a"] * 3] * 4)):
        with pytest.raises(ValueError):
            halos.check_positions(bad)
    with pytest.raises(ValueError):
        halos.check_mass(np.ones(3), 4)
    for bad in (np.ones(4), np.ones(4, dtype=bool), np.ones(3, dtype=int), np.zeros(4, dtype=int), np.array([1, 2 ** 40, 0, 0])):
        with pytest.raises(ValueError):
            halos.check_group(bad, 4)
    labels, n_groups = halos.check_group(lab, 4)
    assert labels.dtype == np.int32 and n_groups == 2
    assert halos.check_group(FofCatalogue(lab), 4)[1] == 2
    with pytest.raises(ValueError):
        halos.check_group(FofCatalogue(np.zeros(4, dtype=int)), 4)
    for bad in (np.zeros((4, 2)), np.zeros((3, 3))):
        with pytest.raises(ValueError):
            halos.check_vel(bad, 4)
    with pytest.raises(ValueError):
        halos.check_phi(np.zeros(3), 4)
    for bad in (0, -1.0, np.inf, np.nan, "box"):
        with pytest.raises(ValueError):
            halos.check_period(bad)
    assert halos.check_period(None) == 0.0 and halos.check_period(2) == 2.0
    for bad in (0, -3, 1.5, True, "many"):
        with pytest.raises(ValueError):
            halos.check_tree_above(bad)
    from topsy_amd import config
    assert halos.check_tree_above(None) == config.HALO_TREE_MEMBERS and halos.check_tree_above(7) == 7
    # the public functions refuse before they need a GPU
    for kw in (dict(eps=-1.0), dict(eps=None), dict(G=0), dict(theta=2), dict(periodicity_scale=-1), dict(tree_above=0)):
        with pytest.raises(ValueError):
            topsy_amd.group_potential(pos, mass, **({"eps": 0.1} | kw), group=lab)
    for kw in (dict(vel=np.zeros((4, 2))), dict(phi=np.zeros(5)), dict(eps=[0.1]), dict(G=np.nan), dict(periodicity_scale=0)):
        with pytest.raises(ValueError):
            topsy_amd.halo_properties(pos, mass, lab, **kw)
    with pytest.raises(ValueError):
        topsy_amd.halo_properties(pos, mass, np.zeros(4, dtype=int))
    with pytest.warns(RuntimeWarning):
        halos.warn_extent(0.3, 1.0)


def test_halo_properties_names_the_columns():
    from topsy_amd import _native, halos
    H = 3
    props = np.arange(H * _native.HALO_NPROPS, dtype=np.float64).reshape(H, -1)
    props[1] = np.nan
    c = _native.HALO_COLUMNS
    props[0, c["S"]:c["S"] + 6] = [4, 0, 0, 1, 0, 0.25]
    raw = dict(count=np.array([5, 0, 7]), n_bound=np.array([3, -1, 7]), i_pot=np.array([2, -1, 9]), props=props)
    h = halos.HaloProperties(raw, G=4.0, phi=np.zeros(1))
    assert len(h) == 3 and h.mass[0] == 0 and np.array_equal(h.com[0], [1, 2, 3]) and np.array_equal(h.L[2], props[2, 13:16])
    assert np.allclose(h.axis_ratios[0], [0.5, 0.25]) and np.isnan(h.axis_ratios[1]).all()
    assert np.isclose(h.v_max[2], np.sqrt(4.0 * props[2, c["v2_max"]])) and h.i_half[1] == -1 and h.i_half[2] == int(props[2, c["i_half"]])
    assert np.array_equal(h.S[0], np.diag([4, 1, 0.25])) and h.n_bound[2] == 7
    assert np.isclose(h.virial_ratio[2], 2 * props[2, c["e_kin"]] / props[2, c["e_pot"]])
    assert halos.HaloProperties(raw).e_pot is None


def test_exported_symbols_and_version():
    from topsy_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(lib, "tsp_group_potential") and hasattr(lib, "tsp_halo_properties")
    assert _native.load_library().tsp_version() >= 125 and _native.ABI_VERSION == 112
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "topsy_splat.h")).read()
    for name, col in _native.HALO_COLUMNS.items():
        define = {"v_com": "VCOM", "e_kin": "EKIN", "e_pot": "EPOT", "r_max": "RMAX", "r_half": "RHALF", "v2_max": "V2MAX", "r_vmax": "RVMAX",
                  "m_bound": "MBOUND", "pot_pos": "POTPOS", "i_half": "IHALF", "i_vmax": "IVMAX"}.get(name, name.upper())
        assert f"#define TSP_HALO_{define} {col} " in header or f"#define TSP_HALO_{define} {col}\n" in header, name
    assert f"#define TSP_HALO_NPROPS {_native.HALO_NPROPS}\n" in header
    assert ctypes.sizeof(_native.GroupPotentialInfo) == 56 and ctypes.sizeof(_native.HaloInfo) == 16
