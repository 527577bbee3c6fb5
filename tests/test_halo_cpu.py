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
    for k, start in ((1, 0), (255, 1), (256, 0), (257, 255), (20000, 77), (32769, 0)):
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


@pytest.mark.parametrize("name", ["clumps", "periodic"])
def test_sampled_potential_model_gives_the_full_models_bits(name):
    scene, full, _ = ref.reference(name)
    targets = ref.target_sample(scene, 4, seed=1)
    part = ref.potential_model(scene, targets=targets)
    assert len(targets) >= 4 * 17 and np.array_equal(part["targets"], targets)
    for k in ("phi", "scale"):
        assert np.array_equal(part[k][targets].view(np.uint64), full[k][targets].view(np.uint64)), k
    rest = np.setdiff1d(np.arange(len(scene["pos"])), targets)
    assert np.isnan(part["phi"][rest]).all() and (part["scale"][rest] == 0).all()
    assert part["info"] == full["info"] and np.array_equal(part["counts"], full["counts"])
    assert np.array_equal(part["member_has_value"], full["member_has_value"])
    assert np.array_equal(full["member_has_value"], ~np.isnan(full["phi"])), "the NaN pattern of the whole array"
    skip = ref.potential_model(scene, max_members=1000, targets=targets)
    assert np.array_equal(skip["member_has_value"], ~np.isnan(ref.potential_model(scene, max_members=1000)["phi"]))


def layout(scene):
    """(sorted position of every particle or -1, starts, counts) of the potential's members"""
    index, starts, counts = ref.sorted_positions(scene)
    where = np.full(len(scene["pos"]), -1, dtype=np.int64)
    where[index] = np.arange(len(index))
    return where, starts, counts


@pytest.mark.parametrize("name", ["edges", "edges+1", "giants", "legion"])
def test_target_sample_holds_every_edge_class(name):
    scene = ref.reference(name)[0]
    targets = ref.reference(name)[1]["targets"] if name in ref.SAMPLED else ref.target_sample(scene, 4, seed=1)
    where, starts, counts = layout(scene)
    p = where[targets]
    assert (p >= 0).all() and len(np.unique(targets)) == len(targets)
    assert np.isin(starts, p).all() and np.isin(starts + counts - 1, p).all(), "every halo's first and last sorted member"
    for modulus, residues in ((1024, (0, 255, 256, 1023)), (512, (0, 511))):
        for r in residues:
            assert (p % modulus == r).sum() >= 3, f"sorted positions = {r} mod {modulus}"
    per_halo = np.bincount(scene["labels"][targets], minlength=scene["n_groups"] + 1)[1:]
    assert (per_halo >= np.minimum(counts, ref.SAMPLED.get(name, 4))).all()
    if name in ref.SAMPLED:
        assert 500 <= len(targets) <= ref.MAX_TARGETS
    if name == "legion":       # the blocks of the second launch have targets of every class of lane plane and tile edge
        block0 = ref.work_items(counts)["launches"][1][0]
        late = p[p >= block0 * 1024]
        assert len(late) >= 50 and {0, 255, 256, 1023} <= set(late % 1024) and {0, 511} <= set(late % 512)


@pytest.mark.parametrize("name", ["edges", "edges+1"])
def test_edges_layout(name):
    scene, pot, props = ref.reference(name)
    extra = int(name == "edges+1")
    counts = props["count"]
    assert list(counts) == list(ref.EDGE_SIZES[:-1]) + [ref.EDGE_SIZES[-1] + extra] and np.array_equal(pot["counts"], counts)
    ends = np.cumsum(counts)
    starts = ends - counts
    lay = [ref.piece_layout(int(s), int(c)) for s, c in zip(starts, counts)]
    H = len(counts)
    assert any(g > 0 and starts[g] % 256 == 0 and lay[g][0] == 0 for g in range(H)), "a later halo that starts a slice"
    assert any(ends[g] % 256 == 0 for g in range(H - 1)), "a halo that ends a slice"
    assert any(g > 0 and counts[g] == 256 and starts[g] % 256 == 0 and lay[g] == (0, 1, 1, 1) for g in range(H)), "one aligned slice"
    one_b = [g for g in range(H) if counts[g] == 256 and starts[g] % 256 == 255]
    assert one_b and lay[one_b[0]] == (1, 2, 1, 2) and ref._pieces(256, int(starts[one_b[0]]))[0] == (0, 1), "a B piece of one member"
    singles = [g for g in range(H - 2) if (counts[g:g + 3] == 1).all() and starts[g + 1] % 256 in (0, 255)]
    assert singles, "three one-member haloes across a slice boundary"
    assert 10 in counts and 9 in counts
    ten, nine = list(counts).index(10), list(counts).index(9)
    assert props["v2_max"][ten] > 0 and props["i_vmax"][ten] >= 0 and np.isnan(props["v2_max"][nine]) and props["i_vmax"][nine] == -1
    assert any(ends[g] % 1024 == 0 and starts[g + 1] == ends[g] for g in range(H - 1)), "a halo that ends a block"
    assert any(counts[g] == 1024 and starts[g] % 1024 == 0 for g in range(H)), "a halo that is exactly one block"
    assert props["n_members"] == pot["info"]["n_members"] == ends[-1] and ends[-1] % 512 == extra
    assert len(scene["pos"]) == ends[-1] + ref.N_BACKGROUND_BIG and set(scene["labels"][scene["labels"] < 1]) == {0, -1, -7}
    assert props["n_key_ambiguous"] == 0, "members whose radial key could round either way"


def test_giants_conditions():
    scene, pot, props = ref.reference("giants")
    counts = props["count"]
    assert list(counts) == list(ref.GIANT_SIZES) and np.array_equal(pot["counts"], counts)
    starts = np.cumsum(counts) - counts
    lay = {name: ref.piece_layout(int(starts[g - 1]), int(counts[g - 1])) for name, g in ref.GIANT_LABELS.items()}
    assert lay == dict(aligned_16384=(0, 64, 1, 64), misaligned_16384=(1, 65, 2, 33), aligned_32768=(0, 128, 2, 64),
                       aligned_32769=(0, 129, 3, 43))
    assert props["n_key_ambiguous"] == 0, "members whose radial key could round either way"
    # the bound fraction, at the sampled members (the potential of every member of a giant is out of the model's reach)
    t = pot["targets"]
    g = scene["labels"][t] - 1
    w = scene["vel"][t].astype(np.float64) - props["v_com"][g]
    bound = 0.5 * (w * w).sum(axis=1) + pot["phi"][t] < 0.0
    frac = np.array([bound[g == k - 1].mean() for k in ref.GIANT_LABELS.values()])
    print(f"\ngiants: bound fractions of the sampled members {frac}")
    assert (frac > 0.5).all() and (frac < 1.0).any(), "n_bound would test nothing"
    assert pot["info"]["max_extent"] == props["max_extent"] and pot["info"]["n_members"] == sum(ref.GIANT_SIZES) == 98561
    # every block of a giant has the 16 work items of the cap, in one launch
    w = ref.work_items(counts)
    assert len(w["launches"]) == 1 and (w["splits_per_block"] == 16).all()


def test_legion_conditions():
    scene, pot, _ = ref.reference("legion")
    counts = pot["counts"]
    assert list(counts) == list(ref.LEGION_SIZES) and (counts[len(ref.GIANT_SIZES):] >= 15872).all()
    assert (counts[len(ref.GIANT_SIZES):] % 256 != 0).all() and len(set(counts)) == len(counts) - 1       # (16384 twice)
    w = ref.work_items(counts)
    items = np.array(w["items"])
    print(f"\nlegion: {pot['info']['n_members']} members, {len(items)} work items, launches {w['launches']}")
    assert len(items) > 4096 and len(w["launches"]) >= 2 and sum(l[2] for l in w["launches"]) == len(items)
    assert all(l[2] <= 4096 for l in w["launches"]) and w["launches"][0][1] == w["launches"][1][0]
    index, starts, _ = ref.sorted_positions(scene)
    p = w["launches"][1][0] * 1024
    lab = scene["labels"][index]                                                # the labels by sorted position
    assert 0 < p < len(lab) and lab[p - 1] == lab[p] and p not in starts, "the launch break falls between two haloes"
    # the slots restart in every launch, and a block's items are consecutive slots
    for b0, b1, n_items in w["launches"]:
        sel = (items[:, 0] >= b0) & (items[:, 0] < b1)
        assert np.array_equal(items[sel, 3], np.arange(n_items))
    tiles = np.array([items[items[:, 0] == b, 2].max() - items[items[:, 0] == b, 1].min() for b in range(len(w["splits_per_block"]))])
    assert ((w["splits_per_block"] == 16) & (tiles % 16 != 0)).any(), "no block at the cap has items of unequal length"
    assert (tiles >= 31).all() and len(set(items[:, 2] - items[:, 1])) >= 3
    assert np.array_equal(np.bincount(items[:, 0]), w["splits_per_block"]) and (items[:, 2] > items[:, 1]).all()
    assert w["pair_slots"] == (items[:, 2] - items[:, 1]).sum() * 512 * 1024
    skip = ref.work_items(counts, ref.LEGION_MAX_MEMBERS)
    none = np.flatnonzero(skip["splits_per_block"] == 0)
    assert len(none) and (skip["splits_per_block"][:none[0]] > 0).any() and (skip["splits_per_block"][none[-1] + 1:] > 0).any()
    model = ref.potential_model(scene, ref.LEGION_MAX_MEMBERS, targets=pot["targets"][:1])
    assert model["info"]["n_skipped_groups"] == 2 and model["info"]["n_skipped_members"] == 32768 + 32769


def test_work_items_of_single_haloes():
    """the pair slots that the contract states outright: blocks x tiles of the block's range x 512 x 1024"""
    w = ref.work_items([2048])
    assert w["pair_slots"] == 2 * 4 * 512 * 1024 and w["launches"] == [(0, 2, 4)] and list(w["splits_per_block"]) == [2, 2]
    assert w["items"] == [(0, 0, 2, 0), (0, 2, 4, 1), (1, 0, 2, 2), (1, 2, 4, 3)]
    assert ref.work_items([1])["pair_slots"] == 512 * 1024 and ref.work_items([1])["items"] == [(0, 0, 1, 0)]
    assert ref.work_items([513])["items"] == [(0, 0, 2, 0)] and ref.work_items([1025])["pair_slots"] == 2 * 3 * 512 * 1024
    assert ref.work_items([0, 0, 0])["items"] == [] and ref.work_items([0])["launches"] == []
    # one halo of 16384: 16 blocks of 32 tiles, 16 items of 2 tiles each; of 16385: 17 blocks of 33 tiles, items of 2 and 3 tiles
    w = ref.work_items([16384])
    assert w["pair_slots"] == 16 * 32 * 512 * 1024 and len(w["items"]) == 256 and {b - a for _, a, b, _ in w["items"]} == {2}
    w = ref.work_items([16385])
    assert len(w["items"]) == 17 * 16 and {b - a for _, a, b, _ in w["items"]} == {2, 3}
    assert [a for blk, a, _, _ in w["items"] if blk == 0] == [33 * s // 16 for s in range(16)]
    # a skipped halo has no items and is left out of its neighbours' ranges
    w = ref.work_items([100, 5000, 100], max_members=1000)
    assert list(w["splits_per_block"]) == [1, 0, 0, 0, 1, 1] and w["items"] == [(0, 0, 1, 0), (4, 9, 11, 1), (5, 9, 11, 2)]
    assert ref.piece_layout(0, 0) == (0, 0, 0, 0) and ref.piece_layout(5, 1) == (1, 1, 1, 1) and ref.piece_layout(255, 2) == (1, 2, 1, 2)


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
