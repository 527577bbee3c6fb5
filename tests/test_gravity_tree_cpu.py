"""Tree gravity without a GPU: the float64 host model (tree_gravity_ref.py) against the direct sum and the quality caps the GPU
test holds the kernel to, the host layer's argument checks, the stand-alone layout arithmetic, and the header against the binding."""
import os
import re

import numpy as np
import pytest

import gravity_ref
import tree_gravity_ref
import tree_gravity_scenes as scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


# ---- the model ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("self_targets", [True, False])
def test_model_with_theta_zero_is_the_direct_sum(self_targets):
    src, mass, eps, tgt = scenes.scene(32 * 64 + 7, 129)
    src[5, 0], mass[40], eps[900] = np.nan, np.inf, np.nan
    mass[[3, 77]] = 0.0
    tgt[17, 2] = np.inf
    targets = None if self_targets else tgt
    got = tree_gravity_ref.tree_sum(src, mass, eps, targets, theta=0.0)
    ref = gravity_ref.direct_sum(src, mass, eps, targets)
    assert np.array_equal(np.isnan(got["pot"]), np.isnan(ref["pot"]))
    ok = ~np.isnan(ref["pot"])
    assert np.abs(got["pot"][ok] - ref["pot"][ok]).max() <= 1e-12 * ref["pot_scale"][ok].max()
    assert (np.abs(got["acc"][ok] - ref["acc"][ok]) <= 1e-12 * ref["acc_scale"][ok]).all()
    n_sorted = len(src) - 1                              # the source with the NaN coordinate is not in the tree
    k = int(ok.sum())
    assert got["pairs_node"] == 0 and got["pairs_direct"] == n_sorted * k - (k if self_targets else 0)
    assert got["n_valid_sources"] == ref["n_valid_sources"] == len(src) - 3


def test_model_moments_follow_the_parallel_axis_rule():
    """every node's M, c and Q, built level by level, equal the sums over its particles"""
    src, mass, eps, _ = scenes.scene(32 * 8 * 3 + 11, 1, seed=2)
    tree = tree_gravity_ref.build_tree(src, mass, eps)
    width = tree_gravity_ref.LEAF
    for level in tree["levels"]:
        for k in (0, len(level["M"]) - 1):
            lo, hi = k * width, min((k + 1) * width, len(tree["m"]))
            m, x = tree["m"][lo:hi], tree["pos"][lo:hi]
            c = (m[:, None] * x).sum(axis=0) / m.sum()
            d = x - c
            assert level["M"][k] == pytest.approx(m.sum(), rel=1e-13) and level["c"][k] == pytest.approx(c, rel=1e-13)
            want_q = [(m * d[:, a] * d[:, b]).sum() for a, b in tree_gravity_ref._PAIRS]
            assert level["Q"][k] == pytest.approx(want_q, rel=1e-9, abs=1e-12 * m.sum())
            assert level["b"][k] >= np.linalg.norm(d, axis=1).max() * (1 - 1e-12)
        width *= tree_gravity_ref.FANOUT
    assert len(tree["levels"][-1]["M"]) == 1


def test_node_term_is_the_expansion_to_second_order():
    """two softened point masses seen from far away: the node term differs from their sum by the third order only"""
    x = np.array([[0.3, -0.1, 0.2], [-0.2, 0.15, -0.1]])
    m = np.array([2.0, 3.0])
    e2 = 0.04
    c = (m[:, None] * x).sum(axis=0) / m.sum()
    d = x - c
    Q = np.array([[(m * d[:, a] * d[:, b]).sum() for a, b in tree_gravity_ref._PAIRS]])
    errors = []
    for r in (10.0, 20.0):
        t = c + r * np.array([0.6, 0.0, 0.8])
        pot, acc = tree_gravity_ref.node_terms((t - c)[None, :], m.sum()[None], np.array([e2]), Q)
        dd = t - x
        r2 = (dd * dd).sum(axis=1) + e2
        want_pot, want_acc = (m / np.sqrt(r2)).sum(), ((m * r2 ** -1.5)[:, None] * dd).sum(axis=0)
        errors.append((abs(pot[0] / want_pot - 1.0), np.linalg.norm(acc[0] - want_acc) / np.linalg.norm(want_acc)))
    assert errors[0][0] < 1e-5 and errors[0][1] < 1e-4
    assert errors[1][0] < errors[0][0] / 6 and errors[1][1] < errors[0][1] / 6         # third order: a factor 8 per doubling of r


@pytest.mark.parametrize("name", ["plummer", "wide_eps", "clumps_and_outlier"])
def test_model_meets_the_caps_with_room(name):
    """theta = 0.5: the host model stays at or below a third of the caps the GPU test asserts, on the same scenes and targets"""
    model = scenes.model_quality(name, 0.5)
    print(f"\n{name}: host model at theta = 0.5: p99(e) = {model['p99']:.3e}, max(e) = {model['max']:.3e}, "
          f"{model['pairs_per_target']:.0f} terms per target")
    assert model["p99"] <= scenes.CAP_P99 / 3 and model["max"] <= scenes.CAP_MAX / 3
    if name != "clumps_and_outlier":
        loose, tight = scenes.model_quality(name, 0.8), scenes.model_quality(name, 0.3)
        assert tight["p99"] <= model["p99"] <= loose["p99"]
        assert tight["pairs_per_target"] > model["pairs_per_target"] > loose["pairs_per_target"]


def test_model_prunes():
    """uniform cube of 65536, theta = 0.5: the model's term count is below n^2 / 4.  A target's count does not depend on the
    other targets, so the total is n times the mean over the targets; the mean is taken over 2048 targets drawn uniformly."""
    src, mass, eps = scenes.uniform_cube()
    n = len(src)
    rows = np.sort(np.random.RandomState(4).choice(n, 2048, replace=False))
    got = tree_gravity_ref.tree_sum(src, mass, eps, None, theta=0.5, rows=rows)
    per_target = got["per_target_pairs"][rows]
    print(f"\nuniform cube, n = {n}: the host model evaluates {per_target.mean():.0f} terms per target (max {per_target.max()})")
    assert per_target.max() < n / 4 and (got["pairs_direct"] + got["pairs_node"]) * (n / len(rows)) < n * n / 4


# ---- the model with the kernel's group decisions and stored records ---------------------------------------------------------------------
def _same_sums(got, want, ref):
    assert np.array_equal(np.isnan(got["pot"]), np.isnan(want["pot"])) and np.array_equal(np.isnan(got["acc"]), np.isnan(want["acc"]))
    ok = ~np.isnan(want["pot"])
    assert (np.abs(got["pot"][ok] - want["pot"][ok]) <= 1e-12 * ref["pot_scale"][ok]).all()
    assert (np.abs(got["acc"][ok] - want["acc"][ok]) <= 1e-12 * ref["acc_scale"][ok]).all()
    assert (got["pairs_direct"], got["pairs_node"]) == (want["pairs_direct"], want["pairs_node"])
    assert np.array_equal(got["per_target_pairs"], want["per_target_pairs"])


@pytest.mark.parametrize("self_targets", [True, False])
def test_group_model_reproduces_the_single_target_model(self_targets):
    """theta = 0 (any groups, stored or not), and one target per group with the unrounded records: today's tree_sum"""
    src, mass, eps, tgt = scenes.scene(32 * 64 + 7, 129)
    src[5, 0], mass[40], eps[900] = np.nan, np.inf, np.nan
    mass[[3, 77]] = 0.0
    tgt[17, 2] = np.inf
    targets = None if self_targets else tgt
    ref = gravity_ref.direct_sum(src, mass, eps, targets)
    k = len(src) if self_targets else len(tgt)
    for stored in (False, True):
        tree = tree_gravity_ref.build_tree(src, mass, eps, stored=stored)
        groups = tree_gravity_ref.sorted_groups(tree) if self_targets else tree_gravity_ref.consecutive_groups(k)
        want = tree_gravity_ref.tree_sum(src, mass, eps, targets, theta=0.0)
        got = tree_gravity_ref.tree_sum(src, mass, eps, targets, theta=0.0, tree=tree, groups=groups)
        _same_sums(got, want, ref)
        assert got["pairs_node"] == 0
        # the scales of the pair terms are the direct sum's
        ok = ~np.isnan(ref["pot"])
        assert got["pot_scale"][ok] == pytest.approx(ref["pot_scale"][ok], rel=1e-12)
        assert got["acc_scale"][ok] == pytest.approx(ref["acc_scale"][ok], rel=1e-12)
    finite = np.nonzero(np.isfinite(src if self_targets else tgt).all(axis=1))[0]
    for theta in (0.5, 1.0):
        want = tree_gravity_ref.tree_sum(src, mass, eps, targets, theta=theta)
        got = tree_gravity_ref.tree_sum(src, mass, eps, targets, theta=theta, groups=[[i] for i in range(k)])
        assert want["pairs_node"] > 0
        _same_sums(got, want, ref)
        assert [len(g["targets"]) for g in got["groups"]] == [int(i in finite) for i in range(k)]


def test_stored_records_are_the_kernels_roundings():
    src, mass, eps, _ = scenes.scene(32 * 8 * 3 + 11, 1, seed=2)
    plain = tree_gravity_ref.build_tree(src, mass, eps)
    tree = tree_gravity_ref.build_tree(src, mass, eps, stored=True)
    up = np.float32(1.0) + np.float32(2.0 ** -20)
    for level, plain_level, raw, rec in zip(tree["levels"], plain["levels"], plain["walk"], tree["walk"]):
        for name in ("M", "c", "Q", "lo", "hi", "rule", "b"):
            assert np.array_equal(level[name], plain_level[name])                                    # parents: from unrounded sums
        for name in ("c", "M", "e2", "Q"):
            assert np.array_equal(rec[name], raw[name].astype(f32).astype(np.float64))
        far = np.maximum(rec["c"] - level["lo"], level["hi"] - rec["c"])
        radius = np.sqrt((far * far).sum(axis=1))                                                    # from the float32 c
        assert np.array_equal(rec["b"], (radius.astype(f32) * up).astype(np.float64))
        assert (rec["b"] >= radius).all() and (rec["b"] <= radius * (1 + 2.0 ** -19)).all()           # never below it
        positive = raw["rule"] > 0
        assert positive.any() and np.array_equal(rec["rule"][positive], (raw["rule"][positive].astype(f32) * up).astype(np.float64))
        assert (rec["rule"][~positive] == 0).all()


@pytest.mark.parametrize("size", list(scenes.CELL_SIZES))
def test_cell_scene_is_sorted_by_its_coarse_cells(size):
    g, n = scenes.CELL_SIZES[size]
    for eps_name in scenes.CELL_EPS:
        src, mass, eps, cells = scenes.term_scene(size, eps_name)
        tree = scenes.term_tree(size, eps_name)
        assert len(tree["levels"]) == int(size[0]) and len(src) == n
        keys = scenes.cell_keys(cells)
        assert len(np.unique(keys)) == n, "two particles share a cell"
        assert np.array_equal(tree["order"], np.argsort(keys, kind="stable"))
        frac = src.astype(np.float64) * g - cells
        inner = np.ones(n, dtype=bool)
        inner[tree["order"][[0, -1]]] = False
        assert (frac[inner] >= 0.25 - 1e-5).all() and (frac[inner] <= 0.75 + 1e-5).all()
        assert (src[tree["order"][0]] == 0).all() and (src[tree["order"][-1]] == 1).all()
        assert mass.max() / mass.min() > 50 and (np.ndim(eps) == 0 or eps.max() / eps.min() > 500)
        Q = tree["levels"][-1]["Q"][0]
        assert (np.abs(Q) > 1e-3 * Q[:3].max()).all() and np.abs(np.diff(np.sort(np.abs(Q)))).min() > 1e-3 * Q[:3].max()


TERM_CASES = [(size, eps_name, theta, self_targets) for size in scenes.CELL_SIZES for eps_name in scenes.CELL_EPS
              for self_targets, thetas in ((False, scenes.TERM_THETAS), (True, scenes.SELF_THETAS)) for theta in thetas]


@pytest.mark.parametrize("size, eps_name, theta, self_targets", TERM_CASES)
def test_term_cases_meet_their_conditions(size, eps_name, theta, self_targets):
    """what the GPU test requires of every case before it compares: at most a tenth of the groups within 1e-4 of a threshold, nodes
    accepted on three levels (two where the 4-level scene's geometry allows no more: tree_gravity_scenes.min_levels)"""
    model = scenes.term_model(size, eps_name, theta, self_targets)
    amb, levels = scenes.check_case_conditions(model, (size, eps_name, theta, self_targets), scenes.min_levels(size, theta, self_targets))
    print(f"\n{size}, {eps_name}, theta = {theta}, self = {self_targets}: {int(amb.sum())} of {len(amb)} groups ambiguous, nodes "
          f"accepted on levels {levels.tolist()}: {model['accepted_per_level'].tolist()}")
    if np.ndim(scenes.term_scene(size, eps_name)[2]):      # eps varies: the second rule decides somewhere
        tree = scenes.term_tree(size, eps_name)
        assert any((rec["rule"] > 0).any() for rec in tree["walk"])


def test_model_at_huge_softening_is_the_closed_form():
    """eps = 1e5: every term is m / eps, so pot_i = -(M - m_i) / eps however the tree partitions the sources -- the model (theta =
    1, the kernel's groups) meets that and the direct sum within 0.01 * 2^-24"""
    g, n = scenes.CELL_SIZES["4 levels"]
    src, mass, _, _ = scenes.cell_scene(g, n, 41, 0.01)
    eps = scenes.PARTITION_EPS
    tree = tree_gravity_ref.build_tree(src, mass, eps)
    got = tree_gravity_ref.tree_sum(src, mass, eps, None, theta=1.0, tree=tree, groups=tree_gravity_ref.sorted_groups(tree))
    assert got["pairs_node"] > 0 and got["pairs_direct"] + got["pairs_node"] < n * n / 2
    m = mass.astype(np.float64)
    tol = 0.01 * 2.0 ** -24
    assert np.abs(got["pot"] * eps / -(m.sum() - m) - 1.0).max() <= tol
    ref = gravity_ref.direct_sum(src, mass, eps)
    assert (np.abs(got["pot"] - ref["pot"]) <= tol * ref["pot_scale"]).all()
    assert (np.abs(got["acc"] - ref["acc"]) <= tol * ref["acc_scale"]).all()


@pytest.mark.parametrize("size", list(scenes.CELL_SIZES))
@pytest.mark.parametrize("mutation", ["Qxy and Qxz swapped", "no parallel-axis term"])
def test_term_bound_notices_a_wrong_moment(size, mutation):
    """a fault put into the MODEL's tree moves its sums by more than 100 times the bound the GPU test asserts, in a group that is
    not ambiguous: the assertion of test_gpu_gravity_tree_terms.py has teeth"""
    from topsy_amd import _native
    eps_name, theta = "eps over three decades", 0.8
    src, mass, eps, _ = scenes.term_scene(size, eps_name)
    model = scenes.term_model(size, eps_name, theta, False)
    tgt, groups = scenes.term_targets()
    if mutation == "no parallel-axis term":
        wrong = tree_gravity_ref.build_tree(src, mass, eps, stored=True, parallel_axis=False)
    else:
        wrong = dict(scenes.term_tree(size, eps_name))
        wrong["walk"] = [dict(rec, Q=rec["Q"][:, [0, 1, 2, 4, 3, 5]]) for rec in wrong["walk"]]
    got = tree_gravity_ref.tree_sum(src, mass, eps, tgt, theta=theta, tree=wrong, groups=groups)
    assert (got["pairs_direct"], got["pairs_node"]) == (model["pairs_direct"], model["pairs_node"])      # the same decisions
    ratios = scenes.group_ratios(got["pot"], got["acc"], model)[~scenes.ambiguous(model)]
    print(f"\n{size}, {mutation}: the model moves by up to {ratios.max():.0f} x 2^-24 scale (bound {_native.GRAVITY_TREE_ERROR_K})")
    assert ratios.max() > 100 * _native.GRAVITY_TREE_ERROR_K


# ---- the host layer -------------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    import topsy_amd
    from topsy_amd import gravity
    assert gravity.check_theta(0) == 0.0 and gravity.check_theta(1) == 1.0 and gravity.check_theta(np.float32(0.5)) == 0.5
    for bad in (-0.01, 1.5, float("nan"), float("inf"), "wide", None):
        with pytest.raises(ValueError, match="theta"):
            gravity.check_theta(bad)
    assert gravity.check_method("tree") == "tree" and gravity.check_method("direct") == "direct"
    with pytest.raises(ValueError, match="method must be 'direct' or 'tree'"):
        gravity.check_method("fmm")
    gravity.check_tree_masses(np.array([0.0, 1.0, np.nan], dtype=f32))
    with pytest.raises(ValueError, match=r"masses >= 0: mass\[1\]"):
        gravity.check_tree_masses(np.array([0.0, -1.0, 2.0], dtype=f32))
    pos = np.zeros((4, 3))
    # every check comes before any GPU work: these raise here, where there is no GPU
    with pytest.raises(ValueError, match="theta"):
        topsy_amd.gravity_tree(pos, np.ones(4), 0.1, theta=1.5)
    with pytest.raises(ValueError, match="masses >= 0"):
        topsy_amd.gravity_tree(pos, [1, 1, -1, 1], 0.1)
    with pytest.raises(ValueError, match="method"):
        topsy_amd.rotation_curve(pos, np.ones(4), 0.1, [1.0], method="fmm")
    with pytest.raises(ValueError, match="theta"):
        topsy_amd.rotation_curve(pos, np.ones(4), 0.1, [1.0], method="tree", theta=-1)
    with pytest.raises(ValueError, match="masses >= 0"):
        topsy_amd.rotation_curve(pos, [1, 1, -1, 1], 0.1, [1.0], method="tree")


def _loader(**kw):
    from topsy_amd.loader import ArrayDataLoader
    rs = np.random.RandomState(5)
    n = 50
    kw = {"quantities": {"temp": np.ones(n)}} | kw
    return ArrayDataLoader(pos=rs.normal(size=(n, 3)), smooth=np.full(n, 0.1), mass=np.ones(n), **kw)


class _StubContext:
    def __init__(self):
        self.calls = []

    def gravity_tree(self, sx, sy, sz, mass, eps, targets=None, theta=0.5, want_pot=True, want_acc=True):
        self.calls.append({"n": len(sx), "theta": theta, "targets": targets, "want_acc": want_acc})
        return np.arange(len(sx), dtype=np.float64), None, {}

    def gravity_direct(self, *args, **kw):
        raise AssertionError("the direct sum was called")


def test_loader_gravity_argument(monkeypatch):
    from topsy_amd import config
    with pytest.raises(ValueError, match="gravity must be 'direct' or 'tree'"):
        _loader(eps=0.05, gravity="fmm")
    with pytest.raises(ValueError, match="theta"):
        _loader(eps=0.05, gravity="tree", gravity_theta=2.0)
    # the names are what they were, with and without the new arguments
    assert _loader().get_quantity_names() == ["temp", "rho"]
    assert _loader(eps=0.05).get_quantity_names() == _loader(eps=0.05, gravity="tree").get_quantity_names() == ["temp", "rho", "phi"]
    assert _loader(eps=0.05, vel=np.zeros((50, 3))).get_quantity_names() == ["temp", "rho", "v_div", "vorticity", "phi"]
    monkeypatch.setattr(config, "GRAVITY_DIRECT_MAX_PAIRS", 2499)
    with pytest.raises(ValueError, match=r"50 x 50 = 2.5e\+03 pairs.*GRAVITY_DIRECT_MAX_PAIRS = 2.5e\+03"):
        _loader(eps=0.05).get_named_quantity("phi")
    with pytest.raises(ValueError, match="GRAVITY_DIRECT_MAX_PAIRS"):
        _loader(eps=0.05, gravity="direct", gravity_theta=0.3).get_named_quantity("phi")
    # the tree is past the limit: it reaches the context
    ld = _loader(eps=0.05, gravity="tree", gravity_theta=0.3)
    stub = _StubContext()
    ld.set_density_context(stub)
    phi = ld.get_named_quantity("phi")
    assert stub.calls == [{"n": 50, "theta": 0.3, "targets": None, "want_acc": False}]
    assert phi.dtype == f32 and np.array_equal(phi, np.arange(50, dtype=f32))
    # ... and a negative mass is refused before it
    from topsy_amd.loader import ArrayDataLoader
    mass = np.ones(50)
    mass[7] = -1.0
    bad = ArrayDataLoader(pos=np.zeros((50, 3)), smooth=np.full(50, 0.1), mass=mass, eps=0.05, gravity="tree")
    bad.set_density_context(_StubContext())
    with pytest.raises(ValueError, match="masses >= 0"):
        bad.get_named_quantity("phi")


def test_from_arrays_and_visualizer_signatures_keep_their_defaults():
    import inspect
    import topsy_amd
    from topsy_amd import visualizer
    sig = inspect.signature(topsy_amd.from_arrays).parameters
    assert sig["gravity"].default == "direct" and sig["gravity_theta"].default == 0.5
    for fn in (topsy_amd.rotation_curve, visualizer.Visualizer.rotation_curve):
        sig = inspect.signature(fn).parameters
        assert sig["method"].default == "direct" and sig["theta"].default == 0.5
    sig = inspect.signature(topsy_amd.gravity_tree).parameters
    assert sig["theta"].default == 0.5 and sig["G"].default == 1.0 and sig["targets"].default is None


# ---- header, binding and the stand-alone layout arithmetic ----------------------------------------------------------------------------
def test_header_and_binding():
    from topsy_amd import _native
    header = open(os.path.join(ROOT, "include", "topsy_splat.h")).read()
    assert re.search(r"\bint tsp_gravity_tree\(tsp_context \*ctx,", header)
    assert re.search(r"^ \* 124: new entry point tsp_gravity_tree", header, flags=re.M)
    fields = re.search(r"typedef struct \{ int64_t ([^}]*); \} tsp_gravity_tree_info;", header).group(1)
    assert [f.strip() for f in fields.split(",")] == [name for name, _ in _native.GravityTreeInfo._fields_]
    assert len(_native.SIGNATURES["tsp_gravity_tree"][1]) == 16 and _native.ABI_VERSION == 112
    for macro, value in (("TSP_GRAVITY_TREE_LEAF", _native.GRAVITY_TREE_LEAF), ("TSP_GRAVITY_TREE_FANOUT", _native.GRAVITY_TREE_FANOUT),
                         ("TSP_GRAVITY_TREE_ERROR_K", _native.GRAVITY_TREE_ERROR_K)):
        assert int(re.search(rf"^#define {macro} (\d+)", header, flags=re.M).group(1)) == value
    assert (_native.GRAVITY_TREE_LEAF, _native.GRAVITY_TREE_FANOUT) == (tree_gravity_ref.LEAF, tree_gravity_ref.FANOUT)
    assert _native.GRAVITY_TREE_ERROR_K <= 168          # 168 * 2^-24 = 1e-5, the project's parity tolerance
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert _native.load_library().tsp_version() >= 124


def test_layout_header_matches_the_model():
    """the level sizes the kernel's layout header computes are the model's (the header is plain C++: read its constants)"""
    text = open(os.path.join(ROOT, "topsy_amd", "csrc", "tsp_gravity_tree_layout.h")).read()
    assert int(re.search(r"constexpr int LEAF = (\d+);", text).group(1)) == tree_gravity_ref.LEAF
    assert int(re.search(r"constexpr int FANOUT = (\d+);", text).group(1)) == tree_gravity_ref.FANOUT
    assert int(re.search(r"constexpr int MAX_LEVELS = (\d+);", text).group(1)) == 10
    counts = [-(-(2 ** 31 - 1) // tree_gravity_ref.LEAF)]
    while counts[-1] > 1:
        counts.append(-(-counts[-1] // tree_gravity_ref.FANOUT))
    assert len(counts) == 10


def test_design_lists_the_call_as_stateless():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "tsp_gravity_tree" in design and "tsp_gravity_tree" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
