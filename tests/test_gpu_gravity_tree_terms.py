"""tsp_gravity_tree on the GPU, term by term and source by source.

1, 2.  The header's rounding promise with theta > 0: against the group-exact host model (tree_gravity_ref.tree_sum(stored=True,
groups=the kernel's groups): the kernel's decisions per group box, the records rounded as store_node rounds them, every term in
float64), |got - model| <= K * 2^-24 * sum |term| per target and component, K = TSP_GRAVITY_TREE_ERROR_K, on scenes whose Morton
order is not in doubt (tree_gravity_scenes.cell_scene), with nodes accepted on three levels and more.  A group within 1e-4 of a
threshold ("ambiguous": the float32 test may decide the other way) is not compared; at most a tenth of a case's groups may be.
Where a call has no ambiguous group its pair counts must be the model's exactly.

3, 4.  The partition promise on deep trees: with eps = 1e5 every term is m / eps, so the potential of every target is
-(M - m_i) / eps (targets = sources) or -M / eps (separate targets at the sources' places) whatever the tree does, as long as every
source with mass reaches every target exactly once; one source lost or doubled of 4096 is 2.4e-4, 4000 * 2^-24.  The accelerations
of sampled targets are compared with the float64 direct sum over the massive sources: there a node's term is M (t - c) / eps^3.

Every test prints what it measured."""
import numpy as np
import pytest

import gravity_ref
import tree_gravity_scenes as scenes
from test_gpu_gravity import cols
from test_gpu_scratch_alloc_failure import native      # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


@pytest.fixture(scope="module")
def ctx(native):
    c = native.Context(16, 2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def K(native):
    return native.GRAVITY_TREE_ERROR_K


def run(ctx, src, mass, eps, tgt=None, theta=0.5, **kw):
    return ctx.gravity_tree(*cols(src), mass, eps, targets=None if tgt is None else cols(tgt), theta=theta, **kw)


# ---- 1, 2. term-exact --------------------------------------------------------------------------------------------------------------------
def term_exact(ctx, K, size, eps_name, theta, self_targets):
    src, mass, eps, _ = scenes.term_scene(size, eps_name)
    tgt = None if self_targets else scenes.term_targets()[0]
    what = f"{size}, {eps_name}, theta = {theta}, {'targets = sources' if self_targets else 'separate targets'}"
    model = scenes.term_model(size, eps_name, theta, self_targets)
    amb, levels = scenes.check_case_conditions(model, what, scenes.min_levels(size, theta, self_targets))
    pot, acc, info = run(ctx, src, mass, eps, tgt, theta=theta)
    assert (info["n_levels"], info["n_nodes"], info["n_valid_sources"]) == (model["n_levels"], model["n_nodes"], len(src))
    assert info["n_valid_targets"] == sum(len(g["targets"]) for g in model["groups"])
    assert np.array_equal(np.isnan(pot), np.isnan(model["pot"])) and np.array_equal(np.isnan(acc), np.isnan(model["acc"]))
    ratios = scenes.group_ratios(pot, acc, model)
    counts = (info["pairs_direct"], info["pairs_node"])
    print(f"\n{what}: worst |got - model| / (2^-24 scale) = {ratios[~amb].max():.3f} over {int((~amb).sum())} groups (bound {K}); "
          f"{int(amb.sum())} ambiguous (worst among them {ratios[amb].max() if amb.any() else 0.0:.3f}); nodes accepted on levels "
          f"{levels.tolist()}; pairs {counts}, the model's {(model['pairs_direct'], model['pairs_node'])}")
    bad = np.nonzero(~amb & ~(ratios <= K))[0]
    assert not len(bad), f"{what}: groups {bad.tolist()} are {ratios[bad].tolist()} x 2^-24 scale from the model (bound {K})"
    assert info["pairs_node"] > 0
    if not amb.any():
        assert counts == (model["pairs_direct"], model["pairs_node"]), what


@pytest.mark.parametrize("theta", scenes.TERM_THETAS)
@pytest.mark.parametrize("eps_name", list(scenes.CELL_EPS))
@pytest.mark.parametrize("size", list(scenes.CELL_SIZES))
def test_separate_targets_term_exact(ctx, K, size, eps_name, theta):
    groups = scenes.term_model(size, eps_name, theta, False)["groups"]
    sizes = [len(g["targets"]) for g in groups]
    assert sizes[:scenes.N_BOX_GROUPS] == [64] * scenes.N_BOX_GROUPS and sizes[scenes.N_BOX_GROUPS:] == [61, 1, 37]
    term_exact(ctx, K, size, eps_name, theta, False)


@pytest.mark.parametrize("theta", scenes.SELF_THETAS)
@pytest.mark.parametrize("eps_name", list(scenes.CELL_EPS))
@pytest.mark.parametrize("size", list(scenes.CELL_SIZES))
def test_targets_are_sources_term_exact(ctx, K, size, eps_name, theta):
    """theta = 1 is the edge of the header's claim that a node holding a target of the group is never accepted: a self term would
    be m / eps, far outside the bound"""
    term_exact(ctx, K, size, eps_name, theta, True)


# ---- 3, 4. partition ---------------------------------------------------------------------------------------------------------------------
def sampled_acc_ratios(src, mass, massive, tgt, acc):
    """|acc - direct| / (2^-24 acc_scale) at the targets, per component: the float64 direct sum over the sources with mass (a target
    at a source's place: that pair's acceleration term is 0); and the same with the header's allowance for the float32 c of a node
    added to the bound: 2^-24 |c| per coordinate, |c| <= max |x|, over all nodes at most 2^-24 max |x| M / eps^3"""
    eps = scenes.PARTITION_EPS
    ref = gravity_ref.direct_sum(src[massive], mass[massive], eps, tgt)
    delta = np.abs(acc - ref["acc"])
    c_allowance = U * np.abs(src[massive].astype(np.float64)).max(axis=0) * mass[massive].astype(np.float64).sum() / eps ** 3
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(delta == 0.0, 0.0, delta / (U * ref["acc_scale"]))
        allowed = np.where(delta == 0.0, 0.0, np.maximum(delta - c_allowance, 0.0) / (U * ref["acc_scale"]))
    return float(np.nan_to_num(ratio, nan=np.inf).max()), float(np.nan_to_num(allowed, nan=np.inf).max())


@pytest.mark.parametrize("case", list(scenes.PARTITION_CASES))
def test_partition_on_a_deep_tree(ctx, K, case):
    """Four calls against the direct sum, and the clump once more where it lies in the scene, 0.2 .. 0.75 from the origin and 0.0075
    wide: there the float32 c of a node may err by 2^-24 |c|, 250 times the rounding bound on the cube's scale (measured: 237), so
    the accelerations are held to the bound plus that allowance of the header; the potentials to the same bound as everywhere."""
    n, eps = scenes.N_DEEP, scenes.PARTITION_EPS
    src, mass = scenes.partition_case(n, case)
    massive = np.nonzero(mass)[0]
    pot, acc, info = run(ctx, src, mass, eps, theta=scenes.PARTITION_THETA)
    assert info["n_levels"] == 7 and info["n_valid_sources"] == info["n_valid_targets"] == n
    total = float(mass.astype(np.float64).sum())
    rel = np.abs(pot * eps / -(total - mass.astype(np.float64)) - 1.0)
    rows = np.concatenate([np.random.RandomState(3).choice(n, 3072, replace=False), massive[:1024]])
    acc_ratio, acc_ratio_allowed = sampled_acc_ratios(src, mass, massive, src[rows], acc[rows])
    pairs = info["pairs_direct"] + info["pairs_node"]
    print(f"\n7 levels, mass in the cube '{case}': max |pot eps / -(M - m_i) - 1| = {rel.max() / U:.3f} x 2^-24 (bound {K + 1}); acc of "
          f"4096 rows within {acc_ratio:.3f} x 2^-24 acc_scale (bound {K}; {acc_ratio_allowed:.3f} beyond the allowance for c); "
          f"{info['pairs_direct']} particle and {info['pairs_node']} node terms, {pairs / n ** 2:.2e} n^2")
    worst = int(np.argmax(rel))
    assert rel.max() <= (K + 1) * U, f"target {worst}: {rel[worst] / U} x 2^-24 = {rel[worst] * total / mass[massive].mean():.3f} mean masses"
    assert (acc_ratio_allowed if case == "clump" else acc_ratio) <= K
    assert 0 < pairs < n * n / 100 and info["pairs_node"] > 0


@pytest.mark.parametrize("order", ["caller's", "sorted by x"])
@pytest.mark.parametrize("case", ["centre", "clump at the origin"])
def test_partition_with_separate_targets(ctx, K, case, order):
    n, eps = scenes.N_SIX, scenes.PARTITION_EPS
    src, mass = scenes.partition_case(n, case)
    massive = np.nonzero(mass)[0]
    picked = np.random.RandomState(5).choice(n, 50_000, replace=False)      # loose groups: each spans the scene
    if order == "sorted by x":
        picked = picked[np.argsort(src[picked, 0], kind="stable")]          # tight in x: thin slabs
    tgt = src[picked]
    pot, acc, info = run(ctx, src, mass, eps, tgt, theta=scenes.PARTITION_THETA)
    assert info["n_levels"] == 6 and info["n_valid_targets"] == len(tgt)
    total = float(mass.astype(np.float64).sum())
    rel = np.abs(pot * eps / -total - 1.0)                                   # a target at a source's place sees that source too
    rows = np.arange(0, len(tgt), 12)[:4096]
    acc_ratio, _ = sampled_acc_ratios(src, mass, massive, tgt[rows], acc[rows])
    print(f"\n6 levels, 50000 targets in {order} order, mass in the cube '{case}': max |pot eps / -M - 1| = {rel.max() / U:.3f} x 2^-24 "
          f"(bound {K + 1}); acc of {len(rows)} rows within {acc_ratio:.3f} x 2^-24 acc_scale (bound {K}); {info['pairs_direct']} "
          f"particle and {info['pairs_node']} node terms")
    assert rel.max() <= (K + 1) * U, f"target {int(np.argmax(rel))}: {rel.max() / U} x 2^-24"
    assert acc_ratio <= K
    assert info["pairs_direct"] + info["pairs_node"] > 0
    if order == "sorted by x":
        assert info["pairs_node"] > 0
