"""Friends-of-friends groups on the CPU: fof_reference, the restatement of the contract of tsp_fof_groups
(include/topsy_splat.h) that test_gpu_fof.py holds the GPU to, the scenes both files use, and the host logic of
topsy_amd.friends_of_friends, halos= and center="halo-N" (no GPU: _native.Context is made to refuse).

fof_reference: candidate pairs from scipy's cKDTree at radius l * (1 + 1e-4) (boxsize = L and positions wrapped, for the tree
only), each decided by the contract's own float32 d2 <= ll2 evaluated in numpy with the operations in the header's order,
components from scipy.sparse.csgraph.connected_components, ranks by (size descending, smallest index ascending).  Because the
link test is the contract's exact arithmetic there is no tolerance: labels are compared for equality.

cliques= (the dense-core scene only): 30 000 points inside a ball of radius l / 4 have 4.5e8 pairs within l, more than the
pair list of query_pairs can hold.  For an index set given as a clique the reference tests every member against the set's first
member with the exact float32 test and *asserts* that each one is linked, takes those edges, and leaves out the candidate pairs
with both ends in the same clique: such a pair joins two particles the hub edges already join, so the components are the same.
Every other candidate pair -- clique to clique, clique to rest, rest to rest -- is generated and tested as usual."""
import functools

import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree


def contract_d2(pa, pb, period):
    """The header's float32 d2 between rows of pa and pb (float32 (m, 3)), operation by operation."""
    L = np.float32(period)
    d = []
    for a in range(3):
        dx = pb[:, a] - pa[:, a]
        if period > 0:
            t = dx / L
            t = np.rint(t)
            dx = dx - L * t
        d.append(dx)
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def _rank(n, valid_idx, comp, min_members):
    """Labels and counts from the component index of every valid particle."""
    labels = np.full(n, -1, dtype=np.int32)
    info = {"n_valid": int(len(valid_idx)), "n_groups": 0, "n_grouped": 0, "largest": 0}
    if len(valid_idx) == 0:
        return labels, info
    ncomp = int(comp.max()) + 1
    size = np.bincount(comp, minlength=ncomp)
    first = np.full(ncomp, n, dtype=np.int64)
    np.minimum.at(first, comp, valid_idx)
    order = np.lexsort((first, -size))                      # size descending, then smallest member index ascending
    order = order[size[order] >= min_members]
    rank = np.zeros(ncomp, dtype=np.int32)
    rank[order] = np.arange(1, len(order) + 1, dtype=np.int32)
    labels[valid_idx] = rank[comp]
    info.update(n_groups=int(len(order)), n_grouped=int(size[order].sum()), largest=int(size[order[0]]) if len(order) else 0)
    return labels, info


def fof_reference(pos, linking_length, period=0.0, min_members=20, cliques=None):
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    n = len(pos)
    ll = np.float32(linking_length)
    ll2 = ll * ll
    valid_idx = np.flatnonzero(np.isfinite(pos).all(axis=1))
    p = pos[valid_idx]
    m = len(p)
    if m == 0:
        return _rank(n, valid_idx, np.zeros(0, dtype=np.int64), min_members)
    tree_pos = p.astype(np.float64)
    boxsize = None
    if period > 0:
        tree_pos = np.mod(tree_pos, float(period))
        tree_pos[tree_pos >= float(period)] = 0.0
        boxsize = float(period)
    radius = float(ll) * (1.0 + 1e-4)
    pairs = []
    if not cliques:
        pairs.append(cKDTree(tree_pos, boxsize=boxsize).query_pairs(radius, output_type="ndarray"))
    else:
        where = np.full(n, -1, dtype=np.int64)
        where[valid_idx] = np.arange(m)
        sets = []
        for c in cliques:
            c = where[np.asarray(c)]
            assert (c >= 0).all()
            hub = np.repeat(c[:1], len(c) - 1)
            assert (contract_d2(p[hub], p[c[1:]], period) <= ll2).all(), "a clique member is not linked to its hub"
            pairs.append(np.stack([hub, c[1:]], axis=1))
            sets.append(c)
        rest = np.setdiff1d(np.arange(m), np.concatenate(sets))
        trees = [cKDTree(tree_pos[s], boxsize=boxsize) for s in sets + [rest]]
        sets.append(rest)
        pairs.append(rest[trees[-1].query_pairs(radius, output_type="ndarray")])
        for a in range(len(sets)):
            for b in range(a + 1, len(sets)):
                cross = trees[a].sparse_distance_matrix(trees[b], radius, output_type="ndarray")
                pairs.append(np.stack([sets[a][cross["i"]], sets[b][cross["j"]]], axis=1))
    pairs = np.concatenate([q.reshape(-1, 2) for q in pairs]).astype(np.int64)
    linked = contract_d2(p[pairs[:, 0]], p[pairs[:, 1]], period) <= ll2
    i, j = pairs[linked, 0], pairs[linked, 1]
    graph = coo_matrix((np.ones(len(i), dtype=np.int8), (i, j)), shape=(m, m))
    _, comp = connected_components(graph, directed=False)
    return _rank(n, valid_idx, comp.astype(np.int64), min_members)


def fof_brute_force(pos, linking_length, period=0.0, min_members=20):
    """O(n^2): every pair by the contract's test."""
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    n = len(pos)
    ll2 = np.float32(linking_length) * np.float32(linking_length)
    valid_idx = np.flatnonzero(np.isfinite(pos).all(axis=1))
    p = pos[valid_idx]
    m = len(p)
    i, j = np.triu_indices(m, 1)
    linked = contract_d2(p[i], p[j], period) <= ll2
    graph = coo_matrix((np.ones(int(linked.sum()), dtype=np.int8), (i[linked], j[linked])), shape=(m, m))
    _, comp = connected_components(graph, directed=False)
    return _rank(n, valid_idx, comp.astype(np.int64), min_members)


# ---- scenes ---------------------------------------------------------------------------------------------------------------
CLUMPS = (((0.25, 0.62, 0.4), 0.02, 60000), ((0.7, 0.3, 0.55), 0.012, 30000), ((0.98, 0.5, 0.02), 0.015, 20000),
          ((0.5, 0.5, 0.9), 0.008, 8000), ((0.1, 0.1, 0.1), 0.004, 1500))
CLUMPS_N = 200000
CLUMPS_LL = 0.2 * CLUMPS_N ** (-1.0 / 3.0)


@functools.lru_cache(maxsize=None)
def clumps():
    """n = 200 000 in the unit box: five Gaussian clumps, one of them across the box faces, over a uniform background."""
    rs = np.random.RandomState(5)
    parts = [np.asarray(c) + s * rs.normal(size=(m, 3)) for c, s, m in CLUMPS]
    parts.append(rs.uniform(size=(CLUMPS_N - sum(m for _, _, m in CLUMPS), 3)))
    pos = np.mod(np.concatenate(parts), 1.0).astype(np.float32)
    pos = pos[rs.permutation(CLUMPS_N)]
    pos.setflags(write=False)
    return pos


@functools.lru_cache(maxsize=None)
def clumps_shifted():
    """The clumps with a seeded third of the particles moved by +-1 on random axes: raw coordinates outside [0, 1)."""
    rs = np.random.RandomState(6)
    pos = clumps().copy()
    moved = rs.permutation(CLUMPS_N)[:CLUMPS_N // 3]
    pos[moved] += rs.randint(-1, 2, size=(len(moved), 3)).astype(np.float32)
    pos.setflags(write=False)
    return pos


@functools.lru_cache(maxsize=None)
def clumps_reference(kind):
    pos, period = {"open": (clumps(), 0.0), "periodic": (clumps(), 1.0), "shifted": (clumps_shifted(), 1.0)}[kind]
    labels, info = fof_reference(pos, CLUMPS_LL, period, 20)
    labels.setflags(write=False)
    return labels, info


def lattice():
    g = np.arange(13, dtype=np.float32)
    return np.stack([v.ravel() for v in np.meshgrid(g, g, g, indexing="ij")], axis=1)


BELOW_ONE = float(np.nextafter(np.float32(1), np.float32(0)))
LATTICE_CASES = ((1.0, 20), (BELOW_ONE, 1), (BELOW_ONE, 2))

DENSE_LL = 0.004
DENSE_BALL = 30000


@functools.lru_cache(maxsize=None)
def dense_core():
    """Three balls of radius l / 4 with 30 000 points each, 2 000 of them exact duplicates of others: the second 0.9 l from the
    surface of the first (one group), the third 1.5 l from the surface of the second (a group of its own), over 20 000
    background points.  Returns (pos, the three index sets)."""
    rs = np.random.RandomState(11)
    ll = DENSE_LL
    centres = np.array([[0.3, 0.3, 0.3], [0.3 + 1.4 * ll, 0.3, 0.3], [0.3 + 1.4 * ll, 0.3 + 2.0 * ll, 0.3]])
    parts = []
    for c in centres:
        v = rs.normal(size=(DENSE_BALL - 2000, 3))
        v *= (0.25 * ll * rs.uniform(size=(len(v), 1)) ** (1.0 / 3.0)) / np.linalg.norm(v, axis=1, keepdims=True)
        v = np.concatenate([v, v[rs.randint(0, len(v), size=2000)]])
        parts.append(c + v)
    parts.append(rs.uniform(size=(20000, 3)))
    pos = np.concatenate(parts).astype(np.float32)
    perm = rs.permutation(len(pos))
    pos = pos[perm]
    where = np.argsort(perm)                                   # old index -> new index
    balls = tuple(np.sort(where[k * DENSE_BALL:(k + 1) * DENSE_BALL]) for k in range(3))
    pos.setflags(write=False)
    return pos, balls


@functools.lru_cache(maxsize=None)
def dense_core_reference():
    pos, balls = dense_core()
    labels, info = fof_reference(pos, DENSE_LL, 0.0, 20, cliques=balls)
    labels.setflags(write=False)
    return labels, info


INVALID_LL = 0.01


@functools.lru_cache(maxsize=None)
def invalid_scene():
    """Two clumps of radius l / 4 whose surfaces are 1.5 l apart; the only particle between them has y = NaN (with a finite y it
    would sit 0.75 l from both).  +-inf coordinates elsewhere, and a thin background.  Returns (pos, clump A, clump B, invalid)."""
    rs = np.random.RandomState(12)
    ll = INVALID_LL
    def ball(c, m):
        v = rs.normal(size=(m, 3))
        return np.asarray(c) + v * (0.25 * ll * rs.uniform(size=(m, 1)) ** (1.0 / 3.0)) / np.linalg.norm(v, axis=1, keepdims=True)
    a, b = ball((0.4, 0.5, 0.5), 500), ball((0.4 + 2.0 * ll, 0.5, 0.5), 333)
    odd = np.array([[0.4 + ll, np.nan, 0.5], [np.inf, 0.2, 0.2], [0.7, -np.inf, 0.7], [0.1, 0.1, np.nan], [np.nan, np.nan, np.nan]])
    pos = np.concatenate([a, b, odd, rs.uniform(size=(200, 3))]).astype(np.float32)
    perm = rs.permutation(len(pos))
    pos = pos[perm]
    where = np.argsort(perm)
    pos.setflags(write=False)
    return pos, where[:500], where[500:833], where[833:838]


# ---- the reference itself ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("period", [0.0, 1.0])
def test_reference_equals_brute_force(period):
    rs = np.random.RandomState(3)
    pos = np.concatenate([rs.uniform(size=(300, 3)), (0.97, 0.5, 0.03) + 0.03 * rs.normal(size=(200, 3))]).astype(np.float32)
    if period == 0.0:
        pos = np.mod(pos, 1.0).astype(np.float32)
    pos[17, 1] = np.nan
    for ll, min_members in ((0.05, 5), (0.02, 1), (0.1, 20)):
        want = fof_brute_force(pos, ll, period, min_members)
        got = fof_reference(pos, ll, period, min_members)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1] and got[0][17] == -1
        assert got[1]["n_valid"] == 499
    # the clique form is the same reference
    clique = np.flatnonzero(np.linalg.norm(pos - np.float32((0.97, 0.5, 0.03)), axis=1) < 0.02)
    assert len(clique) > 10
    assert np.array_equal(fof_reference(pos, 0.05, period, 5, cliques=[clique])[0], fof_brute_force(pos, 0.05, period, 5)[0])


def test_lattice_is_the_exact_boundary():
    pos = lattice()
    labels, info = fof_reference(pos, *LATTICE_CASES[0][:1], 0.0, LATTICE_CASES[0][1])
    assert (labels == 1).all() and info == {"n_valid": 2197, "n_groups": 1, "n_grouped": 2197, "largest": 2197}
    labels, info = fof_reference(pos, BELOW_ONE, 0.0, 1)
    assert np.array_equal(labels, np.arange(1, 2198)) and info == {"n_valid": 2197, "n_groups": 2197, "n_grouped": 2197, "largest": 1}
    labels, info = fof_reference(pos, BELOW_ONE, 0.0, 2)
    assert (labels == 0).all() and info == {"n_valid": 2197, "n_groups": 0, "n_grouped": 0, "largest": 0}


def test_clumps_open_and_periodic():
    assert abs(CLUMPS_LL - 0.0034199) < 1e-7
    labels, info = clumps_reference("open")
    sizes = np.bincount(labels[labels > 0])[1:]
    print("open:", info, sizes)
    assert info["n_groups"] == 9 and sizes[:8].tolist() == [56193, 29207, 15766, 7824, 1493, 1295, 1202, 65]
    labels, info = clumps_reference("periodic")
    sizes = np.bincount(labels[labels > 0])[1:]
    print("periodic:", info, sizes)
    assert info["n_groups"] == 5 and sizes.tolist() == [56193, 29207, 18441, 7824, 1493]
    assert info == {"n_valid": CLUMPS_N, "n_groups": 5, "n_grouped": int(sizes.sum()), "largest": 56193}


def test_shifted_clumps_leave_the_box():
    pos = clumps_shifted()
    assert pos.min() < -0.5 and pos.max() > 1.5
    labels, info = clumps_reference("shifted")
    print("shifted:", info)
    assert info["n_groups"] == 5 and info["largest"] == 56193
    # no pair of this scene sits so close to the linking length that the rounding of the moved coordinates decides it
    assert np.array_equal(labels, clumps_reference("periodic")[0])


def test_dense_core_scene():
    pos, balls = dense_core()
    labels, info = dense_core_reference()
    print("dense core:", info, np.bincount(labels[labels > 0])[1:6])
    assert len(np.unique(pos[balls[0]], axis=0)) <= DENSE_BALL - 1900
    one, two, three = (np.unique(labels[b]) for b in balls)
    assert len(one) == len(two) == len(three) == 1 and one[0] == two[0] == 1 and three[0] == 2
    assert info["largest"] >= 2 * DENSE_BALL


def test_invalid_scene():
    pos, a, b, odd = invalid_scene()
    labels, info = fof_reference(pos, INVALID_LL, 0.0, 20)
    assert (labels[odd] == -1).all() and info["n_valid"] == len(pos) - 5
    assert (labels[a] == 1).all() and (labels[b] == 2).all() and info["n_groups"] == 2
    # with a finite y the particle in the middle would bridge the two
    whole = pos.copy()
    whole[odd[0], 1] = 0.5
    assert fof_reference(whole, INVALID_LL, 0.0, 20)[1]["largest"] == 500 + 333 + 1


# ---- host logic -------------------------------------------------------------------------------------------------------------
def _no_context(monkeypatch):
    from topsy_amd import _native

    def refuse(*a, **k):
        raise AssertionError("a context was created before the arguments were checked")
    monkeypatch.setattr(_native, "Context", refuse)


def test_friends_of_friends_checks_its_arguments_first(monkeypatch):
    import topsy_amd
    _no_context(monkeypatch)
    pos = np.random.RandomState(0).uniform(size=(10, 3)).astype(np.float32)
    flat = pos.copy()
    flat[:, 2] = 0.25
    bad = [
        (dict(pos=np.zeros((10, 2))), r"\(10, 2\)"),
        (dict(pos=np.zeros(30)), r"\(30,\)"),
        (dict(pos=np.zeros((0, 3))), "at least one"),
        (dict(pos=pos, linking_length=0.0), "0.0"),
        (dict(pos=pos, linking_length=-1.0), "-1.0"),
        (dict(pos=pos, linking_length=np.nan), "nan"),
        (dict(pos=pos, linking_length=np.inf), "inf"),
        (dict(pos=pos, linking_length="wide"), "wide"),
        (dict(pos=pos, linking_length=True), "True"),
        (dict(pos=pos, linking_length=1e-60), "1e-60"),
        (dict(pos=pos, b=0.0), "0.0"),
        (dict(pos=pos, b=-0.2), "-0.2"),
        (dict(pos=pos, b=np.nan), "nan"),
        (dict(pos=pos, min_members=0), "0"),
        (dict(pos=pos, min_members=2.5), "2.5"),
        (dict(pos=pos, min_members=True), "True"),
        (dict(pos=pos, periodicity_scale=0.0), "0.0"),
        (dict(pos=pos, periodicity_scale=-1.0), "-1.0"),
        (dict(pos=pos, periodicity_scale=np.inf), "inf"),
        (dict(pos=pos, periodicity_scale="box"), "box"),
        (dict(pos=pos, linking_length=0.5, periodicity_scale=1.0), "half"),
        (dict(pos=pos, linking_length=0.7, periodicity_scale=1.0), "half"),
        (dict(pos=pos, b=5.0, periodicity_scale=1.0), "half"),
        (dict(pos=flat), "explicit linking_length"),
        (dict(pos=np.full((10, 3), np.nan)), "no particle"),
    ]
    for kwargs, match in bad:
        with pytest.raises(ValueError, match=match):
            topsy_amd.friends_of_friends(**kwargs)


def test_default_linking_length():
    from topsy_amd import loader
    rs = np.random.RandomState(1)
    pos = (rs.uniform(size=(1000, 3)) * (2.0, 3.0, 4.0)).astype(np.float32)
    pos[5] = np.nan
    extent = pos[np.isfinite(pos).all(axis=1)].astype(np.float64)
    volume = np.prod(extent.max(axis=0) - extent.min(axis=0))
    assert loader.fof_linking_length(pos, 0.2, 0.0) == 0.2 * (volume / 999) ** (1.0 / 3.0)
    assert loader.fof_linking_length(pos, 0.2, 10.0) == 0.2 * (1000.0 / 999) ** (1.0 / 3.0)
    assert loader.fof_linking_length(pos, 0.1, 10.0) == 0.1 * (1000.0 / 999) ** (1.0 / 3.0)
    assert loader.check_fof_arguments() == (None, 0.2, 20, 0.0)
    assert loader.check_fof_arguments(0.25, 0.3, np.int64(7), 2) == (0.25, 0.3, 7, 2.0)


def test_catalogue_of_labels():
    import topsy_amd
    labels = np.array([2, 0, 1, 1, -1, 1, 2, 0, 4], dtype=np.int64)
    cat = topsy_amd.FofCatalogue(labels)
    assert cat.group.dtype == np.int32 and len(cat) == 4 and cat.sizes.dtype == np.int64 and cat.sizes.tolist() == [3, 2, 0, 1]
    assert cat.members(1).tolist() == [2, 3, 5] and cat.members(2).tolist() == [0, 6] and cat.members(3).tolist() == []
    assert cat.linking_length is None
    with pytest.raises(ValueError, match="4 halo"):
        cat.members(5)
    with pytest.raises(ValueError, match="0"):
        cat.members(0)
    empty = topsy_amd.FofCatalogue(np.zeros(5, dtype=np.int32))
    assert len(empty) == 0 and empty.sizes.shape == (0,)


def test_halos_and_halo_centres_are_checked_first(monkeypatch):
    import topsy_amd
    from topsy_amd import loader
    _no_context(monkeypatch)
    pos = np.random.RandomState(0).uniform(size=(10, 3)).astype(np.float32)
    h = np.ones(10, dtype=np.float32)
    labels = np.array([1, 1, 1, 2, 2, 0, 0, -1, 2, 1])
    for halos, match in (("ahf", "ahf"), ({"ll": 0.1}, "ll"), ({"linking_length": -1.0}, "-1.0"), ({"min_members": 0}, "0"),
                         ({"b": "x"}, "x"), (np.ones(9, dtype=np.int64), r"\(9,\)"), (np.ones(10), "float64"),
                         (np.ones((10, 1), dtype=np.int32), r"\(10, 1\)"), (np.ones(10, dtype=bool), "bool"), (3.5, "float"),
                         ({"linking_length": 0.6}, "half")):
        with pytest.raises(ValueError, match=match):
            topsy_amd.from_arrays(pos, h, h, halos=halos, periodicity_scale=1.0)
        with pytest.raises(ValueError, match=match):
            loader.ArrayDataLoader(pos=pos, smooth=h, mass=h, halos=halos, periodicity_scale=1.0)
    # halo-N: N >= 1, and only with a catalogue
    for center in ("halo-0", "halo--1", "halo-x", "halo-", "halo-1.5", "halo-01"):
        for halos in ("fof", labels, None):
            with pytest.raises(ValueError, match=center):
                loader.ArrayDataLoader(pos=pos, smooth=h, mass=h, center=center, halos=halos)
            with pytest.raises(ValueError, match=center):
                topsy_amd.from_arrays(pos, h, h, center=center, halos=halos)
    with pytest.raises(ValueError, match="halo-3.*halos="):
        loader.ArrayDataLoader(pos=pos, smooth=h, mass=h, center="halo-3")
    with pytest.raises(ValueError, match=r"\(10, 2\)"):
        loader.ArrayDataLoader(pos=np.zeros((10, 2)), smooth=h, mass=h, center="halo-1", halos=labels)
    # accepted without touching the GPU; the catalogue of the caller's labels needs none either
    ld = loader.ArrayDataLoader(pos=pos, smooth=h, mass=h, center="halo-2", halos=labels)
    cat = ld.get_halos()
    assert cat is ld.get_halos() and len(cat) == 2 and cat.sizes.tolist() == [4, 3] and cat.members(2).tolist() == [3, 4, 8]
    with pytest.raises(ValueError, match="2 halo"):
        ld.get_halo_center(3)
    with pytest.raises(ValueError, match="no halo catalogue"):
        loader.ArrayDataLoader(pos=pos, smooth=h, mass=h).get_halos()
    ld = loader.ArrayDataLoader(pos=pos, smooth=h, mass=h)
    ld.set_halos(labels)
    assert ld.get_halos().members(1).tolist() == [0, 1, 2, 9]
    with pytest.raises(ValueError, match=r"\(4,\)"):
        ld.set_halos(labels[:4])
    # "fof" with a bounding box of no volume: refused when the catalogue is asked for, before a context exists
    flat = pos.copy()
    flat[:, 0] = 1.0
    with pytest.raises(ValueError, match="explicit linking_length"):
        loader.ArrayDataLoader(pos=flat, smooth=h, mass=h, halos="fof").get_halos()


def test_labels_survive_the_cell_order():
    from topsy_amd import loader
    rs = np.random.RandomState(2)
    pos = rs.uniform(size=(5000, 3)).astype(np.float32)
    h = np.ones(5000, dtype=np.float32)
    labels = (np.floor(pos[:, 0] * 4).astype(np.int64) - 1)          # -1 .. 2, a function of the position
    ld = loader.ArrayDataLoader(pos=pos, smooth=h, mass=h, halos=labels, with_cells=True)
    assert not np.array_equal(ld.get_positions(), pos)
    assert np.array_equal(ld.get_halos().group, np.floor(ld.get_positions()[:, 0] * 4).astype(np.int32) - 1)
    assert len(ld.get_halos()) == 2 and ld.get_halos().sizes.sum() == (labels > 0).sum()


def test_binding_matches_the_header():
    import ctypes
    import os
    import re
    from topsy_amd import _native, multigpu, surface, visualizer
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "topsy_splat.h")).read()
    assert " * 114: new entry point tsp_fof_groups" in text
    assert re.search(r"int64_t n_valid, n_groups, n_grouped, largest;\s*\} tsp_fof_info;", text)
    assert ctypes.sizeof(_native.FofInfo) == 32
    restype, argtypes = _native.SIGNATURES["tsp_fof_groups"]
    assert restype is ctypes.c_int and len(argtypes) == 10
    assert _native.load_library().tsp_version() >= 114
    assert hasattr(_native.Context, "fof_groups") and hasattr(multigpu.MultiGpuContext, "fof_groups")
    assert hasattr(visualizer.VisualizerBase, "centre_on_halo") or hasattr(visualizer.Visualizer, "centre_on_halo")
    assert hasattr(surface.SurfaceView, "centre_on_halo")
