"""The scenes, the fixed targets and the caps of the truncation-quality tests of tsp_gravity_tree, shared by the CPU test of the
host model (test_gravity_tree_cpu.py) and the GPU test (test_gpu_gravity_tree.py); below them the scenes, targets and group-exact
models of the term and partition tests (test_gpu_gravity_tree_terms.py).  Every reference is computed once per process."""
import functools

import numpy as np

import gravity_ref
import tree_gravity_ref

f32 = np.float32
N_QUALITY = 16384
N_ROWS = 2048
THETAS = (0.3, 0.5, 0.8)
CAP_P99, CAP_MAX = 1e-2, 5e-2          # at theta = 0.5: p99 and max of e = |a_tree - a_direct| / |a_direct| over the fixed targets


def scene(*args, **kw):
    from test_gpu_gravity import scene as gravity_scene
    return gravity_scene(*args, **kw)


def plummer(n, seed):
    """n equal-mass particles of total mass 1 from a Plummer sphere of scale length 1 (test_gpu_gravity.plummer_sphere), float32"""
    rs = np.random.RandomState(seed)
    r = 1.0 / np.sqrt(rs.uniform(size=n) ** (-2.0 / 3.0) - 1.0)
    v = rs.normal(size=(n, 3))
    return (r[:, None] * v / np.linalg.norm(v, axis=1)[:, None]).astype(f32), np.full(n, 1.0 / n, dtype=f32)


@functools.lru_cache(maxsize=None)
def quality_scene(name):
    """-> (src float32 (n, 3), mass float32 (n,), eps: a float or float32 (n,))"""
    if name == "plummer":              # one softening length
        pos, mass = plummer(N_QUALITY, 5)
        return pos, mass, 0.01
    if name == "wide_eps":             # clustered and uniform, masses over two decades, eps over three
        return scene(N_QUALITY, 1, seed=5)[:3]
    if name == "clumps_and_outlier":   # two tight clumps and one particle at 1e6 box units: nearly every key is the same
        rs = np.random.RandomState(8)
        pos = np.concatenate([rs.normal(size=(2000, 3)) * 0.01, rs.normal(size=(2000, 3)) * 0.02 + [1.0, 0.5, -0.3],
                              [[1e6, -1e6, 1e6]]])
        return pos.astype(f32), (10.0 ** rs.uniform(-1, 0, len(pos))).astype(f32), 1e-3
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def quality_rows(name):
    n = len(quality_scene(name)[0])
    return np.sort(np.random.RandomState(1).choice(n, min(N_ROWS, n), replace=False))


@functools.lru_cache(maxsize=None)
def direct_rows(name):
    """gravity_ref.direct_sum's rows at the fixed targets (targets = sources: the pair of a particle with itself left out)"""
    src, mass, eps = quality_scene(name)
    rows = quality_rows(name)
    ref = gravity_ref.direct_sum(src, mass, eps, targets=src[rows])
    # an explicit target at a source's place sees that source too: d = 0, so its acceleration term is 0 and its potential term
    # is m / eps (eps > 0 in these scenes); take it out again
    e = np.full(len(src), eps, dtype=f32) if np.ndim(eps) == 0 else eps
    self_term = mass[rows].astype(np.float64) / e[rows].astype(np.float64)
    ref["pot"] = ref["pot"] + self_term
    ref["pot_scale"] = ref["pot_scale"] - self_term
    return ref


@functools.lru_cache(maxsize=None)
def model_tree(name):
    return tree_gravity_ref.build_tree(*quality_scene(name))


@functools.lru_cache(maxsize=None)
def model_quality(name, theta):
    """the host model at the fixed targets: dict with pot, acc (rows only), e (per target), p99, max, pairs per target"""
    src, mass, eps = quality_scene(name)
    rows = quality_rows(name)
    got = tree_gravity_ref.tree_sum(src, mass, eps, None, theta=theta, rows=rows, tree=model_tree(name))
    e = tree_gravity_ref.relative_acc_error(got["acc"][rows], direct_rows(name)["acc"])
    return {"pot": got["pot"][rows], "acc": got["acc"][rows], "e": e, "p99": float(np.percentile(e, 99)), "max": float(e.max()),
            "pairs_per_target": float(got["per_target_pairs"][rows].mean())}


def rounding_floor(name, K):
    """what the theta = 0 rounding bound allows in e, per target: K 2^-24 |acc_scale| / |a_direct|"""
    ref = direct_rows(name)
    return K * 2.0 ** -24 * np.linalg.norm(ref["acc_scale"], axis=1) / np.linalg.norm(ref["acc"], axis=1)


@functools.lru_cache(maxsize=None)
def uniform_cube(n=65536, seed=17):
    rs = np.random.RandomState(seed)
    return rs.uniform(0.0, 1.0, size=(n, 3)).astype(f32), np.full(n, 1.0 / n, dtype=f32), 1e-3


def exponential_disc(n, seed):
    rs = np.random.RandomState(seed)
    R = rs.exponential(2.0, n)
    phi = rs.uniform(0, 2 * np.pi, n)
    return np.stack([R * np.cos(phi), R * np.sin(phi), rs.normal(size=n) * 0.05], axis=1).astype(f32), np.full(n, 1.0 / n, dtype=f32)


# ---- the term-exact and the partition tests (test_gpu_gravity_tree_terms.py; the model alone: test_gravity_tree_cpu.py) ---------------
CELL_SIZES = {"4 levels": (16, 3000), "5 levels": (32, 20000)}           # (g, n) of cell_scene
CELL_EPS = {"one eps": 0.01, "eps over three decades": (1e-4, 1e-1)}
TERM_THETAS = (0.3, 0.5, 0.8, 1.0)                                       # separate targets
SELF_THETAS = (0.5, 1.0)                                                 # targets = sources
AMBIGUOUS_SHARE = 0.10                   # a condition of the tests, not a measurement: at most this share of a case's groups


def cell_keys(ijk):
    """the place of lattice cells (k, 3) on the Morton curve (x the lowest bit, as tree_gravity_ref.morton_keys)"""
    ijk = np.asarray(ijk, dtype=np.uint64)
    keys = np.zeros(len(ijk), dtype=np.uint64)
    for bit in range(21):
        for a in range(3):
            keys |= ((ijk[:, a] >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit + a)
    return keys


@functools.lru_cache(maxsize=None)
def cell_scene(g, n, seed, eps):
    """A scene whose Morton order is not in doubt: n particles in DISTINCT cells of a g^3 lattice over [0, 1]^3 (g a power of
    two), each in the central half of its cell, per axis in [(i + 0.25) / g, (i + 0.75) / g]; one exactly at (0, 0, 0) and one at
    (1, 1, 1), which pin the bounding box.  The order along the curve is then the order of the coarse cells, whatever the
    quantisation does in its last bits: the model's leaves are the kernel's.  The cells are drawn with the weights of a tilted
    Gaussian plus a uniform floor of 2 % (all six second moments non-zero and different), masses over two decades, the caller's
    order shuffled.  eps: one length, or (lo, hi) for a log-uniform length per particle.
    -> (src float32 (n, 3), mass float32 (n,), eps a float or float32 (n,), cells (n, 3) the lattice cell of each particle)"""
    assert g & (g - 1) == 0 and 2 <= n <= g ** 3
    rs = np.random.RandomState(seed)
    ijk = np.stack(np.meshgrid(np.arange(g), np.arange(g), np.arange(g), indexing="ij"), axis=-1).reshape(-1, 3)
    x = (ijk + 0.5) / g - np.array([0.55, 0.42, 0.6])
    shape = np.array([[0.30, 0.16, 0.08], [0.0, 0.20, 0.10], [0.0, 0.0, 0.12]])          # x = shape @ z, z standard normal
    z = np.linalg.solve(shape, x.T).T
    w = np.exp(-0.5 * (z * z).sum(axis=1))
    w = 0.98 * w / w.sum() + 0.02 / len(w)
    w[[0, len(w) - 1]] = 0.0                                                            # the two corner cells are taken anyway
    chosen = np.concatenate([[0, len(w) - 1], rs.choice(len(w), n - 2, replace=False, p=w / w.sum())])
    cells = ijk[chosen]
    pos = (cells + rs.uniform(0.25, 0.75, size=(n, 3))) / g
    pos[0], pos[1] = 0.0, 1.0
    mass = 10.0 ** rs.uniform(-1.0, 1.0, n)
    e = eps if np.ndim(eps) == 0 else np.exp(rs.uniform(np.log(eps[0]), np.log(eps[1]), n))
    perm = rs.permutation(n)
    pos, cells, mass = pos[perm].astype(f32), cells[perm], mass[perm].astype(f32)
    for a in (pos, cells, mass):
        a.setflags(write=False)
    if np.ndim(e):
        e = e[perm].astype(f32)
        e.setflags(write=False)
    return pos, mass, e, cells


def term_scene(size, eps_name):
    g, n = CELL_SIZES[size]
    return cell_scene(g, n, 41, CELL_EPS[eps_name])


@functools.lru_cache(maxsize=None)
def term_tree(size, eps_name):
    """the model's tree with the records as the kernel stores them"""
    src, mass, eps, _ = term_scene(size, eps_name)
    return tree_gravity_ref.build_tree(src, mass, eps, stored=True)


N_BOX_GROUPS = 40


@functools.lru_cache(maxsize=None)
def term_targets(seed=43):
    """-> (targets float32 (k, 3), groups): 40 groups of 64 targets uniform in boxes (centres uniform in [-0.5, 1.5]^3, half-widths
    log-uniform in 1e-3 .. 0.2), then a group with three non-finite targets among its 64, a group of ONE valid target (its other
    63 are NaN), and a last partial group of 37"""
    rs = np.random.RandomState(seed)
    parts = []
    for _ in range(N_BOX_GROUPS):
        centre, half = rs.uniform(-0.5, 1.5, 3), 10.0 ** rs.uniform(-3.0, np.log10(0.2), 3)
        parts.append(centre + half * rs.uniform(-1.0, 1.0, size=(64, 3)))
    holes = np.array([0.3, 0.6, 0.2]) + 0.05 * rs.uniform(-1.0, 1.0, size=(64, 3))
    holes[[5, 17, 63], [0, 1, 2]] = [np.nan, np.inf, -np.inf]
    single = np.full((64, 3), np.nan)
    single[29] = [0.71, 0.33, 0.52]
    partial = np.array([1.1, 0.4, 0.7]) + 0.02 * rs.uniform(-1.0, 1.0, size=(37, 3))
    tgt = np.concatenate(parts + [holes, single, partial]).astype(f32)
    tgt.setflags(write=False)
    return tgt, tree_gravity_ref.consecutive_groups(len(tgt))


@functools.lru_cache(maxsize=None)
def term_model(size, eps_name, theta, self_targets):
    """the group-exact model of one case: tree_gravity_ref.tree_sum(stored=True, groups=the kernel's)"""
    src, mass, eps, _ = term_scene(size, eps_name)
    tree = term_tree(size, eps_name)
    if self_targets:
        return tree_gravity_ref.tree_sum(src, mass, eps, None, theta=theta, tree=tree, groups=tree_gravity_ref.sorted_groups(tree))
    tgt, groups = term_targets()
    return tree_gravity_ref.tree_sum(src, mass, eps, tgt, theta=theta, tree=tree, groups=groups)


def group_ratios(got_pot, got_acc, model):
    """per group of the model the largest |got - model| / (2^-24 scale) over its valid targets and the four components (a
    component whose scale is 0 must be exactly 0: inf otherwise; a group without valid targets: 0)"""
    out = np.zeros(len(model["groups"]))
    for k, grp in enumerate(model["groups"]):
        rr = grp["targets"]
        if not len(rr):
            continue
        delta = np.concatenate([np.abs(got_pot[rr] - model["pot"][rr])[:, None], np.abs(got_acc[rr] - model["acc"][rr])], axis=1)
        scale = np.concatenate([model["pot_scale"][rr][:, None], model["acc_scale"][rr]], axis=1) * 2.0 ** -24
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(delta == 0.0, 0.0, delta / scale)
        out[k] = np.nan_to_num(ratio, nan=np.inf).max()
    return out


def ambiguous(model):
    return np.array([grp["margin"] < tree_gravity_ref.AMBIGUOUS for grp in model["groups"]])


def min_levels(size, theta, self_targets):
    """On how many levels a case must accept nodes: three, except where the geometry of the 4-level scene rules the third out.  Its
    level-2 nodes hold 2048 and 952 of the 3000 particles, b = 0.95 and 0.73.  No group of the scene's own particles lies b / theta
    from the centre of mass of two thirds or one third of the scene (targets = sources, any theta <= 1), and at theta = 0.3 the
    smaller node needs dmin > 2.44 where the farthest point of [-0.5, 1.5]^3 from its c is 2.03 away.  There: two levels."""
    if size == "4 levels" and (self_targets or theta < 0.5):
        return 2
    return 3


def check_case_conditions(model, what, levels_wanted=3):
    """what a case must offer for its assertions to mean something: few ambiguous groups, nodes accepted on three levels or more"""
    amb = ambiguous(model)
    levels = np.nonzero(model["accepted_per_level"])[0]
    assert amb.sum() <= AMBIGUOUS_SHARE * len(amb), f"{what}: {amb.sum()} of {len(amb)} groups are ambiguous"
    assert model["pairs_node"] > 0 and len(levels) >= levels_wanted, f"{what}: nodes accepted on levels {levels.tolist()} only"
    return amb, levels


# the partition scenes: at eps = 1e5 every term is m / eps
PARTITION_EPS = 1e5
PARTITION_THETA = 0.7
N_DEEP = 32 * 8 ** 5 + 1                 # 7 levels
N_SIX = 32 * 8 ** 4 + 1                  # 6 levels
N_MASSIVE = 4096


@functools.lru_cache(maxsize=None)
def partition_scene(n, seed=47):
    """n positions in the unit cube, half uniform and half in Gaussian clumps (clipped to the cube), float32 -> (pos, the centre
    of the first clump)"""
    rs = np.random.RandomState(seed)
    pos = rs.uniform(0.0, 1.0, size=(n, 3))
    k = n // 2
    centres = rs.uniform(0.15, 0.85, size=(12, 3))
    pos[:k] = np.clip(centres[rs.randint(0, 12, k)] + rs.normal(size=(k, 3)) * (0.004 * 4.0 ** rs.randint(0, 3, k))[:, None], 0.0, 1.0)
    pos = pos[rs.permutation(n)].astype(f32)
    pos.setflags(write=False)
    return pos, centres[0]


# Where the mass sits in a call: the N_MASSIVE particles of the smallest cube about a point that holds that many; "clump": about the
# centre of a clump, in the 7-level scene a cube 0.0075 wide.  The kernel stores a node's c in float32, an absolute error of up to 2^-24 |c| per
# coordinate (the header of tsp_gravity_tree says so and tells the caller to centre sources that lie far from the origin relative
# to their separation): against the DIRECT sum that is within the rounding bound where the box is wide (0.19: 2^-24 |c| M against
# 64 * 2^-24 * M * 0.05), and far outside it for the clump unless the scene is moved so that the clump lies at the origin.
PARTITION_CASES = {"centre": ((0.5, 0.5, 0.5), False), "edge": ((0.02, 0.97, 0.5), False), "corner": ((0.8, 0.2, 0.9), False),
                   "clump at the origin": ("clump", True), "clump": ("clump", False)}


def partition_case(n, name, seed=53):
    """-> (src float32 (n, 3): partition_scene(n), moved by minus the clump's centre where the case says so; mass float32 (n,):
    uniform(0.5, 1.5) for the N_MASSIVE particles of the case's cube, 0 elsewhere)"""
    pos, clump = partition_scene(n)
    centre, at_origin = PARTITION_CASES[name]
    centre = clump if isinstance(centre, str) else np.asarray(centre)
    cheb = np.abs(pos.astype(np.float64) - centre).max(axis=1)
    inside = np.argpartition(cheb, N_MASSIVE)[:N_MASSIVE]
    mass = np.zeros(n, dtype=f32)
    mass[inside] = np.random.RandomState(seed + list(PARTITION_CASES).index(name)).uniform(0.5, 1.5, N_MASSIVE).astype(f32)
    src = (pos.astype(np.float64) - clump).astype(f32) if at_origin else pos
    return src, mass
