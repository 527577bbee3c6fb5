"""The scenes, the fixed targets and the caps of the truncation-quality tests of tsp_gravity_tree, shared by the CPU test of the
host model (test_gravity_tree_cpu.py) and the GPU test (test_gpu_gravity_tree.py).  Every reference is computed once per process."""
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
