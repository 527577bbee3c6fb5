"""Time tsp_fof_groups (friends-of-friends groups) with and without the same-cell shortcut, next to scipy on the CPU.

    python tools/gpu_fof_bench.py --case synthetic --n 1e7 [--cpu] [--repeats 3]
    python tools/gpu_fof_bench.py --case clumps --n 1e7

Cases: "synthetic", the positions of the synthetic snapshot (open box, linking length 0.2 mean separations of the bounding
box); "clumps", the five-clump scene of tests/test_fof_cpu.py scaled to n particles (periodic unit box, linking length
0.2 n^(-1/3)); "core", a ball of radius half a linking length holding a tenth of the particles over a uniform background
(the middle of a massive halo: every member has the whole ball inside its linking length).  Prints one JSON line per mode
("shortcut": TOPSY_FOF_SHORTCUT=1, forced; "no_shortcut": =0; "auto": the library's own choice): the wall time of the
synchronous call (host-to-device copies, the index's sort, linking, ranking and read-back included) and the library's
TOPSY_SMOOTH_STATS report -- the octree level of the shortcut cells, the candidates tested per query, the hooks that joined two
trees, the share of the lanes' scan steps that had a candidate, the groups found.  Both modes must return the same labels.
--cpu adds scipy's cKDTree.query_pairs + connected_components on the same positions (query_pairs runs on one thread: scipy
gives it no workers argument; the tree is built once) and checks the group sizes against it.  Run one case per process, each
under its own time limit; kernel times come from a separate rocprofv3 --kernel-trace --stats run of the same command.
"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.gpu_smoothing_bench import synthetic_positions      # noqa: E402

CLUMPS = (((0.25, 0.62, 0.4), 0.02, 0.3), ((0.7, 0.3, 0.55), 0.012, 0.15), ((0.98, 0.5, 0.02), 0.015, 0.1),
          ((0.5, 0.5, 0.9), 0.008, 0.04), ((0.1, 0.1, 0.1), 0.004, 0.0075))


def clumps_positions(n, seed=5):
    rs = np.random.RandomState(seed)
    parts = [(np.asarray(c) + s * rs.normal(size=(int(f * n), 3))).astype(np.float32) for c, s, f in CLUMPS]
    parts.append(rs.uniform(size=(n - sum(len(p) for p in parts), 3)).astype(np.float32))
    pos = np.mod(np.concatenate(parts), np.float32(1.0))
    return pos[rs.permutation(n)]


def timed_call(ctx, x, y, z, ll, period, shortcut):
    """(seconds, labels, info, the library's report as a dict) of one fof_groups call; stderr is read through a file."""
    os.environ["TOPSY_SMOOTH_STATS"] = "1"
    if shortcut is not None:
        os.environ["TOPSY_FOF_SHORTCUT"] = "1" if shortcut else "0"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        try:
            t0 = time.perf_counter()
            labels, info = ctx.fof_groups(x, y, z, ll, period, 20)
            dt = time.perf_counter() - t0
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            os.environ.pop("TOPSY_SMOOTH_STATS", None)
            os.environ.pop("TOPSY_FOF_SHORTCUT", None)
        f.seek(0)
        report = f.read().decode(errors="replace")
    line = [l for l in report.splitlines() if l.startswith("tsp_fof_groups:")]
    stats = {k: float(v) for k, v in re.findall(r"(\w+)=(-?[0-9.]+)", line[-1])} if line else {}
    return dt, labels, info, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("synthetic", "clumps", "core"), required=True)
    ap.add_argument("--n", type=float, required=True)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu", action="store_true", help="also time scipy's query_pairs + connected_components")
    args = ap.parse_args()
    from topsy_amd import _native, loader
    n = int(args.n)
    if args.case == "synthetic":
        x, y, z = synthetic_positions(n)
        pos = np.stack([x, y, z], axis=1)
        period = 0.0
        ll = loader.fof_linking_length(pos, 0.2, 0.0)
    elif args.case == "clumps":
        pos = clumps_positions(n)
        x, y, z = (np.ascontiguousarray(pos[:, a]) for a in range(3))
        period = 1.0
        ll = 0.2 * n ** (-1.0 / 3.0)
    else:
        rs = np.random.RandomState(13)
        period = 1.0
        ll = 0.2 * n ** (-1.0 / 3.0)
        v = rs.normal(size=(n // 10, 3))
        v *= (0.5 * ll * rs.uniform(size=(len(v), 1)) ** (1.0 / 3.0)) / np.linalg.norm(v, axis=1, keepdims=True)
        pos = np.concatenate([0.5 + v, rs.uniform(size=(n - len(v), 3))]).astype(np.float32)
        pos = pos[rs.permutation(n)]
        x, y, z = (np.ascontiguousarray(pos[:, a]) for a in range(3))
    ctx = _native.Context(16, 2)
    w = clumps_positions(100_000, seed=7)
    timed_call(ctx, w[:, 0], w[:, 1], w[:, 2], 0.004, 1.0, True)          # warm-up: code objects, sort plans
    labels = {}
    for mode in ("shortcut", "no_shortcut", "auto"):
        times = []
        for _ in range(args.repeats):
            dt, labels[mode], info, stats = timed_call(ctx, x, y, z, ll, period, {"shortcut": True, "no_shortcut": False, "auto": None}[mode])
            times.append(dt)
        print(json.dumps({"case": args.case, "n": n, "mode": mode, "linking_length": ll, "period": period, "gpu_s": times,
                          "gpu_s_min": min(times), "info": info, "report": stats}), flush=True)
    ctx.close()
    assert np.array_equal(labels["shortcut"], labels["no_shortcut"]), "the shortcut changed the labels"
    assert np.array_equal(labels["shortcut"], labels["auto"]), "the library's own choice changed the labels"
    if args.cpu:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        from scipy.spatial import cKDTree
        p64 = pos.astype(np.float64)
        if period > 0:
            p64 = np.mod(p64, period)
            p64[p64 >= period] = 0.0
        t0 = time.perf_counter()
        pairs = cKDTree(p64, boxsize=period or None).query_pairs(float(np.float32(ll)), output_type="ndarray")
        t1 = time.perf_counter()
        graph = coo_matrix((np.ones(len(pairs), dtype=np.int8), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
        _, comp = connected_components(graph, directed=False)
        t2 = time.perf_counter()
        sizes = np.sort(np.bincount(comp))[::-1]
        gpu_sizes = np.bincount(labels["shortcut"][labels["shortcut"] > 0])[1:]
        print(json.dumps({"case": args.case, "n": n, "mode": "scipy", "pairs": int(len(pairs)), "query_pairs_s": t1 - t0,
                          "connected_components_s": t2 - t1, "cpu_s": t2 - t0,
                          "largest_sizes_agree": bool(np.array_equal(sizes[:3], gpu_sizes[:3]))}), flush=True)


if __name__ == "__main__":
    main()
