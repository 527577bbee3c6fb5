"""Time tsp_smoothing_lengths (k = 32) on positions of the synthetic snapshot, next to scipy's cKDTree(workers=16).

    python tools/gpu_smoothing_bench.py --n 1e7 [--kdtree] [--repeats 3]

Prints one JSON line per size: the wall time of the synchronous call (host-to-device copies, sort, search and read-back
included), the mean number of distances the search evaluated per query (the library's TOPSY_SMOOTH_STATS report: the window
of 2k + 1 that bounds the search plus every candidate of the cells it scans), and with --kdtree the kd-tree's build + query
time on the same positions and the largest relative difference.  Run one size per process, each under its own time limit;
kernel times come from a separate rocprofv3 --kernel-trace --stats run of the same command.
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


def synthetic_positions(n, seed=1337):
    """x, y, z of an n-particle synthetic snapshot, generated on the device and downloaded."""
    from topsy_amd import _native
    ctx = _native.Context(16, 2)
    try:
        ctx.generate_synthetic(n, 0, n, seed, 0.0)
        d = ctx.download_particles(("x", "y", "z"))
    finally:
        ctx.close()
    return d["x"], d["y"], d["z"]


def timed_call(ctx, x, y, z, k):
    """(seconds, distances per query) of one smoothing_lengths call; the library's stderr report is read through a file."""
    os.environ["TOPSY_SMOOTH_STATS"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        try:
            t0 = time.perf_counter()
            h = ctx.smoothing_lengths(x, y, z, k)
            dt = time.perf_counter() - t0
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            os.environ.pop("TOPSY_SMOOTH_STATS", None)
        f.seek(0)
        report = f.read().decode(errors="replace")
    m = re.findall(r"per_query=([0-9.]+)", report)
    return dt, float(m[-1]) if m else None, h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, required=True)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kdtree", action="store_true", help="also time cKDTree(workers=16) on the same positions")
    args = ap.parse_args()
    from topsy_amd import _native
    n = int(args.n)
    x, y, z = synthetic_positions(n)
    ctx = _native.Context(16, 2)
    wx, wy, wz = synthetic_positions(100_000, seed=7)
    timed_call(ctx, wx, wy, wz, args.k)                        # warm-up: code objects, sort plans
    times, per_query, h = [], None, None
    for _ in range(args.repeats):
        dt, per_query, h = timed_call(ctx, x, y, z, args.k)
        times.append(dt)
    ctx.close()
    result = {"n": n, "k": args.k, "gpu_s": times, "gpu_s_min": min(times), "distances_per_query": per_query,
              "nan": int(np.isnan(h).sum())}
    if args.kdtree:
        from scipy.spatial import cKDTree
        pos = np.stack([x, y, z], axis=1).astype(np.float64)
        t0 = time.perf_counter()
        d, _ = cKDTree(pos).query(pos, k=args.k, workers=16)
        result["kdtree_s"] = time.perf_counter() - t0
        ref = 0.5 * d[:, -1]
        result["max_rel_diff_vs_kdtree"] = float(np.max(np.abs(h - ref) / np.maximum(ref, 1e-300)))
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
