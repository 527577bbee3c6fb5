"""Time tsp_sph_sum (the SPH density) next to tsp_smoothing_lengths (k = 32) on positions of the synthetic snapshot.

    python tools/gpu_density_bench.py --n 1e7 [--kdtree] [--repeats 3]

Prints one JSON line: per call the wall times of the synchronous calls (host-to-device copies, sort, query kernel and
read-back included) over the repeats and their median, after a warm-up on 1e5 particles, both on one context with nothing
else on the GPU; the smoothing call's distances per query and the density call's candidates scanned and terms summed per query
and the share of its lanes' scan steps that had a candidate (the library's TOPSY_SMOOTH_STATS report).  The density call takes the smoothing lengths just computed and unit masses.
--kdtree also times the same
sum in float64 over scipy's cKDTree.query_ball_point(workers=16) -- the CPU figure -- and the largest relative difference.
Run one size per process, each under its own time limit; kernel times come from a separate rocprofv3 --kernel-trace --stats
run of the same command (the wall time less the kernels is the host-side share: upload, sort, download).
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


def timed(call):
    """(seconds, result, the per_query figures of the library's stderr report) of one call"""
    os.environ["TOPSY_SMOOTH_STATS"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        try:
            t0 = time.perf_counter()
            out = call()
            dt = time.perf_counter() - t0
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            os.environ.pop("TOPSY_SMOOTH_STATS", None)
        f.seek(0)
        report = f.read().decode(errors="replace")
    return dt, out, [float(v) for v in re.findall(r"(?:per_query|lane_use)=([0-9.]+)", report)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, required=True)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kdtree", action="store_true", help="also time query_ball_point(workers=16) on the same positions")
    args = ap.parse_args()
    from topsy_amd import _native
    n = int(args.n)
    x, y, z = synthetic_positions(n)
    mass = np.ones(n, dtype=np.float32)
    ctx = _native.Context(16, 2)
    wx, wy, wz = synthetic_positions(100_000, seed=7)
    _, wh, _ = timed(lambda: ctx.smoothing_lengths(wx, wy, wz, args.k))          # warm-up: code objects, sort plans
    timed(lambda: ctx.sph_sum(wx, wy, wz, wh, mass[:len(wx)]))
    t_h, t_rho, h, rho, dist, cand = [], [], None, None, None, None
    for _ in range(args.repeats):
        dt, h, dist = timed(lambda: ctx.smoothing_lengths(x, y, z, args.k))
        t_h.append(dt)
        dt, rho, cand = timed(lambda: ctx.sph_sum(x, y, z, h, mass))
        t_rho.append(dt)
    ctx.close()
    result = {"n": n, "k": args.k, "smoothing_s": t_h, "smoothing_s_median": float(np.median(t_h)), "distances_per_query": dist[-1] if dist else None,
              "density_s": t_rho, "density_s_median": float(np.median(t_rho)),
              "candidates_per_query": cand[0] if cand else None, "terms_per_query": cand[1] if len(cand or []) > 1 else None, "lane_use": cand[2] if len(cand or []) > 2 else None,
              "nan": int(np.isnan(rho).sum()), "rho_min": float(np.nanmin(rho)), "rho_max": float(np.nanmax(rho))}
    if args.kdtree:
        from scipy.spatial import cKDTree
        pos = np.stack([x, y, z], axis=1).astype(np.float64)
        h64 = h.astype(np.float64)
        t0 = time.perf_counter()
        lists = cKDTree(pos).query_ball_point(pos, 2.0 * h64, workers=16)
        result["kdtree_ball_s"] = time.perf_counter() - t0
        ref = np.empty(n)
        for i, js in enumerate(lists):
            u = np.sqrt(((pos[js] - pos[i]) ** 2).sum(axis=1)) / h64[i]
            w = np.where(u < 1, 1 - 1.5 * u ** 2 + 0.75 * u ** 3, np.where(u < 2, 0.25 * (2 - u) ** 3, 0.0))
            ref[i] = w.sum() / (np.pi * h64[i] ** 3)
        result["kdtree_total_s"] = time.perf_counter() - t0
        result["max_rel_diff_vs_kdtree"] = float(np.nanmax(np.abs(rho - ref) / ref))
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
