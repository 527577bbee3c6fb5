"""Time tsp_histogram_2d (weighted 2-D histograms: phase diagrams) on three scenes that differ only in how the particles crowd into
cells, next to numpy.histogram2d of the same three planes on the host.

    python tools/gpu_phase_bench.py --n 1e7 [--bins 256 1024] [--repeats 3]

Per table size (bins x bins, logarithmic edges) and scene, with weights and values (count and three float64 planes):
  * spread:   log-uniform over the whole table;
  * ridge:    a narrow lognormal ridge, rho-T like: most particles share a few cells;
  * one_cell: every particle in a single cell.
Reported per repeat and as medians: the device time of the key pass, the sort and the reduction (hipEvent pairs, from the library's
TOPSY_HIST2D_STATS report), their sum kernel_ms, upload_ms (the host-to-device copies) and call_ms (the whole call, wall clock,
results back on the host).  The check of the no-serial-walk rule is the pair of ratios ridge / spread and one_cell / spread of
kernel_ms on the same table.  numpy_ms is numpy.histogram2d called three times (w, w v, w v v) on this machine's CPUs, once per
scene.  A warm-up on 1e5 particles comes first.  Prints one JSON line.  Run with nothing else on the GPU."""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gpu_orient_bench import timed  # noqa: E402  (captures the library's stderr report)

f32 = np.float32
LO, HI = 1e-3, 1e3


def scenes(n, edges, seed=5):
    rs = np.random.RandomState(seed)
    lo, hi = np.log(LO), np.log(HI)
    out = {"spread": (np.exp(rs.uniform(lo, hi, n)), np.exp(rs.uniform(lo, hi, n)))}
    t = rs.normal(0.0, 1.2, n)
    out["ridge"] = (np.exp(t), np.exp(0.6 * t + rs.normal(0.0, 0.05, n)))
    i = len(edges) // 2
    a, b = edges[i] * 1.001, edges[i + 1] * 0.999
    out["one_cell"] = (rs.uniform(a, b, n), rs.uniform(a, b, n))
    return {k: (x.astype(f32), y.astype(f32)) for k, (x, y) in out.items()}, rs.uniform(0.5, 2.0, n).astype(f32), rs.normal(0.0, 100.0, n).astype(f32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e7)
    ap.add_argument("--bins", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-numpy", action="store_true")
    args = ap.parse_args()
    from topsy_amd import _native, phase
    n = int(args.n)
    os.environ["TOPSY_HIST2D_STATS"] = "1"
    ctx = _native.Context(16, 2)
    rs = np.random.RandomState(0)
    warm = [rs.uniform(0.0, 1.0, 100_000).astype(f32) for _ in range(4)]
    ctx.histogram_2d(*warm, edges_x=np.linspace(0.0, 1.0, 65), edges_y=np.linspace(0.0, 1.0, 65))       # warm-up: code objects
    result = {"n": n, "repeats": args.repeats, "cpus": len(os.sched_getaffinity(0)), "tables": {}}
    for bins in args.bins:
        edges = phase.hist_edges(LO, HI, bins, log=True)
        sc, w, v = scenes(n, edges)
        table = {}
        for label, (x, y) in sc.items():
            rows = []
            for _ in range(args.repeats):
                _, out, report = timed(lambda: ctx.histogram_2d(x, y, w, v, edges_x=edges, edges_y=edges))
                r = re.search(r"upload_ms=([0-9.]+) key_ms=([0-9.]+) sort_ms=([0-9.]+) reduce_ms=([0-9.]+) call_ms=([0-9.]+)", report)
                rows.append([float(g) for g in r.groups()])
            levels = int(re.search(r"levels=(\d+)", report).group(1))
            med = np.median(np.array(rows), axis=0)
            entry = {"upload_ms": med[0], "key_ms": med[1], "sort_ms": med[2], "reduce_ms": med[3], "call_ms": med[4],
                     "kernel_ms": float(med[1] + med[2] + med[3]), "kernel_ms_repeats": [r[1] + r[2] + r[3] for r in rows],
                     "call_ms_repeats": [r[4] for r in rows], "levels": levels, "n_binned": out["n_binned"],
                     "largest_cell": int(out["count"].max()), "cells_occupied": int(np.count_nonzero(out["count"]))}
            if not args.no_numpy:
                x64, y64, w64, v64 = (a.astype(np.float64) for a in (x, y, w, v))
                t0 = time.perf_counter()
                planes = [np.histogram2d(y64, x64, bins=(edges, edges), weights=t)[0] for t in (w64, w64 * v64, w64 * v64 * v64)]
                entry["numpy_ms"] = 1e3 * (time.perf_counter() - t0)
                entry["numpy_agrees"] = bool(np.allclose(out["sums"], np.array(planes), rtol=1e-9, atol=1e-6 * float(np.abs(planes[2]).max())))
            table[label] = {k: (float(val) if isinstance(val, np.floating) else val) for k, val in entry.items()}
        for label in ("ridge", "one_cell"):
            table[label]["kernel_over_spread"] = table[label]["kernel_ms"] / table["spread"]["kernel_ms"]
            table[label]["call_over_spread"] = table[label]["call_ms"] / table["spread"]["call_ms"]
        result["tables"][f"{bins}x{bins}"] = table
    ctx.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
