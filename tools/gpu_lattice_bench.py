"""Time tsp_sph_sample_lattice (SPH fields on a lattice) next to tsp_sph_sum on the same particles.

    python tools/gpu_lattice_bench.py [--n 1e6] [--k 32] [--repeats 3] [--grid 128] [--slice 1024]

The particles are the clustered scene of the velocity-gradient figures in DESIGN.md (half in 50 clumps, half uniform in the unit
cube; the generator of tests/test_gpu_smoothing.py::_clustered, seed 11), random masses.  Timed, all on one context after a
warm-up on 1e5 particles: tsp_smoothing_lengths + tsp_sph_sum at the particles (the yardstick), the density on a grid^3 lattice
of cell centres of the unit cube, the same with four fields, and the density on a slice^2 lattice through z = 0.5.  Prints one
JSON line: per case the wall times of the synchronous calls and the library's TOPSY_SMOOTH_STATS report of the last repeat -- the stage times (index build with the
uploads, k-NN step, sum step, read-back; the stream is synchronised between the stages while the report is on), the distances
of the search, the candidates scanned and the terms summed per query, and the share of the lanes' scan steps that had a
candidate.  Kernel times come from a separate rocprofv3 --kernel-trace --stats run of the same command."""
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


def clustered(n, seed):
    rs = np.random.RandomState(seed)
    n_cl = n // 2
    centres = rs.uniform(0.1, 0.9, size=(50, 3))
    cl = centres[rs.randint(0, 50, size=n_cl)] + rs.normal(size=(n_cl, 3)) * np.exp(rs.uniform(np.log(1e-3), np.log(3e-2), size=(n_cl, 1)))
    return np.concatenate([cl, rs.uniform(0, 1, size=(n - n_cl, 3))]).astype(np.float32)


def timed(call):
    """(seconds, result, the library's stderr report as a dict of its name=number pairs) of one call"""
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
    pairs = re.findall(r"(\w+)=([0-9.eE+-]+)(?=\s|$)", report)
    stats = {}
    for name, v in pairs:                                   # per_query appears once per counter: keep them apart
        key = name
        while key in stats:
            key += "_"
        stats[key] = float(v)
    return dt, out, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e6)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--slice", type=int, default=1024)
    args = ap.parse_args()
    from topsy_amd import _native
    n, k = int(args.n), args.k
    pos = clustered(n, 11)
    x, y, z = (np.ascontiguousarray(pos[:, a]) for a in range(3))
    rs = np.random.RandomState(5)
    mass = rs.uniform(0.5, 2.0, size=n).astype(np.float32)
    more = [rs.uniform(0.5, 2.0, size=n).astype(np.float32) for _ in range(3)]

    def cells(m, nw=None):
        s = 1.0 / m
        return dict(origin=(0.5 * s, 0.5 * s, 0.5 * s if nw is None else 0.5), du=(s, 0, 0), dv=(0, s, 0), dw=(0, 0, s),
                    shape=(m, m, m if nw is None else nw))

    ctx = _native.Context(16, 2)
    w = clustered(100_000, 7)
    wh = ctx.smoothing_lengths(w[:, 0], w[:, 1], w[:, 2], k)                      # warm-up: code objects, sort plans
    ctx.sph_sum(w[:, 0], w[:, 1], w[:, 2], wh, mass[:len(w)])
    for f in ([mass[:len(w)]], [a[:len(w)] for a in [mass] + more]):
        ctx.sph_sample_lattice(w[:, 0], w[:, 1], w[:, 2], f, k, None, **cells(16))
        ctx.sph_sample_lattice(w[:, 0], w[:, 1], w[:, 2], f, k, None, **cells(64, 1))

    result = {"n": n, "k": k, "grid": args.grid, "slice": args.slice}
    h = ctx.smoothing_lengths(x, y, z, k)
    cases = {
        "sph_sum_at_particles": lambda: ctx.sph_sum(x, y, z, h, mass),
        "grid": lambda: ctx.sph_sample_lattice(x, y, z, [mass], k, None, **cells(args.grid)),
        "grid_four_fields": lambda: ctx.sph_sample_lattice(x, y, z, [mass] + more, k, None, **cells(args.grid)),
        "slice": lambda: ctx.sph_sample_lattice(x, y, z, [mass], k, None, **cells(args.slice, 1)),
    }
    outs = {}
    for name, call in cases.items():
        times, stats = [], {}
        for _ in range(args.repeats):
            dt, outs[name], stats = timed(call)
            times.append(dt)
        result[name] = {"wall_s": times, "wall_s_median": float(np.median(times)), "report": stats}
    ctx.close()
    rho = outs["grid"][1][0]
    result["grid_rho"] = {"nan": int(np.isnan(rho).sum()), "min": float(np.nanmin(rho)), "max": float(np.nanmax(rho)),
                          "mean": float(np.nanmean(rho.astype(np.float64))), "mean_particle_density": float(mass.sum())}
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
