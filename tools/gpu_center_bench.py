"""Time tsp_shrink_sphere_center (the shrinking-sphere centre) on the positions of the synthetic snapshot, unit masses.

    python tools/gpu_center_bench.py --n 1e8 [--repeats 3]

The same positions are centred twice: in the generator's order (every index range is a uniform sample of the snapshot, so no
block of 1024 consecutive particles can be skipped) and in the spatial order of tsp_reorder_spatial with one stratum (Morton
order: the blocks are compact and most are skipped once the sphere is small).  Prints one JSON line: per order the wall time of
the synchronous host-array call over the repeats and its median, and from the library's TOPSY_CENTER_STATS report of the last
repeat the upload and preparation times, every pass's kernel time (hipEvent pair), wall time (launch, final sum and read-back
included) and the blocks it read; the first pass's achieved rate, 16 bytes x n / kernel time, beside the streaming-read peak
tsp_measure_read_bandwidth reports in the same process.  A warm-up on 1e5 particles comes first.  Run one size per process.
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


def synthetic_positions(n, spatial_order, seed=1337):
    """x, y, z of the n-particle synthetic snapshot, generated on the device and downloaded; spatial_order: Morton-sorted."""
    from topsy_amd import _native
    ctx = _native.Context(16, 2)
    try:
        ctx.generate_synthetic(n, 0, n, seed, 0.0)
        if spatial_order:
            ctx.reorder_spatial(1, seed)
        d = ctx.download_particles(("x", "y", "z"))
    finally:
        ctx.close()
    return d["x"], d["y"], d["z"]


def timed(call):
    """(seconds, result, the library's stderr report) of one call"""
    os.environ["TOPSY_CENTER_STATS"] = "1"
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
            os.environ.pop("TOPSY_CENTER_STATS", None)
        f.seek(0)
        report = f.read().decode(errors="replace")
    return dt, out, report


def parse_report(report, n):
    head = re.search(r"blocks=(\d+) workgroups=(\d+) upload_ms=([0-9.]+) prepare_ms=([0-9.]+)", report)
    passes = [(float(a), float(b), int(c), int(d)) for a, b, c, d in
              re.findall(r"kernel_ms=([0-9.]+) wall_ms=([0-9.]+) blocks_read=(\d+) inside=(\d+)", report)]
    out = {"blocks": int(head.group(1)), "workgroups": int(head.group(2)), "upload_ms": float(head.group(3)),
           "prepare_ms": float(head.group(4)), "pass_kernel_ms": [p[0] for p in passes], "pass_wall_ms": [p[1] for p in passes],
           "pass_blocks_read": [p[2] for p in passes], "pass_inside": [p[3] for p in passes]}
    if passes:
        full = [p for p in passes if p[2] == out["blocks"]]
        out["first_pass_gbps"] = 16.0 * n / (passes[0][0] * 1e-3) / 1e9
        out["full_passes"] = len(full)
        out["passes_kernel_ms_total"] = float(sum(p[0] for p in passes))
        out["passes_wall_ms_total"] = float(sum(p[1] for p in passes))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, required=True)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    from topsy_amd import _native
    n = int(args.n)
    result = {"n": n}
    ctx = _native.Context(16, 2)
    wx, wy, wz = synthetic_positions(100_000, False, seed=7)
    timed(lambda: ctx.shrink_sphere_center(wx, wy, wz, np.ones(len(wx), dtype=np.float32)))      # warm-up: code objects
    result["read_bandwidth_gbps"] = ctx.measure_read_bandwidth()
    mass = np.ones(n, dtype=np.float32)
    for label, spatial in (("shuffled", False), ("sorted", True)):
        x, y, z = synthetic_positions(n, spatial)
        times, report, out = [], "", None
        for _ in range(args.repeats):
            dt, out, report = timed(lambda: ctx.shrink_sphere_center(x, y, z, mass))
            times.append(dt)
        center, info = out
        result[label] = dict(parse_report(report, n), call_s=times, call_s_median=float(np.median(times)),
                             center=[float(v) for v in center], **info)
    ctx.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
