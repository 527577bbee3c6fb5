"""Time tsp_radial_profile (binned shell sums: radial profiles) next to pass B of tsp_sphere_moments over the same sphere and arrays,
on the positions of the synthetic snapshot, unit masses, with velocities of a rotation about z plus noise.

    python tools/gpu_profile_bench.py --n 1e7 [--bins 100] [--repeats 3]

The sphere is centred on the mean position and reaches to the median distance from it: half the particles are binned.  The same
particles are summed in the generator's order (every index range is a uniform sample of the snapshot: no block is skipped and a
wave's 64 particles fall into many bins) and in the spatial order of tsp_reorder_spatial with one stratum (Morton order: compact
blocks, few bins per wave).  Prints one JSON line: per order the profile's kernel time (hipEvent pair, from the library's
TOPSY_PROFILE_STATS report) of every repeat and the median, the blocks it read, pass B's kernel time and blocks from
TOPSY_ORIENT_STATS likewise, and the ratio of the medians.  A warm-up on 1e5 particles comes first.  Run one size per process.
"""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gpu_center_bench import synthetic_positions  # noqa: E402
from gpu_orient_bench import rotation_velocities, timed  # noqa: E402  (timed sets TOPSY_ORIENT_STATS and captures stderr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, required=True)
    ap.add_argument("--bins", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--geometry", type=int, default=0)
    args = ap.parse_args()
    from topsy_amd import _native
    n = int(args.n)
    os.environ["TOPSY_PROFILE_STATS"] = "1"
    ctx = _native.Context(16, 2)
    wx, wy, wz = synthetic_positions(100_000, False, seed=7)
    wm = np.ones(len(wx), dtype=np.float32)
    timed(lambda: (ctx.sphere_moments(wx, wy, wz, wm, vel=rotation_velocities(wx, wy), r=20.0, r_vel=4.0),
                   ctx.radial_profile(wx, wy, wz, wm, vel=rotation_velocities(wx, wy), edges=np.linspace(0.0, 20.0, args.bins + 1),
                                      geometry=args.geometry)))       # warm-up: code objects
    mass = np.ones(n, dtype=np.float32)
    result = {"n": n, "bins": args.bins, "geometry": args.geometry, "repeats": args.repeats}
    for label, spatial in (("shuffled", False), ("sorted", True)):
        x, y, z = synthetic_positions(n, spatial)
        vel = rotation_velocities(x, y)
        center = np.array([x.mean(dtype=np.float64), y.mean(dtype=np.float64), z.mean(dtype=np.float64)])
        r = float(np.median(np.sqrt((x - center[0]) ** 2 + (y - center[1]) ** 2 + (z - center[2]) ** 2)))
        edges = np.linspace(0.0, r, args.bins + 1)
        profile_ms, pass_b_ms, out, report = [], [], None, ""
        for _ in range(args.repeats):
            _, mo, report = timed(lambda: ctx.sphere_moments(x, y, z, mass, vel=vel, center=center, r=r, r_vel=r / 5))
            b = re.search(r"pass=B kernel_ms=([0-9.]+) blocks_read=(\d+)", report)
            pass_b_ms.append(float(b.group(1)))
            _, out, report = timed(lambda: ctx.radial_profile(x, y, z, mass, vel=vel, edges=edges, geometry=args.geometry,
                                                              center=center, v_cen=mo["v_cen"]))
            p = re.search(r"kernel_ms=([0-9.]+) blocks_read=(\d+)", report)
            profile_ms.append(float(p.group(1)))
        head = re.search(r"blocks=(\d+) workgroups=(\d+) tables=(\d+) upload_ms=([0-9.]+) prepare_ms=([0-9.]+)", report)
        result[label] = {"radius": r, "blocks": int(head.group(1)), "workgroups": int(head.group(2)), "tables": int(head.group(3)),
                         "upload_ms": float(head.group(4)), "prepare_ms": float(head.group(5)), "profile_kernel_ms": profile_ms,
                         "profile_kernel_ms_median": float(np.median(profile_ms)), "profile_blocks_read": int(p.group(2)),
                         "pass_B_kernel_ms": pass_b_ms, "pass_B_kernel_ms_median": float(np.median(pass_b_ms)),
                         "pass_B_blocks_read": int(b.group(2)), "n_binned": out["n_binned"], "n_inside_pass_B": mo["n_inside"],
                         "profile_over_pass_B": float(np.median(profile_ms) / np.median(pass_b_ms))}
    ctx.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
