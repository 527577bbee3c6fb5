"""Time the kinematic maps (TSP_MODE_KINEMATIC) on the synthetic snapshot generated on the device, with normal velocities
(sigma 100, bulk (50, -30, 20)) uploaded from the host.

    python tools/gpu_kinematics_bench.py --n 1e8 [--resolution 1024] [--repeats 5]

Prints one JSON line:
  * weight_ms / weight_gbps: the per-particle weight kernel (32 B per particle: 20 read, 12 written).  It runs inside the first
    render block after a change of the line of sight, so it is timed as the hipEvent time of a one-particle block with a new
    v_ref less that of the same block with the line of sight unchanged (medians); read_gbps is tsp_measure_read_bandwidth in
    the same process;
  * kinematic_ms / rgb_ms: whole frames of the same particles and camera (camera A at scale 200) in the two 4-channel modes,
    weights in place; kinematic_new_axis_ms: the kinematic frame after a change of the line of sight (= frame + weight pass);
  * moments_ms: tsp_velocity_moments at 1024^2 on its own context, wall clock around the call less the same call's device-to-host
    copy measured by tsp_read_image (both synchronous), and the wall-clock times themselves.
Run one size per process."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def camera_a(scale):
    M = np.eye(4, dtype=np.float32)
    M[:3, :3] /= scale
    M[2, :] = [0.0, 0.0, 0.5 / scale, 0.5]
    return M, np.float32(1.0 / scale)


def median(v):
    return float(np.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e8)
    ap.add_argument("--resolution", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    from topsy_amd import _native, kernel_lut
    n, R = int(args.n), args.resolution
    ctx = _native.Context(R, 4)
    ctx.set_kernel_mips(kernel_lut.kernel_mips())
    ctx.generate_synthetic(n, 0, n, 1337, 0.0, with_quantity=False, with_rgb=True)
    ctx.reorder_spatial(max(8, -(-n // (1 << 22))), 1337)
    rng = np.random.default_rng(5)
    vel = [rng.standard_normal(n, dtype=np.float32) * np.float32(100.0) + np.float32(b) for b in (50.0, -30.0, 20.0)]
    ctx.upload_velocities(*vel)
    del vel
    M, sf = camera_a(200.0)
    axis, kin, rgb = (0.0, 0.0, 1.0), _native.MODE_KINEMATIC, _native.MODE_RGB
    one = ([0], [1])

    ctx.set_line_of_sight(axis, (0.0, 0.0, 0.0))
    ctx.render(M, sf, *one, mode=kin)                     # cold: allocates the weights and the workspace
    changed, same = [], []
    for k in range(args.repeats):
        ctx.set_line_of_sight(axis, (float(k + 1), 0.0, 0.0))
        changed.append(ctx.render(M, sf, *one, mode=kin))
        same.append(ctx.render(M, sf, *one, mode=kin))
    weight_ms = median(changed) - median(same)
    read_gbps = ctx.measure_read_bandwidth(1 << 30, 10)

    ctx.render(M, sf, mode=kin)                           # warm: the record lists grow to the frame's need
    ctx.render(M, sf, mode=rgb)
    frames = {"kinematic_ms": [], "rgb_ms": [], "kinematic_new_axis_ms": []}
    for k in range(args.repeats):
        ctx.render(M, sf, mode=kin)                       # (weights of this line of sight in place)
        frames["kinematic_ms"].append(ctx.render(M, sf, mode=kin))
        ctx.render(M, sf, mode=rgb)
        frames["rgb_ms"].append(ctx.render(M, sf, mode=rgb))
        ctx.render(M, sf, *one, mode=kin)                 # back to kinematic weights, outside the timed frame
        ctx.set_line_of_sight(axis, (0.0, float(k + 1), 0.0))
        frames["kinematic_new_axis_ms"].append(ctx.render(M, sf, mode=kin))
    stats = ctx.stats()
    ctx.close()

    small = _native.Context(1024, 4)
    small.set_kernel_mips(kernel_lut.kernel_mips())
    small.generate_synthetic(100_000, 0, 100_000, 1337, 0.0, with_quantity=False, with_rgb=False)
    small.upload_velocities(*(np.zeros(100_000, dtype=np.float32) for _ in range(3)))
    small.set_line_of_sight(axis)
    small.render(M, sf, mode=kin)
    small.velocity_moments()
    wall, copy = [], []
    for _ in range(max(args.repeats, 5)):
        t0 = time.perf_counter()
        small.velocity_moments()
        t1 = time.perf_counter()
        small.read_image()
        t2 = time.perf_counter()
        wall.append((t1 - t0) * 1e3)
        copy.append((t2 - t1) * 1e3)
    small.close()

    print(json.dumps({"n": n, "resolution": R, "repeats": args.repeats,
                      "weight_block_changed_ms": changed, "weight_block_same_ms": same, "weight_ms": weight_ms,
                      "weight_gbps": 32.0 * n / (weight_ms * 1e-3) / 1e9 if weight_ms > 0 else None, "read_gbps": read_gbps,
                      **{k: v for k, v in frames.items()}, **{k + "_median": median(v) for k, v in frames.items()},
                      "n_small": stats["n_small"], "n_mid": stats["n_mid"], "n_huge": stats["n_huge"],
                      "moments_wall_ms": wall, "moments_copy_ms": copy, "moments_ms": median(wall) - median(copy)}), flush=True)


if __name__ == "__main__":
    main()
