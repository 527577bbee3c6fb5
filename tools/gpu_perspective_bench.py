"""Time the perspective camera (tsp_project_perspective) on the synthetic snapshot generated on the device in two contexts.

    python tools/gpu_perspective_bench.py --n 1e8 [--resolution 1024] [--repeats 7] [--fov 60] [--rgb]

Prints one JSON line:
  * project_ms / project_gbps: the projection pass.  The call is synchronous (it returns when the pass has finished), so it is
    timed by the wall clock around it (median; the launch and the wait add some tens of microseconds, which count against it);
    the bytes are the pass's own traffic, 44 per particle (20 read, 24 written; 68 with --rgb) plus 32 per 512-particle block;
    read_gbps is tsp_measure_read_bandwidth in the same process, the yardstick;
  * ortho_ms / perspective_ms: a whole frame (every particle, one block) of the orthographic view at camera A (scale 200) and of
    the perspective view of the same snapshot at the same scale, the transformed snapshot in place, by the render call's own
    hipEvent time (medians); perspective_frame_ms adds the projection: what a fly-through pays per frame;
  * the class counts and the chunk-culled particles of both frames.
A warm-up on 1e5 particles comes first.  Run one size per process."""
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


def contexts(native, kernel_lut, n, R, rgb):
    out = []
    for _ in range(2):
        ctx = native.Context(R, 4 if rgb else 2)
        ctx.set_kernel_mips(kernel_lut.kernel_mips())
        ctx.generate_synthetic(n, 0, n, 1337, 0.0, with_quantity=False, with_rgb=rgb)
        ctx.reorder_spatial(max(8, -(-n // (1 << 22))), 1337)
        out.append(ctx)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e8)
    ap.add_argument("--resolution", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--fov", type=float, default=60.0)
    ap.add_argument("--rgb", action="store_true")
    args = ap.parse_args()
    from topsy_amd import _native, kernel_lut, perspective
    n, R, scale = int(args.n), args.resolution, 200.0
    distance = perspective.fov_to_distance(scale, args.fov)
    near, far = distance * 1e-3, distance + scale
    cam = (np.eye(3), np.zeros(3), distance, near)
    mode = _native.MODE_RGB if args.rgb else _native.MODE_WEIGHTED

    src, dst = contexts(_native, kernel_lut, 100_000, 64, args.rgb)          # warm-up: code objects, first launches
    src.project_perspective(dst, *cam)
    src.close()
    dst.close()

    src, dst = contexts(_native, kernel_lut, n, R, args.rgb)
    src.project_perspective(dst, *cam)                                         # cold: allocates dst's weights and bounds
    project = []
    for k in range(args.repeats):
        moved = (np.eye(3), np.array([0.0, 0.0, 0.01 * k]), distance, near)
        t0 = time.perf_counter()
        src.project_perspective(dst, *moved)
        project.append((time.perf_counter() - t0) * 1e3)
    read_gbps = src.measure_read_bandwidth(1 << 30, 10)
    nbytes = (68.0 if args.rgb else 44.0) * n + 32.0 * (-(-n // 512))

    M_o, sf = camera_a(scale)
    M_p, _ = perspective.clip_matrix(scale, distance, near, far)
    src.project_perspective(dst, *cam)
    src.render(M_o, sf, mode=mode)                                             # warm: the record lists grow to the frame's need
    dst.render(M_p, sf, mode=mode)
    ortho = [src.render(M_o, sf, mode=mode) for _ in range(args.repeats)]
    persp = [dst.render(M_p, sf, mode=mode) for _ in range(args.repeats)]
    st_o, st_p = src.stats(), dst.stats()
    src.close()
    dst.close()

    keys = ("n_small", "n_mid", "n_huge", "n_culled", "n_chunk_culled")
    print(json.dumps({"n": n, "resolution": R, "fov": args.fov, "rgb": args.rgb, "repeats": args.repeats,
                      "project_wall_ms": project, "project_ms": median(project), "project_bytes": nbytes,
                      "project_gbps": nbytes / (median(project) * 1e-3) / 1e9, "read_gbps": read_gbps,
                      "ortho_frame_ms": ortho, "perspective_render_ms": persp, "ortho_ms": median(ortho),
                      "perspective_ms": median(persp), "perspective_frame_ms": median(persp) + median(project),
                      "ortho_counts": {k: st_o[k] for k in keys}, "perspective_counts": {k: st_p[k] for k in keys}}), flush=True)


if __name__ == "__main__":
    main()
