"""Time the spectral cube (tsp_spectral_cube) against the only other way to a cube, ceil(n_channels / 3) TSP_MODE_RGB frames with a
channel response folded into the colours, on the synthetic snapshot generated on the device with normal velocities (sigma 100,
bulk (50, -30, 20)) uploaded from the host.

    python tools/gpu_cube_bench.py --n 1e6 [--resolution 512] [--channels 64,256] [--repeats 3] [--baseline-only]

The band is (-400, 400) and sigma_v = dv, so a line reaches about eleven channels.  Prints one JSON line per channel count:
  * cube_ms: wall clock around the raw tsp_spectral_cube call into a buffer that is already resident in host memory (the call ends
    in a synchronous copy of the cube to the host, which is part of what a caller waits for); read_image_ms: tsp_read_image of
    the R x R x 4 image in the same process, for the rate of such copies; slices: how many slices the call took;
    cube_sum_over_surface_density_sum: the cube's total over that of a kinematic frame's S (the share of the mass inside the band);
  * rgb_frame_ms: the hipEvent time of one whole TSP_MODE_RGB frame of the same particles and camera; baseline_ms = that times
    ceil(n_channels / 3) -- no upload of the re-weighted colours and no read-back is counted, which favours the baseline;
  * ratio = baseline_ms / cube_ms.
--baseline-only needs nothing of the cube: it runs on a checkout that has no tsp_spectral_cube.  Run one size per process."""
import argparse
import ctypes
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
    ap.add_argument("--n", type=float, default=1e6)
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--channels", default="64,256")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline-only", action="store_true")
    args = ap.parse_args()
    from topsy_amd import _native, kernel_lut
    n, R = int(args.n), args.resolution
    lib = _native.load_library()
    ctx = _native.Context(R, 4)
    ctx.set_kernel_mips(kernel_lut.kernel_mips())
    ctx.generate_synthetic(n, 0, n, 1337, 0.0, with_quantity=False, with_rgb=True)
    ctx.reorder_spatial(max(8, -(-n // (1 << 22))), 1337)
    rng = np.random.default_rng(5)
    vel = [rng.standard_normal(n, dtype=np.float32) * np.float32(100.0) + np.float32(b) for b in (50.0, -30.0, 20.0)]
    ctx.upload_velocities(*vel)
    del vel
    M, sf = camera_a(200.0)
    ctx.set_line_of_sight((0.0, 0.0, 1.0), (0.0, 0.0, 0.0))

    rgb = _native.MODE_RGB
    ctx.render(M, sf, mode=rgb)
    ctx.render(M, sf, mode=rgb)                              # warm: the record lists have grown to the frame's need
    frames = [ctx.render(M, sf, mode=rgb) for _ in range(max(args.repeats, 5))]
    stats = ctx.stats()
    ctx.read_image()
    t0 = time.perf_counter()
    for _ in range(5):
        ctx.read_image()
    read_ms = (time.perf_counter() - t0) * 1e3 / 5           # R * R * 16 bytes to the host, with its allocation
    rgb_ms = median(frames)

    fp = ctypes.POINTER(ctypes.c_float)
    Mf = np.ascontiguousarray(M.reshape(16))
    for C in (int(c) for c in args.channels.split(",")):
        out = {"n": n, "resolution": R, "n_channels": C, "repeats": args.repeats, "rgb_frame_ms": rgb_ms, "rgb_frames_ms": frames,
               "baseline_frames": -(-C // 3), "baseline_ms": rgb_ms * -(-C // 3), "read_image_ms": read_ms,
               "n_small": stats["n_small"], "n_mid": stats["n_mid"], "n_huge": stats["n_huge"]}
        if not args.baseline_only:
            dv = 800.0 / C
            cube = np.zeros((C, R, R), dtype=np.float32)     # (resident before the first timed call)

            def call():
                t = time.perf_counter()
                rc = lib.tsp_spectral_cube(ctx._h, Mf.ctypes.data_as(fp), float(sf), -400.0, dv, C, dv, None, cube.ctypes.data_as(fp))
                _native._check(rc)
                return (time.perf_counter() - t) * 1e3
            call()                                           # warm: code objects, the attribute of the tile kernel
            times = [call() for _ in range(args.repeats)]
            lay = _native.spectral_cube_layout(n, R, C)
            total = float(cube.astype(np.float64).sum())
            ctx.render(M, sf, mode=_native.MODE_KINEMATIC)
            S = float(ctx.read_image()[..., 0].astype(np.float64).sum())
            out.update({"cube_ms": median(times), "cube_calls_ms": times, "slices": lay["slices"], "slice_particles": lay["slice_particles"],
                        "cube_bytes": cube.nbytes, "cube_sum_over_surface_density_sum": total / S if S else None,
                        "ratio": rgb_ms * -(-C // 3) / median(times)})
            ctx.render(M, sf, mode=rgb)
        print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
