"""Per-stage GPU times of surface rendering (include/topsy_splat.h "Surface rendering").

    python tools/gpu_surface_bench.py --n 1e8 [--resolution 1024] [--repeats 5]     # cut selection, draw + resolve
    python tools/gpu_surface_bench.py --filter-sizes 1024 4096 --scales 0.01 0.1    # bilateral filter + shading

--n: synthetic particles generated on the device (the headline snapshot's law), camera A at scale 200, the default cut (the
median of rho = m / h^3).  Reports the wall time of the cut selection (device sort of rho + 101 quantiles: a one-off per snapshot)
and the hipEvent times of the occlusion draw and the resolve per frame (median of --repeats after one warm-up), then the filter and
shading of that frame.  --filter-sizes: the filter and the shading alone on a synthetic (q, depth) image.  Prints one JSON line
per measurement.  Run one size per process, each under its own time limit.
"""
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


def present_times(ctx, scale, repeats):
    t = []
    for _ in range(repeats + 1):
        ms = []
        ctx.surface_present(smoothing_scale=scale, light_direction=(0.0, 0.70710677, 0.70710677), ambient_color=(0.0, 0.0, 0.2),
                            content=False, rgba=True, timings=ms)
        t.append(ms)
    t = np.array(t[1:])
    return float(np.median(t[:, 0])), float(np.median(t[:, 1]))


def bench_frame(n, R, repeats, scale=200.0):
    from topsy_amd import _native, kernel_lut
    from topsy_amd.sph import density_quantiles
    ctx = _native.Context(R, 2)
    try:
        ctx.set_kernel_mips(kernel_lut.kernel_mips())
        ctx.set_sphere_mips(kernel_lut.sphere_mips())
        ctx.generate_synthetic(n, 0, n, 1337, 0.0, with_quantity=True)
        t0 = time.perf_counter()
        cuts = density_quantiles(ctx)
        cut_s = time.perf_counter() - t0
        cut = np.float32(cuts[50])
        M, sf = camera_a(scale)
        draw, resolve = [], []
        for k in range(repeats + 1):
            ctx.render_surface(M, sf, cut)
            st = ctx.stats()
            if k:
                draw.append(st["ms_stream"])
                resolve.append(st["ms_mid"])
        drawn = ctx.num_particles - ctx.stats()["n_culled"]
        covered = int((ctx.read_image()[..., 1] > 0).sum())
        filt, shade = present_times(ctx, 0.01, repeats)
    finally:
        ctx.close()
    return {"stage": "frame", "n": n, "resolution": R, "camera": "A", "scale": scale, "cut_percentile": 50,
            "cut_selection_s": round(cut_s, 4), "draw_ms": float(np.median(draw)), "resolve_ms": float(np.median(resolve)),
            "filter_ms_0.01": filt, "shade_ms": shade, "particles_drawn": int(drawn), "pixels_covered": covered,
            "draw_ms_all": draw}


def bench_filter(R, scales, repeats):
    from topsy_amd import _native
    rs = np.random.RandomState(R)
    img = np.zeros((R, R, 2), dtype=np.float32)
    img[..., 0] = rs.normal(size=(R, R))
    yy, xx = np.mgrid[0:R, 0:R].astype(np.float32) / R
    img[..., 1] = np.clip(0.8 - ((xx - 0.5) ** 2 + (yy - 0.5) ** 2), 0, None) + rs.uniform(0, 0.01, size=(R, R))
    ctx = _native.Context(R, 2)
    out = []
    try:
        ctx.write_image(img)
        for s in scales:
            filt, shade = present_times(ctx, s, repeats)
            out.append({"stage": "filter", "resolution": R, "smoothing_scale": s, "filter_ms": filt, "shade_ms": shade})
    finally:
        ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, nargs="*", default=[])
    ap.add_argument("--resolution", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--filter-sizes", type=int, nargs="*", default=[])
    ap.add_argument("--scales", type=float, nargs="*", default=[0.01, 0.1])
    args = ap.parse_args()
    for n in args.n:
        print(json.dumps(bench_frame(int(n), args.resolution, args.repeats)), flush=True)
    for R in args.filter_sizes:
        for line in bench_filter(R, args.scales, args.repeats):
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
