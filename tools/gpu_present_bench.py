"""Frame composition cost (tsp_present) on a resident 1024^2 render: the composition kernel alone (hipEvents around the
launch) and the whole call (host textures in, frame out), at 1920x1080 and 3840x2160 with every layer on (colorbar, scale
bar and label, crosshairs, simulation cube of a periodic view, status line).  Prints one JSON line per canvas.
--surface adds the surface frame (tsp_present_surface) of a SurfaceView of the same scene without the periodic tiling, colouring
by the test quantity, with its default layers (colorbar, scale bar and label, status line): the filter and the composition
kernel apart, and beside them the [filter, shading] times of tsp_surface_present on the same image.

    python tools/gpu_present_bench.py [--iters 50] [--surface]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/gpu_present_bench.py --iters 50
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import topsy_amd  # noqa: E402


def surface_cases(args):
    vis = topsy_amd.test(args.particles, render_resolution=1024)
    vis.quantity_name = "test-quantity"
    view = topsy_amd.SurfaceView(vis)
    view.display_status("bench", timeout=1e9)
    ctx = vis._sph._context
    for W, H in [(1920, 1080), (3840, 2160)]:
        view.get_presentation_image((W, H))           # renders, autoranges, builds every texture once
        params, layers = view._last_presentation
        filter_ms, compose_ms, call_ms, square = [], [], [], []
        for _ in range(args.iters):
            t = []
            t0 = time.perf_counter()
            ctx.present_surface(W, H, params, layers, timings=t)
            call_ms.append((time.perf_counter() - t0) * 1e3)
            filter_ms.append(t[0])
            compose_ms.append(t[1])
            ctx.surface_present(content=False, rgba=True, timings=t, **params)
            square.append(list(t))
        square = np.array(square)
        print(json.dumps({"canvas": f"{W}x{H}", "base": "surface", "resolution": 1024, "layers": len(layers), "iters": args.iters,
                          "weighted_average": bool(params["weighted_average"]),
                          "filter_ms_median": float(np.median(filter_ms)), "filter_ms_min": float(np.min(filter_ms)),
                          "kernel_ms_median": float(np.median(compose_ms)), "kernel_ms_min": float(np.min(compose_ms)),
                          "call_ms_median": float(np.median(call_ms)), "call_ms_min": float(np.min(call_ms)),
                          "surface_present_filter_ms_median": float(np.median(square[:, 0])),
                          "surface_present_shade_ms_median": float(np.median(square[:, 1]))}), flush=True)
    vis.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--particles", type=int, default=200_000)
    ap.add_argument("--surface", action="store_true", help="also time the surface frame (tsp_present_surface)")
    args = ap.parse_args()
    vis = topsy_amd.test(args.particles, render_resolution=1024, periodic_tiling=True)
    vis.crosshairs_visible = True
    vis.display_status("bench", timeout=1e9)
    ctx = vis._sph._context
    for W, H in [(1920, 1080), (3840, 2160)]:
        vis.get_presentation_image((W, H))            # renders, builds every texture once
        base, layers = vis._last_presentation
        kernel_ms, call_ms = [], []
        for _ in range(args.iters):
            t = []
            t0 = time.perf_counter()
            ctx.present(W, H, base, layers, timings=t)
            call_ms.append((time.perf_counter() - t0) * 1e3)
            kernel_ms.append(t[0])
        print(json.dumps({"canvas": f"{W}x{H}", "layers": len(layers), "iters": args.iters,
                          "kernel_ms_median": float(np.median(kernel_ms)), "kernel_ms_min": float(np.min(kernel_ms)),
                          "call_ms_median": float(np.median(call_ms)), "call_ms_min": float(np.min(call_ms))}), flush=True)
    vis.close()
    if args.surface:
        surface_cases(args)


if __name__ == "__main__":
    main()
