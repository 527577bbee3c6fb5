"""Frame composition cost (tsp_present) on a resident 1024^2 render: the composition kernel alone (hipEvents around the
launch) and the whole call (host textures in, frame out), at 1920x1080 and 3840x2160 with every layer on (colorbar, scale
bar and label, crosshairs, simulation cube of a periodic view, status line).  Prints one JSON line per canvas.

    python tools/gpu_present_bench.py [--iters 50]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--particles", type=int, default=200_000)
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


if __name__ == "__main__":
    main()
