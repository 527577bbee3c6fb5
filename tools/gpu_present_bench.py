"""Frame composition cost (tsp_present) on a resident 1024^2 render: the composition kernel alone (hipEvents around the
launch) and the whole call (host textures in, frame out), at 1920x1080 and 3840x2160 with every layer on (colorbar, scale
bar and label, crosshairs, simulation cube of a periodic view, status line).  Prints one JSON line per canvas.
--surface adds the surface frame (tsp_present_surface) of a SurfaceView of the same scene without the periodic tiling, colouring
by the test quantity, with its default layers (colorbar, scale bar and label, status line): the filter and the composition
kernel apart, and beside them the [filter, shading] times of tsp_surface_present on the same image.

--kinematic adds the kinematic frame (the moment bases of tsp_present) of a VelocityView of a rotating copy of the scene: the
v_los and sigma_los frames and, alternately in the same loop, a scalar frame of the same 4-channel image under the same layers
(colorbar, scale bar and label, status line), so that the calls differ by the base alone; then the time of the view's automatic
range per frame, from the device sort (get_range) and by the download and host percentile it replaced.

    python tools/gpu_present_bench.py [--iters 50] [--surface] [--kinematic]
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


def kinematic_cases(args):
    from topsy_amd import config, kinematics, loader
    ld = loader.TestDataLoader(None, args.particles)
    ps, mass = np.asarray(ld.get_pos_smooth(), dtype=np.float32), np.asarray(ld.get_mass(), dtype=np.float32)
    pos = np.ascontiguousarray(ps[:, :3])
    rs = np.random.RandomState(1)
    vel = (np.cross([0.0, 0.0, 1.0], pos) * 10.0 + rs.normal(0.0, 20.0, pos.shape)).astype(np.float32)      # rotation about z, some dispersion
    vis = topsy_amd.from_arrays(pos, np.ascontiguousarray(ps[:, 3]), mass, vel=vel, render_resolution=1024)
    vis.scale = config.DEFAULT_SCALE
    vis.rotation_matrix = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]])
    view = topsy_amd.VelocityView(vis, v_ref=None)
    ctx = vis._sph._context
    for kind in kinematics.KINDS:
        fr = view.frames(kind)
        fr.display_status("bench", timeout=1e9)
        for W, H in [(1920, 1080), (3840, 2160)]:
            fr.get_presentation_image((W, H))             # renders, resolves the range, builds every texture once
            base, layers = fr._last_presentation
            S = ctx.read_image()[..., 0]
            lo, hi = np.percentile(np.log10(S[S > 0]), [1.0, 99.9])
            scalar = {"map": "scalar", "lut": base["lut"], "vmin": lo, "vmax": hi, "log": True, "weighted": False}
            times = {"moment": ([], []), "scalar": ([], [])}
            for _ in range(args.iters):
                for name, b in (("moment", base), ("scalar", scalar)):
                    t = []
                    t0 = time.perf_counter()
                    ctx.present(W, H, b, layers, timings=t)
                    times[name][1].append((time.perf_counter() - t0) * 1e3)
                    times[name][0].append(t[0])
            out = {"canvas": f"{W}x{H}", "base": base["map"], "resolution": 1024, "layers": len(layers), "iters": args.iters}
            for name, (kernel_ms, call_ms) in times.items():
                out |= {f"{name}_kernel_ms_median": float(np.median(kernel_ms)), f"{name}_kernel_ms_min": float(np.min(kernel_ms)),
                        f"{name}_call_ms_median": float(np.median(call_ms)), f"{name}_call_ms_min": float(np.min(call_ms)),
                        f"{name}_call_ms_p10": float(np.percentile(call_ms, 10)), f"{name}_call_ms_p90": float(np.percentile(call_ms, 90))}
            print(json.dumps(out), flush=True)
    for kind in kinematics.KINDS:
        device_ms, host_ms = [], []
        for _ in range(args.iters):
            t0 = time.perf_counter()
            got = view.get_range(kind)
            t1 = time.perf_counter()
            want = kinematics.resolve_range(kind, view.get_maps()[kind])
            t2 = time.perf_counter()
            device_ms.append((t1 - t0) * 1e3)
            host_ms.append((t2 - t1) * 1e3)
            assert got == want, (kind, got, want)
        print(json.dumps({"range": kind, "resolution": 1024, "iters": args.iters, "device_sort_ms_median": float(np.median(device_ms)),
                          "device_sort_ms_min": float(np.min(device_ms)), "download_percentile_ms_median": float(np.median(host_ms)),
                          "download_percentile_ms_min": float(np.min(host_ms))}), flush=True)
    vis.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--particles", type=int, default=200_000)
    ap.add_argument("--surface", action="store_true", help="also time the surface frame (tsp_present_surface)")
    ap.add_argument("--kinematic", action="store_true", help="also time the kinematic frames (the moment bases of tsp_present)")
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
    if args.kinematic:
        kinematic_cases(args)


if __name__ == "__main__":
    main()
