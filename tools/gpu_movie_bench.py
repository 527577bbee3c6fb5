"""Movie export cost (topsy_amd.recorder): a scripted path -- a 90 degree turn and a 4x zoom, built as a timestream -- replayed as
60 frames at 30 frames/s on a device-generated synthetic snapshot, at 1920x1080 and 3840x2160.  Per frame (medians):

  yuv420p: the whole frame (frames(pixel_format="yuv420p"), set state + render + compose + convert + read back), the EXPORT render,
           the present_yuv420 call, its GPU time (hipEvents: composition + conversion) and the host write of the y4m frame;
  rgb24:   the whole frame (frames()), the present call, and the numpy conversion of the RGB frame (tests/yuv420_ref.py).

Prints one JSON line per canvas.  One snapshot size per process:

    python tools/gpu_movie_bench.py --n 1e8
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/gpu_movie_bench.py --n 1e8 --formats yuv420p
"""
import argparse
import json
import os
import pickle
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import topsy_amd  # noqa: E402
import yuv420_ref  # noqa: E402
from topsy_amd.recorder import VisualizationRecorder, y4m_header  # noqa: E402


class QuietRecorder(VisualizationRecorder):
    def _progress_iterator(self, ntot):
        return range(ntot)


def scripted_path(vis, seconds):
    """Timestream of the reference layout: every property at 0 and at `seconds`; the camera turns 90 degrees about the vertical
    axis and zooms in 4x."""
    names = VisualizationRecorder._record_properties
    start = {p: vis.colormap[p[9:-1]] if p.startswith("colormap[") else getattr(vis, p) for p in names}
    end = dict(start)
    end["rotation_matrix"] = vis._x_rotation_matrix(np.pi / 2) @ np.asarray(start["rotation_matrix"])
    end["scale"] = start["scale"] / 4.0
    return {p: [(0.0, start[p]), (seconds, end[p])] for p in names}, seconds


def timed(obj, name, sink, gpu_sink=None):
    """Wrap obj.name so every call appends its wall ms to sink (and the GPU ms it reports through timings= to gpu_sink)."""
    fn = getattr(obj, name)

    def wrapper(*a, **k):
        t0 = time.perf_counter()
        if gpu_sink is not None:
            ms = []
            out = fn(*a, timings=ms, **k)
            gpu_sink.append(ms[0])
        else:
            out = fn(*a, **k)
        sink.append((time.perf_counter() - t0) * 1e3)
        return out
    setattr(obj, name, wrapper)
    return fn


def med(v):
    return float(np.median(v)) if v else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e8)
    ap.add_argument("--resolution", type=int, default=1024, help="render resolution R of the SPH image")
    ap.add_argument("--canvases", default="1920x1080,3840x2160")
    ap.add_argument("--formats", default="yuv420p,rgb24")
    ap.add_argument("--fps", type=float, default=30.0)
    ap.add_argument("--seconds", type=float, default=2.0)
    args = ap.parse_args()
    n = int(args.n)
    t0 = time.perf_counter()
    vis = topsy_amd.synthetic_on_device(n, render_resolution=args.resolution)
    setup_s = time.perf_counter() - t0
    ts, ends_at = scripted_path(vis, args.seconds)
    rec = QuietRecorder(vis)
    with tempfile.TemporaryDirectory() as tmp:
        fn = os.path.join(tmp, "path.timestream")
        with open(fn, "wb") as f:
            pickle.dump((ts, ends_at), f)
        rec.load_timestream(fn)
        ctx = vis._sph._context
        render_ms, present_ms, gpu_ms = [], [], []
        timed(vis, "render_sph", render_ms)
        timed(ctx, "present_yuv420", present_ms, gpu_ms)
        timed(ctx, "present", present_ms)
        for canvas in args.canvases.split(","):
            W, H = (int(v) for v in canvas.split("x"))
            vis.get_presentation_image((W, H))            # warm-up: textures, code objects
            line = {"particles": n, "R": args.resolution, "canvas": canvas, "fps": args.fps, "frames": int(ends_at * args.fps),
                    "setup_s": setup_s}
            for fmt in args.formats.split(","):
                for v in (render_ms, present_ms, gpu_ms):
                    v.clear()
                frame_ms, write_ms, convert_ms = [], [], []
                out = os.path.join(tmp, "movie.y4m")
                with open(out, "wb") as f:
                    f.write(y4m_header(W, H, args.fps))
                    t = time.perf_counter()
                    for frame in rec.frames(args.fps, (W, H), pixel_format=fmt):
                        frame_ms.append((time.perf_counter() - t) * 1e3)
                        t1 = time.perf_counter()
                        if fmt == "rgb24":
                            frame = yuv420_ref.to_yuv420(frame)
                            convert_ms.append((time.perf_counter() - t1) * 1e3)
                            t1 = time.perf_counter()
                        f.write(b"FRAME\n")
                        for p in frame:
                            f.write(p.data)
                        write_ms.append((time.perf_counter() - t1) * 1e3)
                        t = time.perf_counter()
                size = os.path.getsize(out)
                os.remove(out)
                line[fmt] = {"frame_ms": med(frame_ms), "render_ms": med(render_ms), "present_call_ms": med(present_ms),
                             "write_ms": med(write_ms), "file_bytes": size}
                if fmt == "yuv420p":
                    line[fmt]["gpu_compose_convert_ms"] = med(gpu_ms)
                else:
                    line[fmt]["numpy_convert_ms"] = med(convert_ms)
            print(json.dumps(line), flush=True)
    vis.close()


if __name__ == "__main__":
    main()
