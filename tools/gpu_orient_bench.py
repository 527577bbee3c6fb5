"""Time tsp_sphere_moments (the moments a face-on / side-on orientation is taken from) on the positions of the synthetic snapshot,
unit masses, with velocities of a rotation about z plus noise.

    python tools/gpu_orient_bench.py --n 3e7 [--radius 20] [--repeats 3]

The same particles are summed twice: in the generator's order (every index range is a uniform sample of the snapshot, so no
block of 1024 consecutive particles can be skipped: pass B reads all 28 bytes per particle) and in the spatial order of
tsp_reorder_spatial with one stratum (Morton order: the blocks are compact and the r_vel pass reads almost nothing).  Prints one
JSON line: per order the wall time of the synchronous host-array call over the repeats and its median, and from the library's
TOPSY_ORIENT_STATS report of the last repeat the upload and preparation times and each pass's kernel time (hipEvent pair) and the
blocks it read.  Beside pass B's time on the shuffled arrays: the time a plain device-to-device copy of the same 28 x n bytes takes
on the same card (hipMemcpyAsync between two hipEvents, median of 5; a copy also writes what it reads), the time the
streaming-read peak of tsp_measure_read_bandwidth would need for them, and pass B's achieved rate.  A warm-up on 1e5 particles
comes first.  Run one size per process.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import re  # noqa: E402

from gpu_center_bench import synthetic_positions  # noqa: E402


def timed(call):
    """(seconds, result, the library's stderr report) of one call with TOPSY_ORIENT_STATS=1"""
    import tempfile
    import time
    os.environ["TOPSY_ORIENT_STATS"] = "1"
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
            os.environ.pop("TOPSY_ORIENT_STATS", None)
        f.seek(0)
        report = f.read().decode(errors="replace")
    return dt, out, report


def parse_report(report):
    head = re.search(r"blocks=(\d+) workgroups=(\d+) upload_ms=([0-9.]+) prepare_ms=([0-9.]+)", report)
    out = {"blocks": int(head.group(1)), "workgroups": int(head.group(2)), "upload_ms": float(head.group(3)),
           "prepare_ms": float(head.group(4))}
    for name, ms, blocks, inside in re.findall(r"pass=([AB]) kernel_ms=([0-9.]+) blocks_read=(\d+) inside=(\d+)", report):
        out[f"pass_{name}_kernel_ms"] = float(ms)
        out[f"pass_{name}_blocks_read"] = int(blocks)
        out[f"pass_{name}_inside"] = int(inside)
    return out


def rotation_velocities(x, y, seed=11):
    """Unit circular speed about z plus noise of sigma 0.1, float32."""
    rs = np.random.RandomState(seed)
    rho = np.maximum(np.hypot(x, y), np.float32(1e-6))
    noise = rs.normal(scale=0.1, size=(3, len(x))).astype(np.float32)
    return -y / rho + noise[0], x / rho + noise[1], noise[2]


def device_copy_ms(nbytes, repeats=5):
    """Median time (hipEvent pair) of a device-to-device hipMemcpyAsync of nbytes on the current device, through the HIP runtime
    the library has already loaded."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    vp = ctypes.c_void_p

    def check(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed with hipError {rc}")
    hip.hipMalloc.argtypes = [ctypes.POINTER(vp), ctypes.c_size_t]
    hip.hipFree.argtypes = [vp]
    hip.hipMemsetAsync.argtypes = [vp, ctypes.c_int, ctypes.c_size_t, vp]
    hip.hipMemcpyAsync.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int, vp]
    hip.hipEventCreate.argtypes = [ctypes.POINTER(vp)]
    hip.hipEventRecord.argtypes = [vp, vp]
    hip.hipEventSynchronize.argtypes = [vp]
    hip.hipEventDestroy.argtypes = [vp]
    hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), vp, vp]
    src, dst, e0, e1 = vp(), vp(), vp(), vp()
    check(hip.hipMalloc(ctypes.byref(src), nbytes), "hipMalloc")
    times = []
    try:
        check(hip.hipMalloc(ctypes.byref(dst), nbytes), "hipMalloc")
        check(hip.hipEventCreate(ctypes.byref(e0)), "hipEventCreate")
        check(hip.hipEventCreate(ctypes.byref(e1)), "hipEventCreate")
        check(hip.hipMemsetAsync(src, 0, nbytes, None), "hipMemsetAsync")
        for _ in range(repeats + 1):            # (the first is a warm-up)
            check(hip.hipEventRecord(e0, None), "hipEventRecord")
            check(hip.hipMemcpyAsync(dst, src, nbytes, 3, None), "hipMemcpyAsync")      # 3 = hipMemcpyDeviceToDevice
            check(hip.hipEventRecord(e1, None), "hipEventRecord")
            check(hip.hipEventSynchronize(e1), "hipEventSynchronize")
            ms = ctypes.c_float()
            check(hip.hipEventElapsedTime(ctypes.byref(ms), e0, e1), "hipEventElapsedTime")
            times.append(ms.value)
    finally:
        for e in (e0, e1):
            if e:
                hip.hipEventDestroy(e)
        for buf in (src, dst):
            if buf:
                hip.hipFree(buf)
    return float(np.median(times[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, required=True)
    ap.add_argument("--radius", type=float, default=20.0)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    from topsy_amd import _native
    n = int(args.n)
    r, r_vel = args.radius, args.radius / 5
    result = {"n": n, "radius": r, "vel_radius": r_vel, "bytes_per_particle": 28}
    ctx = _native.Context(16, 2)
    wx, wy, wz = synthetic_positions(100_000, False, seed=7)
    timed(lambda: ctx.sphere_moments(wx, wy, wz, np.ones(len(wx), dtype=np.float32), vel=rotation_velocities(wx, wy), r=r,
                                     r_vel=r_vel))      # warm-up: code objects
    read_gbps = ctx.measure_read_bandwidth()
    result["read_bandwidth_gbps"] = read_gbps
    result["read_peak_ms_same_bytes"] = 28.0 * n / (read_gbps * 1e9) * 1e3
    result["device_copy_ms_same_bytes"] = device_copy_ms(28 * n)
    mass = np.ones(n, dtype=np.float32)
    for label, spatial in (("shuffled", False), ("sorted", True)):
        x, y, z = synthetic_positions(n, spatial)
        vel = rotation_velocities(x, y)
        times, report, out = [], "", None
        for _ in range(args.repeats):
            dt, out, report = timed(lambda: ctx.sphere_moments(x, y, z, mass, vel=vel, r=r, r_vel=r_vel))
            times.append(dt)
        stats = parse_report(report)
        stats["pass_B_gbps"] = 28.0 * n * stats["pass_B_blocks_read"] / stats["blocks"] / (stats["pass_B_kernel_ms"] * 1e-3) / 1e9
        norm = float(np.linalg.norm(out["L"]))
        result[label] = dict(stats, call_s=times, call_s_median=float(np.median(times)), n_inside=out["n_inside"],
                             n_inside_vel=out["n_inside_vel"], axis=[float(v) / norm for v in out["L"]], L_over_A=norm / out["A"])
    result["pass_B_shuffled_over_device_copy"] = result["shuffled"]["pass_B_kernel_ms"] / result["device_copy_ms_same_bytes"]
    ctx.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
