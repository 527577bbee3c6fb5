"""Time tsp_gravity_direct (softened direct-sum gravity) in its two regimes.

    python tools/gpu_gravity_bench.py [--n 262144] [--targets 400] [--sources 1e7] [--repeats 3] [--clock-ghz 2.4]
    python tools/gpu_gravity_bench.py --tree [--theta 0.5] [--n 1048576] [--repeats 3] [--direct-up-to 1048576]

Cases, all on one context after a warm-up at 2^14: 'phi' of every particle (targets = sources, n = 2^18, the potential only: what
from_arrays(eps=...) runs), the same with the accelerations, and a rotation curve's shape (400 targets against 1e7 sources, both
outputs).  Particles: a Plummer sphere, one softening length.  Prints one JSON line: per case the wall times of the synchronous
calls, the library's TOPSY_GRAVITY_STATS report of the last repeat (the time of the pair and reduce kernels between two events,
uploads and the read-back excluded), pairs per second over that kernel time, and its share of a ceiling.

The ceiling is what the vector units could issue if nothing else limited the pair loop: per 64 pairs (one wave instruction
each) the inner loop's VALU instructions, counted in the disassembly of gravity_pairs_kernel<4, ACC> as built
(hipcc --offload-arch=gfx950 --save-temps; the unchecked loop: 16 sources x 4 targets per iteration), at their issue cycles on
one SIMD -- full-rate float32 2 cycles, v_rsq_f32 (quarter rate) 8, the float64 conversions and additions 4 -- over
4 SIMDs x CUs at --clock-ghz.  Counts per pair: with accelerations 13.03 full-rate + 1 rsq + 0.5 float64 (930 VALU per 64
pairs); the potential only 8.03 + 1 + 0.125 (586 per 64).

--tree times tsp_gravity_tree instead, on the same Plummer sphere by the same method: targets = sources with accelerations at
--n, the library's report of the walk kernel (kernel_ms), of the tree's build kernels (build_ms) and of the index (index_ms, host
clock: upload, keys, sort), the particle and node terms per target, the walk's terms per second as a share of the direct kernel's
measured pairs per second, and -- up to --direct-up-to particles -- the direct sum of the same particles next to it.
"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# VALU instructions per pair in the inner loop, by issue class (full-rate float32, v_rsq_f32, float64), from the disassembly
SLOTS = {True: (13.03, 1.0, 0.5), False: (8.03, 1.0, 0.125)}
CYCLES = (2.0, 8.0, 4.0)           # issue cycles of a wave64 instruction of each class on one SIMD


def ceiling_pairs_per_s(with_acc, cu_count, clock_ghz):
    cycles_per_wave_pair = sum(n * c for n, c in zip(SLOTS[with_acc], CYCLES))
    return 4 * cu_count * clock_ghz * 1e9 * 64.0 / cycles_per_wave_pair


def plummer(n, seed):
    rs = np.random.RandomState(seed)
    r = 1.0 / np.sqrt(rs.uniform(size=n) ** (-2.0 / 3.0) - 1.0)
    v = rs.normal(size=(n, 3))
    return (r[:, None] * v / np.linalg.norm(v, axis=1)[:, None]).astype(np.float32)


def timed(call):
    """(seconds, the library's stderr report as a dict of the name=number pairs of its last line) of one call"""
    os.environ["TOPSY_GRAVITY_STATS"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        try:
            t0 = time.perf_counter()
            call()
            dt = time.perf_counter() - t0
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            os.environ.pop("TOPSY_GRAVITY_STATS", None)
        f.seek(0)
        lines = [l for l in f.read().decode(errors="replace").splitlines() if "kernel_ms=" in l]
    return dt, {k: float(v) for k, v in re.findall(r"(\w+)=([0-9.eE+-]+)(?=\s|$)", lines[-1])} if lines else {}


def tree_main(args, _native):
    n, eps = int(args.n), 0.01
    ctx = _native.Context(16, 2)
    w = plummer(2 ** 14, 1)
    wm = np.full(len(w), 1.0 / len(w), dtype=np.float32)
    ctx.gravity_tree(w[:, 0], w[:, 1], w[:, 2], wm, eps, theta=args.theta)                   # warm-up: code objects
    ctx.gravity_direct(w[:, 0], w[:, 1], w[:, 2], wm, eps)
    p = plummer(n, 2)
    x, y, z = (np.ascontiguousarray(p[:, k]) for k in range(3))
    m = np.full(n, 1.0 / n, dtype=np.float32)
    result = {"n": n, "theta": args.theta}
    times, report, info = [], {}, {}
    for _ in range(args.repeats):
        holder = []
        dt, report = timed(lambda: holder.append(ctx.gravity_tree(x, y, z, m, eps, theta=args.theta)[2]))
        times.append(dt)
        info = holder[0]
    terms = info["pairs_direct"] + info["pairs_node"]
    kernel_s = 1e-3 * report.get("kernel_ms", float("nan"))
    result["tree"] = {"wall_s": times, "kernel_ms": report.get("kernel_ms"), "build_ms": report.get("build_ms"),
                      "index_ms": report.get("index_ms"), "pairs_direct_per_target": info["pairs_direct"] / n,
                      "pairs_node_per_target": info["pairs_node"] / n, "n_nodes": info["n_nodes"], "n_levels": info["n_levels"],
                      "terms_per_s": terms / kernel_s, "share_of_direct_rate": terms / kernel_s / args.direct_pairs_per_s,
                      "equivalent_direct_pairs_per_s": float(n) * n / kernel_s}
    if n <= args.direct_up_to:
        times, report = [], {}
        for _ in range(args.repeats):
            dt, report = timed(lambda: ctx.gravity_direct(x, y, z, m, eps))
            times.append(dt)
        kernel_s = 1e-3 * report.get("kernel_ms", float("nan"))
        result["direct"] = {"wall_s": times, "kernel_ms": report.get("kernel_ms"), "pairs_per_s": float(n) * n / kernel_s}
    else:
        result["direct_extrapolated"] = {"kernel_ms": 1e3 * float(n) * n / args.direct_pairs_per_s, "pairs_per_s": args.direct_pairs_per_s}
    ctx.close()
    print(json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=2 ** 18)
    ap.add_argument("--targets", type=int, default=400)
    ap.add_argument("--sources", type=float, default=1e7)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--cu-count", type=int, default=256)
    ap.add_argument("--tree", action="store_true", help="time tsp_gravity_tree (targets = sources, with accelerations) at --n")
    ap.add_argument("--theta", type=float, default=0.5)
    ap.add_argument("--direct-up-to", type=float, default=2 ** 20, help="--tree: also time the direct sum up to this n")
    ap.add_argument("--direct-pairs-per-s", type=float, default=2.66e12, help="--tree: the direct kernel's measured rate with accelerations")
    args = ap.parse_args()
    from topsy_amd import _native
    if args.tree:
        return tree_main(args, _native)
    n, n_src, n_tgt = int(args.n), int(args.sources), args.targets
    eps = 0.01
    ctx = _native.Context(16, 2)
    w = plummer(2 ** 14, 1)
    wm = np.full(len(w), 1.0 / len(w), dtype=np.float32)
    ctx.gravity_direct(w[:, 0], w[:, 1], w[:, 2], wm, eps)                                   # warm-up: code objects
    ctx.gravity_direct(w[:, 0], w[:, 1], w[:, 2], wm, eps, want_acc=False)
    ctx.gravity_direct(w[:, 0], w[:, 1], w[:, 2], wm, eps, targets=[w[:300, k].copy() for k in range(3)])

    p = plummer(n, 2)
    x, y, z = (np.ascontiguousarray(p[:, k]) for k in range(3))
    m = np.full(n, 1.0 / n, dtype=np.float32)
    s = plummer(n_src, 3)
    sx, sy, sz = (np.ascontiguousarray(s[:, k]) for k in range(3))
    sm = np.full(n_src, 1.0 / n_src, dtype=np.float32)
    R = np.repeat(np.linspace(0.05, 5.0, (n_tgt + 3) // 4), 4)[:n_tgt]
    ang = np.tile([0.0, np.pi, 0.5 * np.pi, 1.5 * np.pi], (n_tgt + 3) // 4)[:n_tgt]
    probes = [(R * np.cos(ang)).astype(np.float32), (R * np.sin(ang)).astype(np.float32), np.zeros(n_tgt, dtype=np.float32)]
    cases = {
        "phi_all_particles": (lambda: ctx.gravity_direct(x, y, z, m, eps, want_acc=False), float(n) * n, False),
        "pot_and_acc_all_particles": (lambda: ctx.gravity_direct(x, y, z, m, eps), float(n) * n, True),
        "rotation_curve_probes": (lambda: ctx.gravity_direct(sx, sy, sz, sm, eps, targets=probes), float(n_src) * n_tgt, True),
    }
    result = {"n": n, "targets": n_tgt, "sources": n_src, "clock_ghz": args.clock_ghz, "cu_count": args.cu_count}
    for name, (call, pairs, with_acc) in cases.items():
        times, report = [], {}
        for _ in range(args.repeats):
            dt, report = timed(call)
            times.append(dt)
        top = ceiling_pairs_per_s(with_acc, args.cu_count, args.clock_ghz)
        kernel_s = 1e-3 * report.get("kernel_ms", float("nan"))
        result[name] = {"pairs": pairs, "wall_s": times, "kernel_ms": report.get("kernel_ms"), "pairs_per_s": pairs / kernel_s,
                        "pairs_per_s_wall": pairs / float(np.median(times)), "ceiling_pairs_per_s": top,
                        "share_of_ceiling": pairs / kernel_s / top}
    ctx.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
