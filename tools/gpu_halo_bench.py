"""Time tsp_group_potential and tsp_halo_properties (halo properties of a whole catalogue in one call).

    python tools/gpu_halo_bench.py [--repeats 3] [--min-log2 14] [--max-log2 18] [--catalogue-log2 20] [--properties-log2 24]

All on one context after a warm-up; every figure is the last of --repeats calls.  Kernel times are the library's own reports
(TOPSY_HALO_STATS / TOPSY_GRAVITY_STATS: device events around the kernels, uploads and read-back excluded); wall_s is the whole
synchronous call.  Prints one JSON line:
  single_halo: one Plummer halo of 2^k members, k = --min-log2 .. --max-log2: the halo pair kernel's pairs per second next to
      tsp_gravity_direct and tsp_gravity_tree (theta 0.5), both potential-only, on the same particles.
  catalogue: 2^--catalogue-log2 particles in haloes with power-law sizes 20 .. 2^12: kernel time, and the pairs that count over
      the pair slots the kernel evaluated (the cost of the masks and of the partial tiles).
  properties: 2^--properties-log2 particles in haloes of 128 and in one halo: the time of every pass, and the bytes it moves
      (counted from the kernels' loads and stores per member: BYTES) over that time.
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

# bytes per member a pass reads and writes, with velocities and a potential (tsp_halo.hip): pass 1 = the gather of the caller's
# planes into sorted planes (36 + 8 index and key in, 52 out) and the first sums (48 in); pass 2 = 56 in, 20 out; pass 3 (after the
# sort) = three sweeps of key, position, mass and |e| (60 in all)
BYTES = {"pass1": 144, "pass2": 76, "pass3": 60}


def plummer(n, seed, a=1.0):
    rs = np.random.RandomState(seed)
    r = a / np.sqrt(np.maximum(rs.uniform(size=n), 1e-9) ** (-2.0 / 3.0) - 1.0)
    v = rs.normal(size=(n, 3))
    return (r[:, None] * v / np.linalg.norm(v, axis=1)[:, None]).astype(np.float32)


def timed(call):
    """(seconds, the name=number pairs of the library's last report line on stderr) of one call"""
    os.environ["TOPSY_HALO_STATS"] = os.environ["TOPSY_GRAVITY_STATS"] = "1"
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
            os.environ.pop("TOPSY_HALO_STATS", None)
            os.environ.pop("TOPSY_GRAVITY_STATS", None)
        f.seek(0)
        lines = [l for l in f.read().decode(errors="replace").splitlines() if "_ms=" in l or " ms:" in l]
    return dt, {k: float(v) for k, v in re.findall(r"(\w+)=([0-9.eE+-]+)(?=\s|$)", lines[-1])} if lines else {}


def last_of(repeats, call):
    times, report = [], {}
    for _ in range(repeats):
        dt, report = timed(call)
        times.append(dt)
    return times, report


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--min-log2", type=int, default=14)
    ap.add_argument("--max-log2", type=int, default=18)
    ap.add_argument("--catalogue-log2", type=int, default=20)
    ap.add_argument("--properties-log2", type=int, default=24)
    args = ap.parse_args()
    from topsy_amd import _native
    ctx = _native.Context(16, 2)
    eps = 0.01
    w = plummer(2 ** 14, 1)
    wm = np.full(len(w), 1.0 / len(w), dtype=np.float32)
    ones = np.ones(len(w), dtype=np.int32)
    ctx.group_potential(w[:, 0], w[:, 1], w[:, 2], wm, eps, ones, 1)                          # warm-up: code objects
    ctx.halo_properties(w[:, 0], w[:, 1], w[:, 2], wm, ones, 1, vel=[w[:, 0], w[:, 1], w[:, 2]], phi=np.zeros(len(w)))
    ctx.gravity_direct(w[:, 0], w[:, 1], w[:, 2], wm, eps, want_acc=False)
    ctx.gravity_tree(w[:, 0], w[:, 1], w[:, 2], wm, eps, want_acc=False)
    result = {"single_halo": [], "bytes_per_member": BYTES}

    for k in range(args.min_log2, args.max_log2 + 1):
        n = 2 ** k
        p = plummer(n, 2)
        x, y, z = (np.ascontiguousarray(p[:, c]) for c in range(3))
        m = np.full(n, 1.0 / n, dtype=np.float32)
        lab = np.ones(n, dtype=np.int32)
        pairs = float(n) * (n - 1)
        row = {"n": n}
        t, r = last_of(args.repeats, lambda: ctx.group_potential(x, y, z, m, eps, lab, 1))
        row["halo"] = {"wall_s": t[-1], "kernel_ms": r.get("kernel_ms"), "pairs_per_s": pairs / (1e-3 * r.get("kernel_ms", np.nan)),
                       "slots": r.get("slots")}
        t, r = last_of(args.repeats, lambda: ctx.gravity_direct(x, y, z, m, eps, want_acc=False))
        row["direct"] = {"wall_s": t[-1], "kernel_ms": r.get("kernel_ms"), "pairs_per_s": pairs / (1e-3 * r.get("kernel_ms", np.nan))}
        t, r = last_of(args.repeats, lambda: ctx.gravity_tree(x, y, z, m, eps, theta=0.5, want_acc=False))
        row["tree"] = {"wall_s": t[-1], "kernel_ms": r.get("kernel_ms"), "build_ms": r.get("build_ms"), "index_ms": r.get("index_ms")}
        result["single_halo"].append(row)

    # a catalogue: power-law sizes 20 .. 2^12 (dn / ds ~ s^-2), haloes side by side, labels in random order over the particles
    n = 2 ** args.catalogue_log2
    rs = np.random.RandomState(5)
    sizes = []
    while sum(sizes) < n:
        sizes.append(int(min(4096, 20.0 / max(rs.uniform(), 20.0 / 4096))))
    sizes[-1] -= sum(sizes) - n
    sizes = [s for s in sizes if s > 0]
    lab = np.repeat(np.arange(1, len(sizes) + 1, dtype=np.int32), sizes)
    centres = rs.uniform(0, 100, size=(len(sizes), 3))
    p = (centres[lab - 1] + plummer(n, 6, a=0.05)).astype(np.float32)
    order = rs.permutation(n)
    p, lab = p[order], lab[order]
    x, y, z = (np.ascontiguousarray(p[:, c]) for c in range(3))
    m = np.full(n, 1.0 / n, dtype=np.float32)
    holder = []
    t, r = last_of(args.repeats, lambda: holder.append(ctx.group_potential(x, y, z, m, eps, lab, len(sizes))[1]))
    info = holder[-1]
    result["catalogue"] = {"n": n, "haloes": len(sizes), "largest": max(sizes), "wall_s": t[-1], "kernel_ms": r.get("kernel_ms"),
                           "pairs": info["pairs"], "pair_slots": info["pair_slots"], "pairs_over_slots": info["pairs"] / info["pair_slots"],
                           "slots_per_s": info["pair_slots"] / (1e-3 * r.get("kernel_ms", np.nan))}

    n = 2 ** args.properties_log2
    p = plummer(n, 7)
    x, y, z = (np.ascontiguousarray(p[:, c]) for c in range(3))
    vel = [np.ascontiguousarray(v) for v in rs.normal(size=(3, n)).astype(np.float32)]
    m = np.full(n, 1.0 / n, dtype=np.float32)
    phi = -np.ones(n)
    result["properties"] = []
    for n_groups in (n // 128, 1):
        lab = (rs.permutation(n) % n_groups + 1).astype(np.int32)
        t, r = last_of(args.repeats, lambda: ctx.halo_properties(x, y, z, m, lab, n_groups, vel=vel, phi=phi))
        row = {"n": n, "haloes": n_groups, "wall_s": t[-1]}
        for name in ("pass1", "pass2", "sort", "pass3"):
            row[name + "_ms"] = r.get(name)
            if name in BYTES and r.get(name):
                row[name + "_gb_per_s"] = BYTES[name] * n / (1e-3 * r[name]) / 1e9
        result["properties"].append(row)
    ctx.close()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
