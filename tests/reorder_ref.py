"""A NumPy model of the load-time ordering's contract (tsp_reorder_spatial, tsp_get_strata_offsets, tsp_get_cell_layout,
tsp_get_cell_offsets: include/topsy_splat.h, topsy_amd/csrc/tsp_data.hip), operation by operation and without a GPU or library
call: what tests/test_gpu_reorder.py holds the library to, checked on its own by tests/test_reorder_ref_cpu.py.

Box       per axis over the FINITE values only, ordered by the monotone float -> uint map (so -0.0 < +0.0): lo = the minimum.  An
          axis without a finite value: lo = 0, inv = 0.
inv       steps per unit length, float32.  max > min: 65535 / float32(max - min), held at FLT_MAX when the quotient overflows
          (an extent of a few denormals); max - min itself overflowing float32 makes the axis WIDE: inv = float32(65535 /
          (float64(max) - float64(min))).  Otherwise (one value, or none) 0.
step      fx = float32(float32(x - lo) * inv): a subtraction, then a multiplication.  A wide axis forms both in float64 and
          rounds once: fx = float32((float64(x) - float64(lo)) * float64(inv)).  NaN -> 0, then clamp to [0, 65535], truncate.
key       16 bits per axis interleaved (x is bit 0, y bit 1, z bit 2 of every triple); key = stratum << 48 | morton.
stratum   splitmix64(seed ^ i) % n_strata, 0 when n_strata == 1.
order     the STABLE ascending sort of the keys (equal keys keep their index order).
grid      k = the largest value <= 4 with n // (n_strata << 3 k) >= 16; offsets = lower bounds of key >> (48 - 3 k);
          cell_width = float32(1 << (16 - k)) / inv in float32 (+inf for the one cell of a wide axis), 0 when inv == 0.
in-block  segments = (aligned 512-block) x (stratum, cell run).  Arrangement 1: in a segment of L >= 16, rank r goes to slot
          (r % 8) * (L // 8) + min(r % 8, L % 8) + r // 8; shorter segments stay.  Arrangement 2: every segment is ordered by
          ascending 0xFFFFFFFF - bits(h), ties in any order: the model gives the segment bounds and each segment's sorted keys.
culling   StratifiedCells.select_sphere keeps every cell whose centre lies closer than radius + one cell diagonal, and every
          cell whose centre or diagonal is not finite; no particle that is finite on all axes and strictly inside the sphere
          may fall outside the ranges (lost_particles below: exact, no tolerance).

rule="parent" restates the arithmetic before the wide axis and the FLT_MAX hold existed (inv = 65535 / float32(max - min), which
is 0 for an overflowing extent and +inf for a tiny one): kept so that the loss it causes is shown once, on the CPU."""
import numpy as np

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max
BLOCK = 512


def splitmix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def _ordered_u32(v):
    u = np.ascontiguousarray(v, dtype=f32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def _unordered_f32(u):
    u = np.uint32(u)
    v = (u & np.uint32(0x7fffffff)) if (u & np.uint32(0x80000000)) else ~u
    return np.array([v], dtype=np.uint32).view(f32)[0]


def bounding_box(pos, rule="fixed"):
    """(lo, inv, wide) of float32 positions (n, 3): float32 (3,), float32 (3,), bool (3,)."""
    pos = np.ascontiguousarray(pos, dtype=f32)
    lo, inv, wide = np.zeros(3, f32), np.zeros(3, f32), np.zeros(3, bool)
    for a in range(3):
        v = pos[:, a]
        o = _ordered_u32(v[np.isfinite(v)])
        a_, b_ = (_unordered_f32(o.min()), _unordered_f32(o.max())) if len(o) else (f32(0), f32(0))
        lo[a] = a_
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            if not b_ > a_:
                continue
            ext = f32(b_ - a_)
            if rule == "parent":
                inv[a] = f32(65535.0) / ext
            elif not np.isfinite(ext):
                wide[a] = True
                inv[a] = f32(65535.0 / (np.float64(b_) - np.float64(a_)))
            else:
                inv[a] = min(f32(65535.0) / ext, FLT_MAX)
    return lo, inv, wide


def steps(pos, lo, inv, wide):
    """the 16-bit step of every particle on every axis, uint64 (n, 3)"""
    pos = np.ascontiguousarray(pos, dtype=f32)
    out = np.zeros(pos.shape, dtype=np.uint64)
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(3):
            if wide[a]:
                fx = ((pos[:, a].astype(np.float64) - np.float64(lo[a])) * np.float64(inv[a])).astype(f32)
            else:
                d = (pos[:, a] - lo[a]).astype(f32)
                fx = (d * inv[a]).astype(f32)
            fx = np.where(np.isnan(fx), f32(0), np.minimum(np.maximum(fx, f32(0)), f32(65535)))
            out[:, a] = fx.astype(np.uint64)
    return out


def _spread(v):
    v = v.astype(np.uint64) & np.uint64(0xffff)
    out = np.zeros_like(v)
    for j in range(16):
        out |= ((v >> np.uint64(j)) & np.uint64(1)) << np.uint64(3 * j)
    return out


def morton(q):
    return _spread(q[:, 0]) | (_spread(q[:, 1]) << np.uint64(1)) | (_spread(q[:, 2]) << np.uint64(2))


def strata(n, n_strata, seed):
    if n_strata == 1:
        return np.zeros(n, dtype=np.uint64)
    return splitmix64(np.uint64(seed) ^ np.arange(n, dtype=np.uint64)) % np.uint64(n_strata)


def grid_bits(n, n_strata):
    k = 0
    while k < 4 and n // (n_strata << (3 * (k + 1))) >= 16:
        k += 1
    return k


def h_keys(h):
    return (np.uint32(0xFFFFFFFF) - np.ascontiguousarray(h, dtype=f32).view(np.uint32)).astype(np.uint32)


def cell_codes(pos, k, rule="fixed"):
    """Morton code of every particle's cell on the (2^k)^3 grid over the bounding box of `pos` (any order of the particles)"""
    lo, inv, wide = bounding_box(pos, rule)
    return (morton(steps(pos, lo, inv, wide)) >> np.uint64(48 - 3 * k)).astype(np.int64)


def reorder(pos, h=None, n_strata=1, seed=1337, interleave=2, rule="fixed"):
    """The contract on positions `pos` float32 (n, 3) in the caller's order.  Returns a dict:
      perm            new -> old, int64 (n,).  interleave 0 and 1: THE permutation.  interleave 2: the Morton order whose
                      segments the library then sorts by h -- segment [a, e) holds the set perm[a:e]
      segments        int64 (m, 2): the [a, e) of every (512-block) x (stratum, cell run) segment, ascending
      segment_keys    interleave 2 only: uint32 (n,), per segment the ascending 0xFFFFFFFF - bits(h) of its particles
      perm_by_h       interleave 2 only: the permutation itself when no segment holds two equal keys
      strata_offsets  int64 (n_strata + 1,)
      layout          dict(n_strata, cells_per_axis, box_lo float32 (3,), cell_width float32 (3,), offsets int64), the form of
                      Context.cell_layout()
      cell            int64 (n,): (stratum, cell) entry of every particle in the new order"""
    pos = np.ascontiguousarray(pos, dtype=f32)
    n = len(pos)
    lo, inv, wide = bounding_box(pos, rule)
    key = (strata(n, n_strata, seed) << np.uint64(48)) | morton(steps(pos, lo, inv, wide))
    order = np.argsort(key, kind="stable").astype(np.int64)
    skey = key[order]
    k = grid_bits(n, n_strata)
    shift = np.uint64(48 - 3 * k)
    cell = (skey >> shift).astype(np.int64)
    n_entries = (n_strata << (3 * k)) + 1
    offsets = np.searchsorted(cell, np.arange(n_entries), side="left").astype(np.int64)
    strata_offsets = np.searchsorted((skey >> np.uint64(48)).astype(np.int64), np.arange(n_strata + 1), side="left").astype(np.int64)
    with np.errstate(over="ignore", divide="ignore"):
        width = np.array([f32(1 << (16 - k)) / inv[a] if inv[a] > 0 else f32(0) for a in range(3)], dtype=f32)
    idx = np.arange(n, dtype=np.int64)
    first = np.ones(n, dtype=bool)
    first[1:] = (cell[1:] != cell[:-1]) | (idx[1:] % BLOCK == 0)
    seg_a = np.flatnonzero(first)
    seg_e = np.append(seg_a[1:], n)
    out = {"segments": np.stack([seg_a, seg_e], axis=1), "strata_offsets": strata_offsets, "cell": cell,
           "layout": {"n_strata": n_strata, "cells_per_axis": 1 << k, "box_lo": lo, "cell_width": width, "offsets": offsets}}
    if interleave == 1:
        sid = np.cumsum(first) - 1
        a, L = seg_a[sid], (seg_e - seg_a)[sid]
        r = idx - a
        row = r % 8
        slot = np.where(L >= 16, a + row * (L // 8) + np.minimum(row, L % 8) + r // 8, idx)
        perm = np.empty(n, dtype=np.int64)
        perm[slot] = order
        out["perm"] = perm
    else:
        out["perm"] = order
        if interleave == 2:
            hk = h_keys(h)[order]
            sid = np.cumsum(first) - 1
            by_h = np.lexsort((idx, hk, sid))              # per segment by key; equal keys in Morton order (one of the allowed orders)
            out["segment_keys"] = hk[by_h]
            out["perm_by_h"] = order[by_h]                 # THE permutation when no segment holds two equal keys
    return out


# ---- view culling: the property ---------------------------------------------------------------------------------------
def covered_mask(starts, lens, n):
    d = np.zeros(n + 1, dtype=np.int64)
    np.add.at(d, np.asarray(starts, dtype=np.int64), 1)
    np.add.at(d, np.asarray(starts, dtype=np.int64) + np.asarray(lens, dtype=np.int64), -1)
    return np.cumsum(d)[:n] > 0


def inside_sphere(pos_new, centre, radius):
    """particles that are finite on all axes and strictly inside the sphere (float64)"""
    p = np.asarray(pos_new, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.isfinite(p).all(axis=1) & (np.linalg.norm(p - np.asarray(centre, dtype=np.float64), axis=1) < radius)


def lost_particles(cells, pos_new, centre, radius):
    """select_sphere + ranges(0, n) on a StratifiedCells over positions in the NEW order: (indices of the in-sphere particles
    outside every range, the in-sphere mask, the covered mask).  The first must be empty: exact, no tolerance."""
    n = len(pos_new)
    cells.select_sphere(centre, radius)
    st, ln = cells.ranges(0, n)
    cov = covered_mask(st, ln, n)
    ins = inside_sphere(pos_new, centre, radius)
    return np.flatnonzero(ins & ~cov), ins, cov


def spheres(pos, seed, n_centres=16):
    """The test spheres of a scene: centred on particles and displaced from them by 0, 1e-3, 1 and 30 units in a random
    direction; six radii from 1e-3 to twice the extent (the diagonal of the finite bounding box; 1 when that is 0) in equal
    ratios, and a quarter of the extent (smaller than the box whatever the box's size)."""
    rs = np.random.RandomState(seed)
    p = np.asarray(pos, dtype=np.float64)
    fin = np.isfinite(p)
    anchors = p[fin.all(axis=1)]
    if len(anchors) == 0:
        anchors = np.where(fin, p, 0.0)
    with np.errstate(invalid="ignore"):
        ext = [np.ptp(p[fin[:, a], a]) if fin[:, a].any() else 0.0 for a in range(3)]
    E = float(np.linalg.norm(ext)) or 1.0
    radii = np.append(np.geomspace(1e-3, 2.0 * E, 6), 0.25 * E)
    out = []
    for c in anchors[rs.choice(len(anchors), min(n_centres, len(anchors)), replace=len(anchors) < n_centres)]:
        for d in (0.0, 1e-3, 1.0, 30.0):
            u = rs.normal(size=3)
            s = c + d * u / np.linalg.norm(u)
            out += [(s, float(r)) for r in radii]
    return out


def cell_run_fault(layout, pos_new, rule="fixed"):
    """None when every (stratum, cell) run of `layout` holds exactly the particles whose model cell code is that cell, box_lo
    is the model's (bit patterns), and every finite coordinate of a run lies inside the box the layout reports for its cell,
    box_lo + c * cell_width ... + cell_width, to float32 rounding: x - lo is exact in float64 here, the library's step carries
    two float32 roundings and cell_width one, so the faces may be off by 2^-22 (c + 1) cell_width at the most (an axis of
    cell_width 0 holds box_lo only; a cell of width +inf holds everything).  Otherwise a sentence naming the first condition
    that does not hold.  pos_new: the positions in the new order."""
    ca = int(layout["cells_per_axis"])
    k = ca.bit_length() - 1
    ncell = ca ** 3
    off = np.asarray(layout["offsets"], dtype=np.int64)
    n = len(pos_new)
    if len(off) != int(layout["n_strata"]) * ncell + 1:
        return f"{len(off)} offsets for {layout['n_strata']} strata of {ncell} cells"
    if not (off[0] == 0 and off[-1] == n and (np.diff(off) >= 0).all()):
        return f"the offsets do not ascend from 0 to n = {n}: first {off[0]}, last {off[-1]}, {(np.diff(off) < 0).sum()} descents"
    lo, _, _ = bounding_box(pos_new, rule)
    box_lo = np.asarray(layout["box_lo"]).astype(f32)
    if not np.array_equal(box_lo.view(np.uint32), lo.view(np.uint32)):
        return f"box_lo is {box_lo}, the minimum of the finite coordinates {lo}"
    entry = np.searchsorted(off, np.arange(n), side="right") - 1
    code = entry % ncell
    want = cell_codes(pos_new, k, rule)
    if not np.array_equal(code, want):
        i = int(np.flatnonzero(code != want)[0])
        return (f"{(code != want).sum()} particles lie in the run of another cell than their own: particle {i} at {pos_new[i]} "
                f"in the run of cell {code[i]}, its cell is {want[i]}")
    p = np.asarray(pos_new, dtype=np.float64)
    width = np.asarray(layout["cell_width"], dtype=np.float64)
    for a in range(3):
        c = np.zeros(n, dtype=np.int64)
        for j in range(k):
            c |= ((code >> (3 * j + a)) & 1) << j
        fin = np.isfinite(p[:, a])
        d, c, w = p[fin, a] - np.float64(lo[a]), c[fin].astype(np.float64), width[a]
        if w == 0:
            if not (d == 0).all():
                return f"axis {a}: cell_width 0, but {(d != 0).sum()} finite coordinates differ from box_lo"
        elif np.isinf(w):
            if not (w > 0 and ca == 1):
                return f"axis {a}: cell_width {w} with {ca} cells per axis"
        else:
            tol = 2.0 ** -22 * (c + 1) * w
            out = (d < c * w - tol) | (d > (c + 1) * w + tol)
            if not w > 0 or out.any():
                i = int(np.flatnonzero(out)[0]) if out.any() else 0
                return (f"axis {a}: cell_width {w}, {out.sum()} coordinates outside the box of their cell: x - box_lo = {d[i]} "
                        f"in cell {int(c[i])}, which spans {c[i] * w} .. {(c[i] + 1) * w}")
    return None


# ---- scenes: functions of (n, seed) -> float32 (n, 3) ----------------------------------------------------------------
def _uniform(n, seed, lo=-50.0, hi=50.0):
    return np.random.RandomState(seed).uniform(lo, hi, size=(n, 3)).astype(f32)


def scene_uniform(n, seed):
    return _uniform(n, seed)


def scene_plane(n, seed):
    p = _uniform(n, seed)
    p[:, 2] = 3.5
    return p


def scene_line(n, seed):
    p = _uniform(n, seed)
    p[:, 1], p[:, 2] = -7.25, 3.5
    return p


def scene_point(n, seed):
    return np.tile(np.array([1.5, -2.0, 7.0], dtype=f32), (n, 1))


def scene_duplicates(n, seed):
    base = _uniform(n // 100 + 1, seed)
    return base[np.random.RandomState(seed + 1).permutation(np.arange(n) % len(base))]


def scene_nonfinite(n, seed):
    p = _uniform(n, seed)
    rs = np.random.RandomState(seed + 2)
    for a in range(3):
        for bad in (np.nan, np.inf, -np.inf):
            p[rs.choice(n, max(1, n // 40), replace=False), a] = bad
    return p


def scene_nan_axis(n, seed):
    p = _uniform(n, seed)
    p[:, 1] = np.nan
    return p


def scene_offset(n, seed):
    return (1e4 + np.random.RandomState(seed).uniform(0.0, 1.0, size=(n, 3))).astype(f32)


def scene_denormal(n, seed):
    return np.random.RandomState(seed).randint(0, 4, size=(n, 3)).astype(np.uint32).view(f32)


def scene_outlier(n, seed):
    p = _uniform(n, seed)
    p[n // 2, 0] = 1e30
    return p


def scene_overflow(n, seed):
    """two sentinel rows at +-3e38 on x (the extent overflows float32), and rows between them whose x - lo overflows as well"""
    p = _uniform(n, seed)
    vals = [3e38, -3e38, 1e38, -1e38, 2e38, -2e38, 2.9e38, -2.9e38][:n]
    rows = np.random.RandomState(seed + 3).choice(n, len(vals), replace=False)
    p[rows, 0] = np.array(vals, dtype=f32)
    return p


def scene_negative(n, seed):
    return _uniform(n, seed, -300.0, -200.0)


def scene_on_max(n, seed):
    p = _uniform(n, seed)
    for a in range(3):
        p[a::7, a] = p[:, a].max()
    return p


SCENES = {"uniform": scene_uniform, "plane": scene_plane, "line": scene_line, "point": scene_point,
          "duplicates": scene_duplicates, "nonfinite": scene_nonfinite, "nan_axis": scene_nan_axis, "offset": scene_offset,
          "denormal": scene_denormal, "outlier": scene_outlier, "overflow": scene_overflow, "negative": scene_negative,
          "on_max": scene_on_max}
# the particle count of every scene in the culling checks: 70 000 reaches k = 4 at one stratum
SCENE_N = {"uniform": 70000, "overflow": 70000, "nonfinite": 70000, "plane": 5000, "line": 5000, "point": 5000, "duplicates": 5000,
           "nan_axis": 5000, "offset": 5000, "denormal": 5000, "outlier": 5000, "negative": 5000, "on_max": 5000}
