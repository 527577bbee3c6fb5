"""The float64 host model of tsp_gravity_tree (include/topsy_splat.h, topsy_amd/csrc/tsp_gravity_tree.hip), written plainly.

The same tree as the kernel's: the sources with finite coordinates sorted along a 63-bit Morton curve (the model's own float64
quantisation of the bounding box to 2^21 steps per axis; ties keep the caller's order), leaves of LEAF consecutive sorted
particles, nodes of FANOUT consecutive nodes of the level below, per node M, the centre of mass c, the second moments about c,
the mass-weighted mean of eps^2, the radius b = the distance from c to the farthest corner of the members' bounding box, and the
softening rule 8 (e2_max - e2_min) - e2_min over the members with mass.  The same acceptance rule, but per SINGLE target: dmin is
the distance from the target to c (the kernel takes the distance from the bounding box of a group of 64 targets, which is never
larger: the kernel opens a superset of what the model opens).  Everything in float64, nothing rounded up.

Two options make the model the kernel's term by term (their defaults leave the above as it is):
  stored=True   the records the walk reads -- c, M, e2, the six Q, b, rule -- are rounded once to float32 as store_node does
                (b from the float32 c, b and a positive rule multiplied by 1 + 2^-20 in float32); parents are still formed from the
                unrounded float64 sums; decisions and terms use the rounded records in float64 arithmetic: the header's "float64
                evaluation of the same terms".
  groups=[...]  index arrays of targets; a group's valid targets form a box, dmin is per axis max(lo - c, c - hi, 0), ONE decision
                is made per (group, node) and applied to every target of the group, as `classify` in the kernel does.  Per group the
                model then reports its pair counts, the levels it accepted on and `margin`, the smallest relative distance of any
                tested node from either threshold: below AMBIGUOUS the kernel's float32 test may decide the other way."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

LEAF = 32
FANOUT = 8
GROUP = 64                                   # targets per wave of the kernel
ROUND_UP = np.float32(1.0) + np.float32(2.0 ** -20)
# The kernel's float32 test errs by 10 * 2^-24 and b^2 sits 2^-19 above the true radius squared: 2.5e-6 together.  The model decides
# from the same float32 c and float32 targets, so a margin of 1e-4 covers that forty-fold.
AMBIGUOUS = 1e-4


def as_f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def morton_keys(pos):
    """63-bit keys of float64 positions (n, 3) quantised to 2^21 steps per axis of their bounding box"""
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    extent = hi - lo
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(extent > 0, (pos - lo) * (2.0 ** 21 / np.where(extent > 0, extent, 1.0)), 0.0)
    q = np.clip(np.floor(q), 0, 2 ** 21 - 1).astype(np.uint64)
    keys = np.zeros(len(pos), dtype=np.uint64)
    for bit in range(21):
        for a in range(3):
            keys |= ((q[:, a] >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit + a)
    return keys


def _segments(n, width):
    return np.arange(0, n, width)


def _node_level(M, mc, Q_about, m_e2, lo, hi, e2min, e2max):
    """a level's records from the per-node sums: M, mc = sum m x, ..."""
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(M[:, None] > 0, mc / np.where(M > 0, M, 1.0)[:, None], 0.0)
        e2 = np.where(M > 0, m_e2 / np.where(M > 0, M, 1.0), 1.0)
    return {"M": M, "c": c, "m_e2": m_e2, "e2": e2, "lo": lo, "hi": hi, "e2min": e2min, "e2max": e2max, "Q": Q_about}


def _finish(level):
    c, lo, hi = level["c"], level["lo"], level["hi"]
    far = np.maximum(c - lo, hi - c)
    level["b"] = np.sqrt((far * far).sum(axis=1))
    with np.errstate(invalid="ignore"):
        rule = 8.0 * (level["e2max"] - level["e2min"]) - level["e2min"]
    level["rule"] = np.where(level["M"] > 0, rule, 0.0)
    return level


_PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))      # Q as (xx, yy, zz, xy, xz, yz)


def walk_records(level, stored):
    """what the walk reads of a level's nodes, as float64 arrays: c, M, e2, Q, b, rule.  stored: rounded as store_node rounds"""
    if not stored:
        return {k: level[k] for k in ("c", "M", "e2", "Q", "b", "rule")}
    f32 = np.float32
    massive = level["M"] > 0
    c = np.where(massive[:, None], level["c"], 0.0).astype(f32).astype(np.float64)
    far = np.maximum(c - level["lo"], level["hi"] - c)
    b = np.sqrt((far * far).sum(axis=1)).astype(f32) * ROUND_UP                      # a float32 product
    rule = np.where(level["rule"] > 0, level["rule"].astype(f32) * ROUND_UP, f32(0))
    return {"c": c, "M": level["M"].astype(f32).astype(np.float64),
            "e2": np.where(massive, level["e2"], 1.0).astype(f32).astype(np.float64),
            "Q": np.where(massive[:, None], level["Q"], 0.0).astype(f32).astype(np.float64),
            "b": np.where(massive, b, f32(0)).astype(np.float64), "rule": np.where(massive, rule, f32(0)).astype(np.float64)}


def build_tree(src, mass, eps, stored=False, parallel_axis=True):
    """-> dict: order (sorted -> caller's index), pos, m, e2 of the sorted particles, levels (leaves first), n_valid_sources,
    walk (per level: walk_records(level, stored)).  parallel_axis=False forms a parent's Q without the M_c (c_c - c)(c_c - c)^T
    terms: a deliberately wrong tree, for the tests that show that an assertion would notice."""
    src, mass = as_f32(src), as_f32(mass)
    n = len(src)
    e = np.full(n, np.float32(eps), dtype=np.float32) if np.ndim(eps) == 0 else as_f32(eps)
    finite = np.isfinite(src).all(axis=1)
    caller = np.nonzero(finite)[0]
    pos = src[caller].astype(np.float64)
    order = caller[np.argsort(morton_keys(pos), kind="stable")]
    pos = src[order].astype(np.float64)
    ok = np.isfinite(mass[order]) & np.isfinite(e[order])
    m = np.where(ok, mass[order], 0).astype(np.float64)
    e2 = np.where(ok, e[order].astype(np.float64) ** 2, 1.0)
    nv = len(order)
    seg = _segments(nv, LEAF)
    M = np.add.reduceat(m, seg)
    mc = np.add.reduceat(m[:, None] * pos, seg, axis=0)
    massive = m > 0
    leaf = _node_level(M, mc, None, np.add.reduceat(m * e2, seg), np.minimum.reduceat(pos, seg, axis=0),
                       np.maximum.reduceat(pos, seg, axis=0), np.minimum.reduceat(np.where(massive, e2, np.inf), seg),
                       np.maximum.reduceat(np.where(massive, e2, -np.inf), seg))
    d = pos - leaf["c"][np.arange(nv) // LEAF]
    leaf["Q"] = np.stack([np.add.reduceat(m * d[:, a] * d[:, b], seg) for a, b in _PAIRS], axis=1)
    levels = [_finish(leaf)]
    while len(levels[-1]["M"]) > 1:
        ch = levels[-1]
        k = len(ch["M"])
        seg = _segments(k, FANOUT)
        M = np.add.reduceat(ch["M"], seg)
        mc = np.add.reduceat(ch["M"][:, None] * ch["c"], seg, axis=0)
        parent = _node_level(M, mc, None, np.add.reduceat(ch["m_e2"], seg), np.minimum.reduceat(ch["lo"], seg, axis=0),
                             np.maximum.reduceat(ch["hi"], seg, axis=0), np.minimum.reduceat(ch["e2min"], seg),
                             np.maximum.reduceat(ch["e2max"], seg))
        d = ch["c"] - parent["c"][np.arange(k) // FANOUT]
        shift = 1.0 if parallel_axis else 0.0
        parent["Q"] = np.stack([np.add.reduceat(ch["Q"][:, q] + shift * ch["M"] * d[:, a] * d[:, b], seg)
                                for q, (a, b) in enumerate(_PAIRS)], axis=1)      # the parallel-axis rule (a massless child: M = 0, Q = 0)
        levels.append(_finish(parent))
    return {"order": order, "pos": pos, "m": m, "e2": e2, "levels": levels, "n_valid_sources": int(ok.sum()), "stored": bool(stored),
            "walk": [walk_records(lv, stored) for lv in levels]}


def node_terms(d, M, e2, Q):
    """the softened monopole + quadrupole terms (to be subtracted) of nodes at displacements d = t - c: (pot (k,), acc (k, 3))"""
    r2 = (d * d).sum(axis=1) + e2
    inv = 1.0 / np.sqrt(r2)
    inv2 = inv * inv
    u = d * inv[:, None]
    Qu = np.stack([Q[:, 0] * u[:, 0] + Q[:, 3] * u[:, 1] + Q[:, 4] * u[:, 2],
                   Q[:, 3] * u[:, 0] + Q[:, 1] * u[:, 1] + Q[:, 5] * u[:, 2],
                   Q[:, 4] * u[:, 0] + Q[:, 5] * u[:, 1] + Q[:, 2] * u[:, 2]], axis=1)
    s = (u * Qu).sum(axis=1)
    T = Q[:, 0] + Q[:, 1] + Q[:, 2]
    pot = inv * (M + inv2 * (1.5 * s - 0.5 * T))
    acc = inv2[:, None] * ((M + inv2 * (7.5 * s - 1.5 * T))[:, None] * u - 3.0 * inv2[:, None] * Qu)
    return pot, acc


def node_term_scales(d, M, e2, Q):
    """the magnitudes of node_terms' terms as written there, the monopole part and the quadrupole part added in absolute value:
    (pot (k,), acc (k, 3))"""
    r2 = (d * d).sum(axis=1) + e2
    inv = 1.0 / np.sqrt(r2)
    inv2 = inv * inv
    u = d * inv[:, None]
    Qu = np.stack([Q[:, 0] * u[:, 0] + Q[:, 3] * u[:, 1] + Q[:, 4] * u[:, 2],
                   Q[:, 3] * u[:, 0] + Q[:, 1] * u[:, 1] + Q[:, 5] * u[:, 2],
                   Q[:, 4] * u[:, 0] + Q[:, 5] * u[:, 1] + Q[:, 2] * u[:, 2]], axis=1)
    s = (u * Qu).sum(axis=1)
    T = Q[:, 0] + Q[:, 1] + Q[:, 2]
    pot = inv * (np.abs(M) + np.abs(inv2 * (1.5 * s - 0.5 * T)))
    acc = inv2[:, None] * (np.abs(M[:, None] * u) + np.abs(inv2[:, None] * ((7.5 * s - 1.5 * T)[:, None] * u - 3.0 * Qu)))
    return pot, acc


def sorted_groups(tree, width=GROUP):
    """targets = sources: the kernel's groups, `width` consecutive particles of the sorted order, as caller's indices"""
    order = tree["order"]
    return [order[lo:lo + width] for lo in range(0, len(order), width)]


def consecutive_groups(k, width=GROUP):
    """separate targets: the kernel's groups, `width` consecutive targets of the caller's order"""
    return [np.arange(lo, min(lo + width, k)) for lo in range(0, k, width)]


def _one_group(tree, tgt, members, th2, self_targets):
    """one group's walk and sums -> (its report, pot, acc, pot_scale, acc_scale, terms per target) over its valid targets"""
    recs, order, pos, m, e2 = tree["walk"], tree["order"], tree["pos"], tree["m"], tree["e2"]
    nv, n_levels = len(order), len(recs)
    members = np.asarray(members, dtype=np.int64)
    rr = members[np.isfinite(tgt[members]).all(axis=1)]
    info = {"targets": rr, "pairs_direct": 0, "pairs_node": 0, "margin": np.inf, "accepted_per_level": np.zeros(n_levels, dtype=np.int64)}
    if not len(rr):
        return info, None
    t = tgt[rr].astype(np.float64)
    nt = len(rr)
    lo, hi = t.min(axis=0), t.max(axis=0)
    fn = np.zeros(1, dtype=np.int64)
    taken = []                                                    # (level, accepted nodes)
    for l in range(n_levels - 1, -1, -1):
        r = recs[l]
        c = r["c"][fn]
        g = np.maximum(np.maximum(lo - c, c - hi), 0.0)
        d2 = (g * g).sum(axis=1)
        massive = r["M"][fn] > 0
        b2, rule = r["b"][fn] ** 2, r["rule"][fn]
        accept = massive & (d2 * th2 > b2) & (d2 >= rule)
        with np.errstate(divide="ignore", invalid="ignore"):
            near = np.concatenate([(np.abs(d2 * th2 - b2) / b2)[massive & (b2 > 0)], (np.abs(d2 - rule) / rule)[massive & (rule > 0)]])
        if len(near):
            info["margin"] = min(info["margin"], float(near.min()))
        if accept.any():
            taken.append((l, fn[accept]))
            info["accepted_per_level"][l] = int(accept.sum())
        width = FANOUT if l > 0 else LEAF
        limit = len(recs[l - 1]["M"]) if l > 0 else nv
        child = (fn[massive & ~accept][:, None] * width + np.arange(width)[None, :]).ravel()
        fn = child[child < limit]
    p_sum, a_sum = np.zeros(nt), np.zeros((nt, 3))
    p_abs, a_abs = np.zeros(nt), np.zeros((nt, 3))
    terms = np.zeros(nt, dtype=np.int64)
    for l, nodes in taken:
        r = recs[l]
        d = (t[:, None, :] - r["c"][nodes][None, :, :]).reshape(-1, 3)
        args = (d, np.tile(r["M"][nodes], nt), np.tile(r["e2"][nodes], nt), np.tile(r["Q"][nodes], (nt, 1)))
        p, a = node_terms(*args)
        ps, as_ = node_term_scales(*args)
        p_sum += p.reshape(nt, -1).sum(axis=1)
        a_sum += a.reshape(nt, -1, 3).sum(axis=1)
        p_abs += ps.reshape(nt, -1).sum(axis=1)
        a_abs += as_.reshape(nt, -1, 3).sum(axis=1)
        info["pairs_node"] += nt * len(nodes)
        terms += len(nodes)
    # what is left: the particles of the opened leaves, each with every target of the group (axis by axis: (nt, particles) arrays)
    x = pos[fn]
    d = [t[:, a, None] - x[None, :, a] for a in range(3)]
    r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + e2[fn][None, :]
    skip = r2 <= 0.0
    n_pairs = nt * len(fn)
    if self_targets:
        own = order[fn][None, :] == rr[:, None]
        skip |= own
        n_pairs -= int(own.sum())
        terms -= own.sum(axis=1)
    r2[skip] = 1.0
    inv = 1.0 / np.sqrt(r2)
    inv[skip] = 0.0
    p = m[fn][None, :] * inv                                      # (every term of the potential has one sign: m >= 0)
    w = p * inv * inv
    info["pairs_direct"] = n_pairs
    terms += len(fn)
    p_sum += p.sum(axis=1)
    p_abs += p.sum(axis=1)
    for a in range(3):
        wd = w * d[a]
        a_sum[:, a] += wd.sum(axis=1)
        a_abs[:, a] += np.abs(wd, out=wd).sum(axis=1)
    return info, (-p_sum, -a_sum, p_abs, a_abs, terms)


def _group_sums(tree, tgt, groups, theta, self_targets):
    """tree_sum with one decision per (group, node): see the module's docstring"""
    k = len(tgt)
    pot, acc = np.full(k, np.nan), np.full((k, 3), np.nan)
    pot_scale, acc_scale = np.zeros(k), np.zeros((k, 3))
    per_target = np.zeros(k, dtype=np.int64)
    th2 = float(theta) ** 2
    # the groups are independent and NumPy releases the interpreter in its loops: a few threads, the same sums in the same order
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        results = list(pool.map(lambda members: _one_group(tree, tgt, members, th2, self_targets), groups))
    report = []
    for info, sums in results:
        report.append(info)
        if sums is not None:
            rr = info["targets"]
            pot[rr], acc[rr], pot_scale[rr], acc_scale[rr], per_target[rr] = sums
    n_levels = len(tree["walk"])
    return {"pot": pot, "acc": acc, "pot_scale": pot_scale, "acc_scale": acc_scale, "groups": report,
            "pairs_direct": sum(g["pairs_direct"] for g in report), "pairs_node": sum(g["pairs_node"] for g in report),
            "accepted_per_level": sum((g["accepted_per_level"] for g in report), np.zeros(n_levels, dtype=np.int64)),
            "per_target_pairs": per_target, "n_valid_sources": tree["n_valid_sources"], "n_levels": n_levels,
            "n_nodes": sum(len(r["M"]) for r in tree["walk"])}


def tree_sum(src, mass, eps, targets=None, theta=0.5, rows=None, block=256, tree=None, stored=False, groups=None):
    """The model's potential and acceleration at `targets` (k, 3), or at the sources (None: the pair of a particle with itself, by
    the caller's index, is left out).  rows: the targets to evaluate (indices; the others stay NaN and are not counted).
    -> dict pot (k,), acc (k, 3) (NaN at a target with a non-finite coordinate), pairs_direct, pairs_node (summed over the
    evaluated valid targets), per_target_pairs (k,), n_valid_sources, n_levels, n_nodes.
    stored, groups: the module's docstring (a `tree` that is passed in was built with its own `stored`; stored=True without groups:
    every target of `rows` is a group of its own).  Then the dict also holds pot_scale (k,) and acc_scale (k, 3), the sums of
    |term| over the leaf pairs and node terms, accepted_per_level, and groups: per group a dict with targets (its valid ones),
    pairs_direct, pairs_node, margin and accepted_per_level."""
    tree = tree or build_tree(src, mass, eps, stored=stored)
    self_targets = targets is None
    tgt = as_f32(src) if self_targets else as_f32(targets)
    k = len(tgt)
    if groups is not None or tree["stored"]:
        if groups is None:
            groups = [[i] for i in (range(k) if rows is None else rows)]
        return _group_sums(tree, tgt, groups, theta, self_targets)
    rows = np.arange(k) if rows is None else np.asarray(rows)
    rows = rows[np.isfinite(tgt[rows]).all(axis=1)]
    levels, order, pos, m, e2 = tree["levels"], tree["order"], tree["pos"], tree["m"], tree["e2"]
    nv = len(order)
    pot = np.full(k, np.nan)
    acc = np.full((k, 3), np.nan)
    per_target = np.zeros(k, dtype=np.int64)
    pairs_direct = pairs_node = 0
    th2 = float(theta) ** 2
    for lo in range(0, len(rows), block):
        rr = rows[lo:lo + block]
        t = tgt[rr].astype(np.float64)
        nb = len(rr)
        p_sum, a_sum = np.zeros(nb), np.zeros((nb, 3))
        ft, fn = np.arange(nb), np.zeros(nb, dtype=np.int64)          # the frontier: (target of the block, node of the level)
        for l in range(len(levels) - 1, -1, -1):
            lv = levels[l]
            d = t[ft] - lv["c"][fn]
            d2 = (d * d).sum(axis=1)
            massive = lv["M"][fn] > 0
            accept = massive & (d2 * th2 > lv["b"][fn] ** 2) & (d2 >= lv["rule"][fn])
            opened = massive & ~accept
            if accept.any():
                g = fn[accept]
                p, a = node_terms(d[accept], lv["M"][g], lv["e2"][g], lv["Q"][g])
                p_sum += np.bincount(ft[accept], weights=p, minlength=nb)
                for c in range(3):
                    a_sum[:, c] += np.bincount(ft[accept], weights=a[:, c], minlength=nb)
                pairs_node += int(accept.sum())
                per_target[rr] += np.bincount(ft[accept], minlength=nb)
            width = FANOUT if l > 0 else LEAF
            limit = len(levels[l - 1]["M"]) if l > 0 else nv
            child = (fn[opened][:, None] * width + np.arange(width)[None, :]).ravel()
            ct = np.repeat(ft[opened], width)
            keep = child < limit
            ft, fn = ct[keep], child[keep]
        # what is left: (target, sorted particle) pairs of the opened leaves
        d = t[ft] - pos[fn]
        r2 = (d * d).sum(axis=1) + e2[fn]
        counts = r2 > 0.0
        if self_targets:
            evaluated = order[fn] != rr[ft]
            counts &= evaluated
        else:
            evaluated = np.ones(len(fn), dtype=bool)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = np.where(counts, 1.0 / np.sqrt(np.where(counts, r2, 1.0)), 0.0)
        p = m[fn] * inv
        w = (p * inv * inv)[:, None] * d
        p_sum += np.bincount(ft, weights=p, minlength=nb)
        for c in range(3):
            a_sum[:, c] += np.bincount(ft, weights=w[:, c], minlength=nb)
        pairs_direct += int(evaluated.sum())
        per_target[rr] += np.bincount(ft[evaluated], minlength=nb)
        pot[rr] = -p_sum
        acc[rr] = -a_sum
    return {"pot": pot, "acc": acc, "pairs_direct": pairs_direct, "pairs_node": pairs_node, "per_target_pairs": per_target,
            "n_valid_sources": tree["n_valid_sources"], "n_levels": len(levels), "n_nodes": sum(len(lv["M"]) for lv in levels)}


def relative_acc_error(acc, ref_acc):
    """e = |a - a_ref| / |a_ref| per target"""
    return np.linalg.norm(np.asarray(acc) - ref_acc, axis=1) / np.linalg.norm(ref_acc, axis=1)
