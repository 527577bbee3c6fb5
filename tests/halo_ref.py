"""The float64 numpy model of tsp_group_potential and tsp_halo_properties (include/topsy_splat.h), and the scenes of their tests.

The model follows the contract to the bit where the contract fixes the bits: the anchor (the valid member with the smallest
index), the offsets d = (double)x - (double)a with d -= period * rint(d / period), e = (float)d for the pair sums, the key
(float)|e| with index ties, and -- for the float64 sums of the properties -- the documented association: the members in sorted
order (by label, then index), partial sums over slices of 256 consecutive sorted positions, a halo's partials added in 64 chunks
of consecutive partials, then the chunks.  The pair sums are formed in float64 on the float32 e, m, eps (the library's are float32:
it is held to K * 2^-24 * sum |term|).  The model also flags what float32 cannot decide.  work_items and piece_layout restate the
documented planning rule of the pair kernel and the piece layout of the reductions, for the tests that must know which path a
scene takes."""
import numpy as np

f32, f64 = np.float32, np.float64
K = 64                      # TSP_GRAVITY_ERROR_K
U = 2.0 ** -24
SLICE = 256
R2_NORMAL = 2.0 ** -126
CLUMP_SIZES = (1, 2, 19, 20, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 3000)      # 8610 in all
N_BACKGROUND = 500
GIANTS_SEED = 11


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def _plummer(rs, n, a):
    """n positions of a Plummer sphere of scale radius a, cut at 8 a"""
    u = rs.uniform(0.0, (1.0 + 1.0 / 64.0) ** -1.5, n)           # M(<r) / M at r = 8 a
    r = a / np.sqrt(np.maximum(u, 1e-12) ** (-2.0 / 3.0) - 1.0)
    v = rs.normal(size=(n, 3))
    return r[:, None] * v / np.linalg.norm(v, axis=1)[:, None]


def clumps(periodic=False, seed=8):
    """dict(pos, vel (n, 3) f32, mass, eps (n,) f32, labels int32 (n,), n_groups, period).  (The seed is one at which no member's
    radial key is ambiguous -- about one seed in two has such a member among the 8610; test_halo_cpu.py asserts the condition.)"""
    rs = np.random.RandomState(seed)
    sizes = sorted(CLUMP_SIZES, reverse=True)                  # label = size rank, 1 the largest
    centres = rs.uniform(0.15, 0.85, size=(len(sizes), 3))
    if periodic:
        centres[0] = (0.0, 0.0, 0.0)                           # a corner
        centres[3] = (0.0, 1.0, 0.37)                          # an edge
        centres[5] = (0.61, 0.27, 0.0)                         # a face
    pos, vel, mass, labels = [], [], [], []
    for k, n in enumerate(sizes):
        a = 0.004 * (max(n, 8) / 64.0) ** (1.0 / 3.0)
        m = rs.uniform(0.5, 1.5, n) * 1e-4
        sigma = 0.9 * np.sqrt(m.sum() / (6.0 * a))
        pos.append(centres[k] + _plummer(rs, n, a))
        vel.append(rs.normal(size=3) * 0.3 + rs.normal(size=(n, 3)) * sigma)
        mass.append(m)
        labels.append(np.full(n, k + 1))
    pos.append(rs.uniform(0.0, 1.0, size=(N_BACKGROUND, 3)))
    vel.append(rs.normal(size=(N_BACKGROUND, 3)))
    mass.append(rs.uniform(0.5, 1.5, N_BACKGROUND) * 1e-4)
    labels.append(rs.choice([0, -1, -7], N_BACKGROUND))
    pos, vel, mass, labels = np.concatenate(pos), np.concatenate(vel), np.concatenate(mass), np.concatenate(labels)
    if periodic:
        pos = pos - np.floor(pos)
    order = rs.permutation(len(pos))
    eps = rs.uniform(1.0, 2.0, len(pos)) * 2e-4
    return dict(pos=pos[order].astype(f32), vel=vel[order].astype(f32), mass=mass[order].astype(f32), eps=eps.astype(f32),
                labels=labels[order].astype(np.int32), n_groups=len(sizes), period=1.0 if periodic else 0.0)


def crumbs(seed=11):
    """3000 haloes of 1 to 3 members; n_groups = 3005: the last five labels are empty"""
    rs = np.random.RandomState(seed)
    sizes = rs.randint(1, 4, 3000)
    labels = np.repeat(np.arange(1, 3001), sizes)
    centres = rs.uniform(0.0, 1.0, size=(3000, 3))
    pos = centres[labels - 1] + rs.normal(size=(len(labels), 3)) * 1e-3
    n = len(labels)
    order = rs.permutation(n)
    return dict(pos=pos[order].astype(f32), vel=rs.normal(size=(n, 3)).astype(f32), mass=(rs.uniform(0.5, 1.5, n) * 1e-4).astype(f32),
                eps=np.full(n, 2e-4, dtype=f32), labels=labels[order].astype(np.int32), n_groups=3005, period=0.0)


# edges(): sizes in label order; the sorted start of every halo (the running sum) is in the comment
EDGE_SIZES = (256,          # 0     exactly one aligned slice
              256,          # 256   not the first halo, starts and ends on a slice boundary, exactly one aligned slice
              255,          # 512
              256,          # 767   starts at offset 255 of a slice: its B piece has one member
              1,            # 1023  ends at a multiple of 1024: the next halo starts a block
              1024,         # 1024  exactly one aligned block: a uniform block whose halo is two tiles, both the block's own
              10, 9,        # 2048, 2058: v2_max needs rank >= 10
              235,          # 2067
              1, 1, 1, 1, 1,  # 2302 .. 2306: one-member haloes across the slice boundary at 2304
              700,          # 2307
              65)           # 3007  ends at 3072 = 6 * 512: no padding source
# giants(): the smallest sizes that reach each chunk class of halo_combine; spacers set the alignment
GIANT_SIZES = (16384,       # 0      aligned: 64 pieces, chunk 1, 64 lanes
               100,         # 16384
               16384,       # 16484  misaligned: 65 pieces with a B piece, chunk 2, 33 lanes
               156,         # 32868
               32768,       # 33024  aligned: 128 pieces, chunk 2, 64 lanes
               32769)       # 65792  aligned: 129 pieces, chunk 3, 43 lanes; ends at 98561
GIANT_LABELS = dict(aligned_16384=1, misaligned_16384=3, aligned_32768=5, aligned_32769=6)
# legion(): giants() and haloes of at least 15872 members (31 tiles: every block's range is cut into 16 work items)
LEGION_SIZES = GIANT_SIZES + (15901, 16007, 16133, 15877, 16211, 15959, 16063, 16301, 15923, 16177, 16039, 15991)
LEGION_MAX_MEMBERS = 20000
N_BACKGROUND_BIG = 300
MAX_TARGETS = 1000          # of target_sample on the big scenes


def spheres(sizes, seed, n_background=N_BACKGROUND_BIG):
    """Plummer spheres of the given sizes, masses, eps and velocities as in clumps(); label k + 1 has sizes[k] members, so the
    sorted starts are the running sums of sizes; particles permuted, background particles with labels in {0, -1, -7}"""
    rs = np.random.RandomState(seed)
    centres = rs.uniform(0.15, 0.85, size=(len(sizes), 3))
    pos, vel, mass, labels = [], [], [], []
    for k, n in enumerate(sizes):
        a = 0.004 * (max(n, 8) / 64.0) ** (1.0 / 3.0)
        m = rs.uniform(0.5, 1.5, n) * 1e-4
        sigma = 0.9 * np.sqrt(m.sum() / (6.0 * a))
        pos.append(centres[k] + _plummer(rs, n, a))
        vel.append(rs.normal(size=3) * 0.3 + rs.normal(size=(n, 3)) * sigma)
        mass.append(m)
        labels.append(np.full(n, k + 1))
    pos.append(rs.uniform(0.0, 1.0, size=(n_background, 3)))
    vel.append(rs.normal(size=(n_background, 3)))
    mass.append(rs.uniform(0.5, 1.5, n_background) * 1e-4)
    labels.append(rs.choice([0, -1, -7], n_background))
    pos, vel, mass, labels = np.concatenate(pos), np.concatenate(vel), np.concatenate(mass), np.concatenate(labels)
    order = rs.permutation(len(pos))
    eps = rs.uniform(1.0, 2.0, len(pos)) * 2e-4
    return dict(pos=pos[order].astype(f32), vel=vel[order].astype(f32), mass=mass[order].astype(f32), eps=eps.astype(f32),
                labels=labels[order].astype(np.int32), n_groups=len(sizes), period=0.0)


def edges(extra=0, seed=5):
    """The piece, tile and block edges of the sorted layout (EDGE_SIZES): 3072 members, a multiple of 512 -- no padding source;
    extra = 1 gives the last halo one more member.  (test_halo_cpu.py asserts every layout class and n_key_ambiguous == 0.)"""
    return spheres(EDGE_SIZES[:-1] + (EDGE_SIZES[-1] + extra,), seed)


def giants(seed=GIANTS_SEED):
    """98561 members: haloes of 64, 65, 128 and 129 pieces.  (The seed is one at which no member's radial key is ambiguous: at
    about 2e-5 per member roughly one seed in ten, 11 the first of them; test_halo_cpu.py asserts the condition.)"""
    return spheres(GIANT_SIZES, seed)


def legion(seed=GIANTS_SEED):
    """giants() and twelve haloes of about 16000 members, misaligned and unequal: more than 4096 work items, two launches, the
    break inside a halo (test_halo_cpu.py asserts it).  Potential only."""
    return spheres(LEGION_SIZES, seed)


def sparse_labels(scene, n_groups=2 ** 18):
    """The scene with its labels 1..H mapped, in order, to H values spread over 1..n_groups (1 and n_groups among them): the
    sorted layout is the same.  (scene, the new label of every old one)"""
    H = scene["n_groups"]
    new = np.concatenate([[0], np.rint(np.linspace(1, n_groups, H)).astype(np.int64)])
    assert (np.diff(new) > 0).all()
    lab = scene["labels"]
    return dict(scene, labels=np.where(lab >= 1, new[np.maximum(lab, 0)], lab).astype(np.int32), n_groups=n_groups), new[1:]


NONFINITE_FIELDS = ("x", "y", "z", "mass", "eps", "vx", "vy", "vz")


def nonfinite_clumps():
    """The first scene with eight members made non-finite, one field each: the member with the smallest index of eight haloes
    (the anchor moves to the next member)."""
    s = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in clumps().items()}
    bad = [np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan, -np.inf, np.nan]
    for k, (field, value) in enumerate(zip(NONFINITE_FIELDS, bad)):
        i = np.flatnonzero(s["labels"] == 2 * k + 1)[0]
        if field in "xyz":
            s["pos"][i, "xyz".index(field)] = value
        elif field in ("vx", "vy", "vz"):
            s["vel"][i, ("vx", "vy", "vz").index(field)] = value
        else:
            s[field][i] = value
    return s


def reordered(scene, how, seed=3):
    """The scene with the caller's order sorted by label, reversed or permuted: (scene, order) with new[k] = old[order[k]]"""
    n = len(scene["labels"])
    order = {"sorted": np.argsort(scene["labels"], kind="stable"), "reversed": np.arange(n)[::-1],
             "permuted": np.random.RandomState(seed).permutation(n)}[how]
    return {k: (np.ascontiguousarray(v[order]) if isinstance(v, np.ndarray) else v) for k, v in scene.items()}, order


# ---- the shared front end -----------------------------------------------------------------------------------------------------
def members_of(labels, valid, n_groups):
    """[the ascending indices of the valid members of label g + 1], and the sorted position of every halo's first member"""
    member = valid & (labels >= 1) & (labels <= n_groups)
    idx = np.flatnonzero(member)
    order = idx[np.argsort(labels[idx], kind="stable")]
    counts = np.bincount(labels[idx], minlength=n_groups + 1)[1:]
    starts = np.concatenate([[0], np.cumsum(counts)])
    return [order[starts[g]:starts[g + 1]] for g in range(n_groups)], starts[:-1]


def offsets(pos, idx, period):
    p = pos[idx].astype(f64)
    d = p - p[0]
    if period > 0:
        d = d - period * np.rint(d / period)
    return d


# ---- tsp_group_potential --------------------------------------------------------------------------------------------------------
def potential_model(scene, max_members=0, targets=None):
    """dict(phi (n,) float64, NaN as the library; scale (n,) = sum |term| (the bound is K * U * scale); info; counts (n_groups,),
    the valid members of every label; member_has_value (n,) bool: where the library has a value).  With targets (the caller's
    indices) phi and scale are formed for those members only -- rows of a (targets in the halo) x (members of the halo) matrix,
    the same bits as the full model's -- and are NaN and 0 elsewhere; info, counts and member_has_value are for every particle."""
    pos, mass, eps, labels, n_groups, period = (scene[k] for k in ("pos", "mass", "eps", "labels", "n_groups", "period"))
    n = len(pos)
    eps = np.broadcast_to(np.asarray(eps, dtype=f32), (n,))
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(pos).all(axis=1) & np.isfinite(mass) & np.isfinite(eps)
    groups, _ = members_of(labels, valid, n_groups)
    wanted = np.ones(n, dtype=bool)
    if targets is not None:
        wanted = np.zeros(n, dtype=bool)
        wanted[np.asarray(targets, dtype=np.int64)] = True
    phi, scale, has_value = np.full(n, np.nan), np.zeros(n), np.zeros(n, dtype=bool)
    info = dict(n_members=0, n_groups_nonempty=0, pairs=0, n_skipped_groups=0, n_skipped_members=0, max_extent=0.0)
    for idx in groups:
        c = len(idx)
        if c == 0:
            continue
        info["n_members"] += c
        info["n_groups_nonempty"] += 1
        d = offsets(pos, idx, period)
        info["max_extent"] = max(info["max_extent"], float(np.abs(d).max()))
        if max_members and c > max_members:
            info["n_skipped_groups"] += 1
            info["n_skipped_members"] += c
            continue
        info["pairs"] += c * (c - 1)
        has_value[idx] = True
        rows_all = np.flatnonzero(wanted[idx])
        e = d.astype(f32).astype(f64)
        e2 = (eps[idx] * eps[idx]).astype(f64)                  # (one float32 rounding, as the library)
        m = mass[idx].astype(f64)
        step = max(1, (1 << 24) // c)                           # (rows at a time: the matrices stay below 128 MB)
        for k in range(0, len(rows_all), step):
            rows = rows_all[k:k + step]
            r2 = np.zeros((len(rows), c))
            for a in range(3):
                diff = e[rows, None, a] - e[None, :, a]
                r2 += diff * diff
            r2 += e2[None, :]
            with np.errstate(divide="ignore"):
                term = m[None, :] / np.sqrt(r2)
            term[(r2 < R2_NORMAL) | (rows[:, None] == np.arange(c)[None, :])] = 0.0
            phi[idx[rows]] = -term.sum(axis=1)
            scale[idx[rows]] = np.abs(term).sum(axis=1)
    return dict(phi=phi, scale=scale, info=info, counts=np.array([len(idx) for idx in groups], dtype=np.int64),
                member_has_value=has_value, targets=None if targets is None else np.asarray(targets, dtype=np.int64))


def sorted_positions(scene):
    """(the caller's index of every sorted position, the sorted start of every label, the counts) of tsp_group_potential's members"""
    pos, mass, labels, n_groups = (scene[k] for k in ("pos", "mass", "labels", "n_groups"))
    eps = np.broadcast_to(np.asarray(scene["eps"], dtype=f32), (len(pos),))
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(pos).all(axis=1) & np.isfinite(mass) & np.isfinite(eps)
    groups, starts = members_of(labels, valid, n_groups)
    return np.concatenate(groups), starts, np.array([len(g) for g in groups], dtype=np.int64)


def target_sample(scene, per_halo_random, seed, cap=MAX_TARGETS):
    """The caller's indices (ascending) of: every halo's first and last sorted member; the members whose sorted position p has
    p % 1024 in {0, 255, 256, 1023} (block and lane-plane edges) or p % 512 in {0, 511} (tile edges); per_halo_random random
    members of every halo.  Above cap targets the edge members are thinned at random, class by class, to fit."""
    rs = np.random.RandomState(seed)
    index, starts, counts = sorted_positions(scene)
    full = counts > 0
    ends = np.concatenate([starts[full], starts[full] + counts[full] - 1])
    rand = np.concatenate([s + rs.choice(c, min(c, per_halo_random), replace=False) for s, c in zip(starts[full], counts[full])]
                          + [np.zeros(0, dtype=np.int64)])
    p = np.arange(len(index))
    classes = [p[p % 1024 == r] for r in (0, 255, 256, 1023)] + [p[p % 512 == r] for r in (0, 511)]
    room = cap - len(np.union1d(ends, rand))
    if sum(len(c) for c in classes) > room:
        each = max(1, room // len(classes))
        classes = [c if len(c) <= each else rs.choice(c, each, replace=False) for c in classes]
    return np.sort(index[np.unique(np.concatenate([ends, rand] + classes))])


# ---- the planning rule of tsp_group_potential (include/topsy_splat.h) ---------------------------------------
BLOCK, TILE_SOURCES, SPLIT_TILES, MAX_SPLITS, MAX_ITEMS = 1024, 512, 2, 16, 4096


def work_items(counts, max_members=0):
    """The work items of a catalogue whose labels 1, 2, ... have counts[] valid members.  Per block of 1024 sorted targets: the
    tiles [floor(lo / 512), ceil(hi / 512)) that hold the non-skipped haloes it touches, cut into min(16, ceil(tiles / 2)) items
    at t0 + tiles * s // splits; a new launch where one would exceed 4096 items.  dict(items [(block, tile0, tile1, slot in its
    launch)], launches [(block0, block1, n_items)], splits_per_block, pair_slots = tiles * 512 * 1024 summed)."""
    counts = np.asarray(counts, dtype=np.int64)
    counts = counts[counts > 0]
    ends = np.cumsum(counts)
    starts = ends - counts
    n_members = int(ends[-1]) if len(ends) else 0
    keep = ~((counts > max_members) if max_members else np.zeros(len(counts), dtype=bool))
    items, launches, splits_per_block, pair_slots = [], [], [], 0
    block0, in_launch = 0, 0
    for b in range(-(-n_members // BLOCK)):
        first, last = b * BLOCK, min(n_members, (b + 1) * BLOCK)
        touched = (starts < last) & (ends > first) & keep
        splits = 0
        if touched.any():
            t0, t1 = int(starts[touched].min()) // TILE_SOURCES, -(-int(ends[touched].max()) // TILE_SOURCES)
            nt = t1 - t0
            splits = min(MAX_SPLITS, -(-nt // SPLIT_TILES))
            pair_slots += nt * TILE_SOURCES * BLOCK
        if in_launch + splits > MAX_ITEMS:
            launches.append((block0, b, in_launch))
            block0, in_launch = b, 0
        for s in range(splits):
            items.append((b, t0 + nt * s // splits, t0 + nt * (s + 1) // splits, in_launch + s))
        in_launch += splits
        splits_per_block.append(splits)
    if n_members:
        launches.append((block0, -(-n_members // BLOCK), in_launch))
    return dict(items=items, launches=launches, splits_per_block=np.array(splits_per_block, dtype=np.int64), pair_slots=pair_slots)


# ---- tsp_halo_properties --------------------------------------------------------------------------------------------------------
def _pieces(k, start):
    """the runs [p, q) of a halo of k members whose first sorted position is start, cut at the multiples of SLICE"""
    out, p = [], 0
    while p < k:
        q = min(k, ((start + p) // SLICE + 1) * SLICE - start)
        out.append((p, q))
        p = q
    return out


def piece_layout(start, count):
    """(has_b, pieces, chunk, lanes_used) of a halo of count members whose first sorted position is start: whether its first piece
    starts inside a slice (B), its pieces, the consecutive pieces a lane of halo_combine adds, the lanes that hold a value"""
    pieces = len(_pieces(count, start))
    chunk = -(-pieces // 64)
    return int(start % SLICE != 0 and count > 0), pieces, chunk, -(-pieces // chunk) if pieces else 0


def _seq(rows):
    s = rows[0].copy()
    for r in rows[1:]:
        s = s + r
    return s


def ordered_sum(terms, start):
    """the sum of the rows of terms (k, c) in the library's association"""
    pieces = [_seq(terms[p:q]) for p, q in _pieces(len(terms), start)]
    chunk = -(-len(pieces) // 64)
    return _seq([_seq(pieces[l:l + chunk]) for l in range(0, len(pieces), chunk)])


def ordered_cumsum(m, start):
    """the running sum of m (k,) in the library's association: the exclusive prefix of the pieces, then the prefix inside"""
    runs = _pieces(len(m), start)
    sums = [_seq(m[p:q]) for p, q in runs]
    chunk = -(-len(runs) // 64)
    out, before = np.empty(len(m)), 0.0
    for l in range(0, len(runs), chunk):
        lane, acc = 0.0, before
        for (p, q), s in zip(runs[l:l + chunk], sums[l:l + chunk]):
            within = m[p]
            out[p] = acc + within
            for r in range(p + 1, q):
                within = within + m[r]
                out[r] = acc + within
            acc = acc + s
            lane = lane + s
        before = before + lane
    return out


def key_ambiguous(r):
    """|e| within 2^-40 relative of a float32 rounding boundary: the key (float)|e| could round either way"""
    f = r.astype(f32)
    lo, hi = np.nextafter(f, f32(-np.inf)).astype(f64), np.nextafter(f, f32(np.inf)).astype(f64)
    f = f.astype(f64)
    return (np.minimum(np.abs(r - 0.5 * (f + lo)), np.abs(r - 0.5 * (f + hi))) <= 2.0 ** -40 * r) & (r > 0)


def properties_model(scene, phi=None, with_vel=True, phi_bound=None):
    """The properties of every halo, arrays of length n_groups (the library's columns by name), with the scales of the float64
    sums' bounds (scale_*), the member count n_sum of the bound, and the flags: with phi_bound (n,) -- the error bound of the
    float32 potential that phi may differ by -- n_bound_sure / n_bound_ambiguous, m_bound_sure / m_bound_ambiguous (members
    with |E| <= phi_bound), pot_ambiguous (the two lowest phi closer than the sum of their bounds); key_ambiguous (members)."""
    pos, mass, labels, n_groups, period = (scene[k] for k in ("pos", "mass", "labels", "n_groups", "period"))
    vel = scene["vel"] if with_vel else None
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(pos).all(axis=1) & np.isfinite(mass) & (mass > 0)
        if vel is not None:
            valid &= np.isfinite(vel).all(axis=1)
    groups, starts = members_of(labels, valid, n_groups)
    H = n_groups
    nan = lambda *shape: np.full((H,) + shape, np.nan)
    out = dict(count=np.zeros(H, dtype=np.int64), n_bound=np.full(H, -1, dtype=np.int64), i_pot=np.full(H, -1, dtype=np.int64),
               i_half=np.full(H, -1, dtype=np.int64), i_vmax=np.full(H, -1, dtype=np.int64), mass=np.zeros(H), com=nan(3),
               v_com=nan(3), S=nan(6), L=nan(3), e_kin=nan(), sigma2=nan(), r_max=nan(), r_half=nan(), v2_max=nan(), r_vmax=nan(),
               e_pot=nan(), m_bound=nan(), pot_pos=nan(3), scale_com=nan(), scale_S=nan(), scale_L=nan(), scale_e_kin=nan(),
               scale_e_pot=nan(), scale_v_com=nan(), n_bound_sure=np.zeros(H, dtype=np.int64), n_bound_ambiguous=np.zeros(H, dtype=np.int64),
               m_bound_sure=np.zeros(H), m_bound_ambiguous=np.zeros(H), pot_ambiguous=np.zeros(H, dtype=bool),
               n_key_ambiguous=0, n_energy_ambiguous=0, n_members=0, max_extent=0.0)
    for g, idx in enumerate(groups):
        c, start = len(idx), int(starts[g])
        if c == 0:
            continue
        out["n_members"] += c
        out["count"][g] = c
        d = offsets(pos, idx, period)
        out["max_extent"] = max(out["max_extent"], float(np.abs(d).max()))
        m = mass[idx].astype(f64)
        v = vel[idx].astype(f64) if vel is not None else np.zeros((c, 3))
        s1 = ordered_sum(np.column_stack([m, m[:, None] * d, m[:, None] * v]), start)
        M, com_off, v_com = s1[0], s1[1:4] / s1[0], s1[4:7] / s1[0]
        com = pos[idx[0]].astype(f64) + com_off
        if period > 0:
            com = com - period * np.floor(com / period)
            com = np.where(com >= period, com - period, com)
        out["mass"][g], out["com"][g] = M, com
        e = d - com_off
        w = v - v_com if vel is not None else np.zeros((c, 3))
        w2 = w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1] + w[:, 2] * w[:, 2]
        r = np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2])
        cols = [m * e[:, 0] * e[:, 0], m * e[:, 0] * e[:, 1], m * e[:, 0] * e[:, 2], m * e[:, 1] * e[:, 1], m * e[:, 1] * e[:, 2],
                m * e[:, 2] * e[:, 2], m * (e[:, 1] * w[:, 2] - e[:, 2] * w[:, 1]), m * (e[:, 2] * w[:, 0] - e[:, 0] * w[:, 2]),
                m * (e[:, 0] * w[:, 1] - e[:, 1] * w[:, 0]), m * w2]
        if phi is not None:
            ph = phi[idx]
            bound = 0.5 * w2 + ph < 0.0
            cols += [m * ph, np.where(bound, m, 0.0)]
        with np.errstate(invalid="ignore"):
            s2 = ordered_sum(np.column_stack(cols), start)
        out["S"][g], out["r_max"][g] = s2[:6], r.max()
        # com = a + sum m d / M: the sum's scale M max|d| over M, and one rounding of the last addition
        out["scale_com"][g], out["scale_S"][g] = np.abs(d).max() + np.abs(com).max(), M * r.max() ** 2
        if vel is not None:
            out["v_com"][g], out["L"][g], out["e_kin"][g] = v_com, s2[6:9], 0.5 * s2[9]
            out["sigma2"][g] = 2.0 * (0.5 * s2[9]) / (3.0 * M)
            out["scale_L"][g], out["scale_e_kin"][g] = M * r.max() * np.sqrt(w2.max()), M * w2.max()
            out["scale_v_com"][g] = np.abs(v).max()
        if phi is not None and np.isfinite(ph).all():
            out["e_pot"][g], out["m_bound"][g], out["n_bound"][g] = 0.5 * s2[10], s2[11], int(bound.sum())
            out["scale_e_pot"][g] = (m * np.abs(ph)).sum()
            k = np.lexsort((idx, ph))[0]
            out["i_pot"][g], out["pot_pos"][g] = idx[k], pos[idx[k]].astype(f64)
            if phi_bound is not None:
                b = phi_bound[idx]
                ambiguous = np.abs(0.5 * w2 + ph) <= b
                out["n_energy_ambiguous"] += int(ambiguous.sum())
                out["n_bound_sure"][g], out["n_bound_ambiguous"][g] = int((bound & ~ambiguous).sum()), int(ambiguous.sum())
                out["m_bound_sure"][g], out["m_bound_ambiguous"][g] = m[bound & ~ambiguous].sum(), m[ambiguous].sum()
                if c >= 2:
                    lo = np.argsort(ph, kind="stable")[:2]
                    out["pot_ambiguous"][g] = ph[lo[1]] - ph[lo[0]] <= b[lo[0]] + b[lo[1]]
        # pass 3: the radial order
        out["n_key_ambiguous"] += int(key_ambiguous(r).sum())
        order = np.lexsort((idx, r.astype(f32)))
        cum = ordered_cumsum(m[order], start)
        rr = r[order]
        k = int(np.flatnonzero(cum >= M / 2.0)[0])
        out["r_half"][g], out["i_half"][g] = rr[k], idx[order[k]]
        rank = np.arange(1, c + 1)
        ok = (rank >= 10) & (rr > 0)
        if ok.any():
            v2 = np.where(ok, cum / np.where(ok, rr, 1.0), -1.0)
            k = int(np.argmax(v2))                             # (the first of equal maxima: the smallest rank)
            out["v2_max"][g], out["r_vmax"][g], out["i_vmax"][g] = v2[k], rr[k], idx[order[k]]
    return out


# ---- the references the tests share (computed once; do not modify what this returns) -----------------------------------------------
SCENES = {"clumps": clumps, "periodic": lambda: clumps(periodic=True), "crumbs": crumbs, "nonfinite": nonfinite_clumps,
          "edges": edges, "edges+1": lambda: edges(extra=1), "giants": giants, "legion": legion}
SAMPLED = {"giants": 24, "legion": 8}          # the scenes too large for the full matrix: random targets per halo
_REFERENCES = {}


def reference(name):
    """(scene, potential_model(scene), properties_model(scene, the model's phi, flagged with the float32 bound of that phi)).  For
    the scenes of SAMPLED the potential is the model at target_sample's members (pot["targets"]), and the properties are the
    model's without a potential (giants) or None (legion: potential only)."""
    if name not in _REFERENCES:
        scene = SCENES[name]()
        if name in SAMPLED:
            pot = potential_model(scene, targets=target_sample(scene, SAMPLED[name], seed=1))
            _REFERENCES[name] = (scene, pot, properties_model(scene, phi=None) if name == "giants" else None)
        else:
            pot = potential_model(scene)
            _REFERENCES[name] = (scene, pot, properties_model(scene, phi=pot["phi"], phi_bound=K * U * pot["scale"]))
    return _REFERENCES[name]
