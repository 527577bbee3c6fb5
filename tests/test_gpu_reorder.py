"""tsp_reorder_spatial and the cell grid it reports, against the NumPy model of their contract (tests/reorder_ref.py), at the
edges: non-finite coordinates, degenerate axes, duplicated positions, n below one cell / one chunk / one stratum, empty strata,
extents that leave float32 at either end, a second reorder, smoothing lengths that tie or are not positive, groups with an
empty shard.  Everything is an equality (bit patterns for floats) except where a tolerance is named.

One-line mutations of the library this module was run against on an MI355X (each built as a scratch copy, none committed;
every one gives wrong results, none indexes out of bounds), and the tests that failed.  Every test of the module fails under at
least one of them:
  the radix sort over 59 key bits instead of 60 ............... small_counts (all 13 scenes: n_strata = 4096)
  a NaN coordinate quantised to step 65535 instead of 0 ....... small_counts, culling [nan_axis, nonfinite]; 70000, second_reorder [nonfinite]
  a wide axis keyed in float32 (x - lo overflows) ............. small_counts, 70000, culling [overflow]
  min(row, rem) dropped from the transposition ................ small_counts (13), 70000 (3), second_reorder (4), render_does_not_depend (all 26)
  arrangement 2 sorted by ascending h ......................... small_counts (13), 70000 (3), second_reorder (4)
  the second call's permutation not composed with the first ... second_reorder (4)
  wm_valid left set by the reorder ............................ render_does_not_depend [all 13 scenes, weighted]
  key_prefix_offsets_kernel with <= for < ..................... small_counts (13), 70000 (3), second_reorder (4), culling (all 13)
  cells of >= 8 particles instead of >= 16 .................... small_counts (13), second_reorder (4)
  cell_width of 2^(15 - k) steps (half the true width) ........ small_counts (12), 70000 (3), second_reorder (4), culling (11: not point, denormal)
  uploads after the call not permuted ......................... small_counts (13), 70000 (3), second_reorder (4)
  band magnitudes read without the permutation ................ band_magnitudes_after_the_reorder
  the cell offsets kept by a fresh upload ..................... a_fresh_upload_drops_the_ordering
  n_strata = 4097 accepted .................................... refused_calls_change_nothing
  q left out of the attributes the reorder gathers ............ small_counts (13), 70000 (3), second_reorder (4), refused_calls,
                                                                render_does_not_depend [12 scenes, weighted: not nan_axis], group [100003]
  tsp_group_upload_quantity without the shard offset (q + 0) .. group [2, 100003]
  tsp_group_upload_rgb with g at offset 0 ..................... group [2, 100003]
The library before this module (extent and inv in float32 only, box_lo = NaN without a finite value, group uploads that
stop at an empty shard) fails small_counts [overflow, denormal, nan_axis, nonfinite], 70000 [overflow], second_reorder
[overflow], culling [overflow, denormal, nan_axis] and group [2], and nothing else.
"""
import numpy as np
import numpy.testing as npt
import pytest

import reorder_ref as ref

pytestmark = pytest.mark.gpu

f32 = np.float32
R = 64
COUNTS = (1, 2, 15, 16, 127, 128, 511, 512, 513, 1023, 4097)
STRATA = (1, 3, 8, 4096)
ATTRS = ("x", "y", "z", "h", "mass", "q", "r", "g", "b")


@pytest.fixture(scope="module")
def native():
    from topsy_amd import _native
    _native.load_library()
    return _native


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def rel_close(a, b, rtol):
    return (np.abs(a - b) <= rtol * np.maximum(np.abs(a), np.abs(b)) + 1e-30).all()


def smoothing(kind, n, seed):
    """distinct; all equal; a mix with 0, -1, NaN and inf"""
    rs = np.random.RandomState(seed)
    if kind == 0:
        return rs.permutation(n).astype(f32) * f32(0.001) + f32(0.25)
    if kind == 1:
        return np.full(n, 0.75, dtype=f32)
    h = rs.choice(np.array([0.5, 0.5, 2.0, 0.0, -1.0, np.nan, np.inf], dtype=f32), n)
    return h.astype(f32)


def attributes(pos, h, seed):
    """the nine resident arrays; q, r, g, b are arbitrary bit patterns (NaN payloads, denormals, -0) -- they are only moved"""
    rs = np.random.RandomState(seed)
    n = len(pos)
    raw = rs.randint(0, 2 ** 32, size=(5, n), dtype=np.uint64).astype(np.uint32)
    raw[:, ::5] |= 0x7fc00000                                        # a fifth are NaNs with payloads
    d = {"x": pos[:, 0].copy(), "y": pos[:, 1].copy(), "z": pos[:, 2].copy(), "h": h}
    for k, row in zip(("mass", "q", "r", "g", "b"), raw):
        d[k] = row.view(f32).copy()
    return d


def load(ctx, d):
    ctx.upload_particles(d["x"], d["y"], d["z"], d["h"], d["mass"])
    ctx.upload_quantity(d["q"])
    ctx.upload_rgb(d["r"], d["g"], d["b"])


def check_resident(ctx, d, perm):
    got = ctx.download_particles(ATTRS)
    for k in ATTRS:
        assert np.array_equal(bits(got[k]), bits(d[k])[perm]), k


def check_layout(ctx, m, n):
    assert np.array_equal(ctx.strata_offsets(), m["strata_offsets"])
    lay, want = ctx.cell_layout(), m["layout"]
    assert lay["n_strata"] == want["n_strata"] and lay["cells_per_axis"] == want["cells_per_axis"]
    assert np.array_equal(bits(lay["box_lo"]), bits(want["box_lo"])), (lay["box_lo"], want["box_lo"])
    assert np.array_equal(bits(lay["cell_width"]), bits(want["cell_width"])), (lay["cell_width"], want["cell_width"])
    off = lay["offsets"]
    assert np.array_equal(off, want["offsets"])
    assert off[0] == 0 and off[-1] == n and (np.diff(off) >= 0).all()
    return lay


def check_permutation(perm, m, h, interleave):
    n = len(perm)
    assert np.array_equal(np.sort(perm), np.arange(n))
    if interleave != 2:
        assert np.array_equal(perm, m["perm"])
        return
    # every segment holds the model's set, ordered by ascending 0xFFFFFFFF - bits(h): the key sequence is the model's
    sid = np.repeat(np.arange(len(m["segments"])), m["segments"][:, 1] - m["segments"][:, 0])
    assert np.array_equal(perm[np.lexsort((perm, sid))], m["perm"][np.lexsort((m["perm"], sid))])
    keys = ref.h_keys(h)[perm]
    assert np.array_equal(keys, m["segment_keys"])
    same = sid[1:] == sid[:-1]
    assert (keys[1:][same] >= keys[:-1][same]).all()


def reorder_and_check(ctx, pos, h, n_strata, seed, interleave, tag):
    n = len(pos)
    d = attributes(pos, h, seed)
    load(ctx, d)
    ctx.set_option("reorder_interleave", interleave)
    perm = ctx.reorder_spatial(n_strata, seed, want_permutation=True)
    m = ref.reorder(pos, h, n_strata, seed, interleave)
    check_permutation(perm, m, h, interleave)
    check_layout(ctx, m, n)
    check_resident(ctx, d, perm)
    # uploads after the call are given in the caller's order
    d2 = attributes(pos, h, seed + 1)
    ctx.upload_quantity(d2["q"])
    ctx.upload_rgb(d2["r"], d2["g"], d2["b"])
    got = ctx.download_particles(("q", "r", "g", "b"))
    for k in ("q", "r", "g", "b"):
        assert np.array_equal(bits(got[k]), bits(d2[k])[perm]), (tag, k)
    return perm, m, d


@pytest.mark.parametrize("scene", sorted(ref.SCENES))
def test_small_counts_equal_the_model(native, scene):
    """every count around one cell (16), one wave step, one chunk (512) and several chunks x every stratum count (4096 leaves
    strata empty), the three in-block arrangements and the three kinds of smoothing length taking turns"""
    ctx = native.Context(R, 4)
    turn = 0
    for n in COUNTS:
        pos = ref.SCENES[scene](n, 100 + n)
        for n_strata in STRATA:
            for interleave in ((0, 1, 2) if n in (16, 513, 4097) else (turn % 3,)):
                h = smoothing((turn // 3 + interleave) % 3, n, turn)
                reorder_and_check(ctx, pos, h, n_strata, 7 + turn, interleave, (scene, n, n_strata, interleave))
                turn += 1
    ctx.close()


@pytest.mark.parametrize("scene", ["uniform", "overflow", "nonfinite"])
def test_70000_particles_equal_the_model(native, scene):
    """the smallest count that reaches the 16^3 grid (k = 4 at one stratum: n >= 65536)"""
    n = 70000
    pos = ref.SCENES[scene](n, 5)
    ctx = native.Context(R, 4)
    for n_strata, interleave, kind in ((1, 0, 0), (1, 2, 2), (3, 1, 1), (8, 2, 0)):
        perm, m, _ = reorder_and_check(ctx, pos, smoothing(kind, n, 3), n_strata, 99, interleave, (scene, n_strata, interleave))
        assert m["layout"]["cells_per_axis"] == (16 if n_strata == 1 else 8)
    ctx.close()


def test_band_magnitudes_after_the_reorder(native):
    from oracle import oracle_np
    n = 4097
    rs = np.random.RandomState(4)
    pos = ref.scene_duplicates(n, 4)
    mags = rs.uniform(2.0, 14.0, size=(3, n))
    mags[0, ::211] = np.nan
    w = np.diag([0.5, 1.0, 1.0])
    want = oracle_np.band_contraction(mags, w)
    ctx = native.Context(R, 4)
    for interleave in (0, 1, 2):
        ctx.upload_particles(pos[:, 0], pos[:, 1], pos[:, 2], smoothing(0, n, 1), None)
        ctx.set_option("reorder_interleave", interleave)
        perm = ctx.reorder_spatial(3, 11, want_permutation=True)
        ctx.upload_band_magnitudes(mags, w)
        d = ctx.download_particles(("r", "g", "b"))
        got = np.stack([d["r"], d["g"], d["b"]], axis=1)
        npt.assert_allclose(got, want[perm], rtol=1.2e-7, atol=0)        # float64 pow: libm vs device, then one rounding
        assert (got[np.isnan(mags[0][perm]), 0] == 0.0).all()
    ctx.close()


@pytest.mark.parametrize("scene", ["uniform", "duplicates", "nonfinite", "overflow"])
def test_a_second_reorder_composes(native, scene):
    """a second call sorts the particles as they lie now (stable in THEIR order) and reports new -> ORIGINAL indices"""
    n = 4097
    pos = ref.SCENES[scene](n, 21)
    h = smoothing(0, n, 2)                    # distinct: arrangement 2 is one permutation too
    ctx = native.Context(R, 4)
    for interleave in (0, 1, 2):
        d = attributes(pos, h, 8)
        load(ctx, d)
        ctx.set_option("reorder_interleave", interleave)
        key = "perm_by_h" if interleave == 2 else "perm"
        perm1 = ctx.reorder_spatial(3, 5, want_permutation=True)
        assert np.array_equal(perm1, ref.reorder(pos, h, 3, 5, interleave)[key])
        perm2 = ctx.reorder_spatial(8, 77, want_permutation=True)
        m2 = ref.reorder(pos[perm1], h[perm1], 8, 77, interleave)
        assert np.array_equal(perm2, perm1[m2[key]])
        check_layout(ctx, m2, n)
        check_resident(ctx, d, perm2)
        q = attributes(pos, h, 9)["q"]
        ctx.upload_quantity(q)
        assert np.array_equal(bits(ctx.download_particles(("q",))["q"]), bits(q)[perm2])
    ctx.close()


def test_a_fresh_upload_drops_the_ordering(native):
    n = 513
    pos = ref.scene_uniform(n, 1)
    d = attributes(pos, smoothing(0, n, 1), 3)
    ctx = native.Context(R, 4)
    assert len(ctx.strata_offsets()) == 0 and ctx.cell_layout() is None
    load(ctx, d)
    ctx.reorder_spatial(3, 1)
    assert len(ctx.strata_offsets()) == 4 and ctx.cell_layout() is not None
    ctx.upload_particles(d["x"], d["y"], d["z"], d["h"], d["mass"])
    assert len(ctx.strata_offsets()) == 0 and ctx.cell_layout() is None
    ctx.upload_quantity(d["q"])
    got = ctx.download_particles(("x", "q"))
    assert np.array_equal(bits(got["q"]), bits(d["q"])) and np.array_equal(bits(got["x"]), bits(d["x"]))
    ctx.close()


def test_refused_calls_change_nothing(native):
    n = 1023
    pos = ref.scene_nonfinite(n, 6)
    d = attributes(pos, smoothing(2, n, 1), 3)
    ctx = native.Context(R, 4)
    with pytest.raises(native.BackendError, match="error -4:"):          # TSP_ESTATE: no particles
        ctx.reorder_spatial(3, 1)
    assert len(ctx.strata_offsets()) == 0 and ctx.cell_layout() is None
    load(ctx, d)
    for reordered in (False, True):
        if reordered:
            perm = ctx.reorder_spatial(8, 2, want_permutation=True)
        else:
            perm = np.arange(n)
        before = (ctx.strata_offsets(), ctx.cell_layout())
        for bad in (0, 4097, -1):
            with pytest.raises(native.BackendError, match="error -1:"):  # TSP_EINVAL
                ctx.reorder_spatial(bad, 1, want_permutation=True)
            check_resident(ctx, d, perm)
            assert np.array_equal(ctx.strata_offsets(), before[0])
            lay = ctx.cell_layout()
            assert (lay is None) == (before[1] is None)
            if lay is not None:
                assert lay["cells_per_axis"] == before[1]["cells_per_axis"] and np.array_equal(lay["offsets"], before[1]["offsets"])
                assert all(np.array_equal(bits(lay[k]), bits(before[1][k])) for k in ("box_lo", "cell_width"))
    ctx.close()


# ---- view culling on the device's own layout -----------------------------------------------------------------------------
def view(pos, scale_floor=1.0):
    """a camera on the bulk of a scene: centred on the median of the finite values, as wide as their 5-95 % spread (>= 1)"""
    from oracle import oracle_np
    p = pos.astype(np.float64)
    centre, spread = np.zeros(3), 0.0
    for a in range(3):
        v = p[np.isfinite(p[:, a]), a]
        if len(v):
            centre[a] = np.median(v)
            spread = max(spread, np.percentile(v, 95) - np.percentile(v, 5))
    scale = max(spread, scale_floor)
    return oracle_np.transform_matrix(np.eye(3), -centre, scale), scale


def look_at(centre, scale):
    from oracle import oracle_np
    return oracle_np.transform_matrix(np.eye(3), -np.asarray(centre, dtype=np.float64), scale)


@pytest.mark.parametrize("scene", sorted(ref.SCENES))
def test_culling_by_the_device_layout_loses_nothing(native, mips, scene):
    """the property of tests/test_reorder_ref_cpu.py on the layout the device reports and the positions it holds; for three
    spheres the render of the returned ranges is the render of exactly the particles inside those ranges"""
    from topsy_amd.cell_layout import StratifiedCells
    n = ref.SCENE_N[scene]
    pos = ref.SCENES[scene](n, 5)
    (_, _), scale = view(pos)
    h = (np.random.RandomState(1).uniform(0.03, 0.1, n) * scale).astype(f32)
    m = np.ones(n, dtype=f32)
    ctx = native.Context(R, 2)
    ctx.set_kernel_mips(mips)
    ctx.upload_particles(pos[:, 0], pos[:, 1], pos[:, 2], h, m)
    perm = ctx.reorder_spatial(1 if n == 70000 else 3, 99, want_permutation=True)
    lay = ctx.cell_layout()
    d = ctx.download_particles(("x", "y", "z", "h"))
    pos_new = np.stack([d["x"], d["y"], d["z"]], axis=1)
    assert np.array_equal(bits(pos_new), bits(pos[perm]))
    fault = ref.cell_run_fault(lay, pos_new)
    assert fault is None, fault
    cells = StratifiedCells([lay])
    p64 = pos_new.astype(np.float64)
    holding = culled = 0
    for centre, radius in ref.spheres(pos, 17):
        miss, ins, cov = ref.lost_particles(cells, p64, centre, radius)
        assert len(miss) == 0, (scene, centre, radius, miss[:5])
        holding += bool(ins.any())
        culled += not cells.all_selected()
    if scene == "nan_axis":                            # (no particle is finite on all axes: no sphere can hold one)
        assert holding == 0
    else:
        assert holding >= 100
    occupied = len(np.unique(ref.cell_codes(pos, lay["cells_per_axis"].bit_length() - 1)))
    if lay["cells_per_axis"] > 1 and occupied > 1:
        assert culled >= 1
    # three spheres of a tenth of the view's width on particles of the bulk: the render of the returned ranges is the render of
    # exactly the particles inside them (every footprint in the sphere is wider than 30 px at 1.2 x radius)
    other = native.Context(R, 2)
    other.set_kernel_mips(mips)
    for c in (ctx, other):
        c.set_option("count_fragments", 1)
    rendered = 0
    fin = np.flatnonzero(np.isfinite(p64).all(axis=1))
    for i in (fin[[len(fin) // 7, len(fin) // 2, -1 - len(fin) // 5]] if len(fin) else []):
        centre, radius = p64[i], 0.1 * scale
        miss, ins, cov = ref.lost_particles(cells, p64, centre, radius)
        assert len(miss) == 0 and ins[i]
        if cov.all():
            continue                                   # nothing culled: the render adds nothing to the index check
        st, ln = cells.ranges(0, n)
        M, sf = look_at(centre, 1.2 * radius)
        ctx.render(M, sf, st, ln)
        a, fa = ctx.read_image(), ctx.stats()["n_fragments"]
        other.upload_particles(d["x"][cov], d["y"][cov], d["z"][cov], d["h"][cov], m[cov])
        other.render(M, sf)
        b, fb = other.read_image(), other.stats()["n_fragments"]
        assert fa == fb and fa > 0 and np.array_equal(a[..., 0] != 0, b[..., 0] != 0)
        rendered += 1
    if occupied > 1 and scene != "nan_axis":           # (point, denormal: one occupied cell; nan_axis: no finite particle)
        assert rendered == 3, rendered
    ctx.close()
    other.close()


@pytest.mark.parametrize("mode_name", ["weighted", "rgb"])
@pytest.mark.parametrize("scene", sorted(ref.SCENES))
def test_render_does_not_depend_on_the_ordering(native, mips, scene, mode_name):
    """image and exact fragment count before and after the reorder, every in-block arrangement; images to 1e-5 relative (two
    orders of float64 accumulation rounded to float32 once: the bound of tests/test_gpu_scale.py)"""
    mode = native.MODE_RGB if mode_name == "rgb" else native.MODE_WEIGHTED
    n = 4097
    pos = ref.SCENES[scene](n, 31)
    (M, sf), scale = view(pos)
    rs = np.random.RandomState(2)
    h = (np.exp(rs.uniform(np.log(0.005), np.log(0.3), n)) * scale).astype(f32)
    h[::97] = np.array([0.0, -1.0, np.nan, np.inf], dtype=f32)[np.arange(len(h[::97])) % 4]
    mass = rs.uniform(0.5, 2.0, n).astype(f32)
    q = rs.uniform(0.5, 1.5, n).astype(f32)
    rgb = rs.uniform(0.0, 1.0, size=(3, n)).astype(f32)
    ctx = native.Context(R, 4)
    ctx.set_kernel_mips(mips)
    ctx.set_option("count_fragments", 1)
    channels = 3 if mode_name == "rgb" else 2

    def frame():
        ctx.render(M, sf, mode=mode)
        return ctx.read_image().astype(np.float64), ctx.stats()["n_fragments"]

    for interleave in (0, 1, 2):
        ctx.upload_particles(pos[:, 0], pos[:, 1], pos[:, 2], h, mass)
        ctx.upload_quantity(q)
        ctx.upload_rgb(*rgb)
        img0, f0 = frame()
        ctx.set_option("reorder_interleave", interleave)
        ctx.reorder_spatial(3, 5)
        img1, f1 = frame()
        assert f1 == f0
        for c in range(channels):
            assert rel_close(img1[..., c], img0[..., c], 1e-5), (interleave, c)
        if mode_name == "rgb":
            assert np.array_equal(img1[..., 3], img0[..., 3])
        if scene != "nan_axis":
            assert f0 > 0 and img0[..., 0].sum() > 0
    ctx.close()


# ---- groups ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 100_003])
def test_group_with_uploads_and_reorder_equals_one_context(native, mips, n):
    """three members on one device; with n = 2 the first shard is empty (bounds n g / G = 0, 0, 1, 2) and every group call
    must pass it by"""
    rs = np.random.RandomState(2)
    pos = (rs.normal(size=(n, 3)) * 30.0).astype(f32)
    h = np.exp(rs.uniform(np.log(3.0), np.log(30.0), n)).astype(f32)           # (>= 3.8 px: every footprint covers a pixel centre)
    m = rs.uniform(0.5, 2.0, n).astype(f32)
    q = rs.normal(size=n).astype(f32)
    rgb = rs.uniform(0.0, 1.0, size=(3, n)).astype(f32)
    from oracle import oracle_np
    M, sf = oracle_np.transform_matrix(np.eye(3), np.zeros(3), 100.0)
    one = native.Context(R, 4)
    one.set_kernel_mips(mips)
    one.upload_particles(pos[:, 0], pos[:, 1], pos[:, 2], h, m)
    one.upload_quantity(q)
    one.upload_rgb(*rgb)
    grp = native.Group(R, 4, [0, 0, 0])
    grp.set_kernel_mips(mips)
    grp.upload_particles(pos[:, 0], pos[:, 1], pos[:, 2], h, m)
    grp.upload_quantity(q)
    grp.upload_rgb(*rgb)
    grp.reorder_spatial(8, 3)
    assert grp.num_particles == n and [grp.member(g).num_particles for g in range(3)] == [n * (g + 1) // 3 - n * g // 3 for g in range(3)]
    one.render(M, sf)
    want = one.read_image().astype(np.float64)
    grp.render(M, sf)
    grp.end_frame()
    got = grp.root.read_image().astype(np.float64)
    assert want[..., 0].sum() > 0
    assert rel_close(got[..., 0], want[..., 0], 1e-5)
    assert np.abs(got[..., 1] - want[..., 1]).max() <= 1e-4 * np.abs(want[..., 1]).max()      # signed quantity: cancelling sums, other order
    assert grp.stats()["n_particles"] == n
    one.render(M, sf, mode=native.MODE_RGB)
    want = one.read_image().astype(np.float64)
    grp.render(M, sf, mode=native.MODE_RGB)
    grp.end_frame()
    got = grp.root.read_image().astype(np.float64)
    for c in range(3):
        assert rel_close(got[..., c], want[..., c], 1e-5)
    assert np.array_equal(got[..., 3], want[..., 3])
    grp.close()
    one.close()
