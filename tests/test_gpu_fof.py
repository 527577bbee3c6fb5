"""tsp_fof_groups on the GPU against fof_reference (test_fof_cpu.py), on that file's scenes.

Acceptance: group_out equals the reference's labels and info its counts.  The link test of the reference is the contract's own
float32 arithmetic, the partition of a graph is unique and the ranking is a total order, so there is no tolerance anywhere.
Then: the exact boundary on a lattice, a dense core (where the same-cell shortcut and the stop at a cell's first hit act),
invalid particles that must not bridge, small n, order independence, argument errors that change nothing, and the product path
(from_arrays(halos=..., center="halo-N"), centre_on_halo)."""
import ctypes

import numpy as np
import pytest

from test_fof_cpu import (CLUMPS, CLUMPS_LL, CLUMPS_N, DENSE_LL, INVALID_LL, LATTICE_CASES, clumps, clumps_reference,
                          clumps_shifted, dense_core, dense_core_reference, fof_reference, invalid_scene, lattice)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from topsy_amd import _native
    c = _native.Context(64, 2)
    yield c
    c.close()


def _call(ctx, pos, ll, period=0.0, min_members=20):
    return ctx.fof_groups(pos[:, 0], pos[:, 1], pos[:, 2], ll, period, min_members)


def _accept(label, got, want):
    (labels, info), (labels_ref, info_ref) = got, want
    differ = int((labels != labels_ref).sum())
    print(f"{label}: {info} / {info_ref}, labels that differ: {differ}")
    assert labels.dtype == np.int32 and labels.shape == labels_ref.shape
    assert info == info_ref, label
    assert differ == 0, label


@pytest.mark.parametrize("kind", ["open", "periodic", "shifted"])
def test_clumps(ctx, kind, monkeypatch):
    """shifted: raw coordinates outside [0, L); the partition is that of the wrapped positions."""
    pos = clumps_shifted() if kind == "shifted" else clumps()
    period = 0.0 if kind == "open" else 1.0
    got = _call(ctx, pos, CLUMPS_LL, period)
    _accept(kind, got, clumps_reference(kind))
    again = _call(ctx, pos, CLUMPS_LL, period)
    assert np.array_equal(got[0], again[0]) and got[1] == again[1]
    if kind == "shifted":
        assert np.array_equal(got[0], clumps_reference("periodic")[0])
    # no cell of these clumps is full enough for the library to use the same-cell shortcut by itself: force it
    monkeypatch.setenv("TOPSY_FOF_SHORTCUT", "1")
    _accept(kind + ", shortcut forced", _call(ctx, pos, CLUMPS_LL, period), clumps_reference(kind))


@pytest.mark.parametrize("ll,min_members", LATTICE_CASES)
def test_lattice_is_the_exact_boundary(ctx, ll, min_members):
    pos = lattice()
    got = _call(ctx, pos, ll, 0.0, min_members)
    _accept(f"lattice {ll!r} {min_members}", got, fof_reference(pos, ll, 0.0, min_members))
    if ll == 1.0:
        assert (got[0] == 1).all()
    elif min_members == 1:
        assert np.array_equal(got[0], np.arange(1, 2198))
    else:
        assert (got[0] == 0).all() and got[1]["n_groups"] == 0
    # the same lattice in a periodic box of side 13: the faces link at 1, and only there
    got = _call(ctx, pos, ll, 13.0, min_members)
    _accept(f"periodic lattice {ll!r} {min_members}", got, fof_reference(pos, ll, 13.0, min_members))


@pytest.mark.parametrize("shortcut", [None, "0", "1"])
def test_dense_core(ctx, shortcut, monkeypatch):
    """The library uses the same-cell shortcut by itself here (cells of thousands of particles); TOPSY_FOF_SHORTCUT=0 tests
    every pair instead, =1 is what None chooses.  The labels are the reference's each time."""
    if shortcut is not None:
        monkeypatch.setenv("TOPSY_FOF_SHORTCUT", shortcut)
    pos, balls = dense_core()
    got = _call(ctx, pos, DENSE_LL)
    _accept(f"dense core, shortcut {shortcut}", got, dense_core_reference())
    assert (got[0][balls[0]] == 1).all() and (got[0][balls[1]] == 1).all() and (got[0][balls[2]] == 2).all()


def test_invalid_particles_do_not_bridge(ctx):
    pos, a, b, odd = invalid_scene()
    got = _call(ctx, pos, INVALID_LL)
    _accept("invalid", got, fof_reference(pos, INVALID_LL, 0.0, 20))
    assert (got[0][a] == 1).all() and (got[0][b] == 2).all() and (got[0][odd] == -1).all()
    assert got[1]["n_valid"] == len(pos) - 5 and got[1]["n_groups"] == 2
    # nobody is valid
    nobody = np.full((7, 3), np.nan, dtype=np.float32)
    labels, info = _call(ctx, nobody, 0.1)
    assert (labels == -1).all() and info == {"n_valid": 0, "n_groups": 0, "n_grouped": 0, "largest": 0}


def test_small_n(ctx):
    one = np.float32([[0.5, 0.25, 0.125]])
    for min_members, want in ((1, 1), (2, 0), (20, 0)):
        labels, info = _call(ctx, one, 0.1, 0.0, min_members)
        assert labels.tolist() == [want] and info == {"n_valid": 1, "n_groups": want, "n_grouped": want, "largest": want}
    two = np.float32([[0.0, 0.0, 0.0], [0.0, 0.3, 0.4]])          # 0.5 apart, exactly
    for ll, period, min_members, want in ((0.5, 0.0, 2, [1, 1]), (0.5, 0.0, 1, [1, 1]), (0.5, 0.0, 3, [0, 0]),
                                          (0.49, 0.0, 1, [1, 2]), (0.49, 0.0, 2, [0, 0]), (0.5, 8.0, 2, [1, 1])):
        got = _call(ctx, two, ll, period, min_members)
        _accept(f"two {ll} {period} {min_members}", got, fof_reference(two, ll, period, min_members))
        assert got[0].tolist() == want
    # across the faces of a periodic box only
    far = np.float32([[0.05, 0.5, 0.5], [0.95, 0.5, 0.5], [0.5, 0.5, 0.5]])
    assert _call(ctx, far, 0.11, 1.0, 1)[0].tolist() == [1, 1, 2]
    assert _call(ctx, far, 0.11, 0.0, 1)[0].tolist() == [1, 2, 3]
    # duplicates and a linking length below the grid's resolution
    same = np.float32([[1.0, 2.0, 3.0]] * 5 + [[1.0, 2.0, 3.5]])
    assert _call(ctx, same, 1e-12, 0.0, 1)[0].tolist() == [1, 1, 1, 1, 1, 2]
    # every particle on a line (two axes of zero extent)
    line = np.zeros((300, 3), dtype=np.float32)
    line[:, 1] = np.arange(300) * 0.01
    line[150:, 1] += 0.5
    got = _call(ctx, line, 0.0125, 0.0, 1)
    _accept("line", got, fof_reference(line, 0.0125, 0.0, 1))
    assert got[1]["n_groups"] == 2


def _canonical(labels):
    """Every particle's group as the smallest member index (labels >= 1 everywhere)."""
    first = np.full(int(labels.max()) + 1, len(labels), dtype=np.int64)
    np.minimum.at(first, labels, np.arange(len(labels)))
    return first[labels]


def test_order_independence(ctx):
    pos = clumps()
    labels, info = _call(ctx, pos, CLUMPS_LL, 1.0, 1)              # min_members = 1: the whole partition is visible
    assert labels.min() == 1 and info["n_grouped"] == CLUMPS_N
    perm = np.random.RandomState(9).permutation(CLUMPS_N)
    labels_p, info_p = _call(ctx, pos[perm], CLUMPS_LL, 1.0, 1)
    assert info_p == info
    back = np.empty_like(labels_p)
    back[perm] = labels_p                                          # the permuted run's label of every original particle
    # the same sets of members
    a, b = _canonical(labels), _canonical(back)
    assert np.array_equal(a, b)
    # the same sizes by rank, and the same rank wherever the size is not shared
    sizes, sizes_p = np.bincount(labels)[1:], np.bincount(back)[1:]
    assert np.array_equal(sizes, sizes_p)
    unshared = np.flatnonzero(np.bincount(sizes)[sizes] == 1) + 1
    assert len(unshared) >= 5
    sel = np.isin(labels, unshared)
    assert np.array_equal(labels[sel], back[sel])


def test_argument_errors_change_nothing(ctx):
    from topsy_amd import _native
    lib = _native.load_library()
    fp = ctypes.POINTER(ctypes.c_float)
    pos = clumps()[:1000]
    n = len(pos)
    x, y, z = (np.ascontiguousarray(pos[:, a]) for a in range(3))
    out = np.full(n, -77, dtype=np.int32)
    info = _native.FofInfo(-1, -2, -3, -4)
    P = lambda v: v.ctypes.data_as(fp)                                              # noqa: E731
    O = out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    good = [n, P(x), P(y), P(z), 0.05, 0.0, 20, O, ctypes.byref(info)]

    def untouched():
        return (out == -77).all() and (info.n_valid, info.n_groups, info.n_grouped, info.largest) == (-1, -2, -3, -4)

    def but(*changes):
        args = list(good)
        for i, v in changes:
            args[i] = v
        return tuple(args)
    nan, inf = float("nan"), float("inf")
    cases = [but((0, 0)), but((0, -5)), but((0, 1 << 31)), but((1, None)), but((2, None)), but((3, None)), but((7, None)),
             but((4, nan)), but((4, 0.0)), but((4, -0.05)), but((4, inf)), but((5, -1.0)), but((5, nan)), but((5, inf)),
             but((4, 0.5), (5, 1.0)), but((4, 0.7), (5, 1.0)), but((6, 0)), but((6, -3))]
    for args in cases:
        assert lib.tsp_fof_groups(ctx._h, *args) == -1, args          # TSP_EINVAL
        assert untouched(), args
        assert lib.tsp_last_error()
    assert lib.tsp_fof_groups(None, *good) == -1 and untouched()
    # the good call, with and without the optional info
    want = fof_reference(pos, np.float32(0.05), 0.0, 20)
    assert lib.tsp_fof_groups(ctx._h, *good) == 0
    assert np.array_equal(out, want[0]) and info.n_valid == n and info.n_groups == want[1]["n_groups"]
    out[:] = -77
    assert lib.tsp_fof_groups(ctx._h, *but((8, None))) == 0 and np.array_equal(out, want[0])
    assert lib.tsp_fof_groups(ctx._h, *but((4, 0.499), (5, 1.0))) == 0


def test_neighbours_unchanged():
    """A FoF call on a context that holds a rendered image leaves the image, the counts and the particles as they were."""
    from oracle import oracle_np
    from topsy_amd import _native, kernel_lut
    ctx = _native.Context(160, 2)
    try:
        ctx.set_kernel_mips(kernel_lut.kernel_mips())
        g = np.arange(-70.0, 71.0, 20.0, dtype=np.float32)
        gx, gy = (v.ravel() for v in np.meshgrid(g, g))
        ctx.upload_particles(gx, gy, np.zeros(64, dtype=np.float32), np.full(64, 3.0, dtype=np.float32), np.ones(64, dtype=np.float32))
        M, sf = oracle_np.transform_matrix(np.eye(3), np.zeros(3), 90.0)
        ctx.render(M, sf)
        counts = lambda: {k: v for k, v in ctx.stats().items() if not k.startswith("ms_")}      # noqa: E731
        img0, stats0, parts0 = ctx.read_image(), counts(), ctx.download_particles()
        assert np.count_nonzero(img0[..., 0]) > 64 * 20
        pos, a, b, odd = invalid_scene()
        labels, info = _call(ctx, pos, INVALID_LL)
        assert info["n_groups"] == 2
        img1, stats1, parts1 = ctx.read_image(), counts(), ctx.download_particles()
        assert np.array_equal(img0.view(np.uint32), img1.view(np.uint32)) and stats0 == stats1
        for k in parts0:
            assert np.array_equal(parts0[k], parts1[k]), k
    finally:
        ctx.close()


# ---- the public interface and the product path ------------------------------------------------------------------------------
def _nearest_image(d, period):
    return d - period * np.rint(d / period)


def test_friends_of_friends_catalogue():
    import topsy_amd
    pos = clumps()
    cat = topsy_amd.friends_of_friends(pos, periodicity_scale=1.0)
    want = clumps_reference("periodic")
    # the default linking length: 0.2 * (1 / n) ** (1/3), the scene's own
    assert cat.linking_length == float(np.float32(CLUMPS_LL))
    assert np.array_equal(cat.group, want[0]) and cat.info == want[1]
    assert len(cat) == 5 and cat.sizes.tolist() == [56193, 29207, 18441, 7824, 1493] and cat.sizes.dtype == np.int64
    assert np.array_equal(cat.members(3), np.flatnonzero(want[0] == 3))
    with pytest.raises(ValueError, match="5 halo"):
        cat.members(6)
    cat = topsy_amd.friends_of_friends(pos, linking_length=CLUMPS_LL)
    assert np.array_equal(cat.group, clumps_reference("open")[0]) and len(cat) == 9


@pytest.mark.parametrize("variant", ["fof", "fof_two_contexts", "labels", "labels_with_cells"])
def test_from_arrays_opens_on_a_halo(variant, monkeypatch):
    """The bound 0.005 is the one test_gpu_center.py uses for a clump: a quarter to two thirds of the clumps' sigma."""
    import topsy_amd
    from topsy_amd import _native
    pos = clumps()
    mass = np.ones(CLUMPS_N, dtype=np.float32)
    calls = []
    real = _native.Context.fof_groups
    monkeypatch.setattr(_native.Context, "fof_groups", lambda self, *a, **k: calls.append(1) or real(self, *a, **k))
    kw = dict(render_resolution=64)
    if variant == "fof_two_contexts":
        kw["device_ids"] = [0, 0]
    if variant.startswith("labels"):
        halos = np.array(clumps_reference("periodic")[0])
        kw["with_cells"] = variant == "labels_with_cells"
    else:
        halos = "fof"
    h = np.full(CLUMPS_N, 0.01, dtype=np.float32)
    vis = topsy_amd.from_arrays(pos, h, mass, center="halo-3", halos=halos, periodicity_scale=1.0, **kw)
    try:
        ld = vis.data_loader
        centre = ld.get_initial_center()
        assert centre.dtype == np.float64 and centre is ld.get_initial_center()
        assert len(calls) == (0 if variant.startswith("labels") else 1)
        # halo 3 of the periodic catalogue is the clump across the box faces: whole only by nearest image
        assert len(ld.get_halos()) == 5 and ld.get_halos().sizes[2] == 18441
        assert np.linalg.norm(_nearest_image(centre - np.asarray(CLUMPS[2][0]), 1.0)) < 0.005
        assert np.array_equal(vis.position_offset, -centre)
        # jump to halo 1 and back
        offset = vis.centre_on_halo(1)
        assert np.array_equal(offset, vis.position_offset) and np.linalg.norm(-offset - np.asarray(CLUMPS[0][0])) < 0.005
        assert np.array_equal(vis.centre_on_halo(3), -centre)
        with pytest.raises(ValueError, match="5 halo"):
            vis.centre_on_halo(6)
        assert len(calls) == (0 if variant.startswith("labels") else 1)
        if variant == "fof":
            assert np.array_equal(ld.get_halos().group, clumps_reference("periodic")[0])
            from types import SimpleNamespace
            from topsy_amd import surface
            assert np.array_equal(surface.SurfaceView.centre_on_halo(SimpleNamespace(_vis=vis), 2), vis.position_offset)
            assert np.linalg.norm(-vis.position_offset - np.asarray(CLUMPS[1][0])) < 0.005
    finally:
        vis.close()


def test_from_arrays_open_box_and_a_missing_halo():
    """smooth=None: the smoothing lengths, the catalogue and the centre come from the visualizer's context.  The open box: the
    default linking length is b times the mean separation in the bounding box of the positions."""
    import topsy_amd
    from topsy_amd import loader
    pos = clumps()
    mass = np.ones(CLUMPS_N, dtype=np.float32)
    vis = topsy_amd.from_arrays(pos, None, mass, center="halo-2", halos="fof", render_resolution=64)
    try:
        centre = vis.data_loader.get_initial_center()
        cat = vis.data_loader.get_halos()
        print("open box, halos='fof':", cat.linking_length, cat.info, cat.sizes[:9])
        assert np.linalg.norm(centre - np.asarray(CLUMPS[1][0])) < 0.005
        assert abs(cat.linking_length - loader.fof_linking_length(pos, 0.2, 0.0)) <= 1e-7 * cat.linking_length
    finally:
        vis.close()
    # a loader without a visualizer makes a context of its own; the keywords reach the search
    ld = loader.ArrayDataLoader(pos=pos, smooth=None, mass=mass, halos={"linking_length": CLUMPS_LL, "min_members": 20})
    assert np.array_equal(ld.get_halos().group, clumps_reference("open")[0]) and len(ld.get_halos()) == 9
    with pytest.raises(ValueError, match="5 halo"):
        topsy_amd.from_arrays(pos, np.full(CLUMPS_N, 0.01, dtype=np.float32), mass, center="halo-6", halos="fof",
                              periodicity_scale=1.0, render_resolution=64)
