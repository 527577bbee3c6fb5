"""Phase diagrams on the GPU (tsp_histogram_2d, Context.histogram_2d, topsy_amd.phase_diagram, Visualizer.phase_diagram) against
the float64 model of phase_ref.py.

Tolerances come from the contract, not from a run: counts, bin_out, n_valid and n_binned equal the model's; w and w v are exact
in float64 and (w v) v rounds once, and a cell's m terms are added in an order of the library's choosing, so every sum lies
within m * 2^-52 * sum |term| of the model's: any order of summation passes, one misbinned particle does not.  Empty cells are
+0.0 bit for bit."""
import ctypes

import numpy as np
import pytest

import phase_ref as ref

pytestmark = pytest.mark.gpu
f32 = np.float32
EINVAL, ENOMEM = -1, -6


@pytest.fixture(scope="module")
def native():
    from topsy_amd import _native
    _native.load_library()
    return _native


@pytest.fixture(scope="module")
def ctx(native):
    """a context in its first state: no mips, no particles, nothing rendered"""
    c = native.Context(16, 2)
    yield c
    c.close()


def log_edges(lo, hi, n):
    from topsy_amd import phase
    return phase.hist_edges(lo, hi, n, log=True)


_models = {}


def model(x, y, w, v, ex, ey):
    """the float64 model, computed once per input and left unchanged"""
    key = tuple(None if a is None else (a.shape, a.dtype.str, a.tobytes()) for a in (x, y, w, v, ex, ey))
    if key not in _models:
        m = ref.histogram(x, y, w, v, ex, ey)
        for a in m.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _models[key] = m
    return _models[key]


def check(got, m, label, exact=False):
    assert got["count"].dtype == np.int64 and got["count"].shape == m["count"].shape, label
    assert got["sums"].dtype == np.float64 and got["sums"].shape == m["sums"].shape, label
    assert np.array_equal(got["count"], m["count"]), label
    assert (got["n_valid"], got["n_binned"]) == (m["n_valid"], m["n_binned"]), label
    if "bin_index" in got:
        assert got["bin_index"].dtype == np.int32 and np.array_equal(got["bin_index"], m["bin_index"]), label
    empty = np.broadcast_to(m["count"] == 0, got["sums"].shape)
    assert not got["sums"].view(np.uint64)[empty].any(), f"{label}: an empty cell is not +0.0"
    err, bound = np.abs(got["sums"] - m["sums"]), ref.tolerance(m)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)))
    print(f"{label}: worst |got - want| / bound = {worst:.3g}; cells occupied: {np.count_nonzero(m['count'])} of {m['count'].size}")
    assert (err <= bound).all(), (label, worst)
    if exact:
        assert np.array_equal(got["sums"].view(np.uint64), m["sums"].view(np.uint64)), f"{label}: not bit for bit"


def run(ctx, x, y, w, v, ex, ey, want_bins=True):
    return ctx.histogram_2d(x, y, w, v, edges_x=ex, edges_y=ey, want_bins=want_bins)


def same_bytes(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
        else:
            assert a[k] == b[k], k


# ---- 1. against the model ------------------------------------------------------------------------------------------------------
N1 = 20000


@pytest.fixture(scope="module")
def ridge():
    """correlated lognormals over 64 x 48 logarithmic bins that leave some particles outside on every side"""
    rs = np.random.RandomState(17)
    x = np.exp(rs.normal(0.0, 1.6, N1)).astype(f32)
    y = (1e4 * x.astype(np.float64) ** 0.6 * np.exp(rs.normal(0.0, 0.5, N1))).astype(f32)
    w = rs.normal(0.5, 1.0, N1).astype(f32)
    v = rs.normal(10.0, 200.0, N1).astype(f32)
    arrays = (x, y, w, v, log_edges(0.02, 30.0, 64), log_edges(1e3, 1e5, 48))
    for a in arrays:
        a.setflags(write=False)
    return arrays


@pytest.mark.parametrize("with_w", [False, True], ids=["no_w", "w"])
@pytest.mark.parametrize("with_v", [False, True], ids=["no_v", "v"])
def test_matches_the_model(ctx, ridge, with_w, with_v):
    x, y, w, v, ex, ey = ridge
    w, v = (w if with_w else None), (v if with_v else None)
    m = model(x, y, w, v, ex, ey)
    assert 0 < m["n_binned"] < m["n_valid"] == N1 and (m["sums"][0] < 0).any() == with_w and m["count"].max() > 30
    got = run(ctx, x, y, w, v, ex, ey)
    check(got, m, f"ridge w={with_w} v={with_v}")
    plain = run(ctx, x, y, w, v, ex, ey, want_bins=False)
    assert "bin_index" not in plain
    del got["bin_index"]
    same_bytes(plain, got)
    # a transposed table would not pass: the table is not symmetric
    assert m["count"].shape == (48, 64) and not np.array_equal(m["count"][:, :48], m["count"][:, :48].T)


# ---- 2. exactness --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shuffled", [False, True])
def test_integer_terms_are_exact_in_any_order(ctx, ridge, shuffled):
    x, y, _, _, ex, ey = ridge
    rs = np.random.RandomState(3)
    w, v = rs.randint(1, 8, N1).astype(f32), rs.randint(-9, 10, N1).astype(f32)
    if shuffled:
        p = rs.permutation(N1)
        x, y, w, v = x[p], y[p], w[p], v[p]
    check(run(ctx, x, y, w, v, ex, ey), model(x, y, w, v, ex, ey), f"integers, shuffled={shuffled}", exact=True)


# ---- 3. edges ------------------------------------------------------------------------------------------------------------------
def around(values):
    """every value, and one float32 ulp below and above it"""
    values = np.asarray(values, dtype=f32)
    return np.concatenate([np.nextafter(values, f32(-np.inf)), values, np.nextafter(values, f32(np.inf))])


def test_values_on_the_edges(ctx):
    ex = np.array([0.5, 1.0, 1.5, 3.0, 1024.0])            # float32-representable
    ey = np.array([-2.0, -0.25, 0.0, 7.0])
    ax, ay = around(ex), around(ey)
    x = np.concatenate([ax, np.full(len(ay), 1.25, dtype=f32)])
    y = np.concatenate([np.full(len(ax), 1.0, dtype=f32), ay])
    w = np.arange(1, len(x) + 1, dtype=f32)
    m = model(x, y, w, None, ex, ey)
    got = run(ctx, x, y, w, None, ex, ey)
    check(got, m, "edges", exact=True)
    b = got["bin_index"]
    nx, row = 4, 2                                           # y = 1.0 is in row 2, x = 1.25 in column 1
    k = len(ex)
    assert b[:k].tolist() == [-1, row * nx + 0, row * nx + 1, row * nx + 2, row * nx + 3]          # one ulp below every edge
    assert b[k:2 * k].tolist() == [row * nx + 0, row * nx + 1, row * nx + 2, row * nx + 3, -1]      # on it: the upper cell; last: outside
    assert b[2 * k:3 * k].tolist() == [row * nx + 0, row * nx + 1, row * nx + 2, row * nx + 3, -1]
    k0, ky = 3 * k, len(ey)
    assert b[k0:k0 + ky].tolist() == [-1, 0 * nx + 1, 1 * nx + 1, 2 * nx + 1]
    assert b[k0 + ky:k0 + 2 * ky].tolist() == [0 * nx + 1, 1 * nx + 1, 2 * nx + 1, -1]
    assert b[k0 + 2 * ky:].tolist() == [0 * nx + 1, 1 * nx + 1, 2 * nx + 1, -1]


# ---- 4. concentration and spread -----------------------------------------------------------------------------------------------
def test_everything_in_one_cell_of_a_large_table(ctx):
    n = 200_000
    rs = np.random.RandomState(8)
    ex, ey = log_edges(1e-3, 1e3, 1024), log_edges(1e2, 1e8, 1024)
    i, j = 700, 333
    x = rs.uniform(ex[i] * 1.0001, ex[i + 1] * 0.9999, n).astype(f32)
    y = rs.uniform(ey[j] * 1.0001, ey[j + 1] * 0.9999, n).astype(f32)
    w, v = rs.uniform(0.5, 2.0, n).astype(f32), rs.normal(0.0, 50.0, n).astype(f32)
    m = model(x, y, w, v, ex, ey)
    assert m["count"][j, i] == n
    got = run(ctx, x, y, w, v, ex, ey)
    check(got, m, "one cell of 1024 x 1024")
    assert np.count_nonzero(got["count"]) == 1 and np.count_nonzero(got["sums"]) == 3


def test_every_particle_in_a_cell_of_its_own(ctx):
    rs = np.random.RandomState(9)
    ex, ey = np.arange(65.0), np.arange(65.0) * 2.0
    cells = rs.permutation(4096)
    x, y = ((cells % 64) + 0.5).astype(f32), ((cells // 64) * 2.0 + 1.0).astype(f32)
    w, v = rs.normal(0.0, 3.0, 4096).astype(f32), rs.normal(0.0, 3.0, 4096).astype(f32)
    m = model(x, y, w, v, ex, ey)
    assert (m["count"] == 1).all() and np.array_equal(m["bin_index"], cells)
    check(run(ctx, x, y, w, v, ex, ey), m, "4096 particles, 4096 cells", exact=True)      # (one term per cell: no rounding)


def test_ten_members_after_a_call_that_filled_the_table(ctx):
    """the table lives in per-call scratch: what an earlier call left there must not show"""
    ex, ey = np.arange(1025.0), np.arange(1025.0)
    cells = np.arange(1024 * 1024)
    xf, yf = ((cells % 1024) + 0.5).astype(f32), ((cells // 1024) + 0.5).astype(f32)
    wf = np.full(len(cells), 3.0, dtype=f32)
    full = run(ctx, xf, yf, wf, wf, ex, ey, want_bins=False)
    assert (full["count"] == 1).all() and (full["sums"][0] == 3.0).all() and (full["sums"][2] == 27.0).all()
    rs = np.random.RandomState(4)
    x, y = rs.uniform(0.0, 1024.0, 10).astype(f32), rs.uniform(0.0, 1024.0, 10).astype(f32)
    w, v = rs.uniform(1.0, 2.0, 10).astype(f32), rs.uniform(1.0, 2.0, 10).astype(f32)
    m = model(x, y, w, v, ex, ey)
    got = run(ctx, x, y, w, v, ex, ey)
    check(got, m, "ten members of 1024 x 1024")
    assert got["count"].sum() == 10 and np.count_nonzero(got["sums"]) == 3 * np.count_nonzero(m["count"])


# ---- 5. shapes and sizes -------------------------------------------------------------------------------------------------------
def sizes(native):
    block = native.HIST2D_BLOCK
    assert block == native.histogram_2d_layout(1, 1, 1)["block"]
    return [1, 63, 64, 65, 1023, 1024, 1025, block - 1, block, block + 1, 2 * block + 1]


@pytest.mark.parametrize("nx,ny", [(1, 1), (1, 1024), (1024, 1), (3, 5)])
def test_shapes_and_sizes(native, ctx, nx, ny):
    rs = np.random.RandomState(nx + ny)
    ex, ey = np.linspace(-1.0, 1.0, nx + 1), np.linspace(0.0, 4.0, ny + 1)
    for n in sizes(native):
        x, y = rs.uniform(-1.1, 1.1, n).astype(f32), rs.uniform(-0.2, 4.2, n).astype(f32)
        w, v = rs.normal(0.0, 1.0, n).astype(f32), rs.normal(0.0, 1.0, n).astype(f32)
        got = run(ctx, x, y, w, v, ex, ey)
        assert got["count"].shape == (ny, nx)
        check(got, model(x, y, w, v, ex, ey), f"{nx} x {ny}, n = {n}")


def cells_scene(members, nx=8):
    """particles in the cells of one row: members[c] of them in column c, in column order, every term an integer"""
    cells = np.repeat(np.arange(len(members)), members)
    n = len(cells)
    rs = np.random.RandomState(n)
    return (cells + 0.5).astype(f32), np.full(n, 0.5, dtype=f32), rs.randint(1, 8, n).astype(f32), rs.randint(-9, 10, n).astype(f32), \
        np.arange(nx + 1.0), np.array([0.0, 1.0])


def test_runs_at_the_boundaries_of_the_reductions_blocks(native, ctx):
    B = native.HIST2D_BLOCK
    scenes = {"one cell over more than three blocks": [0, 0, 0, 3 * B + 10],
              "one cell over three blocks exactly, neighbours on either side": [5, 3 * B - 5, 0, 3 * B, 7],
              "a cell boundary on a block boundary": [B, B, 2 * B, 11],
              "cell boundaries on wave boundaries": [64, 64, 128, 1, 63, 64],
              "a run that ends one short of a block, one that starts one past it": [B - 1, 2, B - 1, B + 1, B - 1],
              "two levels above the first": [0, 130 * B + 3, 1, 130 * B, 2]}
    for label, members in scenes.items():
        x, y, w, v, ex, ey = cells_scene(members)
        for order in ("sorted", "shuffled"):
            if order == "shuffled":
                p = np.random.RandomState(1).permutation(len(x))
                x, y, w, v = x[p], y[p], w[p], v[p]
            m = model(x, y, w, v, ex, ey)
            assert m["count"][0, :len(members)].tolist() == members
            check(run(ctx, x, y, w, v, ex, ey), m, f"{label} ({order})", exact=True)
    assert native.histogram_2d_layout(3 * B + 10, 8, 1)["blocks"] == 4 and native.histogram_2d_layout(260 * B + 6, 8, 1)["levels"] == 3


# ---- 6. non-finite input -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["x", "y", "w", "v"])
def test_non_finite_particles_are_invalid(ctx, ridge, which):
    arrays = {k: a.copy() for k, a in zip("xywv", ridge[:4])}
    ex, ey = ridge[4:]
    clean = model(*ridge)
    bad = arrays[which]
    bad[10::97], bad[11::97], bad[12::97] = np.nan, np.inf, -np.inf
    hit = ~np.isfinite(bad)
    m = model(arrays["x"], arrays["y"], arrays["w"], arrays["v"], ex, ey)
    assert m["n_valid"] == N1 - hit.sum() and (m["bin_index"][hit] == -1).all()
    assert np.array_equal(m["bin_index"][~hit], clean["bin_index"][~hit])          # everything else is unchanged
    got = run(ctx, arrays["x"], arrays["y"], arrays["w"], arrays["v"], ex, ey)
    check(got, m, f"non-finite {which}")
    assert (got["bin_index"][hit] == -1).all() and np.isfinite(got["sums"]).all()


def test_nothing_in_range_is_zeros_not_an_error(ctx):
    ex, ey = log_edges(1.0, 100.0, 7), log_edges(1.0, 100.0, 5)
    x = np.array([0.0, -0.0, -5.0, 0.5, 100.0, 1e30, np.nan, 50.0, 50.0], dtype=f32)
    y = np.array([5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 0.0, -50.0], dtype=f32)
    m = model(x, y, None, None, ex, ey)
    assert m["n_valid"] == 8 and m["n_binned"] == 0
    got = run(ctx, x, y, None, None, ex, ey)
    check(got, m, "no member")
    assert not got["count"].any() and not got["sums"].view(np.uint64).any() and (got["bin_index"] == -1).all()
    nan = np.full(300, np.nan, dtype=f32)
    got = run(ctx, nan, nan, nan, nan, ex, ey)
    assert got["n_valid"] == 0 and not got["count"].any() and not got["sums"].view(np.uint64).any()


# ---- 7. determinism ------------------------------------------------------------------------------------------------------------
def test_the_same_call_gives_the_same_bytes(native, ctx, ridge):
    first = run(ctx, *ridge)
    same_bytes(first, run(ctx, *ridge))
    fresh = native.Context(64, 4)
    try:
        same_bytes(first, run(fresh, *ridge))
    finally:
        fresh.close()


# ---- a context that holds a scene ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_ctx(native, mips):
    """resident particles and a rendered frame: the call must leave all of it alone"""
    from oracle import oracle_np
    c = native.Context(96, 2)
    c.set_kernel_mips(mips)
    rs = np.random.RandomState(6)
    pos = rs.normal(0.0, 25.0, (300, 3)).astype(f32)
    c.upload_particles(pos[:, 0], pos[:, 1], pos[:, 2], np.full(300, 4.0, dtype=f32), np.ones(300, dtype=f32))
    M, sf = oracle_np.transform_matrix(np.eye(3), np.zeros(3), 90.0)
    c.render(M, sf)
    assert np.count_nonzero(c.read_image()[..., 0]) > 1000
    yield c
    c.close()


def raw_call(native, ctx, x, y, w, v, ex, ey, count, sums, bins=None, info=None, n=None, nx=None, ny=None, null=()):
    lib = native.load_library()
    fp, dp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)
    ptr = lambda name, a, kind: None if a is None or name in null else a.ctypes.data_as(kind)
    spec = native.Hist2dSpec(len(ex) - 1 if nx is None else nx, len(ey) - 1 if ny is None else ny, ptr("edges_x", ex, dp),
                             ptr("edges_y", ey, dp))
    return lib.tsp_histogram_2d(ctx._h, len(x) if n is None else n, ptr("x", x, fp), ptr("y", y, fp), ptr("w", w, fp), ptr("v", v, fp),
                                None if "spec" in null else ctypes.byref(spec), ptr("count", count, ctypes.POINTER(ctypes.c_int64)),
                                ptr("sums", sums, dp), ptr("bins", bins, ctypes.POINTER(ctypes.c_int32)),
                                None if info is None else ctypes.byref(info))


# ---- 8. refused calls ----------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing_and_leave_the_context_alone(native, scene_ctx):
    from test_gpu_scratch_alloc_failure import Outputs, assert_same_state, snapshot
    rs = np.random.RandomState(2)
    x, y, w, v = (rs.uniform(0.0, 4.0, 500).astype(f32) for _ in range(4))
    ex, ey = np.linspace(0.0, 4.0, 1025), np.linspace(0.0, 4.0, 1025)      # long enough for every nx, ny tried below
    ex4, ey3 = np.linspace(0.0, 4.0, 5), np.linspace(0.0, 4.0, 4)
    outs = Outputs(count=np.empty((3, 4), dtype=np.int64), sums=np.empty((3, 3, 4)), bins=np.empty(500, dtype=np.int32),
                   info=native.Hist2dInfo())

    def edges_with(k, value, base=ex4):
        e = base.copy()
        e[k] = value
        return e

    refused = [dict(n=0), dict(n=-1), dict(n=2 ** 31), dict(null=("x",)), dict(null=("y",)), dict(null=("spec",)),
               dict(null=("edges_x",)), dict(null=("edges_y",)), dict(null=("count",)), dict(null=("sums",)),
               dict(ex=ex, nx=0), dict(ex=ex, nx=1025), dict(ex=ex, nx=-1), dict(ey=ey, ny=0), dict(ey=ey, ny=1025)]
    for value in (np.nan, np.inf, -np.inf):
        refused += [dict(ex=edges_with(k, value)) for k in (0, 2, 4)] + [dict(ey=edges_with(k, value, ey3)) for k in (0, 3)]
    refused += [dict(ex=edges_with(2, 1.0)), dict(ex=edges_with(2, 0.5)), dict(ex=ex4[::-1].copy()), dict(ey=edges_with(3, ey3[2], ey3)),
                dict(ey=edges_with(1, -1.0, ey3))]
    before = snapshot(scene_ctx)
    for kw in refused:
        outs.fill()
        args = dict(ex=ex4, ey=ey3)
        args.update(kw)
        assert raw_call(native, scene_ctx, x, y, w, v, args.pop("ex"), args.pop("ey"), outs.count, outs.sums, outs.bins, outs.info,
                        **args) == EINVAL, kw
        assert not outs.written(), (kw, outs.written())
    assert_same_state(before, snapshot(scene_ctx), "after the refused calls")
    outs.fill()
    assert raw_call(native, scene_ctx, x, y, w, v, ex4, ey3, outs.count, outs.sums, outs.bins, outs.info) == 0
    got = {"count": outs.count, "sums": outs.sums, "bin_index": outs.bins, "n_valid": outs.info.n_valid, "n_binned": outs.info.n_binned}
    check(got, model(x, y, w, v, ex4, ey3), "the call after the refusals")
    assert_same_state(before, snapshot(scene_ctx), "after the accepted call")
    # info_out and bin_out are optional
    outs.fill()
    assert raw_call(native, scene_ctx, x, y, w, v, ex4, ey3, outs.count, outs.sums) == 0
    assert np.array_equal(outs.count, got["count"]) and outs.written() == ["count", "sums"]


# ---- 9. failed allocations -----------------------------------------------------------------------------------------------------
def test_failed_scratch_allocations(native, scene_ctx, ridge):
    from test_gpu_scratch_alloc_failure import SCRATCH_SITES, Outputs, walk
    x, y, w, v, ex, ey = ridge
    sites = SCRATCH_SITES["sph_sum"] - set(s for s in SCRATCH_SITES["sph_sum"] if s.startswith("index_"))
    assert sites == {"sph_sum_h", "sph_sum_a"}
    outs = Outputs(count=np.empty((48, 64), dtype=np.int64), sums=np.empty((3, 48, 64)), bins=np.empty(N1, dtype=np.int32),
                   info=native.Hist2dInfo())
    reached = walk(native, scene_ctx, lambda: raw_call(native, scene_ctx, x, y, w, v, ex, ey, outs.count, outs.sums, outs.bins, outs.info),
                   outs, sites)
    assert reached == ["sph_sum_h", "sph_sum_a"]
    got = {"count": outs.count, "sums": outs.sums, "bin_index": outs.bins, "n_valid": outs.info.n_valid, "n_binned": outs.info.n_binned}
    check(got, model(x, y, w, v, ex, ey), "the call after the failures")


# ---- 10. context states --------------------------------------------------------------------------------------------------------
def test_the_call_between_an_upload_a_render_and_a_colormap(native, mips, ridge):
    from oracle import oracle_np
    rs = np.random.RandomState(12)
    pos = rs.normal(0.0, 25.0, (400, 3)).astype(f32)
    h, mass, q = np.full(400, 5.0, dtype=f32), rs.uniform(0.5, 2.0, 400).astype(f32), rs.normal(0.0, 1.0, 400).astype(f32)
    M, sf = oracle_np.transform_matrix(np.eye(3), np.zeros(3), 80.0)
    lut = np.linspace(0.0, 1.0, 256 * 4, dtype=f32)
    want = model(*ridge)

    def session(with_calls):
        c = native.Context(80, 2)
        results = []
        call = (lambda: results.append(run(c, *ridge))) if with_calls else (lambda: None)
        try:
            call()                                              # nothing set yet
            c.set_kernel_mips(mips)
            call()
            c.upload_particles(pos[:, 0], pos[:, 1], pos[:, 2], h, mass)
            c.upload_quantity(q)
            call()
            c.render(M, sf)
            call()
            image, stats = c.read_image(), {k: s for k, s in c.stats().items() if not k.startswith("ms_")}
            rgba = c.colormap_scalar(lut, -1.0, 1.0, False, True)
            call()
            return image, stats, rgba, c.read_image(), results
        finally:
            c.close()

    plain, called = session(False), session(True)
    for a, b in zip(plain[:4], called[:4]):
        assert (a == b) if isinstance(a, dict) else (a.tobytes() == b.tobytes())
    assert len(called[4]) == 5 and np.count_nonzero(plain[0]) > 1000
    for k, got in enumerate(called[4]):
        check(got, want, f"call {k} of the session")
        same_bytes(got, called[4][0])


# ---- 11. Python ----------------------------------------------------------------------------------------------------------------
def test_phase_diagram_of_arrays_with_automatic_ranges(ridge):
    import topsy_amd
    x, y, w, v = (a.copy() for a in ridge[:4])
    x[:4] = [0.0, -3.0, np.nan, np.inf]                        # a logarithmic axis ignores them; a linear one takes the finite ones
    d = topsy_amd.phase_diagram(x.astype(np.float64), y, w, v, bins=(40, 30), x_log=True, return_index=True)
    assert isinstance(d, topsy_amd.PhaseDiagram) and d.shape == (30, 40)
    good = x[4:].astype(np.float64)
    assert d.edges_x[0] == good.min() and d.edges_x[-1] == np.nextafter(good.max(), np.inf)
    assert d.edges_y[0] == float(y.min()) and d.edges_y[-1] == np.nextafter(float(y.max()), np.inf)
    m = model(x, y, w, v, d.edges_x, d.edges_y)
    assert m["n_valid"] == N1 - 2 and m["n_binned"] == N1 - 4
    assert m["bin_index"][4 + int(np.argmax(good))] % 40 == 39 and m["bin_index"][int(np.argmax(y))] // 40 == 29      # the maxima are binned
    got = {"count": d.count, "sums": d.sums, "bin_index": d.bin_index, "n_valid": d.info["n_valid"], "n_binned": d.info["n_binned"]}
    check(got, m, "phase_diagram, automatic ranges")
    occupied = m["sums"][0] != 0
    assert np.allclose(d.mean[occupied], m["sums"][1][occupied] / m["sums"][0][occupied], rtol=1e-9)
    assert np.isnan(d.mean[m["count"] == 0]).all()
    lin = topsy_amd.phase_diagram(x, y, bins=5)
    assert lin.edges_x[0] == -3.0 and lin.mean is None and lin.bin_index is None and lin.count.sum() == N1 - 2
    assert np.array_equal(lin.weight, lin.count.astype(np.float64))
    own = topsy_amd.phase_diagram(x, y, w, edges=(ridge[4], ridge[5]))
    check({"count": own.count, "sums": own.sums, "n_valid": own.info["n_valid"], "n_binned": own.info["n_binned"]},
          model(x, y, w, None, ridge[4], ridge[5]), "phase_diagram, own edges")
    for kw in (dict(y=y[:-1]), dict(weights=w[:5]), dict(bins=0), dict(x_range=(2.0, 1.0)), dict(edges=([1.0], [1.0, 2.0]))):
        args = dict(x=x, y=y)
        args.update(kw)
        with pytest.raises(ValueError):
            topsy_amd.phase_diagram(**args)


def test_visualizer_phase_diagram_by_names():
    import topsy_amd
    n = 5000
    rs = np.random.RandomState(21)
    pos = (rs.normal(0.0, 1.0, (n, 3)) * np.array([20.0, 20.0, 4.0])).astype(f32)
    mass = rs.uniform(0.5, 2.0, n).astype(f32)
    T = np.exp(rs.normal(9.0, 1.5, n)).astype(f32)
    vis = topsy_amd.from_arrays(pos, None, mass, quantities={"temp": T}, render_resolution=64)
    try:
        d = vis.phase_diagram("rho", "temp", bins=(32, 24), value="temp", return_index=True)
        rho = vis.data_loader.get_named_quantity("rho")
        assert rho.shape == (n,) and d.x_log and d.y_log and d.shape == (24, 32)
        m = model(rho, T, mass, T, d.edges_x, d.edges_y)
        got = {"count": d.count, "sums": d.sums, "bin_index": d.bin_index, "n_valid": d.info["n_valid"], "n_binned": d.info["n_binned"]}
        check(got, m, "vis.phase_diagram('rho', 'temp')")
        assert m["n_binned"] == np.count_nonzero(np.isfinite(rho) & (rho > 0)) > n // 2
        occupied = m["sums"][0] != 0
        assert np.allclose(d.mean[occupied], m["sums"][1][occupied] / m["sums"][0][occupied], rtol=1e-9)
        # the mean temperature of a row lies inside the row
        rows = np.nonzero(occupied)[0]
        assert (d.mean[occupied] >= d.edges_y[rows] * (1 - 1e-6)).all() and (d.mean[occupied] <= d.edges_y[rows + 1] * (1 + 1e-6)).all()
        # weight=None counts particles
        counted = vis.phase_diagram("rho", "temp", weight=None, edges=(d.edges_x, d.edges_y))
        assert np.array_equal(counted.count, d.count) and np.array_equal(counted.weight, d.count.astype(np.float64))
        assert counted.mean is None
        # select: exactly the particles the model puts into the rectangle of whole cells
        x_range, y_range = (d.edges_x[8], d.edges_x[20]), (d.edges_y[5], d.edges_y[15])
        i, j = m["bin_index"] % 32, m["bin_index"] // 32
        want = (m["bin_index"] >= 0) & (i >= 8) & (i < 20) & (j >= 5) & (j < 15)
        assert np.array_equal(d.select(x_range, y_range), want) and 0 < want.sum() < n
        with pytest.raises(ValueError):
            counted.select(x_range, y_range)
        # "mass" and "smooth" are names too; linear axes on request
        ms = vis.phase_diagram("smooth", "mass", weight=None, bins=8, y_log=False)
        check({"count": ms.count, "sums": ms.sums, "n_valid": ms.info["n_valid"], "n_binned": ms.info["n_binned"]},
              model(vis.data_loader.get_smooth(), mass, None, None, ms.edges_x, ms.edges_y), "smooth against mass")
        assert ms.count.sum() == n and not ms.y_log
        for kw in (dict(x="nope", y="temp"), dict(x="rho", y="temp", weight="nope"), dict(x="rho", y="temp", value="v_div"),
                   dict(x="rho", y="temp", bins=0)):
            with pytest.raises(ValueError):
                vis.phase_diagram(**kw)
    finally:
        vis.close()


def test_a_loader_without_host_arrays_is_refused():
    import topsy_amd
    vis = topsy_amd.synthetic_on_device(20000, render_resolution=32)
    try:
        with pytest.raises(ValueError):
            vis.phase_diagram("rho", "temp")
    finally:
        vis.close()
