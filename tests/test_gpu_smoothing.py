"""tsp_smoothing_lengths on the GPU: bit-exact against the float32 brute force of test_smoothing_cpu.py on scenes built to
break a spatial search (ties, duplicates, flat and degenerate boxes, faces, outliers, non-finite coordinates, periodic
wrap), within 1e-6 of scipy's kd-tree at 1e6 particles, argument errors that change nothing, and the product path of a
snapshot without smoothing lengths."""
import ctypes

import numpy as np
import pytest

from test_smoothing_cpu import brute_force_smoothing, kdtree_smoothing

pytestmark = pytest.mark.gpu
KS = (2, 8, 32, 64)


def _scenes():
    rs = np.random.RandomState(7)
    out = {}
    out["uniform"] = (rs.uniform(-1, 1, size=(12000, 3)).astype(np.float32), 0.0)
    # clustered cores over a background, plus outliers 1e4 x farther away
    cores = np.concatenate([rs.normal(size=(2500, 3)) * s + c for s, c in ((0.01, 0.3), (0.05, -0.4), (0.002, 0.0))])
    bg = rs.uniform(-1, 1, size=(4000, 3))
    outl = rs.normal(size=(30, 3))
    outl = outl / np.linalg.norm(outl, axis=1, keepdims=True) * 1e4 * rs.uniform(0.5, 1.0, size=(30, 1))
    out["clustered_outliers"] = (np.concatenate([cores, bg, outl]).astype(np.float32), 0.0)
    # integer lattice: many exact ties and duplicates
    out["lattice"] = (rs.randint(0, 14, size=(10000, 3)).astype(np.float32), 0.0)
    # 40 copies of one point: h = 0 for k <= 40
    dup = rs.uniform(-1, 1, size=(3000, 3))
    dup[100:140] = dup[7]
    out["duplicates"] = (dup.astype(np.float32), 0.0)
    # points on the bounding-box faces
    faces = rs.uniform(0, 1, size=(8000, 3))
    sel = rs.randint(0, 3, size=8000)
    side = rs.randint(0, 2, size=8000).astype(np.float64)
    faces[np.arange(8000)[:4000], sel[:4000]] = side[:4000]
    faces[0], faces[1] = 0.0, 1.0
    out["faces"] = (faces.astype(np.float32), 0.0)
    # a plane and a line: zero extent on some axes
    plane = rs.uniform(-2, 2, size=(6000, 3)).astype(np.float32)
    plane[:, 2] = np.float32(0.75)
    out["plane"] = (plane, 0.0)
    line = np.zeros((5000, 3), dtype=np.float32)
    line[:, 0] = rs.uniform(-3, 3, size=5000)
    line[:, 1], line[:, 2] = np.float32(-1.5), np.float32(2.0)
    out["line"] = (line, 0.0)
    # 1 % non-finite coordinates
    nf = rs.normal(size=(10000, 3)).astype(np.float32)
    bad = rs.choice(10000, 100, replace=False)
    nf[bad, rs.randint(0, 3, size=100)] = rs.choice(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), size=100)
    out["non_finite"] = (nf, 0.0)
    # periodic box: neighbours across the faces, positions up to several periods outside [0, L)
    L = 25.0
    per = rs.uniform(0, L, size=(10000, 3))
    per[:3000] = rs.uniform(0, 1.5, size=(3000, 3)) + rs.randint(0, 2, size=(3000, 3)) * (L - 1.5)   # clustered at the corners
    per += rs.randint(-3, 4, size=per.shape) * L
    out["periodic"] = (per.astype(np.float32), L)
    return out


SCENES = _scenes()


@pytest.fixture(scope="module")
def ctx():
    from topsy_amd import _native
    c = _native.Context(64, 2)
    yield c
    c.close()


@pytest.mark.parametrize("name", list(SCENES))
def test_bit_exact_against_brute_force(ctx, name):
    pos, L = SCENES[name]
    want = brute_force_smoothing(pos, KS, period=L)
    for k in KS:
        got = ctx.smoothing_lengths(pos[:, 0], pos[:, 1], pos[:, 2], k, L)
        assert got.dtype == np.float32 and got.shape == (len(pos),)
        same = (got.view(np.uint32) == want[k].view(np.uint32)) | (np.isnan(got) & np.isnan(want[k]))
        assert same.all(), (f"{name}, k={k}: {np.count_nonzero(~same)} of {len(pos)} differ, e.g. index "
                            f"{np.flatnonzero(~same)[:5]}: {got[~same][:5]} vs {want[k][~same][:5]}")
    if name == "duplicates":
        assert (want[32][100:140] == 0).all() and (want[64][100:140] > 0).all()
    if name == "non_finite":
        bad = ~np.isfinite(pos).all(axis=1)
        assert np.isnan(got[bad]).all() and np.isfinite(got[~bad]).all()


def _clustered(n, seed, L=None):
    rs = np.random.RandomState(seed)
    n_cl = n // 2
    centres = rs.uniform(0.1, 0.9, size=(50, 3))
    cl = centres[rs.randint(0, 50, size=n_cl)] + rs.normal(size=(n_cl, 3)) * np.exp(rs.uniform(np.log(1e-3), np.log(3e-2), size=(n_cl, 1)))
    pos = np.concatenate([cl, rs.uniform(0, 1, size=(n - n_cl, 3))])
    if L is not None:
        pos = np.mod(pos * L, L)
    pos = pos.astype(np.float32)
    if L is not None:
        pos[pos >= np.float32(L)] = 0.0
    return pos


@pytest.mark.parametrize("periodic", [False, True])
def test_million_points_against_kdtree(ctx, periodic):
    L = 40.0 if periodic else None
    pos = _clustered(1_000_000, 11, L)
    got = ctx.smoothing_lengths(pos[:, 0], pos[:, 1], pos[:, 2], 32, L)
    want = kdtree_smoothing(pos, 32, period=L)
    assert not np.isnan(got).any()
    # across a periodic face the contract's float32 wrap, (x_j - x_i) - L rint(.), rounds x_j - x_i (close to L) to the
    # spacing of L: an absolute error the float64 kd-tree does not have
    atol = float(np.spacing(np.float32(L))) if periodic else 0.0
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=atol)


# ---- errors: TSP_EINVAL, and nothing changes ----------------------------------------------------------------------------
# Two renders of the same resident snapshot are not bit-identical: the tile kernels sum float32 partial images whose order the
# atomics decide.  Images are compared to 1e-5 (and 1e-5 of the largest value, for the cancelling sums of a signed quantity);
# fragment counts and particles exactly.
def _same_image(a, b):
    np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-5 * float(np.nanmax(np.abs(b))))


def _render_state(ctx, M, sf):
    ctx.render(M, sf)
    st = ctx.stats()
    counts = {k: v for k, v in st.items() if not k.startswith("ms_")}
    return ctx.read_image(), counts, ctx.download_particles()


def test_invalid_arguments_change_nothing(mips):
    from conftest import make_cloud
    from oracle import oracle_np
    from topsy_amd import _native
    lib = _native.load_library()
    fp = ctypes.POINTER(ctypes.c_float)
    ctx = _native.Context(160, 2)
    ctx.set_kernel_mips(mips)
    pos, h, m, q, _ = make_cloud(4000, seed=3)
    ctx.upload_particles(pos[:, 0], pos[:, 1], pos[:, 2], h, m)
    ctx.upload_quantity(q)
    ctx.set_option("count_fragments", 1)
    M, sf = oracle_np.transform_matrix(np.eye(3), np.zeros(3), 90.0)
    img0, counts0, parts0 = _render_state(ctx, M, sf)

    n = 1000
    rs = np.random.RandomState(1)
    x, y, z = (np.ascontiguousarray(rs.uniform(0, 1, n), dtype=np.float32) for _ in range(3))
    few = x.copy()
    few[5:] = np.nan
    out = np.full(n, 7.0, dtype=np.float32)
    P = lambda a: a.ctypes.data_as(fp)                                              # noqa: E731
    cases = [(n, P(x), P(y), P(z), 1, 0.0, P(out)), (n, P(x), P(y), P(z), 65, 0.0, P(out)),
             (n, P(x), P(y), P(z), 0, 0.0, P(out)), (n, P(x), P(y), P(z), -3, 0.0, P(out)),
             (n, P(x), P(y), P(z), 32, -1.0, P(out)), (n, P(x), P(y), P(z), 32, float("nan"), P(out)),
             (n, P(x), P(y), P(z), 32, float("inf"), P(out)), (0, P(x), P(y), P(z), 8, 0.0, P(out)),
             (-5, P(x), P(y), P(z), 8, 0.0, P(out)), (1 << 31, P(x), P(y), P(z), 8, 0.0, P(out)),
             (n, None, P(y), P(z), 8, 0.0, P(out)), (n, P(x), P(y), P(z), 8, 0.0, None),
             (n, P(few), P(y), P(z), 8, 0.0, P(out)), (7, P(x), P(y), P(z), 8, 0.0, P(out))]
    for args in cases:
        assert lib.tsp_smoothing_lengths(ctx._h, *args) == -1, args          # TSP_EINVAL
        assert (out == 7.0).all(), args
    assert lib.tsp_smoothing_lengths(None, n, P(x), P(y), P(z), 8, 0.0, P(out)) == -1

    h_valid = ctx.smoothing_lengths(x, y, z, 8)
    np.testing.assert_array_equal(h_valid, brute_force_smoothing(np.stack([x, y, z], 1), 8))
    img1, counts1, parts1 = _render_state(ctx, M, sf)
    _same_image(img0, img1)
    assert counts0 == counts1 and counts0["n_fragments"] > 0
    for k in parts0:
        assert np.array_equal(parts0[k], parts1[k]), k
    ctx.close()


def test_works_on_a_fresh_context_and_the_multi_gpu_context():
    from topsy_amd import _native, multigpu
    pos, _ = SCENES["lattice"]
    want = brute_force_smoothing(pos, 16)
    ctx = _native.Context(16, 2)
    np.testing.assert_array_equal(ctx.smoothing_lengths(pos[:, 0], pos[:, 1], pos[:, 2], 16), want)
    ctx.close()
    mg = multigpu.MultiGpuContext(16, 2, [0, 0])
    np.testing.assert_array_equal(mg.smoothing_lengths(pos[:, 0], pos[:, 1], pos[:, 2], 16), want)
    mg.close()


# ---- the product path ---------------------------------------------------------------------------------------------------
def _snapshot(n=6000, seed=4, L=None):
    rs = np.random.RandomState(seed)
    pos = np.concatenate([rs.normal(size=(n // 2, 3)) * 3.0, rs.uniform(-15, 15, size=(n - n // 2, 3))])
    if L is not None:
        pos = np.mod(pos, L)
    pos = pos.astype(np.float32)
    mass = rs.uniform(0.5, 2.0, size=n).astype(np.float32)
    temp = rs.lognormal(size=n).astype(np.float32)
    return pos, mass, {"temp": temp}


def _images(vis):
    from topsy_amd.drawreason import DrawReason
    vis.scale = 20.0
    vis.rotate(0.3, 0.2)
    out = []
    for quantity in (None, "temp"):
        vis.quantity_name = quantity
        vis.render_sph(DrawReason.EXPORT)
        out.append(np.array(vis.get_sph_image(), copy=True))
    return out


@pytest.mark.parametrize("variant", ["plain", "with_cells", "periodic", "two_contexts"])
def test_from_arrays_without_smoothing_lengths(variant):
    import topsy_amd
    L = 30.0 if variant == "periodic" else None
    pos, mass, quantities = _snapshot(L=L)
    h = brute_force_smoothing(pos, 32, period=L or 0.0)
    kw = dict(quantities=quantities, render_resolution=128, with_cells=variant == "with_cells", periodicity_scale=L)
    if variant == "two_contexts":
        kw["device_ids"] = [0, 0]
    got_vis = topsy_amd.from_arrays(pos, None, mass, **kw)
    ref_vis = topsy_amd.from_arrays(pos, h, mass, **kw)
    try:
        ld = got_vis.data_loader
        # the loader's order (with_cells sorts the particles): its smoothing lengths are the brute force of its positions
        want = brute_force_smoothing(ld.get_positions(), 32, period=L or 0.0)
        assert np.array_equal(ld.get_smooth().view(np.uint32), want.view(np.uint32))
        assert np.array_equal(ld.get_pos_smooth()[:, 3], want)
        for a, b in zip(_images(got_vis), _images(ref_vis)):
            _same_image(a, b)
            assert np.nanmax(a) > 0          # (the weighted average is NaN where no particle reaches)
    finally:
        got_vis.close()
        ref_vis.close()


def test_from_arrays_n_smooth():
    import topsy_amd
    pos, mass, _ = _snapshot(n=3000)
    vis = topsy_amd.from_arrays(pos, None, mass, n_smooth=8, render_resolution=64)
    try:
        assert np.array_equal(vis.data_loader.get_smooth(), brute_force_smoothing(pos, 8))
    finally:
        vis.close()


def test_public_smoothing_lengths():
    import topsy_amd
    pos, L = SCENES["periodic"]
    np.testing.assert_array_equal(topsy_amd.smoothing_lengths(pos, periodicity_scale=L), brute_force_smoothing(pos, 32, period=L))
    pos, _ = SCENES["non_finite"]
    np.testing.assert_array_equal(topsy_amd.smoothing_lengths(pos, n_smooth=12), brute_force_smoothing(pos, 12))
