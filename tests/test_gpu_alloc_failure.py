"""Real allocation failures leave a context whole and usable.

tsp_render draws a block whole or not at all, and that includes a block whose list or bin allocation fails: the accumulator, the
channel layout and the statistics are restored, and the next call -- one whose need fits whatever capacity the failed one left
behind -- renders correctly.  Option debug_fail_alloc = k makes the k-th device allocation from now on fail as hipMalloc would, so
the tests below walk k = 1, 2, ... over every allocation site a render reaches, each on a fresh context, until the render
succeeds; after every failure the context must give the oracle's images for a smaller block, the failed block, and both
accumulated.  The set of sites reached is written out per mode: a new allocation site fails these tests until it is covered.
"""
import re

import numpy as np
import pytest

from conftest import make_cloud

pytestmark = pytest.mark.gpu

MAX_K = 64
R, SCALE = 512, 200.0
PX = 2.0 * SCALE / R               # world units per pixel: a footprint P pixels wide (4 h) has h = P * PX / 4
A_LEN = 128 * 512                  # block A: one range of 128 chunks (too few for chunk culling)
B_RANGES, B_LEN, B_GAP = 32, 67200, 64   # block B: 32 ranges of 132 chunks each (4224 >= 4096: chunk culling runs)
N_TOTAL = A_LEN + B_RANGES * (B_LEN + B_GAP)
# footprints in view per block: (small < 16 px, mid 16-64 px, huge >= 64 px)
A_COUNTS = (10_000, 20_000, 5_000)     # A's 5000 huge records are binned by band (>= 4096), its lists start at 2^16 records
B_COUNTS = (50_000, 600_000, 70_000)   # B overflows its mid list (N/4 = 537600 records) cold and both lists warm

MODES = ("weighted", "density", "depth", "rgb")
# what a render of block B allocates on a fresh context (cold) and after block A (warm: only what has to grow)
_COMMON_COLD = {"image64_entry", "range_prefix", "alive_list", "mid_geom", "mid_w", "huge_geom", "huge_w", "block_bounds", "cull_info",
                "mid_geom_replay", "mid_w_replay", "mband_count", "mband_base", "mitem_base", "mband_geom", "mband_w", "mitem_tile",
                "hband_geom", "hband_w", "hband_count"}
_COMMON_WARM = {"range_prefix", "alive_list", "block_bounds", "cull_info", "mid_geom_replay", "mid_w_replay", "huge_geom_replay",
                "huge_w_replay", "mband_geom", "mband_w", "mitem_tile", "hband_geom", "hband_w", "hband_count"}
RENDER_SITES = {
    **{(m, "cold"): _COMMON_COLD | {"weights_m"} for m in ("weighted", "density", "depth")},
    ("rgb", "cold"): _COMMON_COLD | {"weights_r", "weights_g", "weights_b", "count_diff", "count_band"},
    **{(m, "warm"): set(_COMMON_WARM) for m in MODES},
}
GENERIC_SITES = {"image64_entry", "range_prefix_generic"}
POSTPASS_SITES = {"colormap_scratch", "lut", "periodic_scratch", "outf", "lut2d", "sort_keys", "sort_keys_alt", "sort_tmp"}
INJECTED = re.compile(r"injected allocation failure at (\w+) \(debug_fail_alloc\)")


@pytest.fixture(scope="module")
def native():
    from topsy_amd import _native
    _native.load_library()
    return _native


def _place(rs, pos, h, idx, p_lo, p_hi):
    """footprints of p_lo..p_hi pixels spread over the whole view (every 64-row band of the image)"""
    pos[idx, 0] = rs.uniform(-0.95 * SCALE, 0.95 * SCALE, len(idx))
    pos[idx, 1] = rs.uniform(-0.95 * SCALE, 0.95 * SCALE, len(idx))
    pos[idx, 2] = rs.uniform(-10.0, 10.0, len(idx))
    h[idx] = rs.uniform(p_lo, p_hi, len(idx)) * (PX / 4)


@pytest.fixture(scope="module")
def scene():
    from oracle import oracle_np
    rs = np.random.RandomState(2024)
    pos = np.empty((N_TOTAL, 3), dtype=np.float32)
    h = np.empty(N_TOTAL, dtype=np.float32)
    # everything starts far outside the view (whole chunks of it are culled); each block's visible particles are shuffled into
    # the front of its index range
    pos[:, 0] = rs.uniform(1e5, 2e5, N_TOTAL)
    pos[:, 1] = rs.uniform(-50.0, 50.0, N_TOTAL)
    pos[:, 2] = rs.uniform(-10.0, 10.0, N_TOTAL)
    h[:] = rs.uniform(0.5, 5.0, N_TOTAL)
    for first, counts in ((0, A_COUNTS), (A_LEN, B_COUNTS)):
        order = first + rs.permutation(sum(counts))
        a, b = counts[0], counts[0] + counts[1]
        _place(rs, pos, h, order[:a], 2.0, 12.0)
        _place(rs, pos, h, order[a:b], 17.0, 30.0)
        _place(rs, pos, h, order[b:], 66.0, 80.0)
    b_starts = A_LEN + np.arange(B_RANGES, dtype=np.int64) * (B_LEN + B_GAP)
    M, sf = oracle_np.transform_matrix(np.eye(3), np.zeros(3), SCALE)
    return dict(pos=pos, h=h.astype(np.float32), m=rs.uniform(0.5, 1.5, N_TOTAL).astype(np.float32),
                q=rs.normal(size=N_TOTAL).astype(np.float32), rgb=rs.uniform(0.0, 1.0, (N_TOTAL, 3)).astype(np.float32),
                A=(np.asarray([0], dtype=np.int64), np.asarray([A_LEN], dtype=np.int64)),
                B=(b_starts, np.full(B_RANGES, B_LEN, dtype=np.int64)), M=M, sf=float(sf))


@pytest.fixture(scope="module")
def refs(scene, mips):
    """oracle images per (mode, block), each computed once: (float64 image, fragments, float64 sum of |terms| of channel 1)"""
    from oracle import oracle_c
    cache = {}
    x, y, z = (np.ascontiguousarray(scene["pos"][:, k]) for k in range(3))
    h, m, q, rgb = scene["h"], scene["m"], scene["q"], scene["rgb"]

    def get(mode, block):
        if (mode, block) not in cache:
            kw = dict(M=scene["M"], sf=scene["sf"], R=R, mips=mips, ranges=scene[block])
            if mode == "rgb":
                img, nf = oracle_c.splat(x, y, z, h, rgb[:, 0].copy(), rgb[:, 1].copy(), rgb[:, 2].copy(), mode=2, **kw)
            elif mode == "depth":
                img, nf = oracle_c.splat(x, y, z, h, m, mode=1, **kw)
            else:
                img, nf = oracle_c.splat(x, y, z, h, m, q if mode == "weighted" else None, mode=0, **kw)
            absq = oracle_c.splat(x, y, z, h, m, np.abs(q), mode=0, **kw)[0][..., 1].astype(np.float64) if mode == "weighted" else None
            cache[(mode, block)] = (img.astype(np.float64), nf, absq)
        return cache[(mode, block)]
    return get


def check_image(mode, got, want, abs_terms, what):
    """test_gpu_parity.py's tolerances"""
    got = got.astype(np.float64)
    if mode == "rgb":
        assert (np.abs(got[..., :3] - want[..., :3]) <= 1e-5 * np.abs(want[..., :3])).all(), f"{what}: colour channels"
        assert np.array_equal(got[..., 3], want[..., 3]), f"{what}: the fragment-count channel must be exact"
        return
    if mode == "depth":
        assert (np.abs(got - want) <= 1e-5 * np.abs(want)).all(), f"{what}: depth channels"
        return
    assert (np.abs(got[..., 0] - want[..., 0]) <= 1e-5 * np.abs(want[..., 0]) + 1e-30).all(), f"{what}: density channel"
    if mode == "density":
        assert (got[..., 1] == 0).all(), f"{what}: channel 1 of a density render must be zero"
    else:
        assert (np.abs(got[..., 1] - want[..., 1]) <= 1e-5 * abs_terms + 1e-30).all(), f"{what}: weighted channel"


def new_context(native, mips, scene, mode, overlap):
    ctx = native.Context(R, 4 if mode == "rgb" else 2)
    ctx.set_kernel_mips(mips)
    p = scene["pos"]
    ctx.upload_particles(p[:, 0], p[:, 1], p[:, 2], scene["h"], None if mode == "rgb" else scene["m"])
    if mode == "rgb":
        ctx.upload_rgb(*(scene["rgb"][:, k] for k in range(3)))
    if mode == "weighted":
        ctx.upload_quantity(scene["q"])
    ctx.set_option("count_fragments", 1)
    ctx.set_option("overlap_mid_huge", overlap)
    return ctx


def render(native, ctx, scene, mode, block, clear=True):
    nm = {"rgb": native.MODE_RGB, "depth": native.MODE_DEPTH}.get(mode, native.MODE_WEIGHTED)
    ctx.render(scene["M"], scene["sf"], scene[block][0], scene[block][1], clear=clear, mode=nm)


def render_and_check(native, ctx, scene, refs, mode, block, what):
    render(native, ctx, scene, mode, block)
    want, nf, absq = refs(mode, block)
    check_image(mode, ctx.read_image(), want, absq, f"{what}, block {block}")
    assert ctx.stats()["n_fragments"] == nf, f"{what}, block {block}: fragment count differs from the oracle"


@pytest.mark.parametrize("warm", ["cold", "warm"])
@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("mode", MODES)
def test_every_failed_allocation_of_a_render_leaves_the_context_usable(native, mips, scene, refs, mode, overlap, warm):
    reached = []
    for k in range(1, MAX_K + 1):
        ctx = new_context(native, mips, scene, mode, overlap)
        try:
            if warm == "warm":
                render(native, ctx, scene, mode, "A")
            before, st_before = ctx.read_image().copy(), ctx.stats()
            ctx.set_option("debug_fail_alloc", k)
            try:
                render(native, ctx, scene, mode, "B")
            except native.BackendError as e:
                found = INJECTED.search(str(e))
                assert found, f"k={k}: not the injected failure: {e}"
                reached.append(found.group(1))
            else:
                ctx.set_option("debug_fail_alloc", 0)
                want, nf, absq = refs(mode, "B")
                check_image(mode, ctx.read_image(), want, absq, f"k={k} (no failure left)")
                break
            what = f"after a failure at {reached[-1]} (k={k})"
            assert np.array_equal(ctx.read_image(), before), f"{what}: the float32 image changed"
            assert ctx.stats() == st_before, f"{what}: the statistics changed"
            ctx.set_option("debug_fail_alloc", 0)
            render_and_check(native, ctx, scene, refs, mode, "A", what)      # its need fits any capacity the failure left
            render_and_check(native, ctx, scene, refs, mode, "B", what)
            render(native, ctx, scene, mode, "A", clear=False)               # A + B accumulated
            (wa, nfa, aa), (wb, _, ab) = refs(mode, "A"), refs(mode, "B")
            check_image(mode, ctx.read_image(), wa + wb, None if aa is None else aa + ab, f"{what}, blocks B + A")
            assert ctx.stats()["n_fragments"] == nfa
        finally:
            ctx.close()
    else:
        pytest.fail(f"the render still failed at k={MAX_K}")
    print(f"\n{mode} overlap={overlap} {warm}: allocation sites reached: {sorted(reached)}")
    assert len(set(reached)) == len(reached), f"a site failed twice: {reached}"
    assert set(reached) == RENDER_SITES[(mode, warm)]


def test_failed_allocation_on_the_generic_path(native, mips):
    from oracle import oracle_c, oracle_np
    Rg = 128
    M, sf = oracle_np.transform_matrix(np.eye(3), np.zeros(3), 150.0)
    pos, h, m, q, _ = make_cloud(5000, seed=9)
    starts, lens = np.asarray([10, 700, 2500], dtype=np.int64), np.asarray([300, 1, 1700], dtype=np.int64)
    x, y, z = (np.ascontiguousarray(pos[:, k]) for k in range(3))
    want, _ = oracle_c.splat(x, y, z, h, m, q, mode=0, M=M, sf=float(sf), R=Rg, mips=mips, ranges=(starts, lens))
    at, _ = oracle_c.splat(x, y, z, h, m, np.abs(q), mode=0, M=M, sf=float(sf), R=Rg, mips=mips, ranges=(starts, lens))
    reached = []
    for k in range(1, MAX_K + 1):
        ctx = native.Context(Rg, 2)
        try:
            ctx.set_kernel_mips(mips)
            ctx.upload_particles(pos[:, 0], pos[:, 1], pos[:, 2], h, m)
            ctx.upload_quantity(q)
            ctx.set_option("debug_fail_alloc", k)
            try:
                ctx.render(M, sf, starts, lens, flags=native.PIPE_GENERIC)
                failed = False
            except native.BackendError as e:
                found = INJECTED.search(str(e))
                assert found, str(e)
                reached.append(found.group(1))
                assert (ctx.read_image() == 0).all(), f"{reached[-1]}: the image changed"
                ctx.set_option("debug_fail_alloc", 0)
                ctx.render(M, sf, starts, lens, flags=native.PIPE_GENERIC)
                failed = True
            ctx.set_option("debug_fail_alloc", 0)
            check_image("weighted", ctx.read_image(), want.astype(np.float64), at[..., 1].astype(np.float64), f"k={k}")
        finally:
            ctx.close()
        if not failed:
            break
    assert set(reached) == GENERIC_SITES


def enumerate_postpass(native, make, call, verify):
    """k = 1, 2, ... on fresh contexts (make) until `call` succeeds; after each injected failure `verify` must succeed"""
    reached = []
    for k in range(1, MAX_K + 1):
        ctx = make()
        try:
            ctx.set_option("debug_fail_alloc", k)
            try:
                call(ctx)
            except native.BackendError as e:
                found = INJECTED.search(str(e))
                assert found, str(e)
                reached.append(found.group(1))
                ctx.set_option("debug_fail_alloc", 0)
                verify(ctx, reached[-1])
            else:
                return reached
        finally:
            ctx.close()
    pytest.fail(f"still failing at k={MAX_K}")


def test_failed_postpass_allocations(native, mips):
    from oracle import oracle_c, oracle_np
    rs = np.random.RandomState(5)
    lut = np.ascontiguousarray(rs.uniform(0, 1, (256, 4)).astype(np.float32))
    big, small = (np.exp(rs.uniform(-8, 2, (s, s, 2))).astype(np.float32) for s in (96, 40))

    # host-image colormap: scratch and LUT, cold and after a smaller call (the failed call grows the scratch)
    def make_cm(warm):
        def make():
            ctx = native.Context(64, 2)
            if warm:
                ctx.colormap_scalar_host(small, lut, -3.0, 1.0, True, False)
            return ctx
        return make

    def verify_cm(ctx, site):
        for img in (small, big):
            assert np.array_equal(ctx.colormap_scalar_host(img, lut, -3.0, 1.0, True, False),
                                  oracle_c.colormap_scalar(img, lut, -3.0, 1.0, True, False)), site
    call_cm = lambda ctx: ctx.colormap_scalar_host(big, lut, -3.0, 1.0, True, False)   # noqa: E731
    reached = enumerate_postpass(native, make_cm(False), call_cm, verify_cm)
    assert reached == ["colormap_scratch", "lut"]
    reached += enumerate_postpass(native, make_cm(True), call_cm, verify_cm)
    assert reached[2:] == ["colormap_scratch"]

    # periodic tiling: the failed call grows the scratch; a smaller one and the same one then match the oracle bit for bit
    Rt = 128
    img = np.exp(rs.uniform(-4, 2, (Rt, Rt, 2))).astype(np.float32)
    off1, w1 = np.asarray([[0.3, -0.2]], dtype=np.float32), np.asarray([0.7], dtype=np.float32)
    offn, wn = rs.uniform(-1.5, 1.5, (64, 2)).astype(np.float32), rs.uniform(0.1, 1.0, 64).astype(np.float32)

    def make_tp():
        ctx = native.Context(Rt, 2)
        ctx.tile_periodic(off1, w1)     # (a small scratch first)
        ctx.write_image(img)
        return ctx

    def verify_tp(ctx, site):
        assert np.array_equal(ctx.read_image(), img), f"{site}: a failed tiling changed the image"
        for off, w in ((off1, w1), (offn, wn)):
            ctx.write_image(img)
            ctx.tile_periodic(off, w)
            assert np.array_equal(ctx.read_image(), oracle_np.periodic_tile(img, off, w)), site
    reached += enumerate_postpass(native, make_tp, lambda ctx: ctx.tile_periodic(offn, wn), verify_tp)
    assert reached[3:] == ["periodic_scratch"]

    # rgb colormap to float: its staging buffer
    rgb4 = np.zeros((64, 64, 4), dtype=np.float32)
    rgb4[..., :3] = np.exp(rs.uniform(-10, 3, (64, 64, 3)))

    def make_rgb():
        ctx = native.Context(64, 4)
        ctx.write_image(rgb4)
        return ctx

    def verify_rgb(ctx, site):
        assert np.array_equal(ctx.colormap_rgb(-6.0, -1.0, 2.2, as_float=True), oracle_c.colormap_rgb(rgb4, -6.0, -1.0, 2.2, as_float=True),
                              equal_nan=True), site
    reached += enumerate_postpass(native, make_rgb, lambda ctx: ctx.colormap_rgb(-6.0, -1.0, 2.2, as_float=True), verify_rgb)
    assert reached[4:] == ["outf"]

    # bivariate LUT: a failed upload leaves "no LUT" (an error, not a read through null), the next upload works
    lut2d = np.ascontiguousarray(rs.uniform(0, 1, (16, 16, 4)).astype(np.float32))
    cm2 = np.exp(rs.uniform(-4, 2, (64, 64, 2))).astype(np.float32)

    def verify_lut2d(ctx, site):
        with pytest.raises(native.BackendError, match="must be called first"):
            ctx.colormap_bivariate_host(cm2, -2.0, 1.0, -3.0, 2.0, True, True)
        ctx.colormap_set_lut2d(lut2d)
        assert np.array_equal(ctx.colormap_bivariate_host(cm2, -2.0, 1.0, -3.0, 2.0, True, True),
                              oracle_c.colormap_bivariate(cm2, lut2d, -2.0, 1.0, -3.0, 2.0, True, True)), site
    reached += enumerate_postpass(native, lambda: native.Context(64, 2), lambda ctx: ctx.colormap_set_lut2d(lut2d), verify_lut2d)
    assert reached[5:] == ["lut2d"]

    # content order statistics (autorange): three buffers of one group
    def make_sort():
        ctx = native.Context(64, 2)
        ctx.write_image(cm2)
        return ctx

    vals = np.sort(cm2[..., 0].ravel())

    def verify_sort(ctx, site):
        assert ctx.content_sort(0) == (vals.size, 0), site
        ranks = np.asarray([0, 1, vals.size // 2, vals.size - 1], dtype=np.int64)
        assert np.array_equal(ctx.content_values(ranks), vals[ranks]), site
    reached += enumerate_postpass(native, make_sort, lambda ctx: ctx.content_sort(0), verify_sort)
    assert reached[6:] == ["sort_keys", "sort_keys_alt", "sort_tmp"]
    assert set(reached) == POSTPASS_SITES


def test_debug_fail_alloc_rejects_negative_values(native):
    ctx = native.Context(64, 2)
    with pytest.raises(native.BackendError, match="debug_fail_alloc"):
        ctx.set_option("debug_fail_alloc", -1)
    ctx.close()
