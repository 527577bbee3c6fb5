"""The image post-passes at their edges: the autorange order statistics (tsp_content_sort / tsp_content_values /
tsp_content_neg_inf), the periodic tiling (tsp_tile_periodic) and the colormaps on host images and odd LUTs, each against a plain
reference (tests/postpass_ref.py, oracle/oracle_np.py, oracle/oracle.c).

Everything is bit equality over every pixel and every rank looked at, with two exceptions that are stated where they are used:
the derived rounding bound of the tiling against float64 (postpass_ref.tiling_bound) and the project's splat tolerance
(rtol 1e-5) where two different splat orders are compared.

One-line mutations of the library these tests were tried against (on a scratch copy; every one gives wrong results, none
indexes out of bounds), and the tests that failed:
  ordered_u32 without the sign-bit set for positives ......... every content_sort test, content_values_errors, all six autoranges
  n_nonpositive counting v < 0 ............................... every content_sort test, all six autoranges
  the radix sort over n - 1 keys ............................. every content_sort test, content_values_errors, all six autoranges
  -inf values not counted .................................... every content_sort test, the two weighted autoranges
  tile_axis inside with s <= R ............................... tiling_bit_exact at R = 1, 33, 257
  the y shift without its negation ........................... tiling_bit_exact (R >= 2), whole_pixels, not_finite, limits, scratch, accumulator
  tile_periodic_kernel<2> launched for four channels ......... tiling_bit_exact (C = 4), whole_pixels, scratch, accumulator[rgb]
  the tiled image converted back into the accumulator ........ tiling_leaves_the_accumulator_untiled (both modes)
  the 2-D LUT's n kept when a smaller LUT is uploaded ........ lut_sizes
  the bivariate map's NaN clamp removed ...................... host_image_colormaps (3 shapes), bivariate_special_values, lut_sizes, parameters
  tsp_colormap_rgb_host accepting H = 0 ...................... host_image_colormaps_refuse_bad_shapes"""
import ctypes

import numpy as np
import pytest

import postpass_ref
from conftest import make_cloud

pytestmark = pytest.mark.gpu

f32 = np.float32
EINVAL, ESTATE = r"error -1:", r"error -4:"


@pytest.fixture(scope="module")
def native():
    from topsy_amd import _native
    _native.load_library()
    return _native


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ================================================================================================ order statistics
_IMAGES = {}


def sort_image(R, C, seed=0):
    """exp(U(-90, 80)) with random sign, then rows (single elements below R = 16) of the values a sort can get wrong"""
    key = (R, C, seed)
    if key not in _IMAGES:
        rs = np.random.RandomState(1000 * seed + 10 * R + C)
        img = (np.exp(rs.uniform(-90, 80, size=(R, R, C))) * rs.choice([-1.0, 1.0], size=(R, R, C))).astype(f32)
        special = [0.0, -0.0, 1e-42, -1e-42, np.inf, -np.inf, np.nan, 3e38, -3e38, 1.5]      # (1.5: duplicates over a whole row)
        if R >= 16:
            for k, s in enumerate(special):
                img[k] = f32(s)
            img[len(special), :, 0] = f32(0.0)            # (0, x): kind 1 gives +-inf and, with the next row, NaN
            img[len(special) + 1, :, :2] = f32(0.0)
            img[len(special) + 2, :, 0] = f32(-0.0)
        else:
            flat = img.reshape(-1)
            for k, s in enumerate(special[:flat.size // 2]):
                flat[2 * k] = f32(s)
        _IMAGES[key] = img
    return _IMAGES[key]


def check_sort(native, ctx, img, kind, scale, label):
    """content_sort's counts, then the values: every rank up to 2^16 finite values, else the ends, the neighbours of n_nonpositive
    and 4096 seeded random ranks"""
    want, n_fin, n_nonpos = postpass_ref.content_values_ref(img, kind, scale)
    n_neg_inf = int(np.isneginf(postpass_ref.content_all(img, kind, scale)).sum())
    assert ctx.content_sort(kind, scale) == (n_fin, n_nonpos), label
    assert ctx.content_neg_inf() == n_neg_inf, label
    if n_fin == 0:
        with pytest.raises(native.BackendError, match=EINVAL):
            ctx.content_values([0])
        return
    if n_fin <= 2 ** 16:
        ranks = np.arange(n_fin, dtype=np.int64)
    else:
        rs = np.random.RandomState(n_fin % 65521)
        ranks = np.concatenate([[0, 1, n_fin - 2, n_fin - 1], np.clip([n_nonpos - 1, n_nonpos], 0, n_fin - 1),
                                rs.randint(0, n_fin, size=4096)]).astype(np.int64)
    got = ctx.content_values(ranks)
    bad = np.flatnonzero(bits(got) != bits(want[ranks]))
    assert bad.size == 0, (label, bad.size, ranks[bad[:4]], got[bad[:4]], want[ranks[bad[:4]]])


SCALES = [1.0, 3.7, 1e-30, 1e10]        # 1e-30: products become denormal (kept, not flushed); 1e10: part of the image overflows
LAYOUTS = [(2, 2, (0, 1, 3)), (4, 4, (0, 1, 2, 3)), (4, 2, (0, 1, 3))]      # (context channels, image channels, valid kinds)


@pytest.mark.parametrize("R", [1, 2, 33, 255, 256])
def test_content_sort_every_kind_layout_and_scale(native, R):
    for c_ctx, c_img, kinds in LAYOUTS:
        ctx = native.Context(R, c_ctx)
        img = sort_image(R, c_img)
        ctx.write_image(img)
        for kind in kinds:
            for scale in SCALES:
                check_sort(native, ctx, img, kind, scale, (R, c_ctx, c_img, kind, scale))
        if c_img == 2:
            with pytest.raises(native.BackendError, match=EINVAL):      # rgb content of a 2-channel image
                ctx.content_sort(2)
        with pytest.raises(native.BackendError, match=EINVAL):
            ctx.content_sort(4)
        with pytest.raises(native.BackendError, match=EINVAL):
            ctx.content_sort(-1)
        ctx.close()


@pytest.mark.parametrize("R", [1024, 2048])
def test_content_sort_large_images(native, R):
    """up to 1.7e7 keys (R = 2048, four channels, kind 3): several radix passes and a grid-stride tail in the key kernel"""
    for c, kinds in ((2, (0, 1, 3)), (4, (0, 1, 2, 3))):
        ctx = native.Context(R, c)
        img = sort_image(R, c)
        ctx.write_image(img)
        for kind in kinds:
            for scale in (SCALES if (kind == 3 and c == 4) else [1.0]):
                check_sort(native, ctx, img, kind, scale, (R, c, kind, scale))
        ctx.close()


def test_content_sort_reuses_its_buffers(native):
    """kind 3 sizes the key buffers; smaller sorts after it, and a sort after a new image, must see only their own keys"""
    R = 200
    ctx = native.Context(R, 4)
    img = sort_image(R, 4)
    ctx.write_image(img)
    for kind in (3, 0, 2, 0):
        check_sort(native, ctx, img, kind, 1.0, ("reuse", kind))
    other = sort_image(R, 4, seed=1)
    assert not np.array_equal(bits(img), bits(other))
    ctx.write_image(other)
    for kind in (0, 3, 1):
        check_sort(native, ctx, other, kind, 3.7, ("new image", kind))
    two = sort_image(R, 2, seed=2)                   # a narrower layout in the same context
    ctx.write_image(two)
    for kind in (3, 1, 0):
        check_sort(native, ctx, two, kind, 1.0, ("two channels", kind))
    ctx.close()


def test_content_values_errors(native):
    R = 16
    ctx = native.Context(R, 2)
    with pytest.raises(native.BackendError, match=ESTATE):      # nothing sorted yet
        ctx.content_values([0])
    with pytest.raises(native.BackendError, match=ESTATE):
        ctx.content_neg_inf()
    ctx.write_image(np.full((R, R, 2), np.nan, dtype=f32))
    for kind in (0, 1, 3):
        assert ctx.content_sort(kind) == (0, 0)
        assert ctx.content_neg_inf() == 0
        for rank in (0, -1, 1, R * R):
            with pytest.raises(native.BackendError, match=EINVAL):
                ctx.content_values([rank])
    img = sort_image(R, 2)
    ctx.write_image(img)
    n_fin, _ = ctx.content_sort(0)
    assert 0 < n_fin < R * R
    lib = native.load_library()
    for rank in (n_fin, -1, 2 ** 40):                              # each as the only rank of its call: `out` stays untouched
        r = np.array([rank], dtype=np.int64)
        out = np.array([123.25], dtype=f32)
        rc = lib.tsp_content_values(ctx._h, r.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 1,
                                    out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
        assert rc == -1 and out[0] == f32(123.25), (rank, rc, out)
    assert ctx.content_values([]).size == 0
    assert same_bits(ctx.content_values([n_fin - 1, 0, 0]), postpass_ref.content_values_ref(img, 0, 1.0)[0][[n_fin - 1, 0, 0]])
    ctx.close()


AUTORANGE_MAPS = {      # name -> (render_mode, weighted_average or None, rgb images?)
    "density": ("univariate", False, False), "weighted": ("univariate", True, False),
    "bivariate_density": ("bivariate", False, False), "bivariate_weighted": ("bivariate", True, False),
    "rgb": ("rgb", None, True), "rgb_hdr": ("rgb-hdr", None, True),
}


@pytest.mark.parametrize("map_name", list(AUTORANGE_MAPS))
def test_device_autorange_equals_host_on_degenerate_images(map_name):
    """Product level: the images of tests/test_autorange_cpu.py in a Visualizer's render target; colormap.autorange(get_image())
    against colormap.autorange_on_device, the equality of test_device_autorange_equals_host_autorange (NaN equal to NaN), or
    both raise."""
    import topsy_amd
    from topsy_amd.drawreason import DrawReason
    mode, weighted, rgb = AUTORANGE_MAPS[map_name]
    v = topsy_amd.test(100, render_resolution=postpass_ref.AUTORANGE_R, render_mode=mode)
    v.render_sph(DrawReason.EXPORT)
    if weighted is not None:
        v.colormap.update_parameters({"weighted_average": weighted})
    images = postpass_ref.autorange_images_rgb() if rgb else postpass_ref.autorange_images()
    stale = {k: None for k in postpass_ref.AUTORANGE_KEYS if k not in ("vmin", "vmax", "log")}
    failures = []

    def run(fn):
        reset = {"vmin": 0.0, "vmax": 1.0} | {k: s for k, s in stale.items() if k in v.colormap.get_parameters()}
        v.colormap.update_parameters(reset)
        try:
            fn()
        except Exception as e:       # noqa: BLE001 -- an empty sample: both paths must fail together
            return "raised", type(e).__name__
        return "ok", v.colormap.get_parameters()
    for name, img in images.items():
        v._sph._context.write_image(img)
        for S in (1.0, 3.7):
            v._sph.last_render_mass_scale = S
            with np.errstate(all="ignore"):
                h_state, host = run(lambda: v.colormap.autorange(v._sph.get_image()))
            d_state, dev = run(lambda: v.colormap.autorange_on_device(S))
            if h_state != d_state:
                failures.append((name, S, host, dev))
            elif h_state == "ok":
                k = postpass_ref.autorange_parameters_equal(host, dev)
                if k is not None:
                    failures.append((name, S, k, host[k], dev[k]))
    v.close()
    assert not failures, failures


# ================================================================================================ periodic tiling
def _rotation(seed):
    rs = np.random.RandomState(seed)
    q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
    return q


ROTATIONS = [np.eye(3), _rotation(1), _rotation(2)]
PANEL_SCALES = [0.3, 100.0 / 130.0, 1.0, 2.5]


def signed_image(R, C, seed):
    rs = np.random.RandomState(seed)
    return (np.exp(rs.uniform(-30, 10, size=(R, R, C))) * rs.choice([-1.0, 1.0], size=(R, R, C))).astype(f32)


def tile(ctx, img, off, w):
    ctx.write_image(img)
    ctx.tile_periodic(off, w)
    return ctx.read_image()


@pytest.mark.parametrize("C", [2, 4])
@pytest.mark.parametrize("R", [1, 2, 33, 200, 257, 1024])
def test_tiling_bit_exact_and_within_the_float64_bound(native, R, C):
    from oracle import oracle_np
    ctx = native.Context(R, C)
    img = signed_image(R, C, seed=R + C)
    for rot in (ROTATIONS[1:2] if R == 1024 else ROTATIONS):      # (the numpy oracle takes seconds at 1024^2)
        for scale in PANEL_SCALES:
            off, w = oracle_np.periodic_instances(rot, scale)
            got = tile(ctx, img, off, w)
            want = oracle_np.periodic_tile(img, off, w)
            assert same_bits(got, want), (R, C, scale, int((bits(got) != bits(want)).sum()))
            if R <= 257:
                total, A, count = postpass_ref.tile_periodic_f64(img, off, w)
                bound = postpass_ref.tiling_bound(A, count)
                for name, res in (("oracle", want), ("device", got)):
                    err = np.abs(res.astype(np.float64) - total)
                    assert (err <= bound).all(), (name, R, C, scale, float((err / np.maximum(bound, 1e-300)).max()))
            else:
                count = postpass_ref.tile_inside_count(R, off)
            assert (bits(got[count == 0]) == 0).all(), "a pixel no instance covers must be exactly +0"
            if scale == 2.5:
                assert count.max() < len(w) / 2, "at this panel scale most instances lie outside the image"
    ctx.close()


def shifted(img, kx, ky):
    """img moved kx columns to the right and ky rows UP, zero where the source lies outside"""
    R = img.shape[0]
    out = np.zeros_like(img)
    j = np.arange(R)
    sj, si = j + ky, j - kx                       # source row / column of every destination row / column
    vj, vi = (sj >= 0) & (sj < R), (si >= 0) & (si < R)
    out[np.ix_(j[vj], j[vi])] = img[np.ix_(sj[vj], si[vi])]
    return out


@pytest.mark.parametrize("R", [64, 1024])
def test_tiling_by_whole_pixels_is_a_shifted_copy(native, R):
    rs = np.random.RandomState(R)
    for C in (2, 4):
        ctx = native.Context(R, C)
        img = np.exp(rs.uniform(-5, 5, size=(R, R, C))).astype(f32)        # positive: x * 1 + y * 0 keeps every bit
        assert (tile(ctx, img, np.zeros((0, 2), dtype=f32), np.zeros(0, dtype=f32)) == 0).all()          # n = 0
        assert same_bits(tile(ctx, img, [[0.0, 0.0]], [1.0]), img)                                        # the identity
        shifts = [(1, 0), (-1, 0), (0, 1), (0, -1), (3, -5), (-7, 2), (R - 1, 0), (0, -(R - 1)), (R // 2, R // 2)]
        for kx, ky in shifts:
            off = np.array([[2.0 * kx / R, 2.0 * ky / R]], dtype=f32)
            assert (off * (f32(0.5) * f32(R)) == np.array([[kx, ky]], dtype=f32)).all(), "the shift must be a whole pixel count"
            got = tile(ctx, img, off, [1.0])
            assert same_bits(got, shifted(img, kx, ky)), (R, C, kx, ky)
        # +y in clip space is up: the bottom row of the image arrives one row higher (lower row index)
        got = tile(ctx, img, [[0.0, 2.0 / R]], [1.0])
        assert same_bits(got[R - 2], img[R - 1]) and (got[R - 1] == 0).all()
        # two instances, weights 0.25 and 0.5 (exact products): one float32 sum per pixel
        off2 = np.array([[2.0 * 2 / R, 0.0], [0.0, 2.0 * -3 / R]], dtype=f32)
        want = (f32(0.0) + shifted(img, 2, 0) * f32(0.25)) + shifted(img, 0, -3) * f32(0.5)
        assert same_bits(tile(ctx, img, off2, [0.25, 0.5]), want)
        for ox, oy in ((2.0, 0.0), (-2.0, 0.0), (0.0, 2.0), (0.0, -2.0), (2.0, -2.0)):                   # a whole image away
            assert (bits(tile(ctx, img, [[ox, oy]], [1.0])) == 0).all(), (ox, oy)
        ctx.close()


def test_tiling_of_values_and_offsets_that_are_not_finite(native):
    from oracle import oracle_np
    R = 64
    rs = np.random.RandomState(3)
    ctx = native.Context(R, 2)
    img = np.exp(rs.uniform(-5, 5, size=(R, R, 2))).astype(f32)
    # weight 0 over an infinite pixel: 0 * inf = NaN, as the oracle (the taps with coefficient 0 touch it too)
    bad = img.copy()
    bad[10, 20, 0] = np.inf
    got = tile(ctx, bad, [[0.0, 0.0]], [0.0])
    want = oracle_np.periodic_tile(bad, [[0.0, 0.0]], [0.0])
    assert np.isnan(got[10, 20, 0]) and np.array_equal(got, want, equal_nan=True)
    assert np.array_equal(np.isnan(got[..., 0]), postpass_ref.tile_touch_mask(R, [[0.0, 0.0]], (10, 20)))
    assert (got[..., 1] == 0).all()
    # an instance with a NaN offset contributes nothing
    off = np.array([[0.11, -0.23], [np.nan, 0.1], [0.2, np.nan], [np.nan, np.nan], [-0.4, 0.31]], dtype=f32)
    w = np.array([0.7, 1.0, 1.0, 1.0, 0.4], dtype=f32)
    got = tile(ctx, img, off, w)
    assert np.isfinite(got).all() and same_bits(got, oracle_np.periodic_tile(img, off[[0, 4]], w[[0, 4]]))
    # NaN and inf pixels reach exactly the output pixels one of whose taps is that pixel
    off, w = oracle_np.periodic_instances(_rotation(5), 0.45)
    for value, pixel in ((np.nan, (31, 7)), (np.inf, (0, 63)), (-np.inf, (63, 0))):
        bad = img.copy()
        bad[pixel[0], pixel[1], 1] = value
        got = tile(ctx, bad, off, w)
        want = oracle_np.periodic_tile(bad, off, w)
        assert np.array_equal(got, want, equal_nan=True), value
        touched = postpass_ref.tile_touch_mask(R, off, pixel)
        assert touched.any() and not touched.all()
        assert np.array_equal(~np.isfinite(got[..., 1]), touched), value
        assert np.isfinite(got[..., 0]).all()
        clean = oracle_np.periodic_tile(img, off, w)
        assert same_bits(got[~touched], clean[~touched])
    ctx.close()


def test_tiling_limits(native, mips):
    from oracle import oracle_np
    from topsy_amd import kernel_lut
    R = 33
    rs = np.random.RandomState(11)
    ctx = native.Context(R, 2)
    img = signed_image(R, 2, seed=1)
    off = rs.uniform(-1.2, 1.2, size=(4097, 2)).astype(f32)
    w = rs.uniform(-1.0, 1.0, size=4097).astype(f32)
    got = tile(ctx, img, off[:4096], w[:4096])                      # the cap itself
    assert same_bits(got, oracle_np.periodic_tile(img, off[:4096], w[:4096]))
    ctx.write_image(img)
    with pytest.raises(native.BackendError, match=EINVAL):
        ctx.tile_periodic(off, w)
    assert same_bits(ctx.read_image(), img), "a refused tiling changed the image"
    # after the occlusion pass the accumulator holds keys: no tiling
    pos, h, m, q, _ = make_cloud(500, seed=4)
    ctx.set_kernel_mips(mips)
    ctx.set_sphere_mips(kernel_lut.sphere_mips())
    ctx.upload_particles(pos[:, 0], pos[:, 1], pos[:, 2], h, m)
    ctx.upload_quantity(q)
    M, sf = oracle_np.transform_matrix(np.eye(3), np.zeros(3), 150.0)
    ctx.render_surface(M, sf, 0.0)
    before = ctx.read_image()
    with pytest.raises(native.BackendError, match=ESTATE):
        ctx.tile_periodic(off[:3], w[:3])
    assert np.array_equal(ctx.read_image(), before, equal_nan=True)
    ctx.close()


def test_tiling_shares_its_scratch_with_the_host_colormaps(native, golden):
    """tile_periodic and the *_host colormaps use one scratch buffer sized on first use: small, larger, then a different split"""
    from oracle import oracle_c, oracle_np
    R = 48
    rs = np.random.RandomState(8)
    lut = golden["colormap_luts.npz"]["viridis"]
    ctx = native.Context(R, 4)
    img2 = signed_image(R, 2, seed=2)
    assert same_bits(tile(ctx, img2, [[0.25, -0.125]], [0.75]), oracle_np.periodic_tile(img2, [[0.25, -0.125]], [0.75]))     # n = 1
    big = np.exp(rs.uniform(-8, 2, size=(2 * R, 2 * R, 2))).astype(f32)                    # four times the context's image
    assert np.array_equal(ctx.colormap_scalar_host(big, lut, -3.0, 1.0, True, False), oracle_c.colormap_scalar(big, lut, -3.0, 1.0, True, False))
    off, w = rs.uniform(-1.2, 1.2, size=(125, 2)).astype(f32), rs.uniform(-1.0, 1.0, size=125).astype(f32)
    assert same_bits(tile(ctx, img2, off, w), oracle_np.periodic_tile(img2, off, w))                                           # n = 125
    img4 = signed_image(R, 4, seed=3)
    assert same_bits(tile(ctx, img4, off, w), oracle_np.periodic_tile(img4, off, w))                                           # C 2 -> 4
    assert np.array_equal(ctx.colormap_scalar_host(big, lut, -3.0, 1.0, True, True), oracle_c.colormap_scalar(big, lut, -3.0, 1.0, True, True))
    assert same_bits(tile(ctx, img2, off[:7], w[:7]), oracle_np.periodic_tile(img2, off[:7], w[:7]))                           # and back
    ctx.close()


@pytest.mark.parametrize("mode", ["weighted", "rgb"])
def test_tiling_leaves_the_accumulator_untiled(native, mips, mode):
    """include/topsy_splat.h: "The float64 accumulator keeps the untiled render, so a later tsp_render(clear = 0) continues from
    the raw image" -- what every periodic REFINE frame relies on.  Two splat orders are compared here, hence the project's splat
    tolerance (rtol 1e-5, atol 1e-30, as test_periodic_sph_output); a tiling that leaked into the accumulator is wrong by a
    factor of the order of the number of instances."""
    from oracle import oracle_np
    R, n = 128, 4000
    pos, h, m, q, rgb = make_cloud(n, seed=12)
    q = np.abs(q) + f32(0.1)          # (no cancellation in the weighted channel: a relative tolerance is meaningful)
    M, sf = oracle_np.transform_matrix(_rotation(7), np.zeros(3), 120.0)
    off, w = oracle_np.periodic_instances(_rotation(7), 100.0 / 130.0)
    images = []
    for tiled_in_between in (True, False):
        ctx = native.Context(R, 4 if mode == "rgb" else 2)
        ctx.set_kernel_mips(mips)
        if mode == "rgb":
            ctx.upload_particles(pos[:, 0], pos[:, 1], pos[:, 2], h, None)
            ctx.upload_rgb(rgb[:, 0], rgb[:, 1], rgb[:, 2])
            kw = {"mode": native.MODE_RGB}
        else:
            ctx.upload_particles(pos[:, 0], pos[:, 1], pos[:, 2], h, m)
            ctx.upload_quantity(q)
            kw = {}
        ctx.render(M, sf, [0], [n // 2], clear=True, **kw)
        if tiled_in_between:
            first = ctx.read_image()
            ctx.tile_periodic(off, w)
            assert same_bits(ctx.read_image(), oracle_np.periodic_tile(first, off, w))
        ctx.render(M, sf, [n // 2], [n - n // 2], clear=False, **kw)
        images.append(ctx.read_image())
        if tiled_in_between:
            ctx.tile_periodic(off, w)
            assert same_bits(ctx.read_image(), oracle_np.periodic_tile(images[0], off, w))
        ctx.close()
    assert images[0].shape[2] == (4 if mode == "rgb" else 2) and (images[0][..., 0] > 0).any()
    assert np.allclose(images[0], images[1], rtol=1e-5, atol=1e-30)


# ================================================================================================ colormaps
def value_image(H, W, C, seed):
    """exp(U(-90, 80)) with a second channel of either sign and a sprinkling of 0, negative, inf, denormal and NaN pixels"""
    rs = np.random.RandomState(seed)
    img = np.exp(rs.uniform(-90, 80, size=(H, W, C))).astype(f32)
    img[..., 1] = (rs.normal(size=(H, W)) * img[..., 0]).astype(f32)
    flat = img.reshape(-1, C)
    for k, s in enumerate([0.0, -1.0, np.inf, 1e-42, np.nan, -0.0]):
        flat[k::17, k % C] = f32(s)
    return img


def subset(img, out, n=64, seed=0):
    """the same n seeded pixels of an image and of its mapped output, as (8, n / 8, .) arrays"""
    idx = np.random.RandomState(seed).randint(0, img.shape[0] * img.shape[1], size=n)
    return img.reshape(-1, img.shape[2])[idx].reshape(8, -1, img.shape[2]), out.reshape(-1, out.shape[2])[idx].reshape(8, -1, out.shape[2])


def random_lut(n, seed):
    rs = np.random.RandomState(seed)
    lut = rs.uniform(-0.3, 1.3, size=(n, 4)).astype(f32)          # entries outside [0, 1] ...
    lut[rs.randint(0, n), rs.randint(0, 4)] = np.nan               # ... and one that is no number
    return lut


def random_lut2d(n, seed):
    rs = np.random.RandomState(seed)
    lut = rs.uniform(-0.3, 1.3, size=(n, n, 4)).astype(f32)
    lut[rs.randint(0, n), rs.randint(0, n), rs.randint(0, 4)] = np.nan
    return lut


SHAPES = [(1, 1), (1, 257), (255, 3), (480, 640)]
SCALAR_PARAMS = [(True, False, -30.0, 30.0), (False, False, 0.0, 1.0), (True, True, -3.0, 1.0), (False, True, -2.0, 2.0)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_image_colormaps_at_every_shape(native, shape):
    from oracle import oracle_c, oracle_np
    H, W = shape
    ctx = native.Context(16, 2)
    lut, lut2d = random_lut(1000, 1), random_lut2d(7, 2)
    ctx.colormap_set_lut2d(lut2d)
    for C in (2, 3, 4):
        img = value_image(H, W, C, seed=H + W + C)
        for log, weighted, vmin, vmax in SCALAR_PARAMS:
            got = ctx.colormap_scalar_host(img, lut, vmin, vmax, log, weighted)
            assert np.array_equal(got, oracle_c.colormap_scalar(img, lut, vmin, vmax, log, weighted)), ("scalar", C, log, weighted)
            si, so = subset(img, got)
            assert np.array_equal(so, oracle_np.colormap_scalar(si, lut, vmin, vmax, log, weighted)), ("scalar/np", C, log, weighted)
            got = ctx.colormap_bivariate_host(img, vmin, vmax, -20.0, 25.0, log, weighted)
            assert np.array_equal(got, oracle_c.colormap_bivariate(img, lut2d, vmin, vmax, -20.0, 25.0, log, weighted)), ("bivariate", C, log, weighted)
            si, so = subset(img, got)
            assert np.array_equal(so, oracle_np.colormap_bivariate(si, lut2d, vmin, vmax, -20.0, 25.0, log, weighted)), ("bivariate/np", C)
    for C in (3, 4, 5):
        img = value_image(H, W, C, seed=H + W + C + 100)
        img[..., 1] = np.abs(img[..., 1])
        for gamma in (1.0, 2.2):
            got = ctx.colormap_rgb_host(img, -20.0, 10.0, gamma)
            assert np.array_equal(got, oracle_c.colormap_rgb(img, -20.0, 10.0, gamma)), ("rgb", C, gamma)
            si, so = subset(img, got)
            assert np.array_equal(so, oracle_np.colormap_rgb(si, -20.0, 10.0, gamma)), ("rgb/np", C, gamma)
            gf = ctx.colormap_rgb_host(img, -20.0, 10.0, gamma, as_float=True)
            assert np.array_equal(gf, oracle_c.colormap_rgb(img, -20.0, 10.0, gamma, as_float=True), equal_nan=True), ("rgb float", C, gamma)
    ctx.close()


def test_host_image_colormaps_refuse_bad_shapes(native):
    ctx = native.Context(16, 2)
    lut = random_lut(16, 1)
    ctx.colormap_set_lut2d(random_lut2d(4, 1))
    with pytest.raises(native.BackendError, match=EINVAL):
        ctx.colormap_scalar_host(np.ones((4, 4, 1), dtype=f32), lut, 0.0, 1.0, False, False)
    with pytest.raises(native.BackendError, match=EINVAL):
        ctx.colormap_bivariate_host(np.ones((4, 4, 1), dtype=f32), 0.0, 1.0, 0.0, 1.0, False, False)
    with pytest.raises(native.BackendError, match=EINVAL):
        ctx.colormap_rgb_host(np.ones((4, 4, 2), dtype=f32), 0.0, 1.0, 1.0)
    # H = 0: an empty array has no usable address, so the C entry points are called with a real buffer and H = 0
    lib = native.load_library()
    fp, u8p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint8)
    buf, out = np.ones(64, dtype=f32), np.full(64, 7, dtype=np.uint8)
    b, o, lp = buf.ctypes.data_as(fp), out.ctypes.data_as(u8p), lut.ctypes.data_as(fp)
    assert lib.tsp_colormap_scalar_host(ctx._h, b, 0, 4, 2, lp, 16, 0.0, 1.0, 0, 0, o) == -1
    assert lib.tsp_colormap_scalar_host(ctx._h, b, 4, 0, 2, lp, 16, 0.0, 1.0, 0, 0, o) == -1
    assert lib.tsp_colormap_bivariate_host(ctx._h, b, 0, 4, 2, 0.0, 1.0, 0.0, 1.0, 0, 0, o) == -1
    assert lib.tsp_colormap_rgb_host(ctx._h, b, 0, 4, 3, 0.0, 1.0, 1.0, o, None) == -1
    assert (out == 7).all()
    ctx.close()


def special_value_image(R, golden_seed=0):
    """the special-value image of test_gpu_parity.test_colormap_bit_exact"""
    rs = np.random.RandomState(golden_seed)
    sp = np.zeros((R, R, 2), dtype=f32)
    sp[..., 0] = np.exp(rs.uniform(-90, 80, size=(R, R)))
    sp[..., 1] = rs.normal(size=(R, R)) * sp[..., 0]
    sp[0, :50] = 0.0
    sp[1, :50, 0] = -1.0
    sp[2, :50, 0] = np.inf
    sp[3, :50, 0] = 1e-42
    sp[4, :50] = np.nan
    return sp


def test_bivariate_map_on_special_values(native):
    from oracle import oracle_c, oracle_np
    R = 200
    sp = special_value_image(R)
    lut2d = random_lut2d(1000, 4)
    for channels in (2, 4):                       # the resident image read with a stride of 2 and of 4 floats
        ctx = native.Context(R, channels)
        img = sp if channels == 2 else np.concatenate([sp, sp[..., ::-1]], axis=-1)
        ctx.write_image(img)
        ctx.colormap_set_lut2d(lut2d)
        for log in (True, False):
            for weighted in (True, False):
                vmin, vmax = (-3.0, 1.0) if log else (-2.0, 2.0)
                want = oracle_c.colormap_bivariate(img, lut2d, vmin, vmax, -30.0, 30.0, log, weighted)
                assert np.array_equal(ctx.colormap_bivariate(vmin, vmax, -30.0, 30.0, log, weighted), want), (channels, log, weighted)
                assert np.array_equal(ctx.colormap_bivariate_host(img, vmin, vmax, -30.0, 30.0, log, weighted), want), (channels, log, weighted)
                si, so = subset(img, want)
                assert np.array_equal(so, oracle_np.colormap_bivariate(si, lut2d, vmin, vmax, -30.0, 30.0, log, weighted))
                lut = random_lut(1000, 9)
                want = oracle_c.colormap_scalar(img, lut, vmin, vmax, log, weighted)
                assert np.array_equal(ctx.colormap_scalar(lut, vmin, vmax, log, weighted), want), ("scalar", channels, log, weighted)
        ctx.close()


def test_lut_sizes(native):
    from oracle import oracle_c, oracle_np
    R = 64
    ctx = native.Context(R, 2)
    img = value_image(R, R, 2, seed=21)
    ctx.write_image(img)
    with pytest.raises(native.BackendError, match=ESTATE):          # no 2-D LUT yet
        ctx.colormap_bivariate(0.0, 1.0, 0.0, 1.0, False, False)
    with pytest.raises(native.BackendError, match=ESTATE):
        ctx.colormap_bivariate_host(img, 0.0, 1.0, 0.0, 1.0, False, False)
    for n in (2, 3, 1000, 65536, 3, 2):                             # (and smaller again: the device buffer is reused)
        lut = random_lut(n, n)
        for log, weighted, vmin, vmax in SCALAR_PARAMS:
            want = oracle_c.colormap_scalar(img, lut, vmin, vmax, log, weighted)
            assert np.array_equal(ctx.colormap_scalar(lut, vmin, vmax, log, weighted), want), (n, log, weighted)
            assert np.array_equal(ctx.colormap_scalar_host(img, lut, vmin, vmax, log, weighted), want), (n, log, weighted)
            si, so = subset(img, want)
            assert np.array_equal(so, oracle_np.colormap_scalar(si, lut, vmin, vmax, log, weighted)), (n, log, weighted)
    for n in (1, 65537):
        with pytest.raises(native.BackendError, match=EINVAL):
            ctx.colormap_scalar(np.zeros((n, 4), dtype=f32), 0.0, 1.0, False, False)
        with pytest.raises(native.BackendError, match=EINVAL):
            ctx.colormap_scalar_host(img, np.zeros((n, 4), dtype=f32), 0.0, 1.0, False, False)
    for n in (7, 1000, 2, 7):                                       # re-upload with another n on the same context
        lut2d = random_lut2d(n, n)
        ctx.colormap_set_lut2d(lut2d)
        for log, weighted, vmin, vmax in SCALAR_PARAMS:
            want = oracle_c.colormap_bivariate(img, lut2d, vmin, vmax, -25.0, 25.0, log, weighted)
            assert np.array_equal(ctx.colormap_bivariate(vmin, vmax, -25.0, 25.0, log, weighted), want), (n, log, weighted)
            assert np.array_equal(ctx.colormap_bivariate_host(img, vmin, vmax, -25.0, 25.0, log, weighted), want), (n, log, weighted)
            si, so = subset(img, want)
            assert np.array_equal(so, oracle_np.colormap_bivariate(si, lut2d, vmin, vmax, -25.0, 25.0, log, weighted)), (n, log, weighted)
    with pytest.raises(native.BackendError, match=EINVAL):
        ctx.colormap_set_lut2d(np.zeros((1, 1, 4), dtype=f32))
    small = np.zeros(64, dtype=f32)                                  # n = 4097 is refused before the table is read
    assert native.load_library().tsp_colormap_set_lut2d(ctx._h, small.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 4097) == -1
    lut2d = random_lut2d(7, 7)                                       # the refused uploads left the last LUT in place
    assert np.array_equal(ctx.colormap_bivariate(-3.0, 1.0, -25.0, 25.0, True, True),
                          oracle_c.colormap_bivariate(img, lut2d, -3.0, 1.0, -25.0, 25.0, True, True))
    ctx.close()


RANGES = [(0.5, 0.5), (-2.0, -2.0), (1.0, -1.0), (-3.0, np.inf), (-np.inf, 3.0), (np.nan, 1.0), (0.0, np.nan)]


def test_colormap_parameters_at_their_edges(native):
    """vmin == vmax (every pixel divides by zero), vmin > vmax, infinite and NaN limits; the rgb map's gamma at 0, below 0 and
    around 1 with pixels 0, inf and NaN"""
    from oracle import oracle_c, oracle_np
    R = 64
    img = value_image(R, R, 2, seed=33)
    img[5, :, 0] = 10.0 ** 0.5                  # pixels exactly at a limit
    img[6, :, 0] = 0.5
    lut, lut2d = random_lut(1000, 3), random_lut2d(16, 3)
    ctx = native.Context(R, 2)
    ctx.write_image(img)
    ctx.colormap_set_lut2d(lut2d)
    for vmin, vmax in RANGES:
        for log in (True, False):
            for weighted in (True, False):
                want = oracle_c.colormap_scalar(img, lut, vmin, vmax, log, weighted)
                assert np.array_equal(ctx.colormap_scalar(lut, vmin, vmax, log, weighted), want), ("scalar", vmin, vmax, log, weighted)
                assert np.array_equal(ctx.colormap_scalar_host(img, lut, vmin, vmax, log, weighted), want), ("scalar host", vmin, vmax)
                si, so = subset(img, want)
                assert np.array_equal(so, oracle_np.colormap_scalar(si, lut, vmin, vmax, log, weighted)), ("scalar/np", vmin, vmax, log, weighted)
                for dvmin, dvmax in ((-25.0, 25.0), (vmin, vmax)):
                    want = oracle_c.colormap_bivariate(img, lut2d, vmin, vmax, dvmin, dvmax, log, weighted)
                    assert np.array_equal(ctx.colormap_bivariate(vmin, vmax, dvmin, dvmax, log, weighted), want), ("bivariate", vmin, vmax, dvmin)
                    si, so = subset(img, want)
                    assert np.array_equal(so, oracle_np.colormap_bivariate(si, lut2d, vmin, vmax, dvmin, dvmax, log, weighted)), ("bivariate/np", vmin, vmax)
    ctx.close()
    rs = np.random.RandomState(34)
    rgb4 = np.zeros((R, R, 4), dtype=f32)
    rgb4[..., :3] = np.exp(rs.uniform(-20, 5, size=(R, R, 3)))
    rgb4[0, :20, :3] = 0.0
    rgb4[1, :20, 0] = np.nan
    rgb4[2, :20, 1] = np.inf
    rgb4[3, :20, 2] = -1.0
    rgb4[4, :20, 0] = 1e-42
    rgb4[5, :, :3] = f32(1e-6)                  # exactly vmin: x = 0
    ctx = native.Context(R, 4)
    ctx.write_image(rgb4)
    for vmin, vmax in [(-6.0, -1.0)] + RANGES:
        for gamma in (0.0, 0.5, 1.0, 2.2, -1.0):
            want = oracle_c.colormap_rgb(rgb4, vmin, vmax, gamma)
            assert np.array_equal(ctx.colormap_rgb(vmin, vmax, gamma), want), ("rgb", vmin, vmax, gamma)
            assert np.array_equal(ctx.colormap_rgb_host(rgb4, vmin, vmax, gamma), want), ("rgb host", vmin, vmax, gamma)
            wf = oracle_c.colormap_rgb(rgb4, vmin, vmax, gamma, as_float=True)
            assert np.array_equal(ctx.colormap_rgb(vmin, vmax, gamma, as_float=True), wf, equal_nan=True), ("rgb float", vmin, vmax, gamma)
            assert np.array_equal(ctx.colormap_rgb_host(rgb4, vmin, vmax, gamma, as_float=True), wf, equal_nan=True), ("rgb float host", vmin, vmax, gamma)
            si, so = subset(rgb4, want)
            assert np.array_equal(so, oracle_np.colormap_rgb(si, vmin, vmax, gamma)), ("rgb/np", vmin, vmax, gamma)
            si, so = subset(rgb4, wf)
            assert np.array_equal(so, oracle_np.colormap_rgb(si, vmin, vmax, gamma, as_float=True), equal_nan=True), ("rgb float/np", vmin, vmax, gamma)
    ctx.close()
