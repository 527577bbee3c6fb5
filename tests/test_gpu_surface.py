"""Surface rendering on the GPU: the occlusion pass, the density cut, the bilateral filter and the shading equal the numpy
restatement (tests/surface_ref.py) bit for bit, on the reference's known-answer scene and on adversarial ones; blocks drawn in any
split give the same image; the error cases and the isolation from the density path."""
import numpy as np
import pytest

import surface_ref
from conftest import make_cloud
from oracle import oracle_c, oracle_np

pytestmark = pytest.mark.gpu

SPHERE = surface_ref.sphere_mips()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def context(R, n_channels=2):
    from topsy_amd import _native, kernel_lut
    ctx = _native.Context(R, n_channels)
    ctx.set_kernel_mips(kernel_lut.kernel_mips())
    ctx.set_sphere_mips(kernel_lut.sphere_mips())
    return ctx


def camera(scale, rot=None):
    return oracle_np.transform_matrix(np.eye(3) if rot is None else rot, np.zeros(3), scale)


def scene(kind, n=1500, seed=0):
    """(pos (n, 3), h, m, q) of one adversarial scene."""
    pos, h, m, q, _ = make_cloud(n, seed=seed)
    if kind == "wide":          # a few footprints wider than the image
        h[:5] = np.float32(400.0)
    elif kind == "ties":        # cz = 0 and 1 exactly (the depth clamp makes equal dc) and duplicated particles
        pos[: n // 4, 2] = np.float32(50.0)          # cz = 1 at scale 50
        pos[n // 4: n // 2, 2] = np.float32(-50.0)   # cz = 0
        pos[n // 2: n // 2 + 200] = pos[:200]
        h[n // 2: n // 2 + 200] = h[:200]
        m[n // 2: n // 2 + 200] = m[:200]
    elif kind == "nonfinite":
        pos[::37, 0] = np.nan
        pos[5::41, 2] = np.inf
        h[::43] = np.inf
        h[3::47] = np.nan
        h[7::53] = 0.0
        m[::59] = np.nan
        m[2::61] = np.inf
        m[4::67] = -1.0
        q[::7] = np.nan
        q[1::11] = np.inf
    return pos, h, m, q


def device_raw(ctx, pos, h, m, q, M, sf, cut, starts=None, lens=None):
    ctx.upload_particles(pos[:, 0], pos[:, 1], pos[:, 2], h, m)
    ctx.upload_quantity(q)
    ctx.render_surface(M, sf, cut, starts, lens)
    return ctx.read_image()


def ref_raw(pos, h, m, q, M, sf, R, cut):
    ps = np.column_stack([pos, h]).astype(np.float32)
    return surface_ref.occlusion(ps, m, q, M, sf, R, cut, SPHERE)


@pytest.mark.parametrize("kind,R,percentile", [("cloud", 64, 50.0), ("cloud", 200, 0.0), ("wide", 333, 50.0),
                                               ("ties", 200, 0.0), ("nonfinite", 200, 50.0), ("cloud", 1024, 50.0),
                                               ("cloud", 200, 100.0)])
def test_occlusion_bit_identical(kind, R, percentile):
    pos, h, m, q = scene(kind)
    M, sf = camera(50.0)
    cut = surface_ref.cut_for_percentile(surface_ref.density_cuts(m, h), percentile)
    if kind == "nonfinite":
        assert np.isnan(cut)                                 # a NaN rho makes every cut NaN, as in numpy: nothing is drawn
        with np.errstate(all="ignore"):
            ok = ~np.isnan(m / ((h * h) * h))
        cut = surface_ref.cut_for_percentile(surface_ref.density_cuts(m[ok], h[ok]), percentile)
    ctx = context(R)
    try:
        idx = np.arange(len(h), dtype=np.float32)           # winner indices through the quantity channel
        got_idx = device_raw(ctx, pos, h, m, idx, M, sf, cut)
        got = device_raw(ctx, pos, h, m, q, M, sf, cut)
    finally:
        ctx.close()
    want, winner = ref_raw(pos, h, m, q, M, sf, R, cut)
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(np.where(winner >= 0, winner, 0), got_idx[..., 0].astype(np.int64))
    if percentile == 100.0:
        assert not want.any()
    else:
        assert (winner >= 0).sum() > 50


def test_every_footprint_class_is_drawn():
    """Sub-pixel to wider than the image: every mip, the bilinear rule, and the wave-wide path of the draw."""
    R = 256
    pos, h, m, q = scene("cloud", n=800, seed=4)
    h = np.geomspace(0.01, 300.0, len(h)).astype(np.float32)
    M, sf = camera(60.0)
    P = (np.float32(sf) * h) * np.float32(2.0) * np.float32(R)
    assert (P < 11).any() and ((P > 12) & (P < 22)).any() and ((P > 46) & (P < 64)).any() and (P > R).any()
    ctx = context(R)
    try:
        got = device_raw(ctx, pos, h, m, q, M, sf, -np.inf)
    finally:
        ctx.close()
    want, _ = ref_raw(pos, h, m, q, M, sf, R, -np.inf)
    assert np.array_equal(bits(got), bits(want))


def test_blocks_in_any_split_equal_one_call():
    R = 200
    pos, h, m, q = scene("ties", n=3000, seed=2)
    M, sf = camera(50.0)
    ctx = context(R)
    try:
        whole = device_raw(ctx, pos, h, m, q, M, sf, 0.0)
        cuts = np.sort(np.random.RandomState(5).choice(np.arange(1, len(h)), 9, replace=False))
        bounds = np.concatenate([[0], cuts, [len(h)]])
        blocks = [(a, b - a) for a, b in zip(bounds[:-1], bounds[1:])]
        order = np.random.RandomState(6).permutation(len(blocks))
        for k, b in enumerate(order):
            ctx.render_surface(M, sf, 0.0, [blocks[b][0]], [blocks[b][1]], clear=(k == 0))
        split = ctx.read_image()
        # several ranges in one call
        ctx.render_surface(M, sf, 0.0, [b[0] for b in blocks[::-1]], [b[1] for b in blocks[::-1]])
        multi = ctx.read_image()
    finally:
        ctx.close()
    assert np.array_equal(bits(split), bits(whole)) and np.array_equal(bits(multi), bits(whole))


@pytest.mark.parametrize("n", [1, 1000, 1000000])
def test_order_statistics_equal_np_quantile(n):
    from topsy_amd.colormap.implementation import quantile_from_order_statistics
    rs = np.random.RandomState(n)
    pos = rs.normal(size=(n, 3)).astype(np.float32)
    h = rs.lognormal(size=n).astype(np.float32)
    m = rs.uniform(0.1, 2.0, size=n).astype(np.float32)
    ctx = context(16)
    try:
        ctx.upload_particles(pos[:, 0], pos[:, 1], pos[:, 2], h, m)
        ranks = np.unique(np.linspace(0, n - 1, 77).astype(np.int64))
        got = ctx.density_order_stats(ranks)
        q = quantile_from_order_statistics(ctx.density_order_stats, n, np.linspace(0, 1, 101))
    finally:
        ctx.close()
    rho = m / ((h * h) * h)
    assert np.array_equal(got, np.sort(rho)[ranks])
    assert np.array_equal(q, surface_ref.density_cuts(m, h))


def test_order_statistics_with_nan_and_inf():
    from topsy_amd.colormap.implementation import quantile_from_order_statistics
    pos, h, m, q = scene("nonfinite", n=5000)
    ctx = context(16)
    try:
        ctx.upload_particles(pos[:, 0], pos[:, 1], pos[:, 2], h, m)
        with np.errstate(all="ignore"):
            rho = m / ((h * h) * h)
            srt = np.sort(rho)
            got = ctx.density_order_stats(np.arange(len(h)))
            qs = quantile_from_order_statistics(ctx.density_order_stats, len(h), np.linspace(0, 1, 101))
    finally:
        ctx.close()
    assert np.array_equal(got, srt, equal_nan=True)
    assert np.isnan(qs).all() and np.isnan(surface_ref.density_cuts(m, h)).all()


def test_order_statistics_of_a_device_synthetic_set():
    import topsy_amd
    vis = topsy_amd.synthetic_on_device(int(1e7), render_resolution=64)
    try:
        from topsy_amd import sph
        occ = sph.DepthSPHWithOcclusion(vis, 64)
        d = vis.particle_buffers.context.download_particles(("h", "mass"))
        assert np.array_equal(occ._percentile_to_den_cut, surface_ref.density_cuts(d["mass"], d["h"]))
        assert occ.get_density_cut_percentile() == 50.0 and occ.get_density_cut_percentile_range() == (0.0, 100.0)
    finally:
        vis.close()


@pytest.mark.parametrize("R,scale", [(64, 1e-6), (64, 0.01), (96, 0.1), (130, 0.2), (200, 0.01)])
def test_filter_bit_identical(R, scale):
    rs = np.random.RandomState(R)
    img = np.zeros((R, R, 2), dtype=np.float32)
    img[..., 0] = rs.normal(size=(R, R))
    img[..., 1] = rs.uniform(0.2, 0.9, size=(R, R))
    img[: R // 3, : R // 4, 1] = 0.0                          # empty corner: an edge of the surface
    img[R // 2:, :, 1] += np.linspace(0, 0.05, R, dtype=np.float32)
    img[-1, :, 1] = 1.2                                       # the clamp at the image edges
    ctx = context(R)
    try:
        ctx.write_image(img)
        got, _ = ctx.surface_present(smoothing_scale=scale, content=True, rgba=False)
    finally:
        ctx.close()
    want = surface_ref.bilateral(img, scale)
    assert np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("opts", [{}, {"weighted_average": True, "log": False, "vmin": -1.0, "vmax": 2.0},
                                  {"weighted_average": True, "log": True, "vmin": -2.0, "vmax": 0.5},
                                  {"depth_scale": 1.7, "light_direction": [0.3, -0.4, 0.866], "light_color": [0.9, 0.5, 0.2],
                                   "ambient_color": [0.1, 0.2, 0.3]}])
def test_shading_bit_identical(opts):
    from topsy_amd.colormap.implementation import _lut_from_matplotlib
    R = 120
    rs = np.random.RandomState(9)
    img = np.zeros((R, R, 2), dtype=np.float32)
    img[..., 0] = rs.lognormal(size=(R, R)) * np.where(rs.uniform(size=(R, R)) < 0.1, -1, 1)
    img[::17, ::13, 0] = np.nan
    yy, xx = np.mgrid[0:R, 0:R]
    img[..., 1] = np.clip(0.8 - ((xx - 60.0) ** 2 + (yy - 50.0) ** 2) / 4000.0, 0, None)
    lut = _lut_from_matplotlib("twilight_shifted", 1000)
    params = dict(surface_ref.DEFAULT_PARAMS) | {"smoothing_scale": 0.02} | opts
    ctx = context(R)
    try:
        ctx.write_image(img)
        filt, rgba = ctx.surface_present(lut_rgba=lut, **params)
    finally:
        ctx.close()
    want_f = surface_ref.bilateral(img, params["smoothing_scale"])
    assert np.array_equal(bits(filt), bits(want_f))
    shade_args = {k: v for k, v in params.items() if k != "smoothing_scale"}
    want = surface_ref.shade(want_f, lut=lut, **shade_args)
    assert np.array_equal(rgba, want)
    assert (rgba[..., 3] == 255).all() and len(np.unique(rgba[..., :3])) > 20


@pytest.fixture(scope="module")
def kat_view():
    import topsy_amd
    from topsy_amd.drawreason import DrawReason
    vis = topsy_amd.test(int(1e5), render_resolution=200)
    vis.quantity_name = "test-quantity"
    vis.scale = 30.0
    vis.rotate(0.0, 1.0)
    vis.render_sph(DrawReason.EXPORT)
    sv = topsy_amd.SurfaceView(vis)
    yield vis, sv
    vis.close()


def test_surface_view_meets_the_reference_kats(kat_view, golden):
    vis, sv = kat_view
    result = sv.get_sph_image()
    pres = sv.get_sph_presentation_image()
    assert result.shape == (200, 200, 2) and result.dtype == np.float32
    assert pres.shape == (200, 200, 4) and pres.dtype == np.uint8
    kats = golden["surface_kats.npz"]
    keep = np.ones(100, dtype=bool)
    keep[67] = False
    np.testing.assert_allclose(result[::20, ::20, 0].ravel()[keep], kats["quantity"][keep], rtol=1e-3)
    np.testing.assert_allclose(result[::20, ::20, 1].ravel(), kats["depth"], rtol=1e-3)
    np.testing.assert_allclose(pres[::20, ::20].ravel().astype(int), kats["presentation"].astype(int), atol=30)


def test_surface_view_equals_the_restatement(kat_view):
    vis, sv = kat_view
    ctx = vis.particle_buffers.context
    raw = sv.get_raw_image()
    d = ctx.download_particles(("x", "y", "z", "h", "mass", "q"))
    cuts = surface_ref.density_cuts(d["mass"], d["h"])
    assert np.array_equal(sv._sph._percentile_to_den_cut, cuts)
    cut = surface_ref.cut_for_percentile(cuts, sv.density_cut_percentile)
    assert sv._sph.density_cut() == cut
    M, sf = sv._sph._get_transform_params()
    ps = np.column_stack([d["x"], d["y"], d["z"], d["h"]])
    want_raw, _ = surface_ref.occlusion(ps, d["mass"], d["q"], M, sf, 200, cut, SPHERE)
    assert np.array_equal(bits(raw), bits(want_raw))
    want_f = surface_ref.bilateral(want_raw, 0.01)
    assert np.array_equal(bits(sv.get_sph_image()), bits(want_f))
    sv["vmin"] = sv["vmax"] = None
    pres = sv.get_sph_presentation_image()
    vmin, vmax, log = surface_ref.autorange(want_raw)
    assert (sv["vmin"], sv["vmax"], sv["log"]) == (vmin, vmax, log)
    want = surface_ref.shade(want_f, weighted_average=True, log=log, vmin=vmin, vmax=vmax, lut=sv.colormap._lut)
    assert np.array_equal(pres, want)
    # a new cut percentile draws fewer spheres; the camera and quantity stay the visualizer's
    sv.density_cut_percentile = 90.0
    assert (sv.get_raw_image()[..., 1] > 0).sum() < (raw[..., 1] > 0).sum()
    sv.density_cut_percentile = 50.0


def test_errors_and_isolation_from_the_density_path():
    from topsy_amd import _native, kernel_lut
    R = 64
    pos, h, m, q = scene("cloud", n=500)
    M, sf = camera(50.0)
    ctx = _native.Context(R, 4)
    try:
        ctx.set_kernel_mips(kernel_lut.kernel_mips())
        ctx.upload_particles(pos[:, 0], pos[:, 1], pos[:, 2], h, m)
        ctx.upload_quantity(q)
        with pytest.raises(_native.BackendError, match="error -4"):      # no sphere texture yet
            ctx.render_surface(M, sf, 0.0)
        ctx.set_sphere_mips(kernel_lut.sphere_mips())
        with pytest.raises(_native.BackendError, match="error -1"):
            ctx.set_sphere_mips(kernel_lut.sphere_mips()[:1024], 32, 4)
        ctx.render(M, sf)
        with pytest.raises(_native.BackendError, match="error -4"):      # clear = 0 onto a density image
            ctx.render_surface(M, sf, 0.0, clear=False)
        ctx.render_surface(M, sf, 0.0)
        with pytest.raises(_native.BackendError, match="error -4"):      # density clear = 0 onto surface keys
            ctx.render(M, sf, clear=False)
        with pytest.raises(_native.BackendError, match="error -1"):
            ctx.density_order_stats([len(h)])
        with pytest.raises(_native.BackendError, match="error -1"):
            ctx.surface_present(smoothing_scale=float("nan"))
        with pytest.raises(_native.BackendError, match="error -1"):
            ctx.surface_present(weighted_average=True, lut_rgba=np.zeros((1, 4), np.float32))
        # the density path after a surface render (clear = 1) matches the oracle
        ctx.render(M, sf)
        got = ctx.read_image()
        x, y, z = (np.ascontiguousarray(pos[:, k]) for k in range(3))
        want, _ = oracle_c.splat(x, y, z, h, m, q, mode=0, M=M, sf=sf, R=R, mips=kernel_lut.kernel_mips())
        assert np.allclose(got[..., 0], want[..., 0], rtol=1e-5, atol=0)
        ctx.write_image(np.zeros((R, R, 4), np.float32))
        with pytest.raises(_native.BackendError, match="error -1"):      # presentation needs the 2-channel layout
            ctx.surface_present()
        ctx.upload_particles(pos[:, 0], pos[:, 1], pos[:, 2], h)          # no mass
        with pytest.raises(_native.BackendError, match="error -1"):
            ctx.render_surface(M, sf, 0.0)
        with pytest.raises(_native.BackendError, match="error -1"):
            ctx.density_order_stats([0])
    finally:
        ctx.close()
