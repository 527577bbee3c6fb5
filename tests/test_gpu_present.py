"""Frame composition on the GPU (tsp_present, VisualizerBase.get_presentation_image): every frame equals the numpy restatement
(tests/present_ref.py) bit for bit, given the same float image and the same host textures -- at W = H = R with no layers it is
get_sph_presentation_image itself; canvases of every shape; each layer alone, all together, the cube and crosshairs of a rotated
periodic view; overlapping semi-transparent primitives; the error cases and what they leave alone; two GPUs."""
import ctypes

import numpy as np
import pytest

import present_ref
import topsy_amd
from topsy_amd import _native, overlays

pytestmark = pytest.mark.gpu

f32 = np.float32


def same(a, b):
    if a.dtype == np.float16:
        return a.shape == b.shape and np.array_equal(a.view(np.uint16), b.view(np.uint16))
    return a.dtype == b.dtype and np.array_equal(a, b)


def reference_frame(vis, W, H):
    """present_ref on what the last get_presentation_image call was composed from."""
    base, layers = vis._last_presentation
    base = dict(base)
    if base["map"] == "bivariate":
        base["lut2d"] = vis.colormap._impl._lut
    return present_ref.compose(vis._sph._context.read_image(), W, H, base, layers)


def no_layers(vis):
    vis.show_colorbar = vis.show_scalebar = vis.show_status = False
    vis.crosshairs_visible = False


@pytest.fixture(scope="module")
def vis512():
    v = topsy_amd.test(3000, render_resolution=512)
    v.quantity_name = "test-quantity"
    yield v
    v.close()


@pytest.mark.parametrize("mode, quantity", [("univariate", None), ("univariate", "test-quantity"), ("bivariate", "test-quantity"),
                                            ("rgb", None), ("rgb-hdr", None)])
def test_square_frame_without_layers_is_the_presentation_image(mode, quantity):
    R = 128
    v = topsy_amd.test(2000, render_resolution=R, render_mode=mode)
    try:
        if quantity:
            v.quantity_name = quantity
        no_layers(v)
        want = v.get_sph_presentation_image()
        got = v.get_presentation_image((R, R))
        assert got.shape == (R, R, 4) and same(got, want)
        assert same(got, reference_frame(v, R, R))
    finally:
        v.close()


@pytest.mark.parametrize("W, H", [(1920, 1080), (640, 480), (480, 640), (3000, 2000), (300, 200), (1, 1)])
def test_canvases_with_default_layers(vis512, W, H):
    vis512.show_colorbar = vis512.show_scalebar = vis512.show_status = True
    vis512.crosshairs_visible = False
    vis512.display_status("frame test", timeout=600)
    got = vis512.get_presentation_image((W, H))
    assert got.shape == (H, W, 4) and got.dtype == np.uint8
    assert same(got, reference_frame(vis512, W, H))


def test_1080p_frame_shows_colorbar_right_and_scale_bar_bottom_left(vis512):
    vis512.show_colorbar = vis512.show_scalebar = True
    vis512.show_status = False
    got = vis512.get_presentation_image((1920, 1080))
    bare = vis512._sph._context.present(1920, 1080, vis512._last_presentation[0], [])     # the same image without layers
    differs = (got != bare).any(axis=-1)
    cols = np.where(differs.any(axis=0))[0]
    bar_w = int(round(1080 * 0.2))
    assert differs[:, -bar_w:].mean() > 0.5                     # the colorbar's half-transparent panel covers the right edge
    assert differs[1080 - 60:, :200].any()                      # the bar and its label at the bottom left
    assert not differs[:900, 200:1920 - bar_w - 10].any()       # nothing else in the middle
    assert cols.min() < 200


@pytest.mark.parametrize("layer", ["colorbar", "scalebar", "status", "crosshairs"])
def test_each_layer_alone(vis512, layer):
    no_layers(vis512)
    setattr(vis512, {"colorbar": "show_colorbar", "scalebar": "show_scalebar", "status": "show_status",
                     "crosshairs": "crosshairs_visible"}[layer], True)
    vis512.display_status("layer test", timeout=600)
    got = vis512.get_presentation_image((800, 600))
    assert len(vis512._last_presentation[1]) == (2 if layer == "scalebar" else 1)
    assert same(got, reference_frame(vis512, 800, 600))


def test_all_layers_on_a_rotated_periodic_view():
    v = topsy_amd.test(3000, render_resolution=256, periodic_tiling=True)
    try:
        v.rotate(0.3, 0.5)
        v.scale = 80.0
        v.crosshairs_visible = True
        v.display_status("periodic", timeout=600)
        for W, H in [(1280, 720), (600, 900)]:
            got = v.get_presentation_image((W, H))
            kinds = [L["kind"] for L in v._last_presentation[1]]
            assert kinds == ["quad", "quad", "quad", "lines", "lines", "quad"]      # colorbar, label, bar, crosshairs, cube, status
            assert same(got, reference_frame(v, W, H))
    finally:
        v.close()


def overlapping_layers(rs):
    tex1 = rs.uniform(0, 1, size=(7, 5, 4)).astype(f32)
    tex1[..., 3] = rs.uniform(0.2, 0.8, size=(7, 5))
    tex2 = rs.uniform(0, 1, size=(3, 9, 4)).astype(f32)
    q1 = overlays.quad(tex1, (-0.7, -0.6, 1.1, 1.2))
    q1["offsets"] = np.array([[0, 0], [0.13, -0.21], [-0.31, 0.17]], dtype=f32)
    q1["weights"] = np.array([1.0, 0.7, 0.45], dtype=f32)
    q2 = overlays.quad(tex2, (-0.2, -0.3, 0.9, 0.8))
    q2["tex"] = (0.1, -0.2, 0.8, 1.5)
    ln = overlays.lines(rs.uniform(-1.2, 1.2, size=(9, 4)), rs.uniform(-1.2, 1.2, size=(9, 4)), (0.9, 0.3, 0.1, 0.35), 7.5,
                        rs.uniform(-1, 1, size=(4, 4)))
    ln["starts"][0] = ln["ends"][0]         # one zero-length segment
    return [q1, ln, q2, overlays.lines([[-1, -1, 0, 1]], [[1, 1, 0, 1]], (0.2, 0.9, 0.4, 0.6), 3.0)]


@pytest.mark.parametrize("W, H", [(333, 211), (64, 200)])
def test_overlapping_semi_transparent_primitives(W, H):
    rs = np.random.RandomState(5)
    ctx = _native.Context(96, 4)
    try:
        img = rs.uniform(0.0, 3.0, size=(96, 96, 4)).astype(f32)
        img[3, 5, 0] = np.nan
        ctx.write_image(img)
        layers = overlapping_layers(rs)
        lut = rs.uniform(0, 1, size=(50, 4)).astype(f32)
        bases = [{"map": "scalar", "lut": lut, "vmin": 0.1, "vmax": 2.5, "log": False, "weighted": True},
                 {"map": "rgb", "vmin": -1.0, "vmax": 0.5, "gamma": 0.8},
                 {"map": "rgb-hdr", "vmin": -1.0, "vmax": 0.2, "gamma": 1.3}]
        for base in bases:
            got = ctx.present(W, H, base, layers)
            want = present_ref.compose(img, W, H, base, layers)
            assert same(got, want), base["map"]
    finally:
        ctx.close()


def call_raw(ctx, W, H, base, layers, out):
    """tsp_present with ctypes structs built by hand, for the argument errors the Python wrapper would refuse first."""
    arr = (_native.PresentLayer * max(1, len(layers or ())))(*(layers or ()))
    return ctx._lib.tsp_present(ctx._h, W, H, None if base is None else ctypes.byref(base), arr if layers is not None else None,
                                0 if layers is None else len(layers), None if out is None else out.ctypes.data, None)


def test_errors_leave_everything_untouched():
    rs = np.random.RandomState(9)
    ctx = _native.Context(64, 2)
    try:
        img = rs.uniform(0.1, 2.0, size=(64, 64, 2)).astype(f32)
        ctx.write_image(img)
        lut = rs.uniform(0, 1, size=(16, 4)).astype(f32)
        good = {"map": "scalar", "lut": lut, "vmin": 0.0, "vmax": 2.0, "log": False, "weighted": False}
        want = present_ref.compose(img, 40, 30, good, [])
        b = _native.PresentBase()
        b.map, b.vmin, b.vmax, b.lut_rgba, b.n_lut = 0, 0.0, 2.0, lut.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 16
        tex = np.ones((2, 2, 4), dtype=f32)
        pts = np.zeros((1, 4), dtype=f32)
        one, zero2 = np.ones(1, dtype=f32), np.zeros(2, dtype=f32)
        fp = ctypes.POINTER(ctypes.c_float)

        def quad(**kw):
            L = _native.PresentLayer()
            L.kind, L.texture_rgba, L.tex_width, L.tex_height = 0, tex.ctypes.data_as(fp), 2, 2
            L.clip_extent[:], L.tex_extent[:] = [1.0, 1.0], [1.0, 1.0]
            L.n_instances, L.instance_offsets, L.instance_weights = 1, zero2.ctypes.data_as(fp), one.ctypes.data_as(fp)
            for k, v in kw.items():
                setattr(L, k, v)
            return L

        def line(**kw):
            L = _native.PresentLayer()
            L.kind, L.n_segments, L.starts, L.ends, L.width_px = 1, 1, pts.ctypes.data_as(fp), pts.ctypes.data_as(fp), 2.0
            for k, v in kw.items():
                setattr(L, k, v)
            return L

        nan_pts = np.full((1, 4), np.nan, dtype=f32)
        cases = [(0, 30, b, []), (40, 0, b, []), (16385, 30, b, []), (-3, 30, b, []), (40, 30, None, []),
                 (40, 30, b, [quad(kind=7)]), (40, 30, b, [quad(texture_rgba=None)]), (40, 30, b, [quad(tex_width=0)]),
                 (40, 30, b, [quad(n_instances=0)]), (40, 30, b, [quad(n_instances=129)]), (40, 30, b, [quad(instance_weights=None)]),
                 (40, 30, b, [quad(clip_extent=(ctypes.c_float * 2)(0.0, 1.0))]),
                 (40, 30, b, [quad(clip_origin=(ctypes.c_float * 2)(np.inf, 0.0))]),
                 (40, 30, b, [quad(tex_extent=(ctypes.c_float * 2)(2000.0, 1.0))]),
                 (40, 30, b, [line(n_segments=0)]), (40, 30, b, [line(starts=None)]), (40, 30, b, [line(width_px=-1.0)]),
                 (40, 30, b, [line(starts=nan_pts.ctypes.data_as(fp))])]
        for W, H, base, layers in cases:
            out = np.full((30, 40, 4), 77, dtype=np.uint8)
            assert call_raw(ctx, W, H, base, layers, out) == -1, (W, H, layers and layers[0].kind)
            assert np.all(out == 77)
            assert np.array_equal(ctx.read_image(), img)
            assert same(ctx.present(40, 30, good), want)
        assert call_raw(ctx, 40, 30, b, [], None) == -1             # no output buffer
        assert call_raw(ctx, 40, 30, b, None, np.empty((30, 40, 4), np.uint8)) == 0   # no layers, NULL list: fine
        b.n_lut = 1
        assert call_raw(ctx, 40, 30, b, [], np.empty((30, 40, 4), np.uint8)) == -1
        b.map = 2                                                   # rgb on a 2-channel image
        assert call_raw(ctx, 40, 30, b, [], np.empty((30, 40, 4), np.uint8)) == -1
        b.map = 1                                                   # bivariate before any 2-D LUT
        assert call_raw(ctx, 40, 30, b, [], np.empty((30, 40, 4), np.uint8)) == -4
        assert np.array_equal(ctx.read_image(), img)
        assert same(ctx.present(40, 30, good), want)
    finally:
        ctx.close()


def test_two_gpus_compose_on_the_root():
    if _native.device_count() < 2:
        pytest.skip("needs two visible GPUs")
    v = topsy_amd.test(5000, render_resolution=256, n_gpus=2)
    try:
        v.display_status("two gpus", timeout=600)
        got = v.get_presentation_image((640, 360))
        assert same(got, reference_frame(v, 640, 360))
        no_layers(v)
        assert same(v.get_presentation_image((256, 256)), v.get_sph_presentation_image())
    finally:
        v.close()
