"""Composed surface frames on the GPU (tsp_present_surface, tsp_present_surface_yuv420, SurfaceView.get_presentation_image and
its 4:2:0 form, a recorded path through the unmodified recorder): every frame equals the numpy restatement
(tests/surface_present_ref.py) byte for byte; at W = H = R without layers it is tsp_surface_present's image; the refusals leave
the image and the output alone."""
import ctypes
import time

import numpy as np
import pytest

import surface_present_ref
import surface_ref
import yuv420_ref
import topsy_amd
from test_gpu_present import overlapping_layers
from test_surface_present_cpu import SHADING_OPTIONS, Clock, shading_image, shading_params
from oracle import oracle_c
from topsy_amd import _native, kernel_lut
from topsy_amd.recorder import STATUS_TEXT, Interpolator, VisualizationRecorder

pytestmark = pytest.mark.gpu

f32 = np.float32
CANVASES = [(120, 120), (333, 211), (211, 333), (64, 40), (1, 1)]


def context(R, n_channels=2):
    ctx = _native.Context(R, n_channels)
    ctx.set_kernel_mips(kernel_lut.kernel_mips())
    ctx.set_sphere_mips(kernel_lut.sphere_mips())
    return ctx


def first_difference(got, want):
    bad = np.argwhere((got != want).any(axis=-1))
    return f"{len(bad)} pixels differ, first at (row, col) {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


def assert_same(got, want):
    assert got.dtype == want.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), first_difference(got, want)


# ---- write_image scenes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", SHADING_OPTIONS)
def test_frames_of_a_written_image_equal_the_restatement(opts):
    img = shading_image()
    params = shading_params(opts)
    layers = overlapping_layers(np.random.RandomState(5))
    ctx = context(120)
    try:
        ctx.write_image(img)
        _, shaded = ctx.surface_present(**params)
        for W, H in CANVASES:
            for ls in ([], layers):
                got = ctx.present_surface(W, H, params, ls)
                assert got.shape == (H, W, 4)
                assert_same(got, surface_present_ref.compose_surface(img, W, H, params, ls))
        assert_same(ctx.present_surface(120, 120, params), shaded)          # the identity at W = H = R
        assert np.array_equal(ctx.read_image().view(np.uint32), img.view(np.uint32))
    finally:
        ctx.close()


# ---- a real view ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    vis = topsy_amd.test(20000, render_resolution=512)
    vis.quantity_name = "test-quantity"
    vis.rotate(0.3, 0.8)
    view = topsy_amd.SurfaceView(vis)
    view.display_status(STATUS_TEXT, timeout=1e6)
    yield vis, view
    vis.close()


def restated(view, W, H):
    """surface_present_ref on what the last frame of the view was composed from."""
    params, layers = view._last_presentation
    return surface_present_ref.compose_surface(view.get_raw_image(), W, H, params, layers)


@pytest.mark.parametrize("W, H", [(1920, 1080), (480, 640), (300, 200), (512, 512)])
def test_view_frames_equal_the_restatement(scene, W, H):
    vis, view = scene
    view.show_colorbar = view.show_scalebar = view.show_status = True
    got = view.get_presentation_image((W, H))
    assert got.shape == (H, W, 4)
    params, layers = view._last_presentation
    assert [L["kind"] for L in layers] == ["quad", "quad", "quad", "quad"]      # colorbar, label, bar, status line
    assert params["weighted_average"] and np.isfinite([params["vmin"], params["vmax"]]).all()
    assert_same(got, restated(view, W, H))


def test_square_view_frame_without_layers_is_the_presentation_image(scene):
    vis, view = scene
    view.show_colorbar = view.show_scalebar = view.show_status = False
    try:
        got = view.get_presentation_image((512, 512))
        assert view._last_presentation[1] == []
        assert_same(got, view.get_sph_presentation_image())
    finally:
        view.show_colorbar = view.show_scalebar = view.show_status = True


def test_colorbar_only_changes_its_quad_and_needs_a_quantity(scene):
    vis, view = scene
    W, H = 1920, 1080
    view.show_scalebar = view.show_status = False
    try:
        with_bar = view.get_presentation_image((W, H))
        (bar,) = view._last_presentation[1]
        view.show_colorbar = False
        without = view.get_presentation_image((W, H))
        assert view._last_presentation[1] == []
        x0, _, w, _ = bar["clip"]
        first_col = int(np.floor((x0 + 1.0) * 0.5 * W)) - 1                  # the quad spans the full height at the right edge
        differs = (with_bar != without).any(axis=-1)
        assert differs.any() and not differs[:, :first_col].any()
        assert differs[:, first_col + 2:].mean() > 0.5
        assert w == pytest.approx(2.0 * H * bar["texture"].shape[1] / bar["texture"].shape[0] / W)
        # no quantity: the material is 1, and the reference draws no colorbar for such a surface map
        view.show_colorbar = True
        view.quantity_name = None
        plain = view.get_presentation_image((W, H))
        params, layers = view._last_presentation
        assert layers == [] and not params["weighted_average"]
        assert_same(plain, restated(view, W, H))
    finally:
        view.quantity_name = "test-quantity"
        view.show_colorbar = view.show_scalebar = view.show_status = True


# ---- 4:2:0 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W, H", [(1920, 1080), (2, 2)])
def test_planes_equal_the_restated_rgba_frame(scene, W, H):
    vis, view = scene
    planes = view.get_presentation_image_yuv420((W, H))
    params, layers = view._last_presentation
    rgba = view._sph._context.present_surface(W, H, params, layers)        # the RGBA frame of the same call arguments
    want = yuv420_ref.to_yuv420(rgba)
    assert [p.shape for p in planes] == [(H, W), (H // 2, W // 2), (H // 2, W // 2)]
    for got, w, name in zip(planes, want, "YUV"):
        assert got.dtype == np.uint8 and np.array_equal(got, w), name
    assert_same(rgba, restated(view, W, H))


def test_odd_sizes_raise(scene):
    vis, view = scene
    for size in [(63, 64), (64, 63), (1, 1)]:
        with pytest.raises(ValueError):
            view.get_presentation_image_yuv420(size)
    view.get_raw_image()
    with pytest.raises(_native.BackendError, match="error -1"):
        view._sph._context.present_surface_yuv420(63, 64, view.colormap.surface_parameters())
    for size in [(0, 10), (10, 16385)]:
        with pytest.raises(ValueError):
            view.get_presentation_image(size)


# ---- movie ----------------------------------------------------------------------------------------------------------
def visualizer_frame(vis):
    """get_sph_presentation_image() of the visualizer with its density render on the float64-atomic pipeline.  Two renders of one
    snapshot on the default pipeline are not bit-identical (its tile kernels sum float32 partial images in the order the
    atomics decide: tests/test_gpu_smoothing.py), so a frame taken before could not equal one taken after even with no view
    in between -- measured on this scene: six back-to-back frames of the visualizer alone differ from the first in 7 to 10
    pixels and about 2e5 float32 values on the default pipeline, in none on this one, whose float64 sums round to the same
    float32 image every time."""
    flags = vis._sph.pipeline_flags
    vis._sph.pipeline_flags = _native.PIPE_GENERIC
    try:
        return vis.get_sph_presentation_image()
    finally:
        vis._sph.pipeline_flags = flags


def test_a_recorded_path_replays_into_surface_frames(scene, tmp_path):
    vis, view = scene
    before = visualizer_frame(vis)
    state = (vis.rotation_matrix.copy(), vis.scale, np.array(vis.position_offset))
    view.display_status(STATUS_TEXT, timeout=1e6)     # the status line already shows the replay's text: no timing in the frames
    time.sleep(0.1)
    view.get_presentation_image((320, 180))
    clock = Clock()
    rec = VisualizationRecorder(view, clock=clock)
    try:
        rec.record()
        for k in range(3):
            clock.t += 0.5
            vis.rotate(0.2, -0.1)
            view.scale = view.scale * 0.85
            view.position_offset = view.position_offset + np.array([0.4, -0.2, 0.1])
            rec.mark()
        rec.stop()
        ends = rec._recording_ends_at
        assert ends == pytest.approx(1.5) and len(rec._timestream["scale"]) == 4
        assert rec._timestream["colormap[type]"][0][1] == "surface"
        frames = list(rec.frames(fps=4, resolution=(320, 180), pixel_format="yuv420p"))
        assert len(frames) == int(ends * 4)
        interps = [(p, c(rec._timestream[p])) for c, p in zip(rec._record_interpolation_class_smoothed, rec._record_properties)]
        for i, planes in enumerate(frames):
            for p, f in interps:
                value = f(i / 4)
                if value is Interpolator.no_value:
                    continue
                if p.startswith("colormap["):
                    view.colormap[p[9:-1]] = value
                else:
                    setattr(view, p, value)
            view.display_status(STATUS_TEXT, timeout=1e6)
            want = view.get_presentation_image_yuv420((320, 180))
            assert [a.shape for a in planes] == [(180, 320), (90, 160), (90, 160)]
            assert all(np.array_equal(a, b) for a, b in zip(planes, want)), i
        assert not np.array_equal(frames[0][0], frames[-1][0])
        assert len(rec._timestream["scale"]) == 4                            # replay frames are not recorded
        fn = tmp_path / "surface.y4m"
        rec.save_y4m(str(fn), 4, (320, 180))
        header = b"YUV4MPEG2 W320 H180 F4:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n"
        data = fn.read_bytes()
        size = 320 * 180 * 3 // 2
        assert data.startswith(header) and len(data) == len(header) + len(frames) * (6 + size)
        assert all(data[len(header) + i * (6 + size):][:6] == b"FRAME\n" for i in range(len(frames)))
    finally:
        view.remove_frame_listener(rec._on_frame)
        vis.rotation_matrix, vis.scale, vis.position_offset = state
    # the visualizer and the view share one device target: the visualizer's own image is what it was
    assert_same(visualizer_frame(vis), before)
    # and on its usual pipeline it is the colormap of its own density render, not of the view's (q, depth) image
    rgba = vis.get_sph_presentation_image()
    p = vis.colormap.get_parameters()
    img = vis._sph._context.read_image()[..., :2]
    assert (img[..., 0] > 0).mean() > 0.5                                    # a density image: the surface's depth is mostly 0
    assert_same(rgba, oracle_c.colormap_scalar(img, vis.colormap._impl._lut, f32(p["vmin"]), f32(p["vmax"]), p["log"],
                                               p["weighted_average"]))


# ---- errors ---------------------------------------------------------------------------------------------------------
def call_raw(ctx, W, H, p, layers, out, yuv=False):
    """The raw symbols with ctypes structs built by hand, for what the Python wrapper would refuse or convert first."""
    arr = (_native.PresentLayer * max(1, len(layers)))(*layers)
    fn = ctx._lib.tsp_present_surface_yuv420 if yuv else ctx._lib.tsp_present_surface
    return fn(ctx._h, W, H, ctypes.byref(p), arr, len(layers), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), None)


def test_errors_leave_everything_untouched():
    rs = np.random.RandomState(3)
    fp = ctypes.POINTER(ctypes.c_float)
    lut = rs.uniform(0, 1, size=(16, 4)).astype(f32)
    good = dict(surface_ref.DEFAULT_PARAMS) | {"weighted_average": True, "vmin": 0.0, "vmax": 2.0, "lut_rgba": lut}

    def params(**fields):
        """struct tsp_surface_params of `good`, then the given fields of the struct overwritten."""
        p, _ = _native.Context._surface_params(**good)
        for k, v in fields.items():
            setattr(p, k, v)
        return p

    tex = np.ones((2, 2, 4), dtype=f32)
    one, zero2 = np.ones(1, dtype=f32), np.zeros(2, dtype=f32)

    def quad(**kw):
        L = _native.PresentLayer()
        L.kind, L.texture_rgba, L.tex_width, L.tex_height = 0, tex.ctypes.data_as(fp), 2, 2
        L.clip_extent[:], L.tex_extent[:] = [1.0, 1.0], [1.0, 1.0]
        L.n_instances, L.instance_offsets, L.instance_weights = 1, zero2.ctypes.data_as(fp), one.ctypes.data_as(fp)
        for k, v in kw.items():
            setattr(L, k, v)
        return L

    nan3 = (ctypes.c_float * 3)(0.0, float("nan"), 1.0)
    ctx = context(64, 4)
    try:
        img = np.zeros((64, 64, 2), dtype=f32)
        img[..., 0] = rs.uniform(0.1, 2.0, size=(64, 64))
        img[..., 1] = rs.uniform(0.2, 0.9, size=(64, 64))
        ctx.write_image(img)
        want = surface_present_ref.compose_surface(img, 40, 30, good)
        assert_same(ctx.present_surface(40, 30, good), want)
        cases = [(40, 30, params(smoothing_scale=float("nan")), []),
                 (40, 30, params(smoothing_scale=float("inf")), []),
                 (40, 30, params(n_lut=1), []),                                      # weighted_average without a usable LUT
                 (40, 30, params(lut_rgba=None, n_lut=16), []),
                 (40, 30, params(n_lut=65537), []),
                 (40, 30, params(light_direction=nan3), []),
                 (40, 30, params(light_color=nan3), []),
                 (40, 30, params(ambient_color=nan3), []),
                 (40, 30, params(vmax=float("inf")), []),
                 (40, 30, params(depth_scale=float("nan")), []),
                 (0, 30, params(), []), (40, 0, params(), []), (16385, 30, params(), []), (-3, 30, params(), []),
                 (40, 30, params(), [quad(n_instances=129)]), (40, 30, params(), [quad(tex_width=0)]),
                 (40, 30, params(), [quad(kind=7)]), (40, 30, params(), [quad()] * 1025)]
        for W, H, p, layers in cases:
            for yuv in (False, True):
                out = np.full((30, 40, 4), 77, dtype=np.uint8)
                assert call_raw(ctx, W, H, p, layers, out, yuv) == -1, (W, H, yuv)
                assert np.all(out == 77)
                assert np.array_equal(ctx.read_image(), img)
        out = np.full((30, 40, 4), 77, dtype=np.uint8)
        assert call_raw(ctx, 41, 30, params(), [], out, yuv=True) == -1 and np.all(out == 77)       # odd 4:2:0 canvas
        assert ctx._lib.tsp_present_surface(ctx._h, 40, 30, None, None, 0, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                            None) == -1
        assert ctx._lib.tsp_present_surface(ctx._h, 40, 30, ctypes.byref(params()), None, 0, None, None) == -1
        for bad in [dict(good, smoothing_scale=float("nan")), dict(good, lut_rgba=lut[:1]), dict(good, vmin=float("nan"))]:
            with pytest.raises(_native.BackendError, match="error -1"):
                ctx.present_surface(40, 30, bad)
        with pytest.raises(_native.BackendError, match="error -1"):
            ctx.present_surface(0, 30, good)
        assert_same(ctx.present_surface(40, 30, good), want)                 # and the context still composes
        # a 4-channel active image
        img4 = rs.uniform(0.1, 2.0, size=(64, 64, 4)).astype(f32)
        ctx.write_image(img4)
        for yuv in (False, True):
            out = np.full((30, 40, 4), 77, dtype=np.uint8)
            assert call_raw(ctx, 40, 30, params(), [], out, yuv) == -1 and np.all(out == 77)
        with pytest.raises(_native.BackendError, match="error -1"):
            ctx.present_surface(40, 30, good)
        assert np.array_equal(ctx.read_image(), img4)
    finally:
        ctx.close()
