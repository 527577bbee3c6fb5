"""The composed surface frame without a GPU: the numpy restatement (tests/surface_present_ref.py) reduces to the shading of
surface_ref at W = H = R, gives the colours and normals the arithmetic of include/topsy_splat.h "tsp_present_surface" predicts on
constant and ramped depths, the header declares the entry points, and SurfaceView offers everything a VisualizationRecorder
touches (checked on a numpy context, no device)."""
import copy
import os
import types

import numpy as np
import pytest

import surface_present_ref
import surface_ref
import yuv420_ref
from conftest import ROOT
from topsy_amd.colormap.implementation import _lut_from_matplotlib

f32 = np.float32

# the option sets and the seeded image of tests/test_gpu_surface.py::test_shading_bit_identical
SHADING_OPTIONS = [{}, {"weighted_average": True, "log": False, "vmin": -1.0, "vmax": 2.0},
                   {"weighted_average": True, "log": True, "vmin": -2.0, "vmax": 0.5},
                   {"depth_scale": 1.7, "light_direction": [0.3, -0.4, 0.866], "light_color": [0.9, 0.5, 0.2],
                    "ambient_color": [0.1, 0.2, 0.3]}]


def shading_image(R=120):
    rs = np.random.RandomState(9)
    img = np.zeros((R, R, 2), dtype=f32)
    img[..., 0] = rs.lognormal(size=(R, R)) * np.where(rs.uniform(size=(R, R)) < 0.1, -1, 1)
    img[::17, ::13, 0] = np.nan
    yy, xx = np.mgrid[0:R, 0:R]
    img[..., 1] = np.clip(0.8 - ((xx - 60.0) ** 2 + (yy - 50.0) ** 2) / 4000.0, 0, None)
    return img


def shading_params(opts):
    lut = _lut_from_matplotlib("twilight_shifted", 1000)
    return dict(surface_ref.DEFAULT_PARAMS) | {"smoothing_scale": 0.02, "lut_rgba": lut} | opts


@pytest.mark.parametrize("opts", SHADING_OPTIONS)
def test_square_canvas_is_the_shading_of_surface_ref(opts):
    img = shading_image()
    params = shading_params(opts)
    got = surface_present_ref.compose_surface(img, 120, 120, params)
    args = {k: v for k, v in params.items() if k not in ("smoothing_scale", "lut_rgba")}
    want = surface_ref.shade(surface_ref.bilateral(img, params["smoothing_scale"]), lut=params["lut_rgba"], **args)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert len(np.unique(got[..., :3])) > 20


@pytest.mark.parametrize("W, H", [(333, 211), (64, 40), (211, 333)])      # linear, nearest, portrait
def test_constant_depth_gives_one_colour(W, H):
    R = 96
    img = np.zeros((R, R, 2), dtype=f32)
    img[..., 0] = np.random.RandomState(1).normal(size=(R, R))
    for depth in (0.3, 0.7):
        img[..., 1] = depth
        params = dict(surface_ref.DEFAULT_PARAMS) | {"light_color": [0.9, 0.6, 0.3], "ambient_color": [0.05, 0.1, 0.2]}
        got = surface_present_ref.compose_surface(img, W, H, params)
        # flat: the normal is (0, 0, 1) exactly, n.L = Lz
        Lz = f32(params["light_direction"][2])
        k = f32(min(depth, 0.5)) * f32(2.0)
        want = [int(np.floor(min(max((f32(lc) * Lz + f32(a)) * k, 0.0), 1.0) * f32(255.0) + f32(0.5)))
                for lc, a in zip(params["light_color"], params["ambient_color"])]
        assert got.shape == (H, W, 4)
        assert (got.reshape(-1, 4) == np.array(want + [255], dtype=np.uint8)).all(), (depth, got[0, 0], want)


@pytest.mark.parametrize("W, H, R", [(480, 480, 120), (600, 400, 150)])
def test_depth_ramp_gives_the_predicted_normal(W, H, R):
    g = 0.002                                              # depth per texel along x
    img = np.zeros((R, R, 2), dtype=f32)
    img[..., 1] = (0.2 + g * np.arange(R))[None, :]
    F = surface_ref.bilateral(img, 1e-7)                   # a 1-pixel kernel: F is the image
    assert np.array_equal(F, img)
    nx, ny, nz, _, _ = surface_present_ref.normals(F, W, H)
    du = R / W
    want = np.array([-g * du, 0.0, 1.0 / W])
    want /= np.linalg.norm(want)
    m = int(np.ceil(2 * max(W, H) / R)) + 1                # away from the clamped edges of the image
    inner = (slice(m, H - m), slice(m, W - m))
    assert np.allclose(nx[inner], want[0], rtol=2e-3, atol=0) and np.allclose(nz[inner], want[2], rtol=2e-3, atol=0)
    # rows are equal, but a float32 lerp of two equal depths d may differ from d by an ulp (6e-8 d): |Dd - Du| <= 1.2e-7 * 0.5,
    # halved and divided by the normal's length (>= 1 / W = 2e-3 here) stays below 2e-5
    assert np.all(np.abs(ny[inner]) < 2e-5)


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "topsy_splat.h")).read()
    assert "int tsp_present_surface(tsp_context *ctx, int width, int height, const tsp_surface_params *params" in text
    assert "int tsp_present_surface_yuv420(tsp_context *ctx, int width, int height, const tsp_surface_params *params" in text
    assert " * 112: surface frames: tsp_present_surface and tsp_present_surface_yuv420" in text
    from topsy_amd import _native
    assert _native.ABI_VERSION == 112
    assert {"tsp_present_surface", "tsp_present_surface_yuv420"} <= set(_native.SIGNATURES)


# ---- SurfaceView on a numpy context -------------------------------------------------------------------------------
class NumpyContext:
    """What SurfaceView and its occlusion renderer ask of a context, answered by the restatements."""
    n_gpus = 1
    num_particles = 0
    resolution = 32

    def __init__(self):
        self.calls = []
        self.matrix = None

    def set_sphere_mips(self, mips):
        pass

    def render_surface(self, M, sf, cut):
        self.matrix = np.array(M)
        return 0.1

    def read_image(self):
        """A bump whose position follows the camera matrix, so that frames of different states differ."""
        R = self.resolution
        yy, xx = np.mgrid[0:R, 0:R]
        cx = 16.0 + 200.0 * float(self.matrix[0, 0])
        img = np.zeros((R, R, 2), dtype=f32)
        img[..., 0] = 1.0 + xx / R
        img[..., 1] = np.clip(0.7 - ((xx - cx) ** 2 + (yy - 14.0) ** 2) / 300.0, 0, None)
        return img

    def present_surface(self, W, H, params, layers=(), timings=None):
        self.calls.append(("rgba", W, H, len(layers)))
        return surface_present_ref.compose_surface(self.read_image(), W, H, params, layers)

    def present_surface_yuv420(self, W, H, params, layers=(), timings=None):
        self.calls.append(("yuv", W, H, len(layers)))
        return yuv420_ref.to_yuv420(surface_present_ref.compose_surface(self.read_image(), W, H, params, layers))


class Progression:
    def get_fraction_volume_selected(self):
        return 1.0


class FakeVisualizer:
    _periodic_tiling = False
    _render_resolution = 32

    def __init__(self):
        self.particle_buffers = types.SimpleNamespace(context=NumpyContext(), ensure_quantity=lambda: None, last_renderer=None)
        self.data_loader = types.SimpleNamespace(get_position_units=lambda: "kpc", get_quantity_label=lambda name: f"label of {name}")
        self._sph = types.SimpleNamespace(rotation_matrix=np.eye(3), position_offset=np.zeros(3), scale=10.0,
                                          _render_progression=Progression())
        self.quantity_name = "test-quantity"

    rotation_matrix = property(lambda s: s._sph.rotation_matrix, lambda s, v: setattr(s._sph, "rotation_matrix", v))
    position_offset = property(lambda s: s._sph.position_offset, lambda s, v: setattr(s._sph, "position_offset", v))
    scale = property(lambda s: s._sph.scale, lambda s, v: setattr(s._sph, "scale", v))


class Clock:
    t = 100.0

    def __call__(self):
        return self.t


@pytest.fixture()
def view():
    from topsy_amd.surface import SurfaceView
    vis = FakeVisualizer()
    return vis, SurfaceView(vis)


def test_surface_view_has_the_frame_interface(view):
    vis, sv = view
    assert (sv.show_colorbar, sv.show_scalebar, sv.show_status, sv.crosshairs_visible) == (True, True, True, False)
    assert sv.canvas_format == "rgba8unorm"
    for name in ("display_status", "get_presentation_image", "get_presentation_image_yuv420", "add_frame_listener",
                 "remove_frame_listener"):
        assert callable(getattr(sv, name))
    # view state is the visualizer's, both ways
    sv.scale = 25.0
    sv.position_offset = np.array([1.0, 2.0, 3.0])
    sv.rotation_matrix = np.diag([1.0, -1.0, -1.0])
    assert vis.scale == 25.0 and np.array_equal(vis.position_offset, [1.0, 2.0, 3.0]) and vis.rotation_matrix[1, 1] == -1.0
    vis.scale = 12.0
    assert sv.scale == 12.0 and sv.quantity_name == "test-quantity"
    # colormap item access; an unknown key reads as None; another type is refused
    assert sv.colormap["type"] == "surface" and sv.colormap["gamma"] is None and sv.colormap["density_vmin"] is None
    sv.colormap["vmin"] = -0.5
    assert sv["vmin"] == -0.5 and sv.colormap["vmin"] == -0.5
    sv.colormap["type"] = "surface"
    with pytest.raises(ValueError):
        sv.colormap["type"] = "density"


def test_frames_layers_and_listeners_on_a_numpy_context(view):
    vis, sv = view
    ctx = vis.particle_buffers.context
    seen = []
    sv.add_frame_listener(seen.append)
    sv.display_status("cpu frame", timeout=600)
    got = sv.get_presentation_image((96, 64))
    params, layers = sv._last_presentation
    assert got.shape == (64, 96, 4) and got.dtype == np.uint8
    assert [L["kind"] for L in layers] == ["quad", "quad", "quad", "quad"]        # colorbar, label, bar, status
    assert sv["vmin"] is not None and sv["vmax"] is not None                       # autoranged from the raw image
    assert params["weighted_average"] and params["vmin"] == sv["vmin"]
    assert np.array_equal(got, surface_present_ref.compose_surface(ctx.read_image(), 96, 64, params, layers))
    planes = sv.get_presentation_image_yuv420((96, 64))
    assert [p.shape for p in planes] == [(64, 96), (32, 48), (32, 48)]
    assert len(seen) == 2 and all(s is sv for s in seen)
    assert ctx.calls == [("rgba", 96, 64, 4), ("yuv", 96, 64, 4)]
    # the colorbar exists only for a quantity (reference visualizer.py:327-328); the quantity setter syncs the material at once
    sv.quantity_name = None
    assert vis.quantity_name is None and sv["weighted_average"] is False and sv["vmin"] is None
    sv.get_presentation_image((96, 64))
    assert [L["kind"] for L in sv._last_presentation[1]] == ["quad", "quad", "quad"]
    sv.show_scalebar = sv.show_status = False
    sv.crosshairs_visible = True
    sv.get_presentation_image((96, 64))
    assert [L["kind"] for L in sv._last_presentation[1]] == ["lines"]
    listener = sv._frame_listeners[0]
    sv.remove_frame_listener(listener)
    sv.get_presentation_image((96, 64))
    assert len(seen) == 4
    for bad in [(0, 10), (10, 16385)]:
        with pytest.raises(ValueError):
            sv.get_presentation_image(bad)
    with pytest.raises(ValueError):
        sv.get_presentation_image_yuv420((95, 64))


def test_the_unmodified_recorder_records_and_replays_a_view(view, tmp_path):
    from topsy_amd.recorder import STATUS_TEXT, Interpolator, VisualizationRecorder
    vis, sv = view
    sv.display_status(STATUS_TEXT, timeout=1e6)
    sv.get_presentation_image((32, 24))
    clock = Clock()
    rec = VisualizationRecorder(sv, clock=clock)
    assert set(rec._timestream) == set(rec._record_properties)
    assert rec._timestream["colormap[type]"][0][1] == "surface" and rec._timestream["colormap[gamma]"][0][1] is None
    rec.record()
    for k in range(3):
        clock.t += 0.5
        sv.scale = sv.scale * 0.8
        rec.mark()
    rec.stop()
    sv.show_colorbar = False
    frames = list(rec.frames(fps=4, resolution=(32, 24), smooth=False, pixel_format="yuv420p"))
    assert len(frames) == int(1.5 * 4) == 6
    assert sv.show_colorbar is False                        # the replay gives the switches back
    # every frame equals the direct call at the interpolated state
    interps = [(p, c(rec._timestream[p])) for c, p in zip(rec._record_interpolation_class_unsmoothed, rec._record_properties)]
    sv.show_colorbar = True
    for i, planes in enumerate(frames):
        for p, f in interps:
            value = f(i / 4)
            if value is not Interpolator.no_value:
                if p.startswith("colormap["):
                    sv.colormap[p[9:-1]] = value
                else:
                    setattr(sv, p, value)
        sv.display_status(STATUS_TEXT, timeout=1e6)
        want = sv.get_presentation_image_yuv420((32, 24))
        assert all(np.array_equal(a, b) for a, b in zip(planes, want)), i
    assert not np.array_equal(frames[0][0], frames[-1][0])
    fn = tmp_path / "surface.y4m"
    rec.save_y4m(str(fn), 4, (32, 24), smooth=False)
    header = b"YUV4MPEG2 W32 H24 F4:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n"
    data = fn.read_bytes()
    assert data.startswith(header) and len(data) == len(header) + 6 * (6 + 32 * 24 * 3 // 2)
    # a timestream of another map type is refused by the surface map
    other = copy.deepcopy(rec._timestream)
    other["colormap[type]"] = [(0.0, "density")]
    rec._timestream = other
    with pytest.raises(ValueError):
        list(rec.frames(fps=4, resolution=(32, 24), smooth=False))
