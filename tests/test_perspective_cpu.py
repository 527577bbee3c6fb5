"""The perspective camera without a GPU: the properties of its NumPy model (tests/perspective_ref.py, the contract of
tsp_project_perspective in include/topsy_splat.h), the field of view against the viewer's distance, the argument errors of
PerspectiveView and of the binding, the binding and the library's version, and the recorder's handling of `fov`."""
import ctypes
import pickle

import numpy as np
import pytest

import perspective_ref as ref
from test_recorder_cpu import Clock, StubVisualizer
from topsy_amd import _native, perspective
from topsy_amd.recorder import (LinearInterpolator, SmoothedLinearInterpolator, VisualizationRecorder)

F = np.float32


def _turn(a, b):
    ca, sa, cb, sb = np.cos(a), np.sin(a), np.cos(b), np.sin(b)
    return (np.array([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]]) @ np.array([[1, 0, 0], [0, cb, -sb], [0, sb, cb]])).astype(F)


def _cloud(n, seed=3):
    rs = np.random.RandomState(seed)
    return {"x": rs.normal(size=n).astype(F) * 5, "y": rs.normal(size=n).astype(F) * 5, "z": rs.normal(size=n).astype(F) * 5,
            "h": rs.uniform(0.01, 1.0, size=n).astype(F), "mass": rs.uniform(0.5, 2.0, size=n).astype(F)}


# ---- the model's properties -----------------------------------------------------------------------------------
def test_particles_on_the_reference_plane_are_unchanged():
    a = _cloud(200)
    a["z"][:] = 0.0
    a.update(r=a["mass"] * F(0.5), g=a["mass"] * F(0.25), b=a["mass"] * F(2.0))
    out = ref.project(a, np.eye(3), np.zeros(3), 17.3, 0.01)
    assert out["visible"].all() and (out["s"] == F(1.0)).all()
    for name in ("x", "y", "z", "h", "mass", "r", "g", "b"):
        assert np.array_equal(out[name], a[name]), name


def test_scaling_keeps_the_vertex_weight_and_scales_as_the_header_says():
    a = _cloud(500)
    rot, off, D, near = _turn(0.3, -0.7), np.array([1.0, -2.0, 0.5]), 20.0, 0.02
    out = ref.project(a, rot, off, D, near)
    vis = out["visible"]
    assert vis.all()
    xv, yv, zv = ref.view_coordinates(a["x"], a["y"], a["z"], *ref.camera(rot, off, D, near)[:2])
    s = F(D) / (F(D) - zv)
    assert np.array_equal(out["s"], s) and np.array_equal(out["x"], xv * s) and np.array_equal(out["z"], zv)
    assert np.array_equal(out["h"], a["h"] * s) and np.array_equal(out["mass"], a["mass"] * (s * s))
    # m' / h'^2 = m / h^2 up to the roundings of s * s, h * s, (h s)^2, m (s s) and the two divisions: six half-ulps
    w0, w1 = ref.weights(a["h"], a["mass"]), ref.weights(out["h"], out["mass"])
    assert (np.abs(w1 / w0 - 1.0) <= 6 * 2.0 ** -24).all()


def test_the_near_plane_is_inclusive_and_the_next_float_below_is_not():
    D, near = F(10.0), F(0.25)
    z_at = D - near                                    # d = D - z = near exactly (9.75 and 0.25 are exact)
    assert D - z_at == near
    z_inside = np.nextafter(z_at, F(np.inf))           # a hair nearer to the viewer: d < near
    assert D - z_inside < near
    a = {"x": np.array([1, 1, 1], dtype=F), "y": np.array([2, 2, 2], dtype=F), "z": np.array([z_at, z_inside, D + 1], dtype=F),
         "h": np.array([0.5, 0.5, 0.5], dtype=F), "mass": np.array([1, 1, 1], dtype=F)}
    out = ref.project(a, np.eye(3), np.zeros(3), D, near)
    assert out["visible"].tolist() == [True, False, False]          # at near; inside near; behind the viewer
    assert out["s"][0] == D / near and out["x"][0] == F(1.0) * (D / near) and out["h"][0] == F(0.5) * (D / near)
    for k in (1, 2):
        assert np.isnan(out["x"][k]) and np.isnan(out["y"][k]) and np.isnan(out["z"][k])
        assert out["h"][k] == 0 and out["mass"][k] == 0


def test_nan_and_infinite_inputs():
    nan, inf = F(np.nan), F(np.inf)
    a = {"x": np.array([nan, 1, 1, inf, 1, 1], dtype=F), "y": np.array([0, 0, 0, 0, 0, 0], dtype=F),
         "z": np.array([0, nan, -inf, 0, inf, 0], dtype=F), "h": np.array([1, 1, 1, 1, 1, nan], dtype=F),
         "mass": np.array([1, 1, 1, 1, 1, inf], dtype=F)}
    out = ref.project(a, np.eye(3), np.zeros(3), 10.0, 0.01)
    # a NaN or infinite x or y reaches zv through 0 * x = NaN, so d is NaN: not visible, like a NaN z and like z = +inf (behind the
    # viewer, d = -inf); z = -inf: d = +inf, s = 0 -- visible, at the vanishing point with h' = m' = 0 and, as xv took 0 * -inf,
    # a NaN position; a NaN h and an infinite mass go through
    assert out["visible"].tolist() == [False, False, True, False, False, True]
    for k in (0, 1, 3, 4):
        assert np.isnan(out["x"][k]) and np.isnan(out["y"][k]) and np.isnan(out["z"][k]) and out["h"][k] == 0 and out["mass"][k] == 0
    assert out["s"][2] == 0 and np.isnan(out["x"][2]) and out["z"][2] == -inf and out["h"][2] == 0 and out["mass"][2] == 0
    assert out["x"][5] == 1 and np.isnan(out["h"][5]) and out["mass"][5] == inf
    # the bounds drop the NaN coordinates and keep the infinite ones; hmax drops the NaN h
    b = ref.block_bounds(out["x"], out["y"], out["z"], out["h"])
    assert b.shape == (1, 2, 4)
    assert b[0, 0, 0] == 1 and b[0, 1, 0] == 1 and b[0, 0, 2] == -inf and b[0, 1, 2] == 0 and b[0, 0, 3] == 0


def test_zero_smoothing_length_and_the_weights():
    a = {"x": np.zeros(2, dtype=F), "y": np.zeros(2, dtype=F), "z": np.array([0, 20], dtype=F), "h": np.array([0, 1], dtype=F),
         "mass": np.array([3, 3], dtype=F)}
    out = ref.project(a, np.eye(3), np.zeros(3), 10.0, 0.01)
    assert out["h"].tolist() == [0, 0] and out["mass"].tolist() == [3, 0]
    w = ref.weights(out["h"], out["mass"])
    assert np.isinf(w[0]) and np.isnan(w[1])          # m / 0 and 0 / 0: weights_kernel's own answers for such particles


def test_block_bounds_by_blocks_of_512():
    a = _cloud(1200)
    out = ref.project(a, _turn(0.2, 0.1), np.zeros(3), 6.0, 0.5)       # a near viewer: some particles are not visible
    assert 0 < (~out["visible"]).sum() < 600
    b = ref.block_bounds(out["x"], out["y"], out["z"], out["h"])
    assert b.shape == (3, 2, 4)
    for k, sl in enumerate((slice(0, 512), slice(512, 1024), slice(1024, 1200))):
        assert b[k, 0, 0] == np.nanmin(out["x"][sl]) and b[k, 1, 1] == np.nanmax(out["y"][sl]) and b[k, 0, 3] == out["h"][sl].max()
        assert b[k, 1, 3] == 0
    empty = ref.block_bounds(np.full(3, np.nan, dtype=F), np.full(3, np.nan, dtype=F), np.full(3, np.nan, dtype=F), np.zeros(3, dtype=F))
    assert empty[0, 0, :3].tolist() == [np.inf] * 3 and empty[0, 1, :3].tolist() == [-np.inf] * 3 and empty[0, 0, 3] == 0


# ---- fov <-> distance -------------------------------------------------------------------------------------------
def test_fov_and_distance():
    assert np.isclose(perspective.fov_to_distance(10.0, 90.0), 10.0)
    assert np.isclose(perspective.fov_to_distance(10.0, 60.0), 10.0 * np.sqrt(3.0))
    assert np.isclose(perspective.fov_to_distance(2.5, 60.0), ref.fov_distance(2.5, 60.0))
    for fov in (1e-3, 1.0, 35.0, 120.0, 179.9):
        assert np.isclose(perspective.distance_to_fov(3.0, perspective.fov_to_distance(3.0, fov)), fov, rtol=1e-12)
    # fov -> 0: the viewer recedes and every s tends to 1, the orthographic view
    d = perspective.fov_to_distance(1.0, 1e-4)
    assert d > 1e6 and abs(d / (d - 1.0) - 1.0) < 1e-6


def test_clip_matrix_maps_near_and_far_onto_the_clip_range():
    M, sf = perspective.clip_matrix(4.0, 10.0, 0.5, 14.0)
    assert M.dtype == np.float32 and sf == F(0.25) and M[0, 0] == F(0.25) and M[1, 1] == F(0.25)
    for zv, want in ((10.0 - 14.0, 0.0), (10.0 - 0.5, 1.0), (0.0, 4.0 / 13.5)):
        assert np.isclose((M @ np.array([0, 0, zv, 1.0]))[2], want, atol=1e-6)
    assert (M[[0, 1, 3]][:, 2] == 0).all() and M[3].tolist() == [0, 0, 0, 1]


# ---- argument errors --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fov", [0, 0.0, -5, 180, 180.0, 200, float("nan"), float("inf"), "wide", None, True])
def test_fov_outside_0_180_raises(fov):
    with pytest.raises(ValueError):
        perspective.check_fov(fov)
    with pytest.raises(ValueError):
        perspective.PerspectiveView(object(), fov=fov)          # refused before the visualizer is looked at


@pytest.mark.parametrize("near", [0, -1.0, float("nan"), float("inf"), "close", True])
def test_near_must_be_positive_and_finite(near):
    with pytest.raises(ValueError):
        perspective.PerspectiveView(object(), fov=60.0, near=near)


class _Stub:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_views_over_several_gpus_or_periodic_tiling_are_refused():
    several = _Stub(particle_buffers=_Stub(context=_Stub(n_gpus=2)), _periodic_tiling=False)
    with pytest.raises(NotImplementedError, match="runs on one GPU"):
        perspective.PerspectiveView(several)
    tiled = _Stub(particle_buffers=_Stub(context=_Stub(n_gpus=1)), _periodic_tiling=True)
    with pytest.raises(NotImplementedError, match="no periodic tiling"):
        perspective.PerspectiveView(tiled)


@pytest.mark.parametrize("rot, offset, distance, near", [
    (np.eye(2), np.zeros(3), 10.0, 0.1), (np.eye(3), np.zeros(2), 10.0, 0.1), (np.eye(3) * np.nan, np.zeros(3), 10.0, 0.1),
    (np.eye(3), [0, np.inf, 0], 10.0, 0.1), (np.eye(3), np.zeros(3), 0.0, 0.1), (np.eye(3), np.zeros(3), -1.0, 0.1),
    (np.eye(3), np.zeros(3), np.nan, 0.1), (np.eye(3), np.zeros(3), np.inf, 0.1), (np.eye(3), np.zeros(3), 10.0, 0.0),
    (np.eye(3), np.zeros(3), 10.0, 10.0), (np.eye(3), np.zeros(3), 10.0, 11.0), (np.eye(3), np.zeros(3), 10.0, np.nan),
    (np.eye(3), np.zeros(3), 10.0, -0.1), ("abc", np.zeros(3), 10.0, 0.1), (np.eye(3), np.zeros(3), "far", 0.1)])
def test_the_binding_refuses_bad_cameras(rot, offset, distance, near):
    with pytest.raises(ValueError):
        _native.perspective_struct(rot, offset, distance, near)


def test_the_binding_rounds_the_camera_to_float32():
    cam = _native.perspective_struct(_turn(0.3, 0.4).astype(np.float64), [0.1, 0.2, 0.3], 10.1, 0.3)
    assert np.array_equal(np.array(cam.rot[:], dtype=F).reshape(3, 3), _turn(0.3, 0.4))
    assert list(cam.offset) == [float(F(0.1)), float(F(0.2)), float(F(0.3))]
    assert cam.distance == float(F(10.1)) and cam.near == float(F(0.3))
    assert ctypes.sizeof(_native.Perspective) == 14 * 4


# ---- binding and version ------------------------------------------------------------------------------------------
def test_binding_and_version():
    assert "tsp_project_perspective" in _native.SIGNATURES
    lib = _native.load_library()
    assert hasattr(lib, "tsp_project_perspective")
    assert lib.tsp_version() >= 128 and _native.ABI_VERSION == 112
    assert callable(_native.Context.project_perspective)


def test_the_library_refuses_null_arguments_without_a_gpu():
    lib = _native.load_library()
    cam = _native.perspective_struct(np.eye(3), np.zeros(3), 10.0, 0.1)
    assert lib.tsp_project_perspective(None, None, ctypes.byref(cam)) < 0
    assert b"NULL" in lib.tsp_last_error()


# ---- the recorder ---------------------------------------------------------------------------------------------------
class StubPerspective(StubVisualizer):
    def __init__(self):
        super().__init__()
        self.fov = 60.0

    def state(self):
        return dict(super().state(), fov=self.fov)


def _fov_path():
    view, clock = StubPerspective(), Clock()
    rec = VisualizationRecorder(view, clock=clock)
    rec.record()
    for fov in (40.0, 90.0):
        clock.t += 0.5
        view.fov = fov
        view.scale = view.scale / 2
        rec.mark()
    rec.stop()
    return view, rec


def test_fov_is_recorded_and_replayed_on_a_target_that_has_one(tmp_path):
    view, rec = _fov_path()
    assert rec._record_properties[-1] == "fov" and rec._record_properties[:-1] == VisualizationRecorder._record_properties
    assert rec._record_interpolation_class_smoothed[-1] is SmoothedLinearInterpolator
    assert rec._record_interpolation_class_unsmoothed[-1] is LinearInterpolator
    assert rec._timestream["fov"] == [(0.0, 60.0), (0.5, 40.0), (1.0, 90.0)]
    frames = list(rec.frames(fps=4, resolution=(4, 2), smooth=False))
    assert len(frames) == 4
    assert [s["fov"] for s in view.rendered] == [60.0, 50.0, 40.0, 65.0]              # linear between the keys
    view.rendered.clear()
    list(rec.frames(fps=4, resolution=(4, 2), smooth=True))
    smoothed = [s["fov"] for s in view.rendered]
    assert len(smoothed) == 4 and all(40.0 <= f <= 90.0 for f in smoothed) and smoothed != [60.0, 50.0, 40.0, 65.0]
    # the timestream round-trips with its fov
    fn = str(tmp_path / "fly.timestream")
    rec.save_timestream(fn)
    other_view = StubPerspective()
    other = VisualizationRecorder(other_view)
    other.load_timestream(fn)
    assert other._timestream["fov"] == rec._timestream["fov"]
    list(other.frames(fps=4, resolution=(4, 2), smooth=False))
    assert [s["fov"] for s in other_view.rendered] == [60.0, 50.0, 40.0, 65.0]


def test_a_visualizer_target_keeps_the_pickle_layout(tmp_path):
    vis, clock = StubVisualizer(), Clock()
    rec = VisualizationRecorder(vis, clock=clock)
    rec.record()
    clock.t += 1.0
    rec.mark()
    rec.stop()
    assert rec._record_properties is VisualizationRecorder._record_properties and "fov" not in rec._timestream
    fn = str(tmp_path / "old.timestream")
    rec.save_timestream(fn)
    with open(fn, "rb") as f:
        ts, ends_at = pickle.load(f)
    assert list(ts) == VisualizationRecorder._record_properties and ends_at == 1.0


def test_a_timestream_without_fov_replays_on_a_perspective_target_and_leaves_fov_alone(tmp_path):
    vis, clock = StubVisualizer(), Clock()
    rec = VisualizationRecorder(vis, clock=clock)
    rec.record()
    clock.t += 1.0
    vis.scale = 2.0
    rec.mark()
    rec.stop()
    fn = str(tmp_path / "old.timestream")
    rec.save_timestream(fn)
    view = StubPerspective()
    view.fov = 33.0
    replay = VisualizationRecorder(view)
    replay.load_timestream(fn)
    frames = list(replay.frames(fps=2, resolution=(4, 2), smooth=False))
    assert len(frames) == 2 and [s["fov"] for s in view.rendered] == [33.0, 33.0]
    assert [s["scale"] for s in view.rendered] == [10.0, 6.0]
