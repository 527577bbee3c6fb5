"""Movie frames on the GPU (tsp_present_yuv420, VisualizerBase.get_presentation_image_yuv420, topsy_amd.recorder): the planes equal
the restatement (tests/yuv420_ref.py) of tsp_present's RGBA frame bit for bit on every canvas shape and map, the refusals leave
everything untouched, and a recorded path replays into frames equal to get_presentation_image taken by hand and into a y4m
file that parses back to the same planes."""
import ctypes
import pickle
import time

import numpy as np
import pytest

import yuv420_ref
import topsy_amd
from topsy_amd import _native
from topsy_amd.recorder import STATUS_TEXT, Interpolator, VisualizationRecorder

pytestmark = pytest.mark.gpu

CANVASES = [(1920, 1080), (3840, 2160), (1366, 768), (480, 640), (2, 2), (16384, 2)]


def assert_planes_equal(planes, rgba):
    want = yuv420_ref.to_yuv420(rgba)
    H, W = rgba.shape[:2]
    assert [p.shape for p in planes] == [(H, W), (H // 2, W // 2), (H // 2, W // 2)]
    for got, w, name in zip(planes, want, "YUV"):
        assert got.dtype == np.uint8 and np.array_equal(got, w), name


def frame_and_planes(vis, W, H):
    """get_presentation_image, then present_yuv420 on the same base and layers, and the visualizer's own 4:2:0 frame."""
    rgba = vis.get_presentation_image((W, H))
    base, layers = vis._last_presentation
    ctx = vis._sph._context
    planes = ctx.present_yuv420(W, H, base, layers)
    own = vis.get_presentation_image_yuv420((W, H))
    again = ctx.present(W, H, *vis._last_presentation)          # what the visualizer's call was composed from
    return rgba, planes, own, again


@pytest.fixture(scope="module")
def vis512():
    v = topsy_amd.test(3000, render_resolution=512)
    v.quantity_name = "test-quantity"
    v.display_status("movie test", timeout=600)
    yield v
    v.close()


@pytest.mark.parametrize("W, H", CANVASES)
def test_planes_equal_the_restated_rgba_frame_on_every_canvas(vis512, W, H):
    vis512.show_colorbar = vis512.show_scalebar = vis512.show_status = True
    rgba, planes, own, again = frame_and_planes(vis512, W, H)
    assert_planes_equal(planes, rgba)
    assert_planes_equal(own, again)


@pytest.mark.parametrize("mode, quantity", [("univariate", None), ("univariate", "test-quantity"), ("bivariate", "test-quantity"),
                                            ("rgb", None)])
def test_planes_for_every_map(mode, quantity):
    v = topsy_amd.test(2000, render_resolution=128, render_mode=mode)
    try:
        if quantity:
            v.quantity_name = quantity
        v.display_status("maps", timeout=600)
        for W, H in [(300, 200), (1366, 768)]:
            rgba, planes, own, again = frame_and_planes(v, W, H)
            assert_planes_equal(planes, rgba)
            assert_planes_equal(own, again)
    finally:
        v.close()


def test_every_layer_on_a_periodic_view():
    v = topsy_amd.test(3000, render_resolution=256, periodic_tiling=True)
    try:
        v.rotate(0.3, 0.5)
        v.scale = 80.0
        v.crosshairs_visible = True
        v.display_status("periodic", timeout=600)
        for W, H in [(1280, 720), (1366, 768)]:
            rgba, planes, own, again = frame_and_planes(v, W, H)
            assert [L["kind"] for L in v._last_presentation[1]] == ["quad", "quad", "quad", "lines", "lines", "quad"]
            assert_planes_equal(planes, rgba)
            assert_planes_equal(own, again)
    finally:
        v.close()


def call_raw(ctx, W, H, base, out):
    b, arr, keep = ctx._present_args(base, [])
    return ctx._lib.tsp_present_yuv420(ctx._h, W, H, ctypes.byref(b), arr, 0, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                       None)


def test_refusals_leave_everything_untouched():
    rs = np.random.RandomState(11)
    for C, base in [(2, {"map": "scalar", "lut": rs.uniform(0, 1, size=(16, 4)).astype(np.float32), "vmin": 0.0, "vmax": 2.0,
                         "log": False, "weighted": False}),
                    (4, {"map": "rgb-hdr", "vmin": -1.0, "vmax": 0.5, "gamma": 1.0})]:
        ctx = _native.Context(64, C)
        try:
            img = rs.uniform(0.1, 2.0, size=(64, 64, C)).astype(np.float32)
            ctx.write_image(img)
            good = base if base["map"] != "rgb-hdr" else dict(base, map="rgb")
            want = ctx.present(40, 30, good)
            cases = [(41, 30), (40, 31), (16386, 2), (2, 16386), (16385, 2), (0, 2), (1, 1), (-2, 2)]
            if base["map"] == "rgb-hdr":
                cases = [(40, 30)]
            for W, H in cases:
                out = np.full(max(W, 2) * max(H, 2) * 2, 77, dtype=np.uint8)
                assert call_raw(ctx, W, H, base, out) == -1, (W, H, base["map"])
                assert np.all(out == 77)
                assert np.array_equal(ctx.read_image(), img)
                assert np.array_equal(ctx.present(40, 30, good), want)
            with pytest.raises(_native.BackendError):
                ctx.present_yuv420(40, 30, base) if base["map"] == "rgb-hdr" else ctx.present_yuv420(41, 30, base)
            assert_planes_equal(ctx.present_yuv420(40, 30, good), want)
        finally:
            ctx.close()


def test_visualizer_refuses_odd_sizes_and_the_hdr_canvas():
    v = topsy_amd.test(1000, render_resolution=64, render_mode="rgb-hdr")
    try:
        with pytest.raises(ValueError):
            v.get_presentation_image_yuv420((64, 64))
    finally:
        v.close()
    v = topsy_amd.test(1000, render_resolution=64)
    try:
        with pytest.raises(ValueError):
            v.get_presentation_image_yuv420((63, 64))
    finally:
        v.close()


def test_frame_listeners_see_the_frames_the_reference_synchronises():
    from topsy_amd.drawreason import DrawReason
    v = topsy_amd.test(1000, render_resolution=64)
    try:
        v.draw(DrawReason.CHANGE)                       # no listener: nothing to call
        seen = []
        listener = seen.append
        v.add_frame_listener(listener)
        v.draw(DrawReason.CHANGE)
        v.draw(DrawReason.REFINE)
        v.draw(DrawReason.PRESENTATION_CHANGE)
        v.draw(DrawReason.EXPORT)
        assert len(seen) == 2
        v.get_sph_presentation_image()
        v.get_presentation_image((32, 24))
        v.get_presentation_image_yuv420((32, 24))
        assert len(seen) == 5 and all(x is v for x in seen)
        v.remove_frame_listener(listener)
        v.get_presentation_image((32, 24))
        assert len(seen) == 5
    finally:
        v.close()


# ---- recording and replay ------------------------------------------------------------------------------------------
class Clock:
    def __init__(self):
        self.t = 1000.0

    def __call__(self):
        return self.t


@pytest.fixture(scope="module")
def recorded():
    vis = topsy_amd.test(100_000, render_resolution=256)
    vis.display_status(STATUS_TEXT, timeout=1e6)      # the status line already shows the replay's text: no timing in the frames
    time.sleep(0.1)
    vis.get_presentation_image((96, 64))
    clock = Clock()
    rec = VisualizationRecorder(vis, clock=clock)
    rec.record()
    vmin = vis.colormap["vmin"]
    for k in range(1, 5):
        clock.t += 0.25
        vis.rotate(0.15, 0.1)                           # a turn
        vis.scale = vis.scale * 0.8                     # a zoom
        vis.position_offset = vis.position_offset + np.array([0.5, -0.3, 0.2])
        if k == 2:
            vis.colormap["vmin"] = vmin + 0.4
        rec.mark()
    rec.stop()
    yield vis, rec
    vis.close()


def by_hand(vis, rec, fps, resolution, smooth):
    """The replay restated: fresh interpolators, the state set in recorded order, then get_presentation_image."""
    classes = rec._record_interpolation_class_smoothed if smooth else rec._record_interpolation_class_unsmoothed
    interps = [(p, c(rec._timestream[p])) for c, p in zip(classes, rec._record_properties)]
    out = []
    for i in range(int(rec._recording_ends_at * fps)):
        for p, f in interps:
            value = f(i / fps)
            if value is Interpolator.no_value:
                continue
            if p.startswith("colormap["):
                vis.colormap[p[9:-1]] = value
            else:
                setattr(vis, p, value)
        vis.display_status(STATUS_TEXT, timeout=1e6)
        out.append(vis.get_presentation_image(resolution)[..., :3])
    return out


@pytest.mark.parametrize("smooth", [False, True])
def test_replayed_frames_equal_frames_set_by_hand(recorded, smooth):
    vis, rec = recorded
    ts = rec._timestream
    assert len(ts["scale"]) == 5 and ts["colormap[vmin]"][2][1] != ts["colormap[vmin]"][1][1]
    frames = list(rec.frames(fps=8, resolution=(96, 64), smooth=smooth))
    assert len(frames) == 8
    want = by_hand(vis, rec, 8, (96, 64), smooth)
    for i, (a, b) in enumerate(zip(frames, want)):
        assert a.shape == (64, 96, 3) and np.array_equal(a, b), i
    assert len(ts["scale"]) == 5                        # replay frames are not recorded
    assert not np.array_equal(frames[0], frames[-1])


def test_save_y4m_parses_back_to_the_restated_frames(recorded, tmp_path):
    vis, rec = recorded
    fn = tmp_path / "path.y4m"
    rec.save_y4m(str(fn), 8, (96, 64), smooth=False)
    rgb = list(rec.frames(fps=8, resolution=(96, 64), smooth=False))
    data = fn.read_bytes()
    header = b"YUV4MPEG2 W96 H64 F8:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n"
    assert data.startswith(header)
    size = 96 * 64 * 3 // 2
    body = data[len(header):]
    assert len(body) == 8 * (6 + size)
    for i, frame in enumerate(rgb):
        chunk = body[i * (6 + size):(i + 1) * (6 + size)]
        assert chunk[:6] == b"FRAME\n"
        y = np.frombuffer(chunk[6:6 + 96 * 64], np.uint8).reshape(64, 96)
        u = np.frombuffer(chunk[6 + 96 * 64:6 + 96 * 64 + 48 * 32], np.uint8).reshape(32, 48)
        v = np.frombuffer(chunk[6 + 96 * 64 + 48 * 32:], np.uint8).reshape(32, 48)
        assert_planes_equal((y, u, v), frame)


def test_a_1080p_y4m_file(recorded, tmp_path):
    vis, rec = recorded
    fn = tmp_path / "hd.y4m"
    rec.save_y4m(str(fn), 4, (1920, 1080))
    data = fn.read_bytes()
    header = b"YUV4MPEG2 W1920 H1080 F4:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n"
    n = int(rec._recording_ends_at * 4)
    assert n == 4 and data.startswith(header) and len(data) == len(header) + n * (6 + 1920 * 1080 * 3 // 2)
    assert all(data[len(header) + i * (6 + 1920 * 1080 * 3 // 2):][:6] == b"FRAME\n" for i in range(n))


def test_a_reference_layout_timestream_loads_and_replays(recorded, golden, tmp_path):
    vis, rec = recorded
    names = golden.json("recorder_kats.json")["properties"]
    start = {p: (vis.colormap[p[9:-1]] if p.startswith("colormap[") else getattr(vis, p)) for p in names}
    end = dict(start, scale=start["scale"] * 0.5, position_offset=np.asarray(start["position_offset"]) + 1.0)
    end["colormap[vmin]"] = start["colormap[vmin]"] + 0.2
    ts = {p: [(0.0, start[p]), (0.4, end[p])] for p in names}
    fn = tmp_path / "desktop.timestream"
    with open(fn, "wb") as f:
        pickle.dump((ts, 0.5), f)
    other = VisualizationRecorder(vis)
    other.load_timestream(str(fn))
    frames = list(other.frames(fps=10, resolution=(64, 48), smooth=False))
    assert len(frames) == 5 and all(f.shape == (48, 64, 3) for f in frames)
    assert vis.scale == pytest.approx(start["scale"] * 0.5)
    assert vis.colormap["vmin"] == end["colormap[vmin]"]
    other.save_timestream(str(tmp_path / "again.timestream"))
    with open(tmp_path / "again.timestream", "rb") as f:
        ts2, ends2 = pickle.load(f)
    assert ends2 == 0.5 and list(ts2) == names
    for p in names:
        assert [t for t, _ in ts2[p]] == [0.0, 0.4]
        for (_, a), (_, b) in zip(ts2[p], ts[p]):
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
