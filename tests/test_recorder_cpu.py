"""Movie recording without a GPU: the interpolators against the reference's known answers (tests/golden/recorder_kats.json),
the recorded properties, the 4:2:0 conversion rule (tests/yuv420_ref.py, include/topsy_splat.h), the y4m and ffmpeg writers,
and VisualizationRecorder's logic on a stub visualizer driven by an injected clock."""
import pickle
import stat
import sys

import numpy as np
import pytest

import yuv420_ref
from topsy_amd.recorder import VisualizationRecorder, interpolator, y4m_header

PROPS = ["colormap[type]", "quantity_name", "colormap[log]", "colormap[vmin]", "colormap[vmax]", "colormap[gamma]",
         "colormap[density_vmin]", "colormap[density_vmax]", "rotation_matrix", "scale", "position_offset"]


@pytest.fixture(scope="module")
def kats(golden):
    return golden.json("recorder_kats.json")


# ---- interpolators ------------------------------------------------------------------------------------------
def _make(case):
    cls = getattr(interpolator, case["class"])
    rotation = "Rotation" in case["class"]
    stream = [(t, np.array(v) if rotation else v) for t, v in case["timestream"]]
    return cls(stream, **case["kwargs"]), stream


def test_every_interpolator_meets_every_known_answer(kats):
    cases = kats["interpolation"]
    assert {c["class"] for c in cases} == {"StepInterpolator", "LinearInterpolator", "SmoothedStepInterpolator",
                                           "RotationInterpolator", "SmoothedLinearInterpolator", "SmoothedRotationInterpolator"}
    n = 0
    for case in cases:
        interp, _ = _make(case)
        for chk in case["checks"]:          # in the order written: the step interpolators need sequential times
            got = interp(chk["t"])
            where = (case["test"], chk)
            if chk["kind"] == "no_value":
                assert got is interpolator.Interpolator.no_value, where
            elif chk["kind"] == "is_none":
                assert got is None, where
            elif chk["kind"] == "eq":
                assert got is not interpolator.Interpolator.no_value and got == chk["value"], where
            else:
                assert np.allclose(got, chk["value"]), where
            n += 1
    assert n >= 40


def test_rotations_stay_orthogonal_and_smoothed_paths_stay_smooth(kats):
    cases = {c["test"]: c for c in kats["interpolation"]}
    for name in ("test_rotation_interpolator", "test_smoothed_rotation_interpolator"):
        interp, stream = _make(cases[name])
        for t in np.arange(0.0, 1.0, 0.1):
            m = interp(t)
            assert np.allclose(m @ m.T, np.eye(3)), (name, t)
    interp, stream = _make(cases["test_rotation_interpolator"])
    mid = interp(0.5)
    assert 0.0 < mid[0, 0] < 1.0 and 0.0 < mid[0, 1] < 1.0
    assert np.allclose(interp(1.0), stream[-1][1])
    interp, _ = _make(cases["test_smoothed_linear_interpolator"])
    assert abs(np.diff(np.diff([interp(x) for x in np.arange(0.0, 4.0, 0.05)]))).max() < 0.02


def test_step_interpolator_needs_sequential_times():
    interp = interpolator.StepInterpolator([(0.0, "a"), (1.0, "b")])
    assert interp(0.5) == "a"
    with pytest.raises(ValueError):
        interp(0.2)


def test_smoothing_a_recording_shorter_than_one_sample_keeps_its_value():
    interp = interpolator.SmoothedLinearInterpolator([(0.0, 2.0), (0.01, 2.0)])
    assert np.isclose(interp(0.0), 2.0)


def test_recorded_properties_and_interpolator_tables_match_the_fixture(kats):
    assert VisualizationRecorder._record_properties == kats["properties"] == PROPS
    assert [c.__name__ for c in VisualizationRecorder._record_interpolation_class_smoothed] == kats["smoothed"]
    assert [c.__name__ for c in VisualizationRecorder._record_interpolation_class_unsmoothed] == kats["unsmoothed"]


# ---- the conversion rule ------------------------------------------------------------------------------------
@pytest.mark.parametrize("rgb, yuv", [((0, 0, 0), (16, 128, 128)), ((255, 255, 255), (235, 128, 128)),
                                      ((128, 128, 128), (126, 128, 128)), ((255, 0, 0), (63, 102, 240)),
                                      ((0, 255, 0), (172, 42, 26)), ((0, 0, 255), (32, 240, 118))])
def test_worked_values(rgb, yuv):
    assert yuv420_ref.pixel(*rgb) == yuv


def test_every_grey_is_neutral():
    g = np.arange(256)
    u, v = yuv420_ref.chroma_of_means(g, g, g)
    assert (u == 128).all() and (v == 128).all()


def test_negative_sums_floor():
    # rounded means r = (10 + 11 + 12 + 13 + 2) >> 2 = 12, g = (803) >> 2 = 200, b = 3 >> 2 = 0
    # U: -26*12 - 86*200 + 128 = -17384, floor(-17384 / 256) = -68 (truncation: -67) -> 60
    # V: 112*12 - 102*200 + 128 = -18928, floor(-18928 / 256) = -74 (truncation: -73) -> 54
    block = np.array([[[10, 200, 0, 255], [11, 201, 1, 0]], [[12, 200, 0, 7], [13, 200, 0, 255]]], dtype=np.uint8)
    y, u, v = yuv420_ref.to_yuv420(block)
    assert (int(u[0, 0]), int(v[0, 0])) == (60, 54)
    # Y = ((47 R + 157 G + 16 B + 128) >> 8) + 16, alpha ignored: 31998 >> 8 = 124 for (10, 200, 0), 125 for the others
    assert y.tolist() == [[140, 141], [141, 141]]


def test_chroma_takes_the_rounded_mean_first():
    # R = 1, 2, 2, 1: the mean 1.5 rounds to 2 and V = ((224 + 128) >> 8) + 128 = 129; a floored mean (1) would give 128
    block = np.zeros((2, 2, 3), dtype=np.uint8)
    block[..., 0] = [[1, 2], [2, 1]]
    y, u, v = yuv420_ref.to_yuv420(block)
    assert (int(u[0, 0]), int(v[0, 0])) == (128, 129)
    assert (y == 16).all()


def test_ranges_need_no_clamp():
    g, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    lo = [255, 255, 255]
    hi = [0, 0, 0]
    for r in range(256):
        rgb = np.stack([np.full_like(g, r), g, b], axis=-1)
        ys = ((47 * rgb[..., 0] + 157 * rgb[..., 1] + 16 * rgb[..., 2] + 128) >> 8) + 16      # unclamped
        u = ((-26 * r - 86 * g + 112 * b + 128) >> 8) + 128
        v = ((112 * r - 102 * g - 10 * b + 128) >> 8) + 128
        for k, a in enumerate((ys, u, v)):
            lo[k], hi[k] = min(lo[k], int(a.min())), max(hi[k], int(a.max()))
    assert (lo[0], hi[0]) == (16, 235)
    assert lo[1] >= 16 and hi[1] <= 240 and lo[2] >= 16 and hi[2] <= 240


# ---- a stub visualizer ----------------------------------------------------------------------------------------
class StubColormap:
    def __init__(self, **params):
        self.params = dict(params)
        self.sets = []

    def __getitem__(self, key):
        return self.params.get(key, None)

    def __setitem__(self, key, value):
        self.sets.append((key, value))
        self.params[key] = value


class StubVisualizer:
    """The public surface the recorder uses; every frame is a deterministic function of the view state."""
    canvas_format = "rgba8unorm"

    def __init__(self):
        self.colormap = StubColormap(type="density", log=True, vmin=-1.0, vmax=2.0, colormap_name="viridis")
        self.quantity_name = None
        self.rotation_matrix = np.eye(3)
        self.scale = 10.0
        self.position_offset = np.zeros(3)
        self.show_colorbar = True
        self.show_scalebar = True
        self.listeners = []
        self.status = []
        self.rendered = []          # the state at every frame produced

    def add_frame_listener(self, callback):
        self.listeners.append(callback)

    def _produced(self):
        for cb in self.listeners:
            cb(self)

    def draw(self, reason=None):
        self._produced()

    def display_status(self, text, timeout=0.5):
        self.status.append((text, timeout))

    def state(self):
        return {"scale": self.scale, "rotation_matrix": np.array(self.rotation_matrix), "position_offset": np.array(self.position_offset),
                "vmin": self.colormap["vmin"], "vmax": self.colormap["vmax"], "quantity_name": self.quantity_name,
                "show_colorbar": self.show_colorbar, "show_scalebar": self.show_scalebar}

    def frame(self, resolution):
        W, H = resolution
        x, y = np.meshgrid(np.arange(W), np.arange(H))
        k = int(self.scale * 7) + int(1000 * self.rotation_matrix[0, 1])
        img = np.stack([(x * 3 + k) % 256, (y * 5 + 2 * k) % 256, (x * y + k) % 256, np.full_like(x, 255)], axis=-1)
        return img.astype(np.uint8)

    def get_presentation_image(self, resolution=(640, 480)):
        self.rendered.append(self.state())
        img = self.frame(resolution)
        self._produced()
        return img

    def get_presentation_image_yuv420(self, resolution=(1920, 1080)):
        self.rendered.append(self.state())
        planes = yuv420_ref.to_yuv420(self.frame(resolution))
        self._produced()
        return planes


class Clock:
    def __init__(self, t=100.0):
        self.t = t

    def __call__(self):
        return self.t


def recorded_path(vis=None):
    """Record a turn, a zoom, an offset and a vmin change at t = 0 .. 1 s (marks at 0.25 s steps)."""
    vis = vis or StubVisualizer()
    clock = Clock()
    rec = VisualizationRecorder(vis, clock=clock)
    rec.record()
    for k in range(1, 5):
        clock.t += 0.25
        a = 0.2 * k
        vis.rotation_matrix = np.array([[np.cos(a), np.sin(a), 0], [-np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
        vis.scale = 10.0 / (1 + k)
        vis.position_offset = np.array([0.5 * k, -0.25 * k, 0.0])
        if k == 2:
            vis.colormap["vmin"] = 0.5
        rec.mark()
    rec.stop()
    return vis, rec, clock


# ---- recording ------------------------------------------------------------------------------------------------
def test_record_seeds_every_property_and_every_frame_samples():
    vis = StubVisualizer()
    clock = Clock(50.0)
    rec = VisualizationRecorder(vis, clock=clock)
    vis.draw()                                          # not recording: nothing kept
    rec.record()
    assert rec.recording
    ts = rec._timestream
    assert list(ts) == PROPS
    assert all(len(v) == 1 and v[0][0] == 0.0 for v in ts.values())
    assert ts["scale"][0][1] == 10.0 and ts["colormap[vmin]"][0][1] == -1.0 and ts["colormap[gamma]"][0][1] is None
    seeded = ts["rotation_matrix"][0][1]
    vis.rotation_matrix[0, 0] = 5.0                     # values are copies
    assert seeded[0, 0] == 1.0
    clock.t += 0.5
    vis.scale = 4.0
    vis.draw()
    clock.t += 0.25
    vis.get_presentation_image((4, 2))
    clock.t += 0.25
    vis.scale = 3.0
    rec.mark()
    assert all(len(v) == 4 for v in ts.values())
    assert [t for t, _ in ts["scale"]] == [0.0, 0.5, 0.75, 1.0]
    assert [v for _, v in ts["scale"]] == [10.0, 4.0, 4.0, 3.0]
    clock.t += 1.0
    rec.stop()
    assert not rec.recording and rec._recording_ends_at == 2.0
    with pytest.raises(RuntimeError):
        rec.mark()


def test_timestream_pickle_layout_and_round_trip(tmp_path):
    vis, rec, _ = recorded_path()
    fn = str(tmp_path / "path.timestream")
    rec.save_timestream(fn)
    with open(fn, "rb") as f:
        data = pickle.load(f)
    assert isinstance(data, tuple) and len(data) == 2
    ts, ends_at = data
    assert ends_at == 1.0 and list(ts) == PROPS
    assert all(isinstance(e, tuple) and len(e) == 2 for v in ts.values() for e in v)
    other = VisualizationRecorder(StubVisualizer())
    other.load_timestream(fn)
    assert other._recording_ends_at == 1.0 and list(other._timestream) == PROPS
    assert np.array_equal(other._timestream["rotation_matrix"][-1][1], ts["rotation_matrix"][-1][1])


def test_replay_before_recording_raises():
    rec = VisualizationRecorder(StubVisualizer())
    with pytest.raises(RuntimeError):
        rec.frames()
    rec.record()                                        # frames() stops a recording first, then replays it
    assert len(list(rec.frames(fps=10, resolution=(4, 2)))) == 0


@pytest.mark.parametrize("fps, n", [(30.0, 30), (24, 24), (29.97, 29), (7.5, 7)])
def test_frame_count(fps, n):
    vis, rec, _ = recorded_path()
    frames = list(rec.frames(fps=fps, resolution=(6, 4)))
    assert len(frames) == n == int(1.0 * fps)
    assert all(f.shape == (4, 6, 3) and f.dtype == np.uint8 and f.flags.c_contiguous for f in frames)


@pytest.mark.parametrize("smooth", [False, True])
def test_interpolated_values_are_set_at_every_frame_time(smooth):
    vis, rec, _ = recorded_path()
    ts = rec._timestream
    frames = list(rec.frames(fps=8, resolution=(4, 2), smooth=smooth))
    assert len(vis.rendered) == len(frames) == 8
    if smooth:
        scale = interpolator.SmoothedLinearInterpolator(ts["scale"])
        rot = interpolator.SmoothedRotationInterpolator(ts["rotation_matrix"])
        off = interpolator.SmoothedLinearInterpolator(ts["position_offset"])
        vmin = interpolator.SmoothedStepInterpolator(ts["colormap[vmin]"])
    else:
        scale = interpolator.LinearInterpolator(ts["scale"])
        rot = interpolator.RotationInterpolator(ts["rotation_matrix"])
        off = interpolator.LinearInterpolator(ts["position_offset"])
        vmin = interpolator.StepInterpolator(ts["colormap[vmin]"])
    v = None
    for i, st in enumerate(vis.rendered):
        t = i / 8
        assert st["scale"] == scale(t)
        assert np.array_equal(st["rotation_matrix"], rot(t))
        assert np.array_equal(st["position_offset"], off(t))
        got = vmin(t)
        v = v if got is interpolator.Interpolator.no_value else got
        assert st["vmin"] == v
    assert vis.status[-2] == ("github.com/pynbody/topsy/", 1e6) and vis.status[-1][0] == "Complete"
    if not smooth:
        assert [s["vmin"] for s in vis.rendered] == [-1.0] * 4 + [0.5] * 4


def test_set_vmin_vmax_false_and_set_quantity_false_exclude_their_properties():
    vis, rec, _ = recorded_path()
    vis.colormap["vmin"] = 7.0
    vis.colormap.sets.clear()
    vis.quantity_name = "sentinel"
    list(rec.frames(fps=8, resolution=(4, 2), set_vmin_vmax=False, set_quantity=False))
    keys = {k for k, _ in vis.colormap.sets}
    assert "vmin" not in keys and "vmax" not in keys and "type" in keys and "log" in keys
    assert all(s["vmin"] == 7.0 for s in vis.rendered)
    assert vis.quantity_name == "sentinel"
    list(rec.frames(fps=8, resolution=(4, 2)))               # by default both are set
    assert {"vmin", "vmax"} <= {k for k, _ in vis.colormap.sets}
    assert vis.quantity_name is None


def test_layer_switches_are_restored_after_a_replay():
    vis, rec, _ = recorded_path()
    vis.show_colorbar, vis.show_scalebar = False, True
    list(rec.frames(fps=4, resolution=(4, 2), show_colorbar=True, show_scalebar=False))
    assert all(s["show_colorbar"] is True and s["show_scalebar"] is False for s in vis.rendered)
    assert (vis.show_colorbar, vis.show_scalebar) == (False, True)
    gen = rec.frames(fps=4, resolution=(4, 2))
    next(gen)
    gen.close()                                               # an abandoned replay restores them too
    assert (vis.show_colorbar, vis.show_scalebar) == (False, True)


def test_replay_frames_are_not_recorded():
    vis, rec, clock = recorded_path()
    before = {k: len(v) for k, v in rec._timestream.items()}
    watcher = VisualizationRecorder(vis, clock=clock)
    for _ in rec.frames(fps=8, resolution=(4, 2)):
        clock.t += 0.125
    assert {k: len(v) for k, v in rec._timestream.items()} == before and not rec.recording
    assert watcher._recording_ends_at is None


def test_bad_formats_are_refused_before_anything_renders():
    vis, rec, _ = recorded_path()
    for res in [(5, 4), (4, 3)]:
        with pytest.raises(ValueError):
            rec.frames(resolution=res, pixel_format="yuv420p")
    with pytest.raises(ValueError):
        rec.frames(resolution=(4, 4), pixel_format="bgr24")
    vis.canvas_format = "rgba16float"
    with pytest.raises(ValueError):
        rec.frames(resolution=(4, 4))
    assert vis.rendered == []


def test_progress_iterator_without_tqdm(monkeypatch):
    monkeypatch.setitem(sys.modules, "tqdm", None)
    assert VisualizationRecorder(StubVisualizer())._progress_iterator(3) == range(3)


# ---- y4m and ffmpeg ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fps, F", [(30, b"30:1"), (30.0, b"30:1"), (24, b"24:1"), (29.97, b"30000:1001")])
def test_y4m_header_bytes(fps, F):
    assert y4m_header(1920, 1080, fps) == b"YUV4MPEG2 W1920 H1080 F" + F + b" Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n"


def parse_y4m(data):
    header, rest = data.split(b"\n", 1)
    fields = header.split(b" ")
    W, H = int(fields[1][1:]), int(fields[2][1:])
    size = W * H * 3 // 2
    frames = []
    while rest:
        assert rest[:6] == b"FRAME\n"
        body, rest = rest[6:6 + size], rest[6 + size:]
        assert len(body) == size
        y = np.frombuffer(body[:W * H], np.uint8).reshape(H, W)
        u = np.frombuffer(body[W * H:W * H + size // 6], np.uint8).reshape(H // 2, W // 2)
        v = np.frombuffer(body[W * H + size // 6:], np.uint8).reshape(H // 2, W // 2)
        frames.append((y, u, v))
    return header + b"\n", frames


@pytest.mark.parametrize("fps", [30, 24, 29.97])
def test_save_y4m_writes_header_markers_and_planes_in_order(tmp_path, fps):
    vis, rec, _ = recorded_path()
    fn = tmp_path / "m.y4m"
    rec.save_y4m(str(fn), fps, (10, 6), smooth=False)
    header, frames = parse_y4m(fn.read_bytes())
    assert header == y4m_header(10, 6, fps)
    assert len(frames) == int(1.0 * fps) == len(vis.rendered)
    rgb = list(rec.frames(fps, (10, 6), smooth=False))
    for (y, u, v), want in zip(frames, rgb):
        wy, wu, wv = yuv420_ref.to_yuv420(want)
        assert np.array_equal(y, wy) and np.array_equal(u, wu) and np.array_equal(v, wv)


def test_save_y4m_refuses_odd_sizes_and_writes_nothing(tmp_path):
    vis, rec, _ = recorded_path()
    fn = tmp_path / "odd.y4m"
    with pytest.raises(ValueError):
        rec.save_y4m(str(fn), 30, (11, 6))
    assert not fn.exists() and vis.rendered == []


def _stand_in(tmp_path, body):
    exe = tmp_path / "fake-ffmpeg"
    exe.write_text(f"#!{sys.executable}\nimport shutil, sys\n{body}\n")
    exe.chmod(exe.stat().st_mode | stat.S_IXUSR)
    return str(exe)


def test_save_mp4_streams_the_y4m_bytes_to_ffmpeg(tmp_path):
    exe = _stand_in(tmp_path, "assert sys.argv[1:8] == ['-y', '-loglevel', 'error', '-f', 'yuv4mpegpipe', '-i', '-']\n"
                              "assert 'bt709' in sys.argv and 'tv' in sys.argv\n"
                              "shutil.copyfileobj(sys.stdin.buffer, open(sys.argv[-1], 'wb'))")
    vis, rec, _ = recorded_path()
    rec.save_y4m(str(tmp_path / "a.y4m"), 30, (8, 6))
    rec.save_mp4(str(tmp_path / "b.mp4"), 30, (8, 6), ffmpeg=exe)
    a, b = (tmp_path / "a.y4m").read_bytes(), (tmp_path / "b.mp4").read_bytes()
    assert a == b and len(a) == len(y4m_header(8, 6, 30)) + 30 * (6 + 8 * 6 * 3 // 2)
    rec.save_mp4(str(tmp_path / "c.mp4"), 30, (8, 6), True, False, False, ffmpeg=exe)      # positional replay arguments
    rec.save_y4m(str(tmp_path / "c.y4m"), 30, (8, 6), show_colorbar=True, show_scalebar=False, smooth=False)
    assert (tmp_path / "c.mp4").read_bytes() == (tmp_path / "c.y4m").read_bytes()


def test_save_mp4_without_ffmpeg_or_with_a_failing_one(tmp_path):
    vis, rec, _ = recorded_path()
    with pytest.raises(RuntimeError, match="save_y4m"):
        rec.save_mp4(str(tmp_path / "x.mp4"), 30, (8, 6), ffmpeg=str(tmp_path / "no-such-ffmpeg"))
    exe = _stand_in(tmp_path, "sys.stdin.buffer.read(100)\nsys.stderr.write('unknown encoder: boom')\nsys.exit(3)")
    with pytest.raises(RuntimeError, match="status 3.*boom"):
        rec.save_mp4(str(tmp_path / "x.mp4"), 30, (8, 6), ffmpeg=exe)
    assert (vis.show_colorbar, vis.show_scalebar) == (True, True)
