"""Kinematic frames without a GPU: the numpy restatement of the moment bases (tests/kinematic_present_ref.py) on hand-made images
that take every branch of the moment rule, the float64 percentile from order statistics against the host rules of
topsy_amd/kinematics.py, and the host logic of VelocityFrames (parameters, colorbar, autorange, the recorder) against a fake
context."""
import os
import re

import numpy as np
import pytest

import kinematic_present_ref as kref
import kinematics_ref
from oracle import oracle_np
from topsy_amd import kinematics
from topsy_amd.colormap.implementation import percentile_f64_from_order_statistics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
CASES = ("plain", "empty", "negative S", "S = 0", "nan", "inf A", "clamp", "A = 0", "noise")
LIT = (2, 1)        # (row, column) of the lone lit pixel in the empty corner of hand_made_image (R >= 16)


def hand_made_image(R, seed=5):
    """(image (R, R, 4) float32 of sums (S, A, B, n), case (R, R) int: the index into CASES of every pixel).  About a third of the
    pixels take one of the special branches of the moment rule; the corner of side R // 4 is empty but, where R >= 16, for the one
    lit pixel LIT."""
    rs = np.random.RandomState(seed)
    S = np.exp(rs.uniform(-4, 4, (R, R))).astype(f32)
    mean = rs.normal(0, 200, (R, R))
    sig = np.exp(rs.uniform(-3, 6, (R, R)))
    img = np.empty((R, R, 4), dtype=f32)
    img[..., 0] = S
    img[..., 1] = (S * mean).astype(f32)
    img[..., 2] = (S * (mean * mean + sig * sig)).astype(f32)
    img[..., 3] = rs.randint(1, 1000, (R, R))
    case = rs.randint(1, 3 * len(CASES), (R, R))
    case[case >= len(CASES)] = 0
    which = rs.randint(0, 3, (R, R))
    corner = R // 4
    case[:corner, :corner] = 1
    if R >= 16:
        case[LIT] = 0
    img[case == 1] = 0.0
    img[case == 2, 0] *= f32(-1.0)
    img[case == 3, 0] = 0.0
    for c in range(3):
        img[(case == 4) & (which == c), c] = np.nan
    img[case == 5, 1] = np.inf
    img[case == 6, 2] *= f32(0.5)                           # B / S < mean^2 for most: clamped
    img[case == 7, 1] = 0.0
    noise = case == 8                                       # var = rounding noise of either sign
    img[noise, 2] = (img[noise, 1].astype(np.float64) ** 2 / img[noise, 0]).astype(f32)
    return img, case


def make_lut(n=257, seed=8):
    return np.random.RandomState(seed).uniform(0, 1, (n, 4)).astype(f32)


BASES = [{"map": "moment-mean", "lut": make_lut(), "vmin": -300.0, "vmax": 300.0, "log": False},
         {"map": "moment-sigma", "lut": make_lut(), "vmin": 0.5, "vmax": 400.0, "log": False},
         {"map": "moment-sigma", "lut": make_lut(64, 3), "vmin": -1.0, "vmax": 2.5, "log": True}]


def base_id(base):
    return base["map"] + (" log" if base["log"] else "")


# --------------------------------------------------------------------------- the reference itself
def test_the_hand_made_image_takes_every_branch():
    img, case = hand_made_image(64)
    assert all((case == k).sum() >= 20 for k in range(len(CASES))), [(CASES[k], int((case == k).sum())) for k in range(len(CASES))]
    maps = kinematics_ref.velocity_moments(img)
    mean, sigma = maps[..., 1], maps[..., 2]
    for k in (1, 2, 3, 4, 5):
        assert np.isnan(mean[case == k]).all() and np.isnan(sigma[case == k]).all(), CASES[k]
    for k in (0, 6, 7, 8):
        assert np.isfinite(mean[case == k]).all() and np.isfinite(sigma[case == k]).all(), CASES[k]
    assert (sigma[case == 6] == 0).sum() > (case == 6).sum() // 2               # the clamp
    assert (mean[case == 7] == 0).all()
    assert (sigma[case == 8] == 0).any() and (sigma[case == 8] > 0).any()        # the noise of either sign


@pytest.mark.parametrize("base", BASES, ids=base_id)
@pytest.mark.parametrize("R", [64, 33])
def test_square_base_is_the_colormap_of_the_moment_maps(R, base):
    img, case = hand_made_image(R)
    got = kref.base_layer(img, R, R, base)
    which = kref.CHANNEL[base["map"]]
    value = np.stack([kinematics_ref.velocity_moments(img)[..., which], np.zeros((R, R), dtype=f32)], axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = oracle_np.colormap_scalar(value, base["lut"], base["vmin"], base["vmax"], base["log"], False)
    assert got.shape == (R, R, 4) and got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(kref.compose(img, R, R, base), want)
    # a pixel without a moment takes the colour of vmin: the first entry of the table
    at_vmin = oracle_np._unorm8(np.asarray(base["lut"], dtype=f32)[:1])[0]
    assert (got[np.isin(case, (1, 2, 3, 4, 5))] == at_vmin).all()
    assert (got[case == 0] != at_vmin).any()


def test_a_lone_lit_pixel_under_magnification_keeps_its_mean():
    """Sampling the sums and dividing afterwards: every canvas pixel the lit texel reaches has the lit pixel's own mean and
    dispersion (to the rounding of the interpolation), however small its share of S; interpolating the maps would give NaN."""
    R, mag = 64, 4
    img, _ = hand_made_image(R)
    lit = kinematics_ref.velocity_moments(img)[LIT]
    assert np.isfinite(lit[1]) and lit[2] > 0
    W = R * mag
    mean = kref.moment_canvas(img, W, W, "moment-mean")
    sigma = kref.moment_canvas(img, W, W, "moment-sigma")
    r0, c0 = LIT[0] * mag, LIT[1] * mag
    block = (slice(r0 - mag // 2, r0 + mag + mag // 2), slice(c0 - mag // 2, c0 + mag + mag // 2))     # where its bilinear weight is > 0
    assert np.isfinite(mean[block]).all() and np.isfinite(sigma[block]).all()
    assert np.allclose(mean[block], lit[1], rtol=1e-5, atol=0)
    # B / S - mean^2 cancels: the relative error of sigma^2 is the float32 rounding of the sums times (mean^2 + sigma^2) / sigma^2
    rms2 = float(lit[1]) ** 2 + float(lit[2]) ** 2
    assert (np.abs(sigma[block].astype(np.float64) ** 2 - float(lit[2]) ** 2) <= 1e-5 * rms2).all()
    ring = np.ones((W, W), dtype=bool)
    ring[block] = False
    ring[2 * R // 4 * mag:, :] = False
    ring[:, 2 * R // 4 * mag:] = False
    corner = np.zeros((W, W), dtype=bool)
    corner[:(R // 4) * mag - mag, :(R // 4) * mag - mag] = True
    assert np.isnan(mean[corner & ring]).all()                # the empty corner beyond the lit texel's reach has no moment


@pytest.mark.parametrize("W, H", [(96, 64), (64, 96), (40, 24), (17, 9), (1, 1)])
def test_reference_canvases_sample_then_divide(W, H):
    import present_ref
    img, _ = hand_made_image(33)
    s, linear = present_ref.sample_base(img, W, H)
    assert linear == (max(W, H) >= 33)
    for base in BASES[:2]:
        want = kref.colormap(kinematics_ref.velocity_moments(s)[..., kref.CHANNEL[base["map"]]], base)
        got = kref.compose(img, W, H, base)
        assert got.shape == (H, W, 4) and np.array_equal(got, want)


# --------------------------------------------------------------------------- the range from order statistics
def fetch_of(values):
    """content_values of a device sort of `values`: its finite values ascending, read by rank"""
    v = np.asarray(values, dtype=f32).ravel()
    order = np.sort(v[np.isfinite(v)])

    def fetch(ranks):
        ranks = np.asarray(ranks)
        assert ((0 <= ranks) & (ranks < len(order))).all()
        return order[ranks]
    return fetch, len(order)


class FakeContext:
    """The calls of _native.Context the kinematic view makes, on moment maps held on the host."""

    def __init__(self, maps):
        self.maps = np.asarray(maps, dtype=f32)        # (R, R, 4): (S, mean, sigma, n)
        self.calls = []
        self._fetch = None

    def moment_sort(self, which, absolute=False):
        v = self.maps[..., which]
        self.calls.append(("moment_sort", which, bool(absolute)))
        self._fetch, n = fetch_of(np.abs(v) if absolute else v)
        return n

    def content_values(self, ranks):
        return self._fetch(ranks)

    def velocity_moments(self):
        raise AssertionError("the maps are not downloaded for a range or a frame")

    def present(self, width, height, base, layers=(), timings=None):
        self.calls.append(("present", width, height, base, layers))
        return np.zeros((height, width, 4), dtype=np.uint8)

    def present_yuv420(self, width, height, base, layers=(), timings=None):
        self.calls.append(("present_yuv420", width, height, base, layers))
        return (np.zeros((height, width), dtype=np.uint8), np.zeros((height // 2, width // 2), dtype=np.uint8),
                np.zeros((height // 2, width // 2), dtype=np.uint8))


def device_ranges(values):
    ctx = FakeContext(np.stack([values] * 4, axis=-1))
    return kinematics.device_range(ctx, "v_los"), kinematics.device_range(ctx, "sigma_los")


def test_device_range_equals_the_host_rules_on_random_samples():
    rs = np.random.RandomState(17)
    for trial in range(200):
        n = int(rs.choice([1, 2, 3, 5, 17, 100, 101, 1000]))
        v = (rs.normal(0, 10.0 ** rs.uniform(-3, 3), n) + rs.normal(0, 50)).astype(f32)
        v[rs.uniform(size=n) < rs.choice([0.0, 0.1, 0.6])] = np.nan
        if trial % 7 == 0:
            v = np.abs(v)
        got_v, got_s = device_ranges(v)
        assert got_v == kinematics.v_los_range(v), (trial, n)
        assert got_s == kinematics.sigma_los_range(v), (trial, n)
        fetch, m = fetch_of(v)
        if m:
            want = np.percentile(v[np.isfinite(v)].astype(np.float64), [1.0, 99.0])
            assert np.array_equal(percentile_f64_from_order_statistics(fetch, 0, m, [1.0, 99.0]), want)
            assert percentile_f64_from_order_statistics(fetch, 0, m, 99.0) == want[1]


@pytest.mark.parametrize("values, v_range, s_range", [
    ([3.5], (-3.5, 3.5), (3.5, 4.5)),                                       # n = 1: an empty sigma range widened by 1
    ([-2.0] * 9, (-2.0, 2.0), (-2.0, -1.0)),                                # all equal
    ([np.nan] * 5, (-1.0, 1.0), (0.0, 1.0)),                                # no finite value
    ([0.0] * 99 + [np.nan], (-1.0, 1.0), (0.0, 1.0)),                       # the 99th percentile is 0
    ([0.0] * 995 + [7.0] * 5, (-1.0, 1.0), (0.0, 1.0)),                     # ... with a few values beyond it
])
def test_device_range_edge_cases(values, v_range, s_range):
    v = np.array(values, dtype=f32)
    assert kinematics.v_los_range(v) == v_range and kinematics.sigma_los_range(v) == s_range
    assert device_ranges(v) == (v_range, s_range)


def test_resolve_range_takes_the_device_rule_and_the_log_rule():
    v = np.array([1.0, 10.0, 100.0, np.nan], dtype=f32)
    auto = kinematics.sigma_los_range(v)
    assert kinematics.resolve_range("sigma_los", lambda: auto) == kinematics.resolve_range("sigma_los", v) == auto
    assert kinematics.resolve_range("sigma_los", v, vmin=2.0) == (2.0, auto[1])
    assert kinematics.resolve_range("sigma_los", v, log=True) == (float(np.log10(auto[0])), float(np.log10(auto[1])))
    assert kinematics.resolve_range("sigma_los", v, vmax=1.5, log=True) == (float(np.log10(auto[0])), 1.5)
    assert kinematics.log_range(0.0, 100.0) == (-1.0, 2.0) and kinematics.log_range(0.0, 1.0) == (-3.0, 0.0)
    assert kinematics.resolve_range("v_los", lambda: pytest.fail("not needed"), vmax=5.0) == (-5.0, 5.0)


# --------------------------------------------------------------------------- VelocityFrames against a fake context
class FakeLoader:
    def get_position_units(self):
        return "kpc"

    def get_velocities(self):
        return np.zeros((1, 3), dtype=f32)


class FakeVis:
    """The view state a VelocityFrames passes through, and a record of the analysis calls."""

    def __init__(self):
        self.data_loader = FakeLoader()
        self.rotation_matrix = np.eye(3)
        self.scale = 10.0
        self.position_offset = np.zeros(3)
        self.quantity_name = None
        self.called = []

    def orient(self, orient, radius, center=None, method=None):
        self.called.append(("orient", orient, radius, center, method))

    def centre_on_halo(self, n):
        self.called.append(("centre_on_halo", n))

    def profile(self, r_max=None, **kwargs):
        self.called.append(("profile", r_max, kwargs))

    def scale_to_virial(self, rho_threshold, r_max, factor=1.0):
        self.called.append(("scale_to_virial", rho_threshold, r_max, factor))


class FakeView(kinematics.VelocityView):
    """A VelocityView without a device: the parameters and the frame sources are the real ones."""

    def __init__(self, vis, context, **parameters):
        self._init_parameters(parameters)
        self._vis = vis
        self._sph = type("FakeSph", (), {"_context": context})()
        self._luts = {}
        self.rendered = []

    def _ensure_rendered(self):
        self.rendered.append((np.array(self._vis.rotation_matrix), self._vis.scale))


def fake_view(**parameters):
    rs = np.random.RandomState(2)
    maps = np.stack([np.ones((16, 16)), rs.normal(0, 100, (16, 16)), np.exp(rs.uniform(0, 5, (16, 16))), np.ones((16, 16))], axis=-1)
    maps[:4, :4, 1:3] = np.nan
    ctx = FakeContext(maps)
    return FakeView(FakeVis(), ctx, **parameters), ctx


def test_frames_map_the_views_parameters():
    view, ctx = fake_view(sigma_los_vmax=80.0)
    fv, fs = view.frames("v_los"), view.frames("sigma_los", label="dispersion")
    assert view.frames("v_los") is fv and view.frames("sigma_los") is fs and fs.label == "dispersion"
    with pytest.raises(ValueError):
        view.frames("speed")
    assert isinstance(fv, kinematics.VelocityFrames) and fv.canvas_format == "rgba8unorm" and fv._render_mode == "kinematic"
    assert fs.colormap["vmax"] == 80.0 and fs.colormap["vmin"] is None and fv.colormap["vmax"] is None
    assert fv.colormap["type"] == fs.colormap["type"] == "kinematic"
    assert fv.colormap["colormap_name"] == "RdBu_r" and fv.colormap["log"] is False
    for key in ("gamma", "density_vmin", "density_vmax", "weighted_average"):
        assert fv.colormap[key] is None
        fv.colormap[key] = None                         # what a replay sets for a parameter the map never had
        with pytest.raises(ValueError):
            fv.colormap[key] = 1.0
    fv.colormap["vmax"] = 120.0
    fs.colormap["vmin"], fs.colormap["colormap_name"], fs.colormap["log"] = 2.0, "magma", True
    assert view["v_los", "vmax"] == 120.0 and view["sigma_los", "vmin"] == 2.0
    assert view["sigma_los", "colormap_name"] == "magma" and view["sigma_los", "log"] is True and view.sigma_los_log is True
    fv.colormap["type"] = "kinematic"
    for bad in ("density", "rgb", "surface", None):
        with pytest.raises(ValueError):
            fv.colormap["type"] = bad
    with pytest.raises(ValueError, match="straddles 0"):
        fv.colormap["log"] = True
    with pytest.raises(ValueError, match="straddles 0"):
        view["v_los", "log"] = True
    with pytest.raises(ValueError, match="straddles 0"):
        fake_view(v_los_log=True)
    fv.colormap["log"] = False
    # the camera and the analyses are the visualizer's
    vis = view._vis
    fv.scale, fv.position_offset, fv.quantity_name = 3.0, np.ones(3), "temp"
    fv.rotation_matrix = np.diag([1.0, -1.0, -1.0])
    assert vis.scale == fs.scale == 3.0 and np.array_equal(vis.position_offset, np.ones(3)) and vis.quantity_name == "temp"
    assert np.array_equal(fs.rotation_matrix, np.diag([1.0, -1.0, -1.0])) and fs.data_loader is vis.data_loader
    fv.orient("sideon", 5.0)
    fv.centre_on_halo(2)
    fv.profile(4.0, n_bins=7)
    fv.scale_to_virial(200.0, 50.0)
    assert vis.called == [("orient", "sideon", 5.0, None, None), ("centre_on_halo", 2), ("profile", 4.0, {"n_bins": 7}),
                          ("scale_to_virial", 200.0, 50.0, 1.0)]


@pytest.mark.parametrize("kind", kinematics.KINDS)
def test_a_frame_is_composed_from_the_device_range_under_a_colorbar(kind):
    pytest.importorskip("matplotlib")
    view, ctx = fake_view()
    fr = view.frames(kind)
    fr.display_status("frame test", timeout=600)
    got = fr.get_presentation_image((160, 90))
    assert got.shape == (90, 160, 4) and len(view.rendered) >= 1
    want = kinematics.resolve_range(kind, ctx.maps[..., 1 if kind == "v_los" else 2])
    assert view.get_range(kind) == want
    name, W, H, base, layers = ctx.calls[-2] if ctx.calls[-1][0] == "moment_sort" else [c for c in ctx.calls if c[0] == "present"][-1]
    assert (name, W, H) == ("present", 160, 90)
    assert base["map"] == ("moment-mean" if kind == "v_los" else "moment-sigma") and base["log"] is False
    assert (base["vmin"], base["vmax"]) == (f32(want[0]), f32(want[1])) and base["lut"].shape == (kinematics.LUT_POINTS, 4)
    assert fr._last_presentation == (base, layers)
    assert [L["kind"] for L in layers] == ["quad", "quad", "quad", "quad"]           # colorbar, scale-bar label, bar, status
    assert fr._colormap.get_parameters() == {"type": "kinematic", "vmin": want[0], "vmax": want[1],
                                             "colormap_name": kinematics.DEFAULT_COLORMAPS[kind], "log": False}
    assert fr._get_colorbar_label() == kinematics.DEFAULT_LABELS[kind]
    fr.label = "km/s"
    assert fr._get_colorbar_label() == "km/s"
    fr.show_colorbar = False
    y, u, v = fr.get_presentation_image_yuv420((64, 48))
    assert y.shape == (48, 64) and u.shape == v.shape == (24, 32)
    assert ctx.calls[-1][:3] == ("present_yuv420", 64, 48) and len(ctx.calls[-1][4]) == 3
    with pytest.raises(ValueError, match="even"):
        fr.get_presentation_image_yuv420((63, 48))


def test_the_log_switch_marks_the_colorbar_label():
    view, _ = fake_view(sigma_los_log=True)
    fr = view.frames("sigma_los")
    assert fr._get_colorbar_label() == r"$\log_{10}$ " + kinematics.DEFAULT_LABELS["sigma_los"]
    base = fr._presentation_base(32, 32)
    lo, hi = kinematics.sigma_los_range(view._sph._context.maps[..., 2])
    assert base["log"] is True and (base["vmin"], base["vmax"]) == (f32(np.log10(lo)), f32(np.log10(hi)))


@pytest.mark.parametrize("kind", kinematics.KINDS)
def test_colormap_autorange_pins_the_ends(kind):
    view, ctx = fake_view()
    fr = view.frames(kind)
    auto = view.get_range(kind)
    view[kind, "vmax"] = 1e6                            # an end set before is replaced too
    fr.colormap_autorange()
    assert (view[kind, "vmin"], view[kind, "vmax"]) == auto
    ctx.maps[..., 1:3] *= f32(3.0)                      # the scene changes: the pinned range stays
    n_sorts = sum(c[0] == "moment_sort" for c in ctx.calls)
    assert view.get_range(kind) == auto and sum(c[0] == "moment_sort" for c in ctx.calls) == n_sorts
    view[kind, "vmin"] = view[kind, "vmax"] = None
    assert view.get_range(kind) != auto


def test_recorder_round_trip_sets_camera_and_range_and_asks_for_the_frames():
    pytest.importorskip("matplotlib")
    import topsy_amd
    view, ctx = fake_view()
    fr = view.frames("v_los")
    now = [0.0]
    rec = topsy_amd.VisualizationRecorder(fr, clock=lambda: now[0])
    quarter = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]])
    fr.colormap["vmin"], fr.colormap["vmax"] = -50.0, 50.0
    rec.record()
    now[0] = 1.0
    fr.rotation_matrix, fr.scale = quarter, 20.0
    fr.colormap["vmin"], fr.colormap["vmax"] = -150.0, 150.0
    rec.mark()
    rec.stop()
    fr.rotation_matrix, fr.scale = np.eye(3), 1.0
    fr.colormap["vmin"] = fr.colormap["vmax"] = None
    ctx.calls.clear()
    view.rendered.clear()
    frames = list(rec.frames(fps=4.0, resolution=(64, 48), smooth=False))
    assert len(frames) == 4 and all(f.shape == (48, 64, 3) and f.dtype == np.uint8 for f in frames)
    presents = [c for c in ctx.calls if c[0] == "present"]
    assert [(c[1], c[2]) for c in presents] == [(64, 48)] * 4
    assert not any(c[0] == "moment_sort" for c in ctx.calls)        # the recorded range is set: nothing is resolved
    assert [c[3]["vmax"] for c in presents] == [f32(50.0)] * 4 and [c[3]["vmin"] for c in presents] == [f32(-50.0)] * 4
    scales = [s for _, s in view.rendered]
    assert np.allclose(scales, [10.0, 12.5, 15.0, 17.5]) and len(view.rendered) == 4
    assert np.allclose(view.rendered[0][0], np.eye(3)) and not np.allclose(view.rendered[2][0], np.eye(3))
    mid = view.rendered[2][0]                                          # half of the quarter turn about x
    c = np.cos(np.pi / 4)
    assert np.allclose(mid, [[1, 0, 0], [0, c, c], [0, -c, c]], atol=1e-12)
    planes = list(rec.frames(fps=4.0, resolution=(64, 48), pixel_format="yuv420p"))
    assert len(planes) == 4 and planes[0][0].shape == (48, 64)
    assert [c[:3] for c in ctx.calls if c[0] == "present_yuv420"] == [("present_yuv420", 64, 48)] * 4


def test_binding_and_header_declare_the_kinematic_frames():
    from topsy_amd import _native
    assert (_native.PRESENT_MOMENT_MEAN, _native.PRESENT_MOMENT_SIGMA) == (4, 5) and _native.ABI_VERSION == 112
    assert "tsp_moment_sort" in _native.SIGNATURES and callable(_native.Context.moment_sort)
    header = open(os.path.join(ROOT, "include", "topsy_splat.h")).read()
    assert re.search(r"TSP_PRESENT_MOMENT_MEAN\s*=\s*4", header) and re.search(r"TSP_PRESENT_MOMENT_SIGMA\s*=\s*5", header)
    assert _native.load_library().tsp_version() >= 119
    for text in (header, open(os.path.join(ROOT, "README.md")).read(), open(os.path.join(ROOT, "DESIGN.md")).read(),
                 kinematics.__doc__):
        assert "canvas-sized frames of the maps, and the recorder" not in " ".join(text.split())
