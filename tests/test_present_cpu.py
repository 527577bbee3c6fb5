"""Frame composition without a GPU: the scale-bar length rule, the geometry of the layers at several canvas sizes, and hand-worked
cases of the numpy restatement of tsp_present (tests/present_ref.py): base-layer sampling with its linear / nearest switch at
k = 1, the top-left coverage rule of quads and lines, and blending quantised after every primitive."""
import time

import numpy as np
import pytest

import present_ref
from topsy_amd import overlays
from topsy_amd.overlays import BarLengthRecommender, length_label, round_down_125

f32 = np.float32


# ------------------------------------------------------------------------------------------------ scale-bar length
@pytest.mark.parametrize("width_kpc, unit", [(1e-6, "au"), (1e-3, "pc"), (0.01, "pc"), (100.0, "kpc"), (110000.0, "Mpc"),
                                             (2100000.0, "Mpc")])
def test_bar_length_unit_and_bound(width_kpc, unit):
    r = BarLengthRecommender(initial_window_width_in_base_units=width_kpc)
    assert r.physical_scalebar_length_base_units <= width_kpc / 2
    assert r.label.endswith(" " + unit)


@pytest.mark.parametrize("width_kpc", [1e-6, 1e-3, 0.01, 1.0, 10.0, 100.0, 1000.0, 10000.0])
def test_bar_length_is_one_two_or_five_times_a_power_of_ten(width_kpc):
    length = BarLengthRecommender(initial_window_width_in_base_units=width_kpc).value_in_unit
    mantissa = length / 10 ** np.floor(np.log10(length))
    assert min(abs(mantissa - t) for t in (1.0, 2.0, 5.0)) < 1e-10


def test_bar_length_in_other_base_units():
    r = BarLengthRecommender(base_units="au")
    r.update_window_width(1e6)          # a million au is about 4.85 pc: the bar is 2 pc
    assert 4e5 < r.physical_scalebar_length_base_units <= 5e5
    assert r.label == "2 pc"


def test_bar_length_follows_the_window():
    r = BarLengthRecommender(initial_window_width_in_base_units=1.0)
    before, label = r.physical_scalebar_length_base_units, r.label
    r.update_window_width(100.0)
    assert r.physical_scalebar_length_base_units != before and r.label != label
    assert r.physical_scalebar_length_base_units <= 50.0
    assert r.label == "50 kpc"


@pytest.mark.parametrize("value, unit, text", [(0.1, "pc", "0.1 pc"), (1.0, "pc", "1 pc"), (10.5, "kpc", "10.5 kpc"),
                                               (0.005, "pc", "$5 \\times 10^{-3}$ pc"), (0.002, "pc", "$2 \\times 10^{-3}$ pc"),
                                               (2000, "Mpc", "$2 \\times 10^{3}$ Mpc"), (0, "pc", "0 pc")])
def test_label_format(value, unit, text):
    assert length_label(value, unit) == text


def test_unknown_base_unit_is_refused():
    with pytest.raises(ValueError):
        BarLengthRecommender(base_units="furlong")


def test_unknown_position_units_leave_out_the_scale_bar(caplog):
    sb = overlays.ScalebarOverlay("furlong")
    assert not sb.available and sb.layers(100.0, 640, 480) == []
    assert "no scale bar" in caplog.text


@pytest.mark.parametrize("x, want", [(1.0, 1.0), (1.99, 1.0), (2.0, 2.0), (4.99, 2.0), (5.0, 5.0), (9.99, 5.0), (0.03, 0.02),
                                     (730.0, 500.0)])
def test_round_down_to_one_two_five(x, want):
    assert round_down_125(x) == pytest.approx(want, rel=1e-12)


def test_status_line_texts():
    class Progression:
        def get_fraction_volume_selected(self):
            return 0.5

    class Sph:
        last_render_fps, last_render_mass_scale, _render_progression = 29.6, 4.0, Progression()
    assert overlays.frame_rate_text(Sph()) == "$30$ fps /4.0ds /2.0gf"
    status = overlays.StatusLine()
    assert status.text == "topsy"
    status.update(Sph())
    assert status.text == "$30$ fps /4.0ds /2.0gf"
    status.display("hello", timeout=60)
    status.update(Sph())                     # a message waits STATUS_LINE_UPDATE_INTERVAL_RAPID after the last change
    assert status.text == "$30$ fps /4.0ds /2.0gf"
    time.sleep(overlays.STATUS_LINE_UPDATE_INTERVAL_RAPID * 1.5)
    status.update(Sph())
    assert status.text == "hello"


def test_text_texture_is_cropped_to_the_text():
    short, longer = overlays.text_to_rgba("1 kpc"), overlays.text_to_rgba("1 kpc, and more")
    assert short.dtype == np.float32 and short.shape[2] == 4 and short.shape[1] < longer.shape[1]
    assert short[..., 3].max() == 1.0 and 10 < short.shape[0] < 60
    q = short.shape[1] // 4
    assert short[:, :q, 3].max() > 0 and short[:, -q:, 3].max() > 0     # ink near both ends: no empty margin kept


# ------------------------------------------------------------------------------------------------ layer geometry
@pytest.mark.parametrize("W, H", [(640, 480), (480, 640), (1920, 1080), (1, 1)])
def test_layer_rectangles(W, H):
    # colorbar: full height, flush with the right edge, the texture's aspect ratio in pixels
    x, y, w, h = overlays.colorbar_clip((H, H // 5 or 1, 4), W, H)
    assert (y, h) == (-1.0, 2.0) and x + w == pytest.approx(1.0)
    assert (w * W / 2) / (h * H / 2) == pytest.approx((H // 5 or 1) / H)
    # text 40 logical pixels high is 20 physical pixels of the canvas (text.py: height 40 / H in clip units)
    x, y, w, h = overlays.text_clip((28, 75, 4), (-0.9, 0.9), 40, W, H)
    assert (x, y) == (-0.9, 0.9) and h * H / 2 == pytest.approx(20.0) and w * W / 2 == pytest.approx(20.0 * 75 / 28)
    # bar: 10 px high, at (-0.9, -0.9)
    x, y, w, h = overlays.bar_clip(-0.9, -0.9, 0.25, 10, H)
    assert (x, y, w) == (-0.9, -0.9, 0.25) and h * H / 2 == pytest.approx(10.0)


@pytest.mark.parametrize("W, H, expect", [(800, 800, 0.8), (1600, 800, 0.8), (800, 1600, 1.6)])
def test_scale_bar_length_in_clip_units(W, H, expect):
    sb = overlays.ScalebarOverlay("kpc")
    # a view of half-width 250 kpc (500 kpc across): the bar is 200 kpc, 0.8 of the square's half-width in clip units,
    # stretched by H / W when the canvas is taller than wide
    assert sb.bar_length(250.0, W, H) == pytest.approx(expect)
    assert sb.label.text == "0.2 Mpc"


def test_screen_squash():
    assert np.array_equal(np.diag(overlays.screen_squash_matrix(200, 100)), [1, 2, 1, 1])
    assert np.array_equal(np.diag(overlays.screen_squash_matrix(100, 200)), [2, 1, 1, 1])
    assert np.array_equal(overlays.screen_squash_matrix(100, 100), np.eye(4))


def test_crosshair_and_cube_segments():
    c = overlays.crosshairs_layer()
    assert c["starts"].shape == (4, 4) and np.array_equal(c["starts"][0], [-1, 0, 0, 0]) and np.array_equal(c["ends"][3], [0, -1, 0, 0])
    cube = overlays.simcube_layer(10.0, np.eye(4, dtype=f32), 100, 100)
    edges = np.abs(cube["ends"][:, :3] - cube["starts"][:, :3])
    assert cube["starts"].shape == (12, 4) and np.all(np.sort(edges, axis=1) == [0, 0, 10])
    assert np.all(np.abs(cube["starts"][:, :3]) == 5) and np.all(cube["starts"][:, 3] == 1)


# ------------------------------------------------------------------------------------------------ present_ref by hand
def test_base_sampling_linear_at_and_below_k_1():
    img = np.zeros((2, 2, 2), dtype=f32)
    img[..., 0] = [[0, 1], [2, 3]]
    # W = H = R: k = 1, the texel itself
    s, linear = present_ref.sample_base(img, 2, 2)
    assert linear and np.array_equal(s, img)
    # 4 x 4: k = 0.5, centres at texel coordinates 0.25, 0.75, 1.25, 1.75 -> taps (0, 0), (0, 1) f .25, (0, 1) f .75, (1, 1)
    s, linear = present_ref.sample_base(img, 4, 4)
    assert linear
    row = np.array([0, 0.25, 0.75, 1], dtype=f32)
    assert np.array_equal(s[0, :, 0], row)                      # top row: texel row 0 only
    assert np.array_equal(s[:, 0, 0], 2 * row)                  # left column: rows 0 -> 2


def test_base_sampling_nearest_above_k_1():
    img = np.zeros((4, 4, 2), dtype=f32)
    img[..., 0] = np.arange(16).reshape(4, 4)
    s, linear = present_ref.sample_base(img, 2, 2)              # k = 2: texels floor(1), floor(3)
    assert not linear and np.array_equal(s[..., 0], [[5, 7], [13, 15]])
    s, linear = present_ref.sample_base(img, 3, 3)              # k = 4/3 > 1 still nearest
    assert not linear and np.array_equal(s[..., 0], [[0, 2, 3], [8, 10, 11], [12, 14, 15]])


def test_base_sampling_wide_and_tall_canvases():
    img = np.zeros((2, 2, 2), dtype=f32)
    img[..., 0] = [[0, 1], [2, 3]]
    # 4 x 2: the square of side 4 is centred, rows 1 and 2 of it are on the canvas
    s, _ = present_ref.sample_base(img, 4, 2)
    full, _ = present_ref.sample_base(img, 4, 4)
    assert np.array_equal(s, full[1:3])
    s, _ = present_ref.sample_base(img, 2, 4)
    assert np.array_equal(s, full[:, 1:3])


def test_nonfinite_neighbour_does_not_leak_at_k_1():
    img = np.zeros((3, 3, 2), dtype=f32)
    img[1, 1] = np.nan
    s, _ = present_ref.sample_base(img, 3, 3)
    assert np.isnan(s[1, 1]).all() and not np.isnan(np.delete(s.reshape(9, 2), 4, axis=0)).any()


def constant_base(rgba=(0.2, 0.4, 0.6, 1.0)):
    return {"map": "scalar", "lut": np.array([rgba, rgba], dtype=f32), "vmin": 0.0, "vmax": 1.0, "log": False, "weighted": False}


def test_quad_top_left_rule():
    W = H = 4
    tex = np.array([[[1.0, 0.0, 0.0, 1.0]]], dtype=f32)
    # pixels X in [1.5, 3.5), Y in [0.5, 2.5): centres 1.5, 2.5 in x and 0.5, 1.5 in y are inside, 3.5 and 2.5 are not
    layer = overlays.quad(tex, (1.5 / 2 - 1, 1 - 2.5 / 2, 1.0, 1.0))
    out = present_ref.compose(np.zeros((4, 4, 2), dtype=f32), W, H, constant_base(), [layer])
    red = (out == [255, 0, 0, 255]).all(axis=-1)
    want = np.zeros((4, 4), dtype=bool)
    want[0:2, 1:3] = True
    assert np.array_equal(red, want)


def test_line_top_left_rule():
    W = H = 8
    # a horizontal line across the canvas, 6 "line.wgsl pixels" wide: its edges lie at Y = 2.5 (closed) and 5.5 (open)
    layer = overlays.lines([[-1, 0, 0, 1]], [[1, 0, 0, 1]], (0, 1, 0, 1), 6.0)
    out = present_ref.compose(np.zeros((8, 8, 2), dtype=f32), W, H, constant_base(), [layer])
    green = (out == [0, 255, 0, 255]).all(axis=-1)
    assert np.array_equal(np.where(green.all(axis=1))[0], [2, 3, 4]) and green.sum() == 24
    # drawn the other way round, the same pixels
    layer = overlays.lines([[1, 0, 0, 1]], [[-1, 0, 0, 1]], (0, 1, 0, 1), 6.0)
    out2 = present_ref.compose(np.zeros((8, 8, 2), dtype=f32), W, H, constant_base(), [layer])
    assert np.array_equal(out, out2)


def test_zero_length_segment_draws_nothing():
    layer = overlays.lines([[0, 0, 0, 1]], [[0, 0, 0, 1]], (0, 1, 0, 1), 6.0)
    base = present_ref.compose(np.zeros((8, 8, 2), dtype=f32), 8, 8, constant_base())
    assert np.array_equal(present_ref.compose(np.zeros((8, 8, 2), dtype=f32), 8, 8, constant_base(), [layer]), base)


def test_blending_is_quantised_after_every_primitive():
    base = constant_base()
    a = overlays.quad(np.array([[[1.0, 0.0, 0.3, 0.5]]], dtype=f32), (-1, -1, 2, 2))
    b = overlays.quad(np.array([[[0.1, 0.9, 0.7, 0.35]]], dtype=f32), (-1, -1, 2, 2))
    out = present_ref.compose(np.zeros((1, 1, 2), dtype=f32), 1, 1, base, [a, b])[0, 0]

    def unorm(c):
        return np.floor(np.clip(c, f32(0), f32(1)) * f32(255) + f32(0.5)).astype(np.uint8)

    def over(dst8, src):
        sa = f32(src[3])
        d = dst8.astype(f32) / f32(255)
        return unorm(np.asarray(src, dtype=f32) * sa + d * (f32(1) - sa))
    d0 = unorm(np.array([0.2, 0.4, 0.6, 1.0], dtype=f32))
    d1 = over(d0, [1.0, 0.0, 0.3, 0.5])
    d2 = over(d1, [0.1, 0.9, 0.7, 0.35])
    assert np.array_equal(out, d2)
    # blending both in float and quantising once gives another colour here: the order of quantisation is observable
    s1, s2 = np.array([1.0, 0.0, 0.3, 0.5], dtype=f32), np.array([0.1, 0.9, 0.7, 0.35], dtype=f32)
    once = unorm((s2 * s2[3] + (s1 * s1[3] + (d0.astype(f32) / f32(255)) * (1 - s1[3])) * (1 - s2[3])).astype(f32))
    assert not np.array_equal(once, d2)


def test_instances_and_weights():
    tex = np.array([[[1.0, 1.0, 1.0, 1.0]]], dtype=f32)
    layer = overlays.quad(tex, (-1, -1, 1, 1))          # the bottom-left quarter...
    layer["offsets"] = np.array([[0, 0], [1, 1]], dtype=f32)     # ...and the top-right one
    layer["weights"] = np.array([1.0, 0.5], dtype=f32)
    out = present_ref.compose(np.zeros((2, 2, 2), dtype=f32), 2, 2, constant_base((0, 0, 0, 1)), [layer])
    assert np.array_equal(out[1, 0], [255, 255, 255, 255])
    # weight 0.5 scales alpha too: 0.5 * 0.5 + 0 = 0.25 of white over black
    assert np.array_equal(out[0, 1], [64, 64, 64, 191])
    assert np.array_equal(out[0, 0], [0, 0, 0, 255]) and np.array_equal(out[1, 1], [0, 0, 0, 255])


def test_hdr_canvas_is_not_clamped():
    img = np.full((2, 2, 4), 1e4, dtype=f32)
    base = {"map": "rgb-hdr", "vmin": 0.0, "vmax": 2.0, "gamma": 1.0}
    out = present_ref.compose(img, 2, 2, base)
    assert out.dtype == np.float16 and np.all(out[..., :3] == np.float16(2.0)) and np.all(out[..., 3] == 1)
    layer = overlays.quad(np.array([[[4.0, 0.0, 0.0, 0.5]]], dtype=f32), (-1, -1, 2, 2))
    out = present_ref.compose(img, 2, 2, base, [layer])
    assert np.all(out[..., 0] == np.float16(3.0)) and np.all(out[..., 1] == np.float16(1.0))
