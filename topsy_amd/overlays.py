"""Layers of the presentation frame: the host side of the reference's overlays (src/topsy/colorbar.py, text.py, scalebar.py,
simcube.py, line.py and the crosshairs of visualizer.py:83-94), restated for tsp_present.

Each overlay produces what tsp_present draws -- a textured quad (an RGBA float32 texture from matplotlib with its clip-space
rectangle) or a set of line segments -- as the layer dicts of _native.Context.present.  The canvas is the requested frame size
with a pixel ratio of 1.  A texture is regenerated only when its content changes (vmin / vmax / colormap name / label /
canvas height for the colorbar, the text for a text overlay), as the reference's overlays do.
"""
import logging
import math
import time

import numpy as np

logger = logging.getLogger(__name__)

STATUS_LINE_UPDATE_INTERVAL = 0.2          # seconds between frame-rate refreshes of the status line (reference config.py:8)
STATUS_LINE_UPDATE_INTERVAL_RAPID = 0.05   # ... between refreshes of a message shown with display_status (config.py:9)
TEXT_HEIGHT_PX = 40                        # logical pixel height of text overlays (visualizer.py:79, scalebar.py:139)
LINE_COLOR, LINE_WIDTH = (1.0, 1.0, 1.0, 0.3), 10.0      # crosshairs and simulation cube
WHITE = (1.0, 1.0, 1.0, 1.0)


# ------------------------------------------------------------------------------------------------ textures
def _agg_canvas(figure):
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    return FigureCanvasAgg(figure)


def text_to_rgba(text, *, dpi=200, color=WHITE):
    """`text` (mathtext allowed) drawn by matplotlib's Agg renderer on a transparent background and cropped to the pixels of
    its own bounding box: (h, w, 4) float32 in [0, 1], row 0 at the top."""
    from matplotlib.figure import Figure
    fig = Figure(figsize=(24.0, 2.0), dpi=dpi, facecolor=(0.0, 0.0, 0.0, 0.0))
    canvas = _agg_canvas(fig)
    artist = fig.text(0.005, 0.5, text, color=color, va="center", ha="left")
    canvas.draw()
    pixels = np.asarray(canvas.buffer_rgba())
    rows, cols = pixels.shape[:2]
    box = artist.get_window_extent(canvas.get_renderer())      # display units: pixels from the bottom left
    left, right = max(0, math.floor(box.x0)), min(cols, math.ceil(box.x1))
    top, bottom = max(0, rows - math.ceil(box.y1)), min(rows, rows - math.floor(box.y0))
    crop = pixels[top:max(bottom, top + 1), left:max(right, left + 1)]
    return np.ascontiguousarray(crop, dtype=np.float32) / np.float32(255.0)


def colorbar_rgba(vmin, vmax, colormap_name, label, canvas_height, *, dpi=72, aspect_ratio=0.2):
    """A vertical colorbar for [vmin, vmax] on a half-transparent white panel canvas_height pixels high and aspect_ratio times
    as wide, the bar in the left third with its ticks and label (reference colorbar.py): (h, w, 4) float32, the panel's bytes
    scaled by 1/256 as the reference scales them."""
    from matplotlib.cm import ScalarMappable
    from matplotlib.colors import Normalize
    from matplotlib.figure import Figure
    inches = canvas_height / dpi
    fig = Figure(figsize=(aspect_ratio * inches, inches), dpi=dpi, facecolor=(1.0, 1.0, 1.0, 0.5))
    canvas = _agg_canvas(fig)
    fig.colorbar(ScalarMappable(Normalize(vmin, vmax), colormap_name), cax=fig.add_axes((0.05, 0.05, 0.3, 0.9)), label=label)
    canvas.draw()
    return np.asarray(canvas.buffer_rgba(), dtype=np.float32) * np.float32(1.0 / 256.0)


# ------------------------------------------------------------------------------------------------ clip-space rectangles
def colorbar_clip(tex_shape, width, height):
    """(x0, y0, w, h): full height at the right edge, the texture's aspect ratio kept (colorbar.py:29-40)."""
    w = 2.0 * height * tex_shape[1] / tex_shape[0] / width
    return 1.0 - w, -1.0, w, 2.0


def text_clip(tex_shape, origin, logical_pixels_height, width, height):
    """(x0, y0, w, h) of a text overlay: logical_pixels_height / height tall, the texture's aspect ratio kept (text.py:19-24)."""
    return (origin[0], origin[1], logical_pixels_height * tex_shape[1] / tex_shape[0] / width, logical_pixels_height / height)


def bar_clip(x0, y0, length, height_pixels, height):
    """(x0, y0, w, h) of the scale bar (scalebar.py BarOverlay.get_clipspace_coordinates)."""
    return x0, y0, length, 2.0 * height_pixels / height


def quad(texture, clip):
    return {"kind": "quad", "texture": texture, "clip": tuple(float(v) for v in clip), "tex": (0.0, 0.0, 1.0, 1.0),
            "offsets": np.zeros((1, 2), dtype=np.float32), "weights": np.ones(1, dtype=np.float32)}


def lines(starts, ends, color, width, transform=None):
    return {"kind": "lines", "starts": np.asarray(starts, dtype=np.float32), "ends": np.asarray(ends, dtype=np.float32),
            "transform": np.eye(4, dtype=np.float32) if transform is None else np.asarray(transform, dtype=np.float32),
            "color": np.asarray(color, dtype=np.float32), "width": float(width)}


# ------------------------------------------------------------------------------------------------ scale bar length
# metres per unit: the IAU astronomical unit and the parsec it defines
_METRES = {"m": 1.0, "cm": 1e-2, "km": 1e3, "au": 1.495978707e11}
_METRES["pc"] = _METRES["au"] * 648000.0 / math.pi
_METRES["kpc"] = 1e3 * _METRES["pc"]
_METRES["Mpc"] = 1e6 * _METRES["pc"]
_METRES["Gpc"] = 1e9 * _METRES["pc"]
BAR_UNITS = ("km", "au", "pc", "kpc", "Mpc")


def round_down_125(x):
    """The largest of 1, 2 or 5 times a power of ten that is <= x (x > 0)."""
    decade = 10.0 ** math.floor(math.log10(x))
    leading = x / decade
    return (5.0 if leading >= 5.0 else 2.0 if leading >= 2.0 else 1.0) * decade


def length_label(value, unit):
    """"<value> <unit>" in plain decimals from 0.01 to 1000 (at most two decimals, no trailing zeros), as mathtext
    "$m \\times 10^{e}$ <unit>" outside that range."""
    if value == 0:
        return f"0 {unit}"
    if 0.01 <= abs(value) <= 1000:
        digits = str(int(value)) if value == int(value) else f"{value:.2f}".rstrip("0").rstrip(".")
        return f"{digits} {unit}"
    e = math.floor(math.log10(abs(value)))
    return f"${value / 10 ** e:.0f} \\times 10^{{{e}}}$ {unit}"


class BarLengthRecommender:
    """A scale-bar length for a window `window_width` base units across (reference scalebar.py BarLengthRecommender): the
    unit u of BAR_UNITS whose size makes log10(window_width / u) closest to 0.5 (the window is about three units wide), and in
    it half the window width rounded down to 1, 2 or 5 times a power of ten."""

    def __init__(self, initial_window_width_in_base_units=1.0, base_units="kpc"):
        if base_units not in _METRES:
            raise ValueError(f"unknown length unit {base_units!r}; known: {sorted(_METRES)}")
        self._unit_sizes = [_METRES[u] / _METRES[base_units] for u in BAR_UNITS]   # in base units
        self._window = None
        self.update_window_width(initial_window_width_in_base_units)

    def update_window_width(self, window_width_in_base_units):
        if window_width_in_base_units == self._window:
            return
        self._window = window_width_in_base_units
        distance = [abs(math.log10(window_width_in_base_units / size) - 0.5) for size in self._unit_sizes]
        best = min(range(len(BAR_UNITS)), key=distance.__getitem__)
        self.value_in_unit = round_down_125(window_width_in_base_units / 2.0 / self._unit_sizes[best])
        self.unit = BAR_UNITS[best]
        self.label = length_label(self.value_in_unit, self.unit)
        self.physical_scalebar_length_base_units = self.value_in_unit * self._unit_sizes[best]


# ------------------------------------------------------------------------------------------------ overlays with state
class TextOverlay:
    """Text at a clip-space origin, logical_pixels_height tall (reference text.py); the texture is redrawn when the text changes."""

    def __init__(self, text, clipspace_origin, logical_pixels_height=TEXT_HEIGHT_PX, *, dpi=200, color=WHITE):
        self.text = text
        self.clipspace_origin = clipspace_origin
        self.pixelspace_height = logical_pixels_height
        self.dpi, self.color = dpi, color
        self._texture, self._texture_for = None, None

    def texture(self):
        if self._texture_for != self.text:
            self._texture = text_to_rgba(self.text, dpi=self.dpi, color=self.color)
            self._texture_for = self.text
        return self._texture

    def clip(self, width, height):
        return text_clip(self.texture().shape, self.clipspace_origin, self.pixelspace_height, width, height)

    def layer(self, width, height):
        return quad(self.texture(), self.clip(width, height))


class ColorbarOverlay:
    """The colorbar at the right edge (reference colorbar.py); its texture follows the colormap parameters, the label and the
    canvas height."""

    def __init__(self, aspect_ratio=0.2, dpi_logical=72):
        self.aspect_ratio = aspect_ratio
        self.dpi_logical = dpi_logical
        self._texture, self._texture_for = None, None

    def texture(self, vmin, vmax, colormap_name, label, canvas_height):
        key = (vmin, vmax, colormap_name, label, canvas_height)
        if self._texture_for != key:
            self._texture = colorbar_rgba(vmin, vmax, colormap_name, label, canvas_height, dpi=self.dpi_logical,
                                          aspect_ratio=self.aspect_ratio)
            self._texture_for = key
        return self._texture

    def layer(self, vmin, vmax, colormap_name, label, width, height):
        tex = self.texture(vmin, vmax, colormap_name, label, height)
        return quad(tex, colorbar_clip(tex.shape, width, height))


class ScalebarOverlay:
    """A white bar 10 px high of a round physical length at the bottom left, its length written above it (reference
    scalebar.py ScalebarOverlay).  Position units the recommender does not know leave the frame without a scale bar (and say
    so once in the log) rather than draw a bar of the wrong length."""

    def __init__(self, position_units="kpc"):
        try:
            self._recommender = BarLengthRecommender(1.0, position_units)
        except ValueError as e:
            logger.warning(f"no scale bar: {e}")
            self._recommender = None
        self.label = TextOverlay("", (-0.9, -0.85))
        self.x0, self.y0, self.height_pixels = -0.9, -0.9, 10
        self._bar_texture = np.array(WHITE, dtype=np.float32).reshape(1, 1, 4)

    @property
    def available(self):
        return self._recommender is not None

    def bar_length(self, scale, width, height):
        """Clip-space length of the bar for a view of half-width `scale` on a width x height canvas; updates the label.  The
        square image spans the canvas width unless the canvas is taller than wide, when only width / height of it shows."""
        self._recommender.update_window_width(2.0 * scale)
        self.label.text = self._recommender.label
        return self._recommender.physical_scalebar_length_base_units / scale * max(1.0, height / width)

    def layers(self, scale, width, height):
        if not self.available:
            return []
        length = self.bar_length(scale, width, height)
        return [self.label.layer(width, height),
                quad(self._bar_texture, bar_clip(self.x0, self.y0, length, self.height_pixels, height))]


def crosshairs_layer():
    """Crosshairs through the centre (reference visualizer.py:83-94).  The reference draws them as one path through a far-off
    point (200, 200) between the horizontal and the vertical stroke, so the two joining segments are drawn as well."""
    path = np.array([(-1, 0, 0, 0), (1, 0, 0, 0), (200, 200, 0, 0), (0, 1, 0, 0), (0, -1, 0, 0)], dtype=np.float32)
    return lines(path[:-1], path[1:], LINE_COLOR, LINE_WIDTH)


def simcube_layer(periodicity_scale, sph_transform, width, height):
    """The 12 edges of the periodic box, side periodicity_scale (1 if none) centred on the origin (reference simcube.py).
    sph_transform: the row-major clip = M @ (x, y, z, 1) matrix of the SPH render; the reference's line transform,
    `transform @ sph_clipspace_to_screen_clipspace_matrix()` as uploaded to a column-major WGSL matrix, is screen_squash @ M
    in this convention."""
    side = float(periodicity_scale or 1.0)
    starts, ends = [], []
    for axis in range(3):                            # every edge joins a corner on the low face of an axis to its partner
        for corner in range(8):
            if corner >> axis & 1:
                continue
            lo = [((corner >> a & 1) - 0.5) * side for a in range(3)]
            hi = list(lo)
            hi[axis] = 0.5 * side
            starts.append(lo + [1.0])
            ends.append(hi + [1.0])
    M = screen_squash_matrix(width, height) @ np.asarray(sph_transform, dtype=np.float32)
    return lines(starts, ends, LINE_COLOR, LINE_WIDTH, M.astype(np.float32))


def screen_squash_matrix(width, height):
    """The aspect correction from the square SPH clip space to the canvas's (reference visualizer.py:407-424): the axis along
    which the canvas is shorter is stretched by the ratio of the sides."""
    return np.diag([max(1.0, height / width), max(1.0, width / height), 1.0, 1.0]).astype(np.float32)


def frame_rate_text(sph):
    """"$<fps>$ fps", then " /<f>ds" when the frame drew a 1/f sample of the particles (f > 1.1) and " /<g>gf" when its view
    selected a fraction 1/g of the volume (g > 1/0.9)."""
    parts = [f"${sph.last_render_fps:.0f}$ fps"]
    sampling = np.round(sph.last_render_mass_scale, 1)
    if sampling > 1.1:
        parts.append(f"/{sampling:.1f}ds")
    volume = sph._render_progression.get_fraction_volume_selected()
    if volume < 0.9:
        parts.append(f"/{1.0 / volume:.1f}gf")
    return " ".join(parts)


class StatusLine:
    """The status text at the top left (reference visualizer.py:426-450): "topsy" until a frame rate is known, then the frame
    rate, refreshed at most every STATUS_LINE_UPDATE_INTERVAL; a message given to display(text, timeout) replaces it until the
    timeout has passed."""

    def __init__(self):
        self.overlay = TextOverlay("topsy", (-0.9, 0.9))
        self._refreshed = 0.0
        self._message, self._message_until = None, 0.0

    @property
    def text(self):
        return self.overlay.text

    def display(self, text, timeout=0.5):
        self._message, self._message_until = text, time.time() + timeout

    def update(self, sph):
        now = time.time()
        showing_message = self._message is not None and now < self._message_until
        wanted = self._message if showing_message else (frame_rate_text(sph) if hasattr(sph, "last_render_fps") else None)
        if showing_message and wanted == self.overlay.text:
            return
        min_gap = STATUS_LINE_UPDATE_INTERVAL_RAPID if showing_message else STATUS_LINE_UPDATE_INTERVAL
        if wanted is not None and now - self._refreshed > min_gap:
            self.overlay.text = wanted
            self._refreshed = now

    def layer(self, width, height):
        return self.overlay.layer(width, height)
