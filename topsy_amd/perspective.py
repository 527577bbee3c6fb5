"""PerspectiveView: a visualizer's scene seen by a perspective camera, for fly-throughs.

Every render call of the library is orthographic.  To first order across each footprint, a perspective view of SPH particles is
the orthographic view of a transformed snapshot: a particle at distance d along the optical axis is drawn as if it lay on the
reference plane at distance D from the viewer -- position scaled by s = D / d, smoothing length h s, mass m s^2 -- which keeps the
vertex weight m / h^2 and with it the column density along the ray through the particle's centre (tsp_project_perspective,
include/topsy_splat.h "Perspective view").  The view keeps that transformed snapshot in a second context, written by one
streaming pass whenever the camera changes, and draws it with the unchanged pipeline at rotation = identity and offset = 0: density,
weighted quantity, rgb, depth, chunk culling and progressive blocks all work as in a visualizer.

    view = topsy_amd.PerspectiveView(vis, fov=60.0)
    view.dolly(0.5 * view.scale)                     # fly half a view width forwards
    frame = view.get_presentation_image((1920, 1080))
    rec = topsy_amd.VisualizationRecorder(view)      # records and replays fov next to the camera

The plane through the view centre fills the frame exactly as in the visualizer's orthographic view (distance = scale /
tan(fov / 2)), and fov -> 0 tends to that view.  A footprint is drawn as a disc, not as the conic it projects to: exact on the
ray through the particle's centre, and elsewhere the kernel is sampled at an impact parameter too large by at most 1 / cos(theta),
theta the ray's angle to the optical axis.  The cost is a second resident snapshot.

Out of scope: kinematic maps, spectral cubes and surface views in perspective; several GPUs; periodic tiling; fields of view of
180 degrees and more."""
import copy
import time

import numpy as np

from . import _native, overlays, particle_buffers, sph
from .drawreason import DrawReason
from .visualizer import VisualizerBase


def check_fov(fov):
    """The field of view in degrees as a float inside (0, 180), or ValueError."""
    try:
        value = float(fov)
    except (TypeError, ValueError):
        raise ValueError(f"fov must be a number of degrees inside (0, 180), not {fov!r}") from None
    if isinstance(fov, bool) or not 0.0 < value < 180.0:        # (False for NaN)
        raise ValueError(f"fov must be a number of degrees inside (0, 180), not {fov!r}")
    return value


def fov_to_distance(scale, fov):
    """The distance from the viewer to the reference plane: the plane's half-width `scale` fills the field of view."""
    return float(scale) / np.tan(np.radians(check_fov(fov)) / 2.0)


def distance_to_fov(scale, distance):
    """The field of view in degrees at which a plane of half-width `scale` at `distance` fills the frame."""
    return float(np.degrees(2.0 * np.arctan2(float(scale), float(distance))))


def _positive_or_none(name, value):
    if value is None:
        return None
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be None or a finite number > 0, not {value!r}") from None
    if isinstance(value, bool) or not (np.isfinite(v) and v > 0):
        raise ValueError(f"{name} must be None or a finite number > 0, not {value!r}")
    return v


def clip_matrix(scale, distance, near, far):
    """(M, scale_factor) of the render of the transformed snapshot: x and y at 1 / scale, view z from distance - far to
    distance - near onto clip z from 0 to 1 (the surface pass's "greater is nearer")."""
    M = np.zeros((4, 4))
    M[0, 0] = M[1, 1] = 1.0 / scale
    M[2, 2] = 1.0 / (far - near)
    M[2, 3] = -(distance - far) / (far - near)
    M[3, 3] = 1.0
    return M.astype(np.float32), np.float32(1.0 / scale)


class _PerspectiveRenderer:
    """Mixed in front of sph.SPH / RGBSPH / DepthSPH over the view's second context: a frame at a new camera (CHANGE or EXPORT,
    not REFINE) first has the view write the transformed snapshot, then draws it with the identity rotation and no offset, in whole
    strata and without the host's cell culling (the cells described world coordinates); the device's chunk culling stays on."""

    def __init__(self, view, render_resolution, wrapping=False, share_render_progression=None):
        if wrapping:
            raise NotImplementedError("PerspectiveView has no periodic tiling")
        super().__init__(view, render_resolution, wrapping, share_render_progression)
        if share_render_progression is None:
            self._render_progression.set_device_cells(None)

    def _begin_view(self, rp):
        rp.select_all()
        self._visualizer._project(self)

    def _get_transform_params(self):
        view = self._visualizer
        near, far = view.near, view.far
        if not far > near:
            raise ValueError(f"far ({far}) must be greater than near ({near})")
        return clip_matrix(self.scale, view.distance, near, far)

    def _get_depth_renderer(self):
        r = PerspectiveDepthSPH(self._visualizer, self._render_resolution, share_render_progression=copy.copy(self._render_progression))
        r.rotation_matrix, r.position_offset, r.scale = self.rotation_matrix, self.position_offset, self.scale
        return r

    def get_depth_image(self, depth_renderer_reason=DrawReason.CHANGE):
        """Density-weighted distance d from the viewer along the optical axis, in simulation units."""
        depth = self._get_depth_renderer()
        depth.render(depth_renderer_reason)
        image = depth.get_image()
        self.has_rendered = False          # the shared render target now holds the depth pass
        view = self._visualizer
        with np.errstate(divide="ignore", invalid="ignore"):
            clip_z = image[..., 1] / image[..., 0]
        return view.far - clip_z * (view.far - view.near)


class PerspectiveSPH(_PerspectiveRenderer, sph.SPH):
    pass


class PerspectiveRGBSPH(_PerspectiveRenderer, sph.RGBSPH):
    pass


class PerspectiveDepthSPH(_PerspectiveRenderer, sph.DepthSPH):
    pass


class _Scalebar(overlays.ScalebarOverlay):
    """The bar's length holds on the reference plane (the plane through the view centre) only: its label says so."""

    def bar_length(self, scale, width, height):
        length = super().bar_length(scale, width, height)
        self.label.text += " at the reference plane"
        return length


class _StatusLine(overlays.StatusLine):
    """The frame rate, then "perspective fov=<degrees>"; a displayed message stands alone."""
    _MARK = "  perspective fov="

    def __init__(self, view):
        super().__init__()
        self._view = view

    def update(self, sph_renderer):
        self.overlay.text = self.overlay.text.split(self._MARK)[0]
        super().update(sph_renderer)
        if not (self._message is not None and time.time() < self._message_until):
            self.overlay.text += f"{self._MARK}{self._view.fov:.4g}"


class PerspectiveView(VisualizerBase):
    """A visualizer of its own over the transformed snapshot: the whole interface of VisualizerBase (camera, quantity_name,
    render_mode, colormap, get_sph_image, get_sph_presentation_image, get_depth_image, the composed frames and their 4:2:0 form,
    frame listeners), with a camera of its own that starts at `visualizer`'s, plus fov, distance, near, far and dolly().  The
    data loader is the visualizer's; the particles are uploaded a second time, in the same resident order."""

    def __init__(self, visualizer, fov=60.0, near=None):
        self._fov = check_fov(fov)
        self._near = _positive_or_none("near", near)
        if getattr(visualizer.particle_buffers.context, "n_gpus", 1) != 1:
            raise NotImplementedError("PerspectiveView runs on one GPU: this visualizer shards its particles over several")
        if getattr(visualizer, "_periodic_tiling", False):
            raise NotImplementedError("PerspectiveView has no periodic tiling")
        self._far = None
        self._vis = visualizer
        self._render_resolution = visualizer._render_resolution
        self._sph = None
        self._colormap = None
        self._device_id = visualizer._device_id
        self._prevent_sph_rendering = False
        self._render_mode = visualizer.render_mode
        self.canvas_format = self._render_mode_to_canvas_format(self._render_mode)
        self.data_loader = visualizer.data_loader
        self.particle_buffers = self._second_buffers(visualizer)
        self.particle_buffers.quantity_name = visualizer.quantity_name
        self.periodicity_scale = visualizer.periodicity_scale
        self._periodic_tiling = False
        self._pending_draw = None
        self._projected = None       # the camera the second context holds the transformed snapshot of
        self.projections = 0         # tsp_project_perspective calls so far
        self._init_frames(self.data_loader.get_position_units())
        self._scalebar = _Scalebar(self.data_loader.get_position_units())
        self._status = _StatusLine(self)
        self._initialize_sph_and_colormap(visualizer.colormap.get_parameter("colormap_name"))

    @staticmethod
    def _second_buffers(visualizer):
        """The loader's snapshot once more, as the visualizer uploaded its own: same resolution, same load-time ordering."""
        ld, first = visualizer.data_loader, visualizer.particle_buffers
        second = particle_buffers.ParticleBuffers(ld, visualizer._render_resolution, visualizer._device_id,
                                                  first._max_draw_calls_per_buffer)
        if hasattr(ld, "set_density_context"):
            ld.set_density_context(first.context)           # (the loader's analysis calls stay on the visualizer's context)
        same_order = (second.context.num_particles == first.context.num_particles
                      and np.array_equal(second.context.strata_offsets(), first.context.strata_offsets()))
        if not same_order:
            second.context.close()
            raise NotImplementedError(f"PerspectiveView needs a data loader whose snapshot can be uploaded twice in one order: "
                                      f"{type(ld).__name__} gave another on the second upload")
        assert np.array_equal(second.context.strata_offsets(), first.context.strata_offsets())
        return second

    # -- the projection: called by the renderer at the start of every frame with a new camera ------------------
    def _project(self, renderer):
        src, dst = self._vis.particle_buffers, self.particle_buffers
        if renderer._mode == _native.MODE_RGB or src._have_rgb or dst._have_rgb:
            src.ensure_rgb()         # (the library wants r, g, b in both contexts or in neither)
            dst.ensure_rgb()
        rot = np.asarray(renderer.rotation_matrix, dtype=np.float32).reshape(3, 3)
        offset = np.asarray(renderer.position_offset, dtype=np.float32).reshape(3)
        distance, near = np.float32(fov_to_distance(renderer.scale, self._fov)), np.float32(self._near_for(renderer.scale))
        key = (rot.tobytes(), offset.tobytes(), float(distance), float(near), dst._have_rgb)
        if key == self._projected:
            return
        self._projected = None
        src.context.project_perspective(dst.context, rot, offset, distance, near)
        self._projected = key
        self.projections += 1

    def get_image(self):
        """The raw SPH image of the current camera, times the frame's mass scale: what the renderer's get_image() returns."""
        return self._sph.get_image()

    def _get_sph_class_for_render_mode(self, render_mode):
        return PerspectiveRGBSPH if render_mode in ("rgb", "rgb-hdr") else PerspectiveSPH

    def reset_view(self, rotation_matrix=None, position_offset=None, scale=None):
        """Back to the visualizer's current camera, where an argument is None."""
        v = self._vis
        super().reset_view(v.rotation_matrix if rotation_matrix is None else rotation_matrix,
                           v.position_offset if position_offset is None else position_offset, v.scale if scale is None else scale)
        self.invalidate()

    # -- the camera's perspective part --------------------------------------------------------------------------
    @property
    def fov(self):
        """The full field of view across the frame, in degrees, inside (0, 180)."""
        return self._fov

    @fov.setter
    def fov(self, value):
        self._fov = check_fov(value)
        self.invalidate()

    @property
    def distance(self):
        """From the viewer to the reference plane (the plane through the view centre): scale / tan(fov / 2)."""
        return fov_to_distance(self.scale, self._fov)

    def _near_for(self, scale):
        return fov_to_distance(scale, self._fov) * 1e-3 if self._near is None else self._near

    @property
    def near(self):
        """Particles nearer to the viewer than this along the optical axis are not drawn (default: distance / 1000)."""
        return self._near_for(self.scale)

    @near.setter
    def near(self, value):
        self._near = _positive_or_none("near", value)
        self.invalidate()

    @property
    def far(self):
        """Particles farther from the viewer than this are not drawn (default: distance + scale, the back face of the
        orthographic view's slab)."""
        return self.distance + self.scale if self._far is None else self._far

    @far.setter
    def far(self, value):
        self._far = _positive_or_none("far", value)
        self.invalidate()

    def dolly(self, delta):
        """Move the viewer `delta` simulation units forwards along the view axis (backwards for delta < 0): position_offset
        moves, the field of view stays.  Returns the new offset."""
        delta = float(delta)
        if not np.isfinite(delta):
            raise ValueError(f"delta must be finite, not {delta!r}")
        axis = np.asarray(self.rotation_matrix, dtype=np.float64)[2]
        self.position_offset = np.asarray(self.position_offset, dtype=np.float64) + axis * delta
        return self.position_offset

    def centre_on_pixel(self, row, col):
        """Move position_offset so that the point seen at pixel (row, col) comes to the view centre: the point on the pixel's
        ray at the distance get_depth_image() gives there, or on the reference plane where that is not finite.  Returns the
        new offset."""
        res = self._render_resolution
        row, col = int(row), int(col)
        if not (0 <= row < res and 0 <= col < res):
            raise ValueError(f"pixel ({row}, {col}) outside the {res} x {res} image")
        distance = self.distance
        d = float(self.get_depth_image()[row, col])
        if not np.isfinite(d):
            d = distance
        plane = np.array([((col + 0.5) * 2.0 / res - 1.0) * self.scale, (1.0 - (row + 0.5) * 2.0 / res) * self.scale])
        view = np.array([plane[0] * d / distance, plane[1] * d / distance, distance - d])
        self.position_offset = np.asarray(self.position_offset, dtype=np.float64) - np.asarray(self.rotation_matrix).T @ view
        return self.position_offset

    # -- the quantity: the visualizer's follows -----------------------------------------------------------------
    @property
    def quantity_name(self):
        return self.particle_buffers.quantity_name

    @quantity_name.setter
    def quantity_name(self, value):
        VisualizerBase.quantity_name.fset(self, value)
        self._vis.quantity_name = value
