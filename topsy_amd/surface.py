"""SurfaceView: surface rendering of a visualizer's scene -- the occlusion pass (sph.DepthSPHWithOcclusion), the bilateral
filter and the lit shading (colormap.surface.ColorAsSurfaceMap), what the reference's render_mode "surface" draws.

It shares the visualizer's context, particles, quantity and camera, and renders into the same device target: a later read of
the visualizer re-renders its own frame, and the other way round.

It has the frame interface of VisualizerBase -- frames.FrameInterface (the lit surface on a canvas of any size under the
colorbar, scale bar, crosshairs and status line, composed on the GPU by tsp_present_surface) and the view-state properties --
so that what is written against a visualizer's frames, topsy_amd.VisualizationRecorder included, works on a view."""
import copy

import numpy as np

from . import sph
from .colormap.surface import ColorAsSurfaceMap
from .drawreason import DrawReason
from .frames import FrameInterface


class SurfaceView(FrameInterface):
    canvas_format = "rgba8unorm"
    _render_mode = "surface"

    def __init__(self, visualizer, **colormap_params):
        if getattr(visualizer.particle_buffers.context, "n_gpus", 1) != 1:
            raise NotImplementedError("SurfaceView runs on one GPU: this visualizer shards its particles over several")
        if getattr(visualizer, "_periodic_tiling", False):
            raise NotImplementedError("SurfaceView has no periodic tiling")
        self._vis = visualizer
        self._sph = sph.DepthSPHWithOcclusion(visualizer, visualizer._render_resolution,
                                              share_render_progression=copy.copy(visualizer._sph._render_progression))
        params = {"vmin": None, "vmax": None, "weighted_average": visualizer.quantity_name is not None}
        self._colormap = ColorAsSurfaceMap(None, self._sph.get_output_texture(), "rgba8unorm", params | colormap_params)
        self._quantity = visualizer.quantity_name
        self._init_frames(visualizer.data_loader.get_position_units())
        self._sync_camera()

    def _sync_camera(self):
        v, s = self._vis._sph, self._sph
        s.rotation_matrix, s.position_offset, s.scale = v.rotation_matrix, v.position_offset, v.scale

    def _sync_quantity(self):
        """A change of the visualizer's quantity switches the material and asks for a new range, as a colormap re-initialisation does."""
        if self._vis.quantity_name != self._quantity:
            self._quantity = self._vis.quantity_name
            self._colormap.update_parameters({"weighted_average": self._quantity is not None, "vmin": None, "vmax": None})

    # -- rendering --------------------------------------------------------------------------------
    def render(self, draw_reason=DrawReason.EXPORT):
        """The occlusion pass at the visualizer's current camera and quantity."""
        self._sync_camera()
        self._sync_quantity()
        return self._sph.render(draw_reason)

    def _ensure_rendered(self):
        self._sync_quantity()
        v, s = self._vis._sph, self._sph
        same_camera = (np.array_equal(s.rotation_matrix, v.rotation_matrix) and np.array_equal(s.position_offset, v.position_offset)
                       and s.scale == v.scale)
        if not (same_camera and self._sph._target_is_mine()):
            self.render()

    def get_raw_image(self):
        """(R, R, 2) float32: (q, depth) of the front-most sphere, before the filter."""
        self._ensure_rendered()
        return self._sph.get_image()

    def get_sph_image(self):
        """(R, R, 2) float32: the bilaterally filtered (q, depth) image (what the reference's get_sph_image returns in this mode)."""
        self._ensure_rendered()
        content, _ = self._colormap.present(self._sph._context, content=True, rgba=False)
        return content

    def get_sph_presentation_image(self):
        """(R, R, 4) uint8: the lit surface; the material range is autoranged first when it is unset."""
        self.render(DrawReason.EXPORT)
        if self._colormap.get_parameter("vmin") is None or self._colormap.get_parameter("vmax") is None:
            self.colormap_autorange()
        _, rgba = self._colormap.present(self._sph._context, content=False, rgba=True)
        return rgba

    def colormap_autorange(self):
        self._colormap.autorange_vmin_vmax(self.get_raw_image())

    # -- the composed frame's base and colorbar (frames.FrameInterface; reference visualizer.py:367-384,480-491 in render_mode "surface")
    def _presentation_base(self, width, height):
        self.render(DrawReason.EXPORT)
        if self._colormap.get_parameter("vmin") is None or self._colormap.get_parameter("vmax") is None:
            self.colormap_autorange()
        return self._colormap.surface_parameters()

    def _compose_frame(self, width, height, params, layers, yuv420):
        ctx = self._sph._context
        return (ctx.present_surface_yuv420 if yuv420 else ctx.present_surface)(width, height, params, layers)

    def _has_colorbar(self):
        return self._colormap.get_parameter("weighted_average")      # only when it colours by a quantity (visualizer.py:327-328)

    # -- view state: the visualizer's ------------------------------------------------------------------
    data_loader = property(lambda self: self._vis.data_loader)

    @property
    def rotation_matrix(self):
        return self._vis.rotation_matrix

    @rotation_matrix.setter
    def rotation_matrix(self, value):
        self._vis.rotation_matrix = value

    @property
    def scale(self):
        return self._vis.scale

    @scale.setter
    def scale(self, value):
        self._vis.scale = value

    @property
    def position_offset(self):
        return self._vis.position_offset

    @position_offset.setter
    def position_offset(self, value):
        self._vis.position_offset = value

    def centre_on_pixel(self, row, col):
        """The visualizer's centre_on_pixel: (row, col) index the shared R x R image; the camera is the visualizer's."""
        return self._vis.centre_on_pixel(row, col)

    def orient(self, orient, radius, center=None, method=None):
        """The visualizer's orient: the camera is the visualizer's."""
        return self._vis.orient(orient, radius, center=center, method=method)

    def profile(self, r_max=None, **kwargs):
        """The visualizer's profile: the camera is the visualizer's."""
        return self._vis.profile(r_max, **kwargs)

    def phase_diagram(self, x, y, weight="mass", value=None, **kwargs):
        """The visualizer's phase_diagram: the particles are the visualizer's."""
        return self._vis.phase_diagram(x, y, weight=weight, value=value, **kwargs)

    def scale_to_virial(self, rho_threshold, r_max, factor=1.0):
        """The visualizer's scale_to_virial: the camera is the visualizer's."""
        return self._vis.scale_to_virial(rho_threshold, r_max, factor)

    def centre_on_halo(self, n, at="shrink"):
        """The visualizer's centre_on_halo: the camera is the visualizer's.  (The default goes through the call as it was.)"""
        return self._vis.centre_on_halo(n) if at == "shrink" else self._vis.centre_on_halo(n, at=at)

    @property
    def quantity_name(self):
        return self._vis.quantity_name

    @quantity_name.setter
    def quantity_name(self, value):
        self._vis.quantity_name = value
        self._sync_quantity()      # now, so that a range set afterwards is not taken for the old quantity's

    # -- parameters -------------------------------------------------------------------------------
    @property
    def colormap(self):
        return self._colormap

    @property
    def density_cut_percentile(self):
        return self._sph.get_density_cut_percentile()

    @density_cut_percentile.setter
    def density_cut_percentile(self, value):
        lo, hi = self._sph.get_density_cut_percentile_range()
        if not lo <= value <= hi:
            raise ValueError(f"density cut percentile {value} outside [{lo}, {hi}]")
        self._sph.set_density_cut_percentile(value)

    def __getitem__(self, key):
        return self._colormap.get_parameter(key)

    def __setitem__(self, key, value):
        self._colormap.update_parameters({key: value})
