"""SurfaceView: surface rendering of a visualizer's scene -- the occlusion pass (sph.DepthSPHWithOcclusion), the bilateral
filter and the lit shading (colormap.surface.ColorAsSurfaceMap), what the reference's render_mode "surface" draws.

It shares the visualizer's context, particles, quantity and camera, and renders into the same device target: a later read of
the visualizer re-renders its own frame, and the other way round."""
import copy

import numpy as np

from . import sph
from .colormap.surface import ColorAsSurfaceMap
from .drawreason import DrawReason


class SurfaceView:
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
