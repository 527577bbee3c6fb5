"""ColorAsSurfaceMap: the lit-surface presentation of the occlusion pass (mirror of reference src/topsy/colormap/surface.py).

The bilateral filter of the (q, depth) image and the shading run on the device (tsp_surface_present; tsp_present_surface for a
canvas-sized frame under the overlays); this class holds the parameters, the material LUT and the autorange.  ColormapHolder does
not select it yet (render_mode "surface" is not wired into the visualizer): topsy_amd.SurfaceView owns one."""
import numpy as np

from .. import config
from .implementation import Colormap


class ColorAsSurfaceMap(Colormap):
    _default_params = {
        "type": "surface",
        "depth_scale": 1.0,
        "light_direction": [0.0, 1.0 / np.sqrt(2.0), 1.0 / np.sqrt(2.0)],
        "light_color": [1.0, 1.0, 1.0],
        "ambient_color": [0.0, 0.0, 0.2],
        "smoothing_scale": 0.01,
        "weighted_average": False,
        "vmin": 0.0,
        "vmax": 1.0,
        "log": False,
        "colormap_name": config.DEFAULT_COLORMAP,
    }

    @classmethod
    def accepts_parameters(cls, parameters):
        return False      # not selectable by ColormapHolder (see the module docstring)

    def update_parameters(self, parameters):
        if parameters.get("type", "surface") != "surface":
            raise ValueError(f"ColorAsSurfaceMap does not accept parameter update: {parameters}")
        self._params.update(parameters)
        self._setup_map_texture()

    def autorange_vmin_vmax(self, vals):
        """From the RAW (q, depth) image: the quantity where a sphere was drawn (reference surface.py:250-253)."""
        valid = vals[..., 1].ravel() > 0.0
        self._autorange_using_values(vals[..., 0].ravel()[valid])

    def filter_parameters(self, resolution):
        """(spatial sigma, range sigma, kernel size) as the reference forms them (surface.py:259-273): float32 sigmas from the
        float64 products, kernel size from the float32 spatial sigma, capped at MAX_SURFACE_SMOOTH_PIXELS."""
        sig = self._params.get("smoothing_scale", 0.01)
        if sig < 1e-5:
            sig = 1e-5
        ss = np.float32(sig * resolution)
        rs = np.float32(sig * 2)
        n_pix = min(int(ss * np.float32(4)) + 1, config.MAX_SURFACE_SMOOTH_PIXELS)
        return ss, rs, n_pix

    def surface_parameters(self):
        """The keywords of _native.Context.surface_present / present_surface for the current parameters."""
        p = self._params
        return dict(smoothing_scale=p.get("smoothing_scale", 0.01), depth_scale=p.get("depth_scale", 1.0),
                    light_direction=p.get("light_direction", [0.0, 0.0, 1.0]), light_color=p.get("light_color", [1.0, 1.0, 1.0]),
                    ambient_color=p.get("ambient_color", [0.2, 0.2, 0.2]), vmin=p["vmin"], vmax=p["vmax"],
                    weighted_average=p["weighted_average"], log=p["log"], lut_rgba=self._lut)

    def present(self, context, content=True, rgba=True, timings=None):
        """Filter the context's (q, depth) image and shade it: (filtered (R, R, 2) float32 or None, (R, R, 4) uint8 or None)."""
        return context.surface_present(content=content, rgba=rgba, timings=timings, **self.surface_parameters())

    def __getitem__(self, key):
        return self.get_parameter(key)

    def __setitem__(self, key, value):
        self.update_parameters({key: value})
