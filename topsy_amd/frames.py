"""FrameInterface: the composed frames of VisualizerBase and of SurfaceView -- get_presentation_image /
get_presentation_image_yuv420 (the base image on a canvas of any size under the colorbar, scale bar, crosshairs and status
line of topsy_amd/overlays.py, composed on the GPU), the show_* switches, display_status and the frame listeners that let the
movie recorder (topsy_amd/recorder) sample the view state at every frame."""
from . import overlays


class FrameInterface:
    """What both classes share.  The class that uses it has _sph, _colormap, scale, quantity_name, data_loader, canvas_format
    and _render_mode (the last two name the canvas in the 4:2:0 error text), and says how its frames differ:
        _presentation_base(width, height)   the EXPORT render and the colormap state; returns what the frame's base is composed from
        _compose_frame(width, height, base, layers, yuv420)   the context's composition call for that base
        _has_colorbar()                     whether the map has a colorbar at all
        _extra_layers(width, height)        layers between the crosshairs and the status line"""
    show_status = True     # layers of get_presentation_image, the reference's defaults (visualizer.py:34,53-60)
    show_colorbar = True
    show_scalebar = True
    crosshairs_visible = False

    def _init_frames(self, position_units):
        self._colorbar = overlays.ColorbarOverlay()
        self._scalebar = overlays.ScalebarOverlay(position_units)
        self._status = overlays.StatusLine()
        self._frame_listeners = []

    def get_presentation_image(self, resolution=(640, 480)):
        """The full frame, (H, W, 4) uint8 (float16 for rgb-hdr) for resolution = (W, H): the colormapped image, or the lit
        surface, on the canvas with the colorbar, scale bar, crosshairs, simulation cube and status line on top (reference
        visualizer.py:480-491, 367-384), composed on the GPU in one call (tsp_present / tsp_present_surface)."""
        return self._present(resolution, False)

    def get_presentation_image_yuv420(self, resolution=(1920, 1080)):
        """The frame get_presentation_image(resolution) composes, as I420 planes for a movie encoder: uint8 Y (H, W), U and V
        (H/2, W/2), BT.709 limited range, converted on the GPU (tsp_present_yuv420 / tsp_present_surface_yuv420,
        include/topsy_splat.h).  W and H must be even; the rgb-hdr canvas has no 8-bit frame (ValueError)."""
        width, height = (int(v) for v in resolution)
        if width % 2 or height % 2:
            raise ValueError(f"4:2:0 frames need an even width and height, not {width} x {height}")
        if self.canvas_format != "rgba8unorm":
            raise ValueError(f"4:2:0 frames are 8-bit: the {self._render_mode} canvas ({self.canvas_format}) has none")
        return self._present(resolution, True)

    def _present(self, resolution, yuv420):
        width, height = (int(v) for v in resolution)
        if not (1 <= width <= 16384 and 1 <= height <= 16384):
            raise ValueError(f"resolution {resolution} outside 1 .. 16384 pixels per side")
        base = self._presentation_base(width, height)
        layers = self._presentation_layers(width, height)
        self._last_presentation = (base, layers)      # what the frame was composed from (tests restate it)
        out = self._compose_frame(width, height, base, layers, yuv420)
        self._frame_produced()
        return out

    def _presentation_layers(self, width, height):
        """The layers in the reference's order (visualizer.py:367-384): colorbar, scale bar, crosshairs, cube, status line."""
        layers = []
        if self.show_colorbar and self._has_colorbar():
            p = self._colormap.get_parameters()
            layers.append(self._colorbar.layer(p["vmin"], p["vmax"], p["colormap_name"], self._get_colorbar_label(), width, height))
        if self.show_scalebar:
            layers += self._scalebar.layers(self.scale, width, height)
        if self.crosshairs_visible:
            layers.append(overlays.crosshairs_layer())
        layers += self._extra_layers(width, height)
        if self.show_status:
            self._status.update(self._sph)
            layers.append(self._status.layer(width, height))
        # a canvas a few pixels high gives the colorbar figure no pixels at all: such a layer has nothing to draw
        return [L for L in layers if L["kind"] != "quad" or min(L["texture"].shape[:2]) > 0]

    def _extra_layers(self, width, height):
        return []

    def _get_colorbar_label(self):
        """The quantity's label, marked as a log10 when the map is logarithmic (reference visualizer.py:341-346)."""
        prefix = r"$\log_{10}$ " if self._colormap.get_parameter("log") else ""
        return prefix + self.data_loader.get_quantity_label(self.quantity_name)

    def display_status(self, text, timeout=0.5):
        """Show `text` in the status line of the next frames for `timeout` seconds (reference visualizer.py:426-428)."""
        self._status.display(text, timeout)

    # -- frame listeners (what the reference's view synchronizer tells the recorder) --------------
    def add_frame_listener(self, callback):
        """Call callback(self) after every frame: get_presentation_image and get_presentation_image_yuv420, and for a
        visualizer draw for any reason but REFINE and PRESENTATION_CHANGE, and get_sph_presentation_image."""
        self._frame_listeners.append(callback)

    def remove_frame_listener(self, callback):
        self._frame_listeners.remove(callback)

    def _frame_produced(self):
        for callback in list(self._frame_listeners):
            callback(self)
