"""VelocityView: the kinematic maps of a visualizer's scene -- per pixel the mass-weighted mean line-of-sight velocity and its
dispersion, the picture that goes with vis.profile's rotation curve (pynbody: image(qty="vz", av_z=True) after sideon).

It shares the visualizer's context, particles and camera, and renders into the same device target (sph.KinematicSPH,
MODE_KINEMATIC): a later read of the visualizer re-renders its own frame, and the other way round.  The line of sight is the view
axis, rotation_matrix[2]; after vis.orient("sideon", r) v_los shows the disc's rotation.

view.frames(kind) is the map as a frame source, VelocityFrames: frames.FrameInterface (the map on a canvas of any size under its
colorbar, the scale bar, crosshairs and status line, composed on the GPU by tsp_present's moment bases) and the view-state
properties, so that what is written against a visualizer's frames, topsy_amd.VisualizationRecorder included, works on it.  The
automatic colour range comes from a device sort of the map (tsp_moment_sort): a handful of values are read back per frame, not the
maps.

Out of scope: several GPUs (MultiGpuContext, tsp_group_*: no sharded velocities) and periodic tiling."""
import copy

import numpy as np

from . import _native, config, kernel_lut, loader, particle_buffers, sph
from .drawreason import DrawReason
from .frames import FrameInterface

KINDS = ("v_los", "sigma_los")
DEFAULT_COLORMAPS = {"v_los": "RdBu_r", "sigma_los": config.DEFAULT_COLORMAP}      # diverging about 0; the density default
DEFAULT_LABELS = {"v_los": r"$v_{\rm los}$", "sigma_los": r"$\sigma_{\rm los}$"}
PARAMETERS = ("vmin", "vmax", "colormap_name", "log")
LUT_POINTS = 1000
_WHICH = {"v_los": 1, "sigma_los": 2}       # the channel of tsp_velocity_moments' maps
_PRESENT_MAP = {"v_los": "moment-mean", "sigma_los": "moment-sigma"}        # the base of Context.present


def check_v_ref(v_ref):
    """v_ref of VelocityView / velocity_maps: "center", None (zero) or three finite components -> "center" or float64 (3,)."""
    if isinstance(v_ref, str):
        if v_ref != "center":
            raise ValueError(f"v_ref must be 'center', None or three finite components, not {v_ref!r}")
        return v_ref
    if v_ref is None:
        return np.zeros(3)
    try:
        v = np.asarray(v_ref, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"v_ref must be 'center', None or three finite components, not {v_ref!r}") from None
    if v.shape != (3,) or not np.isfinite(v).all():
        raise ValueError(f"v_ref must be 'center', None or three finite components, not {v_ref!r}")
    return v.copy()


def check_kind(kind):
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}, not {kind!r}")
    return kind


def v_los_range(v_los):
    """The default range of the v_los map: symmetric about 0, out to the 99th percentile of |v_los| over the finite pixels
    ((-1, 1) where there is none, or where that percentile is 0)."""
    v = np.asarray(v_los, dtype=np.float64)
    v = np.abs(v[np.isfinite(v)])
    top = float(np.percentile(v, 99.0)) if v.size else 0.0
    top = top if top > 0.0 else 1.0
    return -top, top


def sigma_los_range(sigma_los):
    """The default range of the sigma_los map: the 1st to the 99th percentile over the finite pixels ((0, 1) where there is none;
    an empty range is widened by 1 upward)."""
    s = np.asarray(sigma_los, dtype=np.float64)
    s = s[np.isfinite(s)]
    if not s.size:
        return 0.0, 1.0
    lo, hi = (float(v) for v in np.percentile(s, [1.0, 99.0]))
    return (lo, hi) if hi > lo else (lo, lo + 1.0)


def log_range(lo, hi):
    """The ends of an automatic range for a logarithmic map, which compares log10 of the value with vmin and vmax: log10 of the
    linear ends; a lower end that has no logarithm lies 3 dex below the upper one."""
    hi = float(np.log10(hi)) if hi > 0.0 else 0.0
    lo = float(np.log10(lo)) if lo > 0.0 else hi - 3.0
    return (lo, hi) if hi > lo else (lo, lo + 1.0)


def device_range(context, kind):
    """v_los_range / sigma_los_range of the context's kinematic image, to the bit, from a device sort of the map (moment_sort) and
    the few order statistics numpy's float64 percentile reads (content_values)."""
    from .colormap.implementation import percentile_f64_from_order_statistics
    n = context.moment_sort(_WHICH[check_kind(kind)], absolute=kind == "v_los")
    if kind == "v_los":
        top = float(percentile_f64_from_order_statistics(context.content_values, 0, n, 99.0)) if n else 0.0
        top = top if top > 0.0 else 1.0
        return -top, top
    if not n:
        return 0.0, 1.0
    lo, hi = (float(v) for v in percentile_f64_from_order_statistics(context.content_values, 0, n, [1.0, 99.0]))
    return (lo, hi) if hi > lo else (lo, lo + 1.0)


def resolve_range(kind, values, vmin=None, vmax=None, log=False):
    """(vmin, vmax) of a map: what was set, the rest from the default rule of its kind; a v_los range with only one end set is
    symmetric about 0.  `values`: the map, or a callable that returns the default rule's range (the device's).  log: the map is
    logarithmic (sigma_los only), so the automatic ends are log_range's."""
    check_kind(kind)
    if vmin is None or vmax is None:
        if kind == "v_los" and (vmin is None) != (vmax is None):
            auto = (-float(vmax), None) if vmin is None else (None, -float(vmin))
        else:
            auto = values() if callable(values) else (v_los_range if kind == "v_los" else sigma_los_range)(values)
            auto = log_range(*auto) if log else auto
        vmin = auto[0] if vmin is None else vmin
        vmax = auto[1] if vmax is None else vmax
    vmin, vmax = float(vmin), float(vmax)
    if not (np.isfinite(vmin) and np.isfinite(vmax)):
        raise ValueError(f"the range of the {kind} map must be finite, not ({vmin}, {vmax})")
    return vmin, vmax


def maps_dict(maps, mass_scale=1.0):
    """(R, R, 4) (S, mean, sigma, n) of Context.velocity_moments -> the dict of get_maps: only the surface density scales with
    the fraction of the particles a progressive frame drew."""
    return {"surface_density": maps[..., 0] * np.float32(mass_scale), "v_los": maps[..., 1].copy(),
            "sigma_los": maps[..., 2].copy(), "count": maps[..., 3].copy()}


class VelocityView:
    def __init__(self, visualizer, v_ref="center", **parameters):
        if getattr(visualizer.particle_buffers.context, "n_gpus", 1) != 1:
            raise NotImplementedError("VelocityView runs on one GPU: this visualizer shards its particles over several")
        if getattr(visualizer, "_periodic_tiling", False):
            raise NotImplementedError("VelocityView has no periodic tiling")
        if getattr(visualizer.data_loader, "get_velocities", lambda: None)() is None:
            raise ValueError(f"{type(visualizer.data_loader).__name__} has no velocities: VelocityView needs "
                             f"from_arrays(..., vel=vel)")
        self._v_ref_option = check_v_ref(v_ref)
        self._v_ref_cache = None            # (centre, scale, v_cen) of the last "center"
        self._init_parameters(parameters)
        self._vis = visualizer
        self._sph = sph.KinematicSPH(visualizer, visualizer._render_resolution,
                                     share_render_progression=copy.copy(visualizer._sph._render_progression))
        self._luts = {}
        self._sync_camera()

    def _init_parameters(self, parameters):
        self._params = {kind: {"vmin": None, "vmax": None, "colormap_name": DEFAULT_COLORMAPS[kind], "log": False} for kind in KINDS}
        self._frames = {}
        for key, value in parameters.items():       # v_los_vmax=..., sigma_los_colormap_name=...
            if key not in self._parameter_names():
                raise ValueError(f"unknown parameter {key!r}: one of {sorted(self._parameter_names())}")
            setattr(self, key, value)

    # -- camera and reference velocity: the visualizer's -----------------------------------------------
    def _camera(self):
        v = self._vis._sph
        return v.rotation_matrix, v.position_offset, v.scale

    def _current_v_ref(self):
        """v_ref for the visualizer's current camera.  "center": the mean velocity v_cen of the inner fifth of the sphere of
        radius vis.scale about -position_offset (tsp_sphere_moments), the rule vis.profile uses for its own v_cen."""
        if not isinstance(self._v_ref_option, str):
            return self._v_ref_option
        _, offset, scale = self._camera()
        center = -np.asarray(offset, dtype=np.float64)
        if self._v_ref_cache is None or not (np.array_equal(self._v_ref_cache[0], center) and self._v_ref_cache[1] == scale):
            ld = self._vis.data_loader
            pos, mass, vel = loader.check_moments_arrays(ld.get_positions(), ld.get_mass(), ld.get_velocities())
            c, r, r_vel = loader.check_moments_arguments(center, scale, None, True)
            v_cen = ld._with_context(lambda ctx: loader.compute_moments(ctx, pos, mass, vel, c, r, r_vel))["v_cen"]
            if not np.isfinite(v_cen).all():
                raise ValueError(f"v_ref='center': no particle within {r_vel} of {center} to take the mean velocity from; "
                                 f"pass v_ref as three components")
            self._v_ref_cache = (center.copy(), scale, np.asarray(v_cen, dtype=np.float64))
        return self._v_ref_cache[2]

    def _sync_camera(self):
        s = self._sph
        s.rotation_matrix, s.position_offset, s.scale = self._camera()
        s.v_ref = self._current_v_ref()

    @property
    def v_ref(self):
        """The velocity subtracted before the moments are formed (float64 (3,)), at the visualizer's current camera."""
        return np.array(self._current_v_ref(), dtype=np.float64)

    @v_ref.setter
    def v_ref(self, value):
        self._v_ref_option = check_v_ref(value)
        self._v_ref_cache = None

    # -- rendering --------------------------------------------------------------------------------------
    def render(self, draw_reason=DrawReason.EXPORT):
        """The kinematic frame at the visualizer's current camera."""
        self._sync_camera()
        return self._sph.render(draw_reason)

    def needs_refine(self):
        return self._sph.needs_refine()

    def _ensure_rendered(self):
        s = self._sph
        rotation, offset, scale = self._camera()
        same = (np.array_equal(s.rotation_matrix, rotation) and np.array_equal(s.position_offset, offset) and s.scale == scale
                and np.array_equal(s.v_ref, self._current_v_ref()))
        if not (same and s._target_is_mine()):
            self.render()

    def get_raw_image(self):
        """(R, R, 4) float32: the sums (S, A, B) and the fragment count n, unscaled."""
        self._ensure_rendered()
        return self._sph._get_image_unscaled()

    def get_maps(self):
        """dict of (R, R) float32: surface_density (times the frame's mass scale), v_los (the mean of (v - v_ref) along the view
        axis), sigma_los, count; v_los and sigma_los are NaN where nothing was drawn."""
        self._ensure_rendered()
        return maps_dict(self._sph._context.velocity_moments(), self._sph.last_render_mass_scale)

    def phase_diagram(self, x, y, weight="mass", value=None, **kwargs):
        """The visualizer's phase_diagram: the particles are the visualizer's."""
        return self._vis.phase_diagram(x, y, weight=weight, value=value, **kwargs)

    def get_cube(self, v_range=None, n_channels=64, sigma_v=0.0, sigma=None):
        """The spectral cube of the scene at the visualizer's camera and this view's v_ref (topsy_amd.SpectralCube: data
        (n_channels, R, R), v_edges, moment(), spectrum(), pv()): per pixel the whole distribution of the line-of-sight velocity
        that v_los and sigma_los summarise, every particle drawn once in one pass (tsp_spectral_cube).  v_range: (v_min, v_max), or
        None for (-V, V) with V = max |u| over the loader's finite velocities plus 5 times the largest line width.  A particle's
        line is a Gaussian of width sqrt(sigma_v^2 + sigma[i]^2) integrated over each channel; sigma: per particle, in the
        loader's order, or None.  The view's own frame stays as it is."""
        from . import spectral
        return spectral.view_cube(self, v_range=v_range, n_channels=n_channels, sigma_v=sigma_v, sigma=sigma)

    def _lut(self, name):
        if name not in self._luts:
            from .colormap.implementation import _lut_from_matplotlib
            self._luts[name] = _lut_from_matplotlib(name, LUT_POINTS)
        return self._luts[name]

    def get_range(self, kind):
        """(vmin, vmax) get_presentation_image(kind) maps: what was set, else the default rule on the current maps -- exactly
        resolve_range(kind, get_maps()[kind], ...), taken from a sort of the map on the device (device_range): the maps are not
        downloaded."""
        p = self._params[check_kind(kind)]

        def automatic():
            self._ensure_rendered()
            return device_range(self._sph._context, kind)
        return resolve_range(kind, automatic, p["vmin"], p["vmax"], p["log"])

    def get_presentation_image(self, kind="v_los"):
        """(R, R, 4) uint8: the map `kind` ("v_los": a diverging colormap over a range symmetric about 0, out to the 99th percentile
        of |v_los|; "sigma_los": the density colormap from the 1st to the 99th percentile) -- view[kind, "vmin"], "vmax" and
        "colormap_name" override; with view["sigma_los", "log"] the map is of log10(sigma_los) and the ends are logarithms.  Pixels
        without a value (NaN) take the colour of vmin.  The map on a canvas of any size, under a colorbar: frames(kind)."""
        vmin, vmax = self.get_range(kind)
        self._ensure_rendered()
        return self._sph._context.colormap_moment(_WHICH[kind], self._lut(self._params[kind]["colormap_name"]),
                                                  np.float32(vmin), np.float32(vmax), self._params[kind]["log"])

    def frames(self, kind="v_los", label=None):
        """The map `kind` as a frame source (VelocityFrames, one per kind): get_presentation_image((W, H)) with colorbar and
        scale bar, the 4:2:0 planes, and what topsy_amd.VisualizationRecorder needs.  label: the colorbar's label, when given."""
        if check_kind(kind) not in self._frames:
            self._frames[kind] = VelocityFrames(self, kind)
        if label is not None:
            self._frames[kind].label = label
        return self._frames[kind]

    # -- parameters: view["v_los", "vmax"] = 250.0, or view.v_los_vmax = 250.0 ----------------------------
    @staticmethod
    def _parameter_names():
        return {f"{kind}_{name}" for kind in KINDS for name in PARAMETERS}

    @staticmethod
    def _check_key(key):
        if not (isinstance(key, tuple) and len(key) == 2 and key[0] in KINDS and key[1] in PARAMETERS):
            raise KeyError(f"parameters are (kind, name) with kind in {KINDS} and name in {PARAMETERS}, not {key!r}")
        return key

    def __getitem__(self, key):
        kind, name = self._check_key(key)
        return self._params[kind][name]

    def __setitem__(self, key, value):
        kind, name = self._check_key(key)
        if name == "colormap_name":
            if not isinstance(value, str):
                raise ValueError(f"colormap_name must be a matplotlib colormap's name, not {value!r}")
        elif name == "log":
            value = bool(value)
            if value and kind == "v_los":
                raise ValueError("the v_los map has no logarithmic form: its range straddles 0")
        elif value is not None:
            value = float(value)
            if not np.isfinite(value):
                raise ValueError(f"{kind} {name} must be None (automatic) or finite, not {value!r}")
        self._params[kind][name] = value

    # -- view state: the visualizer's ---------------------------------------------------------------------
    data_loader = property(lambda self: self._vis.data_loader)
    rotation_matrix = property(lambda self: self._vis.rotation_matrix, lambda self, v: setattr(self._vis, "rotation_matrix", v))
    scale = property(lambda self: self._vis.scale, lambda self, v: setattr(self._vis, "scale", v))
    position_offset = property(lambda self: self._vis.position_offset, lambda self, v: setattr(self._vis, "position_offset", v))

    def orient(self, orient, radius, center=None, method=None):
        """The visualizer's orient: the camera is the visualizer's."""
        return self._vis.orient(orient, radius, center=center, method=method)


def _parameter_property(kind, name):
    return property(lambda self: self[kind, name], lambda self, value: self.__setitem__((kind, name), value))


for _kind in KINDS:
    for _name in PARAMETERS:
        setattr(VelocityView, f"{_kind}_{_name}", _parameter_property(_kind, _name))


class KinematicColormap:
    """The colormap of a VelocityFrames as the small mapping the recorder reads and sets: "vmin", "vmax", "colormap_name" and "log"
    are the view's (kind, name) parameters (None: automatic), "type" is "kinematic", any other key reads as None."""

    def __init__(self, frames):
        self._frames = frames

    def __getitem__(self, key):
        if key == "type":
            return "kinematic"
        return self._frames._view[self._frames.kind, key] if key in PARAMETERS else None

    def __setitem__(self, key, value):
        if key == "type":
            if value != "kinematic":
                raise ValueError(f"a kinematic map cannot become a colormap of type {value!r}")
        elif key in PARAMETERS:
            self._frames._view[self._frames.kind, key] = value
        elif value is not None:
            raise ValueError(f"a kinematic map has no parameter {key!r}")

    get_parameter = __getitem__

    def get_parameters(self):
        """The parameters of the frame being composed: vmin and vmax are the range its base was resolved to."""
        vmin, vmax = self._frames._resolved_range
        return {"type": "kinematic", "vmin": vmin, "vmax": vmax, "colormap_name": self["colormap_name"], "log": self["log"]}


class VelocityFrames(FrameInterface):
    """One kinematic map of a VelocityView with the frame interface of a visualizer: camera, scene and parameters are the view's,
    which are the visualizer's.  With view[kind, "vmin"] or "vmax" left None every frame resolves its own range from the device
    sort, so the colorbar of a movie moves with the scene; colormap_autorange() pins the current range, which is how a movie gets
    a fixed colorbar."""
    canvas_format = "rgba8unorm"
    _render_mode = "kinematic"

    def __init__(self, view, kind, label=None):
        self._view = view
        self.kind = check_kind(kind)
        self.label = label
        self._vis = view._vis
        self._sph = view._sph
        self._colormap = KinematicColormap(self)
        self._resolved_range = (None, None)
        self._init_frames(view._vis.data_loader.get_position_units())

    # -- the composed frame's base and colorbar (frames.FrameInterface) ------------------------------------
    def _presentation_base(self, width, height):
        view, p = self._view, self._view._params[self.kind]
        view._ensure_rendered()     # the EXPORT frame at the visualizer's camera and v_ref, unless the target already holds it
        vmin, vmax = view.get_range(self.kind)
        self._resolved_range = (vmin, vmax)
        return {"map": _PRESENT_MAP[self.kind], "lut": view._lut(p["colormap_name"]), "vmin": np.float32(vmin),
                "vmax": np.float32(vmax), "log": p["log"]}

    def _compose_frame(self, width, height, base, layers, yuv420):
        ctx = self._sph._context
        return (ctx.present_yuv420 if yuv420 else ctx.present)(width, height, base, layers)

    def _has_colorbar(self):
        return True

    def _get_colorbar_label(self):
        prefix = r"$\log_{10}$ " if self._view._params[self.kind]["log"] else ""
        return prefix + (DEFAULT_LABELS[self.kind] if self.label is None else self.label)

    def colormap_autorange(self):
        """Pin the automatic range of the current scene and camera into view[kind, "vmin"] and view[kind, "vmax"]: the frames
        that follow keep it (a fixed colorbar) until an end is set to None again, which makes every frame resolve its own."""
        view, kind = self._view, self.kind
        view[kind, "vmin"] = view[kind, "vmax"] = None
        view[kind, "vmin"], view[kind, "vmax"] = view.get_range(kind)

    # -- view state and parameters: the visualizer's and the view's ----------------------------------------
    colormap = property(lambda self: self._colormap)
    data_loader = property(lambda self: self._vis.data_loader)
    rotation_matrix = property(lambda self: self._vis.rotation_matrix, lambda self, v: setattr(self._vis, "rotation_matrix", v))
    scale = property(lambda self: self._vis.scale, lambda self, v: setattr(self._vis, "scale", v))
    position_offset = property(lambda self: self._vis.position_offset, lambda self, v: setattr(self._vis, "position_offset", v))
    quantity_name = property(lambda self: self._vis.quantity_name, lambda self, v: setattr(self._vis, "quantity_name", v))

    def orient(self, orient, radius, center=None, method=None):
        """The visualizer's orient: the camera is the visualizer's."""
        return self._vis.orient(orient, radius, center=center, method=method)

    def centre_on_halo(self, n, at="shrink"):
        """The visualizer's centre_on_halo: the camera is the visualizer's.  (The default goes through the call as it was.)"""
        return self._vis.centre_on_halo(n) if at == "shrink" else self._vis.centre_on_halo(n, at=at)

    def profile(self, r_max=None, **kwargs):
        """The visualizer's profile: the camera is the visualizer's."""
        return self._vis.profile(r_max, **kwargs)

    def phase_diagram(self, x, y, weight="mass", value=None, **kwargs):
        """The visualizer's phase_diagram: the particles are the visualizer's."""
        return self._vis.phase_diagram(x, y, weight=weight, value=value, **kwargs)

    def scale_to_virial(self, rho_threshold, r_max, factor=1.0):
        """The visualizer's scale_to_virial: the camera is the visualizer's."""
        return self._vis.scale_to_virial(rho_threshold, r_max, factor)


def check_maps_arguments(pos, smooth, mass, vel, rotation, center, scale, resolution):
    """The arguments of velocity_maps, checked on the host: float32 arrays of one length, a rotation, a finite centre, scale > 0,
    1 <= resolution <= 16384.  Returns (pos, smooth, mass, vel, rotation float64 (3, 3), center float64 (3,), scale, resolution)."""
    pos, mass, vel = loader.check_moments_arrays(pos, mass, vel)
    if vel is None:
        raise ValueError("vel is required: the (n, 3) velocities")
    smooth = np.asarray(smooth, dtype=np.float32)
    if smooth.shape != (len(pos),):
        raise ValueError(f"pos and smooth must have the same length: smooth has shape {smooth.shape}, not ({len(pos)},)")
    rotation = loader.check_rotation_matrix(np.eye(3) if rotation is None else rotation)
    try:
        c = np.asarray(center, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"center must be three finite coordinates, not {center!r}") from None
    if c.shape != (3,) or not np.isfinite(c).all():
        raise ValueError(f"center must be three finite coordinates, not {center!r}")
    scale = loader._positive_length("scale", scale)
    if isinstance(resolution, bool) or not isinstance(resolution, (int, np.integer)) or not 1 <= resolution <= 16384:
        raise ValueError(f"resolution must be an integer from 1 to 16384, not {resolution!r}")
    return pos, smooth, mass, vel, rotation, c, scale, int(resolution)


def velocity_maps(pos, smooth, mass, vel, rotation=None, center=(0, 0, 0), scale=config.DEFAULT_SCALE,
                  resolution=config.DEFAULT_RESOLUTION, v_ref=None, device_id=0):
    """The kinematic maps of caller-supplied arrays, without a visualizer: every particle drawn once by a camera looking along
    the third row of `rotation` (None: the identity; the matrix of topsy_amd.orientation) at `center`, half-width `scale`,
    `resolution` pixels a side.  v_ref: None (zero), three components, or "center" (the mean velocity of the inner fifth of the
    sphere of radius scale about center, as VelocityView takes it).  Returns get_maps' dict."""
    pos, smooth, mass, vel, rotation, c, scale, resolution = check_maps_arguments(pos, smooth, mass, vel, rotation, center, scale,
                                                                                  resolution)
    v_ref = check_v_ref(v_ref)
    ctx = _native.Context(resolution, 4, device_id)
    try:
        if isinstance(v_ref, str):
            _, r, r_vel = loader.check_moments_arguments(c, scale, None, True)
            v_ref = loader.compute_moments(ctx, pos, mass, vel, c, r, r_vel)["v_cen"]
            if not np.isfinite(v_ref).all():
                raise ValueError(f"v_ref='center': no particle within {r_vel} of {c} to take the mean velocity from")
        ctx.set_kernel_mips(kernel_lut.kernel_mips())
        ctx.upload_particles(pos[:, 0], pos[:, 1], pos[:, 2], smooth, mass)
        if len(pos) > 1:        # the load-time order of a visualizer's particles (particle_buffers.py): coherent chunks, culled by view
            ctx.reorder_spatial(particle_buffers.ParticleBuffers._num_strata(len(pos)), 1337)
        ctx.upload_velocities(vel[:, 0], vel[:, 1], vel[:, 2])
        camera = sph.SPH.__new__(sph.SPH)       # (the camera arithmetic of the renderers, without a renderer)
        camera.rotation_matrix, camera.position_offset, camera.scale = rotation, -c, scale
        M, sf = camera._get_transform_params()
        ctx.set_line_of_sight(rotation[2] / np.sqrt(rotation[2] @ rotation[2]), v_ref)
        ctx.render(M, sf, mode=_native.MODE_KINEMATIC)
        return maps_dict(ctx.velocity_moments())
    finally:
        ctx.close()
