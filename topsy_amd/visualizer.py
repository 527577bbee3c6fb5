"""Headless Visualizer: the orchestrator surface of reference src/topsy/visualizer.py:31-602 for
the accelerated path -- data loader -> resident particle buffers -> SPH renderer -> colormap.

Windowing and view synchronisation are out of scope; what the UI layers call on
the orchestrator -- rotate / scale / position_offset / quantity_name / render_mode / invalidate / draw /
colormap_autorange / get_sph_image / get_sph_presentation_image / get_depth_image / save -- is here with
the reference's semantics, so those layers can sit on top unchanged.
The composed frames (get_presentation_image, get_presentation_image_yuv420), their layer switches and the
frame listeners come from topsy_amd/frames.py, shared with SurfaceView.
"""
import logging

import numpy as np

from . import _native, colormap, config, loader, overlays, particle_buffers, periodic_sph, sph
from .drawreason import DrawReason
from .frames import FrameInterface

logger = logging.getLogger(__name__)

_VALID_MODES = {"univariate", "bivariate", "rgb", "rgb-hdr", "surface"}
_UNSUPPORTED_MODES = {
    "surface": "it is not a mode of the visualizer yet: use topsy_amd.SurfaceView(vis) for the surface rendering",
}


class VisualizerBase(FrameInterface):
    device = None      # kept for signature compatibility; the GPU is owned by particle_buffers.context

    def __init__(self, data_loader_class=loader.TestDataLoader, data_loader_args=(), data_loader_kwargs={},
                 *, render_resolution=config.DEFAULT_RESOLUTION, periodic_tiling=False,
                 colormap_name=config.DEFAULT_COLORMAP, canvas_class=None, render_mode="univariate", device_id=0,
                 n_gpus=None, device_ids=None, shard_assignment=None):
        """n_gpus / device_ids: render on several GPUs of this node from this one process -- the particles are sharded
        by index range, every render block runs on all shards at once and the frame ends with one RCCL sum-reduce of the
        image onto the first device (topsy_amd/multigpu.py); everything else (colormap, autorange, exports) is unchanged.
        shard_assignment: "contiguous" | "interleaved" | "auto" (config.MULTI_GPU_SHARD_ASSIGNMENT)."""
        self._render_resolution = render_resolution
        self._sph = None
        self._colormap = None
        if device_ids is None and n_gpus is not None and n_gpus > 1:
            device_ids = list(range(device_id, device_id + n_gpus))
        self._device_id = device_id if not device_ids else device_ids[0]
        self._prevent_sph_rendering = False
        self._validate_render_mode(render_mode)
        self._render_mode = render_mode
        self.canvas_format = self._render_mode_to_canvas_format(render_mode)
        self.data_loader = data_loader_class(self.device, *data_loader_args, **data_loader_kwargs)
        self.particle_buffers = particle_buffers.ParticleBuffers(
            self.data_loader, render_resolution, self._device_id,
            self.data_loader.get_render_progression().get_max_particle_regions_per_block(), device_ids=device_ids,
            shard_assignment=shard_assignment)
        self.periodicity_scale = self.data_loader.get_periodicity_scale()
        self._periodic_tiling = periodic_tiling
        if periodic_tiling and not self.periodicity_scale:
            raise ValueError("periodic_tiling needs a data loader with a finite periodicity scale")
        self._pending_draw = None
        self._init_frames(self.data_loader.get_position_units())
        self._initialize_sph_and_colormap(colormap_name)

    # -- mode plumbing (reference visualizer.py:96-120, 170-186, 203-231) ----------------------
    def _get_sph_class_for_render_mode(self, render_mode):
        return sph.RGBSPH if render_mode in ("rgb", "rgb-hdr") else sph.SPH

    def _get_colormap_parameters_for_render_mode(self, render_mode):
        params = {"weighted_average": self.quantity_name is not None}
        if render_mode == "rgb":
            params.update({"type": "rgb", "hdr": False, "log": True})
        elif render_mode == "rgb-hdr":
            params.update({"type": "rgb", "hdr": True, "log": True})
        elif render_mode == "bivariate":
            params.update({"type": "bivariate"})
        else:
            params.update({"type": "density"})
        return params

    def _render_mode_to_canvas_format(self, render_mode):
        if render_mode is None:
            return None
        return "rgba16float" if render_mode.endswith("hdr") else "rgba8unorm"

    def _validate_render_mode(self, new_render_mode):
        if new_render_mode not in _VALID_MODES:
            raise ValueError(f"Invalid render_mode '{new_render_mode}'. Valid modes: {_VALID_MODES}")
        if new_render_mode in _UNSUPPORTED_MODES:
            raise ValueError(f"render_mode '{new_render_mode}' is not provided by the MI355X backend: "
                             f"{_UNSUPPORTED_MODES[new_render_mode]}")

    def _initialize_sph_and_colormap(self, colormap_name=None):
        previous = None if self._sph is None else (self._sph.rotation_matrix, self._sph.position_offset, self._sph.scale)
        if self._periodic_tiling:
            self._sph = periodic_sph.PeriodicSPH(self, self._render_resolution)
        else:
            sph_class = self._get_sph_class_for_render_mode(self._render_mode)
            logger.info(f"Using {sph_class.__name__} renderer for render mode '{self._render_mode}'")
            self._sph = sph_class(self, self._render_resolution)
        self.reset_view(*(previous or (None, None, None)))
        self._sph.invalidate()
        if colormap_name is None:
            colormap_name = self._colormap.get_parameter("colormap_name")
        self.render_texture = self._sph.get_output_texture()
        self._colormap = colormap.ColormapHolder(self.device, self.render_texture, self.canvas_format)
        self._colormap.update_parameters({"colormap_name": colormap_name})
        self._initialize_colormap()

    def _initialize_colormap(self):
        changed_type = self._colormap.update_parameters(self._get_colormap_parameters_for_render_mode(self._render_mode))
        params = self._colormap.get_parameters()
        if changed_type or params["vmin"] is None or params["vmax"] is None:
            logger.info("Autorange colormap parameters")
            self._autorange()

    def _update_render_mode(self, new_render_mode, revert_on_failure=True):
        self._validate_render_mode(new_render_mode)
        old = self._render_mode
        self._render_mode = new_render_mode
        try:
            self.canvas_format = self._render_mode_to_canvas_format(new_render_mode)
            self._initialize_sph_and_colormap()
        except Exception:
            if revert_on_failure:
                logger.error(f"Failed to update render mode to '{new_render_mode}'; reverting to '{old}'")
                self._update_render_mode(old, revert_on_failure=False)
            raise
        self.invalidate(DrawReason.CHANGE)

    # -- view state -------------------------------------------------------------------------------
    def invalidate(self, reason=DrawReason.CHANGE):
        """Mark the SPH image stale.  Without an event loop the redraw happens lazily on the next read."""
        self._sph.invalidate(reason)
        self._pending_draw = reason

    @staticmethod
    def _y_rotation_matrix(angle):     # rotates about x (name as in the reference, visualizer.py:347-351)
        c, s = np.cos(angle), np.sin(angle)
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])

    @staticmethod
    def _x_rotation_matrix(angle):     # rotates about y (visualizer.py:353-357)
        c, s = np.cos(angle), np.sin(angle)
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])

    def rotate(self, x_angle, y_angle):
        self.rotation_matrix = self._x_rotation_matrix(x_angle) @ self._y_rotation_matrix(y_angle) @ self.rotation_matrix

    def reset_view(self, rotation_matrix=None, position_offset=None, scale=None):
        self._sph.scale = self.data_loader.get_initial_view_width() if scale is None else scale
        self._sph.position_offset = -self.data_loader.get_initial_center() if position_offset is None else position_offset
        self._sph.rotation_matrix = self.data_loader.get_initial_rotation() if rotation_matrix is None else rotation_matrix

    @property
    def colormap(self):
        return self._colormap

    @property
    def rotation_matrix(self):
        return self._sph.rotation_matrix

    @rotation_matrix.setter
    def rotation_matrix(self, value):
        self._sph.rotation_matrix = value
        self.invalidate()

    @property
    def position_offset(self):
        return self._sph.position_offset

    @position_offset.setter
    def position_offset(self, value):
        self._sph.position_offset = value
        self.invalidate()

    @property
    def scale(self):
        """Half-width of the view in simulation units."""
        return self._sph.scale

    @scale.setter
    def scale(self, value):
        self._sph.scale = value
        self.invalidate()

    @property
    def render_mode(self):
        return self._render_mode

    @render_mode.setter
    def render_mode(self, value):
        self._update_render_mode(value)

    @property
    def quantity_name(self):
        return self.particle_buffers.quantity_name

    @quantity_name.setter
    def quantity_name(self, value):
        if value == self.particle_buffers.quantity_name:
            return
        if value is not None:
            try:
                self.data_loader.get_named_quantity(value)
            except Exception as e:
                raise ValueError(f"Unable to get quantity named '{value}'") from e
        old = self.particle_buffers.quantity_name
        try:
            self._switch_quantity(value)
        except _native.BackendError:
            # the upload failed and left the resident quantity as it was (a failed attribute upload changes nothing,
            # include/topsy_splat.h): go on drawing that one
            logger.error(f"Failed to switch to quantity '{value}'; reverting to '{old}'")
            self._switch_quantity(old)
            raise

    def _switch_quantity(self, value):
        self.particle_buffers.quantity_name = value
        self.invalidate(DrawReason.CHANGE)
        self._colormap.update_parameters({"vmin": None, "vmax": None, "log": None})
        self._initialize_colormap()

    @property
    def averaging(self):
        return self.quantity_name is not None

    def _autorange(self):
        """colormap.autorange(sph.get_image()) (reference visualizer.py:313,336) without the read-back."""
        self._sph.ensure_rendered()
        self._colormap.autorange_on_device(self._sph.last_render_mass_scale)

    def colormap_autorange(self):
        self._autorange()
        self.invalidate(DrawReason.PRESENTATION_CHANGE)

    # -- drawing (reference visualizer.py:386-405) ---------------------------------------------
    def render_sph(self, draw_reason=DrawReason.CHANGE):
        self._sph.render(draw_reason)

    def draw(self, reason, target_texture_view=None):
        """One frame: SPH blocks, fold the sampling fraction into the colormap, colour.  Returns the
        (R, R, 4) presentation array (also written into `target_texture_view` when given)."""
        if not self._prevent_sph_rendering:
            self.render_sph(reason)
        res = self._render_resolution
        self._colormap.set_scaling(res, res, self._sph.last_render_mass_scale)
        out = self._colormap.encode_render_pass(None, target_texture_view)
        self._pending_draw = None
        if reason != DrawReason.EXPORT and not self._prevent_sph_rendering and self._sph.needs_refine():
            self.invalidate(DrawReason.REFINE)
        if reason not in (DrawReason.REFINE, DrawReason.PRESENTATION_CHANGE):   # what SynchronizationMixin.draw forwards
            self._frame_produced()
        return out

    # -- exports (reference visualizer.py:452-570) ---------------------------------------------
    def get_sph_image(self):
        """Logical content of the SPH image (no colormap): density, weighted mean, or rgb."""
        return self._colormap.sph_raw_output_to_content(self._sph.get_image())

    def get_sph_presentation_image(self):
        """Colormapped export-quality image, (R, R, 4) uint8 RGBA (float16 for rgb-hdr)."""
        self.render_sph(DrawReason.EXPORT)
        res = self._render_resolution
        self._colormap.set_scaling(res, res, self._sph.last_render_mass_scale)
        out = self._colormap.encode_render_pass(None, None)
        self._frame_produced()
        return out

    # -- the composed frame's base, colorbar and extra layer (frames.FrameInterface) -----------------
    def _presentation_base(self, width, height):
        self.render_sph(DrawReason.EXPORT)
        self._colormap.set_scaling(width, height, self._sph.last_render_mass_scale)
        return self._colormap.present_base(self._sph._context)

    def _compose_frame(self, width, height, base, layers, yuv420):
        ctx = self._sph._context
        return (ctx.present_yuv420 if yuv420 else ctx.present)(width, height, base, layers)

    def _has_colorbar(self):
        return self._colormap.colormap_kind() != "rgb"        # no colorbar for rgb maps (reference visualizer.py:327-335)

    def _extra_layers(self, width, height):
        if not self._periodic_tiling:
            return []
        return [overlays.simcube_layer(self.data_loader.get_periodicity_scale(), self._sph._transform[0], width, height)]

    def get_depth_image(self):
        depth = self._sph.get_depth_image()
        # the depth pass went through the shared render target: the next frame must redraw the scene
        self.invalidate(DrawReason.CHANGE)
        return depth

    def centre_on_pixel(self, row, col):
        """Move position_offset so that the point drawn at pixel (row, col) of get_sph_image() comes to the image centre and,
        where get_depth_image() is finite at that pixel, its depth to the view plane: the arithmetic of the reference canvas's
        double click (canvas/__init__.py:105-129) without the glide.  Returns the new offset."""
        res = self._render_resolution
        row, col = int(row), int(col)
        if not (0 <= row < res and 0 <= col < res):
            raise ValueError(f"pixel ({row}, {col}) outside the {res} x {res} image")
        # pixel centres in view coordinates: column j at x = ((j + 0.5) * 2 / R - 1) * scale, row i at y = (1 - (i + 0.5) * 2 / R) * scale
        view = np.array([((col + 0.5) * 2.0 / res - 1.0) * self.scale, (1.0 - (row + 0.5) * 2.0 / res) * self.scale, 0.0])
        depth = float(self.get_depth_image()[row, col])     # the line-of-sight position at the pixel, before any move
        if np.isfinite(depth):
            view[2] = depth
        self.position_offset = np.asarray(self.position_offset, dtype=np.float64) - np.asarray(self.rotation_matrix).T @ view
        return self.position_offset

    def halo_properties(self):
        """The HaloProperties of the data loader's halo catalogue (get_halo_properties: every halo's mass, centres, radii, spin
        and, with eps=, energies and bound mass, found on the GPU in one call and cached)."""
        if not hasattr(self.data_loader, "get_halo_properties"):
            raise ValueError(f"{type(self.data_loader).__name__} has no halo catalogue")
        return self.data_loader.get_halo_properties()

    def centre_on_halo(self, n, at="shrink"):
        """Move position_offset to minus the centre of halo n (1 = the largest) of the data loader's halo catalogue
        (halos= of from_arrays / ArrayDataLoader: friends-of-friends groups found on the GPU, or the caller's labels): the
        shrinking-sphere centre of the halo's members (at="shrink"), or, from halo_properties(), its centre of mass (at="com")
        or the position of its potential minimum (at="pot": needs eps=).  The array-snapshot counterpart of centre_on_pixel.
        Returns the new offset."""
        if at not in ("shrink", "com", "pot"):
            raise ValueError(f"at must be 'shrink', 'com' or 'pot', not {at!r}")
        if not hasattr(self.data_loader, "get_halo_center"):
            raise ValueError(f"{type(self.data_loader).__name__} has no halo catalogue")
        if at == "shrink":
            centre = self.data_loader.get_halo_center(n)
        else:
            if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
                raise ValueError(f"halo numbers are integers >= 1, not {n!r}")
            props = self.halo_properties()
            if n > len(props):
                raise ValueError(f"halo {n} does not exist: the catalogue has {len(props)} halo(es)")
            if at == "pot" and props.pot_pos is None:
                raise ValueError("at='pot' needs a potential: pass eps= to from_arrays / ArrayDataLoader")
            centre = (props.com if at == "com" else props.pot_pos)[n - 1]
            if not np.isfinite(centre).all():
                raise ValueError(f"halo {n} has no {'centre of mass' if at == 'com' else 'potential minimum'} (no valid member)")
        self.position_offset = -np.asarray(centre, dtype=np.float64)
        return self.position_offset

    def orient(self, orient, radius, center=None, method=None):
        """Turn the view so that the disc inside the sphere of `radius` around `center` is seen face-on (orient="faceon") or
        edge-on ("sideon", its axis up the screen): pynbody.analysis.angmom.faceon / sideon for an array snapshot, without moving
        a particle.  center=None is -position_offset, what the view is centred on (after centre_on_pixel or centre_on_halo: what
        was just centred).  method: "angmom" (the angular momentum about the mean velocity of the inner fifth of the sphere; the
        default with from_arrays(vel=...)) or "shape" (the minor axis of the second-moment tensor; the default without).  The
        moments are found on the GPU from the loader's host arrays (tsp_sphere_moments).  Returns the new rotation_matrix."""
        if not isinstance(self.data_loader, loader.ArrayDataLoader):
            raise ValueError(f"{type(self.data_loader).__name__} keeps no host arrays to orient by: orient() needs from_arrays / "
                             f"ArrayDataLoader")
        if center is None:
            center = -np.asarray(self.position_offset, dtype=np.float64)
        matrix, self.orient_moments = self.data_loader.orientation(orient, radius, center=center, method=method)
        self.rotation_matrix = matrix
        return matrix

    def _array_loader(self, what):
        if not isinstance(self.data_loader, loader.ArrayDataLoader):
            raise ValueError(f"{type(self.data_loader).__name__} keeps no host arrays to take {what} from: it needs from_arrays / "
                             f"ArrayDataLoader")
        return self.data_loader

    def profile(self, r_max=None, center=None, frame=None, **kwargs):
        """The radial Profile (topsy_amd.radial_profile) of what the view shows: about `center` (None: -position_offset, what
        the view is centred on) in `frame` (None: rotation_matrix, so that geometry="disc" bins in annuli about the view axis:
        after orient("faceon") v_phi is the disc's rotation curve).  The other keywords are radial_profile's (r_min, n_bins,
        bins, geometry, half_height, v_cen, G).  The sums are found on the GPU from the loader's host arrays."""
        ld = self._array_loader("a profile")
        if center is None:
            center = -np.asarray(self.position_offset, dtype=np.float64)
        if frame is None:
            frame = np.asarray(self.rotation_matrix, dtype=np.float64)
        return ld.profile(r_max, center=center, frame=frame, **kwargs)

    def phase_diagram(self, x, y, weight="mass", value=None, **kwargs):
        """The PhaseDiagram (topsy_amd.phase_diagram) of two of the loader's named per-particle arrays, e.g.
        phase_diagram("rho", "temp"): ArrayDataLoader.phase_diagram's arguments (names of quantities, "mass" or "smooth"; both
        axes logarithmic unless told otherwise).  The sums are found on the GPU from the loader's host arrays -- with several GPUs
        on the first: there is nothing to shard."""
        return self._array_loader("a phase diagram").phase_diagram(x, y, weight=weight, value=value, **kwargs)

    def rotation_curve(self, radii, eps=None, G=1.0, method="direct", theta=0.5):
        """The RotationCurve (topsy_amd.rotation_curve: v_circ and the midplane potential from direct sums of the softened forces
        at four probes per radius) of what the view shows: about -position_offset, what the view is centred on, in the frame of
        rotation_matrix -- after orient("faceon", r) the probes lie in the disc's plane and the curve is the disc's, the one to
        compare profile(geometry="disc").v_phi with.  eps=None: the softening given to from_arrays(eps=...).  The sums are found
        on the GPU from the loader's host arrays; 4 len(radii) * n pairs, or by the tree (gravity_tree, opening angle theta) with
        method="tree"."""
        ld = self._array_loader("a rotation curve")
        return ld.rotation_curve(radii, center=-np.asarray(self.position_offset, dtype=np.float64),
                                 frame=np.asarray(self.rotation_matrix, dtype=np.float64), eps=eps, G=G,
                                 method=method, theta=theta)

    def get_slice_image(self, quantity=None, resolution=None):
        """The SPH field on the view's centre plane (depth 0 in view coordinates), float32 (R, R) at R = resolution (None: the
        render resolution): the density for quantity=None, else the kernel-weighted mean of that loader quantity, evaluated at
        the pixel centres with the smoothing length taken at the point (topsy_amd.sph_grid's estimator).  Pixel (row, col) is the
        point centre_on_pixel(row, col) would centre on at zero depth.  The sums are found on the GPU from the loader's host
        arrays (tsp_sph_sample_lattice); the rendered frame stays as it is."""
        from . import lattice
        ld = self._array_loader("a slice")
        res = lattice._count("resolution", self._render_resolution if resolution is None else resolution)
        spec = lattice.slice_lattice(self.rotation_matrix, self.position_offset, self.scale, res)
        out = ld.sample_lattice(spec, quantity)
        return out["rho" if quantity is None else "mean"][0]

    def scale_to_virial(self, rho_threshold, r_max, factor=1.0):
        """Set scale to `factor` times the virial radius (topsy_amd.virial_radius: mean enclosed density rho_threshold, searched
        out to r_max) of what the view is centred on, -position_offset: after centre_on_halo(N) the view then frames halo N.
        Returns the new scale (the virial radius is scale / factor)."""
        ld = self._array_loader("a virial radius")
        factor = loader._positive_length("factor", factor)
        r_vir = ld.virial_radius(rho_threshold, r_max, center=-np.asarray(self.position_offset, dtype=np.float64))
        self.scale = factor * r_vir
        return self.scale

    def save(self, filename="output.npy"):
        self._sph.render(DrawReason.EXPORT)
        if filename.endswith(".npy"):
            np.save(filename, self.get_sph_image())
            return
        import matplotlib.pyplot as plt
        extent = np.array([-1.0, 1.0, -1.0, 1.0]) * self.scale
        fig = plt.figure()
        plt.imshow(self.get_sph_presentation_image(), extent=extent)
        plt.xlabel("$x$/" + self.data_loader.get_position_units())
        plt.savefig(filename)
        plt.close(fig)

    def close(self):
        self.particle_buffers.context.close()


class Visualizer(VisualizerBase):
    pass
