"""Spectral cubes: the whole line-of-sight velocity distribution per pixel, where the kinematic maps (kinematics.py) keep its mean
and dispersion -- a position-position-velocity cube as an HI or CO observation gives it, drawn in one pass on the GPU from the
resident particles (tsp_spectral_cube, include/topsy_splat.h "Spectral cubes").  A warp, a bar, a counter-rotating component or two
clumps on one sight line look alike in v_los / sigma_los and differ in the cube.

spectral_cube(pos, smooth, mass, vel, ...) draws arrays without a visualizer; VelocityView.get_cube() draws a visualizer's scene at
its camera.  Both return a SpectralCube: the (n_channels, R, R) float32 array with its channel edges, and the usual reductions --
moment maps, the integrated spectrum, position-velocity diagrams -- as plain numpy on the downloaded cube.

Out of scope: several GPUs and periodic tiling (as VelocityView), a device-resident cube, optical depth."""
import numpy as np

from . import _native, config, kernel_lut, particle_buffers, sph
from .kinematics import check_maps_arguments, check_v_ref

MAX_CHANNELS = _native.CUBE_MAX_CHANNELS
TRUNCATE = 5.0      # the default band reaches this many line widths beyond the largest |u| (what the kernel itself keeps of a line)


class SpectralCube:
    """data[c, j, i]: the surface density of pixel (row j, column i) in velocity channel c, which spans v_edges[c] .. v_edges[c + 1]
    (the edges are v_min + k * dv in float64, as the library forms them)."""

    def __init__(self, data, v_min, dv):
        data = np.asarray(data)
        if data.ndim != 3 or data.shape[1] != data.shape[2]:
            raise ValueError(f"a cube is (n_channels, R, R), not {data.shape}")
        dv = float(dv)
        if not (np.isfinite(v_min) and np.isfinite(dv) and dv > 0.0):
            raise ValueError(f"v_min must be finite and dv finite and > 0, not {v_min!r}, {dv!r}")
        self.data = data
        self.v_min = float(v_min)
        self.dv = dv

    n_channels = property(lambda self: self.data.shape[0])
    resolution = property(lambda self: self.data.shape[1])

    @property
    def v_edges(self):
        """float64 (n_channels + 1,)"""
        return self.v_min + np.arange(self.n_channels + 1, dtype=np.float64) * self.dv

    @property
    def v_centers(self):
        """float64 (n_channels,)"""
        e = self.v_edges
        return 0.5 * (e[:-1] + e[1:])

    def moment(self, order):
        """float64 (R, R).  0: the surface density, the sum over the channels.  1: the mean velocity, sum(data v_c) / moment 0, NaN
        where moment 0 is not > 0.  2: the dispersion about that mean, with the variance dv^2 / 12 a channel of width dv adds
        (Sheppard's correction) subtracted and the result clipped at 0; NaN where the mean is."""
        if order not in (0, 1, 2):
            raise ValueError(f"order must be 0, 1 or 2, not {order!r}")
        d = self.data.astype(np.float64)
        m0 = d.sum(axis=0)
        if order == 0:
            return m0
        v = self.v_centers[:, None, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = np.where(m0 > 0.0, (d * v).sum(axis=0) / m0, np.nan)
            if order == 1:
                return mean
            var = np.where(m0 > 0.0, (d * (v - mean) ** 2).sum(axis=0) / m0, np.nan) - self.dv ** 2 / 12.0
        return np.sqrt(np.where(var < 0.0, 0.0, var))

    def spectrum(self, mask=None):
        """float64 (n_channels,): the sum over the pixels (the integrated line profile), or over those where `mask`, (R, R)
        booleans, is true."""
        d = self.data.astype(np.float64)
        if mask is None:
            return d.sum(axis=(1, 2))
        m = np.asarray(mask)
        if m.dtype != np.bool_ or m.shape != self.data.shape[1:]:
            raise ValueError(f"mask must be ({self.resolution}, {self.resolution}) booleans, not {m.dtype} {m.shape}")
        return (d * m).sum(axis=(1, 2))

    def pv(self, axis, rows=None):
        """float64 (n_channels, R): a position-velocity diagram, the cube summed along image axis `axis` (0: over the rows, leaving
        position = column; 1: over the columns, leaving position = row) within the band rows = (first, end) of that axis (None: all
        of it)."""
        if axis not in (0, 1):
            raise ValueError(f"axis must be 0 (sum over rows) or 1 (sum over columns), not {axis!r}")
        R = self.resolution
        first, end = (0, R) if rows is None else _check_band(rows, R)
        d = self.data.astype(np.float64)
        return d[:, first:end, :].sum(axis=1) if axis == 0 else d[:, :, first:end].sum(axis=2)


def _check_band(rows, R):
    try:
        first, end = rows
        ok = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in (first, end)) and 0 <= first < end <= R
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"rows must be (first, end) with 0 <= first < end <= {R}, not {rows!r}")
    return int(first), int(end)


def check_cube_arguments(n, resolution, v_range, n_channels, sigma_v, sigma):
    """The spectral arguments, checked on the host: v_range None or (v_min, v_max) finite with v_max > v_min; 1 <= n_channels <=
    4096 with n_channels * resolution^2 <= 2^31; sigma_v finite and >= 0; sigma None or n values (their content is the library's:
    a particle whose sigma is negative or not finite is not drawn).  Returns (v_range or None, n_channels, sigma_v, sigma float32)."""
    if v_range is not None:
        try:
            lo, hi = (float(v) for v in v_range)
        except (TypeError, ValueError):
            raise ValueError(f"v_range must be None or (v_min, v_max), finite with v_max > v_min, not {v_range!r}") from None
        if not (np.isfinite(lo) and np.isfinite(hi) and hi > lo):
            raise ValueError(f"v_range must be None or (v_min, v_max), finite with v_max > v_min, not {v_range!r}")
        v_range = (lo, hi)
    if isinstance(n_channels, bool) or not isinstance(n_channels, (int, np.integer)) or not 1 <= n_channels <= MAX_CHANNELS:
        raise ValueError(f"n_channels must be an integer from 1 to {MAX_CHANNELS}, not {n_channels!r}")
    if int(n_channels) * int(resolution) ** 2 > _native.CUBE_MAX_CELLS:
        raise ValueError(f"n_channels * resolution^2 must be at most 2^31, not {int(n_channels)} * {int(resolution)}^2")
    try:
        sigma_v = float(sigma_v)
    except (TypeError, ValueError):
        raise ValueError(f"sigma_v must be finite and >= 0, not {sigma_v!r}") from None
    if not (np.isfinite(sigma_v) and sigma_v >= 0.0):
        raise ValueError(f"sigma_v must be finite and >= 0, not {sigma_v!r}")
    if sigma is not None:
        sigma = np.asarray(sigma, dtype=np.float32)
        if sigma.shape != (n,):
            raise ValueError(f"sigma must have one value per particle: it has shape {sigma.shape}, not ({n},)")
    return v_range, int(n_channels), sigma_v, sigma


def default_v_range(vel, axis, v_ref, sigma_v, sigma):
    """(-V, V): V = max |u| over the finite u = (vel - v_ref) . axis of the host velocities, plus 5 times the largest line width
    max sqrt(sigma_v^2 + sigma^2) over the finite sigma; (-1, 1) when nothing is finite or V is 0."""
    u = (np.asarray(vel, dtype=np.float64) - np.asarray(v_ref, dtype=np.float64)) @ np.asarray(axis, dtype=np.float64)
    u = np.abs(u[np.isfinite(u)])
    s = float(sigma_v)
    if sigma is not None:
        sp = np.asarray(sigma, dtype=np.float64)
        sp = sp[np.isfinite(sp) & (sp >= 0.0)]
        if sp.size:
            s = float(np.sqrt(s * s + sp.max() ** 2))
    V = (float(u.max()) if u.size else 0.0) + TRUNCATE * s
    if not (np.isfinite(V) and V > 0.0):
        return -1.0, 1.0
    return -V, V


def draw(context, M, scale_factor, v_range, n_channels, sigma_v, sigma):
    """The cube of the context's resident particles along its line of sight, over v_range in n_channels equal channels."""
    dv = (v_range[1] - v_range[0]) / n_channels
    return SpectralCube(context.spectral_cube(M, scale_factor, v_range[0], dv, n_channels, sigma_v, sigma), v_range[0], dv)


def spectral_cube(pos, smooth, mass, vel, v_range=None, n_channels=64, sigma_v=0.0, sigma=None, rotation=None, center=(0, 0, 0),
                  scale=config.DEFAULT_SCALE, resolution=config.DEFAULT_RESOLUTION, v_ref=None, device_id=0):
    """The spectral cube of caller-supplied arrays, without a visualizer: every particle drawn once by the camera of
    velocity_maps (looking along the third row of `rotation` at `center`, half-width `scale`, `resolution` pixels a side), its
    line-of-sight velocity u = (vel - v_ref) . axis spread over n_channels equal channels of v_range as a Gaussian of width
    sqrt(sigma_v^2 + sigma[i]^2) integrated over each channel (a width of 0 puts the particle into the one channel that holds u).
    v_range None: (-V, V) with V = max |u| + 5 max width (default_v_range).  v_ref as velocity_maps.  Returns a SpectralCube."""
    pos, smooth, mass, vel, rotation, c, scale, resolution = check_maps_arguments(pos, smooth, mass, vel, rotation, center, scale,
                                                                                  resolution)
    v_ref = check_v_ref(v_ref)
    v_range, n_channels, sigma_v, sigma = check_cube_arguments(len(pos), resolution, v_range, n_channels, sigma_v, sigma)
    ctx = _native.Context(resolution, 4, device_id)
    try:
        if isinstance(v_ref, str):
            from . import loader
            _, r, r_vel = loader.check_moments_arguments(c, scale, None, True)
            v_ref = loader.compute_moments(ctx, pos, mass, vel, c, r, r_vel)["v_cen"]
            if not np.isfinite(v_ref).all():
                raise ValueError(f"v_ref='center': no particle within {r_vel} of {c} to take the mean velocity from")
        ctx.set_kernel_mips(kernel_lut.kernel_mips())
        ctx.upload_particles(pos[:, 0], pos[:, 1], pos[:, 2], smooth, mass)
        if len(pos) > 1:        # the load-time order of a visualizer's particles, as velocity_maps: screen-coherent lists
            ctx.reorder_spatial(particle_buffers.ParticleBuffers._num_strata(len(pos)), 1337)
        ctx.upload_velocities(vel[:, 0], vel[:, 1], vel[:, 2])
        camera = sph.SPH.__new__(sph.SPH)       # (the camera arithmetic of the renderers, without a renderer)
        camera.rotation_matrix, camera.position_offset, camera.scale = rotation, -c, scale
        M, sf = camera._get_transform_params()
        axis = rotation[2] / np.sqrt(rotation[2] @ rotation[2])
        ctx.set_line_of_sight(axis, v_ref)
        if v_range is None:
            v_range = default_v_range(vel, axis, v_ref, sigma_v, sigma)
        return draw(ctx, M, sf, v_range, n_channels, sigma_v, sigma)
    finally:
        ctx.close()


def view_cube(view, v_range=None, n_channels=64, sigma_v=0.0, sigma=None):
    """VelocityView.get_cube: the cube of the view's visualizer at its current camera and the view's v_ref, every particle drawn
    once (no progressive blocks).  The render target and the view's frame are left as they are."""
    vis, s = view._vis, view._sph
    ld = vis.data_loader
    vel = np.asarray(ld.get_velocities(), dtype=np.float32)
    v_range, n_channels, sigma_v, sigma = check_cube_arguments(len(vel), s._context.resolution, v_range, n_channels, sigma_v, sigma)
    camera = sph.SPH.__new__(sph.SPH)
    camera.rotation_matrix, camera.position_offset, camera.scale = view._camera()
    M, sf = camera._get_transform_params()
    axis = np.asarray(camera.rotation_matrix, dtype=np.float64)[2]
    axis = axis / np.sqrt(axis @ axis)
    v_ref = view._current_v_ref()
    vis.particle_buffers.ensure_velocities()
    s._context.set_line_of_sight(axis, v_ref)
    if v_range is None:
        v_range = default_v_range(vel, axis, v_ref, sigma_v, sigma)
    return draw(s._context, M, sf, v_range, n_channels, sigma_v, sigma)
