"""Data loaders: what the renderer asks of a particle source (host side).

The abstract surface and the synthetic TestDataLoader mirror reference src/topsy/loader.py
(:16-77 and :241-332).  pynbody I/O itself is out of scope for this backend: a pynbody snapshot is
fed through `ArrayDataLoader` (positions / smoothing / mass / named quantities as numpy arrays),
which is what the reference's PynbodyDataInMemory hands to its GPU buffers anyway.
"""
import re
from abc import ABC, abstractmethod

import numpy as np

from . import cell_layout, config


class AbstractDataLoader(ABC):
    def __init__(self, device=None):
        self._device = device

    @abstractmethod
    def __len__(self): ...

    @abstractmethod
    def get_positions(self): ...

    @abstractmethod
    def get_smooth(self): ...

    @abstractmethod
    def get_mass(self): ...

    @abstractmethod
    def get_named_quantity(self, name): ...

    @abstractmethod
    def get_quantity_label(self, quantity_name): ...

    @abstractmethod
    def get_rgb_masses(self): ...

    @abstractmethod
    def get_position_units(self): ...

    def get_pos_smooth(self):
        """(N,4) float32: x, y, z, h -- the reference's vertex layout (loader.py:52-56)."""
        out = np.empty((len(self), 4), dtype=np.float32)
        out[:, :3] = self.get_positions()
        out[:, 3] = self.get_smooth()
        return out

    def get_periodicity_scale(self):
        return np.inf

    def get_render_progression(self):
        from . import progressive_render
        if hasattr(self, "_cell_layout"):
            return progressive_render.RenderProgressionWithCells(self._cell_layout, len(self))
        return progressive_render.RenderProgression(len(self))

    def get_initial_center(self):
        return np.zeros(3, dtype=np.float32)

    def get_initial_rotation(self):
        return np.eye(3)

    def get_initial_view_width(self):
        period = self.get_periodicity_scale()
        return period / 2 if period is not None else config.DEFAULT_SCALE

    def get_quantity_names(self):
        return []

    def get_filename(self):
        return "in-memory data"


class TestDataLoader(AbstractDataLoader):
    """Seeded 3-component Gaussian mixture; bit-for-bit the arrays of the reference's
    TestDataLoader (loader.py:241-332) -- pinned by tests/golden/testdata_n*.npz."""
    __test__ = False   # not a pytest class

    _WEIGHTS = (0.5, 0.4, 0.1)
    _MEANS = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [6.0, 10.0, 0.0]])
    _STDS = np.array([[20.0, 20.0, 20.0], [4.0, 0.2, 4.0], [2.0, 2.0, 3.0]])

    def __init__(self, device=None, n_particles=config.TEST_DATA_NUM_PARTICLES_DEFAULT, n_cells=10, seed=1337,
                 with_cells=False, periodic=False):
        super().__init__(device)
        self._n_particles = n_particles
        self._periodic = periodic
        self._gmm_pos = self._draw_positions(seed)
        self._gmm_den = self._number_density(self._gmm_pos)
        if with_cells:
            self._cell_layout, order = cell_layout.CellLayout.from_positions(
                self._gmm_pos, self._gmm_pos.min() - 1e-3, self._gmm_pos.max() + 1, n_cells)
            self._gmm_pos = self._gmm_pos[order]
            self._gmm_den = self._gmm_den[order]

    def __len__(self):
        return self._n_particles

    def _draw_positions(self, seed):
        np.random.seed(seed)
        n = self._n_particles
        pos = np.empty((n, 3), dtype=np.float32)
        if n == 1:
            pos[0] = self._MEANS[0]
        else:
            filled = 0
            for w, mu, sd in zip(self._WEIGHTS, self._MEANS, self._STDS):
                k = int(n * w)
                pos[filled:filled + k] = np.random.normal(size=(k, 3), scale=1.0).astype(np.float32) * sd[np.newaxis, :] + mu
                filled += k
            assert filled == n, "component sizes int(n*w) must add up to n (as in the reference)"
        return np.random.permutation(pos)

    def _number_density(self, pos):
        # note: exp(-r^2/sigma^2) without the 1/2, as in the reference (loader.py:269-271)
        den = np.zeros(len(pos))
        for w, mu, sd in zip(self._WEIGHTS, self._MEANS, self._STDS):
            den += w * np.exp(-np.sum((pos - mu) ** 2 / sd ** 2, axis=1)) / ((2 * np.pi) ** 1.5 * np.prod(sd))
        return den * self._n_particles

    def get_positions(self):
        return self._gmm_pos

    def get_smooth(self):
        return 2.0 / self._gmm_den ** 0.333333

    def get_mass(self):
        return np.repeat(np.float32(1e-8), self._n_particles)

    def get_named_quantity(self, name):
        if name != "test-quantity":
            raise KeyError("Unknown quantity name")
        p = self._gmm_pos
        return np.sin(p[:, 0]) * np.cos(p[:, 1]) * np.cos(p[:, 2]) * 1e-4

    def get_rgb_masses(self):
        p = self._gmm_pos
        rgb = np.empty((len(p), 3), dtype=np.float32)
        rgb[:, 0] = abs(np.sin(p[:, 0] / 10.0))
        rgb[:, 1] = abs(np.cos(p[:, 1] / 10.0))
        rgb[:, 2] = abs(np.cos(p[:, 2] / 10.0))
        return rgb

    def get_position_units(self):
        return "kpc"

    def get_quantity_names(self):
        return ["test-quantity"]

    def get_quantity_label(self, quantity_name):
        if quantity_name is None:
            return r"test density / $M_{\odot} / \mathrm{kpc}^2$"
        return "test quantity" if quantity_name == "test-quantity" else "unknown"

    def get_filename(self):
        return "test data"

    def get_periodicity_scale(self):
        return 100.0 if self._periodic else None


def check_smoothing_arguments(n_smooth, periodicity_scale):
    """The arguments of a smoothing-length computation, checked on the host (tsp_smoothing_lengths would refuse them):
    returns (n_smooth as int, period as float, 0 = open box).  Raises ValueError."""
    if isinstance(n_smooth, bool) or not isinstance(n_smooth, (int, np.integer)) or not 2 <= n_smooth <= 64:
        raise ValueError(f"n_smooth must be an integer from 2 to 64, not {n_smooth!r}")
    if periodicity_scale is None:
        return int(n_smooth), 0.0
    try:
        period = float(periodicity_scale)
    except (TypeError, ValueError):
        raise ValueError(f"periodicity_scale must be None or a finite number > 0, not {periodicity_scale!r}") from None
    if not (np.isfinite(period) and 0 < period <= float(np.finfo(np.float32).max)):
        raise ValueError(f"periodicity_scale must be None or a finite number > 0, not {periodicity_scale!r}")
    return int(n_smooth), period


ZOOM_MASS_CUT_FACTOR = 1.01      # center="zoom": the particles with mass < 1.01 * mass.min() (reference loader.py:210-211)


def check_center_arguments(select="all", r_start=None, shrink_factor=0.7, min_particles=100):
    """The arguments of a shrinking-sphere centre, checked on the host (tsp_shrink_sphere_center would refuse them): returns
    (mass_cut_factor, r_start as float with 0 = estimated, shrink_factor, min_particles).  Raises ValueError."""
    if select not in ("all", "zoom"):
        raise ValueError(f"select must be 'all' or 'zoom', not {select!r}")
    try:
        r0 = 0.0 if r_start is None else float(r_start)
        shrink = float(shrink_factor)
    except (TypeError, ValueError):
        raise ValueError(f"r_start and shrink_factor must be numbers, not {r_start!r} and {shrink_factor!r}") from None
    if r_start is not None and not (np.isfinite(r0) and r0 > 0):
        raise ValueError(f"r_start must be None or a finite number > 0, not {r_start!r}")
    if not 0.0 < shrink < 1.0:
        raise ValueError(f"shrink_factor must lie strictly between 0 and 1, not {shrink_factor!r}")
    if isinstance(min_particles, bool) or not isinstance(min_particles, (int, np.integer)) or min_particles < 1:
        raise ValueError(f"min_particles must be an integer >= 1, not {min_particles!r}")
    return (ZOOM_MASS_CUT_FACTOR if select == "zoom" else 0.0), r0, shrink, int(min_particles)


FOF_KEYWORDS = ("linking_length", "b", "min_members")


def check_fof_arguments(linking_length=None, b=0.2, min_members=20, periodicity_scale=None):
    """The arguments of a friends-of-friends search, checked on the host (tsp_fof_groups would refuse them): returns
    (linking_length as float or None = from b, b, min_members, period as float with 0 = open box).  Raises ValueError."""
    def number(name, value):
        if isinstance(value, (bool, str)):
            raise ValueError(f"{name} must be a finite number > 0, not {value!r}")
        try:
            v = float(value)
        except (TypeError, ValueError):
            raise ValueError(f"{name} must be a finite number > 0, not {value!r}") from None
        if not (np.isfinite(v) and v > 0 and np.isfinite(np.float32(v)) and np.float32(v) > 0):
            raise ValueError(f"{name} must be a finite number > 0, not {value!r}")
        return v
    ll = None if linking_length is None else number("linking_length", linking_length)
    b = number("b", b)
    if isinstance(min_members, bool) or not isinstance(min_members, (int, np.integer)) or min_members < 1:
        raise ValueError(f"min_members must be an integer >= 1, not {min_members!r}")
    period = 0.0
    if periodicity_scale is not None:
        try:
            period = number("periodicity_scale", periodicity_scale)
        except ValueError:
            raise ValueError(f"periodicity_scale must be None or a finite number > 0, not {periodicity_scale!r}") from None
    if ll is not None and period > 0 and not np.float32(ll) < np.float32(0.5) * np.float32(period):
        raise ValueError(f"linking_length = {linking_length!r} must be below half the periodicity_scale {periodicity_scale!r}")
    return ll, b, int(min_members), period


def fof_linking_length(pos, b, period):
    """b times the mean separation of the particles with finite coordinates, (V / n_valid) ** (1/3) in float64: V = period ** 3
    in a periodic box, else the volume of their bounding box.  Raises ValueError where that is no length."""
    finite = np.isfinite(pos).all(axis=1)
    n_valid = int(finite.sum())
    if n_valid == 0:
        raise ValueError("no particle has finite coordinates: the default linking_length needs at least one")
    if period > 0:
        volume = float(period) ** 3
    else:
        p = pos[finite].astype(np.float64)
        extent = p.max(axis=0) - p.min(axis=0)
        if not (extent > 0).all():
            raise ValueError(f"the particles span no volume (extent {extent.tolist()}): pass an explicit linking_length")
        volume = float(np.prod(extent))
    ll = float(b) * (volume / n_valid) ** (1.0 / 3.0)
    if not (np.isfinite(np.float32(ll)) and np.float32(ll) > 0):
        raise ValueError(f"the default linking_length {ll!r} is no float32 length: pass an explicit linking_length")
    if period > 0 and not np.float32(ll) < np.float32(0.5) * np.float32(period):
        raise ValueError(f"the default linking_length {ll!r} is not below half the periodicity_scale {period!r}: "
                         f"pass an explicit linking_length")
    return ll


def check_fof_positions(pos):
    pos = np.asarray(pos, dtype=np.float32)
    if pos.ndim != 2 or pos.shape[1] != 3:
        raise ValueError(f"pos must have shape (n, 3), not {pos.shape}")
    if len(pos) == 0:
        raise ValueError("pos must have at least one particle")
    return pos


class FofCatalogue:
    """A halo catalogue over n particles: .group, the int32 (n,) labels (N >= 1: halo N, the N-th largest; 0 or less: no halo);
    .sizes, int64, sizes[N - 1] = the members of halo N; len() = the number of haloes; .members(N) = the indices of halo N;
    .linking_length (None for a caller's own labels); .info, what tsp_fof_groups reported (None likewise)."""

    def __init__(self, group, linking_length=None, info=None):
        self.group = np.ascontiguousarray(group, dtype=np.int32)
        self.linking_length = linking_length
        self.info = info
        labelled = self.group[self.group > 0]
        self.sizes = np.bincount(labelled)[1:].astype(np.int64) if len(labelled) else np.zeros(0, dtype=np.int64)

    def __len__(self):
        return len(self.sizes)

    def members(self, n):
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError(f"halo numbers are integers >= 1, not {n!r}")
        if n > len(self):
            raise ValueError(f"halo {n} does not exist: the catalogue has {len(self)} halo(es)")
        return np.flatnonzero(self.group == n)


def compute_fof_catalogue(ctx, pos, linking_length, b, min_members, period):
    """The catalogue of checked arguments (check_fof_arguments, check_fof_positions) on an existing context."""
    ll = fof_linking_length(pos, b, period) if linking_length is None else linking_length
    group, info = ctx.fof_groups(pos[:, 0], pos[:, 1], pos[:, 2], ll, period, min_members)
    return FofCatalogue(group, float(np.float32(ll)), info)


def check_halo_labels(labels, n):
    """A caller's own catalogue: an integer (n,) array, label N >= 1 = halo N, anything <= 0 = no halo.  Raises ValueError."""
    a = np.asarray(labels)
    if a.dtype == bool or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"halo labels must be an integer array, not dtype {a.dtype}")
    if a.shape != (n,):
        raise ValueError(f"halo labels must have shape ({n},), not {a.shape}")
    if a.size and (a.max() > np.iinfo(np.int32).max or a.min() < np.iinfo(np.int32).min):
        raise ValueError("halo labels must fit 32 bits")
    return a.astype(np.int32)


def check_halos_option(halos, n, periodicity_scale):
    """The halos= option of ArrayDataLoader / from_arrays: returns None, a dict of friends-of-friends keywords (checked) or an
    int32 (n,) label array.  Raises ValueError."""
    if halos is None:
        return None
    if isinstance(halos, str):
        if halos != "fof":
            raise ValueError(f"halos must be None, 'fof', a dict of {FOF_KEYWORDS} or an integer label array, not {halos!r}")
        halos = {}
    if isinstance(halos, dict):
        unknown = sorted(set(halos) - set(FOF_KEYWORDS))
        if unknown:
            raise ValueError(f"halos: unknown friends-of-friends keyword(s) {unknown}; known: {FOF_KEYWORDS}")
        check_fof_arguments(periodicity_scale=periodicity_scale, **halos)
        return dict(halos)
    return check_halo_labels(halos, n)


_HALO_CENTER = re.compile(r"halo-([1-9][0-9]*)")


def check_center_option(center, halos=None):
    """The center= option of ArrayDataLoader / from_arrays: returns "none", "all", "zoom", "halo-N" (N >= 1; only with a halo
    catalogue, halos=) or a float64 (3,) array.  Raises ValueError."""
    if isinstance(center, str):
        if center.startswith("halo-") and halos is not None:
            if not _HALO_CENTER.fullmatch(center):
                raise ValueError(f"center={center!r}: the N of 'halo-N' must be an integer >= 1")
            return center
        if center not in ("none", "all", "zoom"):
            raise ValueError(f"center must be 'none', 'all', 'zoom' or three coordinates, not {center!r} "
                             f"('halo-N' needs a halo catalogue: pass halos='fof' or your own label array)")
        return center
    try:
        c = np.asarray(center, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"center must be 'none', 'all', 'zoom' or three coordinates, not {center!r}") from None
    if c.shape != (3,) or not np.isfinite(c).all():
        raise ValueError(f"center must be 'none', 'all', 'zoom' or three finite coordinates, not {center!r}")
    return c.copy()


ORIENTATIONS = ("faceon", "sideon")
ORIENT_METHODS = ("angmom", "shape")
VEL_RADIUS_FRACTION = 0.2        # vel_radius=None: radius / 5, the ratio of pynbody's defaults (1 kpc inside 5 kpc)
_SIDEON_FROM_FACEON = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]])


def _positive_length(name, value):
    if isinstance(value, (bool, str)):
        raise ValueError(f"{name} must be a finite number > 0, not {value!r}")
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a finite number > 0, not {value!r}") from None
    if not (np.isfinite(v) and v > 0):
        raise ValueError(f"{name} must be a finite number > 0, not {value!r}")
    return v


def check_moments_arguments(center, radius, vel_radius, has_vel):
    """The sphere of tsp_sphere_moments, checked on the host (the library would refuse it): returns (center float64 (3,), r,
    r_vel); vel_radius=None is radius / 5 with velocities and 0 without.  Raises ValueError."""
    try:
        c = np.asarray(center, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"center must be three finite coordinates, not {center!r}") from None
    if c.shape != (3,) or not np.isfinite(c).all():
        raise ValueError(f"center must be three finite coordinates, not {center!r}")
    if radius is None:
        raise ValueError("radius is required: the radius of the sphere whose particles are summed, a finite number > 0")
    r = _positive_length("radius", radius)
    if not has_vel:
        if vel_radius is not None:
            raise ValueError(f"vel_radius = {vel_radius!r} needs velocities (vel=)")
        return c.copy(), r, 0.0
    r_vel = VEL_RADIUS_FRACTION * r if vel_radius is None else _positive_length("vel_radius", vel_radius)
    if not r_vel <= r:
        raise ValueError(f"vel_radius = {vel_radius!r} must not exceed radius = {radius!r}")
    return c.copy(), r, r_vel


def check_moments_arrays(pos, mass, vel):
    """float32 pos (n, 3), mass (n,) and vel (n, 3) or None, with at least one valid particle.  Raises ValueError."""
    pos = np.asarray(pos, dtype=np.float32)
    if pos.ndim != 2 or pos.shape[1] != 3:
        raise ValueError(f"pos must have shape (n, 3), not {pos.shape}")
    mass = np.asarray(mass, dtype=np.float32)
    if mass.shape != (len(pos),):
        raise ValueError(f"pos and mass must have the same length: mass has shape {mass.shape}, not ({len(pos)},)")
    if vel is not None:
        vel = np.asarray(vel, dtype=np.float32)
        if vel.shape != pos.shape:
            raise ValueError(f"vel must have the shape of pos, {pos.shape}, not {vel.shape}")
    if len(pos) == 0:
        raise ValueError("pos must have at least one particle")
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(pos).all(axis=1) & np.isfinite(mass) & (mass > 0)
        if vel is not None:
            valid &= np.isfinite(vel).all(axis=1)
    if not valid.any():
        raise ValueError("no particle has finite coordinates" + (" and velocities" if vel is not None else "") +
                         " and a finite mass > 0")
    return pos, mass, vel


def check_orient_arguments(orient, method, has_vel):
    """orient "faceon" | "sideon"; method None | "angmom" | "shape" -> the method (None: "angmom" with velocities, else
    "shape").  Raises ValueError."""
    if orient not in ORIENTATIONS:
        raise ValueError(f"orient must be one of {ORIENTATIONS}, not {orient!r}")
    if method is None:
        return "angmom" if has_vel else "shape"
    if method not in ORIENT_METHODS:
        raise ValueError(f"method must be None or one of {ORIENT_METHODS}, not {method!r}")
    if method == "angmom" and not has_vel:
        raise ValueError("method='angmom' needs velocities (vel=); without them use method='shape'")
    return method


def compute_moments(ctx, pos, mass, vel, center, r, r_vel):
    """tsp_sphere_moments of checked arguments (check_moments_arrays, check_moments_arguments) on an existing context."""
    return ctx.sphere_moments(pos[:, 0], pos[:, 1], pos[:, 2], mass, vel=None if vel is None else (vel[:, 0], vel[:, 1], vel[:, 2]),
                              center=center, r=r, r_vel=r_vel)


def orientation_axis(moments, method):
    """The unit axis a disc is seen along: method "angmom": L / |L|; "shape": the minor axis of the second-moment tensor about
    the centre of mass, its largest-magnitude component positive.  Raises ValueError where there is no such axis."""
    if method == "angmom":
        L = np.asarray(moments["L"], dtype=np.float64)
        norm = float(np.sqrt((L * L).sum()))
        if not norm > 1e-12 * float(moments["A"]):
            raise ValueError(f"no net rotation inside the sphere: |L| = {norm!r} against sum m |d| |v| = {moments['A']!r} "
                             f"(no velocities, or none that is ordered); method='shape' orients by the particles' distribution")
        return L / norm
    if method != "shape":
        raise ValueError(f"method must be one of {ORIENT_METHODS}, not {method!r}")
    xx, xy, xz, yy, yz, zz = (float(v) for v in moments["S"])
    com = np.asarray(moments["com"], dtype=np.float64)
    tensor = np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]]) - float(moments["mass"]) * np.outer(com, com)
    w, v = np.linalg.eigh(tensor)
    if not abs(w[1] - w[0]) > 1e-6 * abs(w[1]):
        raise ValueError(f"no unique minor axis inside the sphere: the second-moment tensor has eigenvalues {w.tolist()}")
    a = v[:, 0]
    return -a if a[np.argmax(np.abs(a))] < 0 else a


def orientation_matrix(moments, orient, method, up=(0, 1, 0)):
    """The (3, 3) float64 rotation that shows the axis of orientation_axis(moments, method) face-on (orient="faceon": the rows
    are p1 = up x a normalised, p2 = a x p1 and a, so that R @ a = +z, toward the viewer -- pynbody's calc_faceon_matrix) or
    side-on ("sideon": the axis up the screen, the disc along x).  |up x a| < 1e-6: (1, 0, 0) takes the place of up."""
    if orient not in ORIENTATIONS:
        raise ValueError(f"orient must be one of {ORIENTATIONS}, not {orient!r}")
    a = orientation_axis(moments, method)
    for up in (up, (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)):       # (the last: a caller's up and the axis both along x)
        p1 = np.cross(np.asarray(up, dtype=np.float64), a)
        if np.sqrt((p1 * p1).sum()) >= 1e-6:
            break
    p1 = p1 / np.sqrt((p1 * p1).sum())
    p2 = np.cross(a, p1)
    faceon = np.stack([p1, p2, a])
    return _SIDEON_FROM_FACEON @ faceon if orient == "sideon" else faceon


def check_rotation_matrix(matrix):
    """A (3, 3) float64 matrix whose rows are orthonormal to 1e-6.  Raises ValueError."""
    try:
        m = np.asarray(matrix, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"a rotation must be a (3, 3) matrix, not {matrix!r}") from None
    if m.shape != (3, 3) or not np.isfinite(m).all():
        raise ValueError(f"a rotation must be a finite (3, 3) matrix, not shape {m.shape}")
    if np.abs(m @ m.T - np.eye(3)).max() > 1e-6:
        raise ValueError(f"the matrix is not orthonormal to 1e-6: R R^T - I reaches {np.abs(m @ m.T - np.eye(3)).max():.3g}")
    return m.copy()


PROFILE_GEOMETRIES = ("sphere", "disc")
PROFILE_MAX_BINS = 512           # tsp_radial_profile's limit
VIRIAL_BINS = 256                # bins per level of virial_radius
VIRIAL_LOG_SPAN = 1024.0         # level 0 of virial_radius spans [r_max / 1024, r_max]


def profile_edges(bins="lin", n_bins=100, r_min=0.0, r_max=None):
    """The bin edges of a profile, float64 (n_bins + 1,): bins="lin": r_min + (r_max - r_min) * k / n_bins; "log" (needs
    r_min > 0): r_min * (r_max / r_min) ** (k / n_bins); both with the end points exact; or the caller's own ascending radii
    (then n_bins, r_min and r_max are not used).  Raises ValueError."""
    if not isinstance(bins, str):
        try:
            edges = np.array(bins, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"bins must be 'lin', 'log' or an ascending array of radii, not {bins!r}") from None
        if edges.ndim != 1 or not 2 <= len(edges) <= PROFILE_MAX_BINS + 1:
            raise ValueError(f"explicit bin edges must be 2 to {PROFILE_MAX_BINS + 1} radii, not shape {edges.shape}")
        if not np.isfinite(edges).all() or edges[0] < 0 or not (np.diff(edges) > 0).all():
            raise ValueError("explicit bin edges must be finite, >= 0 and strictly ascending")
        return edges
    if bins not in ("lin", "log"):
        raise ValueError(f"bins must be 'lin', 'log' or an ascending array of radii, not {bins!r}")
    if isinstance(n_bins, bool) or not isinstance(n_bins, (int, np.integer)) or not 1 <= n_bins <= PROFILE_MAX_BINS:
        raise ValueError(f"n_bins must be an integer from 1 to {PROFILE_MAX_BINS}, not {n_bins!r}")
    if r_max is None:
        raise ValueError("r_max is required: the outer radius of the profile, a finite number > 0")
    r_max = _positive_length("r_max", r_max)
    if isinstance(r_min, (bool, str)):
        raise ValueError(f"r_min must be a finite number >= 0 below r_max, not {r_min!r}")
    try:
        r_min = float(r_min)
    except (TypeError, ValueError):
        raise ValueError(f"r_min must be a finite number >= 0 below r_max, not {r_min!r}") from None
    if not (np.isfinite(r_min) and 0 <= r_min < r_max):
        raise ValueError(f"r_min must be a finite number >= 0 below r_max = {r_max!r}, not {r_min!r}")
    k = np.arange(n_bins + 1, dtype=np.float64) / n_bins
    if bins == "log":
        if not r_min > 0:
            raise ValueError("bins='log' needs r_min > 0")
        edges = r_min * (r_max / r_min) ** k
    else:
        edges = r_min + (r_max - r_min) * k
    edges[0], edges[-1] = r_min, r_max
    if not (np.diff(edges) > 0).all():
        raise ValueError(f"{n_bins} {bins} bins between {r_min!r} and {r_max!r} are not distinct in float64")
    return edges


def check_profile_arguments(center, edges, geometry, frame, half_height, v_cen, G, has_vel):
    """The arguments of a profile besides its edges, checked on the host (the library would refuse them): returns the keyword
    arguments of Context.radial_profile without vel (v_cen None where it is to be taken from the inner fifth) and G.  Raises
    ValueError."""
    try:
        c = np.asarray(center, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"center must be three finite coordinates, not {center!r}") from None
    if c.shape != (3,) or not np.isfinite(c).all():
        raise ValueError(f"center must be three finite coordinates, not {center!r}")
    if geometry not in PROFILE_GEOMETRIES:
        raise ValueError(f"geometry must be one of {PROFILE_GEOMETRIES}, not {geometry!r}")
    frame = np.eye(3) if frame is None else check_rotation_matrix(frame)
    if half_height is None:
        hh = np.inf
    else:
        if geometry != "disc":
            raise ValueError(f"half_height = {half_height!r} needs geometry='disc'")
        if isinstance(half_height, (bool, str)):
            raise ValueError(f"half_height must be None or a number > 0, not {half_height!r}")
        try:
            hh = float(half_height)
        except (TypeError, ValueError):
            raise ValueError(f"half_height must be None or a number > 0, not {half_height!r}") from None
        if not hh > 0:
            raise ValueError(f"half_height must be None or a number > 0, not {half_height!r}")
    if v_cen is not None:
        if not has_vel:
            raise ValueError(f"v_cen = {v_cen!r} needs velocities (vel=)")
        try:
            v_cen = np.asarray(v_cen, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"v_cen must be None or three finite components, not {v_cen!r}") from None
        if v_cen.shape != (3,) or not np.isfinite(v_cen).all():
            raise ValueError(f"v_cen must be None or three finite components, not {v_cen!r}")
    if G is not None:
        G = _positive_length("G", G)
    return dict(edges=edges, geometry=PROFILE_GEOMETRIES.index(geometry), center=c.copy(), v_cen=v_cen, frame=frame,
                half_height=hh), G


class Profile:
    """A radial profile built from the raw sums of tsp_radial_profile by NumPy alone.  geometry "sphere": spherical shells;
    "disc": cylindrical annuli.  Per bin (arrays of n_bins): .edges (n_bins + 1), .rbins (the midpoints, as pynbody), .n (the
    members), .mass, .mass_enc (the mass inside each bin's outer edge: info["mass_inner"] plus the cumulative sum), .r_mean
    (sum m s / mass), .density (sphere: mass over the shell's volume; disc: the surface density, mass over the annulus' area)
    and, with velocities, the mass-weighted mean of each velocity component and its dispersion sqrt(max(<c^2> - <c>^2, 0)) --
    sphere: .v_r, .v_phi, .v_theta, .sigma_r, .sigma_phi, .sigma_theta; disc: .v_R, .v_phi, .v_z, .sigma_R, .sigma_phi, .sigma_z
    -- and .j (n_bins, 3), the specific angular momentum sum m d x u / mass in the caller's frame; without velocities these are
    None.  .v_circ = sqrt(G * mass_enc / edges[1:]) when G was given, else None.  Empty bins have zero mass and NaN means.
    .info: n_valid, n_inner, n_binned, mass_inner.  .sums and .count are the raw arrays."""

    COMPONENTS = {"sphere": ("r", "phi", "theta"), "disc": ("R", "phi", "z")}

    def __init__(self, edges, count, sums, info, geometry="sphere", G=None, with_velocities=True):
        if geometry not in PROFILE_GEOMETRIES:
            raise ValueError(f"geometry must be one of {PROFILE_GEOMETRIES}, not {geometry!r}")
        self.geometry = geometry
        self.edges = np.asarray(edges, dtype=np.float64)
        self.count = self.n = np.asarray(count, dtype=np.int64)
        self.sums = np.asarray(sums, dtype=np.float64)
        n_bins = len(self.edges) - 1
        if self.edges.ndim != 1 or n_bins < 1 or self.n.shape != (n_bins,) or self.sums.shape != (n_bins, 11):
            raise ValueError(f"a profile of {n_bins} bins needs count ({n_bins},) and sums ({n_bins}, 11), not {self.n.shape} and "
                             f"{self.sums.shape}")
        self.info = dict(info)
        lo, hi = self.edges[:-1], self.edges[1:]
        self.rbins = 0.5 * (lo + hi)
        self.mass = self.sums[:, 0].copy()
        self.mass_enc = float(self.info.get("mass_inner", 0.0)) + np.cumsum(self.mass)
        extent = 4.0 / 3.0 * np.pi * (hi ** 3 - lo ** 3) if geometry == "sphere" else np.pi * (hi ** 2 - lo ** 2)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.density = self.mass / extent
            self.r_mean = self.sums[:, 1] / self.mass
            self.j = None
            for k, name in enumerate(self.COMPONENTS[geometry]):
                mean = sigma = None
                if with_velocities:
                    mean = self.sums[:, 2 + k] / self.mass
                    sigma = np.sqrt(np.maximum(self.sums[:, 5 + k] / self.mass - mean * mean, 0.0))
                setattr(self, "v_" + name, mean)
                setattr(self, "sigma_" + name, sigma)
            if with_velocities:
                self.j = self.sums[:, 8:11] / self.mass[:, None]
            self.v_circ = None if G is None else np.sqrt(float(G) * self.mass_enc / hi)

    def __len__(self):
        return len(self.rbins)


def compute_profile(ctx, pos, mass, vel, kwargs, G=None):
    """The Profile of checked arguments (check_moments_arrays, profile_edges, check_profile_arguments) on an existing context.
    v_cen None with velocities: the mean velocity of the inner fifth of the sphere of the outermost edge (sphere_moments'
    default, what orientation uses)."""
    kwargs = dict(kwargs)
    columns = None if vel is None else (vel[:, 0], vel[:, 1], vel[:, 2])
    if vel is None:
        kwargs["v_cen"] = np.zeros(3)
    elif kwargs["v_cen"] is None:
        r = float(kwargs["edges"][-1])
        kwargs["v_cen"] = ctx.sphere_moments(pos[:, 0], pos[:, 1], pos[:, 2], mass, vel=columns, center=kwargs["center"], r=r,
                                             r_vel=VEL_RADIUS_FRACTION * r)["v_cen"]
    raw = ctx.radial_profile(pos[:, 0], pos[:, 1], pos[:, 2], mass, vel=columns, **kwargs)
    info = {k: raw[k] for k in ("n_valid", "n_inner", "n_binned", "mass_inner")}
    info["v_cen"] = np.asarray(kwargs["v_cen"], dtype=np.float64)
    return Profile(kwargs["edges"], raw["count"], raw["sums"], info, PROFILE_GEOMETRIES[kwargs["geometry"]], G, vel is not None)


def check_virial_arguments(center, rho_threshold, r_max, refinements):
    try:
        c = np.asarray(center, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"center must be three finite coordinates, not {center!r}") from None
    if c.shape != (3,) or not np.isfinite(c).all():
        raise ValueError(f"center must be three finite coordinates, not {center!r}")
    if isinstance(refinements, bool) or not isinstance(refinements, (int, np.integer)) or not 0 <= refinements <= 8:
        raise ValueError(f"refinements must be an integer from 0 to 8, not {refinements!r}")
    return c.copy(), _positive_length("rho_threshold", rho_threshold), _positive_length("r_max", r_max), int(refinements)


def find_virial_radius(shell_masses, rho_threshold, r_max, refinements=3):
    """The virial radius by the rule of topsy_amd.virial_radius, from shell_masses(edges) -> (mass per shell, mass inside
    edges[0]).  Returns (radius, (lower, upper) = the last bracket).  Raises ValueError without a crossing."""
    edges = profile_edges("log", VIRIAL_BINS, r_max / VIRIAL_LOG_SPAN, r_max)
    for level in range(refinements + 1):
        mass, mass_inner = shell_masses(edges)
        enclosed = np.concatenate([[mass_inner], mass_inner + np.cumsum(mass)])
        rho = 3.0 * enclosed / (4.0 * np.pi * edges ** 3)
        below = rho < rho_threshold
        if level == 0:
            crossing = np.flatnonzero(~below[:-1] & below[1:])
            if len(crossing) == 0:
                raise ValueError(f"the mean enclosed density never falls from above to below rho_threshold = {rho_threshold!r} "
                                 f"between r_max / {VIRIAL_LOG_SPAN:g} and r_max = {r_max!r}: it runs from {rho[0]!r} to {rho[-1]!r}")
            k = int(crossing[0]) + 1
        else:
            # the bracket's lower edge was above the threshold and its upper edge below: the first edge below it
            inside = np.flatnonzero(below[1:])
            k = int(inside[0]) + 1 if len(inside) else len(edges) - 1
        lower, upper = float(edges[k - 1]), float(edges[k])
        if level < refinements:
            edges = profile_edges("lin", VIRIAL_BINS, lower, upper)
    fraction = (rho[k - 1] - rho_threshold) / (rho[k - 1] - rho[k]) if rho[k - 1] > rho[k] else 0.0
    return lower + min(max(float(fraction), 0.0), 1.0) * (upper - lower), (lower, upper)


def compute_virial_radius(ctx, pos, mass, center, rho_threshold, r_max, refinements):
    """find_virial_radius of checked arguments on an existing context (tsp_radial_profile: shells, no velocities)."""
    def shell_masses(edges):
        raw = ctx.radial_profile(pos[:, 0], pos[:, 1], pos[:, 2], mass, edges=edges, geometry=0, center=center)
        return raw["sums"][:, 0], raw["mass_inner"]
    return find_virial_radius(shell_masses, rho_threshold, r_max, refinements)


VELOCITY_QUANTITIES = ("v_div", "vorticity")     # what an ArrayDataLoader with vel= derives from the velocities


class ArrayDataLoader(AbstractDataLoader):
    """Particles given as numpy arrays (e.g. pulled from a pynbody snapshot by the caller:
    snap['pos'], snap['smooth'], snap['mass'], ...; reference PynbodyDataInMemory, loader.py:79-154).

    smooth=None: the snapshot has no smoothing lengths (dark matter, stars).  The loader then records that it needs them
    (`needs_smoothing`); ParticleBuffers computes them on the GPU from the n_smooth nearest neighbours before the upload
    (the reference calls pynbody.sph.smooth there, loader.py:222-240) and hands them back through set_smooth().

    'rho' is always a quantity, as it is for every pynbody family (the reference hands any such name to the renderer,
    loader.py:123-127): quantities["rho"] when the caller supplied one, else the gather-form SPH density of the particles,
    computed on the GPU at the first get_named_quantity("rho") -- by the visualizer's context once ParticleBuffers has set it
    (set_density_context), else by a context of its own -- and cached; set_density() restores it from the caller's cache.

    With vel, 'v_div' and 'vorticity' are quantities as well, after 'rho' (pynbody derives v_div, v_curl and vorticity the same
    way, on the host): the difference-form SPH divergence of the velocity and the float32 norm of its curl
    (tsp_sph_velocity_gradient), computed on first use on the same context as 'rho' -- after the smoothing lengths and 'rho'
    where those are missing -- and cached; get_velocity_gradient() returns (div, curl), set_velocity_gradient() restores them
    from the caller's cache.  A name the caller supplied in quantities= is returned as given.  Unanswerable particles carry NaN.

    center: where the view opens (the reference centres the snapshot at load, loader.py:201-217).  "none": the origin;
    "all": the shrinking-sphere centre of every particle; "zoom": that of the lightest mass species (mass < 1.01 * mass.min());
    three coordinates: that point.  get_initial_center() computes the centre on the GPU (tsp_shrink_sphere_center) on first use
    -- on the same context as 'rho', from the host arrays, on the first device when there are several -- and caches it;
    set_initial_center() restores it from the caller's cache.  The particles are not moved: the camera is.

    halos: the halo catalogue (arrays carry none).  "fof": friends-of-friends groups found on the GPU (tsp_fof_groups) with the
    defaults of topsy_amd.friends_of_friends, in the periodic box of periodicity_scale when one is given; a dict of its keywords
    (linking_length, b, min_members); or the caller's own integer (n,) labels (halo N is label N, anything <= 0 is no halo;
    permuted with the other arrays under with_cells).  get_halos() computes the catalogue on first use, on the same context as
    'rho', and caches it; set_halos() restores it from the caller's cache.  With a catalogue, center="halo-N" (N >= 1, 1 = the
    largest halo; the reference's --center halo-N, loader.py:203-206) opens the view on the shrinking-sphere centre of the
    members of halo N (get_halo_center(N): in a periodic box the members are first unwrapped by nearest image around the
    lowest-index member, and the centre is in those coordinates).  Out of scope: periodic wrapping of the displacements inside the
    shrinking sphere itself, and DeviceSyntheticLoader (no host arrays).

    vel, orient: the angle the view opens at.  vel is the (n, 3) velocities (kept on the host, permuted with the other arrays under
    with_cells; not resident).  orient="faceon" / "sideon" turns the view so that the disc inside the sphere of radius
    orient_radius around the initial centre (whatever center= produced) is seen face-on / edge-on: along the angular momentum about
    the mean velocity of the inner fifth of that sphere (orient_method "angmom", the default with vel; pynbody.analysis.angmom),
    or along the minor axis of the particles' second-moment tensor ("shape", the default without).  orient_radius is required:
    no single length suits every snapshot.  get_initial_rotation() computes the matrix on the GPU (tsp_sphere_moments) on first
    use, on the same context as 'rho', and caches it (orient_moments holds the moments); set_initial_rotation() restores it from
    the caller's cache.  orientation() gives the matrix for any sphere.  Out of scope: periodic wrapping of the displacements.

    eps: the gravitational softening, one length >= 0 or one per particle (permuted with the other arrays under with_cells).
    With it 'phi' is a quantity, listed after the other derived names (every pynbody snapshot has one): the potential of every
    particle from all the others, Plummer-softened with the source's length, G = 1 -- a direct sum on the GPU
    (tsp_gravity_direct) on first use, on the same context as 'rho', cached as float32.  It costs n^2 pairs; above
    config.GRAVITY_DIRECT_MAX_PAIRS the first use raises ValueError instead.  rotation_curve() is the midplane rotation curve
    (topsy_amd.rotation_curve) from the same arrays.  Without eps nothing changes: names, order, errors.
    gravity="tree" computes 'phi' by the Barnes-Hut tree (tsp_gravity_tree, opening angle gravity_theta) instead: O(n log n), not
    subject to config.GRAVITY_DIRECT_MAX_PAIRS, masses >= 0; the default "direct" leaves every name, order and error as it was."""

    # reference PynbodyDataInMemory.get_rgb_masses (loader.py:115-121): (band, weight) per rgb channel
    RGB_BANDS = (("I", 0.5), ("V", 1.0), ("U", 1.0))

    def __init__(self, device=None, pos=None, smooth=None, mass=None, quantities=None, rgb=None,
                 units="kpc", periodicity_scale=None, with_cells=False, band_magnitudes=None, n_smooth=None,
                 center="none", halos=None, vel=None, orient="none", orient_radius=None, orient_method=None, eps=None,
                 gravity="direct", gravity_theta=0.5):
        super().__init__(device)
        from . import gravity as gravity_checks
        self._gravity_method = gravity_checks.check_method(gravity, "gravity")
        self._gravity_theta = gravity_checks.check_theta(gravity_theta)
        self._pos = np.asarray(pos, dtype=np.float32)
        self._eps = None                 # the gravitational softening: a float, or float32 (n,) in this loader's order
        self._phi = None                 # the computed potential ('phi' with eps=), in this loader's order
        if eps is not None:
            from . import gravity
            self._eps = gravity.check_eps(eps, len(self._pos))
        self._vel = None if vel is None else np.asarray(vel, dtype=np.float32)
        if self._vel is not None and (self._pos.ndim != 2 or self._vel.shape != self._pos.shape or self._pos.shape[1] != 3):
            raise ValueError(f"vel must have shape (n, 3) like pos, not {self._vel.shape} (pos: {self._pos.shape})")
        self._orient_option = orient
        self._orient_radius = self._orient_method = None
        self._rotation = None            # the initial rotation once known (float64 (3, 3))
        self.orient_moments = None       # what tsp_sphere_moments reported for it
        if orient != "none":
            self._orient_method = check_orient_arguments(orient, orient_method, self._vel is not None)
            if orient_radius is None:
                raise ValueError(f"orient={orient!r} needs orient_radius, the radius (in the units of pos) of the sphere around "
                                 f"the centre whose particles define the disc: no single length suits every snapshot "
                                 f"(pynbody's own default is a fixed 5 kpc)")
            self._orient_radius = _positive_length("orient_radius", orient_radius)
        elif orient_method is not None and orient_method not in ORIENT_METHODS:
            raise ValueError(f"orient_method must be None or one of {ORIENT_METHODS}, not {orient_method!r}")
        self._halos_option = check_halos_option(halos, len(self._pos), periodicity_scale)
        self._halos = None               # the catalogue once known
        self._halo_centers = {}          # N -> centre of halo N (float64 (3,))
        self._halo_properties = None     # the HaloProperties of the catalogue once computed
        self._center_option = check_center_option(center, self._halos_option)
        self._center = None              # the initial centre once known (float64 (3,))
        self.needs_smoothing = smooth is None
        self.n_smooth = config.SMOOTH_NEIGHBOURS if n_smooth is None else n_smooth
        if self.needs_smoothing or n_smooth is not None:
            self.n_smooth, _ = check_smoothing_arguments(self.n_smooth, periodicity_scale if self.needs_smoothing else None)
        self._smooth = None if smooth is None else np.asarray(smooth, dtype=np.float32)
        self._mass = np.asarray(mass, dtype=np.float32)
        self._quantities = {k: np.asarray(v, dtype=np.float32) for k, v in (quantities or {}).items()}
        self._rgb = None if rgb is None else np.asarray(rgb, dtype=np.float32)
        # SSP magnitudes per band (snap['I_mag'], ...): the rgb masses derive from them, on the device when rendered
        self._mags = None if band_magnitudes is None else {k: np.asarray(v, dtype=np.float64) for k, v in band_magnitudes.items()}
        self._units = units
        self._period = periodicity_scale
        self._rho = None                 # the computed density ('rho' when the caller supplied none), in this loader's order
        self._density_context = None
        self._velocity_gradient = None   # the computed (div (n,), curl (n, 3)) of vel, in this loader's order
        self._vorticity = None           # the norm of that curl
        if self.needs_smoothing:
            if self._pos.ndim != 2 or self._pos.shape[1] != 3:
                raise ValueError(f"pos must have shape (n, 3), not {self._pos.shape}")
            if len(self._pos) != len(self._mass):
                raise ValueError("pos and mass must have the same length")
        elif not (len(self._pos) == len(self._smooth) == len(self._mass)):
            raise ValueError("pos, smooth and mass must have the same length")
        if isinstance(self._center_option, str) and self._center_option != "none":
            if self._pos.ndim != 2 or self._pos.shape[1] != 3:
                raise ValueError(f"center={self._center_option!r} needs pos of shape (n, 3), not {self._pos.shape}")
            if self._mass.shape != (len(self._pos),) or len(self._pos) == 0:
                raise ValueError(f"center={self._center_option!r} needs one mass per particle: mass has shape {self._mass.shape}, "
                                 f"pos {self._pos.shape}")
        if with_cells:
            # cell sort + shuffle inside cells, as PynbodyDataInMemory.__init__ (loader.py:88-97)
            lo, hi = self._pos.min(), self._pos.max()
            pad = config.CELL_LAYOUT_FRACTIONAL_PADDING * (hi - lo)
            self._cell_layout, order = cell_layout.CellLayout.from_positions(self._pos, lo - pad, hi + pad,
                                                                              config.DEFAULT_CELLS_NSIDE)
            order = order[self._cell_layout.randomize_within_cells()]
            self._pos, self._mass = self._pos[order], self._mass[order]
            if self._smooth is not None:
                self._smooth = self._smooth[order]
            self._quantities = {k: v[order] for k, v in self._quantities.items()}
            if self._rgb is not None:
                self._rgb = self._rgb[order]
            if self._mags is not None:
                self._mags = {k: v[order] for k, v in self._mags.items()}
            if isinstance(self._halos_option, np.ndarray):
                self._halos_option = self._halos_option[order]
            if self._vel is not None:
                self._vel = self._vel[order]
            if isinstance(self._eps, np.ndarray):
                self._eps = self._eps[order]

    def __len__(self):
        return len(self._pos)

    def get_positions(self):
        return self._pos

    def get_smooth(self):
        if self._smooth is None:
            raise RuntimeError("no smoothing lengths yet: they are computed on the GPU when the particles are uploaded")
        return self._smooth

    def set_smooth(self, smooth):
        """Smoothing lengths in this loader's particle order (computed by ParticleBuffers when smooth=None was given)."""
        smooth = np.asarray(smooth, dtype=np.float32)
        if smooth.shape != (len(self),):
            raise ValueError(f"smooth must have shape ({len(self)},), not {smooth.shape}")
        self._smooth = smooth

    def get_mass(self):
        return self._mass

    def get_named_quantity(self, name):
        if name == "rho" and name not in self._quantities:
            return self._density()
        if name in VELOCITY_QUANTITIES and name not in self._quantities and self._vel is not None:
            return self._derived_velocity_quantity(name)
        if name == "phi" and name not in self._quantities and self._eps is not None:
            return self._potential()
        return self._quantities[name]

    def get_quantity_names(self):
        names = list(self._quantities)
        if "rho" not in self._quantities:
            names.append("rho")
        if self._vel is not None:
            names += [name for name in VELOCITY_QUANTITIES if name not in self._quantities]
        if self._eps is not None and "phi" not in self._quantities:
            names.append("phi")
        return names

    def get_softening(self):
        """The gravitational softening of eps=: a float, float32 (n,) in this loader's order, or None."""
        return self._eps

    def _gravity_arrays(self):
        if self._pos.ndim != 2 or self._pos.shape[1] != 3 or self._mass.shape != (len(self._pos),):
            raise ValueError(f"gravity needs pos of shape (n, 3) and one mass per particle, not {self._pos.shape} and "
                             f"{self._mass.shape}")
        return self._pos, self._mass

    def _potential(self):
        """'phi': the potential of every particle from all the others (tsp_gravity_direct, G = 1), float32 like every quantity;
        computed on first use on the context that computes 'rho', and cached."""
        if self._phi is None:
            from . import gravity
            pos, mass = self._gravity_arrays()
            method, theta = self._gravity_method, self._gravity_theta
            if method == "direct":
                gravity.check_pair_count(len(pos), len(pos), "'phi'")
            else:
                gravity.check_tree_masses(mass)
            pot = self._with_context(lambda ctx: gravity.compute_gravity(ctx, pos, mass, self._eps, None, want_acc=False,
                                                                         method=method, theta=theta))[0]
            self._phi = pot.astype(np.float32)
        return self._phi

    def rotation_curve(self, radii, center=None, frame=None, eps=None, G=1.0, method="direct", theta=0.5):
        """The RotationCurve (topsy_amd.rotation_curve) of the particles about `center` (None: the initial centre) in `frame`,
        found on the GPU (tsp_gravity_direct, or tsp_gravity_tree with method="tree") from the host arrays; eps=None: the loader's
        own softening (eps=)."""
        from . import gravity
        pos, mass = self._gravity_arrays()
        eps = self._eps if eps is None else gravity.check_eps(eps, len(pos))
        if eps is None:
            raise ValueError("no softening length: pass eps= here or to from_arrays / ArrayDataLoader")
        center = self.get_initial_center() if center is None else center
        radii, c, frame, G = gravity.check_radii(radii), gravity.check_center(center), gravity.check_frame(frame), gravity.check_G(G)
        method, theta = gravity.check_method(method), gravity.check_theta(theta)
        if method == "tree":
            gravity.check_tree_masses(mass)
        return self._with_context(lambda ctx: gravity.compute_rotation_curve(ctx, pos, mass, eps, radii, c, frame, G, method, theta))

    def set_density_context(self, context):
        """The context that computes 'rho' on first use (ParticleBuffers hands over its own; None: one made for the call)."""
        self._density_context = context

    def set_density(self, rho):
        """The density 'rho' in this loader's particle order (e.g. from the caller's cache, next to set_smooth): it is then
        not computed.  A supplied quantities["rho"] is never replaced."""
        rho = np.asarray(rho, dtype=np.float32)
        if rho.shape != (len(self),):
            raise ValueError(f"rho must have shape ({len(self)},), not {rho.shape}")
        if "rho" in self._quantities:
            raise ValueError("the caller supplied quantities['rho']; it is used as given")
        self._rho = rho

    def _density(self, ctx=None):
        """The computed density; ctx: the context of a caller that already holds one (_with_context)."""
        if self._rho is None:
            period = self._period or 0.0
            if self._pos.ndim != 2 or self._pos.shape[1] != 3:
                raise ValueError(f"pos must have shape (n, 3), not {self._pos.shape}")
            check_smoothing_arguments(self.n_smooth, self._period)

            def work(ctx):
                x, y, z = self._pos[:, 0], self._pos[:, 1], self._pos[:, 2]
                if self._smooth is None:
                    self.set_smooth(ctx.smoothing_lengths(x, y, z, self.n_smooth, period))
                self._rho = ctx.sph_sum(x, y, z, self._smooth, self._mass, period)
            if ctx is None:
                self._with_context(work)
            else:
                work(ctx)
        return self._rho

    def get_velocity_gradient(self):
        """(div (n,), curl (n, 3)) float32 of the velocities in this loader's particle order: the SPH estimates of
        tsp_sph_velocity_gradient, computed on the GPU on first use -- after the smoothing lengths and 'rho' where those are
        missing (a supplied quantities["rho"] is the rho that is used) -- and cached."""
        if self._vel is None:
            raise KeyError("no velocities were supplied (vel=): there is no velocity gradient")
        if self._velocity_gradient is None:
            period = self._period or 0.0

            def work(ctx):
                rho = self._quantities["rho"] if "rho" in self._quantities else self._density(ctx)
                x, y, z = self._pos[:, 0], self._pos[:, 1], self._pos[:, 2]
                v = self._vel
                if self._smooth is None:        # (a density restored by set_density, smoothing lengths not yet computed)
                    check_smoothing_arguments(self.n_smooth, self._period)
                    self.set_smooth(ctx.smoothing_lengths(x, y, z, self.n_smooth, period))
                return ctx.sph_velocity_gradient(x, y, z, self._smooth, self._mass, rho, v[:, 0], v[:, 1], v[:, 2], period)
            self._velocity_gradient = self._with_context(work)
        return self._velocity_gradient

    def set_velocity_gradient(self, div, curl):
        """The velocity divergence (n,) and curl (n, 3) in this loader's particle order (e.g. from the caller's cache, next to
        set_density): they are then not computed."""
        div, curl = np.asarray(div, dtype=np.float32), np.asarray(curl, dtype=np.float32)
        if div.shape != (len(self),):
            raise ValueError(f"div must have shape ({len(self)},), not {div.shape}")
        if curl.shape != (len(self), 3):
            raise ValueError(f"curl must have shape ({len(self)}, 3), not {curl.shape}")
        if self._vel is None:
            raise ValueError("the loader has no velocities (vel=): 'v_div' and 'vorticity' are not among its quantities")
        self._velocity_gradient = (div, curl)
        self._vorticity = None

    def _derived_velocity_quantity(self, name):
        div, curl = self.get_velocity_gradient()
        if name == "v_div":
            return div
        if self._vorticity is None:
            cx, cy, cz = curl[:, 0], curl[:, 1], curl[:, 2]
            with np.errstate(over="ignore", invalid="ignore"):
                self._vorticity = np.sqrt((cx * cx + cy * cy) + cz * cz)      # float32, this order
        return self._vorticity

    def _with_context(self, work):
        """work(ctx) on the visualizer's context once it was handed over (set_density_context), else on one made for the call."""
        ctx = self._density_context
        own = ctx is None
        if own:
            from . import _native
            ctx = _native.Context(1, 2, self._device if isinstance(self._device, int) else 0)
        try:
            return work(ctx)
        finally:
            if own:
                ctx.close()

    def get_halos(self):
        """The halo catalogue (FofCatalogue) of halos=: computed on the GPU on first use unless the labels were supplied."""
        if self._halos is None:
            if self._halos_option is None:
                raise ValueError("no halo catalogue: pass halos='fof', a dict of friends-of-friends keywords or your own labels")
            if isinstance(self._halos_option, np.ndarray):
                self._halos = FofCatalogue(self._halos_option)
            else:
                ll, b, min_members, period = check_fof_arguments(periodicity_scale=self._period, **self._halos_option)
                pos = check_fof_positions(self._pos)
                if ll is None:
                    ll = fof_linking_length(pos, b, period)      # (raises before a context exists)
                self._halos = self._with_context(lambda ctx: compute_fof_catalogue(ctx, pos, ll, b, min_members, period))
        return self._halos

    def set_halos(self, labels):
        """The halo labels in this loader's particle order (e.g. from the caller's cache, next to set_smooth / set_density):
        the catalogue is then not computed."""
        labels = check_halo_labels(labels, len(self))
        if self._halos_option is None:
            self._halos_option = labels
        self._halos = FofCatalogue(labels)
        self._halo_centers = {}
        self._halo_properties = None

    def get_halo_properties(self):
        """The HaloProperties (topsy_amd.halo_properties) of the catalogue of halos=, with this loader's vel, eps and
        periodicity_scale: computed on the GPU on first use, on the same context as 'rho', and cached; set_halos drops them."""
        if getattr(self, "_halo_properties", None) is None:
            from . import halos
            catalogue = self.get_halos()
            pos = halos.check_positions(self._pos)
            mass = halos.check_mass(self._mass, len(pos))
            labels, n_groups = halos.check_group(catalogue, len(pos))
            vel = halos.check_vel(self._vel, len(pos))
            period = halos.check_period(self._period or None)
            tree_above = halos.check_tree_above(None)
            self._halo_properties = self._with_context(lambda ctx: halos.compute_halo_properties(
                ctx, pos, mass, labels, n_groups, vel, self._eps, None, period, 1.0, tree_above, self._gravity_theta))
        return self._halo_properties

    def get_halo_center(self, n):
        """The shrinking-sphere centre (float64 (3,)) of the members of halo n, found on the GPU and cached."""
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError(f"halo numbers are integers >= 1, not {n!r}")
        n = int(n)
        if n not in self._halo_centers:
            members = self.get_halos().members(n)
            if len(members) == 0:
                raise ValueError(f"halo {n} has no members")
            if self._pos.ndim != 2 or self._pos.shape[1] != 3 or self._mass.shape != (len(self._pos),):
                raise ValueError(f"a halo centre needs pos of shape (n, 3) and one mass per particle, not {self._pos.shape} "
                                 f"and {self._mass.shape}")
            pos = self._pos[members].astype(np.float64)
            if self._period:
                # one image of the halo: every member by nearest image around the lowest-index member
                d = pos - pos[0]
                pos = pos[0] + (d - self._period * np.rint(d / self._period))
            pos = pos.astype(np.float32)
            mass = self._mass[members]
            cut, r0, shrink, min_particles = check_center_arguments("all")
            self._halo_centers[n], self.center_info = self._with_context(lambda ctx: ctx.shrink_sphere_center(
                pos[:, 0], pos[:, 1], pos[:, 2], mass, mass_cut_factor=cut, r_start=r0, shrink_factor=shrink,
                min_particles=min_particles))
        return self._halo_centers[n]

    def get_initial_center(self):
        if isinstance(self._center_option, str) and self._center_option == "none":
            return super().get_initial_center()
        if self._center is None:
            if not isinstance(self._center_option, str):
                self._center = self._center_option
            elif self._center_option.startswith("halo-"):
                self._center = self.get_halo_center(int(self._center_option[5:]))
            else:
                cut, r0, shrink, min_particles = check_center_arguments(self._center_option)
                self._center, self.center_info = self._with_context(lambda ctx: ctx.shrink_sphere_center(
                    self._pos[:, 0], self._pos[:, 1], self._pos[:, 2], self._mass, mass_cut_factor=cut, r_start=r0,
                    shrink_factor=shrink, min_particles=min_particles))
        return self._center

    def set_initial_center(self, center):
        """The initial centre (e.g. from the caller's cache, next to set_smooth / set_density): it is then not computed."""
        center = np.asarray(center, dtype=np.float64)
        if center.shape != (3,) or not np.isfinite(center).all():
            raise ValueError(f"center must be three finite coordinates, not {center!r}")
        if isinstance(self._center_option, str) and self._center_option == "none":
            self._center_option = center.copy()
        self._center = center.copy()

    def get_velocities(self):
        """The (n, 3) float32 velocities in this loader's particle order, or None."""
        return self._vel

    def orientation(self, orient, radius, center=None, method=None, vel_radius=None, up=(0, 1, 0)):
        """(matrix float64 (3, 3), moments dict): the rotation that shows the particles inside the sphere of `radius` around
        `center` (None: the initial centre) face-on or side-on, from their moments found on the GPU (tsp_sphere_moments)."""
        method = check_orient_arguments(orient, method, self._vel is not None)
        center = self.get_initial_center() if center is None else center
        c, r, r_vel = check_moments_arguments(center, radius, vel_radius, self._vel is not None)
        pos, mass, vel = check_moments_arrays(self._pos, self._mass, self._vel)
        moments = self._with_context(lambda ctx: compute_moments(ctx, pos, mass, vel, c, r, r_vel))
        return orientation_matrix(moments, orient, method, up), moments

    def profile(self, r_max=None, center=None, r_min=0.0, n_bins=100, bins="lin", geometry="sphere", frame=None, half_height=None,
                v_cen=None, G=None):
        """The radial Profile of the particles about `center` (None: the initial centre), found on the GPU
        (tsp_radial_profile) from the host arrays, with the velocities when the loader has them: the arguments of
        topsy_amd.radial_profile."""
        edges = profile_edges(bins, n_bins, r_min, r_max)
        center = self.get_initial_center() if center is None else center
        kwargs, G = check_profile_arguments(center, edges, geometry, frame, half_height, v_cen, G, self._vel is not None)
        pos, mass, vel = check_moments_arrays(self._pos, self._mass, self._vel)
        return self._with_context(lambda ctx: compute_profile(ctx, pos, mass, vel, kwargs, G))

    def _phase_array(self, role, name):
        """The per-particle array a phase diagram names: a loader quantity (derived ones are computed on first use), "mass" or
        "smooth".  ValueError for any other name."""
        if name == "mass":
            return self._mass
        if name == "smooth":
            return self.get_smooth()
        if not isinstance(name, str) or name not in self.get_quantity_names():
            raise ValueError(f"{role} = {name!r} names no per-particle array: the loader has {self.get_quantity_names()}, "
                             f"'mass' and 'smooth'")
        return self.get_named_quantity(name)

    def phase_diagram(self, x, y, weight="mass", value=None, x_range=None, y_range=None, bins=(256, 256), x_log=True, y_log=True,
                      edges=None, return_index=False):
        """The PhaseDiagram (topsy_amd.phase_diagram) of two named per-particle arrays -- e.g. phase_diagram("rho", "temp"): the
        mass in each cell of the (rho, T) plane -- found on the GPU (tsp_histogram_2d) from the host arrays.  x, y, weight and value
        name a loader quantity ('rho', 'v_div', 'vorticity' and 'phi' are computed on first use as get_named_quantity does), "mass"
        or "smooth"; weight=None counts particles, value=None leaves the mean and the dispersion out.  Both axes are logarithmic
        unless told otherwise; the other keywords are topsy_amd.phase_diagram's."""
        from . import phase
        columns = [self._phase_array(role, name) for role, name in (("x", x), ("y", y))]
        columns += [None if name is None else self._phase_array(role, name) for role, name in (("weight", weight), ("value", value))]
        xa, ya, w, v, edges_x, edges_y = phase.check_phase_arguments(*columns, x_range, y_range, bins, x_log, y_log, edges)
        return self._with_context(lambda ctx: phase.compute_phase_diagram(ctx, xa, ya, w, v, edges_x, edges_y, x_log, y_log,
                                                                          return_index))

    def sample_lattice(self, lattice_spec, quantity=None):
        """{"rho", "smooth"[, "mean"]} of topsy_amd.lattice.sample on the lattice `lattice_spec` (dict: origin, du, dv, dw, shape),
        found on the GPU (tsp_sph_sample_lattice) from the host arrays in the loader's periodic box; quantity: the name of the
        loader quantity whose kernel-weighted mean is "mean" (KeyError if there is none of that name)."""
        from . import lattice
        if self._pos.ndim != 2 or self._pos.shape[1] != 3 or self._mass.shape != (len(self._pos),):
            raise ValueError(f"a lattice needs pos of shape (n, 3) and one mass per particle, not {self._pos.shape} and "
                             f"{self._mass.shape}")
        n_smooth, period = check_smoothing_arguments(self.n_smooth, self._period)
        if quantity is not None and quantity not in self.get_quantity_names():
            raise KeyError(f"no quantity named {quantity!r}: the loader has {self.get_quantity_names()}")
        n_finite = int(np.isfinite(self._pos).all(axis=1).sum())
        if n_finite < n_smooth:
            raise ValueError(f"{n_finite} particles have finite coordinates; n_smooth = {n_smooth} needs at least as many")
        values = None if quantity is None else np.asarray(self.get_named_quantity(quantity), dtype=np.float32)
        pos, mass = np.asarray(self._pos, dtype=np.float32), np.asarray(self._mass, dtype=np.float32)
        return self._with_context(lambda ctx: lattice.sample(ctx, pos, mass, values, n_smooth, period, lattice_spec))

    def virial_radius(self, rho_threshold, r_max, center=None, refinements=3):
        """The radius about `center` (None: the initial centre) inside which the mean density is rho_threshold, by the rule of
        topsy_amd.virial_radius, found on the GPU from the host arrays."""
        center = self.get_initial_center() if center is None else center
        c, rho_threshold, r_max, refinements = check_virial_arguments(center, rho_threshold, r_max, refinements)
        pos, mass, _ = check_moments_arrays(self._pos, self._mass, None)
        return self._with_context(lambda ctx: compute_virial_radius(ctx, pos, mass, c, rho_threshold, r_max, refinements))[0]

    def get_initial_rotation(self):
        if self._rotation is None:
            if self._orient_option == "none":
                return super().get_initial_rotation()
            self._rotation, self.orient_moments = self.orientation(self._orient_option, self._orient_radius,
                                                                   method=self._orient_method)
        return self._rotation

    def set_initial_rotation(self, matrix):
        """The initial rotation (e.g. from the caller's cache, next to set_initial_center): it is then not computed."""
        self._rotation = check_rotation_matrix(matrix)

    def get_quantity_label(self, quantity_name):
        return "density" if quantity_name is None else quantity_name

    def get_rgb_masses(self):
        if self._rgb is not None:
            return self._rgb
        if self._mags is None:
            raise KeyError("no rgb band masses were supplied")
        # _effective_mass_for_band / get_rgb_masses of the reference (loader.py:112-121), on the host
        rgb = np.empty((len(self), 3), dtype=np.float32)
        for c, (band, weight) in enumerate(self.RGB_BANDS):
            rgb[:, c] = (10 ** (-0.4 * self._mags[band])) * weight
        rgb[np.isnan(rgb)] = 0.0
        return rgb

    def get_band_magnitudes(self):
        """(mags (3, n) float64, weights (3, 3) float64) for the device-side contraction (tsp_upload_band_magnitudes), or None."""
        if self._rgb is not None or self._mags is None:
            return None
        mags = np.stack([self._mags[band] for band, _ in self.RGB_BANDS])
        return mags, np.diag([w for _, w in self.RGB_BANDS]).astype(np.float64)

    def get_position_units(self):
        return self._units

    def get_periodicity_scale(self):
        return self._period

    def get_initial_view_width(self):
        return float(np.ptp(self._pos)) if self._period is None else self._period / 2


class DeviceSyntheticLoader(AbstractDataLoader):
    """TestDataLoader's distribution generated ON the GPU by a counter-based generator
    (tsp_generate_synthetic), for sizes that must not be materialised in numpy (1e8-1e9):
    shard [first, first+count) of an n_total-particle snapshot.  The arrays never visit the host;
    ParticleBuffers recognises this loader and skips the upload."""
    on_device = True

    def __init__(self, device=None, n_total=config.TEST_DATA_NUM_PARTICLES_DEFAULT, first=0, count=None, seed=1337,
                 h_cap=0.0, spatial_order=True):
        super().__init__(device)
        self.n_total = int(n_total)
        self.first = int(first)
        self.count = self.n_total - self.first if count is None else int(count)
        self.seed = seed
        self.h_cap = float(h_cap)
        self.spatial_order = spatial_order

    def __len__(self):
        return self.count

    def _not_on_host(self, *a):
        raise RuntimeError("DeviceSyntheticLoader keeps its arrays on the GPU; use Context.download_particles")

    get_positions = get_smooth = get_mass = get_rgb_masses = _not_on_host

    def get_named_quantity(self, name):
        if name != "test-quantity":
            raise KeyError("Unknown quantity name")
        return None     # generated on device

    def get_quantity_names(self):
        return ["test-quantity"]

    def get_quantity_label(self, quantity_name):
        return "test density" if quantity_name is None else "test quantity"

    def get_position_units(self):
        return "kpc"

    def get_periodicity_scale(self):
        return None
