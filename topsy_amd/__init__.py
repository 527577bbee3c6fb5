"""topsy_amd -- MI355X-native SPH particle-splatting backend for topsy's render path.

    import topsy_amd
    vis = topsy_amd.test(1000, render_resolution=200)      # as reference topsy.test(...)
    vis.scale = 200.0
    img = vis.get_sph_presentation_image()                 # (200, 200, 4) uint8

The GPU work goes through libtopsy_splat.so (include/topsy_splat.h).  There is no CPU fallback.
"""
import numpy as np

from . import config
from .drawreason import DrawReason

__version__ = "0.1.0"


def test(nparticle=config.TEST_DATA_NUM_PARTICLES_DEFAULT, **kwargs):
    """Visualizer over the seeded synthetic snapshot (mirror of reference topsy.test, __init__.py:180-187)."""
    from . import visualizer, loader
    kwargs.pop("canvas_class", None)
    return visualizer.Visualizer(data_loader_class=loader.TestDataLoader, data_loader_args=(nparticle,),
                                 data_loader_kwargs={"with_cells": kwargs.pop("with_cells", False),
                                                     "periodic": kwargs.get("periodic_tiling", False)},
                                 **kwargs)


def from_arrays(pos, smooth, mass, quantities=None, rgb=None, with_cells=False, n_smooth=None, periodicity_scale=None,
                center="none", halos=None, vel=None, orient="none", orient_radius=None, orient_method=None, eps=None,
                gravity="direct", gravity_theta=0.5, **kwargs):
    """Visualizer over caller-supplied numpy arrays (e.g. taken from a pynbody snapshot).

    smooth=None computes the smoothing lengths on the GPU from the n_smooth (default config.SMOOTH_NEIGHBOURS) nearest
    neighbours, in the periodic box of side periodicity_scale if one is given; vis.data_loader.get_smooth() returns them.

    'rho' is always a quantity (vis.quantity_name = "rho"; the bivariate map's default): quantities["rho"] if given, else
    the SPH density of the particles, computed on the GPU on first use (sph_density) and cached on the loader --
    vis.data_loader.get_named_quantity("rho") returns it, set_density() restores it from the caller's own cache.

    With vel, 'v_div' and 'vorticity' are quantities too (vis.quantity_name = "v_div"): the SPH divergence of the velocity and the
    norm of its curl, computed on the GPU on first use (sph_velocity_gradient) and cached on the loader --
    vis.data_loader.get_velocity_gradient() returns (div, curl), set_velocity_gradient() restores them.

    center: where the view opens -- "none" (the origin), "all" (the shrinking-sphere centre of the particles, found on the GPU:
    shrink_sphere_center), "zoom" (that of the lightest mass species) or three coordinates.  vis.data_loader.get_initial_center()
    returns it, set_initial_center() restores it from the caller's own cache.

    halos: the halo catalogue -- "fof" (friends-of-friends groups found on the GPU: friends_of_friends, in the periodic box of
    periodicity_scale if one is given), a dict of its keywords (linking_length, b, min_members), or your own integer (n,) labels
    (halo N is label N; <= 0: no halo).  With it center="halo-N" opens the view on halo N (1 = the largest) and
    vis.centre_on_halo(N) jumps there; vis.data_loader.get_halos() returns the catalogue, set_halos() restores it.
    vis.halo_properties() is the HaloProperties of the catalogue (halo_properties, with this call's vel, eps and
    periodicity_scale; computed on the GPU on first use and cached), and vis.centre_on_halo(N, at="com" | "pot") centres on a
    halo's centre of mass or potential minimum instead of its shrinking-sphere centre.

    vel, orient: the angle the view opens at -- orient="faceon" or "sideon" turns the view (no particle moves) so that the disc
    inside the sphere of radius orient_radius (required: a length in the units of pos) around the initial centre, whatever center=
    produced, is seen face-on or edge-on, as pynbody.analysis.angmom.faceon / sideon do.  vel, the (n, 3) velocities, gives the
    axis as the angular momentum about the mean velocity of the inner fifth of the sphere (orient_method="angmom", the default
    with vel); without it the axis is the minor axis of the particles' second-moment tensor ("shape").  The moments are found on
    the GPU (sphere_moments); vis.data_loader.get_initial_rotation() returns the matrix, set_initial_rotation() restores it,
    and vis.orient("faceon" | "sideon", radius) re-orients on whatever the view is centred on.

    vis.profile(r_max, ...) is the radial profile (radial_profile) of what the view shows -- about the view's centre, in the
    view's frame: after orient("faceon"), geometry="disc" gives the rotation curve -- and vis.scale_to_virial(rho_threshold,
    r_max) sets the view's scale to the virial radius (virial_radius) of what it is centred on.

    eps: the gravitational softening, one length or one per particle.  With it 'phi' is a quantity too, listed after the
    other derived names (vis.quantity_name = "phi"): the potential of every particle from all the others with G = 1, a direct
    sum on the GPU on first use (gravity_direct; n^2 pairs, refused above config.GRAVITY_DIRECT_MAX_PAIRS) and cached on the
    loader -- and vis.rotation_curve(radii) is the disc's rotation curve and midplane potential (rotation_curve) about the view's
    centre in the view's frame.  gravity="tree" computes 'phi' by the Barnes-Hut tree instead (gravity_tree with the opening
    angle gravity_theta; O(n log n), no pair limit, masses >= 0)."""
    from . import visualizer, loader
    return visualizer.Visualizer(data_loader_class=loader.ArrayDataLoader,
                                 data_loader_kwargs={"pos": pos, "smooth": smooth, "mass": mass,
                                                     "quantities": quantities, "rgb": rgb, "with_cells": with_cells,
                                                     "n_smooth": n_smooth, "periodicity_scale": periodicity_scale,
                                                     "center": center, "halos": halos, "vel": vel, "orient": orient,
                                                     "orient_radius": orient_radius, "orient_method": orient_method,
                                                     "eps": eps, "gravity": gravity, "gravity_theta": gravity_theta},
                                 **kwargs)


def smoothing_lengths(pos, n_smooth=config.SMOOTH_NEIGHBOURS, periodicity_scale=None, device_id=0):
    """SPH smoothing lengths of an (n, 3) position array on GPU `device_id`: half the distance to the n_smooth-th nearest
    particle, the particle itself included (pynbody's snap['smooth'] convention); NaN where a coordinate is not finite.
    periodicity_scale: side of a periodic box (None: open).  Returns float32 (n,), to be cached as the caller likes."""
    from . import _native, loader
    n_smooth, period = loader.check_smoothing_arguments(n_smooth, periodicity_scale)
    pos = np.asarray(pos, dtype=np.float32)
    if pos.ndim != 2 or pos.shape[1] != 3:
        raise ValueError(f"pos must have shape (n, 3), not {pos.shape}")
    n_finite = int(np.isfinite(pos).all(axis=1).sum())
    if n_finite < n_smooth:
        raise ValueError(f"{n_finite} particles have finite coordinates; n_smooth = {n_smooth} needs at least as many")
    ctx = _native.Context(1, 2, device_id)
    try:
        return ctx.smoothing_lengths(pos[:, 0], pos[:, 1], pos[:, 2], n_smooth, period)
    finally:
        ctx.close()


def _sph_arguments(pos, mass, smooth, n_smooth, periodicity_scale, vel=None, **others):
    """The arguments of sph_density / sph_mean / sph_velocity_gradient, checked on the host: float32 arrays of one length, pos
    (and vel, which comes back as arrays["vel"]) (n, 3)."""
    from . import loader
    n_smooth, period = loader.check_smoothing_arguments(n_smooth, periodicity_scale)
    pos = np.asarray(pos, dtype=np.float32)
    if pos.ndim != 2 or pos.shape[1] != 3:
        raise ValueError(f"pos must have shape (n, 3), not {pos.shape}")
    if vel is not None:
        vel = np.asarray(vel, dtype=np.float32)
        if vel.ndim != 2 or vel.shape[1] != 3:
            raise ValueError(f"vel must have shape (n, 3), not {vel.shape}")
        if len(vel) != len(pos):
            raise ValueError(f"pos and vel must have the same length: vel has shape {vel.shape}, not ({len(pos)}, 3)")
    arrays = {"mass": mass, "smooth": smooth, **others}
    for name, a in arrays.items():
        if a is None:
            continue
        arrays[name] = a = np.asarray(a, dtype=np.float32)
        if a.shape != (len(pos),):
            raise ValueError(f"pos and {name} must have the same length: {name} has shape {a.shape}, not ({len(pos)},)")
    if len(pos) == 0:
        raise ValueError("pos must have at least one particle")
    if smooth is None:
        n_finite = int(np.isfinite(pos).all(axis=1).sum())
        if n_finite < n_smooth:
            raise ValueError(f"{n_finite} particles have finite coordinates; n_smooth = {n_smooth} needs at least as many")
    if vel is not None:
        arrays["vel"] = vel
    return pos, arrays, n_smooth, period


def sph_density(pos, mass, smooth=None, n_smooth=config.SMOOTH_NEIGHBOURS, periodicity_scale=None, device_id=0):
    """SPH density at the particles of an (n, 3) position array on GPU `device_id` (C: tsp_sph_sum): the gather sum
    rho_i = sum_j mass_j W(|r_i - r_j|, smooth_i) with the M4 cubic spline of support 2 smooth_i -- pynbody's snap['rho'].
    smooth=None computes the smoothing lengths first (as smoothing_lengths does, from n_smooth neighbours) on the same
    context.  NaN where a coordinate is not finite or smooth is not finite and > 0.  Returns float32 (n,)."""
    from . import _native
    pos, arr, n_smooth, period = _sph_arguments(pos, mass, smooth, n_smooth, periodicity_scale)
    ctx = _native.Context(1, 2, device_id)
    try:
        x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
        h = ctx.smoothing_lengths(x, y, z, n_smooth, period) if arr["smooth"] is None else arr["smooth"]
        return ctx.sph_sum(x, y, z, h, arr["mass"], period)
    finally:
        ctx.close()


def sph_mean(pos, mass, smooth, values, rho=None, n_smooth=config.SMOOTH_NEIGHBOURS, periodicity_scale=None, device_id=0):
    """SPH interpolant of a per-particle quantity at the particles: sum_j (mass_j values_j / rho_j) W(|r_i - r_j|, smooth_i),
    the weights formed in float32.  rho=None computes the density first (sph_density), smooth=None the smoothing lengths, on
    the same context.  Weights of 0/0 or x/0 are the caller's data and propagate.  Returns float32 (n,)."""
    from . import _native
    pos, arr, n_smooth, period = _sph_arguments(pos, mass, smooth, n_smooth, periodicity_scale, values=values, rho=rho)
    if arr["values"] is None:
        raise ValueError("values must be an array of the same length as pos")
    ctx = _native.Context(1, 2, device_id)
    try:
        x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
        h = ctx.smoothing_lengths(x, y, z, n_smooth, period) if arr["smooth"] is None else arr["smooth"]
        rho = ctx.sph_sum(x, y, z, h, arr["mass"], period) if arr["rho"] is None else arr["rho"]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            a = arr["mass"] * arr["values"] / rho
        return ctx.sph_sum(x, y, z, h, a, period)
    finally:
        ctx.close()


def sph_velocity_gradient(pos, mass, vel, smooth=None, rho=None, n_smooth=config.SMOOTH_NEIGHBOURS, periodicity_scale=None,
                          device_id=0):
    """Divergence and curl of the (n, 3) velocities vel at the particles of an (n, 3) position array on GPU `device_id`
    (C: tsp_sph_velocity_gradient): the difference-form SPH estimates
    v_div_i = (1 / rho_i) sum_j mass_j (v_j - v_i) . grad_i W(r_ij, smooth_i) and
    v_curl_i = (1 / rho_i) sum_j mass_j grad_i W x (v_j - v_i), with the M4 cubic spline of support 2 smooth_i -- pynbody's
    snap['v_div'] and snap['v_curl'] (its 'vorticity' is the norm of the curl).  smooth=None computes the smoothing lengths first
    (from n_smooth neighbours), rho=None the density (sph_density), on the same context.  Exactly zero for a uniform velocity;
    biased low on disordered particles (about 0.77 of the true value on Poisson points with 32 neighbours), because rho contains
    the particle's own term.  NaN where a coordinate is not finite or smooth is not finite and > 0.  Returns (v_div (n,),
    v_curl (n, 3)) float32."""
    from . import _native
    if vel is None:
        raise ValueError("vel must have shape (n, 3): the velocities of the particles")
    pos, arr, n_smooth, period = _sph_arguments(pos, mass, smooth, n_smooth, periodicity_scale, vel=vel, rho=rho)
    ctx = _native.Context(1, 2, device_id)
    try:
        x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
        h = ctx.smoothing_lengths(x, y, z, n_smooth, period) if arr["smooth"] is None else arr["smooth"]
        rho = ctx.sph_sum(x, y, z, h, arr["mass"], period) if arr["rho"] is None else arr["rho"]
        v = arr["vel"]
        return ctx.sph_velocity_gradient(x, y, z, h, arr["mass"], rho, v[:, 0], v[:, 1], v[:, 2], period)
    finally:
        ctx.close()


def sph_grid(pos, mass, values=None, shape=(64, 64, 64), center=(0, 0, 0), size=None, rotation=None,
             n_smooth=config.SMOOTH_NEIGHBOURS, periodicity_scale=None, device_id=0):
    """SPH fields of an (n, 3) position array sampled on a regular 3-D grid on GPU `device_id` (C: tsp_sph_sample_lattice;
    pynbody's to_3d_grid): shape = (nu, nv, nw) samples at the cell centres of a box of side `size` (required: one length or
    three) centred on `center`, whose axes u, v, w are the rows of `rotation` (None: the identity).  The estimator is gather-form
    with the smoothing length taken at the sample point: smooth = half the distance from the point to its n_smooth-th nearest
    particle, rho = sum_j mass_j W(|r - r_j|, smooth) with the M4 cubic spline of support 2 smooth.  Returns a dict of float32
    arrays indexed [k][j][i], shape (nw, nv, nu): "rho", "smooth" and, with `values`, "mean" = sum m q W / sum m W, the
    kernel-weighted mean of values at the point (NaN where rho is 0 or NaN) -- and "points": the three float64 vectors (u, v, w) of
    the samples' offsets from `center` along the axes, sample (i, j, k) lying at center + u[i] rotation[0] + v[j] rotation[1] +
    w[k] rotation[2].  periodicity_scale: the side of a periodic box (None: open); the box may straddle its faces."""
    from . import lattice
    return lattice.sph_grid(pos, mass, values, shape=shape, center=center, size=size, rotation=rotation, n_smooth=n_smooth,
                            periodicity_scale=periodicity_scale, device_id=device_id)


def sph_slice(pos, mass, values=None, resolution=256, center=(0, 0, 0), size=None, rotation=None,
              n_smooth=config.SMOOTH_NEIGHBOURS, periodicity_scale=None, device_id=0):
    """SPH fields on the plane through `center` spanned by the first two rows of `rotation` (None: the x-y plane): sph_grid with
    shape = (resolution, resolution, 1).  size (required): the side of the square, or (side along u, side along v).  Returns the
    dict of sph_grid with (resolution, resolution) arrays indexed [j][i] and "points" = (u, v)."""
    from . import lattice
    n = lattice._count("resolution", resolution)
    if size is not None and np.ndim(size) != 0:
        try:
            size = tuple(size)
        except TypeError:
            size = ()
        if len(size) != 2:
            raise ValueError(f"size must be a finite number > 0 or two of them, not {size!r}")
        size = (size[0], size[1], 1.0)
    out = sph_grid(pos, mass, values, shape=(n, n, 1), center=center, size=size, rotation=rotation, n_smooth=n_smooth,
                   periodicity_scale=periodicity_scale, device_id=device_id)
    return {name: a[:2] if name == "points" else a[0] for name, a in out.items()}


def sph_ray(pos, mass, values=None, start=None, end=None, n_samples=256, n_smooth=config.SMOOTH_NEIGHBOURS,
            periodicity_scale=None, device_id=0):
    """SPH fields along the straight line from `start` to `end` (both required, both sampled; n_samples = 1 samples start):
    tsp_sph_sample_lattice on a lattice of shape (n_samples, 1, 1).  Returns the dict of sph_grid with (n_samples,) arrays and
    "points" = the (n_samples, 3) float64 coordinates of the samples."""
    from . import lattice
    return lattice.sph_ray(pos, mass, values, start=start, end=end, n_samples=n_samples, n_smooth=n_smooth,
                           periodicity_scale=periodicity_scale, device_id=device_id)


def shrink_sphere_center(pos, mass, select="all", r_start=None, shrink_factor=0.7, min_particles=100, device_id=0):
    """Shrinking-sphere centre (Power et al. 2003; pynbody.analysis.halo.center's default) of an (n, 3) position array on GPU
    `device_id` (C: tsp_shrink_sphere_center): starting from the centre of mass and a sphere of radius r_start (None: half the
    x extent), the centre moves to the mass-weighted mean of the particles inside a sphere shrunk by shrink_factor per step,
    until fewer than min_particles are inside.  select="zoom" uses the lightest mass species only (mass < 1.01 * mass.min(),
    the reference's center="zoom").  Particles with a non-finite coordinate or a mass that is not finite and > 0 take no part.
    Returns (center float64 (3,), dict(n_valid, n_inside, iterations, radius, mass_inside)).
    Out of scope: periodic wrapping of the displacements.  The centre of one halo: friends_of_friends(pos).members(N) selects
    its particles; from_arrays(..., halos="fof", center="halo-N") does both."""
    from . import _native, loader
    cut, r0, shrink, min_particles = loader.check_center_arguments(select, r_start, shrink_factor, min_particles)
    pos = np.asarray(pos, dtype=np.float32)
    if pos.ndim != 2 or pos.shape[1] != 3:
        raise ValueError(f"pos must have shape (n, 3), not {pos.shape}")
    mass = np.asarray(mass, dtype=np.float32)
    if mass.shape != (len(pos),):
        raise ValueError(f"pos and mass must have the same length: mass has shape {mass.shape}, not ({len(pos)},)")
    if len(pos) == 0:
        raise ValueError("pos must have at least one particle")
    with np.errstate(invalid="ignore"):
        if not (np.isfinite(pos).all(axis=1) & np.isfinite(mass) & (mass > 0)).any():
            raise ValueError("no particle has finite coordinates and a finite mass > 0")
    ctx = _native.Context(1, 2, device_id)
    try:
        return ctx.shrink_sphere_center(pos[:, 0], pos[:, 1], pos[:, 2], mass, mass_cut_factor=cut, r_start=r0,
                                        shrink_factor=shrink, min_particles=min_particles)
    finally:
        ctx.close()


def sphere_moments(pos, mass, vel=None, center=(0, 0, 0), radius=None, vel_radius=None, device_id=0):
    """Moments of the particles of an (n, 3) position array inside the sphere of `radius` (required) around `center`, on GPU
    `device_id` (C: tsp_sphere_moments), as a dict: n_valid, n_inside, mass, com (the offset of the centre of mass from center),
    S (sum m d_i d_j: xx, xy, xz, yy, yz, zz) and, with vel (n, 3), n_inside_vel, mass_vel and v_cen (the mean velocity inside
    vel_radius; None: radius / 5, the ratio of pynbody's 1 kpc to 5 kpc), L (sum m d x (v - v_cen)) and A (sum m |d| |v - v_cen|).
    Float64 sums of displacements formed in float64.  Particles with a non-finite coordinate or velocity or a mass that is not
    finite and > 0 take no part.  Out of scope: periodic wrapping of the displacements."""
    from . import _native, loader
    pos, mass, vel = loader.check_moments_arrays(pos, mass, vel)
    c, r, r_vel = loader.check_moments_arguments(center, radius, vel_radius, vel is not None)
    ctx = _native.Context(1, 2, device_id)
    try:
        return loader.compute_moments(ctx, pos, mass, vel, c, r, r_vel)
    finally:
        ctx.close()


def orientation(pos, mass, vel=None, center=(0, 0, 0), radius=None, vel_radius=None, orient="faceon", method=None, up=(0, 1, 0),
                device_id=0):
    """The rotation that shows the disc inside the sphere of `radius` around `center` face-on (orient="faceon": its axis toward
    the viewer) or edge-on ("sideon": its axis up the screen), as (matrix float64 (3, 3), the moments of sphere_moments).  The axis:
    method="angmom", the angular momentum L (the default with vel), or "shape", the minor axis of the second-moment tensor about
    the centre of mass (the default without).  The matrix is pynbody's calc_faceon_matrix: rows up x a, a x (up x a), a.
    ValueError where the sphere has no net rotation / no unique minor axis."""
    from . import loader
    method = loader.check_orient_arguments(orient, method, vel is not None)
    moments = sphere_moments(pos, mass, vel, center, radius, vel_radius, device_id)
    return loader.orientation_matrix(moments, orient, method, up), moments


def radial_profile(pos, mass, vel=None, center=(0, 0, 0), r_max=None, r_min=0.0, n_bins=100, bins="lin", geometry="sphere",
                   frame=None, half_height=None, v_cen=None, G=None, device_id=0):
    """The radial profile of the particles of an (n, 3) position array about `center`, on GPU `device_id` (C: tsp_radial_profile),
    as a Profile (topsy_amd/loader.py): pynbody.analysis.profile.Profile for arrays.  geometry="sphere": spherical shells, with
    the velocity components (v_r, v_phi, v_theta); "disc": cylindrical annuli about the third axis of `frame` (None: the identity;
    the matrix of topsy_amd.orientation(..., orient="faceon") puts the disc's axis there), members within |z'| <= half_height
    (None: any height), with (v_R, v_phi, v_z): v_phi is the rotation curve.  The bins: bins="lin" or "log" (needs r_min > 0)
    makes n_bins (1 to 512) bins between r_min and r_max (required), or bins = your own ascending edges.  With vel (n, 3) the
    velocities are taken about v_cen (None: the mean velocity of the inner fifth of the sphere of the outermost edge, as
    sphere_moments and orientation take it).  G: the gravitational constant in the caller's units, for Profile.v_circ.  Float64
    sums of displacements formed in float64; the same call returns the same bits.  Particles with a non-finite coordinate or
    velocity or a mass that is not finite and > 0 take no part.  Out of scope: periodic wrapping of the displacements."""
    from . import _native, loader
    pos, mass, vel = loader.check_moments_arrays(pos, mass, vel)
    edges = loader.profile_edges(bins, n_bins, r_min, r_max)
    kwargs, G = loader.check_profile_arguments(center, edges, geometry, frame, half_height, v_cen, G, vel is not None)
    ctx = _native.Context(1, 2, device_id)
    try:
        return loader.compute_profile(ctx, pos, mass, vel, kwargs, G)
    finally:
        ctx.close()


def gravity_direct(pos, mass, eps, targets=None, G=1.0, device_id=0):
    """The gravitational potential and acceleration of the particles of an (n, 3) position array at `targets` (k, 3), or at the
    particles themselves (None: a particle does not act on itself), by a direct sum on GPU `device_id` (C: tsp_gravity_direct):
    pot_i = -G sum_j mass_j / sqrt(|t_i - r_j|^2 + eps_j^2), acc_i = -G sum_j mass_j (t_i - r_j) / (|t_i - r_j|^2 + eps_j^2)^(3/2)
    -- Plummer softening with the source's length, pynbody's direct sum (snap['phi']).  eps: one softening length >= 0 or one
    per particle.  Pair terms are float32, the sums float64; the rounding stays within 64 * 2^-24 of the sum of the terms'
    magnitudes.  A particle with a non-finite coordinate, mass or eps exerts nothing; a target with a non-finite coordinate gets
    NaN; a pair at distance 0 with eps 0 contributes nothing.  The cost is n * k pairs: no tree, no periodic images.
    Returns (pot float64 (k,), acc float64 (k, 3))."""
    from . import _native, gravity
    pos, mass, eps = gravity.check_arrays(pos, mass, eps)
    G = gravity.check_G(G)
    t = None if targets is None else gravity.check_targets(targets)
    ctx = _native.Context(1, 2, device_id)
    try:
        pot, acc, _ = gravity.compute_gravity(ctx, np.asarray(pos, dtype=np.float32), mass, eps, t)
    finally:
        ctx.close()
    return G * pot, G * acc


def gravity_tree(pos, mass, eps, targets=None, theta=0.5, G=1.0, device_id=0):
    """gravity_direct's potential and acceleration by a Barnes-Hut tree on GPU `device_id` (C: tsp_gravity_tree): O(n log n)
    instead of n * k pairs, with no limit on the pair count.  The particles are sorted along a Morton curve; 32 consecutive ones
    are a leaf, 8 consecutive nodes a node of the next level, each with its mass, centre of mass, second moments and mean eps^2;
    targets are walked in groups of 64 (the particles themselves: neighbours along the curve; `targets`: in the order given, so
    pass neighbours next to each other), and a node farther from the group's box than its radius / theta acts as a softened
    monopole plus quadrupole, a nearer one is opened down to its particles.  theta in [0, 1]: 0 is the direct sum, 0.5 leaves 99 %
    of the accelerations within 1e-2 in the scenes of DESIGN.md.  Masses must be >= 0; everything else -- eps, G, non-finite
    particles and targets, the self pair -- as gravity_direct.  Returns (pot float64 (k,), acc float64 (k, 3))."""
    from . import _native, gravity
    pos, mass, eps = gravity.check_arrays(pos, mass, eps)
    G, theta = gravity.check_G(G), gravity.check_theta(theta)
    gravity.check_tree_masses(mass)
    t = None if targets is None else gravity.check_targets(targets)
    ctx = _native.Context(1, 2, device_id)
    try:
        pot, acc, _ = gravity.compute_gravity(ctx, np.asarray(pos, dtype=np.float32), mass, eps, t, method="tree", theta=theta)
    finally:
        ctx.close()
    return G * pot, G * acc


def rotation_curve(pos, mass, eps, radii, center=(0, 0, 0), frame=None, G=1.0, device_id=0, method="direct", theta=0.5):
    """The midplane rotation curve and potential of the particles of an (n, 3) position array, from direct sums of the softened
    forces at probe points (C: tsp_gravity_direct) on GPU `device_id`: what pynbody's disc profile takes v_circ and pot from
    (gravity.calc.midplane_rot_curve / midplane_potential).  pynbody's source was not at hand when this was written, so the
    rule stated here is the contract.  With the rows (e1, e2, e3) of `frame` (None: the identity; the matrix of
    topsy_amd.orientation(..., orient="faceon") puts the disc's axis in e3), every radius R of `radii` gets four probes,
    center + R e1, center - R e1, center + R e2, center - R e2; v_circ(R) is the mean over the four of
    sqrt(max(0, -a . (p - center))) with a the acceleration at the probe p, pot(R) the mean of the four potentials.  center is
    subtracted from pos in float64 before the sums are formed in float32, so that probes and nearby sources keep their digits.
    eps, G and the treatment of non-finite particles: as gravity_direct.  Unlike Profile.v_circ = sqrt(G M(<r) / r), which is
    exact for a spherical mass distribution only, this is right for a disc.  The cost is 4 len(radii) * n pairs.
    method="tree" forms the forces by gravity_tree with the opening angle `theta` instead (masses >= 0).
    Returns a RotationCurve (topsy_amd/gravity.py): .radii, .v_circ, .pot (n_radii,), .acc (n_radii, 4, 3)."""
    from . import _native, gravity
    pos, mass, eps = gravity.check_arrays(pos, mass, eps)
    radii, c, frame, G = gravity.check_radii(radii), gravity.check_center(center), gravity.check_frame(frame), gravity.check_G(G)
    method, theta = gravity.check_method(method), gravity.check_theta(theta)
    if method == "tree":
        gravity.check_tree_masses(mass)
    ctx = _native.Context(1, 2, device_id)
    try:
        return gravity.compute_rotation_curve(ctx, pos, mass, eps, radii, c, frame, G, method, theta)
    finally:
        ctx.close()


def virial_radius(pos, mass, center, rho_threshold, r_max, refinements=3, device_id=0):
    """The radius about `center` inside which the mean density is rho_threshold (pynbody.analysis.halo.virial_radius for arrays;
    rho_threshold is e.g. 200 times the critical density in the caller's units), on GPU `device_id` (C: tsp_radial_profile).
    The rule: with M(<r) the mass of the valid particles at a distance below r, the mean enclosed density is
    rho(r) = 3 M(<r) / (4 pi r^3).  Level 0 evaluates it at the 257 edges of 256 logarithmic bins on [r_max / 1024, r_max] and takes
    the first bin, going outward, at whose inner edge rho >= rho_threshold and at whose outer edge rho < rho_threshold: where
    the density first falls below the threshold on the way out from where it was above.  That bin is re-binned `refinements`
    times into 256 linear bins (the mass below the bracket comes with each call), each time keeping the bin that ends at the
    first edge with rho < rho_threshold.  The result is the linear interpolation of rho across the last bracket to
    rho_threshold.  Raises ValueError if level 0 finds no such bin (the threshold is never crossed downward inside r_max)."""
    from . import _native, loader
    pos, mass, _ = loader.check_moments_arrays(pos, mass, None)
    c, rho_threshold, r_max, refinements = loader.check_virial_arguments(center, rho_threshold, r_max, refinements)
    ctx = _native.Context(1, 2, device_id)
    try:
        return loader.compute_virial_radius(ctx, pos, mass, c, rho_threshold, r_max, refinements)[0]
    finally:
        ctx.close()


def friends_of_friends(pos, linking_length=None, b=0.2, min_members=20, periodicity_scale=None, device_id=0):
    """Friends-of-friends groups of an (n, 3) position array on GPU `device_id` (C: tsp_fof_groups): particles closer than
    linking_length are friends (nearest image in a periodic box of side periodicity_scale), the groups are the connected
    components.  linking_length=None: b times the mean separation (V / n_valid) ** (1/3), V = periodicity_scale ** 3 or the
    volume of the bounding box of the finite positions.  Returns a FofCatalogue: .group (int32 (n,): N >= 1 = the N-th largest
    group with at least min_members members, 0 = a smaller one, -1 = a non-finite coordinate), .sizes (int64, sizes[N - 1]),
    len(), .members(N), .linking_length, .info."""
    from . import _native, loader
    ll, b, min_members, period = loader.check_fof_arguments(linking_length, b, min_members, periodicity_scale)
    pos = loader.check_fof_positions(pos)
    if ll is None:
        ll = loader.fof_linking_length(pos, b, period)
    ctx = _native.Context(1, 2, device_id)
    try:
        return loader.compute_fof_catalogue(ctx, pos, ll, b, min_members, period)
    finally:
        ctx.close()


def group_potential(pos, mass, eps, group, periodicity_scale=None, G=1.0, tree_above=None, theta=0.5, device_id=0):
    """The self-potential of every halo of a catalogue on GPU `device_id`, in one call (C: tsp_group_potential): for particle i
    of halo N, -G sum over the other members j of N of mass_j / sqrt(|r_i - r_j|^2 + eps_j^2).  group: a FofCatalogue
    (friends_of_friends) or an integer (n,) label array, N >= 1 = halo N, 0 or less = no halo.  The sums are formed on float32
    offsets from each halo's first member (nearest image in a periodic box of side periodicity_scale), with the pair arithmetic
    and the error bound of gravity_direct.  A halo with more than tree_above members (None: config.HALO_TREE_MEMBERS) is summed
    by gravity_tree with the opening angle theta instead.  Returns float64 (n,): NaN for a particle in no halo and for one with
    a non-finite coordinate, mass or eps."""
    from . import _native, gravity, halos
    pos = halos.check_positions(pos)
    mass, eps = halos.check_mass(mass, len(pos)), gravity.check_eps(eps, len(pos))
    labels, n_groups = halos.check_group(group, len(pos))
    period, G, theta = halos.check_period(periodicity_scale), gravity.check_G(G), gravity.check_theta(theta)
    tree_above = halos.check_tree_above(tree_above)
    ctx = _native.Context(1, 2, device_id)
    try:
        return G * halos.compute_group_potential(ctx, pos, mass, eps, labels, n_groups, period, tree_above, theta)[0]
    finally:
        ctx.close()


def halo_properties(pos, mass, group, vel=None, eps=None, phi=None, periodicity_scale=None, G=1.0, tree_above=None, theta=0.5,
                    device_id=0):
    """The properties of every halo of a catalogue on GPU `device_id`, in one call (C: tsp_halo_properties): member count, mass,
    centre of mass, and about it the second moments, r_max, the half-mass radius and v_max = max sqrt(G M(<r) / r) (from the 10th
    member outward); with vel (n, 3) the mean velocity, dispersion, angular momentum and kinetic energy; with a potential the
    potential energy, the position of the potential minimum and the bound members and mass (0.5 |v - v_com|^2 + phi < 0).  The
    potential is phi (n,), taken as already containing G, or, with eps, group_potential(pos, mass, eps, group, ...).  group: a
    FofCatalogue or integer labels.  Everything is summed in float64 on offsets from each halo's first member (nearest image in
    a periodic box of side periodicity_scale).  Returns a HaloProperties (topsy_amd/halos.py)."""
    from . import _native, gravity, halos
    pos = halos.check_positions(pos)
    n = len(pos)
    mass, vel, phi = halos.check_mass(mass, n), halos.check_vel(vel, n), halos.check_phi(phi, n)
    eps = None if eps is None else gravity.check_eps(eps, n)
    labels, n_groups = halos.check_group(group, n)
    period, G, theta = halos.check_period(periodicity_scale), gravity.check_G(G), gravity.check_theta(theta)
    tree_above = halos.check_tree_above(tree_above)
    ctx = _native.Context(1, 2, device_id)
    try:
        return halos.compute_halo_properties(ctx, pos, mass, labels, n_groups, vel, eps, phi, period, G, tree_above, theta)
    finally:
        ctx.close()


def SurfaceView(visualizer, **colormap_params):
    """Surface rendering of `visualizer`'s scene (the reference's render_mode "surface"): the front-most sphere of every
    particle above a density cut, smoothed and lit.  render(), get_sph_image() ((R, R, 2) filtered (q, depth)),
    get_sph_presentation_image() ((R, R, 4) uint8), colormap_autorange(), view["depth_scale"] etc., density_cut_percentile."""
    from . import surface
    return surface.SurfaceView(visualizer, **colormap_params)


def PerspectiveView(visualizer, fov=60.0, near=None):
    """`visualizer`'s scene seen by a perspective camera, for fly-throughs: a view with a visualizer's whole interface (camera,
    quantity_name, render_mode, get_sph_image, get_sph_presentation_image, get_depth_image -- the distance from the viewer --,
    get_presentation_image((W, H)) and its 4:2:0 form) and a camera of its own that starts at the visualizer's, plus fov (degrees,
    inside (0, 180)), distance = scale / tan(fov / 2), near, far and dolly(delta).  The plane through the view centre fills the
    frame as in the orthographic view; fov -> 0 tends to it.  The GPU writes a perspective-transformed copy of the snapshot into a
    second context whenever the camera changes (tsp_project_perspective) and the unchanged pipeline draws it: a footprint is a
    disc, exact on the ray through its centre and good while its rays make a small angle with the optical axis.  A target of
    VisualizationRecorder, which records fov as well.  One GPU, no periodic tiling; no kinematic, cube or surface views in perspective; a second resident snapshot."""
    from . import perspective
    return perspective.PerspectiveView(visualizer, fov=fov, near=near)


def VelocityView(visualizer, v_ref="center", **parameters):
    """The kinematic maps of `visualizer`'s scene (needs from_arrays(..., vel=vel)): per pixel the mass-weighted mean
    line-of-sight velocity and its dispersion along the view axis, drawn on the GPU from resident velocities.  v_ref, subtracted
    from the velocities first: "center" (the mean velocity of the inner fifth of the sphere of radius vis.scale about what the
    view is centred on, the rule vis.profile uses), three components, or None (zero).  get_maps() (dict: surface_density, v_los,
    sigma_los, count), get_presentation_image("v_los" | "sigma_los") ((R, R, 4) uint8), view["v_los", "vmax"] etc.  After
    vis.orient("sideon", r) v_los is the picture of the rotation curve vis.profile gives.  view.frames("v_los" | "sigma_los") is
    the map with a visualizer's frame interface -- get_presentation_image((W, H)) under its colorbar and the scale bar, the 4:2:0
    planes -- and a target of VisualizationRecorder.  One GPU, no periodic tiling."""
    from . import kinematics
    return kinematics.VelocityView(visualizer, v_ref=v_ref, **parameters)


def velocity_maps(pos, smooth, mass, vel, rotation=None, center=(0, 0, 0), scale=config.DEFAULT_SCALE,
                  resolution=config.DEFAULT_RESOLUTION, v_ref=None, device_id=0):
    """The kinematic maps of arrays, without a visualizer, on GPU `device_id` (C: tsp_render in TSP_MODE_KINEMATIC +
    tsp_velocity_moments): the dict of VelocityView.get_maps for a camera looking along the third row of `rotation` (None: the
    identity) at `center` with half-width `scale` and `resolution` pixels a side.  v_ref: None (zero), three components or "center"."""
    from . import kinematics
    return kinematics.velocity_maps(pos, smooth, mass, vel, rotation=rotation, center=center, scale=scale, resolution=resolution,
                                    v_ref=v_ref, device_id=device_id)


def spectral_cube(pos, smooth, mass, vel, v_range=None, n_channels=64, sigma_v=0.0, sigma=None, rotation=None, center=(0, 0, 0),
                  scale=config.DEFAULT_SCALE, resolution=config.DEFAULT_RESOLUTION, v_ref=None, device_id=0):
    """The position-position-velocity cube of arrays, without a visualizer, on GPU `device_id` (C: tsp_spectral_cube): a
    topsy_amd.SpectralCube, data (n_channels, R, R) float32 over n_channels equal velocity channels of v_range (None: wide enough
    for every particle) at velocity_maps' camera, with moment(), spectrum() and pv().  A particle's line is a Gaussian of width
    sqrt(sigma_v^2 + sigma[i]^2) integrated over each channel.  VelocityView.get_cube() is the same at a visualizer's camera."""
    from . import spectral
    return spectral.spectral_cube(pos, smooth, mass, vel, v_range=v_range, n_channels=n_channels, sigma_v=sigma_v, sigma=sigma,
                                  rotation=rotation, center=center, scale=scale, resolution=resolution, v_ref=v_ref,
                                  device_id=device_id)


def phase_diagram(x, y, weights=None, values=None, x_range=None, y_range=None, bins=(256, 256), x_log=False, y_log=False, edges=None,
                  return_index=False, device=None):
    """The phase diagram of arrays on GPU `device` (None: 0; C: tsp_histogram_2d): a topsy_amd.PhaseDiagram (topsy_amd/phase.py) --
    per cell of a 2-D table over (x, y) the particle count, the sum of `weights` (None: the count) and, with `values`, their
    weighted mean and dispersion: pynbody's plot.rho_T / plot.generic.hist2d for arrays, e.g. phase_diagram(rho, temp, mass,
    x_log=True, y_log=True).  bins: an int or (nx, ny), 1 to 1024 each, between x_range / y_range (None: the minimum and the
    maximum of the axis' finite values -- for a logarithmic axis of its finite positive ones -- the upper end moved up by one
    float64 ulp so that the maximum is binned); x_log / y_log make the bins logarithmic; edges = (edges_x, edges_y) takes the
    caller's own ascending edges instead.  Bins are half-open, the last edge is outside.  Arrays are any float dtype, converted to
    float32; a particle with a non-finite x, y, weight or value takes no part; any finite weight is allowed.  The sums are
    float64 in a fixed order: the same call returns the same bits.  return_index keeps every particle's cell
    (PhaseDiagram.bin_index, PhaseDiagram.select).  Raises ValueError for mismatched lengths and bad arguments."""
    from . import _native, phase
    x, y, w, v, edges_x, edges_y = phase.check_phase_arguments(x, y, weights, values, x_range, y_range, bins, x_log, y_log, edges)
    ctx = _native.Context(1, 2, 0 if device is None else device)
    try:
        return phase.compute_phase_diagram(ctx, x, y, w, v, edges_x, edges_y, x_log, y_log, return_index)
    finally:
        ctx.close()


def __getattr__(name):
    """topsy_amd.VisualizationRecorder (movie recording and export, topsy_amd/recorder), topsy_amd.FofCatalogue and
    topsy_amd.Profile (topsy_amd/loader.py), topsy_amd.RotationCurve (topsy_amd/gravity.py), topsy_amd.SpectralCube
    (topsy_amd/spectral.py), topsy_amd.PhaseDiagram (topsy_amd/phase.py), imported on first use."""
    if name == "PhaseDiagram":
        from .phase import PhaseDiagram
        return PhaseDiagram
    if name == "SpectralCube":
        from .spectral import SpectralCube
        return SpectralCube
    if name == "RotationCurve":
        from .gravity import RotationCurve
        return RotationCurve
    if name == "FofCatalogue":
        from .loader import FofCatalogue
        return FofCatalogue
    if name == "HaloProperties":
        from .halos import HaloProperties
        return HaloProperties
    if name == "Profile":
        from .loader import Profile
        return Profile
    if name == "VisualizationRecorder":
        from .recorder import VisualizationRecorder
        return VisualizationRecorder
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def synthetic_on_device(n_total, first=0, count=None, h_cap=0.0, **kwargs):
    """Visualizer over a device-generated shard of the synthetic snapshot (1e8-1e9 particles)."""
    from . import visualizer, loader
    return visualizer.Visualizer(data_loader_class=loader.DeviceSyntheticLoader,
                                 data_loader_kwargs={"n_total": n_total, "first": first, "count": count,
                                                     "h_cap": h_cap},
                                 **kwargs)
