"""SPH fields sampled on a lattice of points (C: tsp_sph_sample_lattice): the host layer of sph_grid, sph_slice, sph_ray and
Visualizer.get_slice_image -- the argument checks, the lattice of each of them, and the one routine that turns the sums into
density, smoothing length and kernel-weighted mean.

A lattice is origin + i du + j dv + k dw for 0 <= (i, j, k) < (nu, nv, nw); every array that comes back is indexed [k][j][i]."""
import numpy as np

from . import config


def _vector(name, v):
    try:
        a = np.asarray(v, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be three finite numbers, not {v!r}") from None
    if a.shape != (3,) or not np.isfinite(a).all():
        raise ValueError(f"{name} must be three finite numbers, not {v!r}")
    return a


def _count(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
        raise ValueError(f"{name} must be an integer >= 1, not {v!r}")
    return int(v)


def box_lattice(shape, center, size, rotation=None):
    """The lattice of sph_grid: shape = (nu, nv, nw) samples at the cell centres of a box of side `size` (one number or three,
    along the three axes) centred on `center`, whose axes u, v, w are the rows of `rotation` (None: the identity).  Returns
    (dict(origin, du, dv, dw, shape), (u, v, w)): the offsets of the samples from `center` along each axis, float64 -- sample
    (i, j, k) lies at center + u[i] rotation[0] + v[j] rotation[1] + w[k] rotation[2].  Raises ValueError."""
    from . import loader
    try:
        dims = tuple(shape)
    except TypeError:
        raise ValueError(f"shape must be three integers >= 1, not {shape!r}") from None
    if len(dims) != 3:
        raise ValueError(f"shape must be three integers >= 1, not {shape!r}")
    dims = tuple(_count("every entry of shape", v) for v in dims)
    if dims[0] * dims[1] * dims[2] >= 2 ** 31:
        raise ValueError(f"shape {dims} has 2^31 points or more")
    c = _vector("center", center)
    if np.ndim(size) == 0:
        sides = np.full(3, loader._positive_length("size", size))
    else:
        try:
            sides = tuple(size)
        except TypeError:
            raise ValueError(f"size must be a finite number > 0 or three of them, not {size!r}") from None
        if len(sides) != 3:
            raise ValueError(f"size must be a finite number > 0 or three of them, not {size!r}")
        sides = np.array([loader._positive_length("every entry of size", v) for v in sides])
    rot = np.eye(3) if rotation is None else loader.check_rotation_matrix(rotation)
    step = sides / np.array(dims, dtype=np.float64)
    first = 0.5 * step - 0.5 * sides
    offsets = tuple(first[a] + step[a] * np.arange(dims[a], dtype=np.float64) for a in range(3))
    lattice = {"origin": c + first @ rot, "du": step[0] * rot[0], "dv": step[1] * rot[1], "dw": step[2] * rot[2], "shape": dims}
    return lattice, offsets


def slice_lattice(rotation_matrix, position_offset, scale, resolution):
    """The lattice of Visualizer.get_slice_image: the view's centre plane at `resolution` pixels a side.  Pixel (row, col) is the
    point centre_on_pixel(row, col) centres on at zero depth: -position_offset + rotation^T (x, y, 0) with
    x = ((col + 0.5) * 2 / R - 1) * scale, y = (1 - (row + 0.5) * 2 / R) * scale; i runs along the columns, j down the rows."""
    rot = np.asarray(rotation_matrix, dtype=np.float64)
    res = int(resolution)
    pixel = 2.0 * float(scale) / res
    corner = np.array([(0.5 * 2.0 / res - 1.0) * float(scale), (1.0 - 0.5 * 2.0 / res) * float(scale), 0.0])
    return {"origin": -np.asarray(position_offset, dtype=np.float64) + rot.T @ corner, "du": pixel * rot[0], "dv": -pixel * rot[1],
            "dw": rot[2].copy(), "shape": (res, res, 1)}


def sample(ctx, pos, mass, values, n_smooth, period, lattice):
    """{"rho", "smooth"[, "mean"]} float32 (nw, nv, nu) on context `ctx`: one tsp_sph_sample_lattice call with the fields (mass) or
    (mass * values, mass).  mean = sum m q W / sum m W, NaN where rho is 0 or NaN."""
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    if values is None:
        h, outs = ctx.sph_sample_lattice(x, y, z, [mass], n_smooth, period, **lattice)
        return {"rho": outs[0], "smooth": h}
    with np.errstate(over="ignore", invalid="ignore"):
        weighted = mass * values
    h, outs = ctx.sph_sample_lattice(x, y, z, [weighted, mass], n_smooth, period, **lattice)
    rho = outs[1]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        mean = np.where(rho == 0, np.float32(np.nan), outs[0] / rho).astype(np.float32)
    return {"rho": rho, "smooth": h, "mean": mean}


def _arguments(pos, mass, values, n_smooth, periodicity_scale):
    from . import _sph_arguments
    pos, arr, n_smooth, period = _sph_arguments(pos, mass, None, n_smooth, periodicity_scale, values=values)
    if arr["mass"] is None:
        raise ValueError("mass must be an array of the same length as pos")
    return pos, arr["mass"], arr["values"], n_smooth, period


def sph_grid(pos, mass, values=None, shape=(64, 64, 64), center=(0, 0, 0), size=None, rotation=None,
             n_smooth=config.SMOOTH_NEIGHBOURS, periodicity_scale=None, device_id=0):
    """topsy_amd.sph_grid (documented there)."""
    from . import _native
    pos, mass, values, n_smooth, period = _arguments(pos, mass, values, n_smooth, periodicity_scale)
    if size is None:
        raise ValueError("size is required: the side of the sampled box, a finite number > 0 or three of them")
    lattice, offsets = box_lattice(shape, center, size, rotation)
    ctx = _native.Context(1, 2, device_id)
    try:
        out = sample(ctx, pos, mass, values, n_smooth, period, lattice)
    finally:
        ctx.close()
    out["points"] = offsets
    return out


def sph_ray(pos, mass, values=None, start=None, end=None, n_samples=256, n_smooth=config.SMOOTH_NEIGHBOURS,
            periodicity_scale=None, device_id=0):
    """topsy_amd.sph_ray (documented there)."""
    from . import _native
    pos, mass, values, n_smooth, period = _arguments(pos, mass, values, n_smooth, periodicity_scale)
    n = _count("n_samples", n_samples)
    if start is None or end is None:
        raise ValueError("start and end are required: the two ends of the ray, three finite numbers each")
    a, b = _vector("start", start), _vector("end", end)
    if n >= 2 ** 31:
        raise ValueError(f"n_samples = {n}: 2^31 or more")
    step = (b - a) / (n - 1) if n > 1 else np.zeros(3)
    lattice = {"origin": a, "du": step, "dv": np.zeros(3), "dw": np.zeros(3), "shape": (n, 1, 1)}
    ctx = _native.Context(1, 2, device_id)
    try:
        out = sample(ctx, pos, mass, values, n_smooth, period, lattice)
    finally:
        ctx.close()
    out = {name: a3[0, 0] for name, a3 in out.items()}
    out["points"] = a[None, :] + np.arange(n, dtype=np.float64)[:, None] * step[None, :]
    return out
