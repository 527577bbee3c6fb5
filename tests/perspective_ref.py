"""A NumPy float32 model of tsp_project_perspective's contract (include/topsy_splat.h "Perspective view"): the transformed
snapshot, the vertex weights and the bounds of every 512 particles, operation for operation, so that the device arrays can be
compared bit for bit."""
import numpy as np

BOUNDS_BLOCK = 512
F = np.float32


def camera(rot, offset, distance, near):
    """The camera as the float32 values the binding hands to the library."""
    return (np.asarray(rot, dtype=F).reshape(3, 3), np.asarray(offset, dtype=F).reshape(3), F(distance), F(near))


def view_coordinates(x, y, z, rot, offset):
    """(xv, yv, zv): float32, the additions and products in the header's order."""
    with np.errstate(all="ignore"):
        tx, ty, tz = (np.asarray(a, dtype=F) + offset[k] for k, a in enumerate((x, y, z)))
        return tuple((rot[k, 0] * tx + rot[k, 1] * ty) + rot[k, 2] * tz for k in range(3))


def project(arrays, rot, offset, distance, near):
    """arrays: dict of float32 arrays with x, y, z, h and optionally mass and r, g, b.  Returns the dict of the transformed arrays
    under the same names, plus "visible" (bool), "s" and "d"."""
    rot, offset, distance, near = camera(rot, offset, distance, near)
    with np.errstate(all="ignore"):
        xv, yv, zv = view_coordinates(arrays["x"], arrays["y"], arrays["z"], rot, offset)
        d = distance - zv
        visible = d >= near                      # False for NaN
        s = distance / d
        ss = s * s
        nan, zero = F(np.nan), F(0.0)
        out = {"x": np.where(visible, xv * s, nan), "y": np.where(visible, yv * s, nan), "z": np.where(visible, zv, nan),
               "h": np.where(visible, np.asarray(arrays["h"], dtype=F) * s, zero)}
        for name in ("mass", "r", "g", "b"):
            if name in arrays:
                out[name] = np.where(visible, np.asarray(arrays[name], dtype=F) * ss, zero)
    for v in out.values():
        assert v.dtype == F
    out.update(visible=visible, s=s, d=d)
    return out


def weights(h, mass):
    """weights_kernel's operations: mass / (h * h)."""
    with np.errstate(all="ignore"):
        h = np.asarray(h, dtype=F)
        return np.asarray(mass, dtype=F) / (h * h)


def block_bounds(x, y, z, h):
    """(blocks, 2, 4) float32: (xmin, ymin, zmin, hmax) and (xmax, ymax, zmax, 0) of every BOUNDS_BLOCK consecutive particles;
    NaN values are dropped, an empty minimum is +inf and an empty maximum -inf (block_bounds_kernel's rules)."""
    n = len(x)
    blocks = -(-n // BOUNDS_BLOCK)
    out = np.zeros((blocks, 2, 4), dtype=F)
    for b in range(blocks):
        sl = slice(b * BOUNDS_BLOCK, min((b + 1) * BOUNDS_BLOCK, n))
        for k, a in enumerate((x, y, z)):
            v = np.asarray(a[sl], dtype=F)
            v = v[~np.isnan(v)]
            out[b, 0, k] = v.min() if len(v) else np.inf
            out[b, 1, k] = v.max() if len(v) else -np.inf
        hh = np.asarray(h[sl], dtype=F)
        hh = hh[~np.isnan(hh)]
        out[b, 0, 3] = hh.max() if len(hh) else -np.inf
    return out


def fov_distance(scale, fov_degrees):
    """The distance from the viewer to the reference plane at which a half-width `scale` fills the field of view."""
    return scale / np.tan(np.radians(fov_degrees) / 2.0)
