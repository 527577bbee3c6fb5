"""numpy restatement of the two kinematic kernels (topsy_amd/csrc/tsp_kinematics.hip, include/topsy_splat.h "Kinematic maps"):
the per-particle weights in float32, one rounding per step, and the per-pixel moments in float64.  Every step is an IEEE
correctly rounded operation, so the device results must equal these bit for bit."""
import numpy as np

f32 = np.float32
NAN32 = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]


def line_of_sight(axis, v_ref):
    """(axis, v_ref) as the library holds them: float32, -0 as +0"""
    a, v = np.asarray(axis, dtype=f32) + f32(0.0), np.asarray(v_ref, dtype=f32) + f32(0.0)
    return a, v


def kinematic_colours(m, vel, axis, v_ref):
    """(r, g, b, u): the "colours" the rgb kernels are fed, before the division by h * h.  float32, in the header's order."""
    a, v = line_of_sight(axis, v_ref)
    m = np.asarray(m, dtype=f32)
    vx, vy, vz = (np.asarray(vel[:, k], dtype=f32) for k in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        t0 = (a[0] * (vx - v[0])).astype(f32)
        t1 = (a[1] * (vy - v[1])).astype(f32)
        t2 = (a[2] * (vz - v[2])).astype(f32)
        u = ((t0 + t1).astype(f32) + t2).astype(f32)
        r = m.copy()
        g = (m * u).astype(f32)
        b = (g * u).astype(f32)
    dead = ~(np.isfinite(m) & np.isfinite(u))
    r[dead] = g[dead] = b[dead] = f32(0.0)
    return r, g, b, u


def kinematic_weights(h, m, vel, axis, v_ref):
    """(wr, wg, wb) = (r, g, b) / (h * h): the form of oracle_np's rgb weights, rgb / (h * h)."""
    r, g, b, _ = kinematic_colours(m, vel, axis, v_ref)
    h = np.asarray(h, dtype=f32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        hh = (h * h).astype(f32)
        return (r / hh).astype(f32), (g / hh).astype(f32), (b / hh).astype(f32)


def velocity_moments(image):
    """(..., 4) float32 (S, A, B, n) -> (..., 4) float32 (S, mean, sigma, n)"""
    image = np.asarray(image, dtype=f32)
    S32, A32, B32 = image[..., 0], image[..., 1], image[..., 2]
    with np.errstate(invalid="ignore"):
        ok = (S32 > 0) & np.isfinite(S32) & np.isfinite(A32) & np.isfinite(B32)
    S = np.where(ok, S32, f32(1.0)).astype(np.float64)
    A, B = A32.astype(np.float64), B32.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        mean = A / S
        var = B / S - mean * mean
        var = np.where(var < 0.0, 0.0, var)
        sigma = np.sqrt(var)
        out = image.copy()
        out[..., 1] = np.where(ok, mean.astype(f32), NAN32)
        out[..., 2] = np.where(ok, sigma.astype(f32), NAN32)
    return out
