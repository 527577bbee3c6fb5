"""Gravity for arrays: the host side of topsy_amd.gravity_direct, topsy_amd.gravity_tree and topsy_amd.rotation_curve (C:
tsp_gravity_direct, tsp_gravity_tree).

The GPU forms the softened sums with G = 1; this module checks the arguments, places the probes of a rotation curve, and
multiplies by G.  Everything but the two compute_* functions runs without a GPU."""
import numpy as np

from . import config


def check_arrays(pos, mass, eps):
    """(pos (n, 3), mass float32 (n,), eps: a Python float >= 0 or float32 (n,)).  pos keeps its dtype (rotation_curve subtracts
    the centre in float64 before the cast)."""
    pos = np.asarray(pos)
    if pos.dtype.kind not in "fiu":
        pos = pos.astype(np.float64)
    if pos.ndim != 2 or pos.shape[1] != 3:
        raise ValueError(f"pos must have shape (n, 3), not {pos.shape}")
    if len(pos) == 0:
        raise ValueError("pos must have at least one particle")
    mass = np.asarray(mass, dtype=np.float32)
    if mass.shape != (len(pos),):
        raise ValueError(f"pos and mass must have the same length: mass has shape {mass.shape}, not ({len(pos)},)")
    return pos, mass, check_eps(eps, len(pos))


def check_eps(eps, n):
    """The softening: one finite length >= 0 (returned as a float) or one per particle (float32 (n,); a non-finite entry leaves
    its source out, as the library does)."""
    if eps is None:
        raise ValueError("eps, the softening length (one number, or one per particle), is required")
    try:
        e = np.asarray(eps, dtype=np.float32)
    except (TypeError, ValueError):
        raise ValueError(f"eps must be a number or an array of {n} numbers, not {eps!r}") from None
    if e.ndim == 0:
        if not np.isfinite(e) or e < 0:
            raise ValueError(f"eps must be finite and >= 0, not {eps!r}")
        return float(e)
    if e.shape != (n,):
        raise ValueError(f"eps must be a number or have shape ({n},), not {e.shape}")
    return e


def check_G(G):
    try:
        g = float(G)
    except (TypeError, ValueError):
        g = np.nan
    if not np.isfinite(g) or g <= 0:
        raise ValueError(f"G must be a finite number > 0, not {G!r}")
    return g


def check_theta(theta):
    """The tree's opening angle: a finite number in [0, 1] (0 accepts no node: the direct sum in Morton order)."""
    try:
        t = float(theta)
    except (TypeError, ValueError):
        t = np.nan
    if not np.isfinite(t) or t < 0 or t > 1:
        raise ValueError(f"theta must be a finite number in [0, 1], not {theta!r}")
    return t


def check_method(method, name="method"):
    if method not in ("direct", "tree"):
        raise ValueError(f"{name} must be 'direct' or 'tree', not {method!r}")
    return method


def check_tree_masses(mass):
    """The tree needs masses >= 0 (a centre of mass); NaN passes (that particle exerts nothing)."""
    with np.errstate(invalid="ignore"):
        negative = np.nonzero(np.asarray(mass) < 0)[0]
    if len(negative):
        raise ValueError(f"the tree needs masses >= 0: mass[{negative[0]}] = {mass[negative[0]]!r} ({len(negative)} negative in all)")


def check_targets(targets):
    t = np.asarray(targets, dtype=np.float32)
    if t.ndim != 2 or t.shape[1] != 3 or len(t) == 0:
        raise ValueError(f"targets must have shape (k, 3) with k >= 1, not {t.shape}")
    return t


def check_pair_count(n_src, n_tgt, what):
    """ValueError above config.GRAVITY_DIRECT_MAX_PAIRS: a direct sum costs n_src * n_tgt pairs, and nothing cuts it short."""
    pairs = int(n_src) * int(n_tgt)
    if pairs > config.GRAVITY_DIRECT_MAX_PAIRS:
        raise ValueError(f"{what} is a direct sum of {n_src} x {n_tgt} = {pairs:.3g} pairs, above the limit "
                         f"config.GRAVITY_DIRECT_MAX_PAIRS = {config.GRAVITY_DIRECT_MAX_PAIRS:.3g}: raise the limit, or sum over "
                         f"fewer particles")
    return pairs


def check_radii(radii):
    r = np.atleast_1d(np.asarray(radii, dtype=np.float64))
    if r.ndim != 1 or len(r) == 0 or not np.isfinite(r).all() or (r <= 0).any():
        raise ValueError(f"radii must be one or more finite numbers > 0, not {radii!r}")
    return r


def check_center(center):
    c = np.asarray(center, dtype=np.float64)
    if c.shape != (3,) or not np.isfinite(c).all():
        raise ValueError(f"center must be three finite coordinates, not {center!r}")
    return c


def check_frame(frame):
    if frame is None:
        return np.eye(3)
    from . import loader
    return loader.check_rotation_matrix(frame)


def rotation_probes(radii, frame):
    """The four probes of every radius as offsets from the centre, float64 (n, 4, 3): +R e1, -R e1, +R e2, -R e2 with e1, e2 the
    first two rows of `frame` (the disc's plane when the third row is its axis)."""
    e1, e2 = frame[0], frame[1]
    units = np.stack([e1, -e1, e2, -e2])
    return radii[:, None, None] * units[None, :, :]


def centred_positions(pos, center):
    """pos - center formed in float64, then rounded to float32: near the centre the sources keep the digits that a float32
    subtraction of two large coordinates would lose."""
    return (np.asarray(pos, dtype=np.float64) - center[None, :]).astype(np.float32)


class RotationCurve:
    """The midplane rotation curve and potential of topsy_amd.rotation_curve: .radii (n,), .v_circ (n,), .pot (n,), .acc
    (n, 4, 3) (the accelerations at the four probes of every radius, in the caller's axes) and .probes (n, 4, 3) (their offsets
    from the centre, as float32 saw them)."""

    def __init__(self, radii, probes, pot, acc, G=1.0):
        n = len(radii)
        self.radii = np.asarray(radii, dtype=np.float64)
        self.probes = np.asarray(probes, dtype=np.float64).reshape(n, 4, 3)
        self.acc = G * np.asarray(acc, dtype=np.float64).reshape(n, 4, 3)
        pot4 = G * np.asarray(pot, dtype=np.float64).reshape(n, 4)
        # v^2 = -a . (p - center) at a probe: the centripetal acceleration times the radius; an outward pull counts as 0
        v2 = -(self.acc * self.probes).sum(axis=2)
        self.v_circ = np.sqrt(np.maximum(v2, 0.0)).mean(axis=1)
        self.pot = pot4.mean(axis=1)

    def __len__(self):
        return len(self.radii)


def compute_gravity(ctx, pos32, mass, eps, targets32, want_pot=True, want_acc=True, method="direct", theta=0.5):
    x, y, z = (np.ascontiguousarray(pos32[:, k]) for k in range(3))
    t = None if targets32 is None else [np.ascontiguousarray(targets32[:, k]) for k in range(3)]
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(pos32).all(axis=1) & np.isfinite(mass) & (True if np.ndim(eps) == 0 else np.isfinite(eps))
    if not valid.any():
        raise ValueError("no particle has finite coordinates, a finite mass and a finite softening length")
    if method == "tree":
        check_tree_masses(mass)
        return ctx.gravity_tree(x, y, z, mass, eps, targets=t, theta=theta, want_pot=want_pot, want_acc=want_acc)
    return ctx.gravity_direct(x, y, z, mass, eps, targets=t, want_pot=want_pot, want_acc=want_acc)


def compute_rotation_curve(ctx, pos, mass, eps, radii, center, frame, G, method="direct", theta=0.5):
    """rotation_curve() on a context: arguments already checked."""
    probes = rotation_probes(radii, frame).reshape(-1, 3).astype(np.float32)
    pot, acc, _ = compute_gravity(ctx, centred_positions(pos, center), mass, eps, probes, method=method, theta=theta)
    return RotationCurve(radii, probes, pot, acc, G)
