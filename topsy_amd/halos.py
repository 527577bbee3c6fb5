"""Halo properties for arrays: the host side of topsy_amd.group_potential and topsy_amd.halo_properties (C: tsp_group_potential,
tsp_halo_properties).

The GPU sorts the particles by halo label and forms, in one call for the whole catalogue, the self-potential of every halo and the
per-halo reductions, with G = 1.  This module checks the arguments, sends the haloes that are too large for a direct sum to the
tree, applies G and names the columns.  Everything but the two compute_* functions runs without a GPU."""
import warnings

import numpy as np

from . import _native, config, gravity


def check_positions(pos):
    pos = np.asarray(pos)
    if pos.dtype.kind not in "fiu":
        raise ValueError(f"pos must be a numeric array, not dtype {pos.dtype}")
    if pos.ndim != 2 or pos.shape[1] != 3:
        raise ValueError(f"pos must have shape (n, 3), not {pos.shape}")
    if len(pos) == 0:
        raise ValueError("pos must have at least one particle")
    return np.ascontiguousarray(pos, dtype=np.float32)


def check_mass(mass, n):
    mass = np.asarray(mass, dtype=np.float32)
    if mass.shape != (n,):
        raise ValueError(f"pos and mass must have the same length: mass has shape {mass.shape}, not ({n},)")
    return mass


def check_group(group, n):
    """(int32 (n,) labels, n_groups) of a FofCatalogue or an integer label array (N >= 1: halo N; 0 or less: no halo).  n_groups
    is the catalogue's length, or the largest label.  Raises ValueError, also for a catalogue without a halo."""
    if hasattr(group, "group") and hasattr(group, "sizes"):
        labels, n_groups = np.asarray(group.group), len(group)
    else:
        labels, n_groups = np.asarray(group), None
    if labels.dtype == bool or not np.issubdtype(labels.dtype, np.integer):
        raise ValueError(f"halo labels must be an integer array or a FofCatalogue, not dtype {labels.dtype}")
    if labels.shape != (n,):
        raise ValueError(f"halo labels must have shape ({n},), not {labels.shape}")
    if labels.size and (labels.max() > np.iinfo(np.int32).max or labels.min() < np.iinfo(np.int32).min):
        raise ValueError("halo labels must fit 32 bits")
    if n_groups is None:
        n_groups = int(labels.max())
    if n_groups < 1:
        raise ValueError("the catalogue has no halo: no label is 1 or more")
    return np.ascontiguousarray(labels, dtype=np.int32), n_groups


def check_vel(vel, n):
    if vel is None:
        return None
    vel = np.asarray(vel, dtype=np.float32)
    if vel.shape != (n, 3):
        raise ValueError(f"vel must have shape ({n}, 3), not {vel.shape}")
    return vel


def check_phi(phi, n):
    if phi is None:
        return None
    phi = np.asarray(phi, dtype=np.float64)
    if phi.shape != (n,):
        raise ValueError(f"phi must have shape ({n},), not {phi.shape}")
    return phi


def check_period(periodicity_scale):
    """0.0 for an open box (None), else the finite side > 0 of the periodic box."""
    if periodicity_scale is None:
        return 0.0
    try:
        p = float(periodicity_scale)
    except (TypeError, ValueError):
        p = np.nan
    if not np.isfinite(p) or p <= 0:
        raise ValueError(f"periodicity_scale must be None or a finite number > 0, not {periodicity_scale!r}")
    return p


def check_tree_above(tree_above):
    """The member count above which a halo's potential comes from the tree: None = config.HALO_TREE_MEMBERS, else an integer
    >= 1."""
    if tree_above is None:
        return int(config.HALO_TREE_MEMBERS)
    if isinstance(tree_above, bool) or not isinstance(tree_above, (int, np.integer)) or tree_above < 1:
        raise ValueError(f"tree_above must be None or an integer >= 1, not {tree_above!r}")
    return int(tree_above)


def warn_extent(max_extent, period):
    if period > 0 and max_extent > period / 4:
        warnings.warn(f"a halo reaches {max_extent:.4g} from its first member along an axis, more than a quarter of the period "
                      f"{period:.4g}: beyond period / 2 the nearest image is no longer the halo's own", RuntimeWarning, stacklevel=3)


def anchor_offsets(pos, members, period):
    """The float64 offsets of pos[members] (ascending indices of valid members) from the first of them, by nearest image in a
    periodic box: the library's rule."""
    p = pos[members].astype(np.float64)
    d = p - p[0]
    if period > 0:
        d -= period * np.rint(d / period)
    return d


def compute_group_potential(ctx, pos, mass, eps, labels, n_groups, period, tree_above, theta):
    """group_potential() on a context, arguments already checked, G = 1: (phi float64 (n,), info).  The haloes the library
    skipped (more than tree_above valid members) are filled from the tree on their members' anchor-relative offsets."""
    phi, info = ctx.group_potential(pos[:, 0], pos[:, 1], pos[:, 2], mass, eps, labels, n_groups, period, tree_above)
    warn_extent(info["max_extent"], period)
    if info["n_skipped_groups"]:
        with np.errstate(invalid="ignore"):
            valid = np.isfinite(pos).all(axis=1) & np.isfinite(mass) & (True if np.ndim(eps) == 0 else np.isfinite(eps))
        member = valid & (labels >= 1)
        counts = np.bincount(labels[member], minlength=n_groups + 1)
        for label in np.flatnonzero(counts > tree_above):
            idx = np.flatnonzero(member & (labels == label))
            e = anchor_offsets(pos, idx, period).astype(np.float32)
            m = mass[idx]
            gravity.check_tree_masses(m)
            pot = ctx.gravity_tree(e[:, 0], e[:, 1], e[:, 2], m, eps if np.ndim(eps) == 0 else eps[idx], theta=theta, want_acc=False)[0]
            phi[idx] = pot
    return phi, info


class HaloProperties:
    """The properties of every halo of a catalogue (topsy_amd.halo_properties), arrays of length n_groups, row N - 1 = halo N:
    .n (members), .mass, .com (H, 3), .v_com (H, 3), .sigma_v, .L (H, 3), .j = L / mass, .S (H, 3, 3) (the second moments about
    the centre of mass), .axis_ratios (H, 2) = (b/a, c/a) from the eigenvalues of S, .r_max, .r_half, .v_max = sqrt(G v2_max),
    .r_vmax, .i_half, .i_vmax; with a potential .e_kin, .e_pot, .virial_ratio = 2 e_kin / |e_pot|, .pot_pos (H, 3), .i_pot, .n_bound,
    .m_bound and .phi, the per-particle potential that was used (else None).  A halo without valid members has n = 0, mass = 0
    and NaN elsewhere.  .raw is the dict the library returned."""

    def __init__(self, raw, G=1.0, phi=None):
        c, p = _native.HALO_COLUMNS, raw["props"]
        self.raw, self.G, self.phi = raw, G, phi
        self.n = raw["count"]
        self.mass = p[:, c["mass"]].copy()
        self.com, self.v_com, self.L = (p[:, c[k]:c[k] + 3].copy() for k in ("com", "v_com", "L"))
        with np.errstate(invalid="ignore", divide="ignore"):
            self.sigma_v = np.sqrt(p[:, c["sigma2"]])
            self.j = self.L / self.mass[:, None]
            self.v_max = np.sqrt(G * p[:, c["v2_max"]])
        s = p[:, c["S"]:c["S"] + 6]
        self.S = s[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)
        self.axis_ratios = np.full((len(p), 2), np.nan)
        ok = np.isfinite(self.S).all(axis=(1, 2))
        if ok.any():
            ev = np.sqrt(np.maximum(np.linalg.eigvalsh(self.S[ok]), 0.0))      # ascending: c, b, a
            with np.errstate(invalid="ignore", divide="ignore"):
                self.axis_ratios[ok] = np.stack([ev[:, 1] / ev[:, 2], ev[:, 0] / ev[:, 2]], axis=1)
        self.r_max, self.r_half, self.r_vmax = (p[:, c[k]].copy() for k in ("r_max", "r_half", "r_vmax"))
        self.i_half, self.i_vmax = (np.where(np.isfinite(p[:, c[k]]), p[:, c[k]], -1).astype(np.int64) for k in ("i_half", "i_vmax"))
        self.e_kin = p[:, c["e_kin"]].copy()
        if phi is None:
            self.e_pot = self.virial_ratio = self.pot_pos = self.i_pot = self.n_bound = self.m_bound = None
        else:
            self.e_pot, self.m_bound = p[:, c["e_pot"]].copy(), p[:, c["m_bound"]].copy()
            self.pot_pos = p[:, c["pot_pos"]:c["pot_pos"] + 3].copy()
            self.i_pot, self.n_bound = raw["i_pot"], raw["n_bound"]
            with np.errstate(invalid="ignore", divide="ignore"):
                self.virial_ratio = 2.0 * self.e_kin / np.abs(self.e_pot)

    def __len__(self):
        return len(self.n)


def compute_halo_properties(ctx, pos, mass, labels, n_groups, vel, eps, phi, period, G, tree_above, theta):
    """halo_properties() on a context: arguments already checked."""
    if phi is None and eps is not None:
        phi = G * compute_group_potential(ctx, pos, mass, eps, labels, n_groups, period, tree_above, theta)[0]
    v = None if vel is None else [np.ascontiguousarray(vel[:, k]) for k in range(3)]
    raw = ctx.halo_properties(pos[:, 0], pos[:, 1], pos[:, 2], mass, labels, n_groups, vel=v, phi=phi, period=period)
    warn_extent(raw["max_extent"], period)
    return HaloProperties(raw, G, phi)
