"""The contract of tsp_sph_velocity_gradient (include/topsy_splat.h) restated in numpy, and the bound the GPU is held to.

brute_force_velocity_gradient is to tsp_sph_velocity_gradient what brute_force_sph_sum (test_density_cpu.py) is to tsp_sph_sum:
every float32 operation in the contract's order, the four row sums in float64.  Next to each value it returns what the bound needs:
A, the float64 sum of |term| over |den|, and T, the number of terms."""
import numpy as np

OUTPUTS = ("div", "curl_x", "curl_y", "curl_z")


def brute_force_velocity_gradient(pos, h, mass, rho, vel, period=0.0, order="pairwise", queries=None, block=256):
    """For every answerable query i (finite coordinates, h[i] finite and > 0), over every j with finite coordinates:
    dx = x[j] - x[i] (nearest image in a periodic box), d2 = (dx dx + dy dy) + dz dz, u = sqrtf(d2) / h[i]; the term exists iff
    d2 > 0 and u < 2; t = 2 - u, f = 3 - 2.25 u below 1 and (0.75 (t t)) / u above, c = mass[j] f, dv = v[j] - v[i],
    term_div = c ((dvx dx + dvy dy) + dvz dz), term_cx = c (dy dvz - dz dvy), term_cy = c (dz dvx - dx dvz),
    term_cz = c (dx dvy - dy dvx); out = (float)(S / (pi (((hd hd) (hd hd)) hd) (double)rho[i])), hd = (double)h[i].
    order: how the float64 row sums run ("pairwise": numpy's own; "forward" / "backward": one term after the other).
    queries: only these indices are evaluated (the others stay NaN, with A = NaN and T = 0).
    Returns (value, A, T): float32 (n, 4) in the order of OUTPUTS, float64 (n, 4), int64 (n,)."""
    pos = np.asarray(pos, dtype=np.float32)
    h = np.asarray(h, dtype=np.float32)
    mass = np.asarray(mass, dtype=np.float32)
    rho = np.asarray(rho, dtype=np.float32)
    vel = np.asarray(vel, dtype=np.float32)
    n = len(pos)
    assert pos.shape == (n, 3) and vel.shape == (n, 3) and h.shape == mass.shape == rho.shape == (n,)
    valid = np.isfinite(pos).all(axis=1)
    P, M, V = pos[valid], mass[valid], vel[valid]
    L = np.float32(period)
    one, two = np.float32(1.0), np.float32(2.0)
    value = np.full((n, 4), np.nan, dtype=np.float32)
    A = np.full((n, 4), np.nan, dtype=np.float64)
    T = np.zeros(n, dtype=np.int64)
    with np.errstate(all="ignore"):
        answerable = valid & np.isfinite(h) & (h > 0)
    if queries is not None:
        chosen = np.zeros(n, dtype=bool)
        chosen[np.asarray(queries)] = True
        answerable &= chosen
    todo = np.flatnonzero(answerable)
    with np.errstate(all="ignore"):
        for b in range(0, len(todo), block):
            idx = todo[b:b + block]
            q, hq, vq = pos[idx], h[idx], vel[idx]
            d = []
            for ax in range(3):
                dx = P[None, :, ax] - q[:, None, ax]
                if period:
                    t = dx / L
                    t = np.rint(t)
                    dx = dx - L * t
                d.append(dx)
            dx, dy, dz = d
            d2 = (dx * dx + dy * dy) + dz * dz
            u = np.sqrt(d2) / hq[:, None]
            inside = (d2 > 0) & (u < two)
            # the rest on the pairs that have a term only (the same float32 operations, element by element)
            rows, cols = np.nonzero(inside)
            dx, dy, dz, u = dx[rows, cols], dy[rows, cols], dz[rows, cols], u[rows, cols]
            t = two - u
            f = np.where(u < one, np.float32(3.0) - np.float32(2.25) * u, (np.float32(0.75) * (t * t)) / u)
            c = M[cols] * f
            dvx, dvy, dvz = (V[cols, ax] - vq[rows, ax] for ax in range(3))
            terms = (c * ((dvx * dx + dvy * dy) + dvz * dz), c * (dy * dvz - dz * dvy), c * (dz * dvx - dx * dvz),
                     c * (dx * dvy - dy * dvx))
            hd = hq.astype(np.float64)
            den = np.pi * (((hd * hd) * (hd * hd)) * hd) * rho[idx].astype(np.float64)
            count = inside.sum(axis=1)
            T[idx] = count
            # each query's terms side by side, in the order of j, padded with zeros (adding 0.0 changes no float64 sum)
            rank = np.arange(len(rows)) - np.repeat(np.cumsum(count) - count, count)
            for k, term in enumerate(terms):
                assert term.dtype == np.float32
                term64 = np.zeros((len(idx), max(int(count.max()), 1)), dtype=np.float64)
                term64[rows, rank] = term.astype(np.float64)
                if order == "pairwise":
                    S = term64.sum(axis=1)
                elif order == "forward":
                    S = np.cumsum(term64, axis=1)[:, -1]
                else:
                    S = np.cumsum(term64[:, ::-1], axis=1)[:, -1]
                value[idx, k] = (S / den).astype(np.float32)
                A[idx, k] = np.abs(term64).sum(axis=1) / np.abs(den)
    return value, A, T


def within_bound(got, want, A, T):
    """Per element: |got - want| <= spacing(|want|) + 2 T 2^-53 A.  Two float64 summations of the same T terms each err by at most
    (T - 1) 2^-53 sum |term|, so S / den differs by at most 2 T 2^-53 A between them; the two roundings to float32 then differ by
    at most one float32 ulp on top.  Equal bits (NaN and infinities included) always pass; a non-finite value passes only so."""
    got = np.asarray(got, dtype=np.float32)
    want = np.asarray(want, dtype=np.float32)
    T = np.asarray(T, dtype=np.float64)
    if got.ndim == 2 and T.ndim == 1:
        T = T[:, None]
    with np.errstate(all="ignore"):
        same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want)) | (got == want)
        both = np.isfinite(got) & np.isfinite(want)
        bound = np.spacing(np.abs(want)).astype(np.float64) + 2.0 * T * 2.0 ** -53 * np.asarray(A, dtype=np.float64)
        near = both & (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= bound)
    return same | near


def velocity_field(pos, seed, shear=0.7, omega=(0.3, -0.5, 0.8), noise=1.0, offset=(0.0, 0.0, 0.0)):
    """v = shear r + Omega x r + offset + unit normal noise, float32 (non-finite positions give non-finite velocities: replaced by 0,
    since the velocity of an invalid particle is never used)."""
    p = np.asarray(pos, dtype=np.float64)
    v = shear * p + np.cross(np.asarray(omega, dtype=np.float64), p) + np.asarray(offset, dtype=np.float64)
    v = v + noise * np.random.RandomState(seed).normal(size=p.shape)
    v[~np.isfinite(v)] = 0.0
    return v.astype(np.float32)
