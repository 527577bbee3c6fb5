"""The contract of tsp_sph_sample_lattice (include/topsy_splat.h) restated as a numpy brute force: what test_lattice_cpu.py pins and
test_gpu_lattice.py holds the GPU to.  The distances and the terms are those of brute_force_smoothing (test_smoothing_cpu.py) and
brute_force_sph_sum (test_density_cpu.py) -- float32, the same operations in the same order, a float64 row sum -- but the queries
are the points of a lattice, which are no particles, and the smoothing length is taken at the point."""
import numpy as np

f32 = np.float32
BRICK = 64      # lattice points per brick: the queries of one wave


def brick_shape(shape):
    """The brick (bu, bv, bw) by which the library (sph_sample_lattice(), tsp_smooth.hip) orders the points of a lattice of
    shape = (nu, nv, nw): 64 x 1 x 1 for a ray (nv == nw == 1), 8 x 8 x 1 for a slice (nw == 1), else 4 x 4 x 4."""
    nu, nv, nw = shape
    if nv == 1 and nw == 1:
        return 64, 1, 1
    return (8, 8, 1) if nw == 1 else (4, 4, 4)


def brick_order(shape):
    """The library's query order (lattice_slot(), tsp_smooth.hip), restated: (slots, 3) int64 lattice indices (i, j, k) per query slot, bricks along u fastest
    and points inside a brick with i fastest, and a bool mask of the slots that lie inside the lattice (a partial brick's other
    slots are masked).  The masked-in slots name every lattice point exactly once."""
    nu, nv, nw = (int(v) for v in shape)
    bu, bv, bw = brick_shape((nu, nv, nw))
    nbu, nbv, nbw = -(-nu // bu), -(-nv // bv), -(-nw // bw)
    slot = np.arange(BRICK * nbu * nbv * nbw, dtype=np.int64)
    brick, within = slot // BRICK, slot % BRICK
    row = brick // nbu
    ijk = np.stack([(brick - row * nbu) * bu + within % bu, (row % nbv) * bv + (within // bu) % bv,
                    (row // nbv) * bw + within // (bu * bv)], axis=1)
    return ijk, (ijk[:, 0] < nu) & (ijk[:, 1] < nv) & (ijk[:, 2] < nw)


def lattice_points(origin, du, dv, dw, shape):
    """(nw, nv, nu, 3) float32: point (i, j, k) is ((origin + i du) + j dv) + k dw in float64, rounded once to float32."""
    nu, nv, nw = (int(v) for v in shape)
    o, du, dv, dw = (np.asarray(v, dtype=np.float64) for v in (origin, du, dv, dw))
    i = np.arange(nu, dtype=np.float64)[None, None, :, None]
    j = np.arange(nv, dtype=np.float64)[None, :, None, None]
    k = np.arange(nw, dtype=np.float64)[:, None, None, None]
    return (((o + i * du) + j * dv) + k * dw).astype(f32)


def sample_points(points, pos, fields, k, period=0.0, block=128):
    """The estimator at arbitrary float32 `points` (m, 3): (h (m,), outs (F, m), A (F, m), T (m,)) with
    h = 0.5f * sqrtf(k-th smallest d2) over the particles with finite coordinates, outs[f] = (float)(S_f / (pi (double)((h h) h)))
    with S_f the float64 sum (numpy's pairwise order) of the float32 terms fields[f][j] * w(u), u = sqrtf(d2) / h < 2; NaN where
    h is 0 or not finite.  A[f] = sum |term| / (pi h^3) in float64 and T = the number of terms, for the bounds of signed fields."""
    points = np.asarray(points, dtype=f32).reshape(-1, 3)
    pos = np.asarray(pos, dtype=f32)
    valid = np.isfinite(pos).all(axis=1)
    P = pos[valid]
    F = [np.asarray(a, dtype=f32)[valid] for a in fields]
    L = f32(period)
    one, two = f32(1.0), f32(2.0)
    m = len(points)
    h = np.empty(m, dtype=f32)
    outs = np.empty((len(F), m), dtype=f32)
    A = np.empty((len(F), m), dtype=np.float64)
    T = np.empty(m, dtype=np.int64)
    with np.errstate(all="ignore"):
        for b in range(0, m, block):
            q = points[b:b + block]
            d = []
            for ax in range(3):
                dx = P[None, :, ax] - q[:, None, ax]
                if period:
                    t = dx / L
                    t = np.rint(t)
                    dx = dx - L * t
                d.append(dx)
            d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            assert d2.dtype == f32
            hq = f32(0.5) * np.sqrt(np.partition(d2, k - 1, axis=1)[:, k - 1])
            h[b:b + block] = hq
            u = np.sqrt(d2) / hq[:, None]
            inside = u < two
            u2 = u * u
            t = two - u
            w = np.where(u < one, (one - f32(1.5) * u2) + f32(0.75) * (u2 * u), f32(0.25) * ((t * t) * t))
            den = np.pi * ((hq * hq) * hq).astype(np.float64)
            answerable = np.isfinite(hq) & (hq > 0)
            T[b:b + block] = np.where(answerable, inside.sum(axis=1), 0)
            for f, a in enumerate(F):
                term = a[None, :] * w
                assert term.dtype == f32
                term64 = np.where(inside, term.astype(np.float64), 0.0)
                outs[f, b:b + block] = np.where(answerable, (term64.sum(axis=1) / den).astype(f32), f32(np.nan))
                A[f, b:b + block] = np.where(answerable, np.abs(term64).sum(axis=1) / den, np.nan)
    return h, outs, A, T


def sample_lattice(pos, fields, k, period, origin, du, dv, dw, shape, with_bound=False):
    """(h (nw, nv, nu), outs (F, nw, nv, nu)) of the lattice; with_bound: also A (F, nw, nv, nu) and T (nw, nv, nu)."""
    nu, nv, nw = (int(v) for v in shape)
    pts = lattice_points(origin, du, dv, dw, shape)
    h, outs, A, T = sample_points(pts.reshape(-1, 3), pos, fields, k, period)
    res = (h.reshape(nw, nv, nu), outs.reshape(-1, nw, nv, nu))
    return res + (A.reshape(-1, nw, nv, nu), T.reshape(nw, nv, nu)) if with_bound else res


class ReferenceContext:
    """Stands in for a _native.Context in tests of the host layer: sph_sample_lattice by the brute force."""

    def sph_sample_lattice(self, x, y, z, fields, k=32, period=None, origin=(0, 0, 0), du=(1, 0, 0), dv=(0, 1, 0), dw=(0, 0, 1),
                           shape=(1, 1, 1)):
        return sample_lattice(np.column_stack([x, y, z]), fields, k, period or 0.0, origin, du, dv, dw, shape)
