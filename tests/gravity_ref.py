"""The float64 model of tsp_gravity_direct (include/topsy_splat.h): the formulae evaluated in float64 on the float32 inputs,
with the header's rules for which sources, pairs and targets count.  It returns, beside the sums, the per-component scales
sum_j |term_ij| that the error bound of the header is stated in."""
import numpy as np

U = 2.0 ** -24


def as_f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def direct_sum(src, mass, eps, targets=None, block=256):
    """src (n, 3), mass (n,), eps a scalar or (n,), targets (k, 3) or None (the targets are the sources; the pair i == j by index
    is left out).  Returns a dict: pot (k,), acc (k, 3), pot_scale (k,), acc_scale (k, 3) float64 (NaN, NaN, 0, 0 at a target with
    a non-finite coordinate), n_valid_sources, n_valid_targets."""
    src = as_f32(src)
    mass = as_f32(mass)
    n = len(src)
    e = np.full(n, np.float32(eps), dtype=np.float32) if np.ndim(eps) == 0 else as_f32(eps)
    assert src.shape == (n, 3) and mass.shape == (n,) and e.shape == (n,)
    self_targets = targets is None
    tgt = src if self_targets else as_f32(targets)
    k = len(tgt)
    valid_src = np.isfinite(src).all(axis=1) & np.isfinite(mass) & np.isfinite(e)
    valid_tgt = np.isfinite(tgt).all(axis=1)
    idx = np.nonzero(valid_src)[0]
    s = src[idx].astype(np.float64)
    m = mass[idx].astype(np.float64)
    e2 = e[idx].astype(np.float64) ** 2
    pot = np.full(k, np.nan)
    acc = np.full((k, 3), np.nan)
    pot_scale = np.zeros(k)
    acc_scale = np.zeros((k, 3))
    for lo in range(0, k, block):
        rows = np.arange(lo, min(lo + block, k))
        rows = rows[valid_tgt[rows]]
        if not len(rows):
            continue
        t = tgt[rows].astype(np.float64)
        d = t[:, None, :] - s[None, :, :]
        r2 = (d * d).sum(axis=2) + e2[None, :]
        counts = r2 > 0.0
        if self_targets:
            counts &= rows[:, None] != idx[None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = np.where(counts, 1.0 / np.sqrt(np.where(counts, r2, 1.0)), 0.0)
        p = m[None, :] * inv
        w = (p * inv * inv)[:, :, None] * d
        pot[rows] = -p.sum(axis=1)
        acc[rows] = -w.sum(axis=1)
        pot_scale[rows] = np.abs(p).sum(axis=1)
        acc_scale[rows] = np.abs(w).sum(axis=1)
    return {"pot": pot, "acc": acc, "pot_scale": pot_scale, "acc_scale": acc_scale,
            "n_valid_sources": int(valid_src.sum()), "n_valid_targets": int(valid_tgt.sum())}


def worst_ratio(got_pot, got_acc, ref):
    """max over the valid targets and the components of |got - want| / (2^-24 * scale): what the header bounds by K.  A component
    whose scale is 0 must be exactly 0 (ratio inf otherwise); the NaN pattern of the invalid targets must agree."""
    worst = 0.0
    for got, want, scale in ((got_pot, ref["pot"], ref["pot_scale"]), (got_acc, ref["acc"], ref["acc_scale"])):
        if got is None:
            continue
        got = np.asarray(got, dtype=np.float64)
        assert got.shape == want.shape, (got.shape, want.shape)
        assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN where the model has none, or none where it has"
        ok = ~np.isnan(want)
        delta = np.abs(got[ok] - want[ok])
        sc = scale[ok] * U
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(delta == 0.0, 0.0, delta / sc)
        if ratio.size:
            worst = max(worst, float(ratio.max()))
    return worst
