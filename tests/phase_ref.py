"""The float64 model of tsp_histogram_2d (include/topsy_splat.h "Weighted 2-D histograms"), NumPy only: half-open bins found by
np.searchsorted on the edges as passed, validity as the contract states it, np.add.at into float64 planes.  It imports neither the
product nor the reference."""
import numpy as np

f32 = np.float32


def bin_of(edges, a):
    """the bin of every float32 a, widened to float64, among the ascending edges: edges[k] <= a < edges[k + 1]; -1 for none"""
    edges = np.asarray(edges, dtype=np.float64)
    a64 = np.asarray(a, dtype=f32).astype(np.float64)
    k = np.searchsorted(edges, a64, side="right") - 1
    k[(k < 0) | (k >= len(edges) - 1) | ~np.isfinite(a64)] = -1
    return k


def histogram(x, y, w, v, edges_x, edges_y):
    """dict: count (ny, nx) int64; sums (1 or 3, ny, nx) float64 -- sum w, sum w v, sum (w v) v in particle order; magnitude, the
    same planes of sum |term| (what the tolerance is made of); bin_index (n,) int32; n_valid, n_binned."""
    x, y = np.asarray(x, dtype=f32), np.asarray(y, dtype=f32)
    n = len(x)
    nx, ny = len(edges_x) - 1, len(edges_y) - 1
    valid = np.isfinite(x) & np.isfinite(y)
    w64 = np.ones(n) if w is None else np.asarray(w, dtype=f32).astype(np.float64)
    valid &= np.isfinite(w64)
    v64 = None
    if v is not None:
        v64 = np.asarray(v, dtype=f32).astype(np.float64)
        valid &= np.isfinite(v64)
    i, j = bin_of(edges_x, x), bin_of(edges_y, y)
    member = valid & (i >= 0) & (j >= 0)
    cell = np.where(member, j * nx + i, -1)
    c = cell[member]
    count = np.zeros(nx * ny, dtype=np.int64)
    np.add.at(count, c, 1)
    terms = [w64[member]]
    if v64 is not None:
        wv = w64[member] * v64[member]
        terms += [wv, wv * v64[member]]
    sums = np.zeros((len(terms), nx * ny))
    magnitude = np.zeros_like(sums)
    for k, t in enumerate(terms):
        np.add.at(sums[k], c, t)
        np.add.at(magnitude[k], c, np.abs(t))
    return {"count": count.reshape(ny, nx), "sums": sums.reshape(-1, ny, nx), "magnitude": magnitude.reshape(-1, ny, nx),
            "bin_index": cell.astype(np.int32), "n_valid": int(valid.sum()), "n_binned": int(member.sum())}


def tolerance(model):
    """per cell and plane m * 2^-52 * sum |term|: w and w v are exact in float64 and (w v) v rounds once (2^-53 of the term), and
    m - 1 additions in any order each round by at most 2^-53 of a partial sum that never exceeds sum |term| (1 + m 2^-53)"""
    return model["count"][None].astype(np.float64) * 2.0 ** -52 * model["magnitude"]
