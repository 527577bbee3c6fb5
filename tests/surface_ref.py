"""Numpy restatement of surface rendering (test infrastructure): the occlusion pass, the density cut, the bilateral filter and the
lit shading, in the float32 operation order of include/topsy_splat.h "Surface rendering".  Reference lines followed (paths
relative to the reference checkout):
  sphere texture ......... src/topsy/sph.py:448-456 (LocalSphereKernel), :497-501 (normalisation 1), :396-426 (mips)
  density cut ............ src/topsy/sph.py:480-515 (np.quantile over 101 samples, index int(p / 100 * 100))
  occlusion pass ......... src/topsy/shaders/sph.wgsl:94-122 (vertex_depth_with_cut), :149-158 (fragment_raw);
                           src/topsy/sph.py:599-646 (depth32float cleared to 0, depth_compare greater)
  bilateral filter ....... src/topsy/shaders/smooth.wgsl:12-48; src/topsy/colormap/surface.py:259-287
  shading ................ src/topsy/shaders/surface.wgsl:28-123; src/topsy/colormap/surface.py:12-24 (defaults)
  autorange .............. src/topsy/colormap/surface.py:250-253; src/topsy/colormap/implementation.py:390-425
"""
import numpy as np

from oracle import oracle_np

f32 = np.float32
MAX_SURFACE_SMOOTH_PIXELS = 100           # reference config.py:44

DEFAULT_PARAMS = {
    "depth_scale": 1.0,
    "light_direction": [0.0, 1.0 / np.sqrt(2.0), 1.0 / np.sqrt(2.0)],
    "light_color": [1.0, 1.0, 1.0],
    "ambient_color": [0.0, 0.0, 0.2],
    "smoothing_scale": 0.01,
}


def sphere_mips():
    """sqrt(4 - d^2) for d < 2 else -0.01 at texel centres, per Python float as LocalSphereKernel.get_value, float32 per level."""
    levels = []
    for n in oracle_np.MIP_SIZES:
        c = np.linspace(-2 + 2.0 / n, 2 - 2.0 / n, n)
        x, y = np.meshgrid(c, c)
        d = np.sqrt(x ** 2 + y ** 2)
        im = np.array([np.sqrt(4.0 - v ** 2) if v < 2.0 else -0.01 for v in d.flatten()]).reshape(n, n)
        levels.append((im * 1.0).astype(f32).ravel())
    return np.concatenate(levels)


def density_cuts(mass, smooth):
    """The reference's _percentile_to_den_cut over float32 m, h."""
    h = np.asarray(smooth, dtype=f32)
    with np.errstate(all="ignore"):
        rho = np.asarray(mass, dtype=f32) / ((h * h) * h)
        return np.quantile(rho, np.linspace(0, 1, 101))


def cut_for_percentile(cuts, percentile):
    return f32(cuts[int(percentile / 100.0 * (101 - 1))])


def occlusion(pos_smooth, mass, qty, M, sf, R, cut, smips=None):
    """Returns (img (R, R, 2) float32 = (q, unclamped depth) of the winner or (0, 0), winner index (R, R) int64 or -1).
    Particles are drawn in index order with a strict greater test on dc = min(depth, 1) against a target cleared to 0."""
    if smips is None:
        smips = sphere_mips()
    pos_smooth = np.asarray(pos_smooth, dtype=f32)
    with np.errstate(all="ignore"):
        pcx, pcy, cz, P, half, invP, keep = oracle_np._project(pos_smooth, M, sf, R)
        h = pos_smooth[:, 3]
        rho = np.asarray(mass, dtype=f32) / ((h * h) * h)
        zs = (h * f32(sf)) * f32(0.5)
    drawn = keep & (rho > f32(cut))
    best = np.zeros((R, R), dtype=f32)
    depth_img = np.zeros((R, R), dtype=f32)
    winner = np.full((R, R), -1, dtype=np.int64)
    for p in np.flatnonzero(drawn):
        fp = oracle_np._footprint(pcx[p], pcy[p], half[p], invP[p], P[p], R, smips)
        if fp is None:
            continue
        j0, i0, K, _ = fp
        depth = cz[p] + zs[p] * K
        dc = np.where(depth < f32(1.0), depth, f32(1.0))
        blk = np.s_[j0:j0 + K.shape[0], i0:i0 + K.shape[1]]
        upd = (K >= 0) & (dc > 0) & (dc > best[blk])
        best[blk][upd] = dc[upd]
        depth_img[blk][upd] = depth[upd]
        winner[blk][upd] = p
    img = np.zeros((R, R, 2), dtype=f32)
    q = np.zeros(len(pos_smooth), dtype=f32) if qty is None else np.asarray(qty, dtype=f32)
    won = winner >= 0
    img[..., 0][won] = q[winner[won]]
    img[..., 1] = depth_img
    return img, winner


def filter_parameters(smoothing_scale, R):
    sig = smoothing_scale
    if sig < 1e-5:
        sig = 1e-5
    ss = f32(sig * R)
    rs = f32(sig * 2)
    n_pix = int(ss * f32(4)) + 1
    return ss, rs, min(n_pix, MAX_SURFACE_SMOOTH_PIXELS)


def bilateral(img, smoothing_scale):
    """(q, sum / wsum) per pixel; dy outer, dx inner, coordinates clamped to the image."""
    img = np.asarray(img, dtype=f32)
    R = img.shape[0]
    ss, rs, n = filter_parameters(smoothing_scale, R)
    half = n // 2
    d = img[..., 1]
    pad = np.pad(d, half, mode="edge")
    s2 = (f32(2.0) * ss) * ss
    r2 = (f32(2.0) * rs) * rs
    acc = np.zeros_like(d)
    wsum = np.zeros_like(d)
    with np.errstate(all="ignore"):
        for dy in range(-half, half + 1):
            for dx in range(-half, half + 1):
                ds = np.sqrt(f32(dx * dx + dy * dy))
                ws = oracle_np.canon_expf(-(ds * ds) / s2)
                s = pad[half + dy:half + dy + R, half + dx:half + dx + R]
                dd = np.abs(s - d)
                wr = oracle_np.canon_expf(-(dd * dd) / r2)
                w = ws * wr
                acc = acc + s * w
                wsum = wsum + w
        out = np.empty_like(img)
        out[..., 0] = img[..., 0]
        out[..., 1] = acc / wsum
    return out


def shade(F, depth_scale=1.0, light_direction=DEFAULT_PARAMS["light_direction"], light_color=(1.0, 1.0, 1.0),
          ambient_color=(0.0, 0.0, 0.2), weighted_average=False, log=False, vmin=0.0, vmax=1.0, lut=None):
    """(R, R, 4) uint8 lit surface of the filtered image F."""
    F = np.asarray(F, dtype=f32)
    R = F.shape[0]
    L = [f32(v) for v in light_direction]
    lc = [f32(v) for v in light_color]
    amb = [f32(v) for v in ambient_color]
    with np.errstate(all="ignore"):
        D = F[..., 1] * f32(depth_scale)
        P = np.pad(D, 1, mode="edge")
        Dl, Dr = P[1:-1, :-2], P[1:-1, 2:]
        Du, Dd = P[:-2, 1:-1], P[2:, 1:-1]
        nx0 = -((Dr - Dl) * f32(0.5))
        ny0 = -((Dd - Du) * f32(0.5))
        nz0 = f32(1.0) / f32(R)
        ln = np.sqrt((nx0 * nx0 + ny0 * ny0) + nz0 * nz0)
        nx, ny, nz = nx0 / ln, ny0 / ln, nz0 / ln
        ndl = (nx * L[0] + ny * L[1]) + nz * L[2]
        ndl = np.where(ndl > 0, ndl, f32(0.0)).astype(f32)
        if weighted_average:
            v = F[..., 0]
            if log:
                v = oracle_np.canon_log10f(v)
            t = (v - f32(vmin)) / (f32(vmax) - f32(vmin))
            t = np.where(np.isnan(t), f32(0.0), np.clip(t, f32(0.0), f32(1.0))).astype(f32)
            mat = oracle_np._lut_sample(np.asarray(lut, dtype=f32), t)[..., :3]
        else:
            mat = np.ones((R, R, 3), dtype=f32)
        k = np.where(D < 0, f32(0.0), np.where(D > f32(0.5), f32(0.5), D)).astype(f32) * f32(2.0)
        rgba = np.ones((R, R, 4), dtype=f32)
        for c in range(3):
            rgba[..., c] = (((lc[c] * ndl) * mat[..., c]) + amb[c] * mat[..., c]) * k
    return oracle_np._unorm8(rgba)


def autorange_values(raw):
    """The values the surface map autoranges over: the raw quantity where a sphere was drawn."""
    valid = raw[..., 1].ravel() > 0.0
    return raw[..., 0].ravel()[valid]


def autorange(raw, percentiles=(1.0, 99.9)):
    """(vmin, vmax, log) of Colormap._autorange_using_values over autorange_values(raw)."""
    vals = autorange_values(raw)
    use_log = not (vals < 0).any()
    with np.errstate(all="ignore"):
        sample = np.log10(vals) if use_log else vals
    sample = sample[np.isfinite(sample)]
    if len(sample) > 200:
        vmin, vmax = np.percentile(sample, list(percentiles))
    elif len(sample) > 2:
        vmin, vmax = np.min(sample), np.max(sample)
    else:
        vmin, vmax = 0.0, 1.0
    return vmin, vmax, use_log
