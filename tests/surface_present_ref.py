"""Numpy restatement of the composed surface frame (test infrastructure): tsp_present_surface in the float32 operation order of
include/topsy_splat.h "tsp_present_surface" -- the bilateral filter of surface_ref, the base layer's sampling rule of present_ref
on both channels of the filtered image at five points per canvas pixel, the shading arithmetic of surface_ref.shade with the
canvas's texel size, then the layers of present_ref.  Reference lines followed (paths relative to the reference checkout):
  surface map as a canvas pass ... src/topsy/visualizer.py:367-384,396; src/topsy/colormap/surface.py:357-365 (texelSize = 1 / canvas)
  shading ........................ src/topsy/shaders/surface.wgsl:28-123 (:69-100 the aspect squash, as colormap.wgsl)
  colorbar rule .................. src/topsy/visualizer.py:327-328
`params` are the keywords of topsy_amd._native.Context.surface_present; layers the dicts of Context.present."""
import numpy as np

import present_ref
import surface_ref
from oracle import oracle_np

f32 = np.float32
ONE, HALF = present_ref.ONE, present_ref.HALF


def canvas_coordinates(R, W, H):
    """(ax (W,), ay (H,), linear): the texel-space coordinates of the pixel centres, and whether the filter is linear (k <= 1)."""
    S = max(W, H)
    k = f32(R) / f32(S)
    ox, oy = HALF * f32(W - S), HALF * f32(H - S)
    xc, yc = present_ref.pixel_centres(W, H)
    return ((xc - ox) * k).astype(f32), ((yc - oy) * k).astype(f32), bool(k <= ONE)


def sample(F, x, y, linear):
    """Both channels of F at the texel-space coordinates x (W,), y (H,) by the base layer's rule -> (H, W, 2)."""
    R = F.shape[0]
    if linear:
        X, Y = np.meshgrid(x, y)
        return present_ref._bilinear(F, X, Y)
    i = np.clip(np.floor(x).astype(np.int64), 0, R - 1)
    j = np.clip(np.floor(y).astype(np.int64), 0, R - 1)
    return F[j[:, None], i[None, :]]


def normals(F, W, H, depth_scale=1.0):
    """(nx, ny, nz, Dc, q) of every canvas pixel: the normalised normal, the scaled centre depth and the sampled quantity."""
    F = np.asarray(F, dtype=f32)
    R = F.shape[0]
    ax, ay, linear = canvas_coordinates(R, W, H)
    du, dv = f32(R) / f32(W), f32(R) / f32(H)
    ds = f32(depth_scale)
    with np.errstate(all="ignore"):
        c = sample(F, ax, ay, linear)
        Dc = c[..., 1] * ds
        Dl = sample(F, (ax - du).astype(f32), ay, linear)[..., 1] * ds
        Dr = sample(F, (ax + du).astype(f32), ay, linear)[..., 1] * ds
        Du = sample(F, ax, (ay - dv).astype(f32), linear)[..., 1] * ds
        Dd = sample(F, ax, (ay + dv).astype(f32), linear)[..., 1] * ds
        nx0 = -((Dr - Dl) * HALF)
        ny0 = -((Dd - Du) * HALF)
        nz0 = ONE / f32(W)
        ln = np.sqrt((nx0 * nx0 + ny0 * ny0) + nz0 * nz0)
        return nx0 / ln, ny0 / ln, nz0 / ln, Dc, c[..., 0]


def shade_canvas(F, W, H, depth_scale=1.0, light_direction=surface_ref.DEFAULT_PARAMS["light_direction"],
                 light_color=(1.0, 1.0, 1.0), ambient_color=(0.0, 0.0, 0.2), weighted_average=False, log=False, vmin=0.0, vmax=1.0,
                 lut=None):
    """(H, W, 4) uint8: the lit surface of the filtered image F on the canvas (surface_ref.shade's arithmetic after the normal)."""
    L = [f32(v) for v in light_direction]
    lc = [f32(v) for v in light_color]
    amb = [f32(v) for v in ambient_color]
    nx, ny, nz, D, v = normals(F, W, H, depth_scale)
    with np.errstate(all="ignore"):
        ndl = (nx * L[0] + ny * L[1]) + nz * L[2]
        ndl = np.where(ndl > 0, ndl, f32(0.0)).astype(f32)
        if weighted_average:
            if log:
                v = oracle_np.canon_log10f(v)
            t = (v - f32(vmin)) / (f32(vmax) - f32(vmin))
            t = np.where(np.isnan(t), f32(0.0), np.clip(t, f32(0.0), f32(1.0))).astype(f32)
            mat = oracle_np._lut_sample(np.asarray(lut, dtype=f32), t)[..., :3]
        else:
            mat = np.ones((H, W, 3), dtype=f32)
        k = np.where(D < 0, f32(0.0), np.where(D > f32(0.5), f32(0.5), D)).astype(f32) * f32(2.0)
        rgba = np.ones((H, W, 4), dtype=f32)
        for c in range(3):
            rgba[..., c] = (((lc[c] * ndl) * mat[..., c]) + amb[c] * mat[..., c]) * k
    return oracle_np._unorm8(rgba)


def draw_layers(frame, layers):
    """The layers of present_ref.compose over an (H, W, 4) uint8 frame, in place."""
    H, W = frame.shape[:2]
    xc, yc = present_ref.pixel_centres(W, H)
    for layer in layers:
        if layer["kind"] == "quad":
            tex = np.asarray(layer["texture"], dtype=f32)
            th, tw = tex.shape[:2]
            for X0, X1, Y0, Y1, u0, du, v0, dv, wt in present_ref.quad_primitives(layer, W, H):
                cols = np.where((X0 <= xc) & (xc < X1))[0]
                rows = np.where((Y0 <= yc) & (yc < Y1))[0]
                if not len(cols) or not len(rows):
                    continue
                u = (u0 + ((xc[cols] - X0) / (X1 - X0)) * du).astype(f32)
                v = (v0 + ((yc[rows] - Y0) / (Y1 - Y0)) * dv).astype(f32)
                U, V = np.meshgrid((u * f32(tw)).astype(f32), (v * f32(th)).astype(f32))
                src = (present_ref._bilinear(tex, U, V) * wt).astype(f32)
                present_ref._blend(frame, rows, cols, src, np.ones(U.shape, dtype=bool), False)
        else:
            color = np.asarray(layer["color"], dtype=f32)
            for prim in present_ref.line_primitives(layer, W, H):
                if prim is None:
                    continue
                rows, cols, mask = present_ref.line_coverage(prim, W, H)
                if mask.any():
                    present_ref._blend(frame, rows, cols, np.broadcast_to(color, mask.shape + (4,)), mask, False)
    return frame


def compose_surface(raw, W, H, params, layers=()):
    """tsp_present_surface in numpy: (H, W, 4) uint8 of the raw (q, depth) image `raw`.  A key `params` lacks takes the value of
    surface_ref.DEFAULT_PARAMS (the device call has defaults of its own: give both the same dict)."""
    p = dict(surface_ref.DEFAULT_PARAMS) | dict(params)
    F = surface_ref.bilateral(raw, p.pop("smoothing_scale"))
    lut = p.pop("lut_rgba", None)
    return draw_layers(shade_canvas(F, W, H, lut=lut, **p), layers)
