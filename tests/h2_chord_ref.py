"""Kernel H2's strip test and row clip restated in NumPy float32 (tsp_pipeline.h: reaches_strip, chord_limit, row_outside_chord), and the
footprints the two chord tests pin.  Every operation is the kernel's, in its order, on float32 values."""
import numpy as np

f32 = np.float32
DISC_K2 = f32(0.5235) * f32(0.5235)
SW = 64                                  # strip width of every density / multi-channel build (W = 1)


def strip_dist(c, s0, s1):
    return np.maximum(np.maximum(f32(s0) - c, c - f32(s1)), f32(0.0))


def reaches_strip(pcx, pcy, P, sx0, sy0, sh, k2=DISC_K2):
    half = f32(0.5) * P
    sdx, sdy = strip_dist(pcx, sx0, sx0 + SW), strip_dist(pcy, sy0, sy0 + sh)
    return bool(P > 0 and sdx < half and sdy < half and not (k2 > 0 and sdx * sdx + sdy * sdy >= k2 * P * P))


def strip_rows(pcx, pcy, P, sx0, sy0, sh, k2=DISC_K2):
    """(covered, cleared) per pixel row of the strip at (sx0, sy0), sh rows high: the rows of the footprint's square, and those of
    them the row clip takes out"""
    half = f32(0.5) * P
    sdx = strip_dist(pcx, sx0, sx0 + SW)
    limit = k2 * P * P - sdx * sdx if k2 > 0 else f32(np.inf)
    d = (np.arange(sy0, sy0 + sh, dtype=f32) + f32(0.5)) - pcy
    covered = np.abs(d) < half
    return covered, covered & (d * d >= limit)


def texel_pairs(c, pc, P):
    """What a pixel centre coordinate c reads along one axis, as the kernel forms it (the clamped canonical coordinate): the two level-0
    texel indices, the weight of the second (the first has one minus it), and whether the square covers c.  At the low edge the clamp
    gives index 0 with fraction 0: the second texel, index 1, is read with an exactly zero weight."""
    half, invP = f32(0.5) * P, f32(1.0) / P
    d = c - pc
    t = np.clip((d + half) * invP * f32(64.0) - f32(0.5), f32(0.0), f32(63.0))
    i0 = t.astype(np.int32)
    return i0, np.minimum(i0 + 1, 63), t - i0.astype(f32), np.abs(d) < half


def centre_to_world(R, px, py):
    """world (x, y) of the particle whose footprint centre falls on pixel coordinates (px, py) under the test view (scale R / 2)"""
    return px - R / 2.0, R / 2.0 - py


# ---- scene (c): the clip empties a hit's rows in a strip that reaches_strip keeps -----------------------------------------
# reaches_strip measures to the strip rectangle, the row test to the row centres half a pixel inside it.  P = 300: the disc's radius is
# 0.5235 P = 157.05 px.  A centre 111 px right of and 110.9 px below the strip corner (64, 32) -- a corner of the 64 x 32 and of the
# 64 x 16 strips alike -- is 156.91 px from the corner (the strip is kept) and >= 157.26 px from every row centre of the strip
# (sqrt(111^2 + 111.4^2)): all its rows are cleared.  The second record is the mirror case at the corner (192, 224).
EMPTIED_P = 300.0
EMPTIED = [
    # (centre x, centre y, strip x0, strip y0 for 32-row strips, strip y0 for 16-row strips)
    (64.0 + 111.0, 32.0 + 110.9, 0, 0, 16),
    (192.0 - 111.0, 224.0 - 110.9, 192, 224, 224),
]
