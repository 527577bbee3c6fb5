"""numpy restatement of tsp_present_yuv420's conversion (include/topsy_splat.h): an RGB(A) uint8 frame to I420 planes.

Integer arithmetic only; numpy's `>>` on signed integers is an arithmetic shift (floor), as the header specifies."""
import numpy as np


def luma(rgb):
    """Y of every pixel of an (..., >= 3) uint8 array."""
    c = np.asarray(rgb)[..., :3].astype(np.int64)
    return (((47 * c[..., 0] + 157 * c[..., 1] + 16 * c[..., 2] + 128) >> 8) + 16).astype(np.uint8)


def chroma_of_means(r, g, b):
    """(U, V) of the rounded 2 x 2 means r, g, b."""
    r, g, b = (np.asarray(v, dtype=np.int64) for v in (r, g, b))
    u = ((-26 * r - 86 * g + 112 * b + 128) >> 8) + 128
    v = ((112 * r - 102 * g - 10 * b + 128) >> 8) + 128
    return u.astype(np.uint8), v.astype(np.uint8)


def to_yuv420(rgb):
    """(Y, U, V) of an (H, W, >= 3) uint8 frame with even H and W; alpha, if present, is ignored."""
    rgb = np.asarray(rgb)
    H, W = rgb.shape[:2]
    assert rgb.dtype == np.uint8 and H % 2 == 0 and W % 2 == 0, (rgb.dtype, rgb.shape)
    c = rgb[..., :3].astype(np.int64)
    s = c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
    m = (s + 2) >> 2
    u, v = chroma_of_means(m[..., 0], m[..., 1], m[..., 2])
    return luma(rgb), u, v


def pixel(r, g, b):
    """(Y, U, V) of a frame whose pixels all have the colour (r, g, b)."""
    y, u, v = to_yuv420(np.array([[[r, g, b]] * 2] * 2, dtype=np.uint8))
    return int(y[0, 0]), int(u[0, 0]), int(v[0, 0])
