"""Float64 model of tsp_spectral_cube (include/topsy_splat.h "Spectral cubes"): k from the oracle's projection and footprint, u from
the kinematic weights' restatement, the channel response from math.erf / math.erfc with NO truncation at 5 s."""
import math

import numpy as np

import kinematics_ref
from oracle import oracle_np

f32 = np.float32
SQRT2 = math.sqrt(2.0)


def edges(v_min, dv, n_channels):
    return float(v_min) + np.arange(n_channels + 1, dtype=np.float64) * float(dv)


def response(u, s, e):
    """g_c of every channel of the edges e (float64, len n + 1) for a line of width s about u: the Gaussian integrated over the
    channel in the cancellation-free form of the header; s == 0: the one channel with e_c <= u < e_{c+1}."""
    n = len(e) - 1
    g = np.zeros(n, dtype=np.float64)
    u, s = float(u), float(s)
    if s == 0.0:
        for c in range(n):
            if e[c] <= u < e[c + 1]:
                g[c] = 1.0
        return g
    for c in range(n):
        a, b = (e[c] - u) / s, (e[c + 1] - u) / s
        if a >= 0.0:
            g[c] = 0.5 * (math.erfc(a / SQRT2) - math.erfc(b / SQRT2))
        elif b <= 0.0:
            g[c] = 0.5 * (math.erfc(-b / SQRT2) - math.erfc(-a / SQRT2))
        else:
            g[c] = 0.5 * (math.erf(b / SQRT2) - math.erf(a / SQRT2))
    return g


def line_widths(n, sigma_v, sigma):
    """(s float64, dead) per particle: s = sqrt(sigma_v^2 + sigma_p^2); dead where sigma_p is not finite or negative"""
    sp = np.zeros(n, dtype=f32) if sigma is None else np.asarray(sigma, dtype=f32)
    dead = ~np.isfinite(sp) | (sp < 0)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.sqrt(float(f32(sigma_v)) ** 2 + sp.astype(np.float64) ** 2)
    return s, dead


def cube(pos, h, m, vel, M, sf, R, axis, v_ref, v_min, dv, n_channels, sigma_v=0.0, sigma=None, mips=None):
    """(cube float64 (n_channels, R, R), S float64 (R, R)): the model, and per pixel the sum over ALL velocities of k w0 of the
    live particles (what the tolerance scales with; the cube's channel sum where the band holds every line)."""
    mips = oracle_np.kernel_mips() if mips is None else mips
    ps = np.column_stack([np.asarray(pos, dtype=f32), np.asarray(h, dtype=f32)])
    pcx, pcy, cz, P, half, invP, keep = oracle_np._project(ps, M, sf, R)
    m = np.asarray(m, dtype=f32)
    hh = ps[:, 3] * ps[:, 3]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        w0 = m / hh
    u = kinematics_ref.kinematic_colours(m, vel, axis, v_ref)[3]
    s, dead = line_widths(len(m), sigma_v, sigma)
    dead |= ~(np.isfinite(m) & np.isfinite(u))
    e = edges(v_min, dv, n_channels)
    out = np.zeros((n_channels, R, R), dtype=np.float64)
    S = np.zeros((R, R), dtype=np.float64)
    for p in range(len(m)):
        if dead[p] or not keep[p]:
            continue
        fp = oracle_np._footprint(pcx[p], pcy[p], half[p], invP[p], P[p], R, mips)
        if fp is None:
            continue
        j0, i0, K, _ = fp
        kw = K.astype(np.float64) * float(w0[p])
        S[j0:j0 + K.shape[0], i0:i0 + K.shape[1]] += kw
        g = response(float(u[p]), s[p], e)
        nz = np.nonzero(g)[0]
        if len(nz):
            out[nz, j0:j0 + K.shape[0], i0:i0 + K.shape[1]] += g[nz, None, None] * kw[None]
    return out, S


def within(got, want, S, rel=1e-5, floor=1e-6):
    """|got - want| <= rel * want + floor * S_pixel per cell -> (ok, the worst excess ratio)"""
    bound = rel * np.abs(want) + floor * S[None]
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return bool((err <= bound).all()), float(ratio.max())
