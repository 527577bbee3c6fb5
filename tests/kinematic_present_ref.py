"""Numpy restatement of the composed kinematic frame (test infrastructure): the moment bases of tsp_present
(include/topsy_splat.h "Frame composition", "Moment bases") -- the four raw channels (S, A, B, n) sampled onto the canvas by
present_ref.sample_base, the moments of the sampled sums by kinematics_ref.velocity_moments (float64, one rounding per step),
the scalar map of oracle_np on (value, 0), unweighted, then the layers by present_ref's rules.  `base` and the layers are the
dicts of topsy_amd._native.Context.present."""
import numpy as np

import kinematics_ref
import present_ref
import surface_present_ref
from oracle import oracle_np

f32 = np.float32
CHANNEL = {"moment-mean": 1, "moment-sigma": 2}


def moment_canvas(img, W, H, which):
    """(H, W) float32: the moment (`which`: a key of CHANNEL) of the sums sampled onto the canvas; NaN where there is none."""
    s, _ = present_ref.sample_base(img, W, H)
    return kinematics_ref.velocity_moments(s)[..., CHANNEL[which]]


def colormap(value, base):
    """The scalar map, unweighted, of a float32 array of any shape -> (..., 4) uint8."""
    pair = np.stack([value, np.zeros_like(value)], axis=-1).astype(f32)
    return oracle_np.colormap_scalar(pair, base["lut"], base["vmin"], base["vmax"], base.get("log", False), False)


def base_layer(img, W, H, base):
    """(H, W, 4) uint8: the colormapped canvas before the layers."""
    return colormap(moment_canvas(img, W, H, base["map"]), base)


def compose(img, W, H, base, layers=()):
    """tsp_present with a moment base in numpy: (H, W, 4) uint8."""
    return surface_present_ref.draw_layers(base_layer(img, W, H, base), layers)
