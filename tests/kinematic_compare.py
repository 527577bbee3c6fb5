"""The comparison of a kinematic frame with the oracle, shared by the kinematic tests and the session matrix: the oracle's rgb
splat fed the reference weights' colours (kinematics_ref.kinematic_colours), and the project's tolerances for its four channels.
R = 128 throughout."""
import numpy as np

import kinematics_ref as ref
import parity_scenes as ps

R = 128
f32 = np.float32
_cache = {}


def oracle_kinematic(scene, mips, M, sf, axis, v_ref, ranges=None):
    """(image (S, A, B, n), fragments, sum|terms| of A) of the oracle's rgb splat of the reference colours; computed once"""
    key = (ps._key(scene["pos"], scene["h"], scene["m"], scene["vel"], np.asarray(M, dtype=f32), f32(sf), np.asarray(axis, dtype=f32),
                   np.asarray(v_ref, dtype=f32)),
           None if ranges is None else tuple(map(tuple, ranges)))      # (the scene is part of the key: the matrix draws several)
    if key not in _cache:
        r, g, b, _ = ref.kinematic_colours(scene["m"], scene["vel"], axis, v_ref)
        want, nfrag = ps.oracle_render(scene["pos"], scene["h"], r, g, b, 2, M, sf, R, mips, ranges)
        terms = ps.oracle_render(scene["pos"], scene["h"], r, np.abs(g), b, 2, M, sf, R, mips, ranges)[0][..., 1]
        want.setflags(write=False)
        terms.setflags(write=False)
        _cache[key] = (want, int(nfrag), terms)
    return _cache[key]


def check_kinematic(got, want, terms, label):
    """the project's tolerances (parity_scenes): S and B 1e-5 relative, the signed A within 1e-5 * sum|terms|, the count exact"""
    assert got.shape == want.shape == (R, R, 4), label
    for c, name in ((0, "S"), (2, "B")):
        d = np.abs(got[..., c].astype(np.float64) - want[..., c])
        rel = np.max(d / np.maximum(np.abs(want[..., c]).astype(np.float64), 1e-300))
        print(f"{label}: channel {name} max rel err {rel:.3g}")
        assert np.allclose(got[..., c], want[..., c], rtol=1e-5, atol=0), (label, name, rel)
    d1 = np.abs(got[..., 1].astype(np.float64) - want[..., 1])
    print(f"{label}: channel A max err / sum|terms| {np.max(d1 / np.maximum(terms.astype(np.float64), 1e-300)):.3g}")
    assert (d1 <= 1e-5 * terms + 1e-30).all(), (label, "A")
    assert np.array_equal(got[..., 3], want[..., 3]), (label, "count")
