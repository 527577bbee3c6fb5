"""What the GPU parity tests share: the oracle call and its tolerances, one scene with every footprint
class at any resolution, and kernel LUTs that differ from the reference's in the two properties the library derives from an upload.

Tolerances, one place (render_and_check): density channel 1e-5 relative; weighted channel within 1e-5 * sum|terms| (it can
cancel); depth channel 1 rtol 1e-5, atol 1e-30; rgb colour channels 1e-5 relative, counter channel exactly equal; the fragment
count exactly the oracle's whenever it is counted.
"""
import hashlib

import numpy as np

MODES = ("density", "weighted", "depth", "rgb")
MIP_SIZES = (64, 32, 16, 8)
MIP_OFFSETS = (0, 4096, 5120, 5376)


def oracle_render(pos, h, a, b, c, mode, M, sf, R, mips, ranges=None):
    from oracle import oracle_c
    x, y, z = (np.ascontiguousarray(pos[:, k]) for k in range(3))
    return oracle_c.splat(x, y, z, h, a, b, c, mode=mode, M=M, sf=sf, R=R, mips=mips, ranges=ranges)


def abs_terms_image(pos, h, m, q, M, sf, R, mips):
    """sum of |val * q| per pixel: the scale of the weighted channel's rounding noise."""
    img, _ = oracle_render(pos, h, m, np.abs(q), None, 0, M, sf, R, mips)
    return img[..., 1]


def check_2ch(got, want, abs_terms, rtol=1e-5):
    d0 = np.abs(got[..., 0] - want[..., 0])
    assert (d0 <= rtol * np.abs(want[..., 0]) + 1e-30).all(), \
        f"density channel: max rel err {np.max(d0 / np.maximum(np.abs(want[..., 0]).astype(np.float64), 1e-300))}"
    d1 = np.abs(got[..., 1] - want[..., 1])
    assert (d1 <= rtol * abs_terms + 1e-30).all(), "weighted channel beyond atol scaled by sum|terms|"


def _rot(a, b):
    ca, sa, cb, sb = np.cos(a), np.sin(a), np.cos(b), np.sin(b)
    rx = np.array([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]])
    ry = np.array([[1, 0, 0], [0, cb, -sb], [0, sb, cb]])
    return rx @ ry


def roll(c):
    """rotation about the line of sight"""
    return np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])


def lut_contract_camera(scale=100.0):
    """(M, sf) of the tilted and rolled camera of the LUT contract tests: the CPU test counts, for this view of all_class_scene(200),
    the (record, strip) pairs that only the exact corner culling drops"""
    from oracle import oracle_np
    return oracle_np.transform_matrix(_rot(0.15, -0.1) @ roll(0.9), np.zeros(3), scale)


# --------------------------------------------------------------------------- scenes
BOUNDARY_WIDTHS = [15.99, 16.0, 16.0001, 32.0, 63.999, 64.0, 64.0001, 128.0]


def make_scene(pos, h, m, q, rgb, P=None, scale=None):
    """A scene is a dict of float32 arrays in the caller's order (pos (n, 3), h, m, q, rgb (n, 3)); P = the nominal widths in px."""
    return {"pos": np.ascontiguousarray(pos, dtype=np.float32), "h": np.ascontiguousarray(h, dtype=np.float32),
            "m": np.ascontiguousarray(m, dtype=np.float32), "q": np.ascontiguousarray(q, dtype=np.float32),
            "rgb": np.ascontiguousarray(rgb, dtype=np.float32), "P": P, "scale": scale}


def all_class_scene(R, n=1500, seed=1, scale=100.0):
    """Footprints of every class at resolution R, whatever R is: widths P log-uniform in [0.3, 4000] px (the first 24 on the class
    boundaries 16 and 64 px and on mip thresholds), h = P * scale / (2 R), centres within +-1.3 image half-widths (partly
    off-screen), every 7th on a pixel corner (ties), z partly outside the slab.  For a camera of that `scale`."""
    rs = np.random.RandomState(seed)
    P = np.exp(rs.uniform(np.log(0.3), np.log(4000.0), n))
    P[:24] = BOUNDARY_WIDTHS * 3
    h = (P * scale / (2.0 * R)).astype(np.float32)
    pos = np.zeros((n, 3), dtype=np.float32)
    pos[:, 0] = rs.uniform(-1.3, 1.3, n) * scale
    pos[:, 1] = rs.uniform(-1.3, 1.3, n) * scale
    pos[:, 2] = rs.uniform(-0.9, 0.9, n) * scale
    pos[::7, :2] = np.round(pos[::7, :2] / (2 * scale / R)) * (2 * scale / R)      # centres on pixel corners: ties
    m = rs.uniform(0.5, 2.0, n).astype(np.float32)
    q = rs.normal(size=n).astype(np.float32)
    rgb = rs.uniform(0.0, 1.0, size=(n, 3)).astype(np.float32)
    return make_scene(pos, h, m, q, rgb, P=P, scale=scale)


def wide_scene(R, n=6000, seed=17, scale=100.0):
    """n footprints of 64 - 3000 px, all inside the z-slab: more than 4096 huge records, so that kernel H2 reads them from band bins"""
    rs = np.random.RandomState(seed)
    pos = np.zeros((n, 3), dtype=np.float32)
    pos[:, :2] = rs.uniform(-1.2, 1.2, size=(n, 2)) * scale
    pos[:, 2] = rs.uniform(-0.5, 0.5, n) * scale
    P = np.exp(rs.uniform(np.log(64.0), np.log(3000.0), n))
    P[:40] = [64.0, 64.0001, 127.99, 128.0] * 10          # class boundary and band-edge widths
    h = (P * scale / (2.0 * R)).astype(np.float32)
    m = rs.uniform(0.5, 2.0, n).astype(np.float32)
    q = rs.normal(size=n).astype(np.float32)
    rgb = rs.uniform(0.0, 1.0, size=(n, 3)).astype(np.float32)
    return make_scene(pos, h, m, q, rgb, P=P, scale=scale)


def class_counts(P):
    """particles by nominal width: below 16 px, in [16, 64), at or above 64 px"""
    P = np.asarray(P)
    return int((P < 16.0).sum()), int(((P >= 16.0) & (P < 64.0)).sum()), int((P >= 64.0).sum())


# --------------------------------------------------------------------------- kernel LUTs
def reference():
    """a copy of the reference's kernel LUT (kernel_lut.kernel_mips() hands out one shared array)"""
    from topsy_amd import kernel_lut
    return kernel_lut.kernel_mips().copy()


def _level(lut, l):
    n = MIP_SIZES[l]
    return lut[MIP_OFFSETS[l]:MIP_OFFSETS[l] + n * n].reshape(n, n)      # (a view: rows j, columns i)


def _outside_disc(n):
    """texels of an n x n level whose centre (-2 + (k + 0.5) * 4 / n per axis) is at least 2 from the middle"""
    c = -2.0 + (np.arange(n) + 0.5) * 4.0 / n
    return c[None, :] ** 2 + c[:, None] ** 2 >= 4.0


def corner_lit(levels, frac=0.25):
    """every outside-the-disc texel of the given levels set to frac * that level's maximum: mirror-symmetric, corners not zero"""
    lut = reference()
    for l in levels:
        T = _level(lut, l)
        T[_outside_disc(MIP_SIZES[l])] = np.float32(frac) * T.max()
    return lut


def one_texel_lit():
    """a single outside-the-disc texel of level 0 lit, in one quadrant only: neither property holds"""
    lut = reference()
    T = _level(lut, 0)
    assert _outside_disc(64)[3, 2]
    T[3, 2] = np.float32(0.25) * T.max()
    return lut


def skew():
    """every texel scaled by its own factor in [1, 1.05): no symmetry left; the corners stay zero (0 * x = 0)"""
    lut = reference()
    lut *= (1.0 + 0.05 * np.random.RandomState(2).uniform(size=lut.shape)).astype(np.float32)
    return lut


def _scaled_lines(axis):
    lut = reference()
    for l, n in enumerate(MIP_SIZES):
        f = (1.0 + 0.05 * np.arange(n) / n).astype(np.float32)
        _level(lut, l)[...] *= f[:, None] if axis == 0 else f[None, :]
    return lut


def lr_only():
    """row j scaled by 1 + 0.05 j / n: the left-right mirror image still equals the level, the top-bottom one does not"""
    return _scaled_lines(0)


def tb_only():
    """column i scaled by 1 + 0.05 i / n: only the top-bottom mirror symmetry survives"""
    return _scaled_lines(1)


def level3_asym():
    """one inside-the-disc texel of level 3 changed by 5 %, levels 0-2 untouched"""
    lut = reference()
    T = _level(lut, 3)
    assert not _outside_disc(8)[2, 3] and T[2, 3] > 0
    T[2, 3] *= np.float32(1.05)
    return lut


def lut_mirror_axes(lut):
    """(left-right, top-bottom): every level equals that mirror image of itself bit for bit"""
    lut = np.ascontiguousarray(lut, dtype=np.float32)
    lr = tb = True
    for l in range(4):
        B = _level(lut, l).view(np.uint32)
        lr = lr and bool(np.array_equal(B, B[:, ::-1]))
        tb = tb and bool(np.array_equal(B, B[::-1, :]))
    return lr, tb


def lut_properties(lut):
    """(zero_outside_disc, mirror_symmetric) as tsp_internal.h defines them: on every mip level, each texel whose centre is at
    least 2 h from the middle is exactly 0 (either sign); every level equals both of its mirror images bit for bit."""
    lut = np.ascontiguousarray(lut, dtype=np.float32)
    zero = all(bool((_level(lut, l)[_outside_disc(MIP_SIZES[l])] == 0.0).all()) for l in range(4))
    lr, tb = lut_mirror_axes(lut)
    return zero, lr and tb


# --------------------------------------------------------------------------- render and compare
_oracle_cache = {}


def _key(*arrays):
    hh = hashlib.sha1()
    for a in arrays:
        hh.update(np.ascontiguousarray(a).tobytes())
    return hh.hexdigest()


def oracle_images(mode, scene, M, sf, R, lut):
    """(image, fragment count, sum|terms| of the weighted channel or None) of the oracle, computed once per input and read-only"""
    pos, h, m, q, rgb = (scene[k] for k in ("pos", "h", "m", "q", "rgb"))
    attrs = {"density": (m,), "weighted": (m, q), "depth": (m,), "rgb": (rgb,)}[mode]
    key = (mode, R, _key(pos, h, *attrs, np.asarray(M, dtype=np.float32), np.float32(sf), lut))
    if key not in _oracle_cache:
        terms = None
        if mode == "rgb":
            want, nfrag = oracle_render(pos, h, rgb[:, 0].copy(), rgb[:, 1].copy(), rgb[:, 2].copy(), 2, M, sf, R, lut)
        elif mode == "depth":
            want, nfrag = oracle_render(pos, h, m, None, None, 1, M, sf, R, lut)
        elif mode == "weighted":
            want, nfrag = oracle_render(pos, h, m, q, None, 0, M, sf, R, lut)
            terms = abs_terms_image(pos, h, m, q, M, sf, R, lut)
            terms.setflags(write=False)
        else:
            want, nfrag = oracle_render(pos, h, m, None, None, 0, M, sf, R, lut)
        want.setflags(write=False)
        _oracle_cache[key] = (want, int(nfrag), terms)
    return _oracle_cache[key]


def upload_scene(ctx, scene, mode):
    """the particles and what `mode` draws, in the caller's order (density: no quantity resident)"""
    pos = scene["pos"]
    ctx.upload_particles(pos[:, 0], pos[:, 1], pos[:, 2], scene["h"], None if mode == "rgb" else scene["m"])
    if mode == "weighted":
        ctx.upload_quantity(scene["q"])
    if mode == "rgb":
        ctx.upload_rgb(scene["rgb"][:, 0].copy(), scene["rgb"][:, 1].copy(), scene["rgb"][:, 2].copy())


def compare_with_oracle(got, mode, want, terms, label=""):
    if mode == "weighted":
        check_2ch(got, want, terms)
    elif mode == "density":
        assert np.allclose(got[..., 0], want[..., 0], rtol=1e-5, atol=0), ("density channel", label)
        assert (got[..., 1] == 0).all(), ("channel 1 of a density render is not 0", label)
    elif mode == "depth":
        assert np.allclose(got[..., 0], want[..., 0], rtol=1e-5, atol=0), ("density channel", label)
        assert np.allclose(got[..., 1], want[..., 1], rtol=1e-5, atol=1e-30), ("depth channel", label)
    else:
        assert np.allclose(got[..., :3], want[..., :3], rtol=1e-5, atol=0), ("colour channels", label)
        assert np.array_equal(got[..., 3], want[..., 3]), ("fragment-count channel must be exact", label)


def render_and_check(ctx, native, mode, scene, M, sf, R, lut, count, flags=None, label=""):
    """Render what is resident in `ctx` in `mode` with count_fragments = count and compare the image (and, when counted, the
    number of fragments) with the oracle fed `scene` and `lut`.  Returns (image, stats)."""
    md = {"density": native.MODE_WEIGHTED, "weighted": native.MODE_WEIGHTED, "depth": native.MODE_DEPTH, "rgb": native.MODE_RGB}[mode]
    ctx.set_option("count_fragments", int(count))
    ctx.render(M, sf, mode=md, flags=native.PIPE_DEFAULT if flags is None else flags)
    got = ctx.read_image()
    st = ctx.stats()
    want, nfrag, terms = oracle_images(mode, scene, M, sf, R, lut)
    label = (mode, R, "count" if count else "cull", label)
    assert got.shape == want.shape, label
    compare_with_oracle(got, mode, want, terms, label)
    if count:
        assert st["n_fragments"] == nfrag, label
    return got, st
