"""Weights that are not finite: a particle changes only the pixels its footprint square covers.

The contract comes from the reference's rasteriser: no fragment runs outside a particle's quad, so an infinite or NaN mass,
quantity or colour (or a finite mass whose m / h^2 overflows float32) makes the pixels of that square non-finite and leaves
every other pixel alone.  Each scene below holds clean particles everywhere (the pixels outside the bad squares are non-zero,
so they are really checked) and about 1 % bad ones -- inside the image, cut by each image edge and, for kernel H2, wider than
the image -- and is drawn through every kernel route and option that selects a different build.  Per channel:

  * outside the squares of the bad particles that feed it: finite and equal to the oracle (test_gpu_parity.py's tolerances);
  * where such a particle's kernel value is > 0: not finite (where it is 0, kernels may skip the texel or strip);
  * channels no bad value feeds equal the oracle everywhere (the count channel exactly; channel 1 of a density render is 0);
  * with count_fragments = 1 the fragment count is the oracle's;
  * afterwards the clean particles, rendered with clear = True, equal the oracle (nothing survives in the float64 target).
"""
import numpy as np
import pytest

MODES = ["density", "weighted", "depth", "rgb"]
ORACLE_MODE = {"density": 0, "weighted": 0, "depth": 1, "rgb": 2}
SCALE_PER_PX = 0.01                 # camera scale = 0.01 R: h = P * SCALE_PER_PX / 2 < 1 below 200 px (room for m / h^2 to overflow)


@pytest.fixture(scope="module")
def native():
    from topsy_amd import _native
    _native.load_library()
    return _native


def _camera(R):
    from oracle import oracle_np
    scale = SCALE_PER_PX * R
    M, sf = oracle_np.transform_matrix(np.eye(3), np.zeros(3), scale)
    return M, sf, scale


def _oracle(x, y, z, h, a, b, c, mode, R, mips):
    from oracle import oracle_c
    M, sf, _ = _camera(R)
    return oracle_c.splat(x, y, z, h, a, b, c, mode=mode, M=M, sf=sf, R=R, mips=mips)


# ---- scenes ------------------------------------------------------------------------------------------------------------------
# Pixel coordinates: column i covers [i, i + 1) and the image spans [0, R); world x = (px / R * 2 - 1) * scale, y flipped.

def _to_world(px, py, R):
    scale = SCALE_PER_PX * R
    return ((px / R) * 2.0 - 1.0) * scale, (1.0 - (py / R) * 2.0) * scale


def _scene(route, R, seed):
    """Particle attributes (float32) and the pixel width P of every footprint for one route."""
    rs = np.random.RandomState(seed)
    if route == "small_window":
        # clusters of 512 consecutive particles (one chunk of kernel S) within 28 x 28 px: every chunk's small footprints fit the
        # 40-px LDS window of the rgb build; cluster centres reach past every image edge
        n_cl = 24
        n = 512 * n_cl
        P = np.exp(rs.uniform(np.log(0.6), np.log(10.0), n))
        cen = rs.uniform(-8.0, R + 8.0, size=(n_cl, 2))
        cen[:4] = [[-6.0, R / 2], [R + 6.0, R / 3], [R / 2, -6.0], [R / 4, R + 6.0]]      # clusters cut by each edge
        off = rs.uniform(-1.0, 1.0, size=(n, 2)) * (14.0 - P[:, None] / 2.0)
        pxy = np.repeat(cen, 512, axis=0) + off
    elif route == "small_scattered":
        # unordered: a chunk spans far more than the LDS window, so most footprints leave it for the mid list
        n = 30000
        P = np.exp(rs.uniform(np.log(0.4), np.log(11.0), n))
        pxy = rs.uniform(-4.0, R + 4.0, size=(n, 2))
    elif route == "mid":
        n = 6000
        P = np.exp(rs.uniform(np.log(16.5), np.log(63.9), n))
        P[:12] = [63.999, 32.0, 32.0001, 16.5, 45.3, 17.0] * 2
        pxy = rs.uniform(-20.0, R + 20.0, size=(n, 2))
    elif route == "huge":
        n = 4800                                  # > 4096 visible records: the band bins are used unless huge_band_mib = 0
        P = np.exp(rs.uniform(np.log(64.5), np.log(420.0), n))
        wide = rs.uniform(size=n) < 0.04
        P[wide] = np.exp(rs.uniform(np.log(420.0), np.log(3000.0), wide.sum()))
        P[:8] = [64.0001, 64.5, 65.0, 127.999, 128.0, 256.0, 511.9, 1024.0]
        pxy = rs.uniform(-30.0, R + 30.0, size=(n, 2))
    else:
        raise ValueError(route)
    n = len(P)
    x, y = _to_world(pxy[:, 0], pxy[:, 1], R)
    scale = SCALE_PER_PX * R
    z = rs.uniform(-0.5, 0.5, n) * scale
    h = P * scale / (2.0 * R)
    m = rs.uniform(0.5, 2.0, n)
    q = rs.normal(size=n)
    rgb = rs.uniform(0.1, 1.0, size=(n, 3))
    f = lambda v: np.ascontiguousarray(v, dtype=np.float32)      # noqa: E731
    return dict(route=route, n=n, R=R, P=P, pxy=pxy, x=f(x), y=f(y), z=f(z), h=f(h), m=f(m), q=f(q), rgb=f(rgb))


MASS_KINDS = [("m", np.inf), ("m", -np.inf), ("m", np.nan), ("m", 3.0e38)]          # 3e38 / h^2 overflows: h < 1 for every bad particle
Q_KINDS = [("q", np.inf), ("q", -np.inf), ("q", np.nan)]
RGB_KINDS = [("r", np.inf), ("g", np.nan), ("b", -np.inf), ("r", np.nan), ("g", np.inf), ("b", np.nan), ("r", 3.0e38)]


def _make_bad(sc, mode, seed):
    """Copies of the scene's attributes with ~1 % bad particles (each kind of bad value on its own particles), placed inside the
    image, cut by each image edge and (kernel H2's scene) wider than the image.  Returns (attributes, {kind: particle mask})."""
    rs = np.random.RandomState(seed + 17)
    n, R, P = sc["n"], sc["R"], sc["P"]
    kinds = {"density": MASS_KINDS, "depth": MASS_KINDS, "weighted": MASS_KINDS + Q_KINDS, "rgb": RGB_KINDS}[mode]
    huge = P.min() >= 64.0                   # kernel H2's scene: 1 % of its squares would cover the whole 300^2 image
    nb = 2 * len(kinds) if huge else max(len(kinds) * 4, n // 100)
    bad = np.sort(rs.choice(n, nb, replace=False))
    att = {k: sc[k].copy() for k in ("x", "y", "z", "h", "m", "q", "rgb")}
    # placement: every fifth bad particle inside, the others centred just across / on one of the four edges
    pxy = sc["pxy"][bad].copy()
    Pb = rs.uniform(64.5, 90.0, nb) if huge else P[bad].copy()
    half = Pb / 2.0
    for j, i in enumerate(bad):
        where = j % 5 if sc["route"] != "small_window" else -1      # (kernel S's clusters: bad ones stay in theirs, some cut by an edge)
        if where == 1:
            pxy[j, 0] = -0.4 * half[j]
        elif where == 2:
            pxy[j, 0] = R + 0.4 * half[j]
        elif where == 3:
            pxy[j, 1] = -0.4 * half[j]
        elif where == 4:
            pxy[j, 1] = R + 0.4 * half[j]
        elif where == 0 and half[j] < R / 2:
            pxy[j] = np.clip(pxy[j], half[j], R - half[j])
    if huge:                                 # narrow ones, and some wider than the image reaching 15 % of it past one edge
        for j in range(2, nb, 5):
            Pb[j] = R * rs.uniform(1.2, 3.0)
            e, t = j % 4, rs.uniform(0.1, 0.9) * R
            pxy[j] = [[0.15 * R - Pb[j] / 2, t], [R - 0.15 * R + Pb[j] / 2, t], [t, 0.15 * R - Pb[j] / 2], [t, R - 0.15 * R + Pb[j] / 2]][e]
    scale = SCALE_PER_PX * R
    wx, wy = _to_world(pxy[:, 0], pxy[:, 1], R)
    att["x"][bad] = wx; att["y"][bad] = wy
    att["h"][bad] = Pb * scale / (2.0 * R)
    masks = {}
    for j, i in enumerate(bad):
        what, val = kinds[j % len(kinds)]
        if val == 3.0e38 and att["h"][i] >= 1.0:      # (overflow needs h < 1: a wide footprint takes an infinite weight instead)
            val = np.inf
        if what == "m":
            att["m"][i] = val
        elif what == "q":
            att["q"][i] = val
        else:
            att["rgb"][i, "rgb".index(what)] = val
        masks.setdefault(what, np.zeros(n, dtype=bool))[i] = True
    for k in ("x", "y", "h"):
        att[k] = np.ascontiguousarray(att[k], dtype=np.float32)
    return att, masks


def _weights(att, mode):
    if mode == "rgb":
        return att["rgb"][:, 0].copy(), att["rgb"][:, 1].copy(), att["rgb"][:, 2].copy()
    if mode == "weighted":
        return att["m"], att["q"], None
    return att["m"], None, None


def _feeds(mode, masks, n):
    """Per image channel: the bad particles whose value reaches it."""
    none = np.zeros(n, dtype=bool)
    mm = masks.get("m", none)
    if mode == "density":
        return [mm, None]                                          # channel 1 stays exactly 0
    if mode == "depth":
        return [mm, mm]
    if mode == "weighted":
        return [mm, mm | masks.get("q", none)]
    return [masks.get("r", none), masks.get("g", none), masks.get("b", none), none]      # the count channel takes no weight


class Reference:
    """Oracle images of one (scene, mode), computed once and reused for every route option."""

    def __init__(self, sc, att, masks, mode, mips):
        R, n = sc["R"], sc["n"]
        self.mode = mode
        a, b, c = _weights(att, mode)
        geo = (att["x"], att["y"], att["z"], att["h"])
        with np.errstate(all="ignore"):
            self.want, self.nfrag = _oracle(*geo, a, b, c, ORACLE_MODE[mode], R, mips)
            self.abs_terms = _oracle(*geo, a, np.abs(b), None, 0, R, mips)[0][..., 1] if mode == "weighted" else None
            # the clean scene (the bad values replaced by the clean ones): what the final clear render must give
            ca, cb, cc = _weights({k: sc[k] for k in ("m", "q", "rgb")}, mode)
            self.clean, self.clean_frag = _oracle(*geo, ca, cb, cc, ORACLE_MODE[mode], R, mips)
            self.clean_terms = _oracle(*geo, ca, np.abs(cb), None, 0, R, mips)[0][..., 1] if mode == "weighted" else None
        # per channel: the squares of the bad particles feeding it (count channel of an rgb render of them alone) and where one of
        # their kernel values is > 0 (its channel 0)
        self.touched, self.kpos = [], []
        cache = {}
        ones = np.ones(n, dtype=np.float32)
        for sel in _feeds(mode, masks, n):
            if sel is None or not sel.any():
                self.touched.append(None); self.kpos.append(None)
                continue
            key = sel.tobytes()
            if key not in cache:
                img, _ = _oracle(*(np.ascontiguousarray(v[sel]) for v in geo), ones[sel], ones[sel], ones[sel], 2, R, mips)
                cache[key] = (img[..., 3] > 0, img[..., 0] > 0)
            self.touched.append(cache[key][0]); self.kpos.append(cache[key][1])
        self.feeds = _feeds(mode, masks, n)

    def check(self, got, label, clean=False):
        want = self.clean if clean else self.want
        terms = self.clean_terms if clean else self.abs_terms
        C = want.shape[-1]
        for ch in range(C):
            g, w = got[..., ch], want[..., ch]
            if self.mode == "density" and ch == 1:
                assert (g == 0).all(), f"{label}: channel 1 of a density render is not 0"
                continue
            out = np.ones(g.shape, dtype=bool) if (clean or self.touched[ch] is None) else ~self.touched[ch]
            assert np.isfinite(w[out]).all(), f"{label}: the oracle is not finite outside the bad squares (channel {ch})"
            assert np.isfinite(g[out]).all(), \
                f"{label}: channel {ch} is not finite at {int((~np.isfinite(g[out])).sum())} pixels outside every bad square"
            d = np.abs(g[out].astype(np.float64) - w[out])
            if self.mode == "rgb" and ch == 3:
                assert np.array_equal(g, w), f"{label}: fragment-count channel differs"
            elif self.mode == "weighted" and ch == 1:
                assert (d <= 1e-5 * terms[out] + 1e-30).all(), f"{label}: weighted channel beyond atol scaled by sum|terms|"
            else:
                tol = 1e-5 * np.abs(w[out]) + (1e-30 if (self.mode == "depth" and ch == 1) else 0.0)
                assert (d <= tol).all(), \
                    f"{label}: channel {ch} max rel err {np.max(d / np.maximum(np.abs(w[out]), 1e-300))} outside the bad squares"
            if not clean and self.kpos[ch] is not None:
                inside = self.kpos[ch]
                assert inside.any()
                bad = np.isfinite(g[inside])
                assert not bad.any(), f"{label}: channel {ch} is finite at {int(bad.sum())} pixels where a bad weight has k > 0"


def _context(native, sc, mode, att, mips):
    ctx = native.Context(sc["R"], 4 if mode == "rgb" else 2)
    ctx.set_kernel_mips(mips)
    _upload(native, ctx, mode, att)
    return ctx


def _upload(native, ctx, mode, att):
    ctx.upload_particles(att["x"], att["y"], att["z"], att["h"], None if mode == "rgb" else att["m"])
    if mode == "rgb":
        ctx.upload_rgb(att["rgb"][:, 0].copy(), att["rgb"][:, 1].copy(), att["rgb"][:, 2].copy())
    elif mode == "weighted":
        ctx.upload_quantity(att["q"])


def _native_mode(native, mode):
    return {"density": native.MODE_WEIGHTED, "weighted": native.MODE_WEIGHTED, "depth": native.MODE_DEPTH,
            "rgb": native.MODE_RGB}[mode]


DEFAULTS = {"huge_variant": 1, "h2_walk": 1, "huge_band_mib": 6144, "huge_split": 0, "p_small_milli": 16000,
            "mid_narrow_px_milli": 64000, "count_fragments": 0}


def _combos(route, mode):
    if route in ("small_window", "small_scattered"):
        base = [{}]
    elif route == "mid":
        base = [{"p_small_milli": 0, "mid_narrow_px_milli": v} for v in (64000, 0, 24000)]
    else:
        variants = (1, 2, 4, 5, 6, 7) if mode == "density" else (1, 4)
        walks = (0, 1) if mode == "density" else (1,)
        base = [{"huge_variant": v, "h2_walk": w, "huge_band_mib": b, "huge_split": s}
                for v in variants for w in walks for b in (6144, 0) for s in (0, 1)]
    return [dict(o, count_fragments=c) for o in base for c in (0, 1)]


def _route_stats(route, st, n):
    if route == "small_window":
        assert st["n_small"] > 0.6 * n and st["n_mid"] == 0 and st["n_huge"] == 0, st
    elif route == "small_scattered":
        assert st["n_mid"] > n // 4 and st["n_small"] > 0 and st["n_huge"] == 0, st
    elif route == "mid":
        assert st["n_small"] == 0 and st["n_huge"] == 0 and st["n_mid"] > 0.8 * n, st
    else:
        assert st["n_small"] == 0 and st["n_mid"] == 0 and st["n_huge"] > 4096, st


ROUTES = [("small_window", 300), ("small_scattered", 1024), ("mid", 300), ("huge", 300)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_nonfinite_weights_touch_only_their_squares(native, mips, route, mode):
    route, R = route
    seed = {"small_window": 1, "small_scattered": 2, "mid": 3, "huge": 4}[route]
    sc = _scene(route, R, seed)
    att, masks = _make_bad(sc, mode, seed)
    ref = Reference(sc, att, masks, mode, mips)
    M, sf, _ = _camera(R)
    md = _native_mode(native, mode)
    ctx = _context(native, sc, mode, att, mips)
    try:
        for opts in _combos(route, mode):
            for k, v in dict(DEFAULTS, **opts).items():
                ctx.set_option(k, v)
            ctx.render(M, sf, mode=md)
            got = ctx.read_image()
            st = ctx.stats()
            label = f"{route}/{mode} {opts}"
            _route_stats(route, st, sc["n"])
            ref.check(got, label)
            if opts["count_fragments"]:
                assert st["n_fragments"] == ref.nfrag, label
        # the per-pixel generic kernel: the contract in its plainest form
        for count in (0, 1):
            ctx.set_option("count_fragments", count)
            ctx.render(M, sf, mode=md, flags=native.PIPE_GENERIC)
            ref.check(ctx.read_image(), f"{route}/{mode} generic")
            if count:
                assert ctx.stats()["n_fragments"] == ref.nfrag
        # nothing non-finite survives in the float64 target: the clean particles, rendered with clear, equal the oracle
        for k, v in DEFAULTS.items():
            ctx.set_option(k, v)
        _upload(native, ctx, mode, {k: sc[k] for k in ("x", "y", "z", "h", "m", "q", "rgb")} | {k: att[k] for k in ("x", "y", "z", "h")})
        ctx.render(M, sf, mode=md, clear=True)
        ref.check(ctx.read_image(), f"{route}/{mode} clean after bad", clean=True)
    finally:
        ctx.close()


def test_oracles_agree_on_nonfinite_weights(mips):
    """The GPU test's reference, held to the same contract on every run: the C oracle and the numpy oracle give the same
    finite / non-finite pattern and values on a bad-weight scene, and outside the bad squares the image is bit for bit the render
    without the bad particles."""
    from oracle import oracle_c, oracle_np
    R = 48
    M, sf, scale = _camera(R)
    rs = np.random.RandomState(5)
    n = 260
    P = np.exp(rs.uniform(np.log(0.8), np.log(40.0), n))
    pxy = rs.uniform(-5.0, R + 5.0, size=(n, 2))
    x, y = _to_world(pxy[:, 0], pxy[:, 1], R)
    x, y = x.astype(np.float32), y.astype(np.float32)
    z = np.zeros(n, np.float32)
    h = (P * scale / (2.0 * R)).astype(np.float32)
    m = rs.uniform(0.5, 2.0, n).astype(np.float32)
    q = rs.normal(size=n).astype(np.float32)
    rgb = rs.uniform(0.1, 1.0, size=(n, 3)).astype(np.float32)
    bad = np.arange(3, n, 37)
    bm = np.zeros(n, dtype=bool); bm[bad] = True
    m[bad[0::4]] = np.inf; m[bad[1::4]] = np.nan; m[bad[2::4]] = -np.inf; q[bad[3::4]] = np.nan
    rgb[bad[0::3], 0] = np.inf; rgb[bad[1::3], 1] = np.nan; rgb[bad[2::3], 2] = 3.0e38
    ps = np.stack([x, y, z, h], axis=1)
    cases = [(0, m, q, None), (0, m, None, None), (2, rgb[:, 0].copy(), rgb[:, 1].copy(), rgb[:, 2].copy())]
    for mode, a, b, c in cases:
        with np.errstate(all="ignore"):
            got_c, _ = oracle_c.splat(x, y, z, h, a, b, c, mode=mode, M=M, sf=sf, R=R, mips=mips)
            got_np = oracle_np.splat(ps, a, b, M, sf, R, mips) if mode == 0 else oracle_np.splat_rgb(ps, np.stack([a, b, c], 1), M, sf, R, mips)
        assert np.array_equal(np.isfinite(got_c), np.isfinite(got_np)), mode
        fin = np.isfinite(got_c)
        assert (~fin).any() and fin.any()
        assert np.allclose(got_c[fin], got_np[fin], rtol=1e-5, atol=0), mode
        # without the bad particles: identical outside their squares
        keep = ~bm
        clean, _ = oracle_c.splat(x[keep], y[keep], z[keep], h[keep], a[keep], None if b is None else b[keep],
                                  None if c is None else c[keep], mode=mode, M=M, sf=sf, R=R, mips=mips)
        ones = np.ones(bm.sum(), np.float32)
        sq, _ = oracle_c.splat(x[bm], y[bm], z[bm], h[bm], ones, ones, ones, mode=2, M=M, sf=sf, R=R, mips=mips)
        outside = sq[..., 3] == 0
        assert outside.any() and (~outside).any()
        assert np.array_equal(got_c[outside], clean[outside]), mode
        assert np.isfinite(got_c[outside]).all()
