"""Kernel H2's row clip (option h2_chord: 1 = a hit's pixel rows outside the chord of the footprint's inscribed disc are not walked,
0 = every row of the square) draws the same strips.

A clipped row contributed weight x (0 top + 0 bot) to every pixel, so the float32 strip sums are bit-identical; only the order of the
float64 flush atomics may differ between two renders.  Each scene is drawn with both settings on both density strip heights
(huge_variant 5: 64x16, 7: 64x32; the two-channel and rgb scenes take the C++ walk's 64x16 builds under either) and must give equal
record and fragment counts, images equal to 1e-6 relative with exact zeros where the oracle has them, and each image the oracle's to
1e-5.  The scenes are the smallest at which the clip can go wrong (h2_chord_ref.py restates the row test; test_h2_chord_cpu.py checks
it, and the pinned footprints of `emptied`, on the CPU)."""
import numpy as np
import pytest

import h2_chord_ref as ref

pytestmark = pytest.mark.gpu

f32 = np.float32


@pytest.fixture(scope="module")
def native():
    from topsy_amd import _native
    _native.load_library()
    return _native


def _random(R, widths_px, n_per_width, seed, edge_band=0.0):
    """as tests/test_gpu_h2_walk.py: footprints `widths_px` pixels wide (1 px = 1 length unit at scale R / 2) at random sub-pixel
    centres over the image plus `edge_band` pixels past each edge"""
    rs = np.random.RandomState(seed)
    P = np.repeat(np.asarray(widths_px, np.float64), n_per_width)
    n = len(P)
    lo, hi = -R / 2 - edge_band, R / 2 + edge_band
    x = rs.uniform(lo, hi, n).astype(f32)
    y = rs.uniform(lo, hi, n).astype(f32)
    m = rs.uniform(0.5, 2.0, n).astype(f32)
    return {"R": R, "x": x, "y": y, "z": np.zeros(n, f32), "h": (P / 4).astype(f32), "m": m, "mode": "density"}


def _pinned(R, centres_px, P, seed=0):
    """footprints P pixels wide centred on the given pixel coordinates"""
    rs = np.random.RandomState(seed)
    n = len(centres_px)
    xy = np.array([ref.centre_to_world(R, px, py) for px, py in centres_px])
    return {"R": R, "x": xy[:, 0].astype(f32), "y": xy[:, 1].astype(f32), "z": np.zeros(n, f32), "h": np.full(n, P / 4, f32),
            "m": rs.uniform(0.5, 2.0, n).astype(f32), "mode": "density"}


def _with_channels(scene, mode, seed):
    rs = np.random.RandomState(seed)
    n = len(scene["x"])
    out = dict(scene, mode=mode)
    if mode == "weighted":
        out["q"] = rs.uniform(0.5, 1.5, n).astype(f32)
    else:
        out["rgb"] = rs.uniform(0.1, 1.0, size=(3, n)).astype(f32)
    return out


def _infinite_mass(scene, i):
    out = dict(scene, m=scene["m"].copy(), nonfinite=i)
    out["m"][i] = np.inf
    return out


SCENES = {
    # (a) one footprint of 300 px centred in the image: the shoulder strips exist
    "one300": _pinned(333, [(166.5, 166.5)], 300.0),
    # (a') its centre 0.5 px either side of a strip's column edge (x = 128) and of a strip's row edge (y = 160, an edge of the 16- and of
    # the 32-row strips): sdx = 0 against sdx > 0, and the first or last clipped row on a row-group boundary
    "edges300": _pinned(333, [(127.5, 170.3), (128.5, 170.3), (170.3, 159.5), (170.3, 160.5)], 300.0),
    # (b) widths just above the bilinear threshold: a texel-row change on every pixel row, float32 rounding may skip one -- also on the
    # row that the clip makes the first covered one
    "p64_70": _random(300, np.concatenate([np.linspace(64.0, 64.05, 11), np.linspace(64.1, 70.0, 9)]), 40, 1, 40.0),
    # (c) the clip empties a hit's rows in a strip that the strip test keeps (h2_chord_ref.EMPTIED)
    "emptied": _pinned(333, [(cx, cy) for cx, cy, _, _, _ in ref.EMPTIED], ref.EMPTIED_P),
    # (d) footprints cut by the right and bottom image edges, R no multiple of a tile or a strip
    "mixed_edges": _random(191, [64.5, 77.0, 130.0, 256.0, 700.0], 25, 5, 80.0),
    # (e) nothing to clip
    "p1500": _random(257, [1500.0, 1499.3], 4, 4, 0.0),
    # (f) one record with an infinite mass among finite ones: it never reaches kernel H2
    "inf_mass": _infinite_mass(_random(333, [300.0, 301.7], 10, 3, 100.0), 7),
    # the C++ walk's multi-channel builds take the clipped masks too
    "weighted": _with_channels(_random(300, [100.0, 180.3], 40, 6, 60.0), "weighted", 16),
    "rgb": _with_channels(_random(300, [100.0, 180.3], 40, 7, 60.0), "rgb", 17),
}


def _view(scene):
    from oracle import oracle_np
    return oracle_np.transform_matrix(np.eye(3), np.zeros(3), scene["R"] / 2.0)


def _upload(native, mips, scene):
    rgb = scene["mode"] == "rgb"
    ctx = native.Context(scene["R"], 4 if rgb else 2)
    ctx.set_kernel_mips(mips)
    ctx.upload_particles(scene["x"], scene["y"], scene["z"], scene["h"], scene["m"])
    if scene["mode"] == "weighted":
        ctx.upload_quantity(scene["q"])
    if rgb:
        ctx.upload_rgb(*scene["rgb"])
    return ctx


def _render(native, mips, scene, variant, chord, count):
    M, sf = _view(scene)
    ctx = _upload(native, mips, scene)
    try:
        ctx.set_option("huge_variant", variant)
        ctx.set_option("h2_walk", 1)
        ctx.set_option("h2_chord", chord)
        ctx.set_option("count_fragments", count)
        ctx.render(M, sf, mode=native.MODE_RGB if scene["mode"] == "rgb" else native.MODE_WEIGHTED)
        st = ctx.stats()
        return ctx.read_image().astype(np.float64), st["n_fragments"], st["n_huge"]
    finally:
        ctx.close()


_oracles = {}


def _oracle(mips, name):
    """(image, fragment count) of the float64 oracle, computed once per scene"""
    if name not in _oracles:
        from oracle import oracle_c
        s = SCENES[name]
        M, sf = _view(s)
        args = (s["x"], s["y"], s["z"], s["h"])
        if s["mode"] == "rgb":
            _oracles[name] = oracle_c.splat(*args, *s["rgb"], mode=2, M=M, sf=sf, R=s["R"], mips=mips)
        else:
            _oracles[name] = oracle_c.splat(*args, s["m"], s.get("q"), mode=0, M=M, sf=sf, R=s["R"], mips=mips)
    return _oracles[name]


def _square_mask(scene, i):
    """pixels within one pixel of record i's footprint square"""
    R = scene["R"]
    pcx, pcy, half = scene["x"][i] + R / 2.0, R / 2.0 - scene["y"][i], 2.0 * scene["h"][i]
    c = np.arange(R) + 0.5
    return (np.abs(c - pcy) < half + 1.0)[:, None] & (np.abs(c - pcx) < half + 1.0)[None, :]


@pytest.mark.parametrize("variant", [5, 7])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_row_clip_changes_no_pixel(native, mips, name, variant):
    scene = SCENES[name]
    want, nfrag = _oracle(mips, name)
    want = want.astype(np.float64)
    value_channels = {"density": [0], "weighted": [0, 1], "rgb": [0, 1, 2]}[scene["mode"]]
    for count in (1, 0):
        img0, nf0, nh0 = _render(native, mips, scene, variant, 0, count)
        img1, nf1, nh1 = _render(native, mips, scene, variant, 1, count)
        assert nh0 == nh1 and nh0 > 0, "the scene must reach kernel H2"
        if count:
            assert nf0 == nf1 and nf0 > 0
            assert nf0 == nfrag, f"{name}, huge_variant {variant}: fragment count differs from the oracle"
        check = np.ones(want.shape[:2], bool)
        if "nonfinite" in scene:
            # NaN / inf appear only inside that record's square, the same ones under both settings; the rest is checked as usual
            bad0, bad1 = ~np.isfinite(img0).all(axis=-1), ~np.isfinite(img1).all(axis=-1)
            assert bad0.any() and np.array_equal(bad0, bad1)
            assert not (bad0 & ~_square_mask(scene, scene["nonfinite"])).any()
            assert np.array_equal(np.isnan(img0), np.isnan(img1))
            check = ~_square_mask(scene, scene["nonfinite"])
        for c in value_channels:
            a, b, w = img0[..., c][check], img1[..., c][check], want[..., c][check]
            assert a.max() > 0
            print(f"{name} v{variant} count {count} ch {c}: 1 vs 0 max rel {np.max(np.abs(b - a) / np.maximum(np.abs(a), 1e-300)):.3g}; "
                  f"vs the oracle {np.max(np.abs(a - w) / np.maximum(np.abs(w), 1e-300)):.3g} / "
                  f"{np.max(np.abs(b - w) / np.maximum(np.abs(w), 1e-300)):.3g}")
            nz = w != 0
            assert (np.abs(b[nz] - a[nz]) <= 1e-6 * np.abs(a[nz])).all(), f"{name}, huge_variant {variant}, channel {c}"
            assert (a[~nz] == 0).all() and (b[~nz] == 0).all(), f"{name}, huge_variant {variant}, channel {c}: the oracle's zeros"
            for chord, img in ((0, a), (1, b)):
                assert (np.abs(img - w) <= 1e-5 * np.abs(w)).all(), f"{name}, huge_variant {variant}, h2_chord {chord}, channel {c}"
        if scene["mode"] == "density":
            assert (img0[..., 1][check] == 0).all() and (img1[..., 1][check] == 0).all()
        if scene["mode"] == "rgb":      # (the count channel does not go through kernel H2)
            assert np.array_equal(img0[..., 3], want[..., 3]) and np.array_equal(img1[..., 3], want[..., 3])


def test_option_is_read_by_every_render(native, mips):
    """one context, h2_chord 1, then 0, then 1: the same image each time"""
    scene = SCENES["edges300"]
    M, sf = _view(scene)
    ctx = _upload(native, mips, scene)
    try:
        imgs = []
        for chord in (1, 0, 1):
            ctx.set_option("h2_chord", chord)
            ctx.render(M, sf)
            imgs.append(ctx.read_image()[..., 0].astype(np.float64))
        assert imgs[0].max() > 0
        for img in imgs[1:]:
            assert (np.abs(img - imgs[0]) <= 1e-6 * np.abs(imgs[0])).all()
    finally:
        ctx.close()


def test_h2_chord_option_range(native):
    ctx = native.Context(16, 2)
    try:
        ctx.set_option("h2_chord", 0)
        ctx.set_option("h2_chord", 1)
        with pytest.raises(Exception):
            ctx.set_option("h2_chord", 2)
    finally:
        ctx.close()
