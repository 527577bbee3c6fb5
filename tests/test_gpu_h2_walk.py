"""Kernel H2's two row walks (option h2_walk: 1 = the asm walk, 0 = the C++ walk) draw the same strips.

The asm walk performs the C++ walk's float32 operations in the same order, so the float32 strip sums are bit-identical; only the
order of the float64 flush atomics may differ between two renders.  Each scene is drawn with both walks on both density strip
heights (huge_variant 5: 64x16, 7: 64x32) and must give equal fragment counts and images equal to 1e-6 relative."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from topsy_amd import _native
    _native.load_library()
    return _native


def _scene(R, widths_px, n_per_width, seed, edge_band=0.0):
    """Particles at z = 0 whose footprints are `widths_px` pixels wide (1 px = 1 length unit at scale R / 2), centres at random
    sub-pixel positions over the image plus `edge_band` pixels past each edge (footprints cut by the image border)."""
    rs = np.random.RandomState(seed)
    P = np.repeat(np.asarray(widths_px, np.float64), n_per_width)
    n = len(P)
    lo, hi = -R / 2 - edge_band, R / 2 + edge_band
    x = rs.uniform(lo, hi, n).astype(np.float32)
    y = rs.uniform(lo, hi, n).astype(np.float32)
    z = np.zeros(n, np.float32)
    h = (P / 4).astype(np.float32)      # (the kernel reaches 2 h: a footprint is 4 h wide)
    m = rs.uniform(0.5, 2.0, n).astype(np.float32)
    return x, y, z, h, m


SCENES = {
    # widths just above the bilinear threshold: the texel row changes on every pixel row, float32 rounding may skip one
    "p64_70": (300, np.concatenate([np.linspace(64.0, 64.05, 11), np.linspace(64.1, 70.0, 9)]), 40, 1, 40.0),
    "p100": (300, [100.0, 100.37], 60, 2, 60.0),
    "p300": (333, [300.0, 301.7], 20, 3, 150.0),
    "p1500": (257, [1500.0, 1499.3], 4, 4, 0.0),
    # R not a multiple of the tile (128 x 64 / 128 x 32) nor of a strip: strips cut by the right and bottom image edges
    "mixed_edges": (191, [64.5, 77.0, 130.0, 256.0, 700.0], 25, 5, 80.0),
}


def _render(native, mips, scene, variant, walk, count):
    from oracle import oracle_np
    R, widths, n_per, seed, band = scene
    x, y, z, h, m = _scene(R, widths, n_per, seed, band)
    M, sf = oracle_np.transform_matrix(np.eye(3), np.zeros(3), R / 2.0)
    ctx = native.Context(R, 2)
    try:
        ctx.set_kernel_mips(mips)
        ctx.set_option("huge_variant", variant)
        ctx.set_option("h2_walk", walk)
        ctx.set_option("count_fragments", count)
        ctx.upload_particles(x, y, z, h, m)
        ctx.render(M, sf)
        st = ctx.stats()
        return ctx.read_image(), st["n_fragments"], st["n_huge"]
    finally:
        ctx.close()


def _oracle(mips, scene):
    from oracle import oracle_c, oracle_np
    R, widths, n_per, seed, band = scene
    x, y, z, h, m = _scene(R, widths, n_per, seed, band)
    M, sf = oracle_np.transform_matrix(np.eye(3), np.zeros(3), R / 2.0)
    return oracle_c.splat(x, y, z, h, m, mode=0, M=M, sf=sf, R=R, mips=mips)


@pytest.mark.parametrize("variant", [5, 7])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_asm_walk_matches_cpp_walk(native, mips, name, variant):
    """...and each walk matches the float64 oracle (1e-5, exact fragment count): a mistake both walks share does not pass."""
    scene = SCENES[name]
    want, nfrag = _oracle(mips, scene)
    for count in (1, 0):
        img0, nf0, nh0 = _render(native, mips, scene, variant, 0, count)
        img1, nf1, nh1 = _render(native, mips, scene, variant, 1, count)
        assert nh0 == nh1 and nh0 > 0, "the scene must reach kernel H2"
        if count:
            assert nf0 == nf1 and nf0 > 0
            assert nf0 == nfrag, f"{name}, huge_variant {variant}: fragment count differs from the oracle"
        d = img0[..., 0]
        assert d.max() > 0
        assert (np.abs(img1[..., 0] - d) <= 1e-6 * np.abs(d) + 1e-30).all(), \
            f"{name}, huge_variant {variant}: max rel {np.max(np.abs(img1[..., 0] - d) / np.maximum(np.abs(d), 1e-300))}"
        for walk, img in ((0, img0), (1, img1)):
            w = want[..., 0]
            assert (np.abs(img[..., 0] - w) <= 1e-5 * np.abs(w)).all(), \
                f"{name}, huge_variant {variant}, h2_walk {walk}: max rel err vs the oracle " \
                f"{np.max(np.abs(img[..., 0] - w) / np.maximum(np.abs(w), 1e-300))}"
            assert (img[..., 1] == 0).all()


def test_h2_walk_option_range(native):
    ctx = native.Context(16, 2)
    try:
        ctx.set_option("h2_walk", 0)
        ctx.set_option("h2_walk", 1)
        with pytest.raises(Exception):
            ctx.set_option("h2_walk", 2)
    finally:
        ctx.close()
