"""Spectral cubes without a GPU: the float64 model's channel response against Sheppard's formulas, the s = 0 rule, the SpectralCube
reductions on a hand-made cube, every ValueError of the argument checks, and the slice and carve arithmetic of
topsy_amd/csrc/tsp_cube_layout.h at its edges, driven through tsp_spectral_cube_layout (a host function: it needs no device)."""
import numpy as np
import pytest

import spectral_cube_ref as ref

f32 = np.float32


# ---- the model's channel response ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [1.0, 0.5, 0.25])                 # dv / s
@pytest.mark.parametrize("u", [0.0, 3.7, -41.3, 12.5, 10.0])       # inside a channel, on a centre, on an edge
def test_response_obeys_sheppard(u, ratio):
    """On a band covering u -+ 8 s with dv <= s: sum g = 1, the mean is u and the variance s^2 + dv^2 / 12, up to the aliasing terms
    of order exp(-2 pi^2 s^2 / dv^2) (3e-9 at dv = s) and the tails beyond 8 s (1e-15).  Measured here at dv = s: |sum g - 1| <= 2.3e-16,
    |mean - u| <= 8.1e-10 s, |var - (s^2 + dv^2 / 12)| <= 3.4e-9 s^2 (at dv <= s / 2: 1e-15, 3e-15); the bounds asserted are 1e-12,
    1e-6 s and 1e-6 s^2."""
    s = 7.3
    dv = ratio * s
    n = int(np.ceil(16.0 * s / dv)) + 4
    v_min = u - 8.0 * s - 1.3 * dv
    e = ref.edges(v_min, dv, n)
    assert e[0] <= u - 8 * s and e[-1] >= u + 8 * s
    g = ref.response(u, s, e)
    vc = 0.5 * (e[:-1] + e[1:])
    total, mean = g.sum(), (g * vc).sum()
    var = (g * (vc - u) ** 2).sum()
    print(f"u={u} dv/s={ratio}: sum-1={total - 1:.3e} (mean-u)/s={(mean - u) / s:.3e} dvar/s^2={(var - (s * s + dv * dv / 12)) / (s * s):.3e}")
    assert (g >= 0).all()
    assert abs(total - 1.0) <= 1e-12
    assert abs(mean - u) <= 1e-6 * s
    assert abs(var - (s * s + dv * dv / 12.0)) <= 1e-6 * s * s


def test_response_keeps_its_tails():
    """the cancellation-free form: far channels are tiny and positive, not 0 or noise"""
    e = ref.edges(0.0, 1.0, 40)
    g = ref.response(0.5, 1.0, e)
    assert g[0] == pytest.approx(0.3829249225480262, rel=1e-14)
    assert 0 < g[30] < 1e-190 and (np.diff(g) < 0).all()
    assert np.array_equal(ref.response(39.5, 1.0, e), g[::-1])


def test_zero_width_line_falls_in_one_channel_and_an_edge_in_the_upper_one():
    e = ref.edges(-400.0, 20.0, 40)
    for u, c in ((-400.0, 0), (-380.0, 1), (0.0, 20), (19.999, 20), (399.99, 39), (-0.0, 20)):
        g = ref.response(u, 0.0, e)
        assert g.sum() == 1.0 and g[c] == 1.0, (u, c)
    for u in (-400.001, 400.0, 1e9, -1e9):
        assert ref.response(u, 0.0, e).sum() == 0.0, u


def test_dead_particles_of_the_model():
    s, dead = ref.line_widths(5, 3.0, np.array([0.0, np.nan, np.inf, -1.0, 4.0], dtype=f32))
    assert dead.tolist() == [False, True, True, True, False]
    assert s[0] == 3.0 and s[4] == 5.0


# ---- SpectralCube --------------------------------------------------------------------------------------------------------------
def hand_made():
    from topsy_amd.spectral import SpectralCube
    d = np.zeros((4, 3, 3), dtype=f32)
    d[:, 0, 0] = [1, 1, 1, 1]        # flat over the band
    d[2, 1, 1] = 5.0                 # one channel
    d[0, 2, 1], d[3, 2, 1] = 2.0, 2.0
    return SpectralCube(d, -20.0, 10.0)


def test_cube_axes():
    c = hand_made()
    assert c.n_channels == 4 and c.resolution == 3 and c.dv == 10.0
    assert c.v_edges.dtype == np.float64 and np.array_equal(c.v_edges, [-20.0, -10.0, 0.0, 10.0, 20.0])
    assert c.v_centers.dtype == np.float64 and np.array_equal(c.v_centers, [-15.0, -5.0, 5.0, 15.0])


def test_cube_moments():
    c = hand_made()
    m0, m1, m2 = c.moment(0), c.moment(1), c.moment(2)
    assert m0.dtype == np.float64 and m0[0, 0] == 4.0 and m0[1, 1] == 5.0 and m0[2, 1] == 4.0 and m0[1, 0] == 0.0
    assert m1[0, 0] == 0.0 and m1[1, 1] == 5.0 and m1[2, 1] == 0.0
    assert np.isnan(m1[1, 0]) and np.isnan(m2[1, 0])
    # flat over four channels: variance (225 + 25) / 2 = 125, less Sheppard's 100 / 12
    assert m2[0, 0] == pytest.approx(np.sqrt(125.0 - 100.0 / 12.0), rel=1e-15)
    assert m2[1, 1] == 0.0                       # one channel: 0 - dv^2 / 12, clipped
    assert m2[2, 1] == pytest.approx(np.sqrt(225.0 - 100.0 / 12.0), rel=1e-15)
    with pytest.raises(ValueError, match="order must be 0, 1 or 2"):
        c.moment(3)


def test_cube_spectrum_and_pv():
    c = hand_made()
    assert c.spectrum().dtype == np.float64 and np.array_equal(c.spectrum(), [3.0, 1.0, 6.0, 3.0])
    mask = np.zeros((3, 3), dtype=bool)
    mask[2, 1] = True
    assert np.array_equal(c.spectrum(mask), [2.0, 0.0, 0.0, 2.0])
    with pytest.raises(ValueError, match="mask must be"):
        c.spectrum(np.ones((3, 3)))
    with pytest.raises(ValueError, match="mask must be"):
        c.spectrum(np.ones((2, 3), dtype=bool))
    pv0 = c.pv(0)
    assert pv0.shape == (4, 3) and np.array_equal(pv0[:, 1], [2.0, 0.0, 5.0, 2.0]) and np.array_equal(pv0[:, 0], [1, 1, 1, 1])
    assert np.array_equal(c.pv(0, rows=(1, 2))[:, 1], [0.0, 0.0, 5.0, 0.0])
    pv1 = c.pv(1)
    assert np.array_equal(pv1[:, 2], [2.0, 0.0, 0.0, 2.0]) and np.array_equal(c.pv(1, rows=(0, 1))[:, 2], [0, 0, 0, 0])
    with pytest.raises(ValueError, match="axis must be 0"):
        c.pv(2)
    for bad in ((2, 2), (-1, 2), (0, 4), (0.0, 2), "ab", 3):
        with pytest.raises(ValueError, match="rows must be"):
            c.pv(0, rows=bad)


def test_cube_constructor_checks():
    from topsy_amd.spectral import SpectralCube
    with pytest.raises(ValueError, match="a cube is"):
        SpectralCube(np.zeros((4, 3)), 0.0, 1.0)
    with pytest.raises(ValueError, match="a cube is"):
        SpectralCube(np.zeros((4, 3, 2)), 0.0, 1.0)
    for v_min, dv in ((np.nan, 1.0), (0.0, 0.0), (0.0, -1.0), (0.0, np.inf)):
        with pytest.raises(ValueError, match="v_min must be finite"):
            SpectralCube(np.zeros((4, 3, 3)), v_min, dv)


# ---- argument checks -----------------------------------------------------------------------------------------------------------
def test_check_cube_arguments():
    from topsy_amd.spectral import check_cube_arguments
    ok = dict(n=10, resolution=64, v_range=(-1.0, 1.0), n_channels=8, sigma_v=0.0, sigma=None)
    assert check_cube_arguments(**ok) == ((-1.0, 1.0), 8, 0.0, None)
    assert check_cube_arguments(**(ok | {"v_range": None}))[0] is None
    out = check_cube_arguments(**(ok | {"sigma": [1.0] * 10, "sigma_v": 2}))
    assert out[2] == 2.0 and out[3].dtype == f32 and out[3].shape == (10,)
    # NaN, inf and negative values of sigma are the library's to drop, not an error
    check_cube_arguments(**(ok | {"sigma": [np.nan, np.inf, -1.0] + [0.0] * 7}))
    for bad in ((1.0, 1.0), (2.0, 1.0), (np.nan, 1.0), (0.0, np.inf), (1.0,), "ab", 5, (1.0, 2.0, 3.0)):
        with pytest.raises(ValueError, match="v_range must be None or"):
            check_cube_arguments(**(ok | {"v_range": bad}))
    for bad in (0, -1, 4097, 8.0, True, None, "8"):
        with pytest.raises(ValueError, match="n_channels must be an integer from 1 to 4096"):
            check_cube_arguments(**(ok | {"n_channels": bad}))
    with pytest.raises(ValueError, match="at most 2\\^31"):
        check_cube_arguments(**(ok | {"n_channels": 4096, "resolution": 1024}))
    check_cube_arguments(**(ok | {"n_channels": 2048, "resolution": 1024}))         # exactly 2^31
    for bad in (-1.0, np.nan, np.inf, "x", None):
        with pytest.raises(ValueError, match="sigma_v must be finite and >= 0"):
            check_cube_arguments(**(ok | {"sigma_v": bad}))
    for bad in ([1.0] * 9, np.zeros((10, 1)), 1.0):
        with pytest.raises(ValueError, match="sigma must have one value per particle"):
            check_cube_arguments(**(ok | {"sigma": bad}))


def test_spectral_cube_checks_its_arrays_before_it_needs_a_gpu():
    import topsy_amd
    pos = np.zeros((4, 3), dtype=f32)
    one = np.ones(4, dtype=f32)
    with pytest.raises(ValueError, match="vel is required"):
        topsy_amd.spectral_cube(pos, one, one, None)
    with pytest.raises(ValueError, match="n_channels must be"):
        topsy_amd.spectral_cube(pos, one, one, pos, n_channels=0)
    with pytest.raises(ValueError, match="v_ref must be"):
        topsy_amd.spectral_cube(pos, one, one, pos, v_ref="middle")
    with pytest.raises(ValueError, match="resolution must be"):
        topsy_amd.spectral_cube(pos, one, one, pos, resolution=0)
    assert topsy_amd.SpectralCube is topsy_amd.spectral.SpectralCube


def test_default_v_range():
    from topsy_amd.spectral import default_v_range
    vel = np.array([[0, 0, 30.0], [0, 0, -80.0], [0, 0, np.nan], [0, 0, np.inf]], dtype=f32)
    axis, zero = np.array([0.0, 0.0, 1.0]), np.zeros(3)
    assert default_v_range(vel, axis, zero, 0.0, None) == (-80.0, 80.0)
    assert default_v_range(vel, axis, np.array([0, 0, 20.0]), 0.0, None) == (-100.0, 100.0)
    assert default_v_range(vel, axis, zero, 3.0, np.array([4.0, np.nan, -7.0, 0.0], dtype=f32)) == (-105.0, 105.0)
    assert default_v_range(vel[2:], axis, zero, 0.0, None) == (-1.0, 1.0)
    assert default_v_range(vel[:0], axis, zero, 0.0, None) == (-1.0, 1.0)


# ---- the layout header ---------------------------------------------------------------------------------------------------------
TILE, BLOCK, LIST_CAPACITY, MAX_SLICE = 16, 32, 1 << 27, 1 << 22


def layout(n, R, C, option=0, has_sigma=False):
    from topsy_amd import _native
    return _native.spectral_cube_layout(n, R, C, option, has_sigma)


def check_carve(L, n, R, C, has_sigma):
    """regions in order, 256-byte aligned, none overlapping, each large enough for what the kernels index"""
    per, cap, bins = L["slice_particles"], L["list_capacity"], L["bins"]
    h = [("h_sigma", n * 4 if has_sigma else 0), ("h_geom", per * 16), ("h_line", per * 24), ("h_bytes", 0)]
    a = [("a_cube", C * R * R * 4), ("a_count", (per + 1) * 4), ("a_offset", (per + 1) * 4), ("a_keys", cap * 4),
         ("a_keys_sorted", cap * 4), ("a_index", cap * 4), ("a_index_sorted", cap * 4), ("a_bin_first", bins * 4),
         ("a_bin_end", bins * 4), ("a_tmp", 0), ("a_bytes", 0)]
    for regions in (h, a):
        assert L[regions[0][0]] == 0
        for (name, size), (following, _) in zip(regions, regions[1:]):
            assert L[name] % 256 == 0 and L[name] + size <= L[following], (name, L)


@pytest.mark.parametrize("C", [1, 32, 33, 4096])
@pytest.mark.parametrize("R", [1, 8, 15, 16, 17, 100, 128])
def test_layout_grid_and_carve(R, C):
    for n, option, has_sigma in ((0, 0, False), (1, 0, True), (1500, 0, False), (1500, 1, True), (1500, 256, True), (10 ** 7, 0, True)):
        L = layout(n, R, C, option, has_sigma)
        tiles, blocks = -(-R // TILE), -(-C // BLOCK)
        assert (L["tiles"], L["blocks"], L["bins"]) == (tiles, blocks, tiles * tiles * blocks)
        assert (1 << L["key_bits"]) >= L["bins"] and (L["key_bits"] == 1 or (1 << (L["key_bits"] - 1)) < L["bins"])
        per = L["slice_particles"]
        want = min(LIST_CAPACITY // L["bins"], MAX_SLICE)
        want = min(want, option) if option else want
        assert per == max(min(want, n), 1)
        assert L["slices"] == (0 if n == 0 else -(-n // per))
        assert L["slices"] * per >= n and (L["slices"] - 1) * per < max(n, 1)
        # a slice can never overflow its lists: a particle emits at most one pair per bin
        assert L["list_capacity"] == min(per * L["bins"], LIST_CAPACITY) and per * L["bins"] <= LIST_CAPACITY
        check_carve(L, n, R, C, has_sigma)


def test_layout_slices_at_the_list_bound():
    """R = 512 with 256 channels: 1024 tiles x 8 blocks; a slice is 2^27 / 2^13 = 16384 particles whatever n is (above it)"""
    L = layout(10 ** 7, 512, 256)
    assert L["bins"] == 8192 and L["slice_particles"] == 16384 and L["slices"] == 611 and L["list_capacity"] == LIST_CAPACITY
    assert layout(16384, 512, 256)["slices"] == 1 and layout(16385, 512, 256)["slices"] == 2
    assert layout(10 ** 7, 512, 256, option=100)["slice_particles"] == 100
    assert layout(10 ** 7, 512, 256, option=10 ** 9)["slice_particles"] == 16384          # the option only lowers it
    assert layout(2 ** 31 - 1, 16, 1)["slice_particles"] == MAX_SLICE                     # the record bound
    L = layout(5, 724, 4096)                 # the most bins a cube of 2^31 cells can have at 4096 channels
    assert L["bins"] == 46 * 46 * 128 and L["bins"] * 5 <= LIST_CAPACITY and L["slices"] == 1


def test_layout_refusals():
    from topsy_amd import _native
    for args in ((-1, 64, 8), (2 ** 31, 64, 8), (10, 0, 8), (10, 64, 0), (10, 64, 4097), (10, 1024, 2049)):
        with pytest.raises(_native.BackendError):
            layout(*args)
    with pytest.raises(_native.BackendError):
        layout(10, 64, 8, option=-1)
    layout(10, 1024, 2048)


def test_header_constants_match_the_binding():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "topsy_amd", "csrc", "tsp_cube_layout.h")).read()
    const = {k: v for k, v in re.findall(r"constexpr \w+ (\w+) = ([^;]+);", text)}
    assert int(const["TILE"]) == TILE and int(const["CHANNEL_BLOCK"]) == BLOCK and int(const["MAX_CHANNELS"]) == 4096
    assert const["LIST_CAPACITY"] == "1ll << 27" and const["MAX_SLICE_PARTICLES"] == "1ll << 22" and const["MAX_CELLS"] == "1ll << 31"
    from topsy_amd import _native
    assert _native.CUBE_MAX_CHANNELS == 4096 and _native.CUBE_MAX_CELLS == 1 << 31
    assert _native.load_library().tsp_version() >= 126
    public = open(os.path.join(root, "include", "topsy_splat.h")).read()
    assert f"#define TSP_CUBE_LAYOUT_VALUES {len(_native.CUBE_LAYOUT_NAMES)}" in public
    assert "#define TSP_CUBE_TILE 16" in public and "#define TSP_CUBE_CHANNEL_BLOCK 32" in public
