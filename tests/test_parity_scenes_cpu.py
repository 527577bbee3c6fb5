"""The conditions that give the GPU tests built on tests/parity_scenes.py their power, checked without a GPU: each LUT builder
has the two properties its name promises, the all-class scene really holds every footprint class at every resolution used,
its view holds (record, strip) pairs that only the exact corner culling drops, and an image rendered with lit corners is far
from one rendered without them.  Also the figures that docstrings of test_gpu_parity.py quote.
"""
import numpy as np
import pytest

import parity_scenes as ps
from conftest import make_cloud

SMALL_R = (1, 2, 3, 8, 15, 16, 17, 31, 33, 63)          # test_gpu_small_images.py
ALL_R = SMALL_R + (128, 200)                            # + test_gpu_resident_state.py, test_gpu_lut_contract.py

LUTS = {
    # name: (builder, (zero_outside_disc, mirror_symmetric), (left-right, top-bottom))
    "reference": (ps.reference, (True, True), (True, True)),
    "corner_lit_all": (lambda: ps.corner_lit((0, 1, 2, 3)), (False, True), (True, True)),
    "corner_lit_0": (lambda: ps.corner_lit((0,)), (False, True), (True, True)),
    "corner_lit_1": (lambda: ps.corner_lit((1,)), (False, True), (True, True)),
    "corner_lit_2": (lambda: ps.corner_lit((2,)), (False, True), (True, True)),
    "corner_lit_3": (lambda: ps.corner_lit((3,)), (False, True), (True, True)),
    "one_texel_lit": (ps.one_texel_lit, (False, False), (False, False)),
    "skew": (ps.skew, (True, False), (False, False)),
    "lr_only": (ps.lr_only, (True, False), (True, False)),
    "tb_only": (ps.tb_only, (True, False), (False, True)),
    "level3_asym": (ps.level3_asym, (True, False), (False, False)),
}


@pytest.mark.parametrize("name", list(LUTS))
def test_lut_builders_have_the_properties_they_are_named_for(name, mips):
    build, props, axes = LUTS[name]
    lut = build()
    assert lut.dtype == np.float32 and lut.shape == mips.shape
    assert ps.lut_properties(lut) == props
    assert ps.lut_mirror_axes(lut) == axes
    assert np.isfinite(lut).all() and (lut >= 0).all()
    differs = np.flatnonzero(lut.view(np.uint32) != mips.view(np.uint32))
    if name == "reference":
        assert differs.size == 0
    if name == "one_texel_lit":
        assert differs.size == 1 and differs[0] < 4096
    if name == "level3_asym":
        assert differs.size == 1 and differs[0] >= ps.MIP_OFFSETS[3]
    if name.startswith("corner_lit_") and name[-1].isdigit():      # only the named level changes
        l = int(name[-1])
        assert ((differs >= ps.MIP_OFFSETS[l]) & (differs < ps.MIP_OFFSETS[l] + ps.MIP_SIZES[l] ** 2)).all() and differs.size > 0


def test_builders_leave_the_shared_reference_lut_alone(mips):
    before = mips.copy()
    for build, _, _ in LUTS.values():
        build()
    assert np.array_equal(before.view(np.uint32), mips.view(np.uint32))


def test_skewed_reference_lut_keeps_zero_corners(mips):
    """what test_asymmetric_kernel_lut_uses_full_tables (test_gpu_parity.py) uploads: asymmetric, corners still exactly zero"""
    skew = mips.copy()
    skew *= (1.0 + 0.05 * np.random.RandomState(2).uniform(size=skew.shape)).astype(np.float32)
    assert ps.lut_properties(skew) == (True, False)
    assert np.array_equal(skew, ps.skew())


@pytest.mark.parametrize("R", ALL_R)
def test_all_class_scene_holds_every_class(R):
    for n in (1500, 3000):
        sc = ps.all_class_scene(R, n=n)
        nominal = ps.class_counts(sc["P"])
        assert min(nominal) >= 100
        if n == 1500:
            assert nominal == (604, 231, 665)
        # by the width the library works out from the float32 smoothing length (the boundary widths may round either way)
        seen = ps.class_counts(sc["h"].astype(np.float64) * 2.0 * R / sc["scale"])
        assert min(seen) >= 100 and max(abs(a - b) for a, b in zip(seen, nominal)) <= 12
        assert list(sc["P"][:24]) == ps.BOUNDARY_WIDTHS * 3
        px = 2 * sc["scale"] / R
        on_corner = sc["pos"][::7, :2] / np.float32(px)
        assert np.abs(on_corner - np.round(on_corner)).max() < 1e-3


def test_wide_scene_and_the_bands_of_its_images():
    """bin_huge_records (tsp_huge.hip) bins from 4096 huge records on, and only an image of two bands (HBAND_H = 64 rows) or more:
    R = 17 is never binned, R = 65 and 129 are -- with a last band of one row"""
    for R, n_bands, last_rows in ((17, 1, 17), (65, 2, 1), (129, 3, 1)):
        sc = ps.wide_scene(R)
        assert len(sc["h"]) == 6000 and sc["P"].min() >= 64.0 and sc["P"].max() <= 3000.0
        assert -(-R // 64) == n_bands and R - 64 * (n_bands - 1) == last_rows


def test_tiny_resolution_cloud_of_the_parity_suite():
    """test_tiny_and_odd_resolutions (test_gpu_parity.py): what its cloud reaches at each resolution, by width"""
    _, h, _, _, _ = make_cloud(3000, seed=21)
    P = {R: 2.0 * h.astype(np.float64) * R / 90.0 for R in (1, 2, 8, 33, 65)}
    assert 1.3 < P[1].max() < 1.4 and 2.6 < P[2].max() < 2.7 and 10.6 < P[8].max() < 10.7
    for R in (1, 2, 8):
        assert ps.class_counts(P[R]) == (3000, 0, 0)
    assert ps.class_counts(P[33]) == (2617, 383, 0)
    assert ps.class_counts(P[65]) == (2358, 522, 120)


def _culled_only_pairs(pcx, pcy, P, sel, R, w, hgt):
    """(record, strip) pairs over the w x hgt strips of an R^2 image that the footprint square reaches and the disc of radius
    0.5235 P does not: reaches_strip (tsp_pipeline.h) restated in float64, with disc_k2 = 0 and with disc_k2 = 0.5235^2"""
    x0 = np.arange(-(-R // w), dtype=np.float64) * w
    y0 = np.arange(-(-R // hgt), dtype=np.float64) * hgt
    n = 0
    for p in np.flatnonzero(sel):
        sdx = np.maximum(np.maximum(x0 - pcx[p], pcx[p] - (x0 + w)), 0.0)[None, :]
        sdy = np.maximum(np.maximum(y0 - pcy[p], pcy[p] - (y0 + hgt)), 0.0)[:, None]
        half = 0.5 * P[p]
        square = (sdx < half) & (sdy < half)
        disc = sdx * sdx + sdy * sdy < 0.5235 * 0.5235 * P[p] * P[p]
        n += int((square & ~disc).sum())
    return n


def test_lut_contract_view_holds_pairs_only_the_disc_culling_drops():
    """Strip shapes (columns x rows) as the code has them: kernel N 16 (NSW, tsp_mid.hip) x HR, kernel G 64 x HR, with HR = 32
    (TSP_G_HR1) for density and 16 for two and more channels; kernel H2 64 x 32 and 64 x 16 for density (launch_gather_mode,
    tsp_huge.hip: huge_variant 2 / 6 / 7 and 4 / 5 / default), 64 x 16 otherwise.  Kernels N and G draw the mid list: every footprint
    below 64 px once p_small_milli = 0; kernel H2 the ones from 64 px on.  A culling switched on for a LUT with lit corners
    would drop exactly these pairs."""
    R = 200
    sc = ps.all_class_scene(R)
    M, sf = ps.lut_contract_camera(sc["scale"])
    # the projection in the canonical float32 operation order (oracle_np's docstring) that the kernels share; the test itself in float64
    f32 = np.float32
    Mf = np.asarray(M, dtype=f32).reshape(4, 4)
    x, y, z = (sc["pos"][:, k] for k in range(3))
    cx, cy, cz = (((Mf[r, 0] * x + Mf[r, 1] * y) + Mf[r, 2] * z) + Mf[r, 3] for r in range(3))
    P = ((f32(sf) * sc["h"]) * f32(2.0)) * f32(R)
    pcx, pcy = (cx + f32(1.0)) * f32(R / 2.0), (f32(1.0) - cy) * f32(R / 2.0)
    assert all(a.dtype == f32 for a in (cz, P, pcx, pcy))
    keep = (cz >= 0) & (cz <= 1)
    pcx, pcy, P = (a.astype(np.float64) for a in (pcx, pcy, P))
    mid, huge = keep & (P < 64.0), keep & (P >= 64.0)
    counts = {
        "N 16x32": _culled_only_pairs(pcx, pcy, P, mid, R, 16, 32),
        "G 64x32": _culled_only_pairs(pcx, pcy, P, mid, R, 64, 32),
        "H2 64x32": _culled_only_pairs(pcx, pcy, P, huge, R, 64, 32),
        "H2 64x16": _culled_only_pairs(pcx, pcy, P, huge, R, 64, 16),
        "N 16x16": _culled_only_pairs(pcx, pcy, P, mid, R, 16, 16),
        "G 64x16": _culled_only_pairs(pcx, pcy, P, mid, R, 64, 16),
    }
    assert all(v >= 20 for v in counts.values()), counts
    assert counts == {"N 16x32": 69, "G 64x32": 22, "H2 64x32": 181, "H2 64x16": 369, "N 16x16": 134, "G 64x16": 39}      # (what docstrings and the commit quote)


@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_lit_corners_change_the_oracle_image(level, mips):
    """a render that ignored the corners of one level cannot pass the 1e-5 comparison: > 1000 pixels differ by more than that"""
    R = 200
    sc = ps.all_class_scene(R)
    M, sf = ps.lut_contract_camera(sc["scale"])
    ref, nfrag_ref, _ = ps.oracle_images("density", sc, M, sf, R, mips)
    lit, nfrag_lit, _ = ps.oracle_images("density", sc, M, sf, R, ps.corner_lit((level,)))
    assert nfrag_lit == nfrag_ref                       # coverage does not depend on the LUT
    a, b = ref[..., 0].astype(np.float64), lit[..., 0].astype(np.float64)
    differ = int((np.abs(a - b) > 1e-5 * np.abs(a)).sum())
    assert differ > 1000, differ                        # (40000 / 14654 / 3791 / 1146 for level 0 .. 3)


def test_oracle_images_are_shared_and_read_only(mips):
    sc = ps.all_class_scene(8)
    from oracle import oracle_np
    M, sf = oracle_np.transform_matrix(np.eye(3), np.zeros(3), sc["scale"])
    a = ps.oracle_images("weighted", sc, M, sf, 8, mips)
    b = ps.oracle_images("weighted", dict(sc), M, sf, 8, mips.copy())
    assert a[0] is b[0] and not a[0].flags.writeable and not a[2].flags.writeable
    c = ps.oracle_images("weighted", dict(sc, q=-sc["q"]), M, sf, 8, mips)
    assert c[0] is not a[0] and np.array_equal(c[0][..., 1], -a[0][..., 1]) and np.array_equal(c[2], a[2])
