"""What tsp_set_kernel_mips derives from the uploaded LUT, seen through rendered frames: exact corner culling in kernels N, G
and H2 only for a LUT that is zero outside the inscribed disc, kernel G's one-quadrant table only for a LUT with both mirror
symmetries.  Every frame is compared with the oracle fed the same LUT (tolerances: parity_scenes.render_and_check).

The scene holds every footprint class at R = 200 (partial tiles on both axes); test_parity_scenes_cpu.py counts the (record,
strip) pairs of this view that a wrongly enabled culling would drop, per kernel, and shows that lit corners on any one level move
more than 1000 pixels of the oracle image beyond the tolerance."""
import numpy as np
import pytest

import parity_scenes as ps

pytestmark = pytest.mark.gpu

R = 200
LUTS = {
    "reference": ps.reference,
    "corner_lit_all": lambda: ps.corner_lit((0, 1, 2, 3)),
    "corner_lit_0": lambda: ps.corner_lit((0,)),
    "corner_lit_3": lambda: ps.corner_lit((3,)),
    "one_texel_lit": ps.one_texel_lit,
    "skew": ps.skew,
    "lr_only": ps.lr_only,
    "tb_only": ps.tb_only,
    "level3_asym": ps.level3_asym,
}


@pytest.fixture(scope="module")
def native():
    from topsy_amd import _native
    _native.load_library()
    return _native


@pytest.fixture(scope="module")
def scene():
    return ps.all_class_scene(R)


@pytest.mark.parametrize("mode", ps.MODES)
@pytest.mark.parametrize("lut_name", list(LUTS))
def test_frames_follow_the_uploaded_lut(native, scene, lut_name, mode):
    """count_fragments 1 (no culling) and 0 (culling when the LUT allows it); the mid list by kernel N or by kernel G; with
    p_small_milli = 0 the footprints of mip levels 2 and 3 reach kernels N and G as well."""
    lut = LUTS[lut_name]()
    M, sf = ps.lut_contract_camera(scene["scale"])
    ctx = native.Context(R, 4 if mode == "rgb" else 2)
    try:
        ctx.set_kernel_mips(lut)
        ps.upload_scene(ctx, scene, mode)
        for p_small in (None, 0):                  # None: the library's default, the option untouched
            if p_small is not None:
                ctx.set_option("p_small_milli", p_small)
            for narrow in (64000, 0):
                for count in (1, 0):
                    ctx.set_option("mid_narrow_px_milli", narrow)
                    _, st = ps.render_and_check(ctx, native, mode, scene, M, sf, R, lut, count, label=(lut_name, p_small, narrow))
                    assert st["n_mid"] > 0 and st["n_huge"] > 0, st
                    if p_small is None:
                        assert st["n_small"] > 0, st
                    else:
                        assert st["n_small"] == 0, st
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", ps.MODES)
def test_flags_follow_the_latest_upload(native, scene, mode):
    """reference -> lit corners -> reference on one context: each frame is the one of the LUT set last"""
    M, sf = ps.lut_contract_camera(scene["scale"])
    ref, lit = ps.reference(), ps.corner_lit((0, 1, 2, 3))
    ctx = native.Context(R, 4 if mode == "rgb" else 2)
    try:
        ps.upload_scene(ctx, scene, mode)
        frames = []
        for name, lut in (("reference", ref), ("corner_lit_all", lit), ("reference again", ref)):
            ctx.set_kernel_mips(lut)
            for narrow in (64000, 0):
                ctx.set_option("mid_narrow_px_milli", narrow)
                got, _ = ps.render_and_check(ctx, native, mode, scene, M, sf, R, lut, 0, label=(name, narrow))
            frames.append(got[..., 0].astype(np.float64))
            ps.render_and_check(ctx, native, mode, scene, M, sf, R, lut, 1, label=name)
        assert (np.abs(frames[1] - frames[0]) > 1e-5 * np.abs(frames[0])).sum() > 1000
        assert np.allclose(frames[2], frames[0], rtol=1e-5, atol=0)
    finally:
        ctx.close()
