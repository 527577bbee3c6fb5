"""Images smaller than one tile of the tile kernels (kernel N 16 x 16 / 16 x 32 strips, kernel G 64 x 16 / 64 x 32, kernel H2 tiles
of 2 x 2 strips of 64 x 16 / 64 x 32, the 64-row bands of the rgb counter's rectangle sums), with footprints of every class: a camera
zoomed into a small preview image.  Every frame against the oracle (tolerances: parity_scenes.render_and_check), the exact
fragment count included, the class counts asserted.  An image of at most 64 rows is one band of the huge-record bins, and
bin_huge_records (tsp_huge.hip) never bins a one-band image: kernel H2 scans the whole list there, however many records it holds;
the last test goes on to the smallest images that are binned."""
import numpy as np
import pytest

import parity_scenes as ps

pytestmark = pytest.mark.gpu

RESOLUTIONS = (1, 2, 3, 8, 15, 16, 17, 31, 33, 63)


@pytest.fixture(scope="module")
def native():
    from topsy_amd import _native
    _native.load_library()
    return _native


def camera(scale):
    from oracle import oracle_np
    return oracle_np.transform_matrix(ps._rot(0.2, 0.1), np.zeros(3), scale)


@pytest.mark.parametrize("mode", ps.MODES)
@pytest.mark.parametrize("R", RESOLUTIONS)
def test_every_class_on_an_image_below_one_tile(native, mips, R, mode):
    scene = ps.all_class_scene(R)
    n = len(scene["h"])
    M, sf = camera(scene["scale"])
    ctx = native.Context(R, 4 if mode == "rgb" else 2)
    try:
        ctx.set_kernel_mips(mips)
        ps.upload_scene(ctx, scene, mode)
        for narrow in (64000, 0, 24000):           # the mid list by kernel N, by kernel G, by both
            for count in (1, 0):
                ctx.set_option("mid_narrow_px_milli", narrow)
                _, st = ps.render_and_check(ctx, native, mode, scene, M, sf, R, mips, count, label=narrow)
                assert st["n_small"] > 0 and st["n_mid"] > 0 and st["n_huge"] > 0, st
                assert st["n_small"] + st["n_mid"] + st["n_huge"] + st["n_culled"] == n, st
        ctx.set_option("mid_narrow_px_milli", 64000)
        for count in (1, 0):                       # the generic kernel as a second opinion
            ps.render_and_check(ctx, native, mode, scene, M, sf, R, mips, count, flags=native.PIPE_GENERIC, label="generic")
        if mode == "density":                      # kernel H2's single-channel strip shapes / occupancies, both row walks
            for variant in (2, 4, 5, 6, 7):
                for walk in (0, 1):
                    for count in (1, 0):
                        ctx.set_option("huge_variant", variant); ctx.set_option("h2_walk", walk)
                        ps.render_and_check(ctx, native, mode, scene, M, sf, R, mips, count, label=(variant, walk))
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", ["weighted", "rgb"])
@pytest.mark.parametrize("R", [17, 65, 129])
def test_many_huge_records_on_one_two_and_three_bands(native, mips, R, mode):
    """More than 4096 huge records, the count from which kernel H2 reads them from 64-row band bins -- on an image of two bands and
    more.  R = 17 is one band: the whole list is scanned whatever option huge_band_mib says, and both settings must give the
    oracle's frame.  R = 65 (a last band of one row) and R = 129 (three bands, the last of one row) are binned at the default budget
    and scanned as one list with huge_band_mib = 0 (test_parity_scenes_cpu.py pins the band counts).  The rgb counter channel comes
    from the rectangle sums."""
    scene = ps.wide_scene(R)
    M, sf = camera(scene["scale"])
    ctx = native.Context(R, 4 if mode == "rgb" else 2)
    try:
        ctx.set_kernel_mips(mips)
        ps.upload_scene(ctx, scene, mode)
        for mib in (None, 0):                      # None: the library's default budget
            if mib is not None:
                ctx.set_option("huge_band_mib", mib)
            for count in (1, 0):
                _, st = ps.render_and_check(ctx, native, mode, scene, M, sf, R, mips, count, label=("huge_band_mib", mib))
                assert st["n_huge"] > 4096, st             # (the 64.0-px widths may round below the class boundary)
    finally:
        ctx.close()
