"""Kernel H2's row clip (option h2_chord) on the CPU: the row test of tsp_pipeline.h restated in NumPy float32 (h2_chord_ref.py).

A pixel row that the clip clears must be one whose every fragment is an exact zero: each of the strip's 64 columns is either outside
the footprint's square (its column factors are 0) or reads, with the row's two texel rows, four texels of the level-0 kernel image
that are exactly 0 wherever their interpolation weight is not (h2_chord_ref.texel_pairs).  And the rows it clears are a prefix and a
suffix of the square's rows in the strip, never a hole: both row walks of the kernel take the covered rows for contiguous."""
import numpy as np

import h2_chord_ref as ref
from topsy_amd import kernel_lut

f32 = np.float32
R = 1024


def _lut():
    return kernel_lut.kernel_mips()[:64 * 64].reshape(64, 64)


def _check_pair(lut, pcx, pcy, P, sx0, sy0, sh):
    """-> (covered rows, cleared rows) of the pair after checking both properties"""
    covered, cleared = ref.strip_rows(pcx, pcy, P, sx0, sy0, sh)
    kept = np.flatnonzero(covered & ~cleared)
    if len(kept):
        assert kept[-1] - kept[0] + 1 == len(kept), f"hole in the rows kept: P {P} centre ({pcx}, {pcy}) strip ({sx0}, {sy0}) x {sh}"
    if cleared.any():
        rows = (np.arange(sy0, sy0 + sh, dtype=f32) + f32(0.5))[cleared]
        cols = np.arange(sx0, sx0 + ref.SW, dtype=f32) + f32(0.5)
        r0, r1, fy, _ = ref.texel_pairs(rows, pcy, P)
        c0, c1, fx, cov_x = ref.texel_pairs(cols, pcx, P)
        c0, c1, fx = c0[cov_x], c1[cov_x], fx[cov_x]
        # (a texel whose interpolation weight is exactly 0 -- the second one where the clamp at the low edge sets the fraction to 0 --
        # contributes 0 x a finite texel: it may hold anything)
        for r, wy in ((r0, np.ones_like(fy)), (r1, fy)):
            for c, wx in ((c0, np.ones_like(fx)), (c1, fx)):
                read = lut[np.ix_(r, c)] * ((wy != 0)[:, None] & (wx != 0)[None, :])
                assert not read.any(), \
                    f"a cleared row reads a non-zero texel: P {P} centre ({pcx}, {pcy}) strip ({sx0}, {sy0}) x {sh}"
    return int(covered.sum()), int(cleared.sum())


def test_lut_is_zero_outside_the_disc():
    """what the library checks before it sets disc_k2 (lut_zero_outside_disc), level 0: texel centres at >= 2 h hold exact zeros"""
    lut = _lut()
    c = -2.0 + (np.arange(64) + 0.5) * 4.0 / 64
    outside = c[None, :] ** 2 + c[:, None] ** 2 >= 4.0
    assert outside.any() and not lut[outside].any()


def test_cleared_rows_read_only_zero_texels_and_leave_no_hole():
    lut = _lut()
    rs = np.random.RandomState(7)
    n_cov = n_clr = n_pairs = 0
    for sh in (32, 16):
        for _ in range(150):
            P = f32(np.exp(rs.uniform(np.log(64.0), np.log(2500.0))))
            pcx, pcy = f32(rs.uniform(-80.0, R + 80.0)), f32(rs.uniform(-80.0, R + 80.0))
            # every strip the kernel would keep for this footprint
            for sx0 in range(0, R, ref.SW):
                if ref.strip_dist(pcx, sx0, sx0 + ref.SW) >= f32(0.5) * P:
                    continue
                for sy0 in range(0, R, sh):
                    if not ref.reaches_strip(pcx, pcy, P, sx0, sy0, sh):
                        continue
                    cov, clr = _check_pair(lut, pcx, pcy, P, sx0, sy0, sh)
                    n_cov += cov; n_clr += clr; n_pairs += 1
    assert n_pairs > 10000 and n_cov > 0
    assert n_clr > 1000, (n_clr, n_cov)      # (the properties above were checked on cleared rows, not on none)


def test_widths_at_the_bilinear_threshold():
    """P = 64 ... 70: one texel row per pixel row; the margin of the disc constant is smallest in pixels here"""
    lut = _lut()
    rs = np.random.RandomState(8)
    for P in np.concatenate([np.linspace(64.0, 64.05, 11), np.linspace(64.1, 70.0, 9)]).astype(f32):
        for _ in range(40):
            pcx, pcy = f32(rs.uniform(0.0, 300.0)), f32(rs.uniform(0.0, 300.0))
            for sh in (32, 16):
                for sx0 in range(0, 320, ref.SW):
                    for sy0 in range(0, 320, sh):
                        if ref.reaches_strip(pcx, pcy, P, sx0, sy0, sh):
                            _check_pair(lut, pcx, pcy, P, sx0, sy0, sh)


def test_without_a_disc_nothing_is_cleared():
    """disc_k2 = 0 (fragment counting, or a kernel image that is not zero outside the disc): the limit is +inf"""
    covered, cleared = ref.strip_rows(f32(170.3), f32(140.2), f32(300.0), 0, 0, 32, k2=f32(0.0))
    assert covered.any() and not cleared.any()


def test_pinned_footprints_lose_every_row_of_a_strip_that_is_kept():
    """scene (c) of tests/test_gpu_h2_chord.py"""
    lut = _lut()
    P = f32(ref.EMPTIED_P)
    for cx, cy, sx0, sy0_32, sy0_16 in ref.EMPTIED:
        for sh, sy0 in ((32, sy0_32), (16, sy0_16)):
            assert ref.reaches_strip(f32(cx), f32(cy), P, sx0, sy0, sh)
            cov, clr = _check_pair(lut, f32(cx), f32(cy), P, sx0, sy0, sh)
            assert cov == sh and clr == sh
            # ... by a margin that the float32 rounding of the world-to-pixel transform (~1e-5 px) does not reach
            for ex in (-0.05, 0.05):
                for ey in (-0.05, 0.05):
                    assert ref.reaches_strip(f32(cx + ex), f32(cy + ey), P, sx0, sy0, sh)
                    covered, cleared = ref.strip_rows(f32(cx + ex), f32(cy + ey), P, sx0, sy0, sh)
                    assert covered.all() and cleared.all()
