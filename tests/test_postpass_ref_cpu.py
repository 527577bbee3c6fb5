"""The periodic-tiling oracle against its float64 restatement (tests/postpass_ref.py), without a GPU: oracle_np.periodic_tile is
what tsp_tile_periodic must equal bit for bit (tests/test_gpu_postpass.py), so its own distance from exact arithmetic is pinned
here, by a bound that is derived and not measured (postpass_ref.tiling_bound)."""
import numpy as np
import pytest

import postpass_ref
from oracle import oracle_np

f32 = np.float32


def _rotation(seed):
    q, _ = np.linalg.qr(np.random.RandomState(seed).normal(size=(3, 3)))
    return q


@pytest.mark.parametrize("C", [2, 4])
@pytest.mark.parametrize("R", [1, 2, 33, 200, 257])
def test_oracle_tiling_within_the_float64_bound(R, C):
    rs = np.random.RandomState(R + C)
    img = (np.exp(rs.uniform(-30, 10, size=(R, R, C))) * rs.choice([-1.0, 1.0], size=(R, R, C))).astype(f32)
    worst = 0.0
    for rot in (np.eye(3), _rotation(1), _rotation(2)):
        for scale in (0.3, 100.0 / 130.0, 1.0, 2.5):
            off, w = oracle_np.periodic_instances(rot, scale)
            got = oracle_np.periodic_tile(img, off, w)
            total, A, count = postpass_ref.tile_periodic_f64(img, off, w)
            assert np.array_equal(count, postpass_ref.tile_inside_count(R, off))
            bound = postpass_ref.tiling_bound(A, count)
            err = np.abs(got.astype(np.float64) - total)
            assert (err <= bound).all(), (R, C, scale)
            assert (got[count == 0] == 0).all()
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    print(f"R={R} C={C}: the oracle reaches {worst:.3f} of the bound")


def test_oracle_tiling_by_whole_pixels():
    """+x in clip space moves the image to higher columns, +y to LOWER rows (up)"""
    R = 64
    img = np.exp(np.random.RandomState(0).uniform(-5, 5, size=(R, R, 2))).astype(f32)
    right = oracle_np.periodic_tile(img, [[2.0 * 3 / R, 0.0]], [1.0])
    assert np.array_equal(right[:, 3:], img[:, :-3]) and (right[:, :3] == 0).all()
    up = oracle_np.periodic_tile(img, [[0.0, 2.0 * 5 / R]], [1.0])
    assert np.array_equal(up[:-5], img[5:]) and (up[-5:] == 0).all()
    assert np.array_equal(postpass_ref.tile_touch_mask(R, [[0.0, 0.0]], (10, 20)).nonzero(), ([9, 9, 10, 10], [19, 20, 19, 20]))
