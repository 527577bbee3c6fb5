"""The kinematic maps without a GPU: the numpy restatement of the weight and moment arithmetic (kinematics_ref.py) on hand
cases, and the range rules and argument checks of topsy_amd.kinematics that need no device."""
import inspect
import os
import re

import numpy as np
import pytest

import kinematics_ref as ref
from topsy_amd import kinematics

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------- weights
def test_constant_velocity_equal_to_v_ref_gives_exact_zeros():
    n = 50
    v0 = np.array([123.456, -78.9, 0.125], dtype=f32)
    vel = np.tile(v0, (n, 1))
    m = np.linspace(0.5, 2.0, n).astype(f32)
    axis = np.array([0.6, 0.0, 0.8], dtype=f32)
    r, g, b, u = ref.kinematic_colours(m, vel, axis, v0)
    assert (u == 0).all() and (g == 0).all() and (b == 0).all()
    assert np.array_equal(r, m)
    assert not np.signbit(g).any() and not np.signbit(b).any()


def test_integer_lattice_is_exact():
    """integer masses and velocities along an axis of the lattice: m u and m u^2 are exact in float32, and so are the weights
    with h a power of two"""
    ux = np.arange(-20, 21)
    m = np.arange(1, 42)
    vel = np.stack([ux + 7, 3 * ux, -ux], axis=1).astype(f32)
    h = np.full(len(m), 0.5, dtype=f32)
    for k, axis in enumerate(np.eye(3, dtype=f32)):
        v_ref = np.array([7.0, 0.0, 0.0], dtype=f32)
        u_want = (vel[:, k].astype(np.int64) - int(v_ref[k]))
        r, g, b, u = ref.kinematic_colours(m, vel, axis, v_ref)
        assert np.array_equal(u, u_want) and np.array_equal(r, m)
        assert np.array_equal(g, m * u_want) and np.array_equal(b, m * u_want * u_want)
        wr, wg, wb = ref.kinematic_weights(h, m, vel, axis, v_ref)
        assert np.array_equal(wr, 4 * m) and np.array_equal(wg, 4 * m * u_want) and np.array_equal(wb, 4 * m * u_want ** 2)


def test_operation_order_is_the_headers():
    """u sums its three products left to right, each product rounded to float32: a case where another order differs"""
    axis = np.array([1.0, 1.0, 1.0], dtype=f32)       # (the restatement does not ask for a unit axis)
    vel = np.array([[1e8, 1.0, -1e8]], dtype=f32)
    _, _, _, u = ref.kinematic_colours(np.ones(1, dtype=f32), vel, axis, np.zeros(3))
    assert u[0] == 0.0        # (1e8 + 1) rounds to 1e8 first; (1e8 + -1e8) + 1 would give 1


def test_nonfinite_mass_or_velocity_gives_zero_weights():
    m = np.array([1.0, np.nan, np.inf, 1.0, 1.0, 1.0, 2.0], dtype=f32)
    vel = np.zeros((7, 3), dtype=f32)
    vel[3, 0], vel[4, 1], vel[5, 2] = np.nan, np.inf, -np.inf
    vel[6] = (1.0, 2.0, 3.0)
    axis = np.array([1.0, 1.0, 1.0], dtype=f32) / f32(np.sqrt(3.0))
    h = np.full(7, 2.0, dtype=f32)
    wr, wg, wb = ref.kinematic_weights(h, m, vel, axis, np.zeros(3))
    for w in (wr, wg, wb):
        assert (w[1:6] == 0).all() and not np.signbit(w[1:6]).any()
    assert wr[0] == 0.25 and wg[0] == 0 and wb[0] == 0
    assert wr[6] == 0.5 and np.isfinite(wg[6]) and wg[6] > 0 and wb[6] > 0
    # a velocity component the axis does not see still kills the particle only through u: inf * 0 is NaN
    wr2, _, _ = ref.kinematic_weights(h, m, vel, np.array([1.0, 0.0, 0.0], dtype=f32), np.zeros(3))
    assert wr2[4] == 0 and wr2[5] == 0


def test_weights_divide_by_h_squared_as_the_oracle_does():
    """the restatement and oracle_np form rgb / (h * h): one product, one division (not rgb / h / h, not rgb * (1 / hh))"""
    from oracle import oracle_np
    src = inspect.getsource(oracle_np)
    assert re.search(r"rgb\[p, c\]\.astype\(f32\) / hh\[p\]", src) and re.search(r"hh = h \* h", src)
    rs = np.random.RandomState(3)
    h = np.exp(rs.uniform(-3, 3, 1000)).astype(f32)
    m = rs.uniform(0.5, 2.0, 1000).astype(f32)
    vel = rs.normal(0, 100, (1000, 3)).astype(f32)
    axis = np.array([0.0, 0.6, 0.8], dtype=f32)
    r, g, b, _ = ref.kinematic_colours(m, vel, axis, np.zeros(3))
    wr, wg, wb = ref.kinematic_weights(h, m, vel, axis, np.zeros(3))
    hh = h * h
    assert np.array_equal(wr, r / hh) and np.array_equal(wg, g / hh) and np.array_equal(wb, b / hh)
    assert not np.array_equal(wg, (g / h) / h)      # (the other form differs somewhere in 1000 draws)


# --------------------------------------------------------------------------- moments
def test_moments_of_hand_cases():
    img = np.zeros((8, 4), dtype=f32)
    img[0] = (2.0, 6.0, 26.0, 5.0)          # mean 3, var 13 - 9 = 4
    img[1] = (0.0, 1.0, 1.0, 2.0)           # S = 0
    img[2] = (-1.0, 1.0, 1.0, 1.0)          # S < 0
    img[3] = (np.nan, 1.0, 1.0, 1.0)
    img[4] = (1.0, np.nan, 1.0, 1.0)
    img[5] = (1.0, 1.0, np.inf, 1.0)
    img[6] = (1.0, 3.0, 8.0, 7.0)           # B / S = 8 < mean^2 = 9: clamped
    img[7] = (np.inf, 1.0, 1.0, 1.0)
    out = ref.velocity_moments(img)
    assert np.array_equal(out[:, 0], img[:, 0], equal_nan=True) and np.array_equal(out[:, 3], img[:, 3])
    assert out[0, 1] == 3.0 and out[0, 2] == 2.0
    assert np.isnan(out[[1, 2, 3, 4, 5, 7], 1:3]).all()
    assert out[6, 1] == 3.0 and out[6, 2] == 0.0
    assert out.dtype == f32
    assert (out[[1, 2, 3, 4, 5, 7], 1].view(np.uint32) == 0x7FC00000).all()


def test_moments_round_once_from_float64():
    S, A, B = f32(3.0), f32(1.0), f32(1.0)
    out = ref.velocity_moments(np.array([[S, A, B, 0.0]], dtype=f32))
    mean = 1.0 / 3.0
    assert out[0, 1] == f32(mean) and out[0, 2] == f32(np.sqrt(1.0 / 3.0 - mean * mean))


# --------------------------------------------------------------------------- ranges
def test_v_los_range_is_symmetric_at_the_99th_percentile_of_the_finite_pixels():
    v = np.linspace(-50.0, 200.0, 1001).astype(f32).reshape(7, 143)
    v[0, :5] = np.nan
    v[1, 0] = np.inf
    lo, hi = kinematics.v_los_range(v)
    fin = np.abs(v[np.isfinite(v)].astype(np.float64))
    assert hi == np.percentile(fin, 99.0) and lo == -hi
    assert kinematics.v_los_range(np.full((4, 4), np.nan)) == (-1.0, 1.0)
    assert kinematics.v_los_range(np.zeros((4, 4))) == (-1.0, 1.0)


def test_sigma_los_range_is_the_1st_to_99th_percentile():
    s = np.random.RandomState(1).uniform(0, 80, (32, 32)).astype(f32)
    s[3, 3] = np.nan
    lo, hi = kinematics.sigma_los_range(s)
    fin = s[np.isfinite(s)].astype(np.float64)
    assert (lo, hi) == tuple(np.percentile(fin, [1.0, 99.0]))
    assert kinematics.sigma_los_range(np.full(5, np.nan)) == (0.0, 1.0)
    assert kinematics.sigma_los_range(np.full(5, 3.0)) == (3.0, 4.0)


def test_set_ends_override_the_rules():
    v = np.linspace(-10, 30, 100)
    assert kinematics.resolve_range("v_los", v, None, None) == kinematics.v_los_range(v)
    assert kinematics.resolve_range("v_los", v, None, 12.0) == (-12.0, 12.0)
    assert kinematics.resolve_range("v_los", v, -5.0, None) == (-5.0, 5.0)
    assert kinematics.resolve_range("v_los", None, -5.0, 7.0) == (-5.0, 7.0)
    lo, hi = kinematics.sigma_los_range(v)
    assert kinematics.resolve_range("sigma_los", v, None, 100.0) == (lo, 100.0)
    assert kinematics.resolve_range("sigma_los", v, 2.0, None) == (2.0, hi)
    with pytest.raises(ValueError):
        kinematics.resolve_range("speed", v)
    with pytest.raises(ValueError):
        kinematics.resolve_range("v_los", v, 0.0, np.inf)


# --------------------------------------------------------------------------- arguments
def test_v_ref_forms():
    assert kinematics.check_v_ref("center") == "center"
    assert np.array_equal(kinematics.check_v_ref(None), np.zeros(3))
    assert np.array_equal(kinematics.check_v_ref([1, 2, 3]), [1.0, 2.0, 3.0])
    for bad in ("centre", [1, 2], [1, 2, np.nan], [[1, 2, 3]], object()):
        with pytest.raises(ValueError):
            kinematics.check_v_ref(bad)


class _FakeContext:
    n_gpus = 1


class _FakeVis:
    def __init__(self, loader, n_gpus=1, periodic=False):
        self.data_loader = loader
        self._periodic_tiling = periodic
        self.particle_buffers = type("PB", (), {})()
        self.particle_buffers.context = _FakeContext()
        self.particle_buffers.context.n_gpus = n_gpus


def test_view_refuses_what_it_cannot_draw_before_touching_a_device():
    from topsy_amd import loader
    no_vel = loader.TestDataLoader(None, 100)
    with pytest.raises(ValueError, match="no velocities"):
        kinematics.VelocityView(_FakeVis(no_vel))
    with_vel = type("L", (), {"get_velocities": lambda self: np.zeros((3, 3), dtype=f32)})()
    with pytest.raises(NotImplementedError, match="one GPU"):
        kinematics.VelocityView(_FakeVis(with_vel, n_gpus=2))
    with pytest.raises(NotImplementedError, match="periodic"):
        kinematics.VelocityView(_FakeVis(with_vel, periodic=True))
    with pytest.raises(ValueError, match="v_ref"):
        kinematics.VelocityView(_FakeVis(with_vel), v_ref="middle")
    with pytest.raises(ValueError, match="unknown parameter"):
        kinematics.VelocityView(_FakeVis(with_vel), v_ref=None, vmax=3.0)


def test_velocity_maps_checks_its_arrays_before_touching_a_device():
    pos = np.zeros((10, 3), dtype=f32)
    h, m, vel = np.ones(10, dtype=f32), np.ones(10, dtype=f32), np.zeros((10, 3), dtype=f32)
    ok = dict(rotation=None, center=(0, 0, 0), scale=10.0, resolution=64)
    kinematics.check_maps_arguments(pos, h, m, vel, **ok)
    for change, exc in ((dict(scale=0.0), "scale"), (dict(scale=np.nan), "scale"), (dict(resolution=0), "resolution"),
                        (dict(resolution=64.5), "resolution"), (dict(center=(0, 0)), "center"),
                        (dict(rotation=np.ones((3, 3))), "orthonormal")):
        with pytest.raises(ValueError, match=exc):
            kinematics.check_maps_arguments(pos, h, m, vel, **(ok | change))
    with pytest.raises(ValueError, match="vel"):
        kinematics.check_maps_arguments(pos, h, m, None, **ok)
    with pytest.raises(ValueError, match="vel"):
        kinematics.check_maps_arguments(pos, h, m, vel[:5], **ok)
    with pytest.raises(ValueError, match="smooth"):
        kinematics.check_maps_arguments(pos, h[:5], m, vel, **ok)


def test_binding_declares_the_kinematic_entry_points():
    from topsy_amd import _native
    assert _native.MODE_KINEMATIC == 3
    for name in ("tsp_upload_velocities", "tsp_set_line_of_sight", "tsp_velocity_moments", "tsp_colormap_moment"):
        assert name in _native.SIGNATURES
    header = open(os.path.join(ROOT, "include", "topsy_splat.h")).read()
    assert re.search(r"TSP_MODE_KINEMATIC\s*=\s*3", header)
    for name in ("upload_velocities", "set_line_of_sight", "velocity_moments", "colormap_moment"):
        assert callable(getattr(_native.Context, name))
    assert " * 117: kinematic maps" in header and "6e-8" in header
    assert _native.load_library().tsp_version() >= 117
