"""tsp_gravity_direct on the GPU against the float64 model (gravity_ref.py).

Every comparison is |got - want| <= K * 2^-24 * sum_j |term_ij| per output component, K = TSP_GRAVITY_ERROR_K of the header
(the kernel's own rounding account); each test prints the worst ratio |got - want| / (2^-24 * scale) it met."""
import ctypes

import numpy as np
import pytest

import gravity_ref
from test_gpu_scratch_alloc_failure import Outputs, assert_same_state, frame_ctx, native, snapshot, walk      # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

f32 = np.float32
U = 2.0 ** -24
EINVAL = -1
_fp = ctypes.POINTER(ctypes.c_float)
_dp = ctypes.POINTER(ctypes.c_double)


def P(a, kind=_fp):
    return None if a is None else a.ctypes.data_as(kind)


def cols(a):
    return [np.ascontiguousarray(a[:, k], dtype=f32) for k in range(3)]


def scene(n_src, n_tgt, seed=3):
    """clustered plus uniform sources about 100 box units from the origin, masses over two decades, eps log-uniform in
    [1e-3, 1]; targets among and around them"""
    rs = np.random.RandomState(seed)
    src = rs.uniform(0.0, 25.0, size=(n_src, 3))
    k = n_src // 3
    src[:k] = rs.normal(size=(k, 3)) * 0.3 + rs.randint(0, 2, size=(k, 3)) * 20.0 + 2.5
    src = (src + np.array([100.0, -100.0, 100.0])).astype(f32)
    mass = (10.0 ** rs.uniform(-1.0, 1.0, n_src)).astype(f32)
    eps = (10.0 ** rs.uniform(-3.0, 0.0, n_src)).astype(f32)
    tgt = rs.uniform(-2.0, 27.0, size=(n_tgt, 3))
    m = min(n_tgt // 2, n_src)
    tgt[:m] = src[:m] + rs.normal(size=(m, 3)) * 0.05            # half of them close to a source
    tgt[m:] += np.array([100.0, -100.0, 100.0])
    return src, mass, eps, tgt.astype(f32)


@pytest.fixture(scope="module")
def ctx(native):
    c = native.Context(16, 2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def K(native):
    return native.GRAVITY_ERROR_K


def run(ctx, src, mass, eps, tgt=None, **kw):
    return ctx.gravity_direct(*cols(src), mass, eps, targets=None if tgt is None else cols(tgt), **kw)


def check(got_pot, got_acc, ref, K, what):
    worst = gravity_ref.worst_ratio(got_pot, got_acc, ref)
    print(f"\n{what}: worst |got - want| / (2^-24 scale) = {worst:.3f} (bound {K})")
    assert worst <= K, f"{what}: {worst} > {K}"
    return worst


# ---- 1. size edges ------------------------------------------------------------------------------------------------------------------
def test_size_edges(native, ctx, K):
    T, B = native.GRAVITY_SOURCE_TILE, native.GRAVITY_TARGETS_PER_WORKGROUP
    n_srcs = [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 7]
    n_tgts = [1, 63, 65, B - 1, B, B + 1]
    src, mass, eps, tgt = scene(max(n_srcs), max(n_tgts))
    worst = 0.0
    for n_src in n_srcs:
        ref = gravity_ref.direct_sum(src[:n_src], mass[:n_src], eps[:n_src], tgt)      # a target's sums do not depend on the others
        for n_tgt in n_tgts:
            pot, acc, info = run(ctx, src[:n_src], mass[:n_src], eps[:n_src], tgt[:n_tgt])
            assert info == {"n_valid_sources": n_src, "n_valid_targets": n_tgt}
            part = {k: v[:n_tgt] for k, v in ref.items() if isinstance(v, np.ndarray)}
            worst = max(worst, check(pot, acc, part, K, f"{n_src} sources x {n_tgt} targets"))
    print(f"\nsize edges: worst ratio {worst:.3f}")


# ---- 2. every source is read exactly once -------------------------------------------------------------------------------------------
def test_every_source_counts_once(native, ctx):
    T = native.GRAVITY_SOURCE_TILE
    worst = 0.0
    for n in (T + 1, 2 * T + 7):
        src, _, eps, tgt = scene(n, 70, seed=9)
        for j in (0, 63, 64, T - 1, T, n - 1):
            mass = np.zeros(n, dtype=f32)
            mass[j] = 3.0
            pot, acc, _ = run(ctx, src, mass, eps, tgt)
            d = tgt.astype(np.float64) - src[j].astype(np.float64)
            r2 = (d * d).sum(axis=1) + float(eps[j]) ** 2
            want_pot = -3.0 / np.sqrt(r2)
            want_acc = -3.0 * r2[:, None] ** -1.5 * d
            ratio = max(np.abs(pot / want_pot - 1.0).max(), np.abs(acc / want_acc - 1.0).max()) / U
            worst = max(worst, ratio)
            assert ratio <= 32, f"n = {n}, the one massive source {j}: {ratio} x 2^-24 from the single-pair value"
    print(f"\nsingle pairs: worst relative error {worst:.3f} x 2^-24 (bound 32)")


# ---- 3. targets = sources -----------------------------------------------------------------------------------------------------------
def test_targets_are_the_sources(native, ctx, K):
    T = native.GRAVITY_SOURCE_TILE
    n = 2 * T + 7
    src, mass, eps, _ = scene(n, 1, seed=4)
    src[700] = src[5]                      # two coincident particles, eps > 0: they see each other
    src[T] = src[T - 1]                    # ... across a tile edge
    pot, acc, info = run(ctx, src, mass, eps)
    ref = gravity_ref.direct_sum(src, mass, eps)
    assert info == {"n_valid_sources": n, "n_valid_targets": n}
    check(pot, acc, ref, K, "targets = sources")
    # the self pair would be m / eps, far above the bound, at every particle: also at the tile edges
    for i in (0, T - 1, T, 2 * T - 1, 2 * T, n - 1):
        assert mass[i] / eps[i] > 100 * K * U * ref["pot_scale"][i]
    assert pot[5] < -mass[700] / eps[700] * (1 - 1e-6)           # the coincident partner is there
    # eps = 0 and coincidence: that pair contributes nothing, every output is finite
    pot0, acc0, _ = run(ctx, src, mass, 0.0)
    assert np.isfinite(pot0).all() and np.isfinite(acc0).all()
    check(pot0, acc0, gravity_ref.direct_sum(src, mass, 0.0), K, "targets = sources, eps = 0")
    # explicit targets at the sources' places with eps = 0: the pair at distance 0 contributes nothing either
    pot1, acc1, _ = run(ctx, src, mass, 0.0, src[:100])
    assert np.isfinite(pot1).all() and np.isfinite(acc1).all()
    check(pot1, acc1, gravity_ref.direct_sum(src, mass, 0.0, src[:100]), K, "targets on sources, eps = 0")


# ---- 4. few targets, many sources ---------------------------------------------------------------------------------------------------
def test_few_targets_many_sources(ctx, K):
    src, mass, eps, tgt = scene(200_000, 4, seed=6)
    pot, acc, info = run(ctx, src, mass, eps, tgt)
    assert info == {"n_valid_sources": 200_000, "n_valid_targets": 4}
    check(pot, acc, gravity_ref.direct_sum(src, mass, eps, tgt, block=4), K, "4 targets x 200000 sources")
    # one target workgroup either way: the split of the sources is the same, and so are the bits (the header's contract)
    pot2, acc2, _ = run(ctx, src, mass, eps, tgt[:2])
    assert np.array_equal(pot2.view(np.uint64), pot[:2].view(np.uint64))
    assert np.array_equal(acc2.view(np.uint64), acc[:2].view(np.uint64))


# ---- 5. validity --------------------------------------------------------------------------------------------------------------------
def test_validity(ctx, K):
    src, mass, eps, tgt = scene(1500, 300, seed=7)
    bad = {"x": (10, np.nan), "y": (200, np.inf), "z": (511, -np.inf), "m": (512, np.nan), "m2": (900, np.inf), "e": (1400, np.nan),
           "e2": (63, np.inf)}
    src[10, 0], src[200, 1], src[511, 2] = np.nan, np.inf, -np.inf
    mass[512], mass[900] = np.nan, np.inf
    eps[1400], eps[63] = np.nan, np.inf
    mass[[0, 64, 1499]] = 0.0                               # massless sources take part and are harmless
    tgt[[0, 100, 299], [0, 1, 2]] = [np.nan, np.inf, -np.inf]
    pot, acc, info = run(ctx, src, mass, eps, tgt)
    ref = gravity_ref.direct_sum(src, mass, eps, tgt)
    assert ref["n_valid_sources"] == 1500 - len(bad) and ref["n_valid_targets"] == 297
    assert info == {"n_valid_sources": ref["n_valid_sources"], "n_valid_targets": ref["n_valid_targets"]}
    assert np.isnan(pot[[0, 100, 299]]).all() and np.isnan(acc[[0, 100, 299]]).all()
    check(pot, acc, ref, K, "non-finite sources and targets")
    # targets = sources: a source left out for its mass or eps is still a target; one with a bad coordinate gets NaN
    pot, acc, info = run(ctx, src, mass, eps)
    ref = gravity_ref.direct_sum(src, mass, eps)
    assert info == {"n_valid_sources": 1500 - len(bad), "n_valid_targets": 1497}
    assert np.isnan(pot[[10, 200, 511]]).all() and np.isfinite(pot[[512, 900, 1400, 63]]).all()
    check(pot, acc, ref, K, "non-finite sources, targets = sources")


# ---- 6, 7, 8. the forms of one call ---------------------------------------------------------------------------------------------------
def bits(a):
    return a.view(np.uint64)


def test_forms_of_one_call_agree_bit_for_bit(ctx):
    src, mass, _, tgt = scene(1100, 600, seed=8)
    eps_all = float(f32(0.037))
    pot, acc, _ = run(ctx, src, mass, eps_all, tgt)
    # 6. a scalar eps against the same value as an array
    pot_a, acc_a, _ = run(ctx, src, mass, np.full(len(src), eps_all, dtype=f32), tgt)
    assert np.array_equal(bits(pot), bits(pot_a)) and np.array_equal(bits(acc), bits(acc_a))
    # 7. the potential only, the accelerations only
    pot_p, none, _ = run(ctx, src, mass, eps_all, tgt, want_acc=False)
    assert none is None and np.array_equal(bits(pot), bits(pot_p))
    none, acc_p, _ = run(ctx, src, mass, eps_all, tgt, want_pot=False)
    assert none is None and np.array_equal(bits(acc), bits(acc_p))
    # 8. the same call twice
    pot_b, acc_b, _ = run(ctx, src, mass, eps_all, tgt)
    assert np.array_equal(bits(pot), bits(pot_b)) and np.array_equal(bits(acc), bits(acc_b))
    # ... and with the targets the sources
    first, second = run(ctx, src, mass, eps_all), run(ctx, src, mass, eps_all)
    assert np.array_equal(bits(first[0]), bits(second[0])) and np.array_equal(bits(first[1]), bits(second[1]))
    only = run(ctx, src, mass, eps_all, want_acc=False)
    assert np.array_equal(bits(first[0]), bits(only[0]))


# ---- 9. refused calls ---------------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing(native, frame_ctx):
    lib = native.load_library()
    src, mass, eps, tgt = scene(300, 40, seed=10)
    x, y, z = cols(src)
    tx, ty, tz = cols(tgt)
    nan_mass = np.full(300, np.nan, dtype=f32)
    outs = Outputs(pot=np.empty(300, dtype=np.float64), acc=np.empty((300, 3), dtype=np.float64), info=native.GravityInfo())

    def call(n_src=300, sx=x, sm=mass, e=eps, eps_all=0.0, n_tgt=40, t=(tx, ty, tz), pot=outs.pot, acc=outs.acc):
        return lib.tsp_gravity_direct(frame_ctx._h, n_src, P(sx), P(y), P(z), P(sm), P(e), eps_all, n_tgt, P(t[0]), P(t[1]), P(t[2]),
                                      P(pot, _dp), P(acc, _dp), ctypes.byref(outs.info))
    cases = {
        "n_src = 0": dict(n_src=0), "n_src = 2^31": dict(n_src=2 ** 31), "n_tgt = 0": dict(n_tgt=0), "n_tgt = 2^31": dict(n_tgt=2 ** 31),
        "NULL sx": dict(sx=None), "NULL mass": dict(sm=None),
        "eps_all < 0": dict(e=None, eps_all=-0.5), "eps_all NaN": dict(e=None, eps_all=float("nan")),
        "eps_all inf": dict(e=None, eps_all=float("inf")),
        "one target array NULL": dict(t=(tx, None, tz)), "two target arrays NULL": dict(t=(None, None, tz)),
        "no output": dict(pot=None, acc=None),
        "targets = sources with n_tgt != n_src": dict(t=(None, None, None), n_tgt=40),
        "no valid source": dict(sm=nan_mass),
    }
    for what, kw in cases.items():
        before = snapshot(frame_ctx)
        outs.fill()
        rc = call(**kw)
        assert rc == EINVAL, f"{what}: return code {rc}: {lib.tsp_last_error().decode(errors='replace')}"
        assert not outs.written(), f"{what}: outputs written: {outs.written()}"
        assert_same_state(before, snapshot(frame_ctx), what)
    outs.fill()
    assert call() == 0 and set(outs.written()) == {"pot", "acc", "info"}


# ---- 10. injected allocation failures -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("self_targets", [False, True])
def test_allocation_failures(native, frame_ctx, K, self_targets):
    lib = native.load_library()
    src, mass, eps, tgt = scene(700, 300, seed=11)
    x, y, z = cols(src)
    tx, ty, tz = (None, None, None) if self_targets else cols(tgt)
    n_tgt = 700 if self_targets else 300
    outs = Outputs(pot=np.empty(n_tgt, dtype=np.float64), acc=np.empty((n_tgt, 3), dtype=np.float64), info=native.GravityInfo())
    walk(native, frame_ctx,
         lambda: lib.tsp_gravity_direct(frame_ctx._h, 700, P(x), P(y), P(z), P(mass), P(eps), 0.0, n_tgt, P(tx), P(ty), P(tz),
                                        P(outs.pot, _dp), P(outs.acc, _dp), ctypes.byref(outs.info)),
         outs, {"sph_sum_h", "sph_sum_a"})
    assert (outs.info.n_valid_sources, outs.info.n_valid_targets) == (700, n_tgt)
    check(outs.pot, outs.acc, gravity_ref.direct_sum(src, mass, eps, None if self_targets else tgt), K, "after the failures")


# ---- 11. the Python layer -----------------------------------------------------------------------------------------------------------
def test_gravity_direct_with_G(K):
    import topsy_amd
    src, mass, eps, tgt = scene(900, 130, seed=12)
    G = 4.30091e-6
    pot, acc = topsy_amd.gravity_direct(src, mass, eps, targets=tgt, G=G)
    assert pot.dtype == np.float64 and acc.shape == (130, 3)
    check(pot / G, acc / G, gravity_ref.direct_sum(src, mass, eps, tgt), K, "topsy_amd.gravity_direct / G")
    pot_s, acc_s = topsy_amd.gravity_direct(src, mass, 0.05)
    check(pot_s, acc_s, gravity_ref.direct_sum(src, mass, 0.05), K, "topsy_amd.gravity_direct, targets = sources")


def plummer_sphere(n, seed):
    """n equal-mass particles of total mass 1 drawn from a Plummer sphere of scale length 1"""
    rs = np.random.RandomState(seed)
    r = 1.0 / np.sqrt(rs.uniform(size=n) ** (-2.0 / 3.0) - 1.0)
    v = rs.normal(size=(n, 3))
    return r[:, None] * v / np.linalg.norm(v, axis=1)[:, None], np.full(n, 1.0 / n)


def plummer_curve_margin(n, radii, eps, sigmas=5.0):
    """The sampling noise of v_circ of n particles of a unit Plummer sphere (M = a = 1), relative, times `sigmas`.
    v^2 = R a_R.  Two independent sources of noise in a_R at a probe, both Poisson: the number of particles inside R, which
    carries the monopole, N_enc = n R^3 / (1 + R^2)^1.5, relative 1 / sqrt(N_enc); and the softened pulls of the particles
    near the probe, each m x / (r^2 + eps^2)^1.5 along the radius, whose variance for a number density nu is
    nu m^2 (4 pi / 3) int r^4 / (r^2 + eps^2)^3 dr = nu m^2 pi^2 / (4 eps), against the mean field M(<R) / R^2.  The four probes
    of a radius share the first and average the second.  v carries half the relative error of v^2.  The softening itself
    lowers v^2 by less than 1.5 eps^2 / R^2, which is added."""
    m = 1.0 / n
    enclosed = radii ** 3 / (1.0 + radii ** 2) ** 1.5
    nu = n * 3.0 / (4.0 * np.pi) * (1.0 + radii ** 2) ** -2.5
    field = enclosed / radii ** 2
    local = np.sqrt(nu * m * m * np.pi ** 2 / (4.0 * eps) / 4.0) / field
    return 0.5 * (sigmas * np.sqrt(1.0 / (n * enclosed) + local ** 2) + 1.5 * eps ** 2 / radii ** 2)


def test_rotation_curve_of_a_plummer_sphere():
    import topsy_amd
    n, eps, G = 20_000, 0.05, 2.5
    pos, mass = plummer_sphere(n, seed=21)
    center = np.array([300.0, -200.0, 100.0])                    # far from the origin: the centre is subtracted in float64
    radii = np.array([0.5, 1.0, 2.0, 4.0])
    curve = topsy_amd.rotation_curve(pos + center, mass, eps, radii, center=center, G=G)
    want = np.sqrt(G * radii ** 2 / (1.0 + radii ** 2) ** 1.5)
    rel = np.abs(curve.v_circ / want - 1.0)
    margin = plummer_curve_margin(n, radii, eps)
    print(f"\nPlummer sphere: v_circ / analytic - 1 = {rel}, margin {margin}")
    assert (rel <= margin).all() and (margin < 0.1).all()
    pot_rel = np.abs(curve.pot / (-G / np.sqrt(1.0 + radii ** 2)) - 1.0)
    assert (pot_rel <= 5.0 / np.sqrt(n) + eps ** 2).all(), pot_rel       # the potential is a sum over all n: relative 1 / sqrt(n)
    assert curve.acc.shape == (4, 4, 3) and np.array_equal(curve.radii, radii)


def tilted_disc(n, seed):
    rs = np.random.RandomState(seed)
    R = rs.exponential(2.0, n)
    phi = rs.uniform(0, 2 * np.pi, n)
    flat = np.stack([R * np.cos(phi), R * np.sin(phi), rs.normal(size=n) * 0.05], axis=1)
    vflat = np.stack([-np.sin(phi), np.cos(phi), np.zeros(n)], axis=1) * 150.0
    a = np.array([0.3, -0.5, 0.81])
    a /= np.linalg.norm(a)
    e1 = np.cross(a, [1.0, 0.0, 0.0])
    e1 /= np.linalg.norm(e1)
    rot = np.stack([e1, np.cross(a, e1), a])                     # rows: the disc's axes in the box
    return (flat @ rot).astype(f32), (vflat @ rot).astype(f32), a


def test_visualizer_rotation_curve_and_phi(K):
    import topsy_amd
    n = 6000
    pos, vel, axis = tilted_disc(n, seed=31)
    mass = np.full(n, 1.0 / n, dtype=f32)
    h = np.full(n, 0.2, dtype=f32)
    eps = 0.1
    radii = np.array([1.0, 3.0, 6.0])
    vis = topsy_amd.from_arrays(pos, h, mass, vel=vel, eps=eps, render_resolution=64)
    try:
        matrix = vis.orient("faceon", 8.0)
        assert abs(matrix[2] @ axis) > 0.999
        curve = vis.rotation_curve(radii)
        frame, _ = topsy_amd.orientation(pos, mass, vel, radius=8.0, orient="faceon")
        assert np.array_equal(frame, matrix)
        direct = topsy_amd.rotation_curve(pos, mass, eps, radii, frame=frame)
        assert np.array_equal(curve.v_circ, direct.v_circ) and np.array_equal(curve.pot, direct.pot)
        assert np.array_equal(curve.acc, direct.acc) and (curve.v_circ > 0).all()
        # 'phi' is a quantity: it equals the direct sum in the loader's order, and renders
        names = vis.data_loader.get_quantity_names()
        assert names[-1] == "phi" and names.index("vorticity") < names.index("phi")
        phi = vis.data_loader.get_named_quantity("phi")
        pot, _ = topsy_amd.gravity_direct(pos, mass, eps)
        assert phi.dtype == f32 and np.array_equal(phi, pot.astype(f32))
        check(pot, None, gravity_ref.direct_sum(pos, mass, eps), K, "'phi' of the disc")
        assert vis.data_loader.get_named_quantity("phi") is phi             # cached
        vis.scale = 10.0
        vis.quantity_name = "phi"
        image = vis.get_sph_presentation_image()
        assert image.shape == (64, 64, 4) and image.dtype == np.uint8
        content = np.asarray(vis.get_sph_image(), dtype=np.float64)          # the mass-weighted mean of phi along the line of sight
        drawn = np.isfinite(content) & (content != 0.0)
        assert content.shape == (64, 64) and drawn.sum() > 64 * 8
        lo, hi = float(phi.min()), float(phi.max())
        assert hi < 0 and (content[drawn] >= lo * (1 + 1e-5)).all() and (content[drawn] <= hi * (1 - 1e-5)).all()
        assert content[drawn].max() - content[drawn].min() > 0.01 * (hi - lo)
    finally:
        vis.close()
