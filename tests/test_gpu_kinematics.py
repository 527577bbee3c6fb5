"""Kinematic maps on the GPU (TSP_MODE_KINEMATIC, tsp_velocity_moments, tsp_colormap_moment, topsy_amd.VelocityView):
the render against the oracle's rgb splat fed the reference weights' colours, the isolation of the two 4-channel modes, the
moment and colormap kernels bit for bit against their restatements, bounds derived from the number formats, and the Python layer.
R = 128 throughout; all_class_scene(128) covers the three footprint classes."""

import numpy as np
import pytest

import kinematics_ref as ref
import parity_scenes as ps
from kinematic_compare import check_kinematic, oracle_kinematic

pytestmark = pytest.mark.gpu
R = 128
SCALE = 100.0
f32 = np.float32


@pytest.fixture(scope="module")
def native():
    from topsy_amd import _native
    _native.load_library()
    return _native


@pytest.fixture(scope="module")
def scene():
    sc = ps.all_class_scene(R)
    rs = np.random.RandomState(11)
    sc["vel"] = (rs.normal(0.0, 100.0, size=sc["pos"].shape) + np.array([50.0, -30.0, 20.0])).astype(f32)
    for a in sc.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return sc


def camera(rotation=None):
    from oracle import oracle_np
    rotation = np.eye(3) if rotation is None else rotation
    M, sf = oracle_np.transform_matrix(rotation, np.zeros(3), SCALE)
    axis = rotation[2] / np.sqrt(rotation[2] @ rotation[2])
    return M, sf, axis.astype(f32)


TILT = ps._rot(0.15, -0.1) @ ps.roll(0.9)


def new_context(native, mips, scene, velocities=True, rgb=False, channels=4):
    ctx = native.Context(R, channels)
    ctx.set_kernel_mips(mips)
    p = scene["pos"]
    ctx.upload_particles(p[:, 0], p[:, 1], p[:, 2], scene["h"], scene["m"])
    if velocities:
        ctx.upload_velocities(*(scene["vel"][:, k] for k in range(3)))
    if rgb:
        ctx.upload_rgb(*(scene["rgb"][:, k].copy() for k in range(3)))
    return ctx


V_BULK = np.array([50.0, -30.0, 20.0], dtype=f32)


# --------------------------------------------------------------------------- the render against the oracle
@pytest.mark.parametrize("case", ["whole", "two_blocks", "tilted", "reorder_after_upload", "reorder_before_upload"])
def test_kinematic_render_matches_the_oracle(native, mips, scene, case):
    M, sf, axis = camera(TILT if case == "tilted" else None)
    n = len(scene["h"])
    ctx = native.Context(R, 4)
    ctx.set_kernel_mips(mips)
    p = scene["pos"]
    ctx.upload_particles(p[:, 0], p[:, 1], p[:, 2], scene["h"], scene["m"])
    vel = [scene["vel"][:, k] for k in range(3)]
    perm = None
    if case == "reorder_before_upload":
        perm = ctx.reorder_spatial(4, 7, want_permutation=True)
    ctx.upload_velocities(*vel)
    if case == "reorder_after_upload":
        perm = ctx.reorder_spatial(4, 7, want_permutation=True)
    ctx.set_line_of_sight(axis, V_BULK)
    ctx.set_option("count_fragments", 1)
    want, nfrag, terms = oracle_kinematic(scene, mips, M, sf, axis, V_BULK)
    if case == "two_blocks":
        cut = 700
        ctx.render(M, sf, [0], [cut], clear=True, mode=native.MODE_KINEMATIC)
        n0 = ctx.stats()["n_fragments"]
        ctx.render(M, sf, [cut], [n - cut], clear=False, mode=native.MODE_KINEMATIC)
        n1 = ctx.stats()["n_fragments"]
        assert n0 == oracle_kinematic(scene, mips, M, sf, axis, V_BULK, ([0], [cut]))[1]
        assert n1 == oracle_kinematic(scene, mips, M, sf, axis, V_BULK, ([cut], [n - cut]))[1]
        assert n0 + n1 == nfrag
    else:
        ctx.render(M, sf, mode=native.MODE_KINEMATIC)
        assert ctx.stats()["n_fragments"] == nfrag
    if perm is not None:
        assert sorted(perm.tolist()) == list(range(n)) and not np.array_equal(perm, np.arange(n))
    check_kinematic(ctx.read_image(), want, terms, case)
    ctx.close()


# --------------------------------------------------------------------------- the two 4-channel modes do not see each other
def two_term_scene():
    """Footprints of all three classes with at most two fragments on any pixel.  The kernels add float32 terms in an order that
    differs from run to run, so two renders of all_class_scene differ in the last bits whatever the weights are; a sum of two
    terms has one value in any order, so here equal weights give equal bits.  Four 64 px footprints tile the image; on top, per
    32 px cell of a checkerboard, one footprint of 17 - 28 px or four of 3 - 12 px in its 16 px quarters, none overlapping."""
    rs = np.random.RandomState(21)
    px = 2.0 * SCALE / R
    cx, cy, P = [], [], []
    for qx in (32.0, 96.0):
        for qy in (32.0, 96.0):
            cx.append(qx), cy.append(qy), P.append(64.0)
    for i in range(4):
        for j in range(4):
            x0, y0 = 32.0 * i + 16.0, 32.0 * j + 16.0
            if (i + j) % 2 == 0:
                cx.append(x0 + rs.uniform(-2, 2)), cy.append(y0 + rs.uniform(-2, 2)), P.append(rs.uniform(17.0, 28.0))
            else:
                for dx in (-8.0, 8.0):
                    for dy in (-8.0, 8.0):
                        cx.append(x0 + dx + rs.uniform(-2, 2)), cy.append(y0 + dy + rs.uniform(-2, 2)), P.append(rs.uniform(3.0, 12.0))
    n = len(P)
    pos = np.zeros((n, 3), dtype=f32)
    pos[:, 0] = (np.array(cx) - R / 2) * px
    pos[:, 1] = (R / 2 - np.array(cy)) * px
    h = (np.array(P) * SCALE / (2.0 * R)).astype(f32)
    sc = ps.make_scene(pos, h, rs.uniform(0.5, 2.0, n), rs.normal(size=n), rs.uniform(0.0, 1.0, (n, 3)), P=np.array(P), scale=SCALE)
    sc["vel"] = (rs.normal(0.0, 100.0, size=(n, 3)) + V_BULK).astype(f32)
    return sc


def test_rgb_and_kinematic_frames_do_not_leak_into_each_other(native, mips):
    scene = two_term_scene()
    assert all(c > 0 for c in ps.class_counts(scene["P"]))
    M, sf, axis = camera()
    plain = new_context(native, mips, scene, velocities=False, rgb=True)
    plain.render(M, sf, mode=native.MODE_RGB)
    rgb_want = plain.read_image()
    st = plain.stats()
    assert st["n_small"] > 0 and st["n_mid"] > 0 and st["n_huge"] > 0
    plain.render(M, sf, mode=native.MODE_RGB)
    assert np.array_equal(plain.read_image(), rgb_want), "the scene's sums are not independent of their order"
    plain.close()
    assert rgb_want[..., 3].max() == 2 and (rgb_want[..., :3].sum(axis=(0, 1)) > 0).all()

    ctx = new_context(native, mips, scene, rgb=True)
    ctx.set_line_of_sight(axis, V_BULK)
    ctx.render(M, sf, mode=native.MODE_KINEMATIC)
    kin_first = ctx.read_image()
    assert not np.array_equal(kin_first[..., :3], rgb_want[..., :3])
    ctx.render(M, sf, mode=native.MODE_RGB)
    assert np.array_equal(ctx.read_image(), rgb_want), "an rgb frame after a kinematic one"
    ctx.render(M, sf, mode=native.MODE_KINEMATIC)
    assert np.array_equal(ctx.read_image(), kin_first), "a kinematic frame after an rgb one"
    ctx.close()

    # the reverse order, against a context that never drew rgb
    other = new_context(native, mips, scene, rgb=True)
    other.render(M, sf, mode=native.MODE_RGB)
    assert np.array_equal(other.read_image(), rgb_want)
    other.set_line_of_sight(axis, V_BULK)
    other.render(M, sf, mode=native.MODE_KINEMATIC)
    assert np.array_equal(other.read_image(), kin_first), "a kinematic frame after an rgb one, on a second context"
    other.close()


def test_a_change_of_v_ref_or_of_the_axis_alone_redraws(native, mips, scene):
    M, sf, axis = camera()
    ctx = new_context(native, mips, scene)
    other_axis = camera(TILT)[2]
    for a, v in ((axis, V_BULK), (axis, np.zeros(3, dtype=f32)), (other_axis, np.zeros(3, dtype=f32)), (axis, V_BULK)):
        ctx.set_line_of_sight(a, v)
        ctx.render(M, sf, mode=native.MODE_KINEMATIC)
        want, _, terms = oracle_kinematic(scene, mips, M, sf, a, v)
        check_kinematic(ctx.read_image(), want, terms, f"axis {a} v_ref {v}")
    ctx.close()


def refused(native, code, call):
    with pytest.raises(native.BackendError, match=rf"libtopsy_splat error {code}:"):
        call()


ESTATE, EINVAL = -4, -1


def test_refused_calls_leave_the_image_as_it_was(native, mips, scene):
    M, sf, axis = camera()
    other_axis = camera(TILT)[2]
    kin = dict(mode=native.MODE_KINEMATIC)
    vel = [scene["vel"][:, k] for k in range(3)]

    # nothing to draw from yet: no velocities, then no line of sight
    ctx = new_context(native, mips, scene, velocities=False, rgb=True)
    ctx.render(M, sf, mode=native.MODE_RGB)
    rgb_img, rgb_stats = ctx.read_image(), ctx.stats()

    def unchanged(img, stats=None):
        assert np.array_equal(ctx.read_image(), img)
        if stats is not None:
            assert ctx.stats() == stats

    refused(native, ESTATE, lambda: ctx.render(M, sf, **kin))
    unchanged(rgb_img, rgb_stats)
    for partial in ((vel[0], None, None), (vel[0], vel[1], None), (None, vel[1], vel[2])):
        refused(native, EINVAL, lambda: ctx.upload_velocities(*partial))
    refused(native, ESTATE, lambda: ctx.render(M, sf, **kin))       # (a refused upload left none)
    ctx.upload_velocities(*vel)
    refused(native, ESTATE, lambda: ctx.render(M, sf, **kin))       # no line of sight
    unchanged(rgb_img, rgb_stats)
    for bad in ((0.0, 0.0, 1.1), (0.0, 0.0, 0.0), (np.nan, 0.0, 1.0), (np.inf, 0.0, 0.0), (0.0, 0.0, 1.0 + 1e-4)):
        refused(native, EINVAL, lambda: ctx.set_line_of_sight(bad, (0.0, 0.0, 0.0)))
    refused(native, EINVAL, lambda: ctx.set_line_of_sight(axis, (0.0, np.nan, 0.0)))
    refused(native, ESTATE, lambda: ctx.render(M, sf, **kin))       # (a refused line of sight set none)
    unchanged(rgb_img, rgb_stats)

    # clear = 0 across the two 4-channel modes, and across lines of sight
    ctx.set_line_of_sight(axis, V_BULK)
    refused(native, ESTATE, lambda: ctx.render(M, sf, clear=False, **kin))
    unchanged(rgb_img, rgb_stats)
    ctx.render(M, sf, [0], [700], **kin)
    kin_img, kin_stats = ctx.read_image(), ctx.stats()
    refused(native, ESTATE, lambda: ctx.render(M, sf, [700], [800], clear=False, mode=native.MODE_RGB))
    unchanged(kin_img, kin_stats)
    ctx.set_line_of_sight(other_axis, V_BULK)
    refused(native, ESTATE, lambda: ctx.render(M, sf, [700], [800], clear=False, **kin))
    unchanged(kin_img, kin_stats)
    ctx.set_line_of_sight(axis, np.zeros(3))
    refused(native, ESTATE, lambda: ctx.render(M, sf, [700], [800], clear=False, **kin))
    unchanged(kin_img, kin_stats)
    refused(native, EINVAL, lambda: ctx.set_line_of_sight((0.0, 2.0, 0.0), V_BULK))      # ... which leaves the last good one
    refused(native, ESTATE, lambda: ctx.render(M, sf, [700], [800], clear=False, **kin))
    refused(native, EINVAL, lambda: ctx.render(M, sf, flags=native.PIPE_GENERIC, **kin))
    unchanged(kin_img, kin_stats)
    # the block it was started with continues, and gives the whole frame
    ctx.set_line_of_sight(axis, V_BULK)
    ctx.render(M, sf, [700], [800], clear=False, **kin)
    want, _, terms = oracle_kinematic(scene, mips, M, sf, axis, V_BULK)
    check_kinematic(ctx.read_image(), want, terms, "continued after refusals")
    ctx.close()

    # a 2-channel context has no kinematic mode; its image stays
    two = new_context(native, mips, scene, channels=2)
    two.set_line_of_sight(axis, V_BULK)
    two.render(M, sf)
    img2 = two.read_image()
    refused(native, EINVAL, lambda: two.render(M, sf, **kin))
    assert np.array_equal(two.read_image(), img2)
    two.close()

    # velocities need particles
    empty = native.Context(R, 4)
    refused(native, ESTATE, lambda: empty.upload_velocities(*[np.zeros(0, dtype=f32)] * 3))
    empty.close()


# --------------------------------------------------------------------------- moments and their colormap
def moment_test_image():
    rs = np.random.RandomState(5)
    S = np.exp(rs.uniform(-20, 10, (R, R))).astype(f32)
    mean = rs.normal(0, 200, (R, R))
    sig = np.exp(rs.uniform(-3, 6, (R, R)))
    img = np.empty((R, R, 4), dtype=f32)
    img[..., 0] = S
    img[..., 1] = (S * mean).astype(f32)
    img[..., 2] = (S * (mean * mean + sig * sig)).astype(f32)
    img[..., 3] = rs.randint(0, 1000, (R, R))
    img[0, :32] = 0.0                                   # nothing drawn
    img[1, :32, 0] = -img[1, :32, 0]                    # negative S
    img[2, :32, 0] = 0.0                                # S = 0 with sums
    img[2, 32:40, 0] = -0.0
    img[3, :8, 0], img[3, 8:16, 1], img[3, 16:24, 2] = np.nan, np.nan, np.nan
    img[4, :8, 0], img[4, 8:16, 1], img[4, 16:24, 2] = np.inf, -np.inf, np.inf
    img[5, :32, 2] = img[5, :32, 2] * f32(0.5)          # B / S < mean^2 for most: clamped
    img[6, :32, 1] = 0.0                                # mean 0
    img[6, 32:40, 2] = -0.0
    img[7, :32, 2] = (img[7, :32, 1].astype(np.float64) ** 2 / img[7, :32, 0]).astype(f32)      # var = rounding noise of either sign
    img[8, :16, 0] = np.finfo(f32).tiny / 4             # a denormal S
    img[8, 16:32, :3] = np.finfo(f32).max               # the largest finite sums
    return img


def test_moments_and_their_colormap_are_bit_exact(native, mips, scene):
    from oracle import oracle_c
    M, sf, axis = camera()
    ctx = new_context(native, mips, scene)
    refused(native, ESTATE, ctx.velocity_moments)
    ctx.set_line_of_sight(axis, V_BULK)
    ctx.render(M, sf, [0], [64], mode=native.MODE_KINEMATIC)
    stats = ctx.stats()
    img = moment_test_image()
    ctx.write_image(img)
    want = ref.velocity_moments(img)
    assert np.isnan(want[..., 1]).sum() > 100 and (want[5, :32, 2] == 0).sum() > 16 and np.isfinite(want[..., 2]).sum() > R * R // 2
    got = ctx.velocity_moments()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
        f"{(got.view(np.uint32) != want.view(np.uint32)).sum()} values differ from the float64 restatement"
    lut = np.random.RandomState(8).uniform(0, 1, (257, 4)).astype(f32)
    for which, (vmin, vmax) in ((1, (-300.0, 300.0)), (2, (0.5, 400.0))):
        for log, (lo, hi) in ((False, (vmin, vmax)), (True, (-1.0, 2.5))):
            value = np.stack([want[..., which], np.zeros((R, R), dtype=f32)], axis=-1)
            with np.errstate(invalid="ignore", divide="ignore"):
                expect = oracle_c.colormap_scalar(value, lut, lo, hi, log, False)
            assert np.array_equal(ctx.colormap_moment(which, lut, lo, hi, log), expect), (which, log)
    refused(native, EINVAL, lambda: ctx.colormap_moment(0, lut, 0.0, 1.0))
    refused(native, EINVAL, lambda: ctx.colormap_moment(3, lut, 0.0, 1.0))
    # neither call changed the image, the accumulator (a clear = 0 block of nothing rounds it again) or the stats
    assert np.array_equal(ctx.read_image(), img, equal_nan=True) and ctx.stats() == stats
    ctx.render(M, sf, [0], [0], clear=False, mode=native.MODE_KINEMATIC)
    assert np.array_equal(ctx.read_image(), img, equal_nan=True)
    # another mode ends the kinematic image
    ctx.render(M, sf)
    refused(native, ESTATE, ctx.velocity_moments)
    refused(native, ESTATE, lambda: ctx.colormap_moment(1, lut, 0.0, 1.0))
    ctx.close()


# --------------------------------------------------------------------------- bounds that follow from the formats
def test_constant_velocity_fields(native, mips, scene):
    M, sf, axis = camera(TILT)
    ctx = new_context(native, mips, scene, velocities=False)
    v0 = np.array([123.456, -78.9, 310.25], dtype=f32)
    n = len(scene["h"])
    ctx.upload_velocities(*(np.full(n, v0[k], dtype=f32) for k in range(3)))
    # all velocities equal to v_ref: u, m u and m u^2 are exactly +0, so the maps are exactly 0 wherever anything was drawn
    ctx.set_line_of_sight(axis, v0)
    ctx.render(M, sf, mode=native.MODE_KINEMATIC)
    maps = ctx.velocity_moments()
    drawn = maps[..., 0] > 0
    assert drawn.sum() > R * R // 2
    assert (maps[..., 1][drawn] == 0).all() and (maps[..., 2][drawn] == 0).all()
    assert np.isnan(maps[..., 1][~drawn]).all() and np.isnan(maps[..., 2][~drawn]).all()
    # v_ref = 0: every particle has the same float32 u.  A weight carries at most three float32 roundings (m u, the quotient, and
    # m / hh of S), a fragment one more (k w), the channel one: (3 + 1 + 1 + 2 of S) * 6e-8 = 4.2e-7 < 1e-6.  B / S - mean^2
    # cancels u^2 to the same 1.3e-6 or so: sigma <= sqrt(1.3e-6) |u| = 1.1e-3 |u| < 2e-3 |u|
    ctx.set_line_of_sight(axis, np.zeros(3))
    ctx.render(M, sf, mode=native.MODE_KINEMATIC)
    maps = ctx.velocity_moments()
    u = float(ref.kinematic_colours(np.ones(1, dtype=f32), v0[None, :], axis, np.zeros(3))[3][0])
    assert abs(u) > 100
    drawn = maps[..., 0] > 0
    err = np.abs(maps[..., 1][drawn].astype(np.float64) - u).max() / abs(u)
    sig = maps[..., 2][drawn].astype(np.float64).max() / abs(u)
    print(f"constant field: max |v_los - u| / |u| = {err:.3g}, max sigma_los / |u| = {sig:.3g}")
    assert err <= 1e-6
    assert sig <= 2e-3
    ctx.close()


# --------------------------------------------------------------------------- the Python layer
VIEW = 16.0        # the disc views' half-width: 1 / VIEW and the pixel, 2 VIEW / R = 0.25, are exact in float32


def disc(n_half=1500, seed=4, omega=16.0):
    """A thin solid-body disc in the xy plane, v = omega z^ x r, in mirror pairs x <-> -x: (pos, h, m, vel).
    Seen edge-on at half-width VIEW every number the splat forms from a pair is exact and mirrored: x and z put the footprint
    centres on odd sixteenths of a pixel (so no fragment sits on a texel boundary, where nearest-texel sampling would take the two
    sides differently), the widths are powers of two in pixels, omega is a power of two.  The two halves of the image then hold
    the same terms, and differ by the order of their sums alone."""
    rs = np.random.RandomState(seed)
    px = 2.0 * VIEW / R
    x = (2 * rs.randint(0, 320, n_half) + 1) / 16.0 * px                       # (0, 10]
    z = (2 * rs.randint(-12, 12, n_half) + 1) / 16.0 * px                      # within 1.5 px of the plane
    y = rs.uniform(-1.0, 1.0, n_half) * np.sqrt(np.maximum(100.0 - x * x, 0.0))
    half = np.stack([x, y, z], axis=1).astype(f32)
    assert np.array_equal(half[:, 0], x) and np.array_equal(half[:, 2], z)
    pos = np.concatenate([half, half * np.array([-1.0, 1.0, 1.0], dtype=f32)])
    P = 2.0 ** rs.randint(1, 8, n_half)                                        # 2 .. 128 px: every footprint class
    h = np.tile((P * px / 4.0).astype(f32), 2)
    m = np.tile(rs.uniform(0.5, 2.0, n_half).astype(f32), 2)
    vel = np.stack([-omega * pos[:, 1], omega * pos[:, 0], np.zeros(len(pos))], axis=1).astype(f32)
    return pos, h, m, vel


EDGE_ON = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]])      # the line of sight is -y: u = -v_y = -omega x


@pytest.fixture(scope="module")
def disc_vis():
    import topsy_amd
    pos, h, m, vel = disc()
    vis = topsy_amd.from_arrays(pos, h, m, vel=vel, render_resolution=R)
    vis.scale = VIEW
    yield vis, (pos, h, m, vel)
    vis.close()


def maps_close(a, b, label):
    """Two renders of one scene.  The kernels add float32 terms in an order that differs from run to run, so each render is only
    known to be within the project's 1e-5 of the exact sums: S and B within 1e-5, A within 1e-5 * sum|terms| <= 1e-5 sqrt(S B)
    (Cauchy-Schwarz).  With rms^2 = B / S = v^2 + sigma^2 two renders then agree in S to 2e-5, in v = A / S to 2e-5 rms + 2e-5 |v|
    <= 4e-5 rms, and in sigma^2 = B / S - v^2 to 4e-5 rms^2 + 2 |v| 4e-5 rms <= 1.2e-4 rms^2.  The count is exact."""
    assert np.array_equal(a["count"], b["count"]), label
    assert np.array_equal(np.isnan(a["v_los"]), np.isnan(b["v_los"])), label
    ok = ~np.isnan(a["v_los"])
    assert ok.sum() > 1000
    assert np.allclose(a["surface_density"][ok], b["surface_density"][ok], rtol=2e-5, atol=0), label
    va, vb = a["v_los"][ok].astype(np.float64), b["v_los"][ok].astype(np.float64)
    sa, sb = a["sigma_los"][ok].astype(np.float64), b["sigma_los"][ok].astype(np.float64)
    rms2 = np.maximum(va * va + sa * sa, vb * vb + sb * sb)
    print(f"{label}: max |dv| / rms = {np.max(np.abs(va - vb) / np.sqrt(np.maximum(rms2, 1e-300))):.3g}, "
          f"max |d sigma^2| / rms^2 = {np.max(np.abs(sa * sa - sb * sb) / np.maximum(rms2, 1e-300)):.3g}")
    assert (np.abs(va - vb) <= 4e-5 * np.sqrt(rms2) + 1e-30).all(), label
    assert (np.abs(sa * sa - sb * sb) <= 1.2e-4 * rms2 + 1e-30).all(), label


def test_velocity_view_follows_the_visualizer(disc_vis):
    import topsy_amd
    from topsy_amd import loader
    vis, (pos, h, m, vel) = disc_vis
    vis.rotation_matrix = np.eye(3)
    view = topsy_amd.VelocityView(vis, v_ref=None)
    ctx = vis.particle_buffers.context

    # face-on: the line of sight is z and v_z = 0, so u is exactly 0
    face = view.get_maps()
    assert set(face) == {"surface_density", "v_los", "sigma_los", "count"} and all(a.shape == (R, R) for a in face.values())
    raw = ctx.velocity_moments()
    scale = np.float32(view._sph.last_render_mass_scale)
    assert np.array_equal(face["surface_density"], raw[..., 0] * scale)
    for k, name in ((1, "v_los"), (2, "sigma_los"), (3, "count")):
        assert np.array_equal(face[name], raw[..., k], equal_nan=True)
    drawn = face["surface_density"] > 0
    assert drawn.sum() > 1000 and (face["v_los"][drawn] == 0).all() and (face["sigma_los"][drawn] == 0).all()

    # a read of the visualizer in between is its own frame, and the view then draws its own again
    density = vis.get_sph_image()
    assert density.shape[:2] == (R, R) and np.isfinite(density).any() and (density[np.isfinite(density)] > 0).any()
    again = view.get_maps()
    maps_close(again, face, "the view's frame after a read of the visualizer")
    assert (again["v_los"][drawn] == 0).all()
    assert np.allclose(vis.get_sph_image(), density, rtol=2e-5, atol=0, equal_nan=True)      # (two renders: 1e-5 each)

    # edge-on: the view follows the visualizer's rotation; v_los = -omega x' is odd under x' -> -x'
    vis.rotation_matrix = EDGE_ON
    edge = view.get_maps()
    assert not np.array_equal(edge["count"], face["count"])
    S, A, B, _ = np.moveaxis(view.get_raw_image().astype(np.float64), -1, 0)
    # the render tolerance, twice (a pixel and its mirror image): S to 1e-5, A to 1e-5 * sum|terms| <= 1e-5 * sqrt(S B) (Cauchy-Schwarz)
    assert (np.abs(S - S[:, ::-1]) <= 2e-5 * np.maximum(S, S[:, ::-1])).all()
    bound = np.sqrt(np.maximum(S * B, (S * B)[:, ::-1]))
    assert (np.abs(A + A[:, ::-1]) <= 2e-5 * bound + 1e-30).all()
    ok = S > 0
    v = edge["v_los"].astype(np.float64)
    rms = np.sqrt(np.maximum(B / np.where(ok, S, 1.0), 0.0))
    assert (np.abs(v + v[:, ::-1])[ok] <= 4e-5 * np.maximum(rms, rms[:, ::-1])[ok] + 1e-30).all()
    x = ((np.arange(R) + 0.5) * 2.0 / R - 1.0) * VIEW
    mid = edge["v_los"][R // 2 - 2:R // 2 + 2]
    assert np.nanmean(mid[:, x > 3], axis=None) < -40 and np.nanmean(mid[:, x < -3], axis=None) > 40       # -omega x', omega = 16

    # arrays only: the same camera gives the same maps
    alone = topsy_amd.velocity_maps(pos, h, m, vel, rotation=EDGE_ON, scale=VIEW, resolution=R)
    maps_close(edge, alone, "velocity_maps against the view")

    # presentation images and parameters
    for kind in ("v_los", "sigma_los"):
        rgba = view.get_presentation_image(kind)
        assert rgba.shape == (R, R, 4) and rgba.dtype == np.uint8 and len(np.unique(rgba[..., :3].reshape(-1, 3), axis=0)) > 10
    lo, hi = view.get_range("v_los")
    fin = np.abs(edge["v_los"][np.isfinite(edge["v_los"])].astype(np.float64))
    assert hi == np.percentile(fin, 99.0) and lo == -hi
    view["v_los", "vmax"] = 50.0
    assert view.get_range("v_los") == (-50.0, 50.0)
    view.sigma_los_vmin, view.sigma_los_vmax = 1.0, 30.0
    assert view["sigma_los", "vmax"] == 30.0 and view.get_range("sigma_los") == (1.0, 30.0)
    narrow = view.get_presentation_image("v_los")
    view["v_los", "vmax"] = None
    assert not np.array_equal(narrow, view.get_presentation_image("v_los"))
    with pytest.raises(KeyError):
        view["v_los", "gamma"]
    with pytest.raises(ValueError):
        view.get_presentation_image("speed")

    # v_ref = "center": the mean velocity about the view's centre, (0, 0, 0) for this disc up to its sampling
    centred = topsy_amd.VelocityView(vis, v_ref="center")
    m5 = vis.data_loader._with_context(lambda c: c.sphere_moments(pos[:, 0], pos[:, 1], pos[:, 2], m, vel=[vel[:, k] for k in range(3)],
                                                                  center=-np.asarray(vis.position_offset, dtype=np.float64), r=VIEW,
                                                                  r_vel=loader.VEL_RADIUS_FRACTION * VIEW))
    assert np.array_equal(centred.v_ref, m5["v_cen"])
    got = centred.get_maps()
    want = topsy_amd.velocity_maps(pos, h, m, vel, rotation=EDGE_ON, scale=VIEW, resolution=R, v_ref="center")
    maps_close(got, want, "v_ref = center")
    vis.rotation_matrix = np.eye(3)


def test_progressive_kinematic_frames_refine_to_the_export_frame():
    """a CHANGE frame draws a prefix of the strata, REFINE frames add the rest without clearing (along the line of sight that
    started the frame); only the surface density carries the frame's mass scale"""
    import topsy_amd
    from topsy_amd.drawreason import DrawReason
    n = 200_000
    rs = np.random.RandomState(9)
    pos = (rs.normal(size=(n, 3)) * 30.0).astype(f32)
    h = np.exp(rs.uniform(np.log(0.3), np.log(8.0), n)).astype(f32)
    m = rs.uniform(0.5, 2.0, n).astype(f32)
    vel = (rs.normal(0.0, 100.0, (n, 3)) + np.array([0.0, 0.0, 3.0]) * pos[:, :1]).astype(f32)
    vis = topsy_amd.from_arrays(pos, h, m, vel=vel, render_resolution=R)
    vis.scale = 100.0
    view = topsy_amd.VelocityView(vis, v_ref=None)
    full = view.get_maps()
    rp = view._sph._render_progression
    rp._recommended_num_particles_to_render = 50_000
    timer = view._sph._render_timer
    real_add = timer.add_block
    timer.add_block = lambda ms, wall_seconds=None: real_add(40.0)      # one block per interactive frame (test_gpu_visualizer.py)
    view.render(DrawReason.CHANGE)
    scale = view._sph.last_render_mass_scale
    assert 2.0 < scale < 8.0 and view.needs_refine()
    part = view.get_maps()
    assert view._sph.last_render_mass_scale == scale, "reading the maps must not redraw the frame"
    assert 0.9 < part["surface_density"].sum(dtype=np.float64) / full["surface_density"].sum(dtype=np.float64) < 1.1
    assert part["count"].sum(dtype=np.float64) < 0.6 * full["count"].sum(dtype=np.float64)
    frames = 1
    while view.needs_refine():
        view.render(DrawReason.REFINE)
        frames += 1
    assert frames > 1 and view._sph.last_render_mass_scale == 1.0
    maps_close(view.get_maps(), full, "refined against the export frame")
    vis.close()


def test_velocity_view_refuses_loaders_and_visualizers_it_cannot_draw(native):
    import topsy_amd
    vis = topsy_amd.test(500, render_resolution=64)
    with pytest.raises(ValueError, match="no velocities"):
        topsy_amd.VelocityView(vis)
    vis.close()
    per = topsy_amd.test(500, render_resolution=64, periodic_tiling=True)
    with pytest.raises((NotImplementedError, ValueError)):
        topsy_amd.VelocityView(per)
    per.close()
    pos, h, m, vel = disc(50)
    with pytest.raises(ValueError, match="vel"):
        topsy_amd.velocity_maps(pos, h, m, None)
    with pytest.raises(ValueError, match="v_ref"):
        topsy_amd.velocity_maps(pos, h, m, vel, v_ref="middle", resolution=64)
