"""The perspective camera on the GPU: tsp_project_perspective against its NumPy model (tests/perspective_ref.py) bit for bit, the
unchanged pipeline on the transformed snapshot against the oracle, the fused bounds and weights, the reference plane against the
orthographic view, the small-angle claim against exact line integrals, the refused calls, and PerspectiveView with its frames and
its recorder."""
import ctypes

import numpy as np
import pytest

import perspective_ref as ref
import present_ref
import topsy_amd
from parity_scenes import abs_terms_image, check_2ch, oracle_render
from topsy_amd import _native, kernel_lut, perspective
from topsy_amd.drawreason import DrawReason

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ("x", "y", "z", "h", "mass")
RGB = ("r", "g", "b")


def turn(a, b):
    ca, sa, cb, sb = np.cos(a), np.sin(a), np.cos(b), np.sin(b)
    return (np.array([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]]) @ np.array([[1, 0, 0], [0, cb, -sb], [0, sb, cb]])).astype(F)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def same_bits(got, want, names):
    for k in names:
        assert np.array_equal(bits(got[k]), bits(want[k])), k


def max_rel(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    den = np.maximum(np.abs(a), np.abs(b))
    lit = den > 0
    return float((np.abs(a - b)[lit] / den[lit]).max()) if lit.any() else 0.0


def pair(R, channels, arrays, mips, rgb=None, reorder=None):
    """Two contexts holding the same snapshot in the same resident order."""
    out = []
    for _ in range(2):
        ctx = _native.Context(R, channels)
        ctx.set_kernel_mips(mips)
        ctx.upload_particles(*[arrays[k] for k in NAMES])
        if reorder:
            ctx.reorder_spatial(*reorder)
        if rgb is not None:
            ctx.upload_rgb(rgb[:, 0], rgb[:, 1], rgb[:, 2])
        out.append(ctx)
    return out


# ---- 1. the projection against the model ------------------------------------------------------------------------------
def snapshot(n, golden):
    if n == 1:
        return {"x": np.array([0.5], dtype=F), "y": np.array([-0.25], dtype=F), "z": np.array([2.0], dtype=F),
                "h": np.array([0.125], dtype=F), "mass": np.array([1.5], dtype=F)}, np.array([[0.25, 0.5, 0.75]], dtype=F)
    if n == 1000:
        d = golden["testdata_n1000.npz"]
        ps = d["pos_smooth"]
        a = {"x": ps[:, 0].copy(), "y": ps[:, 1].copy(), "z": ps[:, 2].copy(), "h": ps[:, 3].copy(), "mass": d["mass"].copy()}
        rgb = d["rgb"].astype(F)
    else:
        rs = np.random.RandomState(100 + n)
        a = {"x": rs.normal(size=n).astype(F) * 3, "y": rs.normal(size=n).astype(F) * 2, "z": rs.normal(size=n).astype(F) * 4,
             "h": np.exp(rs.uniform(np.log(0.01), np.log(2.0), size=n)).astype(F), "mass": rs.uniform(0.5, 2.0, size=n).astype(F)}
        rgb = rs.uniform(0.0, 1.0, size=(n, 3)).astype(F)
    return a, rgb


def grazing_camera(a, rot, offset):
    """(distance, near, k): a viewer so near that about a tenth of the particles lie behind it or inside `near`, with particle
    k at d == near exactly: near is the float32 difference the kernel forms for it."""
    _, _, zv = ref.view_coordinates(a["x"], a["y"], a["z"], *ref.camera(rot, offset, 1.0, 0.5)[:2])
    order = np.argsort(zv)
    k = int(order[int(0.9 * (len(zv) - 1))])
    distance = F(zv[k] + F(0.05) * (F(1.0) + np.abs(zv[k])))
    near = distance - zv[k]
    assert 0 < near < distance
    return distance, near, k


@pytest.mark.parametrize("with_rgb", [False, True], ids=["density", "rgb"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 511, 512, 513, 1000])
def test_projection_equals_the_model_bit_for_bit(n, with_rgb, golden, mips):
    a, rgb = snapshot(n, golden)
    rot, offset = turn(0.4, -0.3), np.array([0.3, -0.2, 0.1], dtype=F)
    distance, near, k = grazing_camera(a, rot, offset)
    if n >= 63:
        j = (k + 1) % n
        a["x"][j] = a["y"][j] = a["z"][j] = np.nan                    # a NaN row
    src, dst = pair(64, 4, a, mips, rgb if with_rgb else None, reorder=(2, 7) if n in (513, 1000) else None)
    try:
        names = NAMES + (RGB if with_rgb else ())
        before = src.download_particles(names)
        assert np.array_equal(bits(before["x"]), bits(dst.download_particles(("x",))["x"]))      # the two resident orders agree
        want = ref.project(before, rot, offset, distance, near)
        # the camera is what the issue asks for: one particle exactly at d == near (visible), about a tenth not visible
        kk = int(np.flatnonzero(want["d"] == near)[0])
        assert want["visible"][kk] and not np.isnan(want["x"][kk])
        hidden = int((~want["visible"]).sum())
        if n >= 63:
            assert 0.05 * n <= hidden <= 0.2 * n, hidden
        src.project_perspective(dst, rot, offset, distance, near)
        same_bits(dst.download_particles(names), want, names)
        same_bits(src.download_particles(names), before, names)      # src is only read
        # the weights and bounds of the same pass are what a fresh upload of the transformed particles forms for itself
        R = 64
        M, sf = perspective.clip_matrix(4.0, float(distance), float(near), float(distance) + 20.0)
        dst.render(M, sf, mode=_native.MODE_WEIGHTED)
        got = dst.read_image()
        fresh = _native.Context(R, 2)
        fresh.set_kernel_mips(mips)
        fresh.upload_particles(*[want[k_] for k_ in NAMES])
        fresh.render(M, sf, mode=_native.MODE_WEIGHTED)
        assert max_rel(got[..., 0], fresh.read_image()[..., 0]) <= 1e-5
        fresh.close()
    finally:
        src.close()
        dst.close()


# ---- 2. render parity of the transformed snapshot ---------------------------------------------------------------------
PARITY_R = 256
PARITY_CAMERAS = {
    # scale, fov, rot, offset: outside the cloud looking in; and the viewer inside the cloud's near edge
    "outside": (0.5, 60.0, turn(0.3, -0.7), np.zeros(3, dtype=F)),
    "inside": (0.4, 90.0, turn(-0.2, 0.25), np.array([0.03, -0.02, 0.0], dtype=F)),
}


@pytest.fixture(scope="module", params=list(PARITY_CAMERAS))
def parity_scene(request, golden, mips):
    scale, fov, rot, offset = PARITY_CAMERAS[request.param]
    pos = (golden["cells_20000.npz"]["pos"] - 0.5).astype(F)
    n = len(pos)
    rs = np.random.RandomState(11)
    a = {"x": pos[:, 0].copy(), "y": pos[:, 1].copy(), "z": pos[:, 2].copy(),
         "h": np.exp(rs.uniform(np.log(1e-4), np.log(0.3), size=n)).astype(F), "mass": rs.uniform(0.5, 2.0, size=n).astype(F)}
    q = rs.normal(size=n).astype(F)
    rgb = rs.uniform(0.0, 1.0, size=(n, 3)).astype(F)
    distance = F(perspective.fov_to_distance(scale, fov))
    near = F(distance * 1e-3)
    far = float(distance) + 1.0
    # one particle grazing the viewer on the optical axis, d = 2 near: s = 500, its footprint is wider than the image
    p = np.linalg.solve(rot.astype(np.float64), np.array([0.0, 0.0, float(distance) - 2.0 * float(near)])) - offset
    a["x"][0], a["y"][0], a["z"][0], a["h"][0] = p[0], p[1], p[2], 0.01
    want = ref.project(dict(a, r=rgb[:, 0], g=rgb[:, 1], b=rgb[:, 2]), rot, offset, distance, near)
    hidden = (~want["visible"]).mean()
    assert hidden <= 0.15, hidden
    if request.param == "inside":
        assert hidden >= 0.02, hidden
    assert want["visible"][0] and 2.0 * want["h"][0] * PARITY_R / scale > PARITY_R
    src, dst = pair(PARITY_R, 4, a, mips, rgb)
    dst.upload_quantity(q)
    src.project_perspective(dst, rot, offset, distance, near)
    dst.set_option("count_fragments", 1)
    names = NAMES + RGB
    got = dst.download_particles(names)
    same_bits(got, want, names)
    fin = np.isfinite(got["x"]) & np.isfinite(got["y"]) & np.isfinite(got["z"])
    pos_t = np.stack([got["x"][fin], got["y"][fin], got["z"][fin]], axis=1)
    M, sf = perspective.clip_matrix(scale, float(distance), float(near), far)
    scene = {"dst": dst, "M": M, "sf": sf, "pos": pos_t, "h": got["h"][fin], "m": got["mass"][fin], "q": q[fin],
             "rgb": [got[c][fin].copy() for c in RGB]}
    yield scene
    src.close()
    dst.close()


@pytest.mark.parametrize("mode", ["density", "weighted", "rgb", "depth"])
def test_render_of_the_projected_context_matches_the_oracle(parity_scene, mode, mips):
    s, R = parity_scene, PARITY_R
    dst, M, sf, pos, h, m = s["dst"], s["M"], s["sf"], s["pos"], s["h"], s["m"]
    if mode == "rgb":
        dst.render(M, sf, mode=_native.MODE_RGB)
        got = dst.read_image()
        want, nfrag = oracle_render(pos, h, s["rgb"][0], s["rgb"][1], s["rgb"][2], 2, M, sf, R, mips)
        assert np.allclose(got[..., :3], want[..., :3], rtol=1e-5, atol=0)
        assert np.array_equal(got[..., 3], want[..., 3]), "fragment-count channel must be exact"
    elif mode == "depth":
        dst.render(M, sf, mode=_native.MODE_DEPTH)
        want, nfrag = oracle_render(pos, h, m, None, None, 1, M, sf, R, mips)
        assert np.allclose(dst.read_image(), want, rtol=1e-5, atol=0)
    elif mode == "density":
        dst.set_option("use_quantity", 0)
        dst.render(M, sf, mode=_native.MODE_WEIGHTED)
        dst.set_option("use_quantity", 1)
        got = dst.read_image()
        want, nfrag = oracle_render(pos, h, m, None, None, 0, M, sf, R, mips)
        assert np.allclose(got[..., 0], want[..., 0], rtol=1e-5, atol=0)
        assert (got[..., 1] == 0).all()
    else:
        dst.render(M, sf, mode=_native.MODE_WEIGHTED)
        want, nfrag = oracle_render(pos, h, m, s["q"], None, 0, M, sf, R, mips)
        check_2ch(dst.read_image(), want, abs_terms_image(pos, h, m, s["q"], M, sf, R, mips))
    st = dst.stats()
    assert st["n_fragments"] == nfrag
    assert st["n_small"] > 0 and st["n_mid"] > 0 and st["n_huge"] > 0      # footprints reach all three kernels


# ---- 3. the fused bounds and weights ------------------------------------------------------------------------------------
CULL_N = 2_200_000          # chunk culling starts at 4096 chunks of 512 particles
COUNT_KEYS = ("n_particles", "n_small", "n_mid", "n_huge", "n_culled", "n_fragments")


def synthetic_context(R, mips):
    ctx = _native.Context(R, 2)
    ctx.set_kernel_mips(mips)
    ctx.generate_synthetic(CULL_N, 0, CULL_N, 99, 0.0, with_quantity=False)
    ctx.reorder_spatial(8, 99)
    ctx.set_option("count_fragments", 1)
    return ctx


def render_both_ways(ctx, M, sf):
    out = []
    for cull in (1, 0):
        ctx.set_option("chunk_cull", cull)
        ctx.render(M, sf, mode=_native.MODE_WEIGHTED)
        out.append((ctx.read_image(), ctx.stats()))
    ctx.set_option("chunk_cull", 1)
    return out


def same_frame(a, b):
    """Two renders of one scene: the same counts, the same lit pixels and, as the float64 atomics arrive in another order, sums
    within 1e-5 (the criterion of the chunk-culling tests)."""
    (img_a, st_a), (img_b, st_b) = a, b
    for k in COUNT_KEYS:
        assert st_a[k] == st_b[k], (k, st_a[k], st_b[k])
    assert np.array_equal(img_a == 0, img_b == 0)
    assert max_rel(img_a, img_b) <= 1e-5


def test_fused_bounds_and_weights_cull_and_follow_the_camera(mips):
    R = 128
    cam_a = (turn(0.0, 0.0), np.array([-150.0, 90.0, -40.0], dtype=F), 25.0, 40.0)     # an off-centre zoom: most blocks lie outside
    cam_b = (turn(0.7, -0.4), np.array([-20.0, -10.0, 60.0], dtype=F), 40.0, 70.0)
    src, dst = synthetic_context(R, mips), synthetic_context(R, mips)
    fresh = None
    try:
        assert np.array_equal(src.strata_offsets(), dst.strata_offsets())
        frames = {}
        for name, (rot, offset, scale, fov) in (("a", cam_a), ("b", cam_b)):
            distance = perspective.fov_to_distance(scale, fov)
            near, far = distance * 1e-3, distance + 40.0 * scale
            src.project_perspective(dst, rot, offset, distance, near)
            M, sf = perspective.clip_matrix(scale, distance, near, far)
            on, off = render_both_ways(dst, M, sf)
            assert off[1]["n_chunk_culled"] == 0 and on[1]["n_chunk_culled"] > 0, name
            assert on[1]["n_small"] + on[1]["n_mid"] + on[1]["n_huge"] > 0, name
            same_frame(on, off)
            frames[name] = (on, M, sf, (rot, offset, distance, near))
        assert np.array_equal(dst.strata_offsets(), src.strata_offsets()) and dst.cell_layout() is None
        # the second camera on a context that saw the first equals the second camera on a fresh context
        on_b, M, sf, cam = frames["b"]
        fresh = synthetic_context(R, mips)
        src.project_perspective(fresh, *cam)
        same_bits(fresh.download_particles(NAMES), dst.download_particles(NAMES), NAMES)
        fresh.render(M, sf, mode=_native.MODE_WEIGHTED)
        same_frame(on_b, (fresh.read_image(), fresh.stats()))
        assert fresh.stats()["n_chunk_culled"] == on_b[1]["n_chunk_culled"]
    finally:
        for c in (src, dst, fresh):
            if c is not None:
                c.close()


# ---- 4. the reference plane ---------------------------------------------------------------------------------------------
def sparse_plane_snapshot(R=256):
    """A flattened snapshot no pixel of which is covered by more than two footprints, for a view of scale 1 at R^2: one huge
    footprint (110 px), three mid ones (60, 40, 24 px) and a 16 x 16 lattice of small ones (0.5 to 14 px on a 16 px pitch,
    centres jittered by a pixel).  Two renders of one context differ in the last bits wherever three or more terms meet (the
    partial sums arrive in another order); with at most two terms per pixel every sum is one commutative addition, so a
    bit-for-bit comparison of two images is meaningful."""
    rs = np.random.RandomState(5)
    px = 2.0 / R
    big = np.array([[-0.45, -0.45, 110.0], [0.5, 0.5, 60.0], [0.5, -0.5, 40.0], [-0.5, 0.5, 24.0]])
    lattice = (np.arange(16) + 0.5) / 8.0 - 1.0
    gx, gy = (g.ravel() for g in np.meshgrid(lattice, lattice))
    small = np.stack([gx + rs.uniform(-px, px, 256), gy + rs.uniform(-px, px, 256), rs.uniform(0.5, 14.0, 256)], axis=1)
    both = np.concatenate([big, small])
    pos = np.zeros((len(both), 3), dtype=F)
    pos[:, :2] = both[:, :2]
    h = (both[:, 2] * px / 4.0).astype(F)                # a footprint is 4 h wide
    mass = rs.uniform(0.5, 2.0, len(both)).astype(F)
    return pos, h, mass, rs.normal(size=len(both)).astype(F)


@pytest.mark.parametrize("quantity", [None, "q"])
def test_a_snapshot_on_the_reference_plane_draws_as_the_orthographic_view(golden, quantity):
    R = 256
    pos, h, mass, q = sparse_plane_snapshot(R)
    vis = topsy_amd.from_arrays(pos, h, mass, quantities={"q": q}, render_resolution=R)
    view = None
    try:
        vis.quantity_name = quantity
        vis.scale = 1.0
        view = topsy_amd.PerspectiveView(vis, fov=70.0)
        assert view.quantity_name == quantity and view.scale == 1.0
        got = view.get_image()
        vis.render_sph(DrawReason.EXPORT)
        want = vis._sph.get_image()
        st = view._sph._context.stats()
        assert st["n_small"] > 0 and st["n_mid"] > 0 and st["n_huge"] > 0 and (want[..., 0] > 0).sum() > 0.2 * R * R
        same_bits(view._sph._context.download_particles(NAMES), vis._sph._context.download_particles(NAMES), NAMES)
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want))
    finally:
        if view is not None:
            view.close()
        vis.close()


def test_a_dense_snapshot_on_the_reference_plane_differs_by_no_more_than_two_renders_of_one_context(golden):
    """Where many footprints overlap, two renders of one context already differ in the last bits (measured: some hundred of
    the 128^2 pixels of this scene, visualizer against itself), so here the resident particles are compared bit for bit and the
    images by the criterion of the chunk-culling tests: the same lit pixels, sums within 1e-5."""
    d = golden["testdata_n1000.npz"]
    pos = d["pos_smooth"][:, :3].copy()
    pos[:, 2] = 0.0
    vis = topsy_amd.from_arrays(pos, d["pos_smooth"][:, 3].copy(), d["mass"].copy(), render_resolution=128)
    view = None
    try:
        vis.scale = 12.0
        view = topsy_amd.PerspectiveView(vis, fov=70.0)
        got = view.get_image()
        vis.render_sph(DrawReason.EXPORT)
        want = vis._sph.get_image()
        same_bits(view._sph._context.download_particles(NAMES), vis._sph._context.download_particles(NAMES), NAMES)
        assert np.array_equal(got == 0, want == 0) and (want[..., 0] > 0).any() and max_rel(got, want) <= 1e-5
    finally:
        if view is not None:
            view.close()
        vis.close()


# ---- 5. the small-angle claim against exact line integrals --------------------------------------------------------------
def test_small_angle_images_against_exact_line_integrals(mips):
    """Three particles, each subtending 0.05 rad, at 32^2 and fov = 6 degrees: one on the axis on the reference plane, one at
    twice the distance (s = 1/2), one at half of it (s = 2), each with m = h^2 so that every peak is g(0).  The exact column
    density along a pixel's ray through a spherical kernel depends on the ray's impact parameter b alone: sum_j (m_j / h_j^2)
    g(b_j / h_j), g = kernel2d / pi, in float64.
      * the orthographic renderer against its own exact integrals (b = the distance in the image plane) errs by E_o of the
        peak: the error of the kernel texture and its mips;
      * the perspective image samples g at b' = the distance between the ray and the particle in the particle's plane, where
        b = b' sqrt(1 - sin^2(theta) cos^2(phi)) >= b' cos(theta), theta the ray's angle to the optical axis: |g(b/h) - g(b'/h)|
        <= max|g'| (b' - b) / h <= max|g'| (2 / cos(theta)) (1 - cos(theta)), theta at most the angle of the particle's centre
        plus its angular radius.  That is the margin for the first-order approximation.
    Measured on an MI355X: E_o = 2.07e-1 of the peak (the 8^2 mip under the 7.6 px footprint of the third particle); the margin
    is 7.8e-3 of the peak; the perspective image errs by 1.442e-1 of the peak.  A mass scaled by s instead of s^2 would lose half
    the peak of the third particle and double that of the second.  The second assertion replaces E_o by the texture error on
    the transformed particles, the footprints the perspective image is drawn with (1.444e-1): what is left is the margin."""
    R, scale, fov = 32, 1.0, 6.0
    D = perspective.fov_to_distance(scale, fov)
    h = np.array([0.0125 * D, 0.0125 * 2.0 * D, 0.0125 * 0.5 * D])                      # 4 h / d = 0.05 rad each
    zv = np.array([0.0, -D, 0.5 * D])
    d = D - zv
    plane = np.array([[0.0, 0.0], [0.45, 0.4], [-0.5, -0.45]])                        # where they are seen
    xy = plane * (d / D)[:, None]
    a = {"x": xy[:, 0].astype(F), "y": xy[:, 1].astype(F), "z": zv.astype(F), "h": h.astype(F), "mass": (h.astype(F) ** 2)}
    x, y, z, hh = (a[k].astype(np.float64) for k in ("x", "y", "z", "h"))
    w = a["mass"].astype(np.float64) / hh ** 2
    assert (4.0 * hh / (D - z) <= 0.0501).all()
    c = ((np.arange(R) + 0.5) * 2.0 / R - 1.0) * scale
    px, py = np.meshgrid(c, -c)                                                          # row 0 is the top

    def g(u):
        return kernel_lut.kernel2d(u) / np.pi

    u = np.linspace(0.0, 2.0, 20001)
    g_slope = np.abs(np.gradient(g(u), u)).max()
    exact_o = sum(w[j] * g(np.hypot(px - x[j], py - y[j]) / hh[j]) for j in range(3))
    ray = np.stack([px, py, np.full_like(px, -D)], axis=-1)
    ray /= np.linalg.norm(ray, axis=-1, keepdims=True)
    exact_p = 0.0
    for j in range(3):
        rel = np.array([x[j], y[j], z[j] - D])                                          # from the viewer at (0, 0, D)
        exact_p = exact_p + w[j] * g(np.linalg.norm(np.cross(rel, ray), axis=-1) / hh[j])
    theta = np.arctan(np.hypot(x, y) / (D - z)) + 2.0 * hh / (D - z)
    margin = float((w * g_slope * (2.0 / np.cos(theta)) * (1.0 - np.cos(theta))).sum())

    src, dst = pair(R, 2, a, mips)
    try:
        M_o = np.diag([1.0 / scale, 1.0 / scale, 1.0 / (6.0 * D), 1.0]).astype(F)
        M_o[2, 3] = 0.5
        src.render(M_o, F(1.0 / scale), mode=_native.MODE_WEIGHTED)
        ortho = src.read_image()[..., 0].astype(np.float64)
        near, far = 1e-3 * D, 2.5 * D
        src.project_perspective(dst, np.eye(3), np.zeros(3), D, near)
        M, sf = perspective.clip_matrix(scale, D, near, far)
        dst.render(M, sf, mode=_native.MODE_WEIGHTED)
        persp = dst.read_image()[..., 0].astype(np.float64)
        # ... and the orthographic renderer on the transformed particles, the footprints the perspective image is drawn with
        t = ref.project(a, np.eye(3), np.zeros(3), D, near)
        fresh = _native.Context(R, 2)
        fresh.set_kernel_mips(mips)
        fresh.upload_particles(*[t[k] for k in NAMES])
        fresh.render(M, sf, mode=_native.MODE_WEIGHTED)
        ortho_t = fresh.read_image()[..., 0].astype(np.float64)
        fresh.close()
    finally:
        src.close()
        dst.close()
    tx, ty, th = (t[k].astype(np.float64) for k in ("x", "y", "h"))
    tw = t["mass"].astype(np.float64) / th ** 2
    exact_t = sum(tw[j] * g(np.hypot(px - tx[j], py - ty[j]) / th[j]) for j in range(3))
    e_t = np.abs(ortho_t - exact_t).max()
    peak_o, peak_p = exact_o.max(), exact_p.max()
    e_o = np.abs(ortho - exact_o).max() / peak_o
    e_p = np.abs(persp - exact_p).max()
    print(f"small-angle: E_o = {e_o:.3e} of the peak, margin = {margin / peak_p:.3e} of the peak, "
          f"perspective error = {e_p / peak_p:.3e} of the peak")
    assert (persp > 0.5 * peak_p).sum() >= 3                                          # all three are drawn
    assert e_o * peak_p + margin < 0.5 * peak_p       # the bound can tell s from s^2: the third particle would lose half its peak
    assert e_p <= e_o * peak_p + margin
    # the same bound with the texture error of exactly the footprints drawn: this one is tight (the margin is what is left)
    print(f"small-angle: texture error on the transformed particles = {e_t / peak_p:.3e} of the peak")
    assert e_p <= e_t + margin


# ---- 6. states --------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_dst_as_it_was(golden, mips):
    a, rgb = snapshot(513, golden)
    cam = (np.eye(3), np.zeros(3), 30.0, 0.1)
    src, dst = pair(64, 4, a, mips)
    others = []
    try:
        M, sf = perspective.clip_matrix(8.0, 30.0, 0.1, 60.0)
        dst.render(M, sf, mode=_native.MODE_WEIGHTED)
        image_before, before = dst.read_image(), dst.download_particles(NAMES)

        def refused(source, target, match):
            with pytest.raises(_native.BackendError, match=match):
                source.project_perspective(target, *cam)

        def unchanged():
            same_bits(dst.download_particles(NAMES), before, NAMES)
            dst.render(M, sf, mode=_native.MODE_WEIGHTED)
            again = dst.read_image()
            assert np.array_equal(again == 0, image_before == 0) and max_rel(again, image_before) <= 1e-5
        # unequal n
        small = _native.Context(64, 4)
        others.append(small)
        small.upload_particles(*[a[k][:100] for k in NAMES])
        refused(small, dst, "100 particles")
        unchanged()
        # src has rgb, dst has none; src has no mass, dst has
        with_rgb = _native.Context(64, 4)
        others.append(with_rgb)
        with_rgb.upload_particles(*[a[k] for k in NAMES])
        with_rgb.upload_rgb(rgb[:, 0], rgb[:, 1], rgb[:, 2])
        refused(with_rgb, dst, "rgb")
        massless = _native.Context(64, 4)
        others.append(massless)
        massless.upload_particles(a["x"], a["y"], a["z"], a["h"], None)
        refused(massless, dst, "mass")
        unchanged()
        # a dst (or a src) without particles; src == dst
        empty = _native.Context(64, 4)
        others.append(empty)
        refused(src, empty, "dst holds no particles")
        refused(empty, dst, "src holds no particles")
        refused(dst, dst, "two contexts")
        unchanged()
        # a camera the binding would have refused, handed to the library directly
        bad = _native.perspective_struct(*cam)
        bad.near = bad.distance
        assert src._lib.tsp_project_perspective(src._h, dst._h, ctypes.byref(bad)) == -1       # TSP_EINVAL
        bad = _native.perspective_struct(*cam)
        bad.rot[4] = float("nan")
        assert src._lib.tsp_project_perspective(src._h, dst._h, ctypes.byref(bad)) == -1
        unchanged()
        # a dst on another device, where there is one
        if _native.device_count() > 1:
            far_ctx = _native.Context(64, 4, device_id=1)
            others.append(far_ctx)
            far_ctx.upload_particles(*[a[k] for k in NAMES])
            refused(src, far_ctx, "device")
        # after a projection dst is still an ordinary context: a host upload into it works and draws
        src.project_perspective(dst, *cam)
        assert not np.array_equal(bits(dst.download_particles(("x",))["x"]), bits(before["x"]))
        dst.upload_particles(*[a[k] for k in NAMES])
        unchanged()
    finally:
        for c in [src, dst] + others:
            c.close()


# ---- 7. the view --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def view20000():
    vis = topsy_amd.test(20000, render_resolution=128)
    view = topsy_amd.PerspectiveView(vis, fov=50.0)
    yield vis, view
    view.close()
    vis.close()


def reference_frame(view, W, H):
    base, layers = view._last_presentation
    return present_ref.compose(view._sph._context.read_image(), W, H, dict(base), layers)


def test_view_frame_is_composed_from_its_own_image(view20000):
    vis, view = view20000
    assert view.data_loader is vis.data_loader and np.array_equal(view.rotation_matrix, vis.rotation_matrix)
    assert np.isclose(view.distance, view.scale / np.tan(np.radians(25.0))) and np.isclose(view.near, view.distance * 1e-3)
    assert np.isclose(view.far, view.distance + view.scale)
    assert np.array_equal(view.particle_buffers.context.strata_offsets(), vis.particle_buffers.context.strata_offsets())
    W, H = 320, 240
    got = view.get_presentation_image((W, H))
    assert got.shape == (H, W, 4) and got.dtype == np.uint8
    assert np.array_equal(got, reference_frame(view, W, H))
    assert "perspective fov=50" in view._status.text
    assert view._scalebar.label.text.endswith("at the reference plane")
    y, u, v = view.get_presentation_image_yuv420((W, H))
    assert y.shape == (H, W) and u.shape == v.shape == (H // 2, W // 2)
    rgba = view.get_sph_presentation_image()
    assert rgba.shape == (128, 128, 4) and rgba.dtype == np.uint8 and rgba[..., :3].max() > 0


def test_dolly_changes_the_picture_and_refine_does_not_project_again(view20000):
    vis, view = view20000
    view.reset_view()
    first = view.get_image().copy()
    n = view.projections
    assert np.array_equal(bits(view.get_image()), bits(first)) and view.projections == n     # nothing changed: nothing projected
    offset = np.array(view.position_offset, dtype=np.float64)
    moved = view.dolly(0.5 * view.scale)
    assert np.allclose(moved - offset, np.asarray(view.rotation_matrix)[2] * 0.5 * view.scale)
    second = view.get_image()
    assert view.projections == n + 1 and not np.array_equal(first, second)
    view.draw(DrawReason.CHANGE)
    n = view.projections
    view._projected = None                        # (forget which camera dst holds: any request would now project)
    view.draw(DrawReason.REFINE)
    view.draw(DrawReason.PRESENTATION_CHANGE)
    assert view.projections == n
    view.fov = 80.0
    view.draw(DrawReason.CHANGE)
    assert view.projections == n + 1
    # the depth image is the distance from the viewer: inside (near, far) where anything was drawn
    depth = view.get_depth_image()
    seen = np.isfinite(depth)
    assert seen.any() and (depth[seen] >= view.near * (1 - 1e-5)).all() and (depth[seen] <= view.far * (1 + 1e-5)).all()
    # the visualizer's own picture is untouched by all this
    assert view.quantity_name == vis.quantity_name
    view.fov = 50.0
    view.reset_view()


def test_recorded_path_with_a_changing_fov_replays_to_the_hand_set_frames(view20000):
    vis, view = view20000
    view.reset_view()
    view.show_status = False                      # (the status line's refresh is throttled by wall-clock time)

    class Clock:
        t = 10.0

        def __call__(self):
            return self.t

    clock = Clock()
    s0 = view.scale
    keys = [(50.0, s0, 0.0), (30.0, 0.75 * s0, 0.25 * s0), (80.0, 0.5 * s0, 0.5 * s0)]
    start = np.array(view.position_offset, dtype=np.float64)
    axis = np.asarray(view.rotation_matrix, dtype=np.float64)[2]

    def set_key(fov, scale, forward):
        view.fov, view.scale, view.position_offset = fov, scale, start + axis * forward

    rec = topsy_amd.VisualizationRecorder(view, clock=clock)
    set_key(*keys[0])
    rec.record()
    for key in keys[1:]:
        clock.t += 0.5
        set_key(*key)
        rec.mark()
    clock.t += 0.5
    rec.stop()
    assert [v for _, v in rec._timestream["fov"]] == [50.0, 30.0, 80.0]
    W, H = 160, 120
    replayed, states = [], []
    for frame in rec.frames(fps=2, resolution=(W, H), smooth=False):
        replayed.append(frame)
        states.append((view.fov, view.scale, np.array(view.position_offset), np.array(view.rotation_matrix)))
    assert len(replayed) == 3
    for (fov, scale, offset, _), key in zip(states, keys):
        assert np.isclose(fov, key[0]) and np.isclose(scale, key[1]) and np.allclose(offset, start + axis * key[2])
    assert not np.array_equal(replayed[0], replayed[1]) and not np.array_equal(replayed[1], replayed[2])
    for frame, (fov, scale, offset, rotation) in zip(replayed, states):
        view.fov, view.scale, view.position_offset, view.rotation_matrix = fov, scale, offset, rotation
        by_hand = view.get_presentation_image((W, H))[..., :3]
        assert np.array_equal(frame, by_hand)
    view.show_status = True
    view.fov = 50.0
    view.reset_view()
