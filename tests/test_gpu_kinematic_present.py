"""Kinematic frames on the GPU: the moment bases of tsp_present / tsp_present_yuv420, tsp_moment_sort, the device range of
VelocityView and the frames of VelocityFrames (a recorder's target).  Every comparison is bit for bit against the numpy
restatement (tests/kinematic_present_ref.py) of the float image the device holds."""
import ctypes

import numpy as np
import pytest

import kinematic_present_ref as kref
import kinematics_ref
import present_ref
import yuv420_ref
from test_kinematic_present_cpu import BASES, base_id, hand_made_image, make_lut

pytestmark = pytest.mark.gpu

f32 = np.float32
EINVAL, ESTATE, ENOMEM = -1, -4, -6
VIEW = 16.0
TILTED = np.array([[1.0, 0.0, 0.0], [0.0, 0.5, np.sqrt(0.75)], [0.0, -np.sqrt(0.75), 0.5]])     # 60 degrees from face-on, about x


@pytest.fixture(scope="module")
def native():
    from topsy_amd import _native
    _native.load_library()
    return _native


def disc(n=2000, seed=4, omega=16.0):
    """A thin disc of radius 10 in the xy plane in solid-body rotation with a little random motion: (pos, h, m, vel).  At
    half-width VIEW it leaves the corners of the image empty."""
    rs = np.random.RandomState(seed)
    r, phi = 10.0 * np.sqrt(rs.uniform(0, 1, n)), rs.uniform(0, 2 * np.pi, n)
    pos = np.stack([r * np.cos(phi), r * np.sin(phi), rs.normal(0, 0.2, n)], axis=1).astype(f32)
    h = np.exp(rs.uniform(np.log(0.15), np.log(1.5), n)).astype(f32)
    m = rs.uniform(0.5, 2.0, n).astype(f32)
    vel = (np.stack([-omega * pos[:, 1], omega * pos[:, 0], np.zeros(n)], axis=1) + rs.normal(0, 15.0, (n, 3))).astype(f32)
    return pos, h, m, vel


def kinematic_context(native, R, channels=4):
    """A context whose last render was kinematic (the state a written image keeps): one particle, drawn once."""
    from oracle import oracle_np
    from topsy_amd import kernel_lut
    ctx = native.Context(R, channels)
    ctx.set_kernel_mips(kernel_lut.kernel_mips())
    one, zero = np.ones(1, dtype=f32), np.zeros(1, dtype=f32)
    ctx.upload_particles(zero, zero, zero, one, one)
    ctx.upload_velocities(one, zero, zero)
    ctx.set_line_of_sight(np.array([0.0, 0.0, 1.0]), np.zeros(3))
    M, sf = oracle_np.transform_matrix(np.eye(3), np.zeros(3), 10.0)
    ctx.render(M, sf, mode=native.MODE_KINEMATIC)
    return ctx


_contexts = {}


@pytest.fixture(scope="module")
def written(native):
    """written(R) -> (context holding hand_made_image(R) as a kinematic image, the image); one context per R for the module"""
    def get(R):
        if R not in _contexts:
            ctx = kinematic_context(native, R)
            img, _ = hand_made_image(R)
            ctx.write_image(img)
            _contexts[R] = (ctx, img)
        return _contexts[R]
    yield get
    for ctx, _ in _contexts.values():
        ctx.close()
    _contexts.clear()


def layers_of(with_layers):
    """a quad, an instanced quad and two line sets, overlapping and semi-transparent (test_gpu_present.overlapping_layers)"""
    from test_gpu_present import overlapping_layers
    return overlapping_layers(np.random.RandomState(5)) if with_layers else []


# --------------------------------------------------------------------------- tsp_present with the moment bases
@pytest.mark.parametrize("with_layers", [False, True], ids=["bare", "layers"])
@pytest.mark.parametrize("canvas", ["R", (96, 64), (64, 96), (200, 120), (40, 24), (17, 9), (1, 1)], ids=str)
@pytest.mark.parametrize("R", [64, 33])
def test_present_equals_the_reference(written, R, canvas, with_layers):
    ctx, img = written(R)
    W, H = (R, R) if canvas == "R" else canvas
    layers = layers_of(with_layers)
    for base in BASES:                                  # the mean, sigma, and sigma on a log scale
        got = ctx.present(W, H, base, layers)
        want = kref.compose(img, W, H, base, layers)
        assert got.shape == (H, W, 4) and got.dtype == np.uint8
        assert np.array_equal(got, want), f"{base_id(base)}: {np.count_nonzero((got != want).any(axis=-1))} of {W * H} pixels differ"
        if canvas == "R" and not with_layers:
            which = kref.CHANNEL[base["map"]]
            assert np.array_equal(got, ctx.colormap_moment(which, base["lut"], base["vmin"], base["vmax"], base["log"])), base_id(base)
    assert np.array_equal(ctx.read_image().view(np.uint32), img.view(np.uint32))


@pytest.mark.parametrize("W, H", [(96, 64), (70, 46), (2, 2)])
@pytest.mark.parametrize("R", [64, 33])
def test_yuv420_planes_are_the_converted_frame(written, R, W, H):
    ctx, img = written(R)
    layers = layers_of(True)
    for base in BASES:
        planes = ctx.present_yuv420(W, H, base, layers)
        want = yuv420_ref.to_yuv420(kref.compose(img, W, H, base, layers))
        for got, ref, name in zip(planes, want, "YUV"):
            assert got.shape == ref.shape and np.array_equal(got, ref), (base_id(base), name)


def raw_present(native, ctx, W, H, base, out, yuv420=False):
    """the raw entry point: (return code, error text)"""
    lib = native.load_library()
    b, arr, _keep = native.Context._present_args(base, [])
    entry = lib.tsp_present_yuv420 if yuv420 else lib.tsp_present
    rc = entry(ctx._h, W, H, ctypes.byref(b), arr, 0, out.ctypes.data_as(entry.argtypes[6]), None)
    return rc, lib.tsp_last_error().decode(errors="replace")


def test_refused_calls_write_nothing(native, written):
    from oracle import oracle_np
    from topsy_amd import kernel_lut
    rs = np.random.RandomState(3)
    good_scalar = {"map": "scalar", "lut": make_lut(16), "vmin": 0.0, "vmax": 2.0, "log": False, "weighted": False}
    M, sf = oracle_np.transform_matrix(np.eye(3), np.zeros(3), 10.0)

    # a density image, and an rgb image: not kinematic
    density = native.Context(64, 2)
    rgb = native.Context(64, 4)
    try:
        img2 = rs.uniform(0.1, 2.0, (64, 64, 2)).astype(f32)
        density.write_image(img2)
        rgb.set_kernel_mips(kernel_lut.kernel_mips())
        x = rs.uniform(-5, 5, 50).astype(f32)
        rgb.upload_particles(x, x[::-1].copy(), np.zeros(50, dtype=f32), np.ones(50, dtype=f32), np.ones(50, dtype=f32))
        rgb.upload_rgb(*(rs.uniform(0.1, 1.0, 50).astype(f32) for _ in range(3)))
        rgb.render(M, sf, mode=native.MODE_RGB)
        img4 = rgb.read_image()
        assert img4.shape == (64, 64, 4) and np.count_nonzero(img4[..., 0]) > 100
        for ctx, img, good in ((density, img2, good_scalar), (rgb, img4, {"map": "rgb", "vmin": -1.0, "vmax": 0.5, "gamma": 0.8})):
            for base in BASES[:2]:
                for yuv420 in (False, True):
                    out = np.full(40 * 30 * 4, 77, dtype=np.uint8)
                    rc, err = raw_present(native, ctx, 40, 30, base, out, yuv420)
                    assert rc == ESTATE and "kinematic" in err, (rc, err)
                    assert (out == 77).all()
                    assert np.array_equal(ctx.read_image().view(np.uint32), img.view(np.uint32))
            n = ctypes.c_int64(-7)
            for which in (1, 2):
                assert native.load_library().tsp_moment_sort(ctx._h, which, 0, ctypes.byref(n)) == ESTATE and n.value == -7
            assert np.array_equal(ctx.present(40, 30, good), present_ref.compose(img, 40, 30, good, []))
    finally:
        density.close()
        rgb.close()

    # a kinematic image, bad arguments
    ctx, img = written(64)
    base = BASES[0]
    short = dict(base, lut=make_lut(1))
    for b, W, H, yuv420 in ((short, 40, 30, False), (short, 40, 30, True), (base, 41, 30, True), (base, 40, 31, True),
                            (base, 0, 30, False), (base, 40, 16385, False)):
        out = np.full(41 * 31 * 4, 77, dtype=np.uint8)
        rc, err = raw_present(native, ctx, W, H, b, out, yuv420)
        assert rc == EINVAL, (W, H, yuv420, rc, err)
        assert (out == 77).all()
        assert np.array_equal(ctx.read_image().view(np.uint32), img.view(np.uint32))
        assert np.array_equal(ctx.present(40, 30, base), kref.compose(img, 40, 30, base))
    lib = native.load_library()
    n = ctypes.c_int64(-7)
    assert lib.tsp_moment_sort(ctx._h, 0, 0, ctypes.byref(n)) == EINVAL and lib.tsp_moment_sort(ctx._h, 3, 1, ctypes.byref(n)) == EINVAL
    assert lib.tsp_moment_sort(ctx._h, 1, 0, None) == EINVAL and lib.tsp_moment_sort(None, 1, 0, ctypes.byref(n)) == EINVAL
    assert n.value == -7


# --------------------------------------------------------------------------- tsp_moment_sort
@pytest.mark.parametrize("R", [1, 2, 33, 256])
def test_moment_sort_gives_the_order_statistics_of_the_maps(written, R):
    ctx, img = written(R)
    maps = kinematics_ref.velocity_moments(img)
    stats = ctx.stats()
    for which in (1, 2):
        for absolute in (False, True):
            v = maps[..., which].ravel()
            v = np.abs(v) if absolute else v
            want = np.sort(v[np.isfinite(v)])
            n = ctx.moment_sort(which, absolute)
            assert n == len(want), (which, absolute)
            got = ctx.content_values(np.arange(n))
            assert np.array_equal(got, want), (which, absolute)
            assert np.array_equal(np.signbit(got), np.signbit(want))
            assert ctx.content_neg_inf() == 0
            with pytest.raises(Exception):
                ctx.content_values([n])
    if R >= 33:
        assert 0 < n < R * R
    assert np.array_equal(ctx.read_image().view(np.uint32), img.view(np.uint32)) and ctx.stats() == stats
    # a content sort afterwards is what it was
    nf, _ = ctx.content_sort(0)
    S = img[..., 0].ravel()
    assert np.array_equal(ctx.content_values(np.arange(nf)), np.sort(S[np.isfinite(S)]))


# --------------------------------------------------------------------------- the view
@pytest.fixture(scope="module", params=[64, 33])
def disc_view(request):
    import topsy_amd
    pos, h, m, vel = disc()
    vis = topsy_amd.from_arrays(pos, h, m, vel=vel, render_resolution=request.param)
    vis.scale = VIEW
    vis.rotation_matrix = TILTED
    view = topsy_amd.VelocityView(vis, v_ref=None)
    yield vis, view, request.param
    vis.close()


def reset(vis, view):
    vis.scale, vis.rotation_matrix, vis.position_offset = VIEW, TILTED, np.zeros(3)
    for kind in ("v_los", "sigma_los"):
        view[kind, "vmin"] = view[kind, "vmax"] = None
        fr = view.frames(kind)
        fr.show_colorbar = fr.show_scalebar = fr.show_status = True
        fr.crosshairs_visible = False


def test_device_range_is_the_host_rule(disc_view):
    from topsy_amd import kinematics
    vis, view, R = disc_view
    reset(vis, view)
    maps = view.get_maps()
    assert np.isnan(maps["v_los"]).sum() > R and np.isfinite(maps["v_los"]).sum() > R * R // 4      # empty corners, a drawn disc
    for kind in kinematics.KINDS:
        got = view.get_range(kind)
        assert got == kinematics.resolve_range(kind, view.get_maps()[kind]), kind
        assert got[1] > got[0] and got != ((-1.0, 1.0) if kind == "v_los" else (0.0, 1.0))
    view["sigma_los", "vmin"] = 2.5
    view["v_los", "vmax"] = 70.0
    assert view.get_range("sigma_los") == kinematics.resolve_range("sigma_los", view.get_maps()["sigma_los"], vmin=2.5)
    assert view.get_range("sigma_los")[0] == 2.5 and view.get_range("v_los") == (-70.0, 70.0)
    reset(vis, view)
    vis.position_offset = np.array([1000.0, 0.0, 0.0])          # a camera looking at empty space
    assert not np.isfinite(view.get_maps()["v_los"]).any()
    for kind in kinematics.KINDS:
        assert view.get_range(kind) == kinematics.resolve_range(kind, view.get_maps()[kind]) == \
            ((-1.0, 1.0) if kind == "v_los" else (0.0, 1.0))
    reset(vis, view)


def reference_frame(view, kind, W, H):
    base, layers = view.frames(kind)._last_presentation
    return kref.compose(view._sph._context.read_image(), W, H, base, layers)


@pytest.mark.parametrize("kind", ["v_los", "sigma_los"])
def test_frames_equal_the_reference(disc_view, kind):
    from topsy_amd import kinematics
    vis, view, R = disc_view
    reset(vis, view)
    fr = view.frames(kind)
    fr.display_status("frame test", timeout=600)
    for W, H in ((160, 90), (R, R)):
        got = fr.get_presentation_image((W, H))
        base, layers = fr._last_presentation
        assert got.shape == (H, W, 4) and got.dtype == np.uint8
        assert base["map"] == ("moment-mean" if kind == "v_los" else "moment-sigma")
        assert (base["vmin"], base["vmax"]) == tuple(f32(v) for v in kinematics.resolve_range(kind, view.get_maps()[kind]))
        if (W, H) == (160, 90):
            assert len(layers) == 4                                 # colorbar, scale-bar label, bar, status line
        assert np.array_equal(got, reference_frame(view, kind, W, H)), (W, H)
        bare = view._sph._context.present(W, H, base, [])
        assert (got != bare).any() and len(np.unique(bare.reshape(-1, 4), axis=0)) > 10
    # without layers the square frame is the view's own presentation image
    fr.show_colorbar = fr.show_scalebar = fr.show_status = False
    got = fr.get_presentation_image((R, R))
    assert fr._last_presentation[1] == [] and np.array_equal(got, view.get_presentation_image(kind))
    reset(vis, view)


def test_the_shared_target_is_redrawn_both_ways(disc_view):
    vis, view, R = disc_view
    reset(vis, view)
    fr = view.frames("v_los")
    fr.display_status("shared target", timeout=600)
    first = fr.get_presentation_image((96, 64))
    assert np.array_equal(first, reference_frame(view, "v_los", 96, 64))
    density = vis.get_presentation_image((96, 64))                  # the visualizer's own frame, on the same target
    base, layers = vis._last_presentation
    image = vis._sph._context.read_image()
    assert image.shape == (R, R, 2) and np.array_equal(density, present_ref.compose(image, 96, 64, base, layers))
    assert not np.array_equal(density, first)
    again = fr.get_presentation_image((96, 64))                     # ... and the kinematic frame again
    assert view._sph._context.read_image().shape == (R, R, 4)
    assert np.array_equal(again, reference_frame(view, "v_los", 96, 64))
    assert np.mean((again != first).any(axis=-1)) < 0.02            # two renders of one scene: the same picture to the rounding
    y, u, v = view.frames("sigma_los").get_presentation_image_yuv420((96, 64))
    want = yuv420_ref.to_yuv420(reference_frame(view, "sigma_los", 96, 64))
    assert all(np.array_equal(a, b) for a, b in zip((y, u, v), want))


@pytest.mark.parametrize("pixel_format", ["rgb24", "yuv420p"])
def test_recorder_replays_a_quarter_turn(disc_view, pixel_format):
    import topsy_amd
    from topsy_amd.recorder import RotationInterpolator
    vis, view, R = disc_view
    reset(vis, view)
    fr = view.frames("v_los")
    now = [0.0]
    rec = topsy_amd.VisualizationRecorder(fr, clock=lambda: now[0])
    edge_on = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]])
    vis.rotation_matrix = np.eye(3)
    fr.colormap_autorange()
    pinned = (view["v_los", "vmin"], view["v_los", "vmax"])
    rec.record()
    now[0] = 1.0
    vis.rotation_matrix = edge_on
    rec.mark()
    rec.stop()
    vis.rotation_matrix = np.eye(3)
    seen = []

    def capture(frames):
        """after every frame: the state it was drawn at, and the frame composed directly from what the device holds"""
        base, layers = frames._last_presentation
        direct = kref.compose(view._sph._context.read_image(), 64, 48, base, layers)
        seen.append((np.array(vis.rotation_matrix), (base["vmin"], base["vmax"]), direct))
    fr.add_frame_listener(capture)
    try:
        got = list(rec.frames(fps=4.0, resolution=(64, 48), smooth=False, pixel_format=pixel_format))
    finally:
        fr.remove_frame_listener(capture)
    assert len(got) == len(seen) == 4
    turn = RotationInterpolator([(0.0, np.eye(3)), (1.0, edge_on)])
    for i, (frame, (rotation, ends, direct)) in enumerate(zip(got, seen)):
        assert np.allclose(rotation, turn(i / 4.0), atol=1e-12) and ends == (f32(pinned[0]), f32(pinned[1])), i
        if pixel_format == "rgb24":
            assert frame.shape == (48, 64, 3) and np.array_equal(frame, direct[..., :3]), i
        else:
            assert all(np.array_equal(a, b) for a, b in zip(frame, yuv420_ref.to_yuv420(direct))), i
    assert not np.array_equal(seen[0][2], seen[3][2])               # face-on shows the random motion only, later frames the rotation
    reset(vis, view)


def test_a_dispersion_movie_is_written(disc_view, tmp_path):
    import topsy_amd
    from topsy_amd.recorder import y4m_header
    vis, view, R = disc_view
    reset(vis, view)
    fr = view.frames("sigma_los")
    now = [0.0]
    rec = topsy_amd.VisualizationRecorder(fr, clock=lambda: now[0])
    rec.record()
    now[0] = 0.5
    vis.rotation_matrix = np.eye(3)
    rec.mark()
    rec.stop()
    path = tmp_path / "turn.y4m"
    rec.save_y4m(path, 4, (64, 48))
    data = path.read_bytes()
    header = y4m_header(64, 48, 4)
    assert data.startswith(header) and len(data) == len(header) + 2 * (len(b"FRAME\n") + 64 * 48 * 3 // 2)
    last = np.frombuffer(data[-(64 * 48 * 3 // 2):], dtype=np.uint8)
    want = yuv420_ref.to_yuv420(reference_frame(view, "sigma_los", 64, 48))        # the device still holds the last frame's image
    assert np.array_equal(last, np.concatenate([p.ravel() for p in want]))
    reset(vis, view)


# --------------------------------------------------------------------------- failed allocations
@pytest.mark.parametrize("yuv420", [False, True])
def test_failed_allocations_of_a_moment_frame(native, yuv420):
    from test_gpu_scratch_alloc_failure import H, SCRATCH_SITES, W, Outputs, assert_frame, frame_buffer, walk
    lib = native.load_library()
    img, _ = hand_made_image(33)
    layers = layers_of(True)
    ctx = kinematic_context(native, 33)
    try:
        ctx.write_image(img)
        for base in BASES[:2]:
            b, arr, _keep = native.Context._present_args(base, layers)
            entry = lib.tsp_present_yuv420 if yuv420 else lib.tsp_present
            outs = Outputs(frame=frame_buffer(yuv420), ms=ctypes.c_double())
            walk(native, ctx, lambda: entry(ctx._h, W, H, ctypes.byref(b), arr, len(layers), outs.frame.ctypes.data_as(entry.argtypes[6]),
                                            ctypes.byref(outs.ms)),
                 outs, SCRATCH_SITES[("present_yuv420" if yuv420 else "present", True)])
            assert_frame(outs.frame, kref.compose(img, W, H, base, layers), yuv420)
    finally:
        ctx.close()


def test_failed_allocations_of_a_moment_sort(native):
    from test_gpu_scratch_alloc_failure import Outputs, walk
    lib = native.load_library()
    img, _ = hand_made_image(33)
    want = np.sort(np.abs(kinematics_ref.velocity_moments(img)[..., 1][np.isfinite(kinematics_ref.velocity_moments(img)[..., 1])]))
    ctx = kinematic_context(native, 33)
    try:
        ctx.write_image(img)
        outs = Outputs(n=ctypes.c_int64())
        reached = walk(native, ctx, lambda: lib.tsp_moment_sort(ctx._h, 1, 1, ctypes.byref(outs.n)), outs,
                       {"sort_keys", "sort_keys_alt", "sort_tmp"})
        assert reached == ["sort_keys", "sort_keys_alt", "sort_tmp"]
        assert outs.n.value == len(want) and np.array_equal(ctx.content_values(np.arange(len(want))), want)
        # the buffers are there now: a second sort allocates nothing, so an injection armed for it is still armed afterwards
        ctx.set_option("debug_fail_alloc", 1)
        assert ctx.moment_sort(2) == np.isfinite(kinematics_ref.velocity_moments(img)[..., 2]).sum()
        ctx.set_option("debug_fail_alloc", 0)
    finally:
        ctx.close()
