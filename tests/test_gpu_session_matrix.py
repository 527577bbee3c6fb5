"""One context switching between every render path, against the host model of its state (tests/session_model.py).

Every kernel family is compared with the oracle from a freshly created context elsewhere; here one context lives through every
order of the frame kinds -- the four splat modes, kinematic frames along two lines of sight, the surface pass -- and through the
other producers of an image (tsp_write_image, tsp_tile_periodic, tsp_render_undo, blocks without clear) and the changes of what is
resident.  After every producer the frame is compared with the model's expected frame (the project's tolerances for the summed
modes, bit for bit for the surface pass and the tiling), tsp_get_stats must describe that producer, every consumer the model
allows is compared bit for bit with its restatement fed the image just read back, and every call the model lists as refused must
raise with its code and leave image, statistics and a colormap of the image as they were.  tests/test_session_model_cpu.py
asserts that no frame of this scene can pass for another one of its layout, so a stale image, weight array or tag fails here."""
import numpy as np
import pytest

import kinematics_ref
import parity_scenes as ps
import postpass_ref
import present_ref
import session_model as sm
import surface_present_ref
import surface_ref
import yuv420_ref
import kinematic_present_ref as kref
from kinematic_compare import check_kinematic
from session_model import ESTATE, PRODUCERS, SPLATS

pytestmark = pytest.mark.gpu

R = sm.R
f32 = np.float32
CANVAS = (160, 96)


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


@pytest.fixture(scope="module")
def native():
    from topsy_amd import _native
    _native.load_library()
    return _native


@pytest.fixture(scope="module")
def scene():
    return sm.first_scene()


def random_lut(n, seed):
    return np.random.RandomState(seed).uniform(0, 1, (n, 4)).astype(f32)


LUT = random_lut(257, 8)
LUT2D = np.random.RandomState(9).uniform(0, 1, (16, 16, 4)).astype(f32)
SURFACE_PARAMS = dict(surface_ref.DEFAULT_PARAMS, weighted_average=True, log=False, vmin=-1.0, vmax=2.0)
TILES = (np.array([[0.0, 0.0], [0.37, -0.21], [-0.6, 0.5]], dtype=f32), np.array([1.0, 0.5, 0.25], dtype=f32))
_layers = []


def layers():
    if not _layers:
        from test_gpu_present import overlapping_layers
        _layers.append(overlapping_layers(np.random.RandomState(5)))
    return _layers[0]


class Driver:
    """The context and its model, driven together: call() asks the model whether the library must refuse the call, makes it, and
    checks that the library agrees."""

    def __init__(self, native, mips, scene=None, channels=4):
        from topsy_amd import kernel_lut
        self.native, self.mips = native, mips
        self.ctx = native.Context(R, channels)
        self.model = sm.Session(channels)
        self.M, self.sf = sm.camera()
        self.stats = {}                      # model.stats_id -> the statistics of that render
        self.ctx.set_kernel_mips(mips)
        self.ctx.set_sphere_mips(kernel_lut.sphere_mips())
        self.ctx.set_option("count_fragments", 1)
        self.ctx.colormap_set_lut2d(LUT2D)
        if scene is not None:
            self.upload_all(scene)

    def close(self):
        self.ctx.close()

    def upload_all(self, scene, attributes=None):
        a = attributes or scene
        self.call("upload_particles", scene=scene)
        self.call("upload_quantity", q=a["q"])
        self.call("upload_rgb", rgb=a["rgb"])
        self.call("upload_velocities", vel=a["vel"])

    # ---- one call on the context
    def _make(self, name, a):
        ctx, nat = self.ctx, self.native
        if name == "upload_particles":
            p = a["scene"]["pos"]
            return ctx.upload_particles(p[:, 0], p[:, 1], p[:, 2], a["scene"]["h"], a["scene"]["m"])
        if name == "upload_quantity":
            return ctx.upload_quantity(a["q"])
        if name == "upload_rgb":
            return ctx.upload_rgb(*(a["rgb"][:, k].copy() for k in range(3)))
        if name == "upload_band_magnitudes":
            return ctx.upload_band_magnitudes(a["mags"], a["weights"])
        if name == "upload_velocities":
            return ctx.upload_velocities(None) if a["vel"] is None else ctx.upload_velocities(*(a["vel"][:, k] for k in range(3)))
        if name == "set_line_of_sight":
            return ctx.set_line_of_sight(*a["los"])
        if name == "set_use_quantity":
            return ctx.set_option("use_quantity", int(a["on"]))
        if name == "reorder_spatial":
            return ctx.reorder_spatial(4, 7)
        block = a.get("block")
        starts, lens = (None, None) if block is None else ([block[0]], [block[1]])
        if name == "render":
            mode = {"density": nat.MODE_WEIGHTED, "weighted": nat.MODE_WEIGHTED, "depth": nat.MODE_DEPTH, "rgb": nat.MODE_RGB}.get(
                a["kind"], nat.MODE_KINEMATIC)
            return ctx.render(self.M, self.sf, starts, lens, clear=a.get("clear", True), mode=mode)
        if name == "render_surface":
            return ctx.render_surface(self.M, self.sf, sm.surface_cut(self.model.scene), starts, lens, clear=a.get("clear", True))
        if name == "write_image":
            return ctx.write_image(a["img"])
        if name == "tile_periodic":
            return ctx.tile_periodic(*TILES)
        if name == "render_undo":
            return ctx.render_undo()
        if name == "set_reduced_image":
            return ctx.set_reduced_image(a["img"])
        if name == "velocity_moments":
            return ctx.velocity_moments()
        if name == "colormap_moment":
            return ctx.colormap_moment(1, LUT, -300.0, 300.0)
        if name == "moment_sort":
            return ctx.moment_sort(1)
        if name == "present_moment":
            return ctx.present(*CANVAS, {"map": "moment-mean", "lut": LUT, "vmin": -300.0, "vmax": 300.0, "log": False})
        if name == "colormap_rgb":
            return ctx.colormap_rgb(-1.0, 0.5, 0.8)
        if name == "present_rgb":
            return ctx.present(*CANVAS, {"map": "rgb", "vmin": -1.0, "vmax": 0.5, "gamma": 0.8})
        if name == "content_sort":
            return ctx.content_sort(a["kind"], 3.7)
        if name == "surface_present":
            return ctx.surface_present(lut_rgba=LUT, **SURFACE_PARAMS)
        if name == "present_surface":
            return ctx.present_surface(*CANVAS, dict(SURFACE_PARAMS, lut_rgba=LUT))
        raise KeyError(name)

    def call(self, name, label="", **a):
        """-> (refused code or None, what the call returned)"""
        margs = {k: v for k, v in a.items() if k not in ("mags", "weights", "img")}
        if name == "write_image":
            margs["channels"] = a["img"].shape[2]
        code = self.model.refusal(name, **margs)
        out = None
        if code is None:
            out = self._make(name, a)
        else:
            with pytest.raises(self.native.BackendError, match=rf"libtopsy_splat error {code}:"):
                self._make(name, a)
                pytest.fail(f"{label or name} {margs.get('kind', '')}: the library accepted a call the model refuses with {code}")
        assert self.model.op(name, **margs) == code
        if name == "render_undo" and code is None:
            self.ctx.active_channels = self.model.C          # (the caller restores it: _native.Context.render_undo)
        if name in ("render", "render_surface") and code is None:
            self.stats[self.model.stats_id] = self.ctx.stats()
        return code, out

    def produce(self, kind, **a):
        """the render of one frame kind (a block of it with block=, onto the image with clear=False)"""
        if kind == "surface":
            self.call("set_use_quantity", on=True)
            return self.call("render_surface", **a)[0]
        if kind in sm.LINES_OF_SIGHT:
            self.call("set_line_of_sight", los=sm.LINES_OF_SIGHT[kind])
        self.call("set_use_quantity", on=kind != "density")
        return self.call("render", kind=kind, **a)[0]

    # ---- what the image must be
    def check_frame(self, label):
        """the image against the model's frame, and the statistics against the producer that ran; -> the image"""
        frame, ctx = self.model.frame, self.ctx
        assert ctx.active_channels == self.model.C == frame.C, label
        got = ctx.read_image()
        if not frame.complete or frame.tiled:
            return got
        want, _, terms = sm.expected(frame, self.mips)
        if frame.kind == "surface":
            assert np.array_equal(bits(got), bits(want)), (label, "the surface frame is not the restatement's bit for bit",
                                                           int((bits(got) != bits(want)).sum()))
        elif frame.kind in sm.LINES_OF_SIGHT:
            check_kinematic(got, want, terms, str(label))
        else:
            ps.compare_with_oracle(got, frame.kind, want, terms, label)
        return got

    def check_stats_of_whole_frame(self, label):
        """tsp_get_stats after a producer that drew every particle: the particle count, the oracle's exact fragment count and the
        class counts' sum for a splat, no fragment and no class count for the surface pass.  What this can tell apart: a splat
        from the surface pass, and a whole frame from a block (n_particles; the two-block test also checks both blocks' fragment
        counts).  What it cannot: two splat kinds of one scene and camera have the same counts, since the fragments depend on
        the geometry alone, so statistics left over from the splat before would pass here.  The copy in self.stats is taken
        from the same call, so that comparison says something only after tsp_render_undo, where it is the copy of an EARLIER call."""
        frame, st = self.model.frame, self.ctx.stats()
        n = len(frame.scene["h"])
        assert st == self.stats[self.model.stats_id], (label, "the statistics are not those of the last render")
        assert st["n_particles"] == n, (label, st)
        if frame.kind == "surface":
            assert st["n_fragments"] == 0 and st["n_small"] == st["n_mid"] == st["n_huge"] == 0 and 0 <= st["n_culled"] < n, (label, st)
        else:
            assert st["n_fragments"] == sm.expected(frame, self.mips)[1], (label, "fragment count", st)
            assert st["n_small"] + st["n_mid"] + st["n_huge"] + st["n_culled"] == n, (label, st)

    # ---- the consumers, bit for bit against their restatements fed the image read back
    def check_consumers(self, img, label):
        from oracle import oracle_c
        ctx = self.ctx
        W, H = CANVAS
        for name in self.model.consumers():
            tag = (label, name)
            with np.errstate(all="ignore"):
                if name == "colormap_scalar":
                    for log, weighted, vmin, vmax in ((False, False, -1.0, 2.0), (True, True, -3.0, 1.0)):
                        assert np.array_equal(ctx.colormap_scalar(LUT, vmin, vmax, log, weighted),
                                              oracle_c.colormap_scalar(img, LUT, vmin, vmax, log, weighted)), (tag, log)
                elif name == "colormap_bivariate":
                    assert np.array_equal(ctx.colormap_bivariate(-3.0, 1.0, -5.0, 5.0, True, True),
                                          oracle_c.colormap_bivariate(img, LUT2D, -3.0, 1.0, -5.0, 5.0, True, True)), tag
                elif name == "colormap_rgb":
                    assert np.array_equal(ctx.colormap_rgb(-1.0, 0.5, 0.8), oracle_c.colormap_rgb(img, -1.0, 0.5, 0.8)), tag
                    assert np.array_equal(ctx.colormap_rgb(-1.0, 0.5, 0.8, as_float=True),
                                          oracle_c.colormap_rgb(img, -1.0, 0.5, 0.8, as_float=True), equal_nan=True), tag
                elif name == "content_sort":
                    for kind in (0, 1, 3) + ((2,) if img.shape[2] == 4 else ()):
                        want, n_fin, n_nonpos = postpass_ref.content_values_ref(img, kind, 3.7)
                        assert ctx.content_sort(kind, 3.7) == (n_fin, n_nonpos), (tag, kind)
                        assert ctx.content_neg_inf() == int(np.isneginf(postpass_ref.content_all(img, kind, 3.7)).sum()), (tag, kind)
                        self.check_ranks(want, n_fin, n_nonpos, (tag, kind))
                elif name == "velocity_moments":
                    maps = kinematics_ref.velocity_moments(img)
                    assert np.array_equal(bits(ctx.velocity_moments()), bits(maps)), tag
                elif name == "colormap_moment":
                    maps = kinematics_ref.velocity_moments(img)
                    for which, lo, hi in ((1, -300.0, 300.0), (2, 0.5, 400.0)):
                        value = np.stack([maps[..., which], np.zeros((R, R), dtype=f32)], axis=-1)
                        assert np.array_equal(ctx.colormap_moment(which, LUT, lo, hi), oracle_c.colormap_scalar(value, LUT, lo, hi, False, False)), tag
                elif name == "moment_sort":
                    maps = kinematics_ref.velocity_moments(img)
                    for which, absolute in ((1, False), (1, True), (2, False)):
                        v = np.abs(maps[..., which]) if absolute else maps[..., which]
                        want, n_fin, n_nonpos = postpass_ref.content_values_ref(np.stack([v, np.ones_like(v)], axis=-1), 0, 1.0)
                        assert ctx.moment_sort(which, absolute) == n_fin and ctx.content_neg_inf() == 0, (tag, which, absolute)
                        self.check_ranks(want, n_fin, n_nonpos, (tag, which, absolute))
                elif name == "surface_present":
                    filt, rgba = ctx.surface_present(lut_rgba=LUT, **SURFACE_PARAMS)
                    want_f = surface_ref.bilateral(img, SURFACE_PARAMS["smoothing_scale"])
                    assert np.array_equal(bits(filt), bits(want_f)), tag
                    shade = {k: v for k, v in SURFACE_PARAMS.items() if k != "smoothing_scale"}
                    assert np.array_equal(rgba, surface_ref.shade(want_f, lut=LUT, **shade)), tag
                elif name == "present_surface":
                    params = dict(SURFACE_PARAMS, lut_rgba=LUT)
                    want = surface_present_ref.compose_surface(img, W, H, params, layers())
                    self.check_planes(ctx.present_surface(W, H, params, layers()), ctx.present_surface_yuv420(W, H, params, layers()), want, tag)
                else:
                    base = {"present_scalar": {"map": "scalar", "lut": LUT, "vmin": -3.0, "vmax": 1.0, "log": True, "weighted": True},
                            "present_rgb": {"map": "rgb", "vmin": -1.0, "vmax": 0.5, "gamma": 0.8},
                            "present_moment": {"map": "moment-mean", "lut": LUT, "vmin": -300.0, "vmax": 300.0, "log": False}}[name]
                    want = (kref if name == "present_moment" else present_ref).compose(img, W, H, base, layers())
                    self.check_planes(ctx.present(W, H, base, layers()), ctx.present_yuv420(W, H, base, layers()), want, tag)
            assert np.array_equal(bits(ctx.read_image()), bits(img)), (tag, "a consumer changed the image")

    def check_ranks(self, want, n_fin, n_nonpos, tag):
        """the sorted values at the ends, around n_nonpositive and at 64 seeded ranks (every rank is one 4-byte copy)"""
        if n_fin == 0:
            return
        rs = np.random.RandomState(n_fin % 65521)
        ranks = np.unique(np.concatenate([[0, 1, n_fin - 2, n_fin - 1], [n_nonpos - 1, n_nonpos], rs.randint(0, n_fin, size=64)]).clip(0, n_fin - 1))
        assert np.array_equal(bits(self.ctx.content_values(ranks)), bits(want[ranks])), tag

    @staticmethod
    def check_planes(frame, planes, want, tag):
        assert frame.shape == want.shape and np.array_equal(frame, want), (tag, int((frame != want).any(axis=-1).sum()), "pixels differ")
        for got, ref, name in zip(planes, yuv420_ref.to_yuv420(want), "YUV"):
            assert np.array_equal(got, ref), (tag, name)

    # ---- the calls that must be refused
    def check_refusals(self, img, label):
        ctx = self.ctx
        st = ctx.stats()
        rgba = ctx.colormap_scalar(LUT, -1.0, 2.0, False, False)
        seen = []
        for what, name, args, code in self.model.refused_calls():
            if name == "render" and args["kind"] in sm.LINES_OF_SIGHT:
                self.call("set_line_of_sight", los=sm.LINES_OF_SIGHT[args["kind"]])
            if name == "render":
                self.call("set_use_quantity", on=args["kind"] != "density")
            got, _ = self.call(name, label=(label, what), **args)
            assert got == code, (label, what)
            assert np.array_equal(bits(ctx.read_image()), bits(img)), (label, what, "a refused call changed the image")
            assert ctx.stats() == st, (label, what, "a refused call changed the statistics")
            seen.append(what)
        assert np.array_equal(ctx.colormap_scalar(LUT, -1.0, 2.0, False, False), rgba), (label, "the colormap after the refused calls")
        return seen

    def check_all(self, label, reduced=True):
        img = self.check_frame(label)
        self.check_consumers(img, label)
        seen = self.check_refusals(img, label)
        if reduced:
            # the image is this context's own, not a reduced one: the hand-over of a sum is accepted once, and only once
            self.call("set_reduced_image", img=img)
            with pytest.raises(self.native.BackendError, match=rf"libtopsy_splat error {ESTATE}:"):
                self.ctx.set_reduced_image(img)
            assert np.array_equal(bits(self.ctx.read_image()), bits(img)), label
        return img, seen


@pytest.fixture(scope="module")
def session(native, mips, scene):
    """the one context that lives through the whole pair matrix"""
    d = Driver(native, mips, scene)
    yield d
    print(f"session matrix: {d.model.transitions} allowed calls and {d.model.refusals} refused calls crossed on one context")
    d.close()


# --------------------------------------------------------------------------- every ordered pair of the seven producers
@pytest.mark.parametrize("a, b", sm.PAIRS, ids=[f"{a}-{b}" for a, b in sm.PAIRS])
def test_pair(session, a, b):
    d = session
    for kind in (a, b):
        assert d.produce(kind) is None
        d.check_stats_of_whole_frame((a, b, kind))
        _, seen = d.check_all((a, b, kind))
        assert seen, "no refused call in this state"
        if sm.CHANNELS[kind] == 2:
            assert "render(rgb, clear=0)" in seen and "content_sort" in seen and "velocity_moments" in seen
        else:
            assert "render(weighted, clear=0)" in seen and "surface_present" in seen
        if kind == "surface":
            assert {f"render({k}, clear=0)" for k in SPLATS} <= set(seen) and "tile_periodic" in seen and "render_undo" in seen
        else:
            assert "render_surface(clear=0)" in seen
        if kind == "rgb":
            assert "render(kinematic_a, clear=0)" in seen and "moment_sort" in seen
        if kind == "kinematic_a":
            assert "render(rgb, clear=0)" in seen and "render(kinematic_b, clear=0)" in seen and "render(kinematic_a, clear=0)" not in seen


# --------------------------------------------------------------------------- blocks without clear
PREDECESSORS = ("surface", "rgb", "weighted", "kinematic_b")


@pytest.mark.parametrize("kind", PRODUCERS)
def test_two_blocks_equal_the_whole_from_any_predecessor(native, mips, scene, kind):
    d = Driver(native, mips, scene)
    n, cut = len(scene["h"]), 700
    try:
        for pred in PREDECESSORS:
            assert d.produce(pred) is None
            assert d.produce(kind, block=(0, cut)) is None
            first = d.ctx.stats()
            d.check_refusals(d.ctx.read_image(), (pred, kind, "first block"))
            assert d.produce(kind, clear=False, block=(cut, n - cut)) is None
            assert d.model.frame.complete
            img = d.check_frame((pred, kind, "two blocks"))
            second = d.ctx.stats()
            assert first["n_particles"] == cut and second["n_particles"] == n - cut
            if kind != "surface":
                assert first["n_fragments"] + second["n_fragments"] == sm.expected(d.model.frame, mips)[1]
            d.check_consumers(img, (pred, kind, "two blocks"))
    finally:
        d.close()


# --------------------------------------------------------------------------- tsp_render_undo
@pytest.mark.parametrize("a, b", sm.PAIRS, ids=[f"{a}-{b}" for a, b in sm.PAIRS])
def test_undo_after_b_restores_a(native, mips, scene, a, b):
    """a, then b, then tsp_render_undo: valid iff b was a tsp_render that did not replace a surface image; a's frame comes back bit
    for bit with its layout, tags and statistics -- a's consumers run again, the others are refused again"""
    d = Driver(native, mips, scene)
    try:
        assert d.produce(a) is None
        img_a, st_a = d.ctx.read_image(), d.ctx.stats()
        assert d.produce(b) is None
        img_b, st_b = d.ctx.read_image(), d.ctx.stats()
        code, _ = d.call("render_undo")
        assert (code is None) == (a != "surface" and b != "surface")
        if code is None:
            assert d.ctx.active_channels == sm.CHANNELS[a] and d.model.frame.kind == a
            assert np.array_equal(bits(d.ctx.read_image()), bits(img_a)), "the frame before the render did not come back"
            assert d.ctx.stats() == st_a == d.stats[d.model.stats_id]
        else:
            assert np.array_equal(bits(d.ctx.read_image()), bits(img_b)) and d.ctx.stats() == st_b
        d.check_all((a, b, "after the undo"))
    finally:
        d.close()


@pytest.mark.parametrize("call", ["write_image", "tile_periodic", "render_surface", "reorder_spatial", "upload_quantity", "upload_rgb",
                                  "upload_velocities", "upload_band_magnitudes", "upload_particles", "set_reduced_image", "refused_render"])
def test_undo_is_refused_after_every_other_call(native, mips, scene, call):
    """include/topsy_splat.h: tsp_render_undo is valid only while tsp_render is the last call that changed the image -- no write,
    reduce, tiling, surface pass, upload or reorder since.  (A refused tsp_render counts as one that failed: valid once.)"""
    d = Driver(native, mips, scene)
    try:
        assert d.produce("weighted") is None
        img = d.ctx.read_image()
        args = {"write_image": {"img": img}, "set_reduced_image": {"img": img}, "upload_quantity": {"q": scene["q"]},
                "upload_rgb": {"rgb": scene["rgb"]}, "upload_velocities": {"vel": scene["vel"]}, "upload_particles": {"scene": scene},
                "upload_band_magnitudes": {"rgb": scene["rgb"], "mags": np.zeros((1, len(scene["h"]))), "weights": np.ones((3, 1))}}
        if call == "refused_render":
            assert d.produce("rgb", clear=False) == ESTATE
            assert d.call("render_undo")[0] is None
        else:
            assert d.call(call, **args.get(call, {}))[0] is None
        before = d.ctx.read_image()
        assert d.call("render_undo")[0] == ESTATE
        assert np.array_equal(bits(d.ctx.read_image()), bits(before))
    finally:
        d.close()


# --------------------------------------------------------------------------- tsp_tile_periodic
@pytest.mark.parametrize("kind", ["density", "weighted", "rgb", "kinematic_a"])
def test_tiling_takes_the_right_image_and_leaves_the_accumulator(native, mips, scene, kind):
    from oracle import oracle_np
    d = Driver(native, mips, scene)
    n, cut = len(scene["h"]), 700
    try:
        for pred in PREDECESSORS:
            assert d.produce(pred) is None
            assert d.produce(kind, block=(0, cut)) is None
            part = d.ctx.read_image()
            assert d.call("tile_periodic")[0] is None
            tiled = d.ctx.read_image()
            assert tiled.shape == part.shape == (R, R, sm.CHANNELS[kind])
            want = oracle_np.periodic_tile(part, *TILES)
            assert np.array_equal(bits(tiled), bits(want)), (pred, kind, int((bits(tiled) != bits(want)).sum()))
            assert not np.array_equal(bits(tiled), bits(part))
            d.check_consumers(tiled, (pred, kind, "tiled"))
            d.check_refusals(tiled, (pred, kind, "tiled"))
            # a refused render is "a render that failed": the undo forms the image again from the accumulator, which is untiled
            assert d.call("render_undo")[0] is None
            assert np.array_equal(bits(d.ctx.read_image()), bits(part)), (pred, kind, "the accumulator was tiled")
            assert d.call("tile_periodic")[0] is None
            assert np.array_equal(bits(d.ctx.read_image()), bits(want))
            # the next block continues from the untiled accumulator
            assert d.produce(kind, clear=False, block=(cut, n - cut)) is None
            d.check_frame((pred, kind, "continued after the tiling"))
    finally:
        d.close()


# --------------------------------------------------------------------------- tsp_write_image
def written_image(C, seed):
    rs = np.random.RandomState(seed)
    img = np.exp(rs.uniform(-8, 3, (R, R, C))).astype(f32)
    img[..., 1] *= rs.choice([-1.0, 1.0], (R, R)).astype(f32)
    if C == 4:
        img[..., 2] = (img[..., 1].astype(np.float64) ** 2 / img[..., 0] * rs.uniform(1.0, 3.0, (R, R))).astype(f32)
        img[..., 3] = rs.randint(0, 50, (R, R))
    else:
        img[..., 1] = np.abs(img[..., 1]) % f32(1.0)          # a depth
    return img


@pytest.mark.parametrize("pred", ["surface", "rgb", "kinematic_a"])
def test_a_written_image_replaces_any_frame_and_the_next_render_of_every_kind_is_right(native, mips, scene, pred):
    d = Driver(native, mips, scene)
    try:
        for C in (2, 4, 2):
            for kind in PRODUCERS:
                assert d.produce(pred) is None
                img = written_image(C, 7 * C + len(kind))
                assert d.call("write_image", img=img)[0] is None
                assert d.ctx.active_channels == C and np.array_equal(bits(d.ctx.read_image()), bits(img))
                # the keys are gone with a surface image, the kinematic tag stays with a kinematic one (in its 4-channel layout)
                assert d.model.keys is False and (d.model.refusal("velocity_moments") is None) == (pred == "kinematic_a" and C == 4)
                if kind == PRODUCERS[0]:                      # (the consumers and refusals of the written state: once per layout)
                    d.check_consumers(img, (pred, C, "written"))
                    d.check_refusals(img, (pred, C, "written"))
                    # a block of no particle onto the written image rounds the accumulator again: it holds the written image
                    empty_kind = "weighted" if C == 2 else ("kinematic_a" if pred == "kinematic_a" else "rgb")
                    assert d.produce(empty_kind, clear=False, block=(0, 0)) is None
                    assert np.array_equal(bits(d.ctx.read_image()), bits(img)), (pred, C, "the accumulator does not hold the written image")
                assert d.produce(kind) is None
                d.check_stats_of_whole_frame((pred, C, kind))
                d.check_frame((pred, C, kind, "after a written image"))
    finally:
        d.close()


# --------------------------------------------------------------------------- changes of what is resident
def show_every_kind(d, label, full=()):
    """every producer in turn: the model says which are refused; the others must show the attributes that are current"""
    for kind in PRODUCERS:
        code = d.produce(kind)
        if code is None:
            d.check_stats_of_whole_frame((label, kind))
            if kind in full:
                d.check_all((label, kind))
            else:
                d.check_frame((label, kind))
        else:
            assert code == sm.ESTATE, (label, kind)


def test_uploads_show_in_the_kinds_that_read_them_and_in_no_other(native, mips, scene):
    from oracle import oracle_np
    n = len(scene["h"])
    second = sm.second_attributes(n)
    d = Driver(native, mips, scene)
    try:
        show_every_kind(d, "first attributes")
        d.call("upload_quantity", q=second["q"])
        show_every_kind(d, "second quantity")
        d.call("upload_rgb", rgb=second["rgb"])
        show_every_kind(d, "second colours")
        d.call("upload_velocities", vel=second["vel"])
        show_every_kind(d, "second velocities", full=("kinematic_b",))
        rs = np.random.RandomState(5)
        mags, weights = rs.uniform(-2.5, 5.0, size=(3, n)), np.diag([0.5, 1.0, 1.0])
        d.call("upload_band_magnitudes", rgb=oracle_np.band_contraction(mags, weights), mags=mags, weights=weights)
        show_every_kind(d, "band magnitudes", full=("rgb",))
        # the velocities go: the kinematic kinds are refused, the kinematic image that is there stays one
        assert d.produce("kinematic_a") is None
        img = d.check_frame("before the velocities go")
        d.call("upload_velocities", vel=None)
        assert d.produce("kinematic_a") == ESTATE and d.produce("kinematic_b", clear=False) == ESTATE
        assert np.array_equal(bits(d.ctx.read_image()), bits(img))
        d.check_consumers(img, "a kinematic image without resident velocities")
        show_every_kind(d, "no velocities")
        d.call("upload_velocities", vel=scene["vel"])
        d.call("upload_quantity", q=scene["q"])
        show_every_kind(d, "the first velocities and quantity again")
    finally:
        d.close()


@pytest.mark.parametrize("upload", [False, True], ids=["cached", "uploaded"])
def test_the_shared_weight_arrays_follow_mode_line_of_sight_and_uploads(native, mips, scene, upload):
    """rgb -> kinematic -> rgb and kinematic A -> B -> A on one context: wr, wg, wb hold the weights of one of them at a time"""
    second = sm.second_attributes(len(scene["h"]))
    d = Driver(native, mips, scene)
    try:
        for seq, name, key in ((("rgb", "kinematic_a", "rgb"), "upload_rgb", "rgb"),
                               (("kinematic_a", "kinematic_b", "kinematic_a"), "upload_velocities", "vel"),
                               (("kinematic_b", "rgb", "kinematic_b"), "upload_velocities", "vel")):
            for step, kind in enumerate(seq):
                if upload and step == 2:
                    d.call(name, **{key: second[key]})
                assert d.produce(kind) is None
                d.check_stats_of_whole_frame((seq, step, upload))
                d.check_frame((seq, step, upload))
            if upload:
                d.call(name, **{key: scene[key]})
    finally:
        d.close()


def test_a_line_of_sight_alone_changes_no_image_but_the_next_frame(native, mips, scene):
    d = Driver(native, mips, scene)
    try:
        assert d.produce("kinematic_a", block=(0, 700)) is None
        img = d.ctx.read_image()
        d.call("set_line_of_sight", los=sm.LINES_OF_SIGHT["kinematic_b"])
        assert np.array_equal(bits(d.ctx.read_image()), bits(img))
        d.check_consumers(img, "the image along A with B set")                     # the moments of the image that is there
        assert d.call("render", kind="kinematic_b", clear=False, block=(700, 800))[0] == ESTATE
        assert d.produce("kinematic_a", clear=False, block=(700, 800)) is None      # (sets A again: the frame continues)
        d.check_frame("continued along A")
        assert d.produce("kinematic_b") is None
        d.check_all("B after A")
    finally:
        d.close()


def test_reorder_keeps_every_kind_right_and_ends_a_surface_frame(native, mips, scene):
    d = Driver(native, mips, scene)
    try:
        assert d.produce("surface", block=(0, 700)) is None
        img = d.ctx.read_image()
        d.call("reorder_spatial")
        assert np.array_equal(bits(d.ctx.read_image()), bits(img))
        assert d.call("render_surface", clear=False, block=(700, 800))[0] == ESTATE       # the keys named the old order
        assert np.array_equal(bits(d.ctx.read_image()), bits(img))
        show_every_kind(d, "after the reorder", full=("surface", "kinematic_a"))
        second = sm.second_attributes(len(scene["h"]))
        d.call("upload_velocities", vel=second["vel"])                                  # uploads arrive in the caller's order
        d.call("upload_quantity", q=second["q"])
        d.call("upload_rgb", rgb=second["rgb"])
        show_every_kind(d, "uploads after the reorder")
    finally:
        d.close()


@pytest.mark.parametrize("n", [1001, 3])
def test_fresh_particles_drop_what_belonged_to_the_old_ones(native, mips, scene, n):
    """another n: not a multiple of 4 (the tail of the kinematic weights), and below 4 (one block)"""
    fresh = sm.fresh_scene(n)
    d = Driver(native, mips, scene)
    try:
        assert d.produce("kinematic_a") is None
        img = d.check_frame("before")
        d.call("upload_particles", scene=fresh)
        assert d.ctx.num_particles == n
        assert np.array_equal(bits(d.ctx.read_image()), bits(img))
        d.check_consumers(img, "the old kinematic image after fresh particles")
        for kind in ("rgb", "kinematic_a", "kinematic_b"):
            assert d.produce(kind) == ESTATE, kind
        assert d.call("render_surface", clear=False)[0] == ESTATE
        for kind in ("density", "depth"):
            assert d.produce(kind) is None
            d.check_stats_of_whole_frame((n, kind))
            d.check_frame((n, kind))
        d.call("upload_velocities", vel=fresh["vel"])
        assert d.produce("kinematic_b") is None and d.produce("rgb") == ESTATE
        d.call("upload_quantity", q=fresh["q"])
        d.call("upload_rgb", rgb=fresh["rgb"])
        show_every_kind(d, ("fresh", n), full=("kinematic_a", "surface"))
        d.upload_all(scene)                                                          # and the first scene again
        show_every_kind(d, ("the first scene after", n))
    finally:
        d.close()


def test_attributes_and_reorder_need_particles(native, mips, scene):
    """without resident particles the uploads of attributes and the reorder are refused with TSP_ESTATE; freeing is not"""
    d = Driver(native, mips)
    n = len(scene["h"])
    try:
        empty, empty3 = np.zeros(0, dtype=f32), np.zeros((0, 3), dtype=f32)      # (the binding checks lengths against n = 0)
        for call, args in (("upload_quantity", {"q": empty}), ("upload_rgb", {"rgb": empty3}), ("upload_velocities", {"vel": empty3}),
                           ("upload_band_magnitudes", {"rgb": empty3, "mags": np.zeros((1, 0)), "weights": np.ones((3, 1))}),
                           ("reorder_spatial", {})):
            assert d.call(call, **args)[0] == ESTATE, call
        assert d.call("upload_velocities", vel=None)[0] is None
        assert d.ctx.num_particles == 0 and n > 0
    finally:
        d.close()
