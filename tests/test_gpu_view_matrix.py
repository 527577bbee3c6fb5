"""The Python layer's views of one visualizer after one another, in every order.

SPH / BivariateSPH / RGBSPH, the depth query (DepthSPH), SurfaceView (DepthSPHWithOcclusion) and VelocityView (KinematicSPH) share
one device render target and decide by particle_buffers.last_renderer (SPH._target_is_mine) whether the frame in it is theirs to
refine or to present again.  ONE visualizer lives through the whole matrix, with one long-lived SurfaceView and VelocityView: its
three scene views -- weighted, bivariate, rgb -- are reached by switching vis.render_mode, which replaces vis._sph under the views
that were made with the old renderer.  For every ordered pair of the six views the first is drawn, then the second is asked for
its frame with DrawReason.CHANGE, PRESENTATION_CHANGE and REFINE (the latter also after a first frame that is partial and needs
refining): the image must be the second view's own frame for its own camera (the oracle's, at the tolerances of the session
matrix; the surface frame bit for bit), and the view must redraw exactly when the target is not its own -- the returned flag and
last_render_blocks.  The scene and the distinctness of its frames are those of tests/session_model.py."""
import numpy as np
import pytest

import parity_scenes as ps
import session_model as sm
import surface_ref
from kinematic_compare import check_kinematic, oracle_kinematic

pytestmark = pytest.mark.gpu

R = sm.R
f32 = np.float32
SCENE_MODES = {"weighted": "univariate", "bivariate": "bivariate", "rgb": "rgb"}      # scene view -> vis.render_mode
VIEWS = ("weighted", "bivariate", "rgb", "depth", "surface", "velocity")
REASONS = ("CHANGE", "PRESENTATION_CHANGE", "REFINE", "REFINE_PARTIAL")


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


class Views:
    def __init__(self, scene):
        import topsy_amd
        self.scene = scene
        self.vis = topsy_amd.from_arrays(scene["pos"], scene["h"], scene["m"], quantities={"q": scene["q"]}, rgb=scene["rgb"],
                                         vel=scene["vel"], render_resolution=R)
        self.vis.scale = sm.SCALE
        self.vis.quantity_name = "q"
        self.surface = topsy_amd.SurfaceView(self.vis)
        self.velocity = topsy_amd.VelocityView(self.vis, v_ref=sm.V_BULK.astype(np.float64))
        self.ctx = self.vis.particle_buffers.context
        self.switches = 0
        self._resident = None

    def close(self):
        self.vis.close()

    def ensure_mode(self, view):
        """the scene views are render modes of the one visualizer: a switch replaces vis._sph (the views keep theirs).  -> whether
        it switched.  The switch autoranges, which draws: afterwards the new renderer is marked stale and owns nothing."""
        if view not in SCENE_MODES or self.vis.render_mode == SCENE_MODES[view]:
            return False
        old = self.vis._sph
        self.vis.render_mode = SCENE_MODES[view]
        new = self.vis._sph
        self.switches += 1
        assert new is not old and self.vis.render_mode == SCENE_MODES[view]
        assert (new.scale, new.rotation_matrix.tolist(), list(new.position_offset)) == (old.scale, old.rotation_matrix.tolist(),
                                                                                        list(old.position_offset))
        for r in (new, old, self.surface._sph, self.velocity._sph):
            assert not r._target_is_mine(), "after a change of mode no renderer may take the target for its own"
        return True

    def renderer(self, view):
        if view in ("surface", "velocity"):
            return (self.surface if view == "surface" else self.velocity)._sph
        return self.vis._sph               # (the depth query runs on a renderer of its own with the scene's camera)

    def draw(self, view, reason):
        """-> whether the view says it drew"""
        self.ensure_mode(view)
        if view in SCENE_MODES:
            return self.vis._sph.render(reason)
        if view == "depth":
            depth = self.vis._sph.get_depth_image(reason)
            assert depth.shape == (R, R)
            return True
        return (self.surface if view == "surface" else self.velocity).render(reason)

    def resident(self):
        """the particles and q in the resident order (the surface pass breaks ties by the resident index)"""
        if self._resident is None:
            self._resident = self.ctx.download_particles(("x", "y", "z", "h", "mass", "q"))
        return self._resident

    def check(self, view, mips, label):
        """the image in the target is the frame of `view` for its own camera"""
        got = self.ctx.read_image()
        rend = self.renderer(view)
        M, sf = rend._get_transform_params()
        assert rend.last_render_mass_scale == 1.0 or view == "depth", label
        sc = self.scene
        if view == "surface":
            d = self.resident()
            want, winner = surface_ref.occlusion(np.column_stack([d["x"], d["y"], d["z"], d["h"]]), d["mass"], d["q"], M, sf, R,
                                                 rend.density_cut(), surface_ref.sphere_mips())
            assert (winner >= 0).sum() > 1000
            assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (label, "surface frame")
        elif view == "velocity":
            axis = rend.line_of_sight().astype(f32)
            want, _, terms = oracle_kinematic(sc, mips, M, sf, axis, sm.V_BULK)
            check_kinematic(got, want, terms, str(label))
        else:
            kind = {"depth": "depth", "rgb": "rgb"}.get(view, "weighted")
            assert type(rend).__name__ == ("RGBSPH" if self.vis.render_mode == "rgb" else "SPH"), label
            want, _, terms = ps.oracle_images(kind, sc, M, sf, R, mips)
            assert got.shape == want.shape, (label, got.shape)
            ps.compare_with_oracle(got, kind, want, terms, label)
        return got


@pytest.fixture(scope="module")
def views():
    v = Views(sm.first_scene())
    yield v
    print(f"view matrix: {v.switches} changes of the render mode on one visualizer")
    v.close()


def make_partial(rend):
    """the renderer's next CHANGE frame draws a prefix of the strata only (test_gpu_visualizer.py); -> the undo"""
    rp, timer = rend._render_progression, rend._render_timer
    saved = (rp._recommended_num_particles_to_render, timer.add_block)
    real_add = timer.add_block
    rp._recommended_num_particles_to_render = 400
    timer.add_block = lambda ms, wall_seconds=None: real_add(40.0)

    def undo():
        rp._recommended_num_particles_to_render, timer.add_block = saved
    return undo


# (the depth query and the surface pass draw every particle in one frame: after them there is nothing to refine)
CASES = [(a, b, r) for a in VIEWS for b in VIEWS for r in REASONS if not (r == "REFINE_PARTIAL" and a in ("depth", "surface"))]


@pytest.mark.parametrize("first, second, reason", CASES, ids=["-".join(c) for c in CASES])
def test_second_view_after_first(views, mips, first, second, reason):
    from topsy_amd.drawreason import DrawReason
    v = views
    label = (first, second, reason)
    undo = None
    v.ensure_mode(first)
    if reason == "REFINE_PARTIAL":
        undo = make_partial(v.renderer(first))
    try:
        assert v.draw(first, DrawReason.CHANGE) is True
        first_rend = v.renderer(first)
        if undo is not None:
            assert first_rend.needs_refine(), "the first frame is not partial"
        first_image = v.ctx.read_image()
        own = first == second and first != "depth"            # (every depth query is a renderer of its own)
        switched = v.ensure_mode(second)                    # (asking a scene view of another mode begins with the switch)
        rend = v.renderer(second)
        if first in SCENE_MODES and second in SCENE_MODES:
            assert switched == (first != second) and (rend is first_rend) == (first == second), label
        if second != "depth":
            assert rend._target_is_mine() == own, label
        blocks_before = getattr(rend, "last_render_blocks", None)
        drew = v.draw(second, getattr(DrawReason, reason.split("_PARTIAL")[0]))
        if reason == "PRESENTATION_CHANGE" and own:
            assert drew is False and rend.last_render_blocks == blocks_before
            assert np.array_equal(bits(v.ctx.read_image()), bits(first_image)), (label, "a presentation change redrew its own frame")
        else:
            assert drew is True, label
        if reason == "REFINE_PARTIAL" and own:
            while rend.needs_refine():                          # its own partial frame: the refinement completes it
                assert v.draw(second, DrawReason.REFINE) is True
        elif not own and second != "depth":
            assert rend.last_render_blocks >= 1, (label, "another view's frame was refined or presented again")
        if second != "depth":
            assert not rend.needs_refine() and rend._target_is_mine(), label
            assert v.vis.particle_buffers.last_renderer is rend, label
        v.check(second, mips, label)
    finally:
        if undo is not None:
            undo()


def periodic_visualizer(sc):
    import topsy_amd
    vis = topsy_amd.from_arrays(sc["pos"], sc["h"], sc["m"], quantities={"q": sc["q"]}, vel=sc["vel"], render_resolution=R,
                                periodic_tiling=True, periodicity_scale=150.0)
    vis.scale = sm.SCALE
    vis.quantity_name = "q"
    return vis


def test_views_a_periodic_visualizer_cannot_have():
    """a periodic visualizer that carries velocities: both views refuse it for its tiling, as they document"""
    import topsy_amd
    per = periodic_visualizer(sm.first_scene())
    try:
        assert per.data_loader.get_velocities() is not None
        with pytest.raises(NotImplementedError, match="SurfaceView has no periodic tiling"):
            topsy_amd.SurfaceView(per)
        with pytest.raises(NotImplementedError, match="VelocityView has no periodic tiling"):
            topsy_amd.VelocityView(per)
    finally:
        per.close()


def test_periodic_scene_and_depth_query_in_every_order(mips):
    """the periodic visualizer's own frame is tiled; a depth query leaves an untiled depth frame, after which the scene is
    redrawn and tiled again whatever the draw reason, also when the frame before the query was partial"""
    from oracle import oracle_np
    from topsy_amd import periodic_sph
    from topsy_amd.drawreason import DrawReason
    sc = sm.first_scene()
    vis = periodic_visualizer(sc)
    try:
        ctx, rend = vis.particle_buffers.context, vis._sph
        off, w = periodic_sph.instance_offsets_and_weights(rend.rotation_matrix, vis.periodicity_scale / vis.scale, rend.num_repetitions)
        M, sf = rend._get_transform_params()
        want, _, terms = ps.oracle_images("weighted", dict(sc, rgb=None), M, sf, R, mips)
        want_depth, _, _ = ps.oracle_images("depth", dict(sc, rgb=None), M, sf, R, mips)

        def check_tiled(label):
            """The complete tiled frame: its untiled form within the project's tolerance of the oracle's, the tiling bit for bit.
            The untiled form is recovered below the renderer: a block of no particle forms the float32 image again from the
            accumulator, which the tiling never touches, and the same tiling is then applied again.  The target afterwards holds
            the renderer's own frame bit for bit (asserted), so its has_rendered and last_renderer, which this does not touch,
            are as truthful as before."""
            assert rend.last_render_mass_scale == 1.0 and not rend.needs_refine() and rend._target_is_mine(), label
            tiled = ctx.read_image()
            ctx.render(M, sf, [0], [0], clear=False)
            untiled = ctx.read_image()
            ps.compare_with_oracle(untiled, "weighted", want, terms, label)
            assert np.array_equal(bits(tiled), bits(oracle_np.periodic_tile(untiled, off, w))), (label, "tiling")
            ctx.tile_periodic(off, w)
            assert np.array_equal(bits(ctx.read_image()), bits(tiled)), (label, "the frame was not put back")

        def depth_query(label):
            depth = vis.get_depth_image()
            assert depth.shape == (R, R) and not rend._target_is_mine()
            ps.compare_with_oracle(ctx.read_image(), "depth", want_depth, None, label)

        for reason in (DrawReason.CHANGE, DrawReason.PRESENTATION_CHANGE, DrawReason.REFINE):
            assert rend.render(DrawReason.CHANGE) is True
            check_tiled(("scene", reason))
            assert rend.render(DrawReason.PRESENTATION_CHANGE) is False
            depth_query(("depth after the tiled scene", reason))
            assert rend.render(reason) is True and rend.last_render_blocks >= 1, reason
            check_tiled(("scene after the depth query", reason))

        # a partial frame, refined to the end: every refinement continues from the untiled accumulator and tiles again
        undo = make_partial(rend)
        try:
            vis.invalidate()
            assert rend.render(DrawReason.CHANGE) is True and rend.needs_refine() and rend.last_render_mass_scale > 1.0
            frames = 1
            while rend.needs_refine():
                assert rend.render(DrawReason.REFINE) is True
                frames += 1
            assert frames > 1
            check_tiled("refined to the end")
            # ... and a depth query in the middle of it: the REFINE that follows starts the scene again
            vis.invalidate()
            assert rend.render(DrawReason.CHANGE) is True and rend.needs_refine()
            depth_query("depth after a partial tiled scene")
            assert rend.render(DrawReason.REFINE) is True and rend.last_render_blocks >= 1 and rend._target_is_mine()
            while rend.needs_refine():
                assert rend.render(DrawReason.REFINE) is True
            check_tiled("refined to the end after a depth query")
        finally:
            undo()
    finally:
        vis.close()
