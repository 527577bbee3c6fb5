"""Frames after a second upload.  The library caches m / h^2 and rgb / h^2 per upload, keeps a load-time permutation that later
uploads go through, and option use_quantity selects the single-channel kernel builds while q stays resident: one context lives
through a product session's sequence of uploads, option changes, mode switches and a reorder, and after every step the frame
is compared with the oracle fed the attributes that are current, in the caller's order (tolerances:
parity_scenes.render_and_check; never bit for bit -- a reorder changes the order of summation)."""
import numpy as np
import pytest

import parity_scenes as ps

pytestmark = pytest.mark.gpu

R = 128


@pytest.fixture(scope="module")
def native():
    from topsy_amd import _native
    _native.load_library()
    return _native


def test_frames_follow_every_upload_on_one_context(native, mips):
    from oracle import oracle_np
    base = ps.all_class_scene(R, n=3000)
    n = len(base["h"])
    M, sf = oracle_np.transform_matrix(ps._rot(0.25, -0.15), np.zeros(3), base["scale"])
    rs = np.random.RandomState(101)
    q2, q3 = (rs.normal(size=n).astype(np.float32) for _ in range(2))
    c1, c2, c3 = (rs.uniform(0.0, 1.0, size=(n, 3)).astype(np.float32) for _ in range(3))
    mags = rs.uniform(-2.5, 5.0, size=(3, n))
    weights = np.diag([0.5, 1.0, 1.0])
    c_band = oracle_np.band_contraction(mags, weights)

    ctx = native.Context(R, 4)
    state = {"scene": base}                   # what the oracle is fed: the attributes current in the caller's order

    def shows(mode, what, counts=(1, 0)):
        """the frame of `mode` is the oracle's for the current attributes; density renders through use_quantity = 0"""
        if mode == "density":
            ctx.set_option("use_quantity", 0)
        try:
            for count in counts:
                got, st = ps.render_and_check(ctx, native, mode, state["scene"], M, sf, R, mips, count, label=what)
        finally:
            if mode == "density":
                ctx.set_option("use_quantity", 1)
        assert got.shape == (R, R, 4 if mode == "rgb" else 2), what
        return got, st

    def upload_rgb(c):
        ctx.upload_rgb(c[:, 0].copy(), c[:, 1].copy(), c[:, 2].copy())
        state["scene"] = dict(state["scene"], rgb=c)

    def upload_quantity(q):
        ctx.upload_quantity(q)
        state["scene"] = dict(state["scene"], q=q)

    def refuses_rgb():
        with pytest.raises(native.BackendError, match="error -4: .*rgb arrays not uploaded"):       # TSP_ESTATE
            ctx.render(M, sf, mode=native.MODE_RGB)

    try:
        ctx.set_kernel_mips(mips)
        with pytest.raises(native.BackendError, match="error -4: .*upload particles before the quantity"):
            ctx.upload_quantity(np.zeros(0, dtype=np.float32))
        empty = np.zeros(0, dtype=np.float32)
        with pytest.raises(native.BackendError, match="error -4: .*upload particles before rgb"):
            ctx.upload_rgb(empty, empty, empty)
        # 1. particles and q
        pos = base["pos"]
        ctx.upload_particles(pos[:, 0], pos[:, 1], pos[:, 2], base["h"], base["m"])
        upload_quantity(base["q"])
        _, st = shows("weighted", "step 1")
        assert st["n_small"] > 0 and st["n_mid"] > 0 and st["n_huge"] > 0, st
        refuses_rgb()                          # no colours resident yet
        # 2. a second quantity
        upload_quantity(q2)
        img2, st2 = shows("weighted", "step 2: second quantity", counts=(0, 1))
        want2, _, terms2 = ps.oracle_images("weighted", state["scene"], M, sf, R, mips)
        want1, _, _ = ps.oracle_images("weighted", base, M, sf, R, mips)
        assert (np.abs(want2[..., 1] - want1[..., 1]) > 1e-5 * terms2).sum() > 1000       # (a frame of the first quantity cannot pass)
        # 3. use_quantity = 0: the single-channel builds, q still resident
        ctx.set_option("use_quantity", 0)
        img3, st3 = ps.render_and_check(ctx, native, "density", state["scene"], M, sf, R, mips, 1, label="step 3: use_quantity 0")
        assert (img3[..., 1] == 0).all() and img2[..., 1].any()
        assert st3["n_fragments"] == st2["n_fragments"]
        ps.render_and_check(ctx, native, "density", state["scene"], M, sf, R, mips, 0, label="step 3: use_quantity 0")
        # 4. and back: q2 again
        ctx.set_option("use_quantity", 1)
        _, st4 = shows("weighted", "step 4: use_quantity 1", counts=(0, 1))
        assert st4["n_fragments"] == st2["n_fragments"]
        # 5. - 6. colours, then other colours
        upload_rgb(c1)
        shows("rgb", "step 5: first colours")
        upload_rgb(c2)
        shows("rgb", "step 6: second colours")
        want_c1, _, _ = ps.oracle_images("rgb", dict(state["scene"], rgb=c1), M, sf, R, mips)
        want_c2, _, _ = ps.oracle_images("rgb", state["scene"], M, sf, R, mips)
        assert (np.abs(want_c2[..., :3] - want_c1[..., :3]) > 1e-5 * np.abs(want_c1[..., :3])).sum() > 1000   # (c1's frame cannot pass)
        # 7. colours from band magnitudes, contracted on the device
        ctx.upload_band_magnitudes(mags, weights)
        state["scene"] = dict(state["scene"], rgb=c_band)
        shows("rgb", "step 7: band magnitudes")
        # 8. mode switches on one context: 2- and 4-channel layouts
        shows("depth", "step 8: depth after rgb")
        shows("weighted", "step 8: weighted after depth")
        shows("rgb", "step 8: rgb after weighted", counts=(0,))
        # 9. the load-time ordering
        ctx.reorder_spatial(8, 4242)
        for mode in ps.MODES:
            shows(mode, "step 9: after the reorder")
        # 10. uploads after the reorder arrive in the caller's order
        upload_quantity(q3)
        upload_rgb(c3)
        shows("weighted", "step 10: quantity after the reorder")
        shows("rgb", "step 10: colours after the reorder")
        # 11. fresh particles: fewer with other smoothing lengths, then more; q, the colours and the ordering are gone with the
        # old ones (a weighted render is density only, an rgb render is refused) until they are uploaded again
        for n_new, seed in ((1000, 3), (4500, 4)):
            fresh = ps.all_class_scene(R, n=n_new, seed=seed)
            pos = fresh["pos"]
            ctx.upload_particles(pos[:, 0], pos[:, 1], pos[:, 2], fresh["h"], fresh["m"])
            state["scene"] = fresh
            assert ctx.num_particles == n_new and ctx.cell_layout() is None
            _, st = ps.render_and_check(ctx, native, "density", fresh, M, sf, R, mips, 1, label=("step 11", n_new))
            assert st["n_small"] + st["n_mid"] + st["n_huge"] + st["n_culled"] == n_new, st
            ps.render_and_check(ctx, native, "density", fresh, M, sf, R, mips, 0, label=("step 11", n_new))
            refuses_rgb()
            shows("depth", ("step 11: depth", n_new))
            upload_quantity(fresh["q"])
            upload_rgb(fresh["rgb"])
            shows("weighted", ("step 11: quantity for the fresh particles", n_new))
            shows("rgb", ("step 11: colours for the fresh particles", n_new))
    finally:
        ctx.close()
