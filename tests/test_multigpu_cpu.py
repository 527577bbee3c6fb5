"""The in-process multi-GPU driver (topsy_amd/multigpu.py) on CPU: `_native.Context` is replaced by a stand-in whose
render is the CPU oracle (test infrastructure), so what runs for real is the product's host logic -- ParticleBuffers,
SPH.render, RenderProgression, the shard arithmetic, the per-block fan-out and the one reduce per frame.
Reference behaviour matched: one frame = the blocks of the render progression, cleared on the first block only, the mass
scale N / N_drawn global (src/topsy/sph.py:306-332, src/topsy/visualizer.py:386-405)."""
import numpy as np
import pytest


class FakeContext:
    """Subset of _native.Context that ParticleBuffers / SPH / MultiGpuContext use, backed by the oracle."""
    log = []

    def __init__(self, resolution, n_channels, device_id=0):
        self.resolution, self.n_channels, self.device_id = resolution, n_channels, device_id
        self.active_channels = 2
        self.image = np.zeros((resolution, resolution, 2), dtype=np.float32)
        self.q = None
        self.n = 0
        self.n_renders = 0
        self.reordered = False
        FakeContext.log.append(self)

    n_gpus = 1

    def set_kernel_mips(self, mips, n0=64, n_levels=4):
        self.mips = np.asarray(mips, dtype=np.float32)

    def upload_particles(self, x, y, z, h, mass=None):
        self.x, self.y, self.z, self.h = (np.ascontiguousarray(a, dtype=np.float32) for a in (x, y, z, h))
        self.m = None if mass is None else np.ascontiguousarray(mass, dtype=np.float32)
        self.n = len(self.x)

    def _refuse_without_particles(self, what):
        # tsp_upload_quantity / _rgb / _band_magnitudes: TSP_ESTATE while no particle is resident (a NumPy empty array still has
        # a non-NULL data pointer, so a zero-length upload is refused like any other)
        if self.n == 0:
            from topsy_amd import _native
            raise _native.BackendError(f"libtopsy_splat error -3: upload particles before {what}")

    def upload_quantity(self, q):
        if q is not None:
            self._refuse_without_particles("the quantity")
        self.q = None if q is None else np.ascontiguousarray(q, dtype=np.float32)

    def upload_rgb(self, r, g, b):
        self._refuse_without_particles("rgb")
        self.rgb = np.stack([np.asarray(v, dtype=np.float32) for v in (r, g, b)], axis=1)

    def upload_band_magnitudes(self, mags, weights):
        self._refuse_without_particles("the band magnitudes")
        assert mags.flags["C_CONTIGUOUS"] and mags.shape[1] == self.n
        self.mags = mags.copy()

    def reorder_spatial(self, n_strata=1, seed=1337, want_permutation=False):
        self.reordered = True
        self.n_strata = n_strata
        return np.arange(self.n, dtype=np.int64) if want_permutation else None

    def strata_offsets(self):
        if not self.reordered:
            return np.empty(0, dtype=np.int64)
        return np.linspace(0, self.n, self.n_strata + 1).astype(np.int64)

    def cell_layouts(self):
        return []

    @property
    def num_particles(self):
        return self.n

    def set_option(self, name, value):
        pass

    fail_render = None        # an exception the next render raises instead of drawing (a failed block changes nothing)

    def render_undo(self):
        self.n_undos = getattr(self, "n_undos", 0) + 1
        if not self.undoable:
            from topsy_amd import _native
            raise _native.BackendError("libtopsy_splat error -3: nothing to undo")
        self.undoable = False
        self.reduced = False
        if self.image_entry is not None:
            self.image = self.image_entry

    undoable, image_entry = False, None

    def render(self, matrix, scale_factor, starts=None, lens=None, clear=True, mode=0, flags=0):
        from oracle import oracle_c
        if self.fail_render is not None:
            e, self.fail_render = self.fail_render, None
            self.undoable, self.image_entry = True, None
            raise e
        self.undoable, self.image_entry = True, self.image.copy()
        if clear:
            self.image[:] = 0
        if starts is None:
            starts, lens = [0], [self.n]
        starts, lens = np.asarray(starts, dtype=np.int64), np.asarray(lens, dtype=np.int64)
        self.last_ranges = (starts.copy(), lens.copy())
        self.n_renders += 1
        self.reduced = False
        if self.n and lens.sum() > 0:
            oracle_c.splat(self.x, self.y, self.z, self.h, self.m, self.q, mode=0, M=matrix, sf=float(scale_factor),
                           R=self.resolution, mips=self.mips, ranges=(starts, lens), out=self.image)
        return self.ms_per_block

    ms_per_block = 1.0

    def end_frame(self, root=0):
        return 0.0

    # a stand-in communicator with the contract of tsp_comm_*: every rank calls the reduce once per frame (the ranks meet
    # at a barrier, as the collective does), a second reduce of the same frame is refused
    groups = {}

    @staticmethod
    def comm_unique_id():
        import os
        return os.urandom(128)

    def comm_init(self, n_ranks, rank, unique_id):
        import threading
        g = FakeContext.groups.setdefault(unique_id, {"members": {}, "barrier": threading.Barrier(n_ranks)})
        g["members"][rank] = self
        self.group, self.rank, self.reduced = g, rank, False

    def comm_reduce_image(self, root=0):
        assert not self.reduced, "already reduced"
        self.group["barrier"].wait(timeout=30)
        if self.rank == root:
            total = self.image.astype(np.float64)
            for r, c in self.group["members"].items():
                if r != root:
                    total += c.image
            self.presented = total.astype(np.float32)
        self.group["barrier"].wait(timeout=30)
        self.reduced = True
        self.n_reduces = getattr(self, "n_reduces", 0) + 1
        return 0.25

    def read_image(self):
        if getattr(self, "reduced", False) and hasattr(self, "presented"):
            return self.presented.copy()          # the float32 presentation copy; the accumulator stays rank-local
        return self.image.copy()

    def write_image(self, img):
        self.image = np.ascontiguousarray(img, dtype=np.float32).copy()

    def set_reduced_image(self, total):
        # tsp_set_reduced_image: the caller's sum becomes the presentation copy, the accumulator stays this shard's
        assert not getattr(self, "reduced", False), "already reduced"
        self.presented = np.ascontiguousarray(total, dtype=np.float32).copy()
        self.reduced = True

    def stats(self):
        return {"n_particles": 0, "ms_total": 1.0}

    def download_particles(self, names=("x", "y", "z", "h", "mass")):
        src = {"x": self.x, "y": self.y, "z": self.z, "h": self.h, "mass": self.m, "q": self.q}
        return {k: src[k].copy() for k in names}

    def comm_destroy(self):
        self.comm_destroyed = True

    def close(self):
        pass


@pytest.fixture
def fake_backend(monkeypatch):
    from topsy_amd import _native
    FakeContext.log = []
    FakeContext.ms_per_block = 1.0
    monkeypatch.setattr(_native, "Context", FakeContext)
    return FakeContext


class _Vis:
    """The part of the Visualizer that SPH touches."""
    periodicity_scale = np.inf

    def __init__(self, n, resolution, device_ids, with_cells=False):
        from topsy_amd import loader, particle_buffers
        self.data_loader = loader.TestDataLoader(None, n, with_cells=with_cells)
        self.particle_buffers = particle_buffers.ParticleBuffers(self.data_loader, resolution, 0, 1, device_ids=device_ids)


def _frame(vis, reason, resolution, scale=60.0):
    from topsy_amd import sph
    s = sph.SPH(vis, resolution)
    s.scale = scale
    s.render(reason)
    return s


@pytest.mark.parametrize("n_gpus", [2, 3])
def test_sph_render_on_several_contexts_matches_one(fake_backend, n_gpus):
    from topsy_amd import multigpu
    from topsy_amd.drawreason import DrawReason
    n, R = 20010, 64
    one = _Vis(n, R, None)
    s1 = _frame(one, DrawReason.EXPORT, R)
    want = s1.get_image()
    many = _Vis(n, R, list(range(n_gpus)))
    ctx = many.particle_buffers.context
    assert isinstance(ctx, multigpu.MultiGpuContext) and ctx.collective == "rccl" and ctx.n_gpus == n_gpus
    sm = _frame(many, DrawReason.EXPORT, R)
    got = sm.get_image()
    np.testing.assert_allclose(got[..., 0], want[..., 0], rtol=1e-5, atol=0)
    # every particle went to exactly one shard, shards are index ranges, every shard saw every block
    shards = ctx.contexts
    assert sum(c.n for c in shards) == n
    assert [c.n for c in shards] == list(np.diff(ctx._bounds))
    assert len({c.n_renders for c in shards}) == 1
    assert all(c.n_reduces == 1 for c in shards), "exactly one reduce per frame on every rank"
    sm.get_image()
    assert all(c.n_reduces == 1 for c in shards), "a second read-back must not reduce again"
    assert sm.last_render_mass_scale == 1.0


def test_progressive_frames_refine_without_double_counting(fake_backend):
    """Interactive frame (a prefix), REFINE frames (clear = False) until complete: after each frame the presented image is
    the sum of the shards' partial images -- the reduced copy never leaks back into a shard's accumulator."""
    from topsy_amd.drawreason import DrawReason
    n, R = 30010, 48
    one = _Vis(n, R, None)
    want = _frame(one, DrawReason.EXPORT, R).get_image()
    many = _Vis(n, R, [0, 0])                   # two contexts on one device: the host collective by construction
    ctx = many.particle_buffers.context
    assert ctx.collective == "host"
    from topsy_amd import sph
    s = sph.SPH(many, R)
    s.scale = 60.0
    s._render_progression._recommended_num_particles_to_render = 7000
    fake_backend.ms_per_block = 25.0           # one block uses up the 1/30 s budget of an interactive frame
    s.render(DrawReason.CHANGE)
    assert s.needs_refine()
    frames = 1
    partial = s.get_image()                    # scaled by N / N_drawn: roughly the final image already
    assert 0.5 < partial[..., 0].sum() / want[..., 0].sum() < 2.0
    while s.needs_refine():
        s._render_progression._recommended_num_particles_to_render = 9000
        s.render(DrawReason.REFINE)
        s.get_image()                           # a presentation between the frames (triggers the lazy reduce path too)
        frames += 1
        assert frames < 20
    assert frames >= 3
    got = s.get_image()
    assert s.last_render_mass_scale == 1.0
    np.testing.assert_allclose(got[..., 0], want[..., 0], rtol=2e-5, atol=0)


def test_multi_context_block_boundaries_and_ranges(fake_backend):
    from topsy_amd import multigpu
    ctx = multigpu.MultiGpuContext(32, 4, [0, 1, 2])
    n = 1000
    rs = np.random.RandomState(3)
    x = rs.normal(size=n).astype(np.float32)
    ctx.set_kernel_mips(np.zeros(5440, dtype=np.float32))
    ctx.upload_particles(x, x, x, np.ones(n, np.float32), np.ones(n, np.float32))
    assert ctx.num_particles == n and list(ctx._bounds) == [0, 333, 666, 1000]
    perm = ctx.reorder_spatial(30, 1, want_permutation=True)
    assert np.array_equal(perm, np.arange(n))                                   # the stand-in keeps the order; shards are offset correctly
    offs = ctx.strata_offsets()
    assert offs[0] == 0 and offs[-1] == n and (np.diff(offs) > 0).all() and {333, 666} <= set(offs.tolist())
    assert len(offs) == 3 * 10 + 1                                              # ceil(30 / 3) strata per shard
    # a block that touches only the middle shard: the others still take part with an empty selection (clear must reach them)
    ctx.render(np.eye(4, dtype=np.float32), 1.0, [400], [100], clear=True)
    r = [c.last_ranges for c in ctx.contexts]
    assert r[0][1].sum() == 0 and r[2][1].sum() == 0 and (r[1][0].tolist(), r[1][1].tolist()) == ([67], [100])
    ctx.render(np.eye(4, dtype=np.float32), 1.0, [300, 660], [100, 10], clear=False)
    r = [c.last_ranges for c in ctx.contexts]
    assert (r[0][0].tolist(), r[0][1].tolist()) == ([300], [33])
    assert (r[1][0].tolist(), r[1][1].tolist()) == ([0, 327], [67, 6])
    assert (r[2][0].tolist(), r[2][1].tolist()) == ([0], [4])
    ctx.close()


def test_interleaved_assignment_index_maps(fake_backend):
    """Block-cyclic shards: every shard's global -> local index map is monotone, so a global (start, len) range is ONE local
    range per shard (what global_to_split_monotonic needs of a split, split_buffers.py:78-116), the shards partition every
    range, and uploads / downloads / quantity swaps address the same particles."""
    from topsy_amd import multigpu
    n, B, G = 10_037, 64, 3
    ctx = multigpu.MultiGpuContext(32, 4, [0, 1, 2], assignment="interleaved", interleave_block=B)
    rs = np.random.RandomState(5)
    x = np.arange(n, dtype=np.float32)                       # x = the particle's global index
    ctx.set_kernel_mips(np.zeros(5440, dtype=np.float32))
    ctx.upload_particles(x, x, x, np.ones(n, np.float32), np.ones(n, np.float32))
    assert ctx.num_particles == n and sum(c.n for c in ctx.contexts) == n
    for g, c in enumerate(ctx.contexts):
        own = c.x.astype(np.int64)
        assert (np.diff(own) > 0).all() and ((own // B) % G == g).all()
        assert max(abs(c.n - n / G) for c in ctx.contexts) <= B
    q = rs.normal(size=n).astype(np.float32)
    ctx.upload_quantity(q)
    for c in ctx.contexts:
        assert np.array_equal(c.q, q[c.x.astype(np.int64)])
    back = ctx.download_particles(("x", "q"))
    assert np.array_equal(back["x"], x) and np.array_equal(back["q"], q)
    for _ in range(50):
        k = rs.randint(1, 6)
        starts = np.sort(rs.randint(0, n, size=k)).astype(np.int64)
        lens = rs.randint(0, 700, size=k).astype(np.int64)
        lens = np.minimum(lens, n - starts)
        ctx.render(np.eye(4, dtype=np.float32), 1.0, starts, lens, clear=True)
        drawn = []
        for c in ctx.contexts:
            ls, ll = c.last_ranges
            assert len(ls) <= k
            for a, b in zip(ls, ll):
                drawn.append(c.x[a:a + b].astype(np.int64))
        drawn = np.sort(np.concatenate(drawn)) if drawn else np.empty(0, dtype=np.int64)
        want = np.sort(np.concatenate([np.arange(a, a + b) for a, b in zip(starts, lens)] + [np.empty(0, dtype=np.int64)]))
        assert np.array_equal(drawn, want)
    # after a library reordering the index space is the concatenation of the shards; the permutation maps back to the caller's order
    perm = ctx.reorder_spatial(6, 1, want_permutation=True)
    assert np.array_equal(np.sort(perm), np.arange(n))
    assert np.array_equal(perm, np.concatenate([c.x.astype(np.int64) for c in ctx.contexts]))
    ctx.render(np.eye(4, dtype=np.float32), 1.0, [0], [ctx.contexts[0].n], clear=True)
    r = [c.last_ranges for c in ctx.contexts]
    assert r[0][1].sum() == ctx.contexts[0].n and r[1][1].sum() == 0 and r[2][1].sum() == 0
    q2 = rs.normal(size=n).astype(np.float32)
    ctx.upload_quantity(q2)                                   # still given in the caller's order
    for c in ctx.contexts:
        assert np.array_equal(c.q, q2[c.x.astype(np.int64)])
    ctx.close()
    assert all(getattr(c, "comm_destroyed", False) for c in ctx.contexts)
    with pytest.raises(AttributeError):
        ctx.write_image                                        # root-only mutations are not forwarded


def test_cell_sorted_loader_is_sharded_interleaved_and_renders_the_same_image(fake_backend):
    """A loader with its own cell layout hands over spatially sorted particles (reference loader.py:88-97): 'auto' deals them
    block-cyclically, the cell progression's (start, len) ranges reach every shard, and the frame equals the one-context frame."""
    from topsy_amd import multigpu
    from topsy_amd.drawreason import DrawReason
    n, R = 30_000, 64
    one = _Vis(n, R, None, with_cells=True)
    want = _frame(one, DrawReason.EXPORT, R).get_image()
    many = _Vis(n, R, [0, 1, 2, 3], with_cells=True)
    ctx = many.particle_buffers.context
    assert isinstance(ctx, multigpu.MultiGpuContext) and ctx.assignment == "interleaved"
    assert max(c.n for c in ctx.contexts) - min(c.n for c in ctx.contexts) <= ctx.interleave_block
    got = _frame(many, DrawReason.EXPORT, R).get_image()
    np.testing.assert_allclose(got[..., 0], want[..., 0], rtol=1e-5, atol=0)
    plain = _Vis(n, R, [0, 1, 2, 3], with_cells=False)
    assert plain.particle_buffers.context.assignment == "contiguous"


def _few_particles(n):
    rs = np.random.RandomState(n)
    x = np.arange(n, dtype=np.float32)
    return x, rs.normal(size=n).astype(np.float32), rs.uniform(size=(3, n)).astype(np.float32), rs.uniform(2.0, 9.0, size=(3, n))


@pytest.mark.parametrize("assignment,block", [("contiguous", 4096), ("interleaved", 4096), ("interleaved", 2)])
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5])
def test_uploads_with_empty_shards(fake_backend, assignment, block, n):
    """Fewer particles than members (contiguous), or no more than one interleave block (every member past the first is empty):
    the member contexts refuse an upload before particles are resident, as the library does, so the driver must leave the empty
    ones out -- and every particle's values must still arrive at the member that holds it."""
    from topsy_amd import multigpu
    G = 4
    ctx = multigpu.MultiGpuContext(16, 4, list(range(G)), assignment=assignment, interleave_block=block)
    x, q, rgb, mags = _few_particles(n)
    ctx.set_kernel_mips(np.zeros(5440, dtype=np.float32))
    ctx.upload_particles(x, x, x, np.ones(n, np.float32), np.ones(n, np.float32))
    sizes = [c.n for c in ctx.contexts]
    assert sum(sizes) == n == ctx.num_particles and (0 in sizes or n >= G)
    if assignment == "interleaved" and block == 4096:
        assert sizes == [n, 0, 0, 0]
    ctx.upload_quantity(q)
    ctx.upload_rgb(rgb[0], rgb[1], rgb[2])
    ctx.upload_band_magnitudes(mags, np.eye(3))
    for c in ctx.contexts:
        if c.n == 0:
            assert c.q is None and not hasattr(c, "rgb") and not hasattr(c, "mags")
            continue
        own = c.x.astype(np.int64)
        assert np.array_equal(c.q, q[own]) and np.array_equal(c.rgb, rgb[:, own].T) and np.array_equal(c.mags, mags[:, own])
    ctx.upload_quantity(None)                                  # dropping the quantity reaches every member, empty or not
    assert all(c.q is None for c in ctx.contexts)
    perm = ctx.reorder_spatial(3, 1, want_permutation=True)
    assert perm.dtype == np.int64 and np.array_equal(np.sort(perm), np.arange(n))
    assert all(c.reordered == (c.n > 0) for c in ctx.contexts)
    offs = ctx.strata_offsets()
    if n:
        assert offs[0] == 0 and offs[-1] == n and (np.diff(offs) >= 0).all()
    assert ctx.cell_layouts() == []
    back = ctx.download_particles(("x",))
    assert np.array_equal(np.sort(back["x"]), x)
    ctx.render(np.eye(4, dtype=np.float32), 1.0, [0], [np.iinfo(np.int64).max], clear=True)
    assert sum(int(c.last_ranges[1].sum()) for c in ctx.contexts) == n
    ctx.close()


@pytest.mark.parametrize("devices", [[0, 0, 0], [0, 1, 2]], ids=["host", "rccl"])
@pytest.mark.parametrize("failing", [0, 1, 2])
def test_failed_block_is_undone_on_every_member(fake_backend, devices, failing):
    """The rollback choreography of MultiGpuContext.render: member `failing` raises, every other member then gets exactly one
    undo, the frame is marked for a new reduce, the exception is the failing member's and names it -- and the retried block
    leaves the image a run without the failure leaves."""
    from topsy_amd import _native, kernel_lut, multigpu
    n, R = 600, 32
    rs = np.random.RandomState(4)
    pos = (rs.normal(size=(n, 3)) * 20.0).astype(np.float32)
    h = rs.uniform(1.0, 8.0, n).astype(np.float32)
    m = rs.uniform(0.5, 2.0, n).astype(np.float32)
    M = np.eye(4, dtype=np.float32)
    M[:3, :3] /= 60.0
    M[2, :] = [0.0, 0.0, 0.5 / 60.0, 0.5]

    def frames(fail):
        ctx = multigpu.MultiGpuContext(R, 2, devices)
        ctx.set_kernel_mips(kernel_lut.kernel_mips())
        ctx.upload_particles(pos[:, 0], pos[:, 1], pos[:, 2], h, m)
        first = [0, 200, 400], [100, 100, 100]
        second = [100, 300, 500], [100, 100, 100]
        ctx.render(M, 1.0 / 60.0, *first, clear=True)
        before = ctx.read_image().copy()
        partial = [c.image.copy() for c in ctx.contexts]
        if fail:
            boom = _native.BackendError("libtopsy_splat error -2: injected")
            ctx.contexts[failing].fail_render = boom
            assert not ctx._needs_reduce
            with pytest.raises(_native.BackendError, match=f"context {failing} .*injected") as info:
                ctx.render(M, 1.0 / 60.0, *second, clear=False)
            assert info.value.__cause__ is boom
            assert ctx._needs_reduce
            for g, c in enumerate(ctx.contexts):
                assert c.n_undos == 1, "every member is put back exactly once (the failing one re-forms its partial image)"
                assert np.array_equal(c.image, partial[g]) and not c.reduced
            assert np.array_equal(ctx.read_image(), before)           # summed anew: the frame before the failed call
        ctx.render(M, 1.0 / 60.0, *second, clear=False)
        out = ctx.read_image().copy()
        ctx.close()
        return out

    assert np.array_equal(frames(True), frames(False))
    # A call that never reaches the library on a member (the binding rejects an argument) must not take back that member's
    # EARLIER block -- its undo state still belongs to it -- and must not ask for a reduce that cannot succeed: after a frame
    # that was already reduced, the root keeps presenting that frame unless the root itself was put back.
    def reduced_frame():
        ctx = multigpu.MultiGpuContext(R, 2, devices)
        ctx.set_kernel_mips(kernel_lut.kernel_mips())
        ctx.upload_particles(pos[:, 0], pos[:, 1], pos[:, 2], h, m)
        ctx.render(M, 1.0 / 60.0, [0], [n], clear=True)
        return ctx, ctx.read_image().copy()

    for who in ("all", "one"):
        ctx, frame = reduced_frame()
        assert not ctx._needs_reduce
        for g, c in enumerate(ctx.contexts):
            if who == "all" or g == failing:
                c.fail_render = ValueError("matrix has 15 elements, expected 16")
        with pytest.raises(ValueError, match="15 elements"):
            ctx.render(M, 1.0 / 60.0, [0], [n], clear=False)
        reached = [who == "one" and g != failing for g in range(3)]
        assert [getattr(c, "n_undos", 0) for c in ctx.contexts] == [int(r) for r in reached]
        assert ctx._needs_reduce == reached[0]
        if who == "one" and failing != 0 and ctx.collective == "rccl":
            # the root was put back, member `failing` still counts as reduced: the collective would wait for it for ever
            with pytest.raises(_native.BackendError, match=rf"contexts \[{failing}\] could not be put back"):
                ctx.read_image()
            assert ctx._needs_reduce
        else:
            assert np.array_equal(ctx.read_image(), frame), "the frame before the failed call"
        ctx.render(M, 1.0 / 60.0, [0], [n], clear=True)                  # ... and a render that succeeds presents again
        assert np.array_equal(ctx.read_image(), frame)
        ctx.close()
    # a wrong argument is refused by the driver itself, before any member is touched
    ctx, frame = reduced_frame()
    with pytest.raises(ValueError):
        ctx.render(np.eye(4, dtype=np.float32).ravel()[:15], 1.0 / 60.0, [0], [n], clear=False)
    with pytest.raises(ValueError, match="equal length"):
        ctx.render(M, 1.0 / 60.0, [0, 5], [n], clear=False)
    assert all(c.n_renders == 1 and getattr(c, "n_undos", 0) == 0 for c in ctx.contexts) and not ctx._needs_reduce
    assert np.array_equal(ctx.read_image(), frame)
    ctx.close()

    # a member that drew the block but cannot be put back: the failing member's error stays, the other is appended, every
    # member's channel layout is the one before the call
    ctx, frame = reduced_frame()
    other = (failing + 1) % 3
    ctx.contexts[failing].fail_render = _native.BackendError("libtopsy_splat error -2: injected")
    ctx.contexts[other].render_undo = lambda: (_ for _ in ()).throw(_native.BackendError("libtopsy_splat error -5: hipMemcpyAsync failed"))
    for c in ctx.contexts:
        c.active_channels = 2
    with pytest.raises(_native.BackendError, match=rf"context {failing} .*injected; and context {other} could not be put back .*hipMemcpyAsync"):
        ctx.render(M, 1.0 / 60.0, [0], [n], clear=False)
    assert all(c.active_channels == 2 for c in ctx.contexts)
    ctx.close()
