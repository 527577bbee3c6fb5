"""world_size-2 gloo test (CPU): the index-range sharding of render blocks and the sum-reduce of
the partial images reproduce the single-rank image.  The per-shard images come from the CPU oracle
(test infrastructure) because there is no GPU here; what is under test is the product's sharding
arithmetic (topsy_amd.distributed) and the N>1 reduction contract (sum, float32, root 0)."""
import os
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch
    import torch.distributed as dist
    from conftest import make_cloud
    from oracle import oracle_c, oracle_np
    from topsy_amd import distributed, kernel_lut, progressive_render
    from topsy_amd.drawreason import DrawReason
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        n, R = 30011, 96
        pos, h, m, q, _ = make_cloud(n, seed=11)
        M, sf = oracle_np.transform_matrix(np.eye(3), np.zeros(3), 180.0)
        mips = kernel_lut.kernel_mips()
        start, length = distributed.shard_range(n, rank, world)
        sl = slice(start, start + length)
        xs, ys, zs = (np.ascontiguousarray(pos[sl, k]) for k in range(3))
        # frame = the block sequence the (unchanged) RenderProgression hands out, here an EXPORT frame
        # split into several blocks plus a multi-range block as the cell-based progression produces
        rp = progressive_render.RenderProgression(n)
        rp.start_frame(DrawReason.EXPORT)
        blocks = [([0], [7000]), ([7000, 9000, 20000], [2000, 11000, 10011])]
        image = np.zeros((R, R, 2), dtype=np.float32)
        drawn = 0
        for starts, lens in blocks:
            s, l = distributed.intersect_ranges(starts, lens, start, length)
            assert (s >= 0).all() and (s + l <= length).all()
            drawn += int(l.sum())
            if len(s):
                oracle_c.splat(xs, ys, zs, h[sl], m[sl], q[sl], mode=0, M=M, sf=sf, R=R, mips=mips, ranges=(s, l), out=image)
        t = torch.from_numpy(image)
        dist.reduce(t, dst=0, op=dist.ReduceOp.SUM)        # the one collective of the path
        total = torch.tensor([drawn])
        dist.all_reduce(total)
        assert int(total) == n, "every particle must be drawn by exactly one shard"
        if rank == 0:
            np.save(os.path.join(out_dir, "reduced.npy"), t.numpy())
        # the RCCL unique id travels through the same out-of-band channel in production
        payload = distributed.torch_broadcaster(dist)(b"x" * 128 if rank == 0 else None)
        assert payload == b"x" * 128
    finally:
        dist.destroy_process_group()


def test_two_rank_sharded_render_matches_single(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import make_cloud, spawn_ranks
    spawn_ranks(_worker, 2, _free_port(), str(tmp_path))
    from oracle import oracle_c, oracle_np
    from topsy_amd import kernel_lut
    pos, h, m, q, _ = make_cloud(30011, seed=11)
    M, sf = oracle_np.transform_matrix(np.eye(3), np.zeros(3), 180.0)
    x, y, z = (np.ascontiguousarray(pos[:, k]) for k in range(3))
    want, _ = oracle_c.splat(x, y, z, h, m, q, mode=0, M=M, sf=sf, R=96, mips=kernel_lut.kernel_mips())
    got = np.load(tmp_path / "reduced.npy")
    np.testing.assert_allclose(got[..., 0], want[..., 0], rtol=1e-5, atol=0)
    scale, _ = oracle_c.splat(x, y, z, h, m, np.abs(q), mode=0, M=M, sf=sf, R=96, mips=kernel_lut.kernel_mips())
    assert (np.abs(got[..., 1] - want[..., 1]) <= 1e-5 * scale[..., 1] + 1e-30).all()


def test_shard_arithmetic():
    from topsy_amd import distributed as d
    for n, g in [(10, 3), (1000000007, 8), (5, 8), (0, 2)]:
        b = d.shard_bounds(n, g)
        assert b[0] == 0 and b[-1] == n and (np.diff(b) >= 0).all() and np.diff(b).max() - np.diff(b).min() <= 1
    # blocks intersected with shards partition the blocks exactly
    rs = np.random.RandomState(0)
    n, g = 100000, 4
    starts = np.sort(rs.randint(0, n, 50)); lens = rs.randint(0, 3000, 50)
    lens = np.minimum(lens, n - starts)
    covered = np.zeros(n, dtype=np.int32); want = np.zeros(n, dtype=np.int32)
    for s, l in zip(starts, lens):
        want[s:s + l] += 1
    for r in range(g):
        s0, ln = d.shard_range(n, r, g)
        ss, ll = d.intersect_ranges(starts, lens, s0, ln)
        for s, l in zip(ss, ll):
            covered[s0 + s:s0 + s + l] += 1
    assert np.array_equal(covered, want)
    assert d.intersect_ranges([5], [10], 100, 50)[0].size == 0


def test_sharded_renderer_whole_set_block():
    """starts = lens = None means the whole snapshot, as in tsp_render: every rank draws exactly its shard."""
    from topsy_amd import distributed as d

    class FakeContext:
        def render(self, matrix, scale_factor, starts, lens, clear, mode, flags):
            self.call = (np.asarray(starts).tolist(), np.asarray(lens).tolist(), clear)
            return 0.0

    n, g = 1000003, 3
    drawn = 0
    for r in range(g):
        ctx = FakeContext()
        sr = d.ShardedRenderer(ctx, n, r, g)
        sr.render_block(np.eye(4), 1.0, None, None, clear=True)
        assert ctx.call == ([0], [sr.shard_len], True)
        drawn += sr.shard_len
    assert drawn == n


I64 = np.iinfo(np.int64)


def _edge_ranges(rs, n, k):
    """k (start, len) pairs around [0, n): random ones, negative starts, "to the end" lengths (2**62, INT64_MAX), empty ones,
    starts at and past the end, in no particular order"""
    starts = rs.randint(-n // 2 - 3, n + n // 2 + 3, size=k).astype(np.int64)
    lens = rs.randint(0, n + 5, size=k).astype(np.int64)
    kind = rs.randint(0, 8, size=k)
    lens[kind == 0] = 2**62
    lens[kind == 1] = I64.max
    lens[kind == 2] = 0
    starts[kind == 3] = rs.choice([0, n - 1, n, n + 1, -1, I64.min, I64.max - 1, I64.max], size=int((kind == 3).sum()))
    return starts, lens


def _members(starts, lens, n):
    """how often each index of [0, n) is drawn, by brute force in Python integers"""
    count = np.zeros(n, dtype=np.int64)
    for s, l in zip(starts.tolist(), lens.tolist()):
        lo, hi = max(s, 0), min(s + l, n)
        if hi > lo:
            count[lo:hi] += 1
    return count


@pytest.mark.parametrize("n,world", [(0, 2), (1, 2), (2, 3), (4, 5), (5, 5), (6, 5), (97, 3), (1500, 5)])
def test_intersect_ranges_against_brute_force(n, world):
    """Every shard's intersection, re-based, covers exactly the brute-force multiset of the block -- for negative starts, lengths
    of 2**62 and INT64_MAX, empty ranges and empty shards (n < world), with the total given or not."""
    from topsy_amd import distributed as d
    rs = np.random.RandomState(100 * n + world)
    bounds = d.shard_bounds(n, world)
    for trial in range(40):
        starts, lens = _edge_ranges(rs, max(n, 1), rs.randint(1, 9))
        want = _members(starts, lens, n)
        for total in (n, None):
            got = np.zeros(n, dtype=np.int64)
            for g in range(world):
                a, ln = int(bounds[g]), int(bounds[g + 1] - bounds[g])
                ss, ll = d.intersect_ranges(starts, lens, a, ln, total)
                assert ss.dtype == np.int64 and ll.dtype == np.int64 and len(ss) == len(ll) <= len(starts)
                assert (ss >= 0).all() and (ll > 0).all() and (ss + ll <= ln).all()
                for s, l in zip(ss.tolist(), ll.tolist()):
                    got[a + s:a + s + l] += 1
            assert np.array_equal(got, want), (starts, lens, total)
    s, l = d.intersect_ranges([10], [I64.max], 50, 50, 100)
    assert (s.tolist(), l.tolist()) == ([0], [50])                     # "to the end" reaches a later shard whole
    s, l = d.intersect_ranges([10], [2**62], 50, 50, 100)
    assert (s.tolist(), l.tolist()) == ([0], [50])


def test_clip_ranges_matches_the_library_rule():
    """tsp_render's clip (clip_ranges in tsp_api.hip): a negative start loses what lies before 0, the end is cut at n"""
    from topsy_amd import distributed as d
    s, l = d.clip_ranges([-5, -5, I64.min, I64.min, 3, 200, -1, 0], [3, 7, I64.max, 5, I64.max, 4, I64.max, -3], 100)
    assert s.tolist() == [0, 0, 0, 0, 3, 100, 0, 0] and l.tolist() == [0, 2, 0, 0, 97, 0, 100, 0]


@pytest.mark.parametrize("n,world,block", [(0, 2, 4), (1, 2, 4), (3, 5, 1), (64, 3, 64), (65, 3, 64), (1500, 3, 64), (1500, 5, 4096),
                                           (1000, 4, 7)])
def test_cyclic_local_ranges_against_brute_force(n, world, block):
    """The block-cyclic driver's global -> local range map (MultiGpuContext._local_ranges over _cyclic_local): every member draws
    exactly its own particles of the block, each global range as at most one local range, for the same edge ranges."""
    from topsy_amd import multigpu
    ctx = multigpu.MultiGpuContext.__new__(multigpu.MultiGpuContext)      # the index arithmetic alone: no library, no contexts
    ctx.interleave_block, ctx.contexts = block, [None] * world
    ctx._cyclic = ctx._cyclic_ranges = True
    ctx._n_uploaded = n
    sizes = [int(ctx._cyclic_local(n, g)) for g in range(world)]
    ctx._bounds = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    owned = [ctx._cyclic_owned(g) for g in range(world)]
    assert [len(o) for o in owned] == sizes and sum(sizes) == n
    assert np.array_equal(np.sort(np.concatenate(owned)), np.arange(n))
    for g in range(world):
        assert ((owned[g] // block) % world == g).all() and (np.diff(owned[g]) > 0).all()
        # _cyclic_local(i, g) = how many of g's particles lie below i
        probe = np.arange(0, n + 1, dtype=np.int64)
        assert np.array_equal(ctx._cyclic_local(probe, g), np.searchsorted(owned[g], probe))
    rs = np.random.RandomState(7 * n + world)
    for trial in range(40):
        starts, lens = _edge_ranges(rs, max(n, 1), rs.randint(1, 9))
        want = _members(starts, lens, n)
        got = np.zeros(n, dtype=np.int64)
        for g in range(world):
            ss, ll = ctx._local_ranges(starts, lens, g)
            assert len(ss) <= len(starts) and (ss >= 0).all() and (ll > 0).all() and (ss + ll <= sizes[g]).all()
            for s, l in zip(ss.tolist(), ll.tolist()):
                np.add.at(got, owned[g][s:s + l], 1)
        assert np.array_equal(got, want), (starts, lens)
    ctx.contexts = []


def test_sharded_renderer_clips_to_the_end_lengths():
    """render_block hands its total to intersect_ranges: a block "from 10 to the end" (INT64_MAX) reaches every later rank"""
    from topsy_amd import distributed as d

    class FakeContext:
        def render(self, matrix, scale_factor, starts, lens, clear, mode, flags):
            self.call = (np.asarray(starts).tolist(), np.asarray(lens).tolist())

    n, world = 100, 2
    drawn = []
    for r in range(world):
        ctx = FakeContext()
        d.ShardedRenderer(ctx, n, r, world).render_block(np.eye(4), 1.0, [10, -4], [I64.max, 6], clear=True)
        drawn.append(ctx.call)
    assert drawn == [([10, 0], [40, 2]), ([0], [50])]
