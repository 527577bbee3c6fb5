"""Sharded rendering at the edges of its shards, held to the oracle.

Several shards go through two drivers: the C device group (tsp_group_*, bound as _native.Group) and the Python driver
multigpu.MultiGpuContext (contiguous or block-cyclic shards).  Both are drawn here on contexts that share device 0 -- the reduce is
then the host collective -- and, for one parity case and the rollback case, on devices [0, 1] (RCCL) where two cards exist.

Every frame is compared with the oracle through parity_scenes.compare_with_oracle (the project's tolerances: density and colour
channels 1e-5 relative, the weighted channel 1e-5 of sum|terms|, the rgb count channel exact); with count_fragments = 1 the
fragment count summed over the shards is the oracle's integer.  The scene is parity_scenes.all_class_scene(128): 1500 particles
of all three footprint classes with ties and off-screen centres, so shards hold 300 - 750 particles, the default interleave block
(4096) is larger than the snapshot, and prefixes of 0 - 6 particles leave shards empty.

The last test makes a block fail on ONE member (debug_fail_stage 1 / 2, debug_fail_alloc) and checks that it is drawn on no
member: tsp_group_render and MultiGpuContext.render put the members that succeeded back (tsp_render_undo).  Its two blocks are
not index halves: each is a set of ranges that reaches every shard (a member whose share of a block is empty never reaches the
injected failure), block 2 in 150 ranges of 5 particles so that every member has to grow its range table -- the allocation
that debug_fail_alloc = 1 fails.  Each member's partial image is recorded BEFORE the frame's reduce (after it the root's float32
image is the sum, which an undone root does not hold again until the next reduce); the root frame is recorded after it.
"""
import ctypes

import numpy as np
import pytest

import parity_scenes
import test_gpu_nonfinite_weights as nonfinite

pytestmark = pytest.mark.gpu

R = 128
I64_MAX = np.iinfo(np.int64).max
KINDS = ("group", "contiguous", "interleaved64")
MODES = parity_scenes.MODES


@pytest.fixture(scope="module")
def native():
    from topsy_amd import _native
    _native.load_library()
    return _native


@pytest.fixture(scope="module")
def scene():
    return parity_scenes.all_class_scene(R)


@pytest.fixture(scope="module")
def camera(scene):
    from oracle import oracle_np
    M, sf = oracle_np.transform_matrix(np.eye(3), np.zeros(3), scene["scale"])
    return M, float(sf)


def _need(native, devices):
    if len(set(devices)) > 1 and native.device_count() < len(set(devices)):
        pytest.skip("needs two GPUs")


def _native_mode(native, mode):
    return {"density": native.MODE_WEIGHTED, "weighted": native.MODE_WEIGHTED, "depth": native.MODE_DEPTH, "rgb": native.MODE_RGB}[mode]


def _sub(scene, idx):
    return parity_scenes.make_scene(*(scene[k][idx] for k in ("pos", "h", "m", "q", "rgb")), scale=scene["scale"])


_UNWRITTEN = np.uint32(0x7FC0DEAD)      # a NaN payload no kernel produces: marks what tsp_read_image did not write


def _raw_image(ctx):
    """(float32 image, channel count) of one context as the LIBRARY holds them: tsp_read_image writes R * R * C floats"""
    buf = np.full(R * R * 4, _UNWRITTEN, dtype=np.uint32)
    rc = ctx._lib.tsp_read_image(ctx._h, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    assert rc == 0
    assert not (buf[:R * R * 2] == _UNWRITTEN).any()
    C = 2 if (buf[R * R * 2:] == _UNWRITTEN).all() else 4
    assert C == 2 or not (buf == _UNWRITTEN).any()
    return buf[:R * R * C].view(np.float32).reshape(R, R, C).copy(), C


class Driver:
    """One interface over _native.Group and MultiGpuContext, 4-channel contexts (they hold 2-channel renders too)"""

    def __init__(self, native, kind, devices, mips):
        from topsy_amd import multigpu
        self.native, self.kind, self.G = native, kind, len(devices)
        self.rccl = len(set(devices)) == len(devices)
        if kind == "group":
            self.d = native.Group(R, 4, devices)
            assert self.d.uses_rccl == self.rccl
        else:
            kw = {"contiguous": dict(assignment="contiguous"), "interleaved64": dict(assignment="interleaved", interleave_block=64),
                  "interleaved4096": dict(assignment="interleaved")}[kind]
            self.d = multigpu.MultiGpuContext(R, 4, devices, **kw)
            assert self.d.collective == ("rccl" if self.rccl else "host")
        self.d.set_kernel_mips(mips)
        self.d.set_option("count_fragments", 1)

    def close(self):
        self.d.close()

    @property
    def members(self):
        return [self.d.member(g) for g in range(self.G)] if self.kind == "group" else list(self.d.contexts)

    def owned(self, g, n):
        """global indices (caller's order) of member g's particles, in its order at upload"""
        if self.kind.startswith("interleaved"):
            B = self.d.interleave_block
            i = np.arange(n)
            return i[(i // B) % self.G == g]
        return np.arange((g * n) // self.G, ((g + 1) * n) // self.G)

    def upload(self, sc, mode):
        parity_scenes.upload_scene(self.d, sc, mode)

    def render(self, camera, mode, starts=None, lens=None, clear=True):
        return self.d.render(camera[0], camera[1], starts, lens, clear=clear, mode=_native_mode(self.native, mode))

    def frame(self):
        """the reduced frame, read on the root"""
        self.d.end_frame()
        return (self.d.root if self.kind == "group" else self.d).read_image()

    def fragments(self):
        return self.d.stats()["n_fragments"]

    def resident(self, names):
        """the resident arrays in the driver's global index order"""
        if self.kind != "group":
            return self.d.download_particles(names)
        parts = [m.download_particles(names) for m in self.members if m.num_particles > 0]
        return {k: np.concatenate([p[k] for p in parts] + [np.empty(0, dtype=np.float32)]) for k in names}

    def resident_scene(self, sc, mode):
        """the scene as resident (after a reorder): what the oracle is fed, attribute by attribute what `mode` draws"""
        names = {"density": ("mass",), "depth": ("mass",), "weighted": ("mass", "q"), "rgb": ("r", "g", "b")}[mode]
        got = self.resident(("x", "y", "z", "h") + names)
        n = len(got["x"])
        pos = np.stack([got["x"], got["y"], got["z"]], axis=1)
        rgb = np.stack([got[k] for k in "rgb"], axis=1) if mode == "rgb" else np.zeros((n, 3), dtype=np.float32)
        return parity_scenes.make_scene(pos, got["h"], got.get("mass", np.zeros(n, np.float32)), got.get("q", np.zeros(n, np.float32)), rgb,
                                        scale=sc["scale"])


def _same_particles(a, b, mode):
    """two scenes hold the same multiset of particles (a reorder moves them, no more)"""
    keys = {"density": ("pos", "h", "m"), "depth": ("pos", "h", "m"), "weighted": ("pos", "h", "m", "q"), "rgb": ("pos", "h", "rgb")}[mode]
    if len(a["h"]) == 0 or len(b["h"]) == 0:
        return len(a["h"]) == len(b["h"])
    rows = [np.concatenate([s[k].reshape(len(s["h"]), -1) for k in keys], axis=1) for s in (a, b)]
    return np.array_equal(rows[0][np.lexsort(rows[0].T)], rows[1][np.lexsort(rows[1].T)])


def _check_frame(drv, camera, mode, sc, mips, label):
    want, nfrag, terms = parity_scenes.oracle_images(mode, sc, camera[0], camera[1], R, mips)
    got = drv.frame()
    assert got.shape == want.shape, label
    parity_scenes.compare_with_oracle(got, mode, want, terms, label)
    assert drv.fragments() == nfrag, (label, "fragment count over the shards")


# ---- ranges: clipped by brute force in Python integers (the oracle forms start + len itself), rendered by the oracle -----------
def _clip(starts, lens, n):
    out = [(max(s, 0), min(s + l, n)) for s, l in zip([int(s) for s in starts], [int(l) for l in lens])]
    out = [(lo, hi - lo) for lo, hi in out if hi > lo]
    return np.asarray([s for s, _ in out], dtype=np.int64), np.asarray([l for _, l in out], dtype=np.int64)


_range_cache = {}


def _oracle_ranges(mode, sc, camera, mips, starts, lens):
    """(image, fragments, sum|terms| or None) of the oracle over the given ranges of the scene, once per input"""
    s, l = _clip(starts, lens, len(sc["h"]))
    key = (mode, parity_scenes._key(sc["pos"], sc["h"], sc["m"], sc["q"], sc["rgb"], s, l, np.asarray(camera[0], dtype=np.float32)))
    if key not in _range_cache:
        pos, h, m, q, rgb = (sc[k] for k in ("pos", "h", "m", "q", "rgb"))
        M, sf = camera
        if len(s) == 0:
            C = 4 if mode == "rgb" else 2
            _range_cache[key] = (np.zeros((R, R, C), dtype=np.float32), 0, np.zeros((R, R)) if mode == "weighted" else None)
            return _range_cache[key]
        kw = dict(ranges=(s, l))
        terms = None
        if mode == "rgb":
            want, nf = parity_scenes.oracle_render(pos, h, rgb[:, 0].copy(), rgb[:, 1].copy(), rgb[:, 2].copy(), 2, M, sf, R, mips, **kw)
        elif mode == "depth":
            want, nf = parity_scenes.oracle_render(pos, h, m, None, None, 1, M, sf, R, mips, **kw)
        elif mode == "weighted":
            want, nf = parity_scenes.oracle_render(pos, h, m, q, None, 0, M, sf, R, mips, **kw)
            terms = parity_scenes.oracle_render(pos, h, m, np.abs(q), None, 0, M, sf, R, mips, **kw)[0][..., 1]
        else:
            want, nf = parity_scenes.oracle_render(pos, h, m, None, None, 0, M, sf, R, mips, **kw)
        want.setflags(write=False)
        _range_cache[key] = (want, int(nf), terms)
    return _range_cache[key]


# ---- 1. parity with the oracle ------------------------------------------------------------------------------------------------
PARITY = ([(k, [0] * G) for k in KINDS for G in (2, 3, 5)] + [("interleaved4096", [0, 0, 0]), ("group", [0, 1]), ("contiguous", [0, 1])])


@pytest.mark.parametrize("kind,devices", PARITY, ids=[f"{k}-{'x'.join(map(str, d))}" for k, d in PARITY])
def test_sharded_frame_equals_the_oracle(native, mips, scene, camera, kind, devices):
    _need(native, devices)
    n = len(scene["h"])
    drv = Driver(native, kind, devices, mips)
    one = native.Context(R, 4)
    try:
        assert [m.num_particles for m in drv.members] == [0] * drv.G
        for mode in MODES:
            drv.upload(scene, mode)
            assert drv.d.num_particles == n
            assert [m.num_particles for m in drv.members] == [len(drv.owned(g, n)) for g in range(drv.G)]
            if kind == "interleaved4096":
                assert [m.num_particles for m in drv.members] == [n, 0, 0]        # one block: every other shard is empty
            drv.render(camera, mode)
            _check_frame(drv, camera, mode, scene, mips, (kind, devices, mode))
            # after the load-time ordering a global index is a position in the concatenation of the shards' new orders
            if kind == "group":
                drv.d.reorder_spatial(4, 7)
            else:
                perm = drv.d.reorder_spatial(4, 7, want_permutation=True)
                assert np.array_equal(np.sort(perm), np.arange(n))
            sc2 = drv.resident_scene(scene, mode)
            assert _same_particles(sc2, scene, mode)
            if kind != "group":
                assert np.array_equal(sc2["pos"], scene["pos"][perm]) and np.array_equal(sc2["h"], scene["h"][perm])
            drv.render(camera, mode)
            _check_frame(drv, camera, mode, sc2, mips, (kind, devices, mode, "reordered"))
            # ... and a range of that order is a range of the oracle's input in that order
            drv.render(camera, mode, [n // 3 - 7], [n // 2])
            want, nfrag, terms = _oracle_ranges(mode, sc2, camera, mips, [n // 3 - 7], [n // 2])
            parity_scenes.compare_with_oracle(drv.frame(), mode, want, terms, (kind, mode, "range after reorder"))
            assert drv.fragments() == nfrag
        # colours from band magnitudes, cut per shard: the one-context contraction, and through it the oracle
        rs = np.random.RandomState(11)
        mags, W = rs.uniform(2.0, 9.0, size=(3, n)), np.diag([0.5, 1.0, 1.0])
        pos = scene["pos"]
        one.set_kernel_mips(mips)
        one.upload_particles(pos[:, 0], pos[:, 1], pos[:, 2], scene["h"], None)
        one.upload_band_magnitudes(mags, W)
        col = one.download_particles(("r", "g", "b"))
        banded = dict(scene, rgb=np.stack([col[k] for k in "rgb"], axis=1))
        drv.d.upload_particles(pos[:, 0], pos[:, 1], pos[:, 2], scene["h"], None)
        drv.d.upload_band_magnitudes(mags, W)
        got = drv.resident(("r", "g", "b"))
        order = np.concatenate([drv.owned(g, n) for g in range(drv.G)]) if kind == "group" else np.arange(n)
        assert all(np.array_equal(got[k], col[k][order]) for k in "rgb"), "the shards' contraction is not the one-context one"
        drv.render(camera, "rgb")
        _check_frame(drv, camera, "rgb", banded, mips, (kind, devices, "band magnitudes"))
    finally:
        drv.close()
        one.close()


# ---- 2. fewer particles than shards, empty shards -----------------------------------------------------------------------------
FEW = [("group", 3), ("group", 5), ("contiguous", 3), ("contiguous", 5), ("interleaved64", 3), ("interleaved4096", 3)]


@pytest.mark.parametrize("kind,G", FEW, ids=[f"{k}-{g}" for k, g in FEW])
def test_fewer_particles_than_shards(native, mips, scene, camera, kind, G):
    drv = Driver(native, kind, [0] * G, mips)
    rs = np.random.RandomState(5)
    try:
        for n in (0, 1, 2, G - 1, G, G + 1):
            sc = _sub(scene, slice(0, n))
            pos = sc["pos"]
            label = (kind, G, n)
            sizes = [len(drv.owned(g, n)) for g in range(G)]
            assert 0 in sizes or n >= G
            # every upload succeeds, whichever shards are empty
            drv.d.upload_particles(pos[:, 0], pos[:, 1], pos[:, 2], sc["h"], sc["m"])
            assert drv.d.num_particles == n and [m.num_particles for m in drv.members] == sizes, label
            drv.d.upload_quantity(sc["q"])
            drv.d.upload_quantity(None)
            drv.render(camera, "density")
            if n:
                _check_frame(drv, camera, "density", sc, mips, label)
            drv.d.upload_quantity(sc["q"])
            drv.d.upload_rgb(sc["rgb"][:, 0].copy(), sc["rgb"][:, 1].copy(), sc["rgb"][:, 2].copy())
            assert drv.d.stats()["n_particles"] == n
            for mode in ("weighted", "depth", "rgb"):
                drv.render(camera, mode)
                if n:
                    _check_frame(drv, camera, mode, sc, mips, label + (mode,))
                else:
                    assert not drv.frame().any() and drv.frame().shape == (R, R, 4 if mode == "rgb" else 2), label
                    assert drv.fragments() == 0
            mags = rs.uniform(2.0, 9.0, size=(3, n))
            drv.d.upload_band_magnitudes(mags, np.diag([0.5, 1.0, 1.0]))
            if n:
                lum = (np.diag([0.5, 1.0, 1.0]) @ 10.0 ** (-0.4 * mags)).astype(np.float32).T        # (tsp_upload_band_magnitudes)
                col = drv.resident(("r", "g", "b"))
                order = np.concatenate([drv.owned(g, n) for g in range(G)]) if kind == "group" else np.arange(n)
                assert np.allclose(np.stack([col[k] for k in "rgb"], axis=1), lum[order], rtol=1e-6, atol=0), label
            drv.d.upload_rgb(sc["rgb"][:, 0].copy(), sc["rgb"][:, 1].copy(), sc["rgb"][:, 2].copy())
            # the load-time ordering and what reports it
            if kind == "group":
                drv.d.reorder_spatial(2, 3)
            else:
                perm = drv.d.reorder_spatial(2, 3, want_permutation=True)
                assert perm.dtype == np.int64 and np.array_equal(np.sort(perm), np.arange(n)), label
                offs = drv.d.strata_offsets()
                assert (len(offs) == 0 and n == 0) or (offs[0] == 0 and offs[-1] == n and (np.diff(offs) >= 0).all()), label
                lays = drv.d.cell_layouts()
                assert len(lays) == sum(s > 0 for s in sizes), label
                assert all(0 <= lay["offsets"][0] <= lay["offsets"][-1] <= n for lay in lays), label
                down = drv.d.download_particles()
                assert all(len(down[k]) == n for k in down), label
                assert np.array_equal(down["h"], sc["h"][perm]), label
            assert drv.d.num_particles == n
            for mode in ("weighted", "rgb"):
                sc2 = drv.resident_scene(sc, mode)
                assert _same_particles(sc2, sc, mode), label
                drv.render(camera, mode)
                if n:
                    _check_frame(drv, camera, mode, sc2, mips, label + (mode, "reordered"))
                else:
                    assert not drv.frame().any(), label
    finally:
        drv.close()


# ---- 3. ranges ----------------------------------------------------------------------------------------------------------------
def _range_cases(n, G):
    b = [(g * n) // G for g in range(G + 1)]
    k = np.arange(40, dtype=np.int64)
    return {
        "straddles every boundary": ([b[1] - 40], [b[G - 1] - b[1] + 90]),
        "inside one shard": ([b[1] + 20], [min(100, b[2] - b[1] - 30)]),
        "negative start": ([-50], [200]),
        "to the end, 2**62": ([b[1] + 200], [2**62]),
        "to the end, INT64_MAX": ([n - 300], [I64_MAX]),
        "everything, from before 0": ([-3], [I64_MAX]),
        "an empty range among others": ([100, 400, n - 600], [50, 0, 30]),
        "descending": ([n - 100, n // 2, 10], [50, 100, 20]),
        "40 short ranges": (list(k * 37 + 5), list(1 + k % 7)),
        "nothing": ([n + 5, 7], [10, 0]),
    }


RANGED = [(k, 3) for k in KINDS] + [("group", 5), ("contiguous", 5), ("interleaved4096", 3)]


@pytest.mark.parametrize("kind,G", RANGED, ids=[f"{k}-{g}" for k, g in RANGED])
def test_ranges_equal_the_oracles_ranges(native, mips, scene, camera, kind, G):
    """Before any reorder a range is a range of the caller's arrays, on the interleaved driver too."""
    n = len(scene["h"])
    drv = Driver(native, kind, [0] * G, mips)
    try:
        for mode in ("weighted", "rgb"):
            drv.upload(scene, mode)
            for name, (starts, lens) in _range_cases(n, G).items():
                drv.render(camera, mode)                         # a full frame first: the block below must clear EVERY shard
                drv.render(camera, mode, starts, lens, clear=True)
                want, nfrag, terms = _oracle_ranges(mode, scene, camera, mips, starts, lens)
                parity_scenes.compare_with_oracle(drv.frame(), mode, want, terms, (kind, G, mode, name))
                assert drv.fragments() == nfrag, (kind, G, mode, name)
                assert drv.d.stats()["n_particles"] == int(_clip(starts, lens, n)[1].sum()), (kind, G, mode, name)
    finally:
        drv.close()


# ---- 4. refinement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS + ("interleaved4096",))
def test_refine_blocks_end_at_the_whole_frame(native, mips, scene, camera, kind):
    n = len(scene["h"])
    drv = Driver(native, kind, [0, 0, 0], mips)
    try:
        for mode in ("weighted", "rgb"):
            drv.upload(scene, mode)
            drv.render(camera, mode, [0], [0], clear=True)                       # an empty first block: the frame starts cleared
            assert not drv.frame().any()
            total = 0
            cuts = [0, 410, 1090, n]
            for a, b in zip(cuts[:-1], cuts[1:]):                                # three clear = False blocks, presented in between
                drv.render(camera, mode, [a], [b - a if b < n else 2**62], clear=False)
                total += drv.fragments()
                want, _, terms = _oracle_ranges(mode, scene, camera, mips, [0], [b])
                parity_scenes.compare_with_oracle(drv.frame(), mode, want, terms, (kind, mode, "prefix", b))
            want, nfrag, terms = parity_scenes.oracle_images(mode, scene, camera[0], camera[1], R, mips)
            parity_scenes.compare_with_oracle(drv.frame(), mode, want, terms, (kind, mode, "three blocks"))
            assert total == nfrag
            # the accumulators stay shard-local and unrounded: two blocks give the one-block frame to float32 rounding
            drv.render(camera, mode, [0], [700], clear=True)
            drv.frame()
            drv.render(camera, mode, [700], [I64_MAX], clear=False)
            two = drv.frame().astype(np.float64)
            drv.render(camera, mode)
            one = drv.frame().astype(np.float64)
            C = 3 if mode == "rgb" else 1                                        # (the weighted channel cancels: it has its own bound above)
            for c in range(C):
                assert np.abs(two[..., c] - one[..., c]).max() <= 2e-7 * one[..., c].max(), (kind, mode, c)
            if mode == "rgb":
                assert np.array_equal(two[..., 3], one[..., 3])
    finally:
        drv.close()


# ---- 5. weights that are not finite, in exactly one shard ---------------------------------------------------------------------
BAD = [640, 655, 670, 690, 700, 835, 850, 870, 880, 895]       # owned by member 1 of 3 under both assignments (block 64: blocks 10, 13)


@pytest.fixture(scope="module")
def bad_scenes(mips):
    """500 particles of each of three routes of test_gpu_nonfinite_weights.py, mixed; per mode the attributes with bad values on
    BAD and that module's Reference (which pixels must be non-finite, the oracle elsewhere)"""
    parts = [nonfinite._scene(route, R, seed) for route, seed in (("small_scattered", 2), ("mid", 3), ("huge", 4))]
    mix = np.random.RandomState(9).permutation(1500)
    sc = {k: np.concatenate([p[k][:500] for p in parts])[mix] for k in ("P", "pxy", "x", "y", "z", "h", "m", "q", "rgb")}
    sc.update(route="mixed", n=1500, R=R)
    on_screen = (np.abs(sc["pxy"][BAD] - R / 2) < R / 2).all(axis=1)
    assert on_screen.sum() >= 3
    out = {}
    for mode in ("weighted", "rgb"):
        att = {k: sc[k].copy() for k in ("x", "y", "z", "h", "m", "q", "rgb")}
        kinds = {"weighted": nonfinite.MASS_KINDS[:3] + nonfinite.Q_KINDS, "rgb": nonfinite.RGB_KINDS[:6]}[mode]
        masks = {}
        for j, i in enumerate(BAD):
            what, val = kinds[j % len(kinds)]
            if what in ("m", "q"):
                att[what][i] = val
            else:
                att["rgb"][i, "rgb".index(what)] = val
            masks.setdefault(what, np.zeros(1500, dtype=bool))[i] = True
        out[mode] = (sc, att, nonfinite.Reference(sc, att, masks, mode, mips))
    return out


@pytest.mark.parametrize("mode", ["weighted", "rgb"])
@pytest.mark.parametrize("kind", KINDS)
def test_nonfinite_weights_in_one_shard(native, mips, bad_scenes, kind, mode):
    sc, att, ref = bad_scenes[mode]
    M, sf, _ = nonfinite._camera(R)
    drv = Driver(native, kind, [0, 0, 0], mips)
    try:
        assert set(BAD) <= set(drv.owned(1, 1500).tolist())
        nonfinite._upload(native, drv.d, mode, att)
        drv.render((M, sf), mode)
        # the bad values live on member 1 alone: the other members' partial images are finite
        assert [bool(np.isfinite(_raw_image(m)[0]).all()) for m in drv.members] == [True, False, True], (kind, mode)
        got = drv.frame()
        ref.check(got, f"{kind}/{mode}")
        assert drv.fragments() == ref.nfrag
    finally:
        drv.close()


# ---- 6. a block that fails on one member is drawn on none ---------------------------------------------------------------------
def _blocks(n):
    run = np.arange(0, n, 250, dtype=np.int64)
    first = (run, np.minimum(125, n - run))
    s2 = np.concatenate([np.arange(a + 125, min(a + 250, n), 5, dtype=np.int64) for a in run])
    second = (s2, np.minimum(5, n - s2))
    return first, second


ROLLBACK = [(k, d) for k in KINDS for d in ([0, 0, 0], [0, 1])]


@pytest.mark.parametrize("failing_clear", [False, True], ids=["refine", "clear"])
@pytest.mark.parametrize("kind,devices", ROLLBACK, ids=[f"{k}-{'x'.join(map(str, d))}" for k, d in ROLLBACK])
def test_block_failing_on_one_member_is_drawn_on_none(native, mips, scene, camera, kind, devices, failing_clear):
    """failing_clear = False: block 2 is a clear = 0 block in the mode of block 1 (a REFINE frame); True: a clear = 1 block in rgb
    over the 2-channel block 1, so that the members that succeed change their channel layout and must get it back."""
    _need(native, devices)
    n, G = len(scene["h"]), len(devices)
    first, second = _blocks(n)
    assert np.array_equal(np.sort(np.concatenate([np.arange(s, s + l) for s, l in zip(*first)] + [np.arange(s, s + l) for s, l in zip(*second)])),
                          np.arange(n))
    mode2 = "rgb" if failing_clear else "weighted"
    failures = [("debug_fail_stage", 1, "after kernel S"), ("debug_fail_stage", 2, "after kernel G"),
                ("debug_fail_alloc", 1, "injected allocation failure")]
    pos = scene["pos"]
    drv = None
    try:
        for option, value, text in failures:
            for g in range(G):
                if drv is None or option == "debug_fail_alloc":      # (a range table that has grown once allocates no more)
                    if drv is not None:
                        drv.close()
                    drv = Driver(native, kind, devices, mips)
                    drv.d.upload_particles(pos[:, 0], pos[:, 1], pos[:, 2], scene["h"], scene["m"])
                    drv.d.upload_quantity(scene["q"])
                    drv.d.upload_rgb(scene["rgb"][:, 0].copy(), scene["rgb"][:, 1].copy(), scene["rgb"][:, 2].copy())
                label = (kind, devices, option, value, "member", g)
                drv.render(camera, "weighted", *first, clear=True)
                frag1 = drv.fragments()
                members = drv.members
                partial = [_raw_image(m) for m in members]
                stats = [m.stats() for m in members]
                before = drv.frame().copy()
                assert all(C == 2 for _, C in partial)
                assert all(s["n_particles"] > 0 for s in stats), "block 1 must reach every member"
                members[g].set_option(option, value)
                with pytest.raises(native.BackendError, match=rf"context {g} .*{text}"):
                    drv.render(camera, mode2, *second, clear=failing_clear)
                members[g].set_option(option, 0)
                for j, m in enumerate(members):
                    img, C = _raw_image(m)
                    assert C == 2, label + ("channel layout of member", j)
                    if kind != "group":
                        assert m.active_channels == 2, label + ("the binding's channel layout of member", j)
                    assert np.array_equal(img, partial[j][0]), label + ("image of member", j)
                    assert m.stats() == stats[j], label + ("statistics of member", j)
                after = drv.frame()
                if drv.rccl:
                    assert np.abs(after.astype(np.float64) - before).max() <= 2e-7 * np.abs(before).max(), label
                else:
                    assert np.array_equal(after, before), label + ("the frame before the failed call",)
                # the same block again: drawn once
                drv.render(camera, mode2, *second, clear=failing_clear)
                assert all(s["n_particles"] > 0 for s in (m.stats() for m in members)), "block 2 must reach every member"
                if failing_clear:
                    want, nfrag, terms = _oracle_ranges("rgb", scene, camera, mips, *second)
                    parity_scenes.compare_with_oracle(drv.frame(), "rgb", want, terms, label)
                    assert drv.fragments() == nfrag, label
                else:
                    want, nfrag, terms = parity_scenes.oracle_images("weighted", scene, camera[0], camera[1], R, mips)
                    parity_scenes.compare_with_oracle(drv.frame(), "weighted", want, terms, label)
                    assert frag1 + drv.fragments() == nfrag, label
    finally:
        if drv is not None:
            drv.close()


def test_render_undo_is_refused_unless_a_render_was_the_last_change(native, mips, scene, camera):
    """tsp_render_undo's own contract on one context: it takes back the last render (accumulator, layout, statistics), once; after
    anything else has changed the image it is refused and changes nothing."""
    ctx = native.Context(R, 4)
    try:
        ctx.set_kernel_mips(mips)
        parity_scenes.upload_scene(ctx, scene, "weighted")
        ctx.upload_rgb(scene["rgb"][:, 0].copy(), scene["rgb"][:, 1].copy(), scene["rgb"][:, 2].copy())
        with pytest.raises(native.BackendError, match="nothing to undo"):
            ctx.render_undo()
        ctx.render(*camera, [0], [700])
        a, st = _raw_image(ctx), ctx.stats()
        ctx.render(*camera, [700], [800], clear=False)
        ab = _raw_image(ctx)
        ctx.render_undo()
        assert np.array_equal(_raw_image(ctx)[0], a[0]) and ctx.stats() == st
        with pytest.raises(native.BackendError, match="nothing to undo"):
            ctx.render_undo()
        ctx.render(*camera, [700], [800], clear=False)                      # the accumulator was put back: A + B again, not A + 2 B
        again = _raw_image(ctx)[0]                                          # (another summation order: the parity tolerances)
        assert np.allclose(again[..., 0], ab[0][..., 0], rtol=1e-5, atol=0)
        assert (np.abs(again[..., 1].astype(np.float64) - ab[0][..., 1]) <= 1e-5 * ab[0][..., 0] * np.abs(scene["q"]).max()).all()
        ab = (again, 2)
        ctx.render(*camera, mode=native.MODE_RGB)                           # a clear = 1 block in another layout
        assert _raw_image(ctx)[1] == 4
        ctx.render_undo()
        assert _raw_image(ctx)[1] == 2 and np.array_equal(_raw_image(ctx)[0], ab[0])
        # after a render that FAILED there is nothing to put back, but the call is valid, once: the presentation image is formed
        # again from the accumulator (here: over a sum another rank handed over) and the context counts as not reduced
        ctx.render(*camera, [0], [700])
        part, st = _raw_image(ctx)[0], ctx.stats()
        ctx.active_channels = 2
        ctx.set_reduced_image(part * np.float32(3.0))
        for option, value in (("debug_fail_alloc", 1), ("debug_fail_stage", 1), ("debug_fail_stage", 2)):      # (the range table grows once)
            ctx.set_option(option, value)
            with pytest.raises(native.BackendError, match="injected"):
                ctx.render(*camera, np.arange(700, 1500, 5), np.full(160, 5), clear=False)
            ctx.set_option(option, 0)
            assert ctx.stats() == st
            assert np.array_equal(_raw_image(ctx)[0], part * np.float32(3.0))          # a failed render leaves the presentation image
            ctx.render_undo()
            assert np.array_equal(_raw_image(ctx)[0], part) and ctx.stats() == st
            with pytest.raises(native.BackendError, match="nothing to undo"):
                ctx.render_undo()
            ctx.set_reduced_image(part * np.float32(3.0))                              # not refused: the context is not reduced
        ctx.render(*camera, [0], [700])
        ctx.active_channels = 2
        ctx.write_image(a[0])
        with pytest.raises(native.BackendError, match="nothing to undo"):
            ctx.render_undo()
        assert np.array_equal(_raw_image(ctx)[0], a[0])
    finally:
        ctx.close()
