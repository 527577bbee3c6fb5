"""Failed device allocations in the uploads leave no half-made state (include/topsy_splat.h, "Failed uploads").

Every allocation of the uploads goes through alloc_group() / scratch_alloc(), so option debug_fail_alloc = k makes the k-th one
fail.  Each test walks k = 1, 2, ... over one entry point and variant until the call succeeds, and the sites reached must be
exactly the set written out in UPLOAD_SITES (test_alloc_sites.py holds the sources to the union of these sets and the others).

  1. Attribute uploads (quantity, rgb, velocities, band magnitudes): after each failure, in this order, (a) the code is
     TSP_ENOMEM with the site's name in tsp_last_error; (b) image, counts and every resident array that can be downloaded are
     what they were, bit for bit (the velocities have no download: (d) covers them); (c) tsp_render_undo still takes the last
     render back and restores its entry image bit for bit; (d) a render in the mode the attribute feeds equals the oracle fed
     the OLD attribute -- or, on a first upload, that mode is still refused and a density render equals the oracle.  At the k
     that succeeds the render equals the oracle fed the NEW attribute.  (d) and the last check are what catch cached vertex
     weights that outlive their attribute (wrgb_source) or are dropped although nothing changed.
  2. Replace-all uploads (tsp_upload_particles, tsp_generate_synthetic) on a context that holds scene A, reordered and rendered:
     after each failure the host-side checks come first, each asserted before the next, so that a library that leaves n > 0
     beside a missing array stops the test before anything is launched: no particles, no array, no layout, every attribute
     upload refused with TSP_ESTATE, image and counts unchanged.  Only then a render (OK, all zeros, n_particles 0) and a
     successful upload of scene B, held to the oracle of B.
  3. The guard of tsp_render / tsp_render_surface (n > 0 with a missing x, y, z or h is TSP_ESTATE) is checked by reading:
     nothing in the library can produce that state any more, and no debug hook fabricates it.  Its lines are the TSP_REQUIRE
     "position / smoothing-length arrays not resident" at the head of render_block() and of tsp_render_surface() in
     topsy_amd/csrc/tsp_api.hip, next to the mass / rgb / velocity checks.
  4. Groups (_native.Group and multigpu.MultiGpuContext, on [0, 0] and, where two cards exist, [0, 1]): the failure is
     injected on ONE member.  A snapshot upload or generation then leaves every member empty and the driver counting 0
     particles; a render draws an all-zero frame; a successful upload matches the oracle.  An attribute upload leaves the failing
     member's attribute bit for bit and every other member's old or new; the upload repeated matches the oracle.
  5. The product path: a `quantity_name` switch whose upload fails raises and leaves the visualizer drawing the previous quantity.

The scene, oracle and tolerances are parity_scenes' (all_class_scene(128): 1500 particles of every footprint class, R = 128,
count_fragments = 1), the kinematic comparison is kinematic_compare's.  Failures are injected only; nothing large is allocated.

Not tested: real (not injected) hipMalloc failures of the uploads -- they take the same two helpers, whose handling of a real
failure is theirs alone; a failing tsp_create; group attribute uploads that are transactional across members (they are not).

Mutations tried on scratch copies of the library, one line each, all of state handling only (none lets a kernel see a missing or
short array), run against this file and test_upload_band_magnitudes of test_gpu_scratch_alloc_failure.py; the tests that failed:
  * tsp_upload_rgb does not reset wrgb_source: test_attribute_upload[upload_rgb-again] and [upload_rgb-reordered] (the render
    after the successful upload shows the old colours) and test_group_attribute_upload[*-rgb-*] on every driver; the two first
    uploads pass, as they must (no weights are cached before them);
  * forget_render_undo() at the head of upload_attributes(), before its allocations: test_attribute_upload[first],
    [reordered] and [first_reordered] of the quantity, rgb and the velocities, the nine that reach a site ("nothing to undo" at
    check (c));
  * tsp_group_upload_particles returning the member's code without empty_after_failure():
    test_group_snapshot_upload[group-0x0-upload_particles-0] and [-1] ("member g still holds particles", 450 of them);
  * tsp_upload_band_magnitudes allocating band_r / band_g / band_b although they are resident:
    test_attribute_upload[upload_band_magnitudes-again] and [-reordered] (after the failure at band_r the colours are gone:
    check (b), before any render) and test_upload_band_magnitudes of test_gpu_scratch_alloc_failure.py.
One mutation was not run, because it lets a kernel see a missing array: p.n = n before the allocations of tsp_upload_particles.
With the clean-up of the failure path (free_particles, which also zeroes p.n) it changes nothing; without that clean-up a failure
at particles_h leaves n > 0 beside h == nullptr, and test_replace_all_upload[particles-*] stops at its first host-side check
(tsp_num_particles == 0), before anything is launched; the guard of 3. would refuse the render besides.
"""
import ctypes

import numpy as np
import pytest

import parity_scenes as ps
from test_gpu_alloc_failure import INJECTED
from test_gpu_scratch_alloc_failure import ENOMEM, SCRATCH_SITES, Outputs, P, _dp, walk

pytestmark = pytest.mark.gpu

R = 128
ESTATE = -4
f32 = np.float32
V_REF = np.array([50.0, -30.0, 20.0], dtype=f32)
AXIS = np.array([0.0, 0.0, 1.0], dtype=f32)
ARRAYS = ("x", "y", "z", "h", "mass", "q", "r", "g", "b")            # tsp_download_particles' order
H_CAP = 40.0        # of the generated snapshots (shard [100, 1300) of 2000): footprints up to 102 px at scale 100, every class

_PARTICLES = {"particles_x", "particles_y", "particles_z", "particles_h"}
_SYNTHETIC = {"synthetic_x", "synthetic_y", "synthetic_z", "synthetic_h", "synthetic_mass"}
_BAND = SCRATCH_SITES["upload_band_magnitudes"]                      # the two staging buffers, walked there on a re-upload too
# (entry point, variant) -> the sites reached.  Attribute variants: "first" (not resident yet), "again" (resident),
# "reordered" (resident, after tsp_reorder_spatial), "first_reordered" (not resident, after tsp_reorder_spatial)
UPLOAD_SITES = {
    ("upload_quantity", "first"): {"quantity_q"},
    ("upload_quantity", "again"): set(),
    ("upload_quantity", "reordered"): {"quantity_staging"},
    ("upload_quantity", "first_reordered"): {"quantity_staging", "quantity_q"},
    ("upload_rgb", "first"): {"rgb_r", "rgb_g", "rgb_b"},
    ("upload_rgb", "again"): set(),
    ("upload_rgb", "reordered"): {"rgb_staging"},
    ("upload_rgb", "first_reordered"): {"rgb_staging", "rgb_r", "rgb_g", "rgb_b"},
    ("upload_velocities", "first"): {"velocities_x", "velocities_y", "velocities_z"},
    ("upload_velocities", "again"): set(),
    ("upload_velocities", "reordered"): {"velocities_staging"},
    ("upload_velocities", "first_reordered"): {"velocities_staging", "velocities_x", "velocities_y", "velocities_z"},
    ("upload_band_magnitudes", "first"): _BAND | {"band_r", "band_g", "band_b"},
    ("upload_band_magnitudes", "again"): _BAND,
    ("upload_band_magnitudes", "reordered"): _BAND,
    ("upload_band_magnitudes", "first_reordered"): _BAND | {"band_r", "band_g", "band_b"},
    ("upload_particles", "mass"): _PARTICLES | {"particles_mass"},
    ("upload_particles", "no_mass"): _PARTICLES,
    ("upload_particles", "larger"): _PARTICLES | {"particles_mass"},
    ("generate_synthetic", "plain"): _SYNTHETIC,
    ("generate_synthetic", "quantity"): _SYNTHETIC | {"synthetic_q"},
    ("generate_synthetic", "rgb"): _SYNTHETIC | {"synthetic_r", "synthetic_g", "synthetic_b"},
}
VARIANTS = ("first", "again", "reordered", "first_reordered")


@pytest.fixture(scope="module")
def native():
    from topsy_amd import _native
    _native.load_library()
    return _native


def _frozen(sc):
    for a in sc.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return sc


def _scene(n, seed):
    """all_class_scene with velocities, band magnitudes (whose contraction is its "rgb") and a second set of every attribute"""
    from oracle import oracle_np
    sc = ps.all_class_scene(R, n=n, seed=seed)
    rs = np.random.RandomState(100 + seed)
    sc["vel"] = (rs.normal(0.0, 100.0, size=sc["pos"].shape) + V_REF).astype(f32)
    new = dict(sc)
    new["q"] = rs.normal(size=n).astype(f32)
    new["rgb"] = rs.uniform(0.0, 1.0, size=(n, 3)).astype(f32)
    new["vel"] = (rs.normal(0.0, 60.0, size=sc["pos"].shape) - V_REF).astype(f32)
    band = []
    for _ in range(2):
        mags = np.ascontiguousarray(rs.uniform(2.0, 14.0, size=(3, n)))
        band.append((mags, dict(sc, rgb=np.ascontiguousarray(oracle_np.band_contraction(mags, BAND_WEIGHTS).astype(f32)))))
    return _frozen(sc), _frozen(new), band


BAND_WEIGHTS = np.ascontiguousarray(np.diag([0.5, 1.0, 1.0]))


@pytest.fixture(scope="module")
def scenes():
    """A: (old, new, band) of 1500 particles; B: 900 particles; B_large: 2100"""
    return {"A": _scene(1500, 1), "B": _scene(900, 2), "B_large": _scene(2100, 3)}


@pytest.fixture(scope="module")
def camera():
    from oracle import oracle_np
    M, sf = oracle_np.transform_matrix(np.eye(3), np.zeros(3), 100.0)
    return M, float(sf)


def new_context(native, mips, sc, mass=True):
    ctx = native.Context(R, 4)
    ctx.set_kernel_mips(mips)
    ctx.set_option("count_fragments", 1)
    ctx.set_line_of_sight(AXIS, V_REF)
    upload_particles(ctx, sc, mass)
    return ctx


def upload_particles(ctx, sc, mass=True):
    p = sc["pos"]
    ctx.upload_particles(p[:, 0], p[:, 1], p[:, 2], sc["h"], sc["m"] if mass else None)


def cols(a):
    return [np.ascontiguousarray(a[:, k]) for k in range(3)]


def shows(native, mips, camera, ctx, mode, sc, what):
    """a render in `mode` equals the oracle fed `sc`, fragment count included"""
    M, sf = camera
    if mode != "kinematic":
        ps.render_and_check(ctx, native, mode, sc, M, sf, R, mips, 1, label=what)
        return
    from kinematic_compare import check_kinematic, oracle_kinematic
    ctx.render(M, sf, mode=native.MODE_KINEMATIC)
    want, nfrag, terms = oracle_kinematic(sc, mips, M, sf, AXIS, V_REF)
    check_kinematic(ctx.read_image(), want, terms, what)
    assert ctx.stats()["n_fragments"] == nfrag, what


def resident(ctx):
    """every array tsp_download_particles hands out, or None where it is not resident (TSP_ESTATE)"""
    out = {}
    for i, name in enumerate(ARRAYS):
        buf = np.empty(max(ctx.num_particles, 1), dtype=f32)
        rc = ctx._lib.tsp_download_particles(ctx._h, *[P(buf) if j == i else None for j in range(len(ARRAYS))])
        assert rc in (0, ESTATE), (name, rc)
        out[name] = buf[:ctx.num_particles].copy() if rc == 0 else None
    return out


def assert_same_arrays(before, after, what):
    for name in ARRAYS:
        assert (before[name] is None) == (after[name] is None), f"{what}: array {name} appeared or went"
        if before[name] is not None:
            assert np.array_equal(before[name].view(np.uint32), after[name].view(np.uint32)), f"{what}: resident array {name} changed"


# ---- 1. attribute uploads ------------------------------------------------------------------------------------------------------
def _attribute(entry, lib, ctx, old, new, band):
    """(mode the attribute feeds, upload of the old values through the binding, raw upload of the new ones, scene after it)"""
    if entry == "upload_quantity":
        return "weighted", lambda: ctx.upload_quantity(old["q"]), lambda: lib.tsp_upload_quantity(ctx._h, P(new["q"])), dict(old, q=new["q"])
    if entry == "upload_rgb":
        c = cols(new["rgb"])
        return ("rgb", lambda: ctx.upload_rgb(*cols(old["rgb"])), lambda: lib.tsp_upload_rgb(ctx._h, P(c[0]), P(c[1]), P(c[2])),
                dict(old, rgb=new["rgb"]))
    if entry == "upload_velocities":
        c = cols(new["vel"])
        return ("kinematic", lambda: ctx.upload_velocities(*cols(old["vel"])),
                lambda: lib.tsp_upload_velocities(ctx._h, P(c[0]), P(c[1]), P(c[2])), dict(old, vel=new["vel"]))
    (m0, _), (m1, sc1) = band
    return ("rgb", lambda: ctx.upload_band_magnitudes(m0, BAND_WEIGHTS),
            lambda: lib.tsp_upload_band_magnitudes(ctx._h, 3, P(m1, _dp), P(BAND_WEIGHTS, _dp)), sc1)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("entry", ["upload_quantity", "upload_rgb", "upload_velocities", "upload_band_magnitudes"])
def test_attribute_upload(native, mips, scenes, camera, entry, variant):
    lib = native.load_library()
    old, new, band = scenes["A"]
    if entry == "upload_band_magnitudes":
        old = band[0][1]
    ctx = new_context(native, mips, old)
    try:
        mode, upload_old, upload_new, after = _attribute(entry, lib, ctx, old, new, band)
        first = variant.startswith("first")
        if not first:
            upload_old()
        if variant.endswith("reordered"):
            ctx.reorder_spatial(4, 7)
        # what the context draws while the new values are not there: the attribute's mode, or -- before a first upload, when
        # that mode is refused -- the density (the context holds no quantity then)
        old_mode = "density" if first else mode
        native_mode = {"weighted": native.MODE_WEIGHTED, "rgb": native.MODE_RGB, "kinematic": native.MODE_KINEMATIC}[mode]
        state = {}

        def draw(sc, what):
            state["entry"] = ctx.read_image()
            shows(native, mips, camera, ctx, old_mode if sc is old else mode, sc, what)

        draw(old, "before the walk")              # (the cached weights of the mode exist now)
        draw(old, "before the walk, again")       # (... and tsp_render_undo has an entry image of this layout to go back to)
        arrays = resident(ctx)

        def after_failure(what):
            assert_same_arrays(arrays, resident(ctx), what)                                               # (b), beyond walk's own
            ctx.render_undo()                                                                             # (c)
            assert np.array_equal(ctx.read_image().view(np.uint32), state["entry"].view(np.uint32)), f"{what}: the undone image"
            with pytest.raises(native.BackendError, match="nothing to undo"):
                ctx.render_undo()
            if first and mode != "weighted":
                with pytest.raises(native.BackendError, match="not uploaded"):
                    ctx.render(*camera, mode=native_mode)
                ctx.active_channels = 2
            draw(old, what + ", the old values")                                                          # (d)

        walk(native, ctx, upload_new, Outputs(), UPLOAD_SITES[(entry, variant)], after_failure=after_failure)
        draw(after, "after the upload")
        draw(after, "after the upload, again")
    finally:
        ctx.close()


# ---- 2. replace-all uploads ----------------------------------------------------------------------------------------------------
def assert_empty(native, ctx, image, counts, what):
    """the ordered host-side checks: nothing here launches a kernel on particle data"""
    lib = ctx._lib
    assert lib.tsp_num_particles(ctx._h) == 0, f"{what}: tsp_num_particles"
    one = np.zeros(4, dtype=f32)
    for i, name in enumerate(ARRAYS):
        rc = lib.tsp_download_particles(ctx._h, *[P(one) if j == i else None for j in range(len(ARRAYS))])
        assert rc == ESTATE, f"{what}: array {name} is still resident (code {rc})"
    ints, floats = [ctypes.c_int(0), ctypes.c_int(0)], [np.zeros(3, dtype=f32), np.zeros(3, dtype=f32)]
    assert lib.tsp_get_cell_layout(ctx._h, ctypes.byref(ints[0]), ctypes.byref(ints[1]), P(floats[0]), P(floats[1])) == ESTATE, what
    offsets = np.zeros(8, dtype=np.int64)
    assert lib.tsp_get_strata_offsets(ctx._h, offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 8) == 0, what
    d = np.zeros(4, dtype=np.float64)
    for name, rc in (("quantity", lib.tsp_upload_quantity(ctx._h, P(one))), ("rgb", lib.tsp_upload_rgb(ctx._h, P(one), P(one), P(one))),
                     ("velocities", lib.tsp_upload_velocities(ctx._h, P(one), P(one), P(one))),
                     ("band magnitudes", lib.tsp_upload_band_magnitudes(ctx._h, 1, P(d, _dp), P(d, _dp)))):
        assert rc == ESTATE, f"{what}: the upload of {name} returned {rc}"
    assert np.array_equal(ctx.read_image().view(np.uint32), image.view(np.uint32)), f"{what}: the image changed"
    assert {k: v for k, v in ctx.stats().items() if not k.startswith("ms_")} == counts, f"{what}: the statistics changed"


def assert_draws_nothing(ctx, camera, what):
    ctx.render(*camera)
    assert ctx.stats()["n_particles"] == 0 and not ctx.read_image().any(), f"{what}: an empty context drew something"


def synthetic_scene(ctx, with_q, with_rgb):
    """the generated snapshot as resident: what the oracle is fed"""
    names = ("x", "y", "z", "h", "mass") + (("q",) if with_q else ()) + (("r", "g", "b") if with_rgb else ())
    got = ctx.download_particles(names)
    n = len(got["x"])
    zero = np.zeros(n, dtype=f32)
    rgb = np.stack([got[k] for k in "rgb"], axis=1) if with_rgb else np.zeros((n, 3), dtype=f32)
    return ps.make_scene(np.stack([got["x"], got["y"], got["z"]], axis=1), got["h"], got["mass"], got.get("q", zero), rgb, scale=100.0)


REPLACE_ALL = [("upload_particles", "mass"), ("upload_particles", "no_mass"), ("upload_particles", "larger"),
               ("generate_synthetic", "plain"), ("generate_synthetic", "quantity"), ("generate_synthetic", "rgb")]


@pytest.mark.parametrize("entry,variant", REPLACE_ALL, ids=[f"{e.split('_')[1]}-{v}" for e, v in REPLACE_ALL])
def test_replace_all_upload(native, mips, scenes, camera, entry, variant):
    lib = native.load_library()
    A = scenes["A"][0]
    B = scenes["B_large" if variant == "larger" else "B"][0]
    mode_a = "rgb" if variant == "no_mass" else "weighted"
    ctx = new_context(native, mips, A, mass=variant != "no_mass")
    px, py, pz = cols(B["pos"])

    def load_a():
        """scene A, reordered and rendered"""
        upload_particles(ctx, A, mass=variant != "no_mass")
        if mode_a == "rgb":
            ctx.upload_rgb(*cols(A["rgb"]))
        else:
            ctx.upload_quantity(A["q"])
            ctx.upload_velocities(*cols(A["vel"]))
        ctx.reorder_spatial(4, 7)
        shows(native, mips, camera, ctx, mode_a, A, "scene A")

    def call():
        if entry == "upload_particles":
            return lib.tsp_upload_particles(ctx._h, len(px), P(px), P(py), P(pz), P(B["h"]), None if variant == "no_mass" else P(B["m"]))
        return lib.tsp_generate_synthetic(ctx._h, 2000, 100, 1200, 99, H_CAP, int(variant == "quantity"), int(variant == "rgb"))

    def check_new(what):
        """what the successful call left draws as the oracle says"""
        if entry == "generate_synthetic":
            mode = {"plain": "density", "quantity": "weighted", "rgb": "rgb"}[variant]
            sc = synthetic_scene(ctx, variant == "quantity", variant == "rgb")
            assert len(sc["h"]) == 1200
        elif variant == "no_mass":
            ctx.upload_rgb(*cols(B["rgb"]))
            mode, sc = "rgb", B
        else:
            ctx.upload_quantity(B["q"])
            mode, sc = "weighted", B
        shows(native, mips, camera, ctx, mode, sc, what)

    try:
        reached = []
        for k in range(1, 16):
            load_a()
            image, counts = ctx.read_image(), {k_: v for k_, v in ctx.stats().items() if not k_.startswith("ms_")}
            ctx.set_option("debug_fail_alloc", k)
            rc = call()
            err = lib.tsp_last_error().decode(errors="replace")
            ctx.set_option("debug_fail_alloc", 0)
            if rc == 0:
                break
            found = INJECTED.search(err)
            assert rc == ENOMEM and found, f"k={k}: return code {rc}, not the injected failure: {err}"
            reached.append(found.group(1))
            what = f"after a failure at {reached[-1]} (k={k})"
            assert_empty(native, ctx, image, counts, what)
            ctx.active_channels = 4 if mode_a == "rgb" else 2
            assert_draws_nothing(ctx, camera, what)
            assert call() == 0, what                                      # the same call, nothing injected
            check_new(what + ", then the call again")
        else:
            pytest.fail("the call still failed at k=15")
        check_new("after the call that succeeded")
        print(f"\nallocation sites reached: {reached}")
        assert len(set(reached)) == len(reached), f"a site failed twice: {reached}"
        assert set(reached) == UPLOAD_SITES[(entry, variant)], reached
    finally:
        ctx.close()


# ---- 4. groups -----------------------------------------------------------------------------------------------------------------
DRIVERS = [("group", [0, 0]), ("group", [0, 1]), ("contiguous", [0, 0])]
DRIVER_IDS = [f"{k}-{'x'.join(map(str, d))}" for k, d in DRIVERS]


def _driver(native, mips, kind, devices):
    import test_gpu_shard_edges as edges
    edges._need(native, devices)
    return edges.Driver(native, kind, devices, mips), edges


@pytest.mark.parametrize("failing", [0, 1])
@pytest.mark.parametrize("entry", ["upload_particles", "generate_synthetic"])
@pytest.mark.parametrize("kind,devices", DRIVERS, ids=DRIVER_IDS)
def test_group_snapshot_upload(native, mips, scenes, camera, kind, devices, entry, failing):
    A, B = scenes["A"][0], scenes["B"][0]
    drv, edges = _driver(native, mips, kind, devices)
    try:
        drv.upload(A, "weighted")
        drv.render(camera, "weighted")
        edges._check_frame(drv, camera, "weighted", A, mips, "scene A")

        def call():
            if entry == "upload_particles":
                drv.upload(B, "weighted")
            else:
                drv.d.generate_synthetic(2000, 100, 1200, 99, H_CAP, with_quantity=True)

        site = "particles_x" if entry == "upload_particles" else "synthetic_x"
        drv.members[failing].set_option("debug_fail_alloc", 1)
        with pytest.raises(native.BackendError, match=rf"injected allocation failure at {site}") as e:
            call()
        if kind == "group":
            assert f"context {failing} " in str(e.value)
        for g, m in enumerate(drv.members):
            m.set_option("debug_fail_alloc", 0)
            assert m.num_particles == 0, f"member {g} still holds particles"
            assert all(v is None for v in resident(m).values()), f"member {g} still holds an array"
        assert drv.d.num_particles == 0
        drv.render(camera, "weighted")
        assert not drv.frame().any() and drv.d.stats()["n_particles"] == 0
        call()
        if entry == "upload_particles":
            drv.render(camera, "weighted")
            edges._check_frame(drv, camera, "weighted", B, mips, "scene B")
        else:
            assert drv.d.num_particles == 1200
            sc = drv.resident_scene({"scale": 100.0}, "weighted")
            drv.render(camera, "weighted")
            edges._check_frame(drv, camera, "weighted", sc, mips, "the generated snapshot")
    finally:
        drv.close()


@pytest.mark.parametrize("failing", [0, 1])
@pytest.mark.parametrize("attribute", ["quantity", "rgb"])
@pytest.mark.parametrize("kind,devices", DRIVERS, ids=DRIVER_IDS)
def test_group_attribute_upload(native, mips, scenes, camera, kind, devices, attribute, failing):
    """on members that were reordered, so that a repeated upload allocates (the staging of the permutation)"""
    old, new, _ = scenes["A"]
    mode, names = ("weighted", ("q",)) if attribute == "quantity" else ("rgb", ("r", "g", "b"))
    after = dict(old, q=new["q"]) if attribute == "quantity" else dict(old, rgb=new["rgb"])
    drv, edges = _driver(native, mips, kind, devices)
    try:
        p = old["pos"]
        drv.d.upload_particles(p[:, 0], p[:, 1], p[:, 2], old["h"], old["m"])
        upload = (lambda sc: drv.d.upload_quantity(sc["q"])) if attribute == "quantity" else (lambda sc: drv.d.upload_rgb(*cols(sc["rgb"])))
        upload(old)
        drv.d.reorder_spatial(8, 7)
        drv.render(camera, mode)
        edges._check_frame(drv, camera, mode, old, mips, "the old values")
        members = drv.members
        before = [m.download_particles(names) for m in members]
        members[failing].set_option("debug_fail_alloc", 1)
        with pytest.raises(native.BackendError, match=rf"injected allocation failure at {attribute}_staging"):
            upload(after)
        for g, m in enumerate(members):
            m.set_option("debug_fail_alloc", 0)
            got = m.download_particles(names)
            own = drv.owned(g, len(old["h"]))
            for c, name in enumerate(names):
                is_old = np.array_equal(got[name].view(np.uint32), before[g][name].view(np.uint32))
                if g == failing:
                    assert is_old, f"the failing member's {name} changed"
                else:
                    values = after["q"] if attribute == "quantity" else after["rgb"][:, c]
                    assert is_old or np.array_equal(np.sort(got[name]), np.sort(values[own])), f"member {g} holds neither the old nor the new {name}"
        upload(after)
        drv.render(camera, mode)
        edges._check_frame(drv, camera, mode, after, mips, "the new values")
    finally:
        drv.close()


# ---- 5. the product path ---------------------------------------------------------------------------------------------------------
def test_failed_quantity_switch_keeps_the_previous_quantity(native):
    import topsy_amd
    from test_gpu_smoothing import _same_image
    from topsy_amd.drawreason import DrawReason
    rs = np.random.RandomState(8)
    n = 4000
    pos = (rs.normal(size=(n, 3)) * 4.0).astype(f32)
    h = rs.uniform(0.2, 1.5, n).astype(f32)
    mass = rs.uniform(0.5, 2.0, n).astype(f32)
    quantities = {"temp": rs.lognormal(size=n).astype(f32), "metals": rs.uniform(0.1, 5.0, n).astype(f32)}
    vis = topsy_amd.from_arrays(pos, h, mass, quantities=quantities, render_resolution=R)
    try:
        def image():
            vis.render_sph(DrawReason.EXPORT)
            return np.array(vis.get_sph_image(), copy=True)

        vis.scale = 12.0
        vis.quantity_name = "temp"
        temp = image()
        ctx = vis.particle_buffers.context
        ctx.set_option("debug_fail_alloc", 1)                  # the switch's upload: its staging (the loader's order was permuted)
        with pytest.raises(native.BackendError, match="injected allocation failure at quantity_staging"):
            vis.quantity_name = "metals"
        ctx.set_option("debug_fail_alloc", 0)
        assert vis.quantity_name == "temp"
        _same_image(image(), temp)
        vis.quantity_name = "metals"                           # a second attempt succeeds
        assert vis.quantity_name == "metals"
        metals = image()
        assert metals.shape == temp.shape and not np.allclose(metals, temp, rtol=1e-3, equal_nan=True)
        vis.quantity_name = "temp"
        _same_image(image(), temp)
    finally:
        vis.close()
