"""tsp_group_potential and tsp_halo_properties on the GPU against the numpy model of halo_ref.py.

Potential: per member |got - want| <= 64 * 2^-24 * sum |term| (the bound of tsp_gravity_direct, which the pair arithmetic is).
Properties: counts and chosen members exact, every float64 sum within 8 (n_h + 16) 2^-53 times its natural scale -- the
summation-order bound: n_h additions, each within 2^-53 of a partial sum that the scale bounds, with room for the terms' own
roundings (derived, not measured) -- radii within 4 ulp, the same bits on a second call.  The model follows the documented
association of the sums, so that the radii, which hang on the centre of mass, can be held to ulps.

The scenes edges, giants and legion of halo_ref.py reach what the small ones cannot: pieces on every slice boundary, haloes of more
than 64 pieces (halo_combine's chunks of 2 and 3), blocks at the cap of 16 work items, a second launch.  Their haloes are too large
for a full float64 matrix: the potential is held to the model at about a thousand sampled members (halo_ref.target_sample), to its
NaN pattern everywhere, and two giants member by member to tsp_gravity_direct.  pair_slots is held to the planning rule
(halo_ref.work_items) in every potential test."""
import ctypes

import numpy as np
import pytest

import halo_ref as ref
from test_gpu_scratch_alloc_failure import Outputs, P, assert_same_state, col, frame_ctx, native, snapshot, walk  # noqa: F401

pytestmark = pytest.mark.gpu

f32 = np.float32
_dp = ctypes.POINTER(ctypes.c_double)
_i64p = ctypes.POINTER(ctypes.c_int64)
_i32p = ctypes.POINTER(ctypes.c_int32)
EINVAL = -1
SUM_BOUND = 8.0 * 2.0 ** -53


@pytest.fixture(scope="module")
def ctx(native):
    c = native.Context(1, 2)
    yield c
    c.close()


def xyz(scene):
    return [np.ascontiguousarray(scene["pos"][:, k]) for k in range(3)]


def gpu_potential(ctx, scene, max_members=0):
    x, y, z = xyz(scene)
    return ctx.group_potential(x, y, z, scene["mass"], scene["eps"], scene["labels"], scene["n_groups"], scene["period"], max_members)


def gpu_properties(ctx, scene, phi=None, with_vel=True):
    x, y, z = xyz(scene)
    vel = [np.ascontiguousarray(scene["vel"][:, k]) for k in range(3)] if with_vel else None
    return ctx.halo_properties(x, y, z, scene["mass"], scene["labels"], scene["n_groups"], vel=vel, phi=phi, period=scene["period"])


def check_potential(got, model, what, max_members=0, only=None):
    """The values against the model's -- at every member, or at model["targets"] where the model is a sampled one (restricted to
    the boolean mask `only`, if given) --, the NaN pattern over the whole array, info against the model's and pair_slots against
    the planning rule (halo_ref.work_items).  Returns the worst |got - want| / (64 * 2^-24 * sum |term|)."""
    phi, info = got
    want, scale = model["phi"], model["scale"]
    assert np.array_equal(np.isnan(phi), ~model["member_has_value"]), f"{what}: NaN where the model has a value, or a value where it has NaN"
    ok = model["member_has_value"].copy()
    if model["targets"] is None:
        assert np.array_equal(np.isnan(phi), np.isnan(want)), f"{what}: NaN where the model has a value, or a value where it has NaN"
    else:
        ok[:] = False
        ok[model["targets"]] = True
        ok &= model["member_has_value"]
        assert not np.isnan(want[ok]).any()
    if only is not None:
        ok &= only
    err, bound = np.abs(phi[ok] - want[ok]), ref.K * ref.U * scale[ok]
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = ratio.max() if len(ratio) else 0.0
    print(f"\n{what}: worst |got - want| / (64 * 2^-24 * sum |term|) = {worst:.4f} ({ref.K * worst:.2f} in units of 2^-24 sum |term|) "
          f"over {ok.sum()} members")
    assert (err <= bound).all(), f"{what}: {np.count_nonzero(err > bound)} members outside the bound, worst ratio {ratio.max()}"
    for k, v in model["info"].items():
        assert info[k] == v, f"{what}: info.{k} = {info[k]}, the model has {v}"
    if "pair_slots" in info:
        mirror = ref.work_items(model["counts"], max_members)["pair_slots"]
        assert info["pair_slots"] == mirror, f"{what}: pair_slots = {info['pair_slots']}, the planning rule gives {mirror}"
    return worst


@pytest.mark.parametrize("name", ["clumps", "periodic", "crumbs", "nonfinite", "edges", "edges+1"])
def test_potential(ctx, name):
    scene, model, _ = ref.reference(name)
    got = gpu_potential(ctx, scene)
    check_potential(got, model, name)
    again = gpu_potential(ctx, scene)
    assert np.array_equal(got[0].view(np.uint64), again[0].view(np.uint64)) and got[1] == again[1], "a second call gives other bits"
    assert got[1]["pair_slots"] >= got[1]["pairs"] and got[1]["pair_slots"] % (512 * 1024) == 0
    if name == "nonfinite":
        assert np.isnan(got[0]).sum() == ref.N_BACKGROUND + 5


def sorted_position(scene):
    """the sorted position of every particle, -1 for one that is no member"""
    index = ref.sorted_positions(scene)[0]
    where = np.full(len(scene["pos"]), -1, dtype=np.int64)
    where[index] = np.arange(len(index))
    return where


def test_potential_giants(ctx):
    """haloes of 64 to 129 pieces, every block at the cap of 16 work items: the model at the sampled members (halo_ref.target_sample)"""
    scene, model, _ = ref.reference("giants")
    got = gpu_potential(ctx, scene)
    check_potential(got, model, "giants")
    again = gpu_potential(ctx, scene)
    assert np.array_equal(got[0].view(np.uint64), again[0].view(np.uint64)) and got[1] == again[1], "a second call gives other bits"
    assert got[1]["pair_slots"] >= got[1]["pairs"] and got[1]["pair_slots"] % (512 * 1024) == 0


def test_potential_legion(ctx):
    """more than 4096 work items: two launches, the second one's slots numbered from 0 again over the same partials"""
    scene, model, _ = ref.reference("legion")
    got = gpu_potential(ctx, scene)
    check_potential(got, model, "legion")
    plan = ref.work_items(model["counts"])
    assert len(plan["launches"]) == 2
    second = sorted_position(scene) >= plan["launches"][1][0] * 1024
    assert second[model["targets"]].sum() >= 50
    check_potential(got, model, f"legion, the blocks {plan['launches'][1][:2]} of the second launch", only=second)
    again = gpu_potential(ctx, scene)
    assert np.array_equal(got[0].view(np.uint64), again[0].view(np.uint64)) and got[1] == again[1], "a second call gives other bits"
    assert got[1]["pair_slots"] >= got[1]["pairs"] and got[1]["pair_slots"] % (512 * 1024) == 0


@pytest.mark.parametrize("which", ["aligned_32769", "misaligned_16384"])
def test_giant_against_the_direct_sum(ctx, which):
    """Every member of a giant against tsp_gravity_direct on the model's float32 offsets of that halo alone.  Masses are positive,
    so sum |term| = |phi|; both kernels are within K * U * sum |term| of the same float64 sum over the same float32 e, m and
    eps^2 (tsp_gravity.hip squares eps in float32 too: gravity_prepare_kernel): |a - b| <= 2 K U |phi|.  The sampled model sees
    a thousand targets; an error in some lanes, planes or blocks of the others shows here."""
    scene = ref.reference("giants")[0]
    a = gpu_potential(ctx, scene)[0]
    idx = np.flatnonzero(scene["labels"] == ref.GIANT_LABELS[which])        # ascending: the sorted order of the halo
    assert len(idx) == ref.GIANT_SIZES[ref.GIANT_LABELS[which] - 1] and np.isfinite(a[idx]).all()
    e = ref.offsets(scene["pos"], idx, scene["period"]).astype(f32)
    b = ctx.gravity_direct(np.ascontiguousarray(e[:, 0]), np.ascontiguousarray(e[:, 1]), np.ascontiguousarray(e[:, 2]),
                           scene["mass"][idx], scene["eps"][idx], want_acc=False)[0]
    ratio = np.abs(a[idx] - b) / (2 * ref.K * ref.U * np.abs(a[idx]))
    print(f"\ngiants, {which}: worst |group - direct| / (2 * 64 * 2^-24 |phi|) = {ratio.max():.4f} over {len(idx)} members")
    assert (a[idx] < 0).all() and (ratio <= 1.0).all(), f"{np.count_nonzero(ratio > 1.0)} members outside the bound"


@pytest.mark.parametrize("how", ["sorted", "reversed", "permuted"])
def test_potential_in_another_order(ctx, how):
    """each order is held to the model with its own anchors; the orders agree within the sum of the bounds"""
    scene, model, _ = ref.reference("periodic")
    other, order = ref.reordered(scene, how)
    other_model = ref.potential_model(other)
    got = gpu_potential(ctx, other)
    check_potential(got, other_model, f"periodic, {how}")
    first = gpu_potential(ctx, scene)[0][order]
    ok = ~np.isnan(first)
    assert (np.abs(first[ok] - got[0][ok]) <= ref.K * ref.U * (model["scale"][order][ok] + other_model["scale"][ok])).all()


def test_potential_with_one_softening_length(ctx):
    scene = dict(ref.reference("clumps")[0], eps=f32(3e-4))
    check_potential(gpu_potential(ctx, scene), ref.potential_model(scene), "clumps, eps_all")


def test_skip(ctx):
    scene, model, _ = ref.reference("clumps")
    phi, info = gpu_potential(ctx, scene, max_members=1000)
    check_potential((phi, info), ref.potential_model(scene, max_members=1000), "clumps, max_members = 1000", max_members=1000)
    assert info["n_skipped_groups"] == 4 and info["n_skipped_members"] == 3000 + 1025 + 1024 + 1023
    big = np.isin(scene["labels"], [1, 2, 3, 4])
    assert np.isnan(phi[big]).all() and not np.isnan(phi[scene["labels"] >= 5]).any()


def test_skip_giants(ctx):
    """the two largest haloes of legion skipped: 63 blocks in the middle of the catalogue have no work item, one launch"""
    scene, full, _ = ref.reference("legion")
    limit = ref.LEGION_MAX_MEMBERS
    model = ref.potential_model(scene, max_members=limit, targets=full["targets"])
    phi, info = gpu_potential(ctx, scene, max_members=limit)
    check_potential((phi, info), model, f"legion, max_members = {limit}", max_members=limit)
    assert info["n_skipped_groups"] == 2 and info["n_skipped_members"] == 32768 + 32769
    big = np.isin(scene["labels"], [ref.GIANT_LABELS["aligned_32768"], ref.GIANT_LABELS["aligned_32769"]])
    assert np.isnan(phi[big]).all() and not np.isnan(phi[(scene["labels"] >= 1) & ~big]).any()
    # a halo that is not skipped has the bits it has without the limit: its blocks' ranges and items are the same
    first = scene["labels"] == ref.GIANT_LABELS["aligned_16384"]
    assert np.array_equal(phi[first].view(np.uint64), gpu_potential(ctx, scene)[0][first].view(np.uint64))


def test_skipped_haloes_come_from_the_tree(native):
    import topsy_amd
    import tree_gravity_scenes as scenes
    scene, model, _ = ref.reference("periodic")
    phi = topsy_amd.group_potential(scene["pos"], scene["mass"], scene["eps"], scene["labels"], periodicity_scale=1.0, tree_above=1000)
    direct = topsy_amd.group_potential(scene["pos"], scene["mass"], scene["eps"], scene["labels"], periodicity_scale=1.0, G=2.0) / 2.0
    check_potential((direct, model["info"]), model, "periodic through topsy_amd.group_potential")
    big = np.isin(scene["labels"], [1, 2, 3, 4])
    small = ~big & ~np.isnan(direct)
    assert np.array_equal(np.isnan(phi), np.isnan(direct))
    assert (np.abs(phi[small] - direct[small]) <= 2 * ref.K * ref.U * model["scale"][small]).all()
    rel = np.abs(phi[big] / direct[big] - 1.0)
    print(f"\ntree-filled haloes: p99 {np.percentile(rel, 99):.3e}, max {rel.max():.3e} of |tree / direct - 1|")
    assert np.percentile(rel, 99) <= scenes.CAP_P99 and rel.max() <= scenes.CAP_MAX and rel.max() > 0


def ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def check_properties(got, model, what, with_vel=True, with_phi=True):
    c = got
    from topsy_amd import _native
    col_of, p = _native.HALO_COLUMNS, got["props"]
    assert got["n_members"] == model["n_members"] and got["max_extent"] == model["max_extent"], what
    assert np.array_equal(c["count"], model["count"]), f"{what}: counts"
    n_h = model["count"].astype(np.float64)
    tol = SUM_BOUND * (n_h + 16.0)
    full = model["count"] > 0

    def column(name, width=1):
        a = p[:, col_of[name]:col_of[name] + width]
        return a[:, 0] if width == 1 else a

    def same_nan(a, b, name):
        assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: {name}: NaN pattern"

    def within(name, width, scale_name, wrap=False):
        a, b = column(name, width), model[name]
        same_nan(a, b, name)
        diff = np.abs(a - b)
        if wrap:
            diff = np.minimum(diff, np.abs(diff - 1.0))
        bound = tol * model[scale_name]
        bound = bound if width == 1 else bound[:, None]
        ok = ~np.isnan(b)
        worst = np.nanmax(np.where(ok, diff / np.where(bound > 0, bound, np.inf), 0.0)) if ok.any() else 0.0
        print(f"{what}: {name}: worst error / bound = {worst:.3g}")
        assert (diff[ok] <= np.broadcast_to(bound, diff.shape)[ok]).all(), f"{what}: {name} outside the summation-order bound"

    print()
    assert np.array_equal(column("mass")[~full], model["mass"][~full])
    mass_err = np.abs(column("mass") - model["mass"])
    assert (mass_err <= tol * model["mass"]).all(), f"{what}: mass"
    within("com", 3, "scale_com", wrap=True)
    within("S", 6, "scale_S")
    for name in ("r_max", "r_half", "r_vmax"):
        a, b = column(name), model[name]
        same_nan(a, b, name)
        ok = ~np.isnan(b)
        worst = ulps(a[ok], b[ok]).max() if ok.any() else 0.0
        print(f"{what}: {name}: worst difference {worst:.2f} ulp")
        assert worst <= 4.0, f"{what}: {name}"
    for name in ("i_half", "i_vmax"):
        a = column(name)
        assert np.array_equal(np.where(np.isnan(a), -1, a).astype(np.int64), model[name]), f"{what}: the member chosen for {name}"
    a, b = column("v2_max"), model["v2_max"]
    same_nan(a, b, "v2_max")
    ok = ~np.isnan(b)
    assert (np.abs(a[ok] - b[ok]) <= tol[ok] * b[ok]).all(), f"{what}: v2_max"
    if with_vel:
        within("v_com", 3, "scale_v_com")          # (sum m v / M: within the bound times max |v|)
        within("L", 3, "scale_L")
        within("e_kin", 1, "scale_e_kin")
        a, b = column("sigma2"), model["sigma2"]
        same_nan(a, b, "sigma2")
        assert np.allclose(a[full], b[full], rtol=1e-12, atol=0)
    else:
        for name, width in (("v_com", 3), ("L", 3), ("e_kin", 1), ("sigma2", 1)):
            assert np.isnan(column(name, width)).all(), f"{what}: {name} without velocities"
    if with_phi:
        assert np.array_equal(c["i_pot"], model["i_pot"]) and np.array_equal(c["n_bound"], model["n_bound"]), f"{what}: i_pot, n_bound"
        within("e_pot", 1, "scale_e_pot")
        a, b = column("m_bound"), model["m_bound"]
        same_nan(a, b, "m_bound")
        ok = ~np.isnan(b)
        assert (np.abs(a[ok] - b[ok]) <= tol[ok] * model["mass"][ok]).all(), f"{what}: m_bound"
        a, b = column("pot_pos", 3), model["pot_pos"]
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(b)], b[~np.isnan(b)]), f"{what}: pot_pos"
    else:
        assert (c["i_pot"] == -1).all() and (c["n_bound"] == -1).all()
        for name, width in (("e_pot", 1), ("m_bound", 1), ("pot_pos", 3)):
            assert np.isnan(column(name, width)).all(), f"{what}: {name} without a potential"


def same_bits(a, b):
    return all(np.array_equal(np.asarray(a[k]).view(np.uint64) if np.asarray(a[k]).dtype == np.float64 else a[k],
                              np.asarray(b[k]).view(np.uint64) if np.asarray(b[k]).dtype == np.float64 else b[k]) for k in a)


def report_bit_equality(got, model, what, with_vel=True, with_phi=True):
    """prints, per column, whether the library's values are the model's bits (a record: the assertions are check_properties')"""
    from topsy_amd import _native
    names = [("mass", 1), ("com", 3), ("S", 6), ("r_max", 1), ("r_half", 1), ("v2_max", 1), ("r_vmax", 1)]
    names += [("v_com", 3), ("L", 3), ("e_kin", 1), ("sigma2", 1)] if with_vel else []
    names += [("e_pot", 1), ("m_bound", 1)] if with_phi else []
    differ = {}
    for name, width in names:
        c = _native.HALO_COLUMNS[name]
        a, b = got["props"][:, c:c + width].reshape(model[name].shape), model[name]
        rows = ~((a == b) | (np.isnan(a) & np.isnan(b))).reshape(len(a), -1).all(axis=1)
        differ[name] = np.flatnonzero(rows) + 1
    print(f"{what}: bit-equal to the model: {', '.join(k for k, v in differ.items() if not len(v)) or 'no column'}")
    for k, v in differ.items():
        if len(v):
            print(f"{what}: {k} differs from the model's bits in the haloes {list(v[:8])} ({len(v)} of {len(model['count'])})")
    return differ


@pytest.mark.parametrize("name", ["clumps", "periodic", "crumbs", "nonfinite", "edges", "edges+1", "giants"])
def test_properties(ctx, name):
    """the contract of tsp_halo_properties: phi is an input, so the model is given the phi the call is given (the GPU's)"""
    scene = ref.reference(name)[0]
    phi = gpu_potential(ctx, scene)[0]
    got = gpu_properties(ctx, scene, phi)
    model = ref.properties_model(scene, phi=phi)
    check_properties(got, model, name)
    report_bit_equality(got, model, name)
    assert same_bits(got, gpu_properties(ctx, scene, phi)), "a second call gives other bits"
    if name in ("edges", "edges+1"):
        from topsy_amd import _native
        ten, nine, v2 = ref.EDGE_SIZES.index(10), ref.EDGE_SIZES.index(9), _native.HALO_COLUMNS["v2_max"]
        assert got["props"][ten, v2] > 0 and np.isnan(got["props"][nine, v2]), "v2_max needs ten members"
    if name == "crumbs":
        assert (got["count"][-5:] == 0).all() and np.isnan(got["props"][-5:, 1:]).all() and (got["props"][-5:, 0] == 0).all()
    if name == "nonfinite":
        assert (got["n_bound"] == -1).sum() == 1 and (got["i_pot"] == -1).sum() == 1       # the halo with a NaN phi member


def test_properties_without_velocities_or_potential(ctx):
    scene = ref.reference("clumps")[0]
    phi = ref.reference("clumps")[1]["phi"]
    check_properties(gpu_properties(ctx, scene, phi, with_vel=False), ref.properties_model(scene, phi=phi, with_vel=False),
                     "clumps, vel=None", with_vel=False)
    check_properties(gpu_properties(ctx, scene, None), ref.properties_model(scene, phi=None), "clumps, phi=None", with_phi=False)


@pytest.mark.parametrize("without", ["vel", "phi"])
def test_giants_properties_without_velocities_or_potential(ctx, without):
    scene = ref.reference("giants")[0]
    if without == "vel":
        phi = gpu_potential(ctx, scene)[0]
        got, model = gpu_properties(ctx, scene, phi, with_vel=False), ref.properties_model(scene, phi=phi, with_vel=False)
    else:
        got, model = gpu_properties(ctx, scene, None), ref.reference("giants")[2]
    check_properties(got, model, f"giants, {without}=None", with_vel=without != "vel", with_phi=without != "phi")
    report_bit_equality(got, model, f"giants, {without}=None", with_vel=without != "vel", with_phi=without != "phi")


def test_sparse_labels(ctx):
    """edges with its 16 labels spread over 1 .. 2^18: the sorted layout, and so every association, is the same -- the rows of
    the labels that have members carry the bits of the dense catalogue's rows, the 262128 others are empty"""
    scene = ref.reference("edges")[0]
    sparse, new = ref.sparse_labels(scene)
    H = sparse["n_groups"]
    assert H == 2 ** 18 and new[0] == 1 and new[-1] == H and len(new) == len(ref.EDGE_SIZES)
    phi, info = gpu_potential(ctx, scene)
    phi_sparse, info_sparse = gpu_potential(ctx, sparse)
    assert np.array_equal(phi.view(np.uint64), phi_sparse.view(np.uint64)) and info == info_sparse
    dense, got = gpu_properties(ctx, scene, phi), gpu_properties(ctx, sparse, phi)
    assert got["n_members"] == dense["n_members"] and got["max_extent"] == dense["max_extent"]
    full = np.zeros(H, dtype=bool)
    full[new - 1] = True
    assert np.array_equal(got["count"][full], ref.EDGE_SIZES) and np.array_equal(got["count"][full], dense["count"])
    assert same_bits({k: got[k][full] for k in ("count", "n_bound", "i_pot", "props")}, {k: dense[k] for k in ("count", "n_bound", "i_pot", "props")})
    assert (got["count"][~full] == 0).all() and (got["n_bound"][~full] == -1).all() and (got["i_pot"][~full] == -1).all()
    assert (got["props"][~full, 0] == 0).all() and np.isnan(got["props"][~full, 1:]).all()
    assert same_bits(got, gpu_properties(ctx, sparse, phi)), "a second call gives other bits"


@pytest.mark.parametrize("name", ["clumps", "periodic"])
def test_pipeline_against_the_models_own_potential(native, name):
    """topsy_amd.halo_properties(eps=...) forms phi in float32 pair terms; the model's own float64 phi decides what it can"""
    import topsy_amd
    scene, pot, model = ref.reference(name)
    h = topsy_amd.halo_properties(scene["pos"], scene["mass"], scene["labels"], vel=scene["vel"], eps=scene["eps"],
                                  periodicity_scale=scene["period"] or None)
    assert np.array_equal(h.n, model["count"])
    clear = ~model["pot_ambiguous"]
    assert np.array_equal(h.i_pot[clear], model["i_pot"][clear])
    lo, hi = model["n_bound_sure"], model["n_bound_sure"] + model["n_bound_ambiguous"]
    print(f"\n{name}: n_bound {h.n_bound}, sure {lo}, ambiguous {model['n_bound_ambiguous']}")
    assert ((h.n_bound >= lo) & (h.n_bound <= hi)).all()
    slack = 1e-12 * model["mass"]
    assert ((h.m_bound >= model["m_bound_sure"] - slack) & (h.m_bound <= model["m_bound_sure"] + model["m_bound_ambiguous"] + slack)).all()
    e_bound = 0.5 * np.array([(scene["mass"][scene["labels"] == g + 1].astype(np.float64) * ref.K * ref.U *
                               pot["scale"][scene["labels"] == g + 1]).sum() for g in range(scene["n_groups"])])
    assert (np.abs(h.e_pot - model["e_pot"]) <= e_bound + SUM_BOUND * (model["count"] + 16) * model["scale_e_pot"]).all()
    assert np.allclose(h.virial_ratio[:12], 2 * model["e_kin"][:12] / np.abs(model["e_pot"][:12]), rtol=1e-4)
    assert np.array_equal(np.isnan(h.phi), np.isnan(pot["phi"]))


# ---- refused calls, failed allocations, the context ------------------------------------------------------------------------------
def raw_calls(native, ctx, scene, phi):
    """(outputs, call) of both entry points as raw ctypes calls"""
    lib = native.load_library()
    n, H = len(scene["pos"]), scene["n_groups"]
    x, y, z = xyz(scene)
    vx, vy, vz = col(scene["vel"])
    m, eps, lab = scene["mass"], np.ascontiguousarray(scene["eps"], dtype=f32), scene["labels"]
    out_p = Outputs(phi=np.empty(n, dtype=np.float64), info=native.GroupPotentialInfo())
    out_h = Outputs(count=np.empty(H, dtype=np.int64), n_bound=np.empty(H, dtype=np.int64), i_pot=np.empty(H, dtype=np.int64),
                    props=np.empty((H, native.HALO_NPROPS), dtype=np.float64), info=native.HaloInfo())

    def potential(n=n, x=x, lab=lab, n_groups=H, period=scene["period"], max_members=0):
        return lib.tsp_group_potential(ctx._h, n, P(x), P(y), P(z), P(m), P(eps), 0.0, P(lab, _i32p), n_groups, period, max_members,
                                       P(out_p.phi, _dp), ctypes.byref(out_p.info))

    def properties(n=n, x=x, lab=lab, n_groups=H, period=scene["period"], vy=vy):
        return lib.tsp_halo_properties(ctx._h, n, P(x), P(y), P(z), P(m), P(vx), P(vy), P(vz), P(phi, _dp), P(lab, _i32p), n_groups, period,
                                       P(out_h.count, _i64p), P(out_h.n_bound, _i64p), P(out_h.i_pot, _i64p), P(out_h.props, _dp),
                                       ctypes.byref(out_h.info))

    return out_p, potential, out_h, properties


def test_refused_calls_write_nothing(native, ctx):
    scene, pot, _ = ref.reference("clumps")
    out_p, potential, out_h, properties = raw_calls(native, ctx, scene, pot["phi"])
    too_high = scene["labels"].copy()
    too_high[17] = scene["n_groups"] + 1
    refusals = [dict(lab=too_high), dict(n=0), dict(x=None), dict(period=-1.0), dict(period=float("nan")), dict(period=float("inf")),
                dict(n_groups=0), dict(lab=None)]
    for kw in refusals:
        for outs, call in ((out_p, potential), (out_h, properties)):
            outs.fill()
            assert call(**kw) == EINVAL, kw
            assert not outs.written(), (kw, outs.written())
    out_p.fill()
    assert potential(max_members=-1) == EINVAL and not out_p.written()
    out_h.fill()
    assert properties(vy=None) == EINVAL and not out_h.written()          # two of three velocities


def test_injected_allocation_failures(native, frame_ctx):
    scene, pot, _ = ref.reference("clumps")
    out_p, potential, out_h, properties = raw_calls(native, frame_ctx, scene, pot["phi"])
    walk(native, frame_ctx, potential, out_p, {"sph_sum_h", "sph_sum_a"})
    info = {k: (float if k == "max_extent" else int)(getattr(out_p.info, k)) for k, _ in out_p.info._fields_}
    check_potential((out_p.phi, info), pot, "after the injected failures")
    walk(native, frame_ctx, properties, out_h, {"sph_sum_h", "sph_sum_a"})
    got = dict(count=out_h.count, n_bound=out_h.n_bound, i_pot=out_h.i_pot, props=out_h.props, n_members=int(out_h.info.n_members),
               max_extent=float(out_h.info.max_extent))
    check_properties(got, ref.properties_model(scene, phi=pot["phi"]), "after the injected failures")


def test_context_unchanged(native, frame_ctx):
    scene, pot, _ = ref.reference("crumbs")
    before = snapshot(frame_ctx)
    gpu_potential(frame_ctx, scene)
    gpu_properties(frame_ctx, scene, pot["phi"])
    assert_same_state(before, snapshot(frame_ctx), "after tsp_group_potential and tsp_halo_properties")


# ---- the Python surface ----------------------------------------------------------------------------------------------------------
def test_python_surface(native):
    import topsy_amd
    from types import SimpleNamespace
    from topsy_amd import kinematics, surface
    scene, pot, model = ref.reference("periodic")
    n = len(scene["pos"])
    h = np.full(n, 0.01, dtype=f32)
    want = topsy_amd.halo_properties(scene["pos"], scene["mass"], scene["labels"], vel=scene["vel"], eps=scene["eps"], periodicity_scale=1.0)
    vis = topsy_amd.from_arrays(scene["pos"], h, scene["mass"], halos=scene["labels"], vel=scene["vel"], eps=scene["eps"],
                                periodicity_scale=1.0, render_resolution=64)
    try:
        got = vis.halo_properties()
        assert got is vis.halo_properties() and got is vis.data_loader.get_halo_properties()          # cached
        assert same_bits(got.raw | {"phi": got.phi}, want.raw | {"phi": want.phi})
        default = vis.centre_on_halo(2).copy()
        assert np.array_equal(default, -vis.data_loader.get_halo_center(2)) and np.array_equal(vis.centre_on_halo(2, at="shrink"), default)
        assert np.array_equal(vis.centre_on_halo(2, at="pot"), -got.pot_pos[1]) and np.array_equal(vis.position_offset, -got.pot_pos[1])
        assert np.array_equal(vis.centre_on_halo(2, at="com"), -got.com[1])
        # the three centres of halo 2 lie within its scale radius (0.0101) of the clump's centre: within 0.02 of each other
        assert np.linalg.norm(got.com[1] - (-default)) < 0.02 and np.linalg.norm(got.pot_pos[1] - (-default)) < 0.02
        assert np.array_equal(surface.SurfaceView.centre_on_halo(SimpleNamespace(_vis=vis), 3, at="com"), -got.com[2])
        assert np.array_equal(kinematics.VelocityFrames.centre_on_halo(SimpleNamespace(_vis=vis), 3, at="pot"), -got.pot_pos[2])
        for bad in (dict(n=2, at="middle"), dict(n=99, at="com"), dict(n=0, at="pot")):
            with pytest.raises(ValueError):
                vis.centre_on_halo(**bad)
        vis.data_loader.set_halos(scene["labels"])
        assert vis.halo_properties() is not got                                                       # set_halos drops the cache
    finally:
        vis.close()
    # one script line from positions to the whole catalogue's properties
    cat = topsy_amd.friends_of_friends(scene["pos"], linking_length=0.004, periodicity_scale=1.0)
    props = topsy_amd.halo_properties(scene["pos"], scene["mass"], cat, vel=scene["vel"], eps=scene["eps"], periodicity_scale=1.0)
    assert len(props) == len(cat) >= 5 and np.array_equal(props.n, cat.sizes) and (props.mass > 0).all()
