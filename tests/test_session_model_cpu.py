"""The host model of the context (tests/session_model.py) and its scene, without a GPU: every session the native matrix runs is
well formed, and no frame of the scene can pass for another one of the same layout -- the condition that makes a stale image, a
stale weight array or a wrongly restored tag fail in tests/test_gpu_session_matrix.py."""
import itertools

import numpy as np
import pytest

import session_model as sm
from session_model import EINVAL, ESTATE, Session

R = sm.R


@pytest.fixture(scope="module")
def scene():
    return sm.first_scene()


def new_session(scene, second=None):
    s = Session(4)
    assert s.op("upload_particles", scene=scene) is None
    assert s.op("upload_quantity", q=(second or scene)["q"]) is None
    assert s.op("upload_rgb", rgb=(second or scene)["rgb"]) is None
    assert s.op("upload_velocities", vel=(second or scene)["vel"]) is None
    return s


def produce(s, kind, **args):
    if kind == "surface":
        return s.op("render_surface", **args)
    if kind in sm.LINES_OF_SIGHT:
        s.op("set_line_of_sight", los=sm.LINES_OF_SIGHT[kind])
    s.op("set_use_quantity", on=kind != "density")
    return s.op("render", kind=kind, **args)


def frames(scene, mips):
    """{kind: (want, fragments, terms)} of the seven producers for `scene`"""
    out = {}
    for kind in sm.PRODUCERS:
        s = new_session(scene)
        assert produce(s, kind) is None and s.frame.complete
        out[kind] = sm.expected(s.frame, mips)
    return out


# --------------------------------------------------------------------------- the sessions are well formed
def test_every_pair_of_the_matrix_is_allowed_and_every_state_refuses_something(scene):
    assert len(sm.PAIRS) == 49 and len(set(sm.PAIRS)) == 49
    s = new_session(scene)
    allowed, refused = set(), set()
    for a, b in sm.PAIRS:
        for kind in (a, b):
            assert produce(s, kind) is None, (a, b, kind)
            assert s.frame.kind == kind and s.frame.complete and s.C == sm.CHANNELS[kind]
            assert s.keys == (kind == "surface")
            cons, ref = s.consumers(), s.refused_calls()
            assert cons and ref, (a, b, kind)
            both = {name for _, name, _, _ in ref} & set(cons)
            assert both <= {"content_sort"}, "a call is both allowed and refused"      # (content_sort: kinds 0, 1, 3 against kind 2)
            for label, name, args, code in ref:
                assert code in (ESTATE, EINVAL)
                before = (s.C, s.keys, s.source, s.frame)
                trial_args = dict(args)
                if name == "render" and args["kind"] in sm.LINES_OF_SIGHT:
                    s.op("set_line_of_sight", los=sm.LINES_OF_SIGHT[args["kind"]])
                assert s.op(name, **trial_args) == code, label
                assert (s.C, s.keys, s.source, s.frame) == before, "a refused call changed the image's tags"
                refused.add((kind, label, code))
            allowed.update((kind, c) for c in cons)
    assert s.transitions > 98 and s.refusals > 98
    # each refusal the matrix must assert, in at least one state
    labels = {(k, l) for k, l, _ in refused}
    assert ("density", "render(rgb, clear=0)") in labels and ("rgb", "render(weighted, clear=0)") in labels      # another channel count
    assert ("rgb", "render(kinematic_a, clear=0)") in labels and ("kinematic_a", "render(rgb, clear=0)") in labels
    assert ("kinematic_a", "render(kinematic_b, clear=0)") in labels and ("kinematic_a", "render(kinematic_a, clear=0)") not in labels
    assert all(("surface", f"render({k}, clear=0)") in labels for k in sm.SPLATS)
    assert all((k, "render_surface(clear=0)") in labels for k in sm.SPLATS) and ("surface", "render_surface(clear=0)") not in labels
    assert ("surface", "tile_periodic") in labels and not any(l == "tile_periodic" for k, l in labels if k != "surface")
    for name in ("velocity_moments", "colormap_moment", "moment_sort"):
        assert all((k, name) in labels for k in sm.PRODUCERS if k not in sm.LINES_OF_SIGHT)
        assert not any((k, name) in labels for k in sm.LINES_OF_SIGHT)
    assert all(((k, "content_sort") in labels) == (sm.CHANNELS[k] == 2) for k in sm.PRODUCERS)
    assert all(((k, "surface_present") in labels) == (sm.CHANNELS[k] == 4) for k in sm.PRODUCERS)
    assert ("surface", "render_undo") in labels


def test_render_undo_is_valid_only_after_a_render(scene):
    s = new_session(scene)
    assert s.op("render_undo") == ESTATE
    for a, b in itertools.permutations(("weighted", "kinematic_a", "rgb"), 2):
        produce(s, a)
        fa, ca, src = s.frame, s.C, s.source
        produce(s, b)
        assert s.op("render_undo") is None and s.op("render_undo") == ESTATE
        assert (s.frame.kind, s.C, s.source) == (fa.kind, ca, src)
        assert (s.refusal("velocity_moments") is None) == (a == "kinematic_a")
    for call, args in (("write_image", {"channels": 4}), ("tile_periodic", {}), ("render_surface", {}), ("reorder_spatial", {}),
                       ("upload_quantity", {"q": scene["q"]}), ("upload_rgb", {"rgb": scene["rgb"]}),
                       ("upload_velocities", {"vel": scene["vel"]}), ("set_reduced_image", {})):
        produce(s, "weighted")
        assert s.op(call, **args) is None and s.op("render_undo") == ESTATE, call
    produce(s, "surface")
    produce(s, "weighted")                                     # replaced a surface image
    assert s.op("render_undo") == ESTATE
    # a refused render leaves "a render that failed" to undo, once; not over surface keys
    assert s.op("render", kind="rgb", clear=False) == ESTATE and s.op("render_undo") is None and s.op("render_undo") == ESTATE
    produce(s, "surface")
    assert s.op("render", kind="weighted", clear=False) == ESTATE and s.op("render_undo") == ESTATE


def test_inputs_that_are_gone_refuse_their_kinds(scene):
    s = Session(4)
    s.op("upload_particles", scene=scene)
    assert produce(s, "rgb") == ESTATE and produce(s, "kinematic_a") == ESTATE and produce(s, "density") is None
    s.op("upload_velocities", vel=scene["vel"])
    assert produce(s, "kinematic_a") is None
    s.op("upload_velocities", vel=None)
    assert produce(s, "kinematic_a") == ESTATE and s.refusal("velocity_moments") is None      # the image is still kinematic
    produce(s, "surface")
    s.op("reorder_spatial")
    assert s.op("render_surface", clear=False) == ESTATE
    two = Session(2)
    two.op("upload_particles", scene=scene)
    two.op("upload_rgb", rgb=scene["rgb"])
    assert produce(two, "rgb") == EINVAL and produce(two, "kinematic_a") == EINVAL
    assert Session(4).op("upload_quantity", q=scene["q"]) == ESTATE


# --------------------------------------------------------------------------- a stale frame cannot pass
def assert_distinct(stale, kind, want, terms, label):
    n = sm.stale_pixels(stale, kind, want, terms)
    print(f"{label}: pixels beyond 100 x the tolerance, per channel: {n.tolist()}")
    assert n.max() >= 1000, (label, n.tolist())


def test_no_frame_passes_for_another_kind_of_its_layout(scene, mips):
    fr = frames(scene, mips)
    assert (fr["surface"][0][..., 1] != 0).sum() > 1000, "the surface pass draws too little of the image"
    for group in ([k for k in sm.PRODUCERS if sm.CHANNELS[k] == 2], [k for k in sm.PRODUCERS if sm.CHANNELS[k] == 4]):
        for stale, kind in itertools.permutations(group, 2):
            want, _, terms = fr[kind]
            assert_distinct(fr[stale][0], kind, want, terms, f"{stale} shown as {kind}")


def test_the_second_attributes_cannot_pass_for_the_first(scene, mips):
    second = sm.second_attributes(len(scene["h"]))
    first = frames(scene, mips)
    other = frames(dict(scene, **second), mips)
    depends = {"weighted": "q", "surface": "q", "rgb": "rgb", "kinematic_a": "vel", "kinematic_b": "vel"}
    for kind in sm.PRODUCERS:
        if kind in depends:
            for a, b, label in ((first, other, "first shown as second"), (other, first, "second shown as first")):
                assert_distinct(a[kind][0], kind, b[kind][0], b[kind][2], f"{kind}: {label}")
        else:
            assert np.array_equal(first[kind][0], other[kind][0]), kind       # density and depth do not read them


def test_fresh_scenes_cross_the_tail_and_the_one_block_launch(mips):
    for n in (1001, 3):
        sc = sm.fresh_scene(n)
        assert len(sc["h"]) == n and n % 4 != 0
        fr = frames(sc, mips)
        assert fr["kinematic_a"][1] > 0 and (fr["kinematic_a"][0][..., 3] > 0).any(), n
