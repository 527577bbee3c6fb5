"""A host model of one tsp_context as a state machine (test infrastructure; plain Python, no GPU).

The library's render paths share one context: the float64 accumulator holds sums or the occlusion keys of the surface pass, the
image is laid out for 2 or 4 active channels, the weight arrays hold rgb or kinematic weights, and a handful of tags decide what a
call may do (DESIGN.md "Context state machine" is this module as a table; include/topsy_splat.h is the contract it restates).
`Session` carries those tags and what is resident, in the caller's order, and answers for every step of a session

  - which frame the image must be: `Session.frame`, turned into the oracle's image by `expected`;
  - which calls must be refused in that state, each with its error code: `Session.refused_calls`;
  - which consumers of the image are valid: `Session.consumers`.

The references are the existing ones, unchanged: parity_scenes.oracle_images for density, weighted, depth and rgb frames,
kinematic_compare.oracle_kinematic for kinematic frames, surface_ref.occlusion (bit for bit) for the surface pass.  A tiled
frame is oracle_np.periodic_tile of the float32 image read back before the tiling, bit for bit, and is formed by the test.

The scene is parity_scenes.all_class_scene(128) with the velocities of the kinematic tests, and a second set of attributes
(quantity, colours, velocities) chosen so that a frame drawn from the first set cannot pass for one of the second, nor any kind
of frame for another kind of the same layout (tests/test_session_model_cpu.py asserts both)."""
import copy

import numpy as np

import parity_scenes as ps
import surface_ref
from kinematic_compare import R, oracle_kinematic

f32 = np.float32
SCALE = 100.0
ESTATE, EINVAL = -4, -1          # TSP_ESTATE, TSP_EINVAL (include/topsy_splat.h)

PRODUCERS = ("density", "weighted", "depth", "rgb", "kinematic_a", "kinematic_b", "surface")
CHANNELS = {"density": 2, "weighted": 2, "depth": 2, "surface": 2, "rgb": 4, "kinematic_a": 4, "kinematic_b": 4}
SPLATS = PRODUCERS[:6]
PAIRS = [(a, b) for a in PRODUCERS for b in PRODUCERS]      # fixed order: the context reaches `a` from a different history each time
NONE, RGB, KINEMATIC = 0, 1, 2                                # the image's 4-channel source (tsp_context::image_source)

AXIS = np.array([0.0, 0.0, 1.0], dtype=f32)                   # the line of sight of the identity camera: its third row
V_BULK = np.array([50.0, -30.0, 20.0], dtype=f32)
LINES_OF_SIGHT = {"kinematic_a": (AXIS, V_BULK), "kinematic_b": (AXIS, np.zeros(3, dtype=f32))}      # one axis, two v_ref
SURFACE_PERCENTILE = 50.0


def camera():
    from oracle import oracle_np
    return oracle_np.transform_matrix(np.eye(3), np.zeros(3), SCALE)


def _freeze(sc):
    for a in sc.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return sc


def with_velocities(sc, seed=11):
    rs = np.random.RandomState(seed)
    sc["vel"] = (rs.normal(0.0, 100.0, size=sc["pos"].shape) + np.array([50.0, -30.0, 20.0])).astype(f32)
    return sc


def first_scene():
    """all_class_scene(128) with the velocities the kinematic tests add: every footprint class, partly off-screen"""
    return _freeze(with_velocities(ps.all_class_scene(R)))


def second_attributes(n, seed=101):
    """another quantity, other colours and other velocities for the n resident particles (uploaded mid-session)"""
    rs = np.random.RandomState(seed)
    return _freeze({"q": rs.normal(size=n).astype(f32), "rgb": rs.uniform(0.0, 1.0, size=(n, 3)).astype(f32),
                    "vel": (rs.normal(0.0, 100.0, size=(n, 3)) + np.array([-20.0, 40.0, -60.0])).astype(f32)})


def fresh_scene(n):
    """n other particles with all attributes: 1001 (not a multiple of 4: the tail of the kinematic weights), 3 (below 4, one
    block).  The first n rows of a larger all-class scene, pulled inside the view so that a tiny n still draws."""
    sc = with_velocities(ps.all_class_scene(R, n=max(n, 24), seed=3), seed=13)
    out = {k: (v[:n].copy() if isinstance(v, np.ndarray) else v) for k, v in sc.items()}
    out["pos"] = (out["pos"] * f32(0.5)).astype(f32)
    return _freeze(out)


def surface_cut(sc):
    return surface_ref.cut_for_percentile(surface_ref.density_cuts(sc["m"], sc["h"]), SURFACE_PERCENTILE)


class Frame:
    """What the image is: the kind of the render that started it, the attributes it was drawn from (a scene dict in the caller's
    order, the line of sight), how many of the particles its blocks hold, and what has been done to it since."""

    def __init__(self, kind=None, C=2, scene=None, los=None, use_q=True):
        self.kind, self.C, self.scene, self.los, self.use_q = kind, C, scene, los, use_q
        self.drawn = 0              # particles in its blocks (disjoint by the tests' construction)
        self.tiled = 0              # tile_periodic calls since the float32 image was last formed from the accumulator
        self.written = False        # write_image replaced it (the accumulator holds the written image)
        self.mixed = False          # a clear = 0 block went onto a written image: no reference

    @property
    def complete(self):
        return self.kind is not None and not self.written and not self.mixed and self.drawn == len(self.scene["h"])


_surface_cache = {}


def expected(frame, mips):
    """(want, fragment count or None, sum|terms| or None) of an untiled, complete frame from the existing references"""
    assert frame.complete and frame.tiled == 0
    M, sf = camera()
    sc = dict({"q": None, "rgb": None}, **frame.scene)        # (what was not resident is not read by the kinds that could draw)
    if frame.kind in ("density", "weighted", "depth", "rgb"):
        return ps.oracle_images(frame.kind, sc, M, sf, R, mips)
    if frame.kind in LINES_OF_SIGHT:
        axis, v_ref = frame.los
        return oracle_kinematic(sc, mips, M, sf, axis, v_ref)
    q = sc["q"] if frame.use_q and sc["q"] is not None else np.zeros_like(sc["m"])      # (q = 0 without an active quantity)
    key = ps._key(sc["pos"], sc["h"], sc["m"], q)
    if key not in _surface_cache:
        want, winner = surface_ref.occlusion(np.column_stack([sc["pos"], sc["h"]]).astype(f32), sc["m"], q, M, sf, R, surface_cut(sc),
                                             surface_ref.sphere_mips())
        want.setflags(write=False)
        _surface_cache[key] = (want, int((winner >= 0).sum()))
    return _surface_cache[key][0], None, None


def tolerance(kind, want, terms):
    """(R, R, C) float64: what the project's comparison of a frame of `kind` allows per value (0: bit for bit or exactly equal).
    parity_scenes.compare_with_oracle, kinematic_compare.check_kinematic."""
    w = np.abs(np.asarray(want, dtype=np.float64))
    tol = 1e-5 * w
    if kind == "density":
        tol[..., 1] = 0.0
    elif kind == "weighted":
        tol[..., 0] += 1e-30
        tol[..., 1] = 1e-5 * terms + 1e-30
    elif kind == "depth":
        tol[..., 1] += 1e-30
    elif kind == "rgb":
        tol[..., 3] = 0.0
    elif kind in LINES_OF_SIGHT:
        tol[..., 1] = 1e-5 * terms + 1e-30
        tol[..., 3] = 0.0
    else:
        tol[...] = 0.0
    return tol


def stale_pixels(stale, kind, want, terms, factor=100.0):
    """per channel, the pixels at which `stale` misses the frame `want` of `kind` by more than factor * its tolerance"""
    d = np.abs(np.asarray(stale, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    return (d > factor * tolerance(kind, want, terms)).reshape(-1, want.shape[-1]).sum(axis=0)


class Session:
    """The context: what is resident and the tags.  Every call is `op(name, **args)`: it returns the error code the library must
    answer with, or None after applying the call's effects.  A refused call has effects too (a refused tsp_render ends or
    re-arms tsp_render_undo), and they are applied."""

    def __init__(self, channels=4):
        self.Ccap = channels
        self.scene = None                    # resident arrays, caller's order: pos, h, m and, when uploaded, q, rgb, vel
        self.los = None
        self.use_quantity = True
        self.C = channels
        self.keys = False                    # surface_keys
        self.source = NONE                   # image_source
        self.image_los = None
        self.undo = 0                        # undo.kind: 0 none, 1 a render that drew, 2 a render that was refused or failed
        self.saved = None
        self.frame = Frame(C=channels)
        self.stats_id = 0                    # which render / surface call tsp_get_stats describes
        self._ids = 0
        self.transitions = 0                 # allowed calls applied
        self.refusals = 0                    # refused calls applied

    # ------------------------------------------------------------------ what is resident
    @property
    def n(self):
        return 0 if self.scene is None else len(self.scene["h"])

    def has(self, name):
        return self.scene is not None and self.scene.get(name) is not None

    def _same_los(self, a, b):
        return a is not None and b is not None and all(np.array_equal(x, y) for x, y in zip(a, b))

    # ------------------------------------------------------------------ the calls
    def refusal(self, name, **a):
        """the error code of `name` in this state, or None"""
        if name == "render":
            kind, clear = a["kind"], a.get("clear", True)
            if not clear and self.keys:
                return ESTATE
            if kind in LINES_OF_SIGHT:
                if self.Ccap != 4:
                    return EINVAL
                if self.n and not (self.has("m") and self.has("vel")) or self.los is None:
                    return ESTATE
            elif kind == "rgb":
                if self.Ccap != 4:
                    return EINVAL
                if self.n and not self.has("rgb"):
                    return ESTATE
            elif self.n and not self.has("m"):
                return ESTATE
            newC = CHANNELS[kind]
            if not clear and newC != self.C:
                return ESTATE
            if not clear and newC == 4 and self.source != NONE:
                if self.source != (KINEMATIC if kind in LINES_OF_SIGHT else RGB):
                    return ESTATE
                if kind in LINES_OF_SIGHT and not self._same_los(self.image_los, self.los):
                    return ESTATE
            return None
        if name == "render_surface":
            if self.n and not self.has("m"):
                return EINVAL
            return None if a.get("clear", True) or self.keys else ESTATE
        if name == "tile_periodic":
            return ESTATE if self.keys else None
        if name == "render_undo":
            return ESTATE if self.undo == 0 else None
        if name in ("velocity_moments", "colormap_moment", "moment_sort", "present_moment"):
            return None if self.source == KINEMATIC and self.C == 4 else ESTATE
        if name in ("colormap_rgb", "present_rgb"):
            return None if self.C == 4 else EINVAL
        if name == "content_sort":
            return EINVAL if a["kind"] == 2 and self.C != 4 else None
        if name in ("surface_present", "present_surface"):
            return None if self.C == 2 else EINVAL
        if name in ("upload_quantity", "upload_rgb", "upload_velocities", "upload_band_magnitudes", "reorder_spatial"):
            return None if self.n or (name == "upload_velocities" and a.get("vel") is None) else ESTATE
        return None

    def op(self, name, **a):
        code = self.refusal(name, **a)
        if code is not None:
            self.refusals += 1
            if name == "render":
                # tsp_render forgets the undo on entry; refused on surface keys it returns at once, otherwise it puts the context
                # back and leaves "a render that failed" to undo -- but never over surface keys
                self.undo = 0 if self.keys else 2
            return code
        self.transitions += 1
        getattr(self, "_" + name, lambda **k: None)(**a)
        return None

    def _stamp(self):
        self._ids += 1
        self.stats_id = self._ids

    def _render(self, kind, clear=True, block=None):
        if self.keys:
            self.undo = 0                    # a render that replaced a surface image cannot be taken back
        else:
            self.undo, self.saved = 1, (copy.copy(self.frame), self.C, self.source, self.image_los, self.stats_id)
        self.keys = False
        self.C = CHANNELS[kind]
        self.source = NONE if self.C == 2 else (KINEMATIC if kind in LINES_OF_SIGHT else RGB)
        if kind in LINES_OF_SIGHT:
            self.image_los = self.los
        if clear:
            self.frame = Frame(kind, self.C, self.scene, self.los if kind in LINES_OF_SIGHT else None, self.use_quantity)
        else:
            self.frame = copy.copy(self.frame)
            self.frame.mixed = self.frame.mixed or self.frame.written or self.frame.kind != kind
            self.frame.tiled = 0             # the float32 image is formed again from the untiled accumulator
        self.frame.drawn += self.n if block is None else block[1]
        self._stamp()

    def _render_surface(self, clear=True, block=None):
        self.undo = 0
        self.C, self.source, self.keys = 2, NONE, True
        if clear:
            self.frame = Frame("surface", 2, self.scene, None, self.use_quantity)
        else:
            self.frame = copy.copy(self.frame)
        self.frame.drawn += self.n if block is None else block[1]
        self._stamp()

    def _write_image(self, channels):
        self.undo = 0
        self.C, self.keys = channels, False                   # (the image's source tag stays: a written image keeps "kinematic")
        self.frame = copy.copy(self.frame)
        self.frame.C, self.frame.written, self.frame.tiled = channels, True, 0

    def _tile_periodic(self):
        self.undo = 0
        self.frame = copy.copy(self.frame)
        self.frame.tiled += 1

    def _render_undo(self):
        if self.undo == 1:
            self.frame, self.C, self.source, self.image_los, self.stats_id = self.saved
        self.frame = copy.copy(self.frame)
        self.frame.tiled = 0                 # either way the float32 image is formed again from the accumulator
        self.undo, self.saved = 0, None

    def _set_reduced_image(self):
        self.undo = 0

    def _set_line_of_sight(self, los):
        self.los = (np.asarray(los[0], dtype=f32), np.asarray(los[1], dtype=f32))

    def _set_use_quantity(self, on):
        self.use_quantity = bool(on)

    def _upload_particles(self, scene):
        """the particles and their mass; quantity, colours, velocities and the ordering go with the old ones, the image stays"""
        self.scene = {k: scene[k] for k in ("pos", "h", "m")}
        self.keys, self.undo = False, 0

    def _upload(self, name, value):
        if self.scene is not None:           # (freeing an attribute of no particles is accepted and changes nothing)
            self.scene = dict(self.scene)
            self.scene[name] = value
        self.undo = 0

    def _upload_quantity(self, q):
        self._upload("q", q)

    def _upload_rgb(self, rgb):
        self._upload("rgb", rgb)

    def _upload_band_magnitudes(self, rgb):
        self._upload("rgb", rgb)

    def _upload_velocities(self, vel):
        self._upload("vel", vel)

    def _reorder_spatial(self):
        self.keys, self.undo = False, 0

    # ------------------------------------------------------------------ what a state allows and refuses
    def consumers(self):
        """the consumers of the image that are valid now"""
        out = ["colormap_scalar", "colormap_bivariate", "content_sort", "present_scalar"]
        out += ["colormap_rgb", "present_rgb"] if self.C == 4 else ["surface_present", "present_surface"]
        if self.source == KINEMATIC and self.C == 4:
            out += ["velocity_moments", "colormap_moment", "moment_sort", "present_moment"]
        return out

    def refused_calls(self):
        """[(label, name, args, code)]: the calls that must be refused now.  Renders without clear of every kind and, for the
        kinematic kinds, along both lines of sight (LINES_OF_SIGHT[kind]: the driver sets it first); the consumers of another
        layout or source; tsp_render_undo, tsp_render_surface(clear = 0) and tsp_tile_periodic where the tags forbid them."""
        out = []
        if self.refusal("render_undo") is not None:
            out.append(("render_undo", "render_undo", {}, ESTATE))
        trial = copy.copy(self)
        for kind in SPLATS:
            args = {"kind": kind, "clear": False}
            if kind in LINES_OF_SIGHT:
                trial.los = LINES_OF_SIGHT[kind]
            code = trial.refusal("render", **args)
            if code is not None:
                out.append((f"render({kind}, clear=0)", "render", args, code))
        for name, args in (("render_surface", {"clear": False}), ("tile_periodic", {}), ("velocity_moments", {}), ("colormap_moment", {}),
                           ("moment_sort", {}), ("present_moment", {}), ("colormap_rgb", {}), ("present_rgb", {}),
                           ("content_sort", {"kind": 2}), ("surface_present", {}), ("present_surface", {})):
            code = self.refusal(name, **args)
            if code is not None:
                out.append((name + ("(clear=0)" if args.get("clear") is False else ""), name, args, code))
        return out
