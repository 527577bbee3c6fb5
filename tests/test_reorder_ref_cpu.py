"""The model of the load-time ordering (tests/reorder_ref.py) checked on its own, without a GPU: the permutation is a bijection,
every (stratum, cell) run holds exactly the particles of its cell, and view culling through StratifiedCells loses no particle
that is finite on all axes and strictly inside the view sphere -- exactly, on every scene of tests/test_gpu_reorder.py.

The scene with sentinel rows at +-3e38 loses particles under the arithmetic the library had before (rule="parent": the float32
extent overflows, inv = 0, cell_width = 0, every cell centre = box_lo), and so does the scene a few denormals wide (inv = +inf,
cell_width = 0 although the particles differ): test_parent_rule_loses_particles shows both once.

nan_axis has no particle that is finite on all axes: no sphere can contain one, so that scene is held to the loss check (which
it passes with nothing to lose) and to the bijection and run checks, and is excepted from "at least 100 spheres contain a
particle"."""
import numpy as np
import pytest

import reorder_ref as ref

f32 = np.float32
from topsy_amd.cell_layout import StratifiedCells

N_STRATA = {"uniform": 1, "overflow": 1, "nonfinite": 3}      # the others: 3 strata at 5000 particles (k = 2)


def _scene(name, rule="fixed"):
    n = ref.SCENE_N[name]
    pos = ref.SCENES[name](n, 5)
    m = ref.reorder(pos, None, N_STRATA.get(name, 3), 99, interleave=0, rule=rule)
    return pos, m


def _sweep(pos, m):
    cells = StratifiedCells([m["layout"]])
    pos_new = pos[m["perm"]].astype(np.float64)
    lost = holding = culled = 0
    for centre, radius in ref.spheres(pos, 17):
        miss, ins, _ = ref.lost_particles(cells, pos_new, centre, radius)
        lost += len(miss)
        holding += bool(ins.any())
        culled += not cells.all_selected()
    return lost, holding, culled


@pytest.mark.parametrize("name", sorted(ref.SCENES))
def test_model_bijection_runs_and_no_loss(name):
    pos, m = _scene(name)
    n = len(pos)
    assert np.array_equal(np.sort(m["perm"]), np.arange(n))
    lay = m["layout"]
    k = lay["cells_per_axis"].bit_length() - 1
    ncell = lay["cells_per_axis"] ** 3
    assert k == ref.grid_bits(n, lay["n_strata"]) and (k == 4) == (n >= 65536 and lay["n_strata"] == 1)
    # runs: entry e = (stratum, cell) holds exactly the particles with that stratum and that model cell code
    code = ref.cell_codes(pos, k)
    stratum = ref.strata(n, lay["n_strata"], 99).astype(np.int64)
    entry_of = stratum * ncell + code
    off = lay["offsets"]
    assert off[0] == 0 and off[-1] == n and (np.diff(off) >= 0).all()
    assert np.array_equal(np.searchsorted(off, np.arange(n), side="right") - 1, entry_of[m["perm"]])
    assert np.array_equal(m["strata_offsets"], off[::ncell])
    fault = ref.cell_run_fault(lay, pos[m["perm"]])
    assert fault is None, fault
    if name not in ("point", "denormal"):       # (their particles sit at box_lo to within 1e-10 of a cell: any width holds them)
        assert ref.cell_run_fault(dict(lay, cell_width=lay["cell_width"] * f32(0.5)), pos[m["perm"]]) is not None, "a halved cell_width passes"
    lost, holding, culled = _sweep(pos, m)
    assert lost == 0
    if name == "nan_axis":
        assert holding == 0
    else:
        assert holding >= 100
    occupied = len(np.unique(code))
    if ncell > 1 and occupied > 1:
        assert culled >= 1, "no sphere culled anything"
    print(f"{name}: n={n} k={k} occupied cells={occupied} spheres holding a particle={holding} culling={culled}")


def test_parent_rule_loses_particles():
    """the arithmetic before the fix, shown once: the +-3e38 scene (and the denormal-wide one) lose in-sphere particles; every
    other scene loses none under either rule"""
    losses = {}
    for name in sorted(ref.SCENES):
        pos, m = _scene(name, rule="parent")
        losses[name] = _sweep(pos, m)[0]
    print("particles lost under the parent's rule:", losses)
    assert losses["overflow"] > 0 and losses["denormal"] > 0
    assert all(v == 0 for k, v in losses.items() if k not in ("overflow", "denormal"))
    lay = _scene("overflow", rule="parent")[1]["layout"]
    assert lay["cell_width"][0] == 0 and _scene("overflow")[1]["layout"]["cell_width"][0] > 0


def test_no_loss_on_a_hand_made_layout():
    """the property does not need the model to have produced the layout: 2^3 cells of width 1 over [0, 2)^3, two strata"""
    rs = np.random.RandomState(3)
    pts = rs.uniform(0.0, 2.0, size=(400, 3))
    code = (pts[:, 0] >= 1).astype(int) | ((pts[:, 1] >= 1).astype(int) << 1) | ((pts[:, 2] >= 1).astype(int) << 2)
    stratum = rs.randint(0, 2, 400)
    order = np.argsort(stratum * 8 + code, kind="stable")
    off = np.searchsorted((stratum * 8 + code)[order], np.arange(17), side="left")
    lay = {"n_strata": 2, "cells_per_axis": 2, "box_lo": np.zeros(3), "cell_width": np.ones(3), "offsets": off}
    cells = StratifiedCells([lay])
    pos_new = pts[order]
    culled = 0
    for centre, radius in ref.spheres(pts, 4, n_centres=10):
        miss, ins, cov = ref.lost_particles(cells, pos_new, centre, radius)
        assert len(miss) == 0
        culled += not cells.all_selected()
    assert culled > 0
    # ... and a wrong layout (the runs of cell 0 and cell 7 swapped in the offsets' geometry) is caught
    bad = dict(lay, box_lo=np.array([2.0, 2.0, 2.0]), cell_width=-np.ones(3))
    cells = StratifiedCells([bad])
    assert any(len(ref.lost_particles(cells, pos_new, c, r)[0]) for c, r in ref.spheres(pts, 4, n_centres=10))


def test_cells_that_cannot_be_placed_are_kept():
    lay = {"n_strata": 1, "cells_per_axis": 1, "box_lo": np.array([-3e38, 0.0, 0.0]), "cell_width": np.array([np.inf, 1.0, 1.0]),
           "offsets": np.array([0, 10])}
    cells = StratifiedCells([lay])
    cells.select_sphere([0.0, 0.0, 0.0], 1e-3)
    assert cells.all_selected()
    lay = dict(lay, box_lo=np.array([0.0, np.nan, 0.0]), cell_width=np.array([1.0, 0.0, 1.0]))
    cells = StratifiedCells([lay])
    cells.select_sphere([100.0, 0.0, 0.0], 1e-3)
    assert cells.all_selected()


def test_in_block_arrangement_one_is_a_bijection_inside_segments():
    pos = ref.scene_uniform(4097, 1)
    m0 = ref.reorder(pos, None, 3, 7, interleave=0)
    m1 = ref.reorder(pos, None, 3, 7, interleave=1)
    assert np.array_equal(np.sort(m1["perm"]), np.arange(4097)) and not np.array_equal(m1["perm"], m0["perm"])
    for a, e in m1["segments"]:
        assert np.array_equal(np.sort(m1["perm"][a:e]), np.sort(m0["perm"][a:e]))
        L = e - a
        if L >= 16:
            assert m1["perm"][a + 1 * (L // 8) + min(1, L % 8)] == m0["perm"][a + 1]      # rank 1 opens row 1
        else:
            assert np.array_equal(m1["perm"][a:e], m0["perm"][a:e])
