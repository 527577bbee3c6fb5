"""Phase diagrams without a GPU: the float64 model (phase_ref.py) against numpy.histogram2d, the NumPy layer of topsy_amd/phase.py
and the host arithmetic of topsy_amd/csrc/tsp_hist2d_layout.h, driven through tsp_histogram_2d_layout (a host function: it needs no
device) and by tools/hist2d_layout_check.cpp under the address and undefined-behaviour sanitizers."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import phase_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def cloud(n=5000, seed=2):
    rs = np.random.RandomState(seed)
    x = np.exp(rs.normal(0.0, 1.5, n)).astype(f32)
    y = (np.exp(rs.normal(8.0, 1.0, n)) * x.astype(np.float64) ** 0.4).astype(f32)
    return x, y, rs.normal(1.0, 1.0, n).astype(f32), rs.normal(0.0, 30.0, n).astype(f32)


# ---- the model -----------------------------------------------------------------------------------------------------------------
def test_model_is_numpy_histogram2d_away_from_the_last_edge():
    from topsy_amd import phase
    x, y, w, v = cloud()
    ex = phase.hist_edges(float(x.min()) * 0.5, float(x.max()) * 2.0, 37, log=True)
    ey = phase.hist_edges(float(y.min()) * 0.5, float(y.max()) * 2.0, 23, log=True)
    m = ref.histogram(x, y, w, v, ex, ey)
    x64, y64, w64, v64 = (a.astype(np.float64) for a in (x, y, w, v))
    for plane, weights in ((None, None), (0, w64), (1, w64 * v64), (2, w64 * v64 * v64)):
        want = np.histogram2d(y64, x64, bins=(ey, ex), weights=weights)[0]         # (rows are y)
        got = m["count"] if plane is None else m["sums"][plane]
        assert got.shape == (23, 37)
        assert np.allclose(got, want, rtol=1e-12, atol=0) and (plane is not None or np.array_equal(got, want))
    assert m["n_valid"] == m["n_binned"] == len(x) == m["count"].sum() and (m["bin_index"] >= 0).all()


def test_model_edges_and_validity():
    ex, ey = np.array([1.0, 2.0, 4.0]), np.array([0.0, 1.0])
    x = np.array([1.0, 2.0, 4.0, np.nextafter(f32(4.0), f32(0.0)), 0.5, 3.0, 3.0, 3.0, np.nan], dtype=f32)
    y = np.array([0.5, 0.5, 0.5, 0.5, 0.5, 1.0, np.inf, 0.0, 0.5], dtype=f32)
    w = np.array([1, 1, 1, 1, 1, 1, 1, np.nan, 1], dtype=f32)
    m = ref.histogram(x, y, w, None, ex, ey)
    assert m["bin_index"].tolist() == [0, 1, -1, 1, -1, -1, -1, -1, -1]
    assert m["n_valid"] == 6 and m["n_binned"] == 3 and m["count"].tolist() == [[1, 2]]


# ---- hist_edges ----------------------------------------------------------------------------------------------------------------
def test_hist_edges():
    from topsy_amd import phase
    e = phase.hist_edges(0.1, 0.7, 7)
    assert e.dtype == np.float64 and len(e) == 8 and e[0] == 0.1 and e[-1] == 0.7 and (np.diff(e) > 0).all()
    assert np.allclose(np.diff(e), 0.6 / 7)
    g = phase.hist_edges(1e-3, 1e7, 1024, log=True)
    assert len(g) == 1025 and g[0] == 1e-3 and g[-1] == 1e7 and np.allclose(np.diff(np.log10(g)), 10.0 / 1024)
    assert phase.hist_edges(-5, -1, 1).tolist() == [-5.0, -1.0]
    for args in ((1.0, 1.0, 4), (2.0, 1.0, 4), (0.0, 1.0, 0), (0.0, 1.0, 1025), (0.0, 1.0, 2.5), (0.0, 1.0, True), (np.nan, 1.0, 4),
                 (0.0, np.inf, 4), ("a", 1.0, 4), (1.0, np.nextafter(1.0, 2.0), 4)):
        with pytest.raises(ValueError):
            phase.hist_edges(*args)
    for lo in (0.0, -1.0):
        with pytest.raises(ValueError):
            phase.hist_edges(lo, 1.0, 4, log=True)


# ---- PhaseDiagram --------------------------------------------------------------------------------------------------------------
def diagram(x, y, w, v, ex, ey, x_log=False, y_log=False, index=True):
    from topsy_amd import phase
    m = ref.histogram(x, y, w, v, ex, ey)
    return phase.PhaseDiagram(ex, ey, m["count"], m["sums"], {"n_valid": m["n_valid"], "n_binned": m["n_binned"]},
                              m["bin_index"] if index else None, x_log, y_log), m


def test_phase_diagram_moments_and_density():
    from topsy_amd import phase
    x, y, _, v = cloud(4000, seed=5)
    w = np.random.RandomState(1).uniform(0.5, 2.0, len(x)).astype(f32)
    ex, ey = phase.hist_edges(0.01, 100.0, 12, log=True), phase.hist_edges(10.0, 1e6, 9, log=True)
    d, m = diagram(x, y, w, v, ex, ey, True, True)
    assert d.shape == (9, 12) and d.count.dtype == np.int64 and np.array_equal(d.count, m["count"])
    assert np.array_equal(d.weight, m["sums"][0])
    empty = m["count"] == 0
    assert empty.any() and (~empty).sum() > 20
    assert np.isnan(d.mean[empty]).all() and np.isnan(d.dispersion[empty]).all() and (d.weight[empty] == 0).all()
    # against the particles of each cell, brute force
    x64, w64, v64 = x.astype(np.float64), w.astype(np.float64), v.astype(np.float64)
    for j, i in zip(*np.nonzero(~empty)):
        sel = m["bin_index"] == j * 12 + i
        mean = (w64[sel] * v64[sel]).sum() / w64[sel].sum()
        var = (w64[sel] * (v64[sel] - mean) ** 2).sum() / w64[sel].sum()
        assert d.mean[j, i] == pytest.approx(mean, rel=1e-10, abs=1e-10)
        assert d.dispersion[j, i] == pytest.approx(np.sqrt(var), rel=1e-6, abs=1e-6)
    area = np.diff(np.log10(ey))[:, None] * np.diff(np.log10(ex))[None, :]
    assert np.allclose(d.density, d.weight / area, rtol=1e-14)
    assert np.allclose(d.x_centres, np.sqrt(ex[:-1] * ex[1:])) and np.allclose(d.y_centres, np.sqrt(ey[:-1] * ey[1:]))
    lin, _ = diagram(x, y, w, None, ex, ey)
    assert lin.mean is None and lin.dispersion is None
    assert np.allclose(lin.density, lin.weight / (np.diff(ey)[:, None] * np.diff(ex)[None, :]), rtol=1e-14)
    assert np.allclose(lin.x_centres, 0.5 * (ex[:-1] + ex[1:]))


def test_phase_diagram_zero_weight_sum_is_nan_and_one_member_has_no_dispersion():
    ex, ey = np.array([0.0, 1.0, 2.0]), np.array([0.0, 1.0])
    x, y = np.array([0.5, 0.5, 1.5], dtype=f32), np.array([0.5, 0.5, 0.5], dtype=f32)
    d, _ = diagram(x, y, np.array([1.0, -1.0, 2.0], dtype=f32), np.array([3.0, 5.0, 7.0], dtype=f32), ex, ey)
    assert d.count.tolist() == [[2, 1]] and d.weight.tolist() == [[0.0, 2.0]]
    assert np.isnan(d.mean[0, 0]) and np.isnan(d.dispersion[0, 0]) and d.mean[0, 1] == 7.0 and d.dispersion[0, 1] == 0.0


def test_select_against_a_brute_force_mask():
    from topsy_amd import phase
    x, y, w, _ = cloud(3000, seed=9)
    x[::50] = np.nan
    ex, ey = phase.hist_edges(0.05, 20.0, 16, log=True), phase.hist_edges(100.0, 1e5, 10, log=True)
    d, m = diagram(x, y, w, None, ex, ey, True, True)
    x_range, y_range = (ex[3], ex[9]), (ey[2] * 0.99, ey[7] * 1.01)
    got = d.select(x_range, y_range)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    brute = (x64 >= ex[3]) & (x64 < ex[9]) & (y64 >= ey[2]) & (y64 < ey[7]) & np.isfinite(w)
    assert got.dtype == bool and got.shape == x.shape and np.array_equal(got, brute) and 0 < got.sum() < len(x)
    assert np.array_equal(d.select(), m["bin_index"] >= 0)
    assert np.array_equal(d.select(x_range=(ex[3], ex[9])), (m["bin_index"] >= 0) & (x64 >= ex[3]) & (x64 < ex[9]))
    assert not d.select((ex[3] * 1.001, ex[4]), None).any()       # no cell lies wholly inside
    with pytest.raises(ValueError):
        diagram(x, y, w, None, ex, ey, index=False)[0].select(x_range, y_range)
    with pytest.raises(ValueError):
        d.select((1.0,), None)


# ---- argument checks -----------------------------------------------------------------------------------------------------------
def test_check_phase_arguments():
    from topsy_amd import phase
    x, y, w, v = cloud(100)
    xs, ys, ws, vs, ex, ey = phase.check_phase_arguments(x.astype(np.float64), y, w, None, bins=8, x_log=True)
    assert xs.dtype == f32 and ws.dtype == f32 and vs is None and len(ex) == 9 and len(ey) == 9
    assert ex[0] == float(x.min()) and ex[-1] == np.nextafter(float(x.max()), np.inf)
    assert ey[0] == float(y.min()) and ey[-1] == np.nextafter(float(y.max()), np.inf)
    assert np.allclose(np.diff(np.log10(ex)), np.diff(np.log10(ex))[0]) and np.allclose(np.diff(ey), np.diff(ey)[0])
    _, _, _, _, ex, ey = phase.check_phase_arguments(x, y, bins=(5, 3), x_range=(1.0, 2.0), y_range=(0.0, 9.0))
    assert (len(ex), len(ey)) == (6, 4) and (ex[0], ex[-1], ey[0], ey[-1]) == (1.0, 2.0, 0.0, 9.0)
    # a logarithmic axis takes its range from the finite positive values
    z = x.copy()
    z[:5] = [0.0, -3.0, np.nan, np.inf, -np.inf]
    _, _, _, _, ex, _ = phase.check_phase_arguments(z, y, bins=4, x_log=True)
    assert ex[0] == float(z[5:].min()) and ex[-1] == np.nextafter(float(z[5:].max()), np.inf)
    _, _, _, _, ex, _ = phase.check_phase_arguments(z, y, bins=4)
    assert ex[0] == -3.0
    own = (np.array([0.0, 1.0, 5.0]), [1.0, 2.0])
    _, _, _, _, ex, ey = phase.check_phase_arguments(x, y, edges=own)
    assert ex.tolist() == [0.0, 1.0, 5.0] and ey.tolist() == [1.0, 2.0]
    bad = [dict(y=y[:-1]), dict(weights=w[:-1]), dict(values=v[:5]), dict(x=np.zeros((10, 2)), y=np.zeros(10)), dict(x=x[:0], y=y[:0]),
           dict(bins=0), dict(bins=1025), dict(bins=(4, 4, 4)), dict(bins=2.5), dict(bins=(4, True)), dict(x_range=(1.0,)),
           dict(x_range=(2.0, 1.0)), dict(y_range=(0.0, np.inf)), dict(x_range=(0.0, 1.0), x_log=True),
           dict(x=np.full(100, -1.0), x_log=True), dict(x=np.full(100, np.nan)), dict(edges=(own[0],)),
           dict(edges=(own[0], [1.0])), dict(edges=([0.0, 0.0, 1.0], own[1])), dict(edges=([0.0, np.nan], own[1])),
           dict(edges=(np.arange(1026.0), own[1])), dict(x=["a"] * 100)]
    for kw in bad:
        args = dict(x=x, y=y)
        args.update(kw)
        with pytest.raises(ValueError):
            phase.check_phase_arguments(**args)


def test_public_names():
    import topsy_amd
    from topsy_amd import kinematics, loader, phase, surface, visualizer
    assert topsy_amd.PhaseDiagram is phase.PhaseDiagram and callable(topsy_amd.phase_diagram)
    for cls in (loader.ArrayDataLoader, visualizer.Visualizer, surface.SurfaceView, kinematics.VelocityView):
        assert callable(cls.phase_diagram)
    with pytest.raises(ValueError):        # mismatched lengths are refused before any device is touched
        topsy_amd.phase_diagram(np.ones(4), np.ones(5))


def test_loader_names_are_checked_before_the_gpu():
    from topsy_amd import loader
    rs = np.random.RandomState(0)
    ld = loader.ArrayDataLoader(pos=rs.normal(size=(50, 3)), smooth=np.ones(50), mass=np.ones(50),
                                quantities={"temp": rs.uniform(1.0, 2.0, 50)})
    for kw in (dict(x="nope", y="temp"), dict(x="temp", y="T"), dict(x="temp", y="mass", weight="w"),
               dict(x="temp", y="mass", value="v_div"), dict(x="temp", y="mass", value=3)):      # (no vel: 'v_div' is no name here)
        with pytest.raises(ValueError):
            ld.phase_diagram(**kw)


# ---- the layout header ---------------------------------------------------------------------------------------------------------
H_REGIONS = ("h_x", "h_y", "h_w", "h_v")
A_REGIONS = ("a_count", "a_sums", "a_edges", "a_counters", "a_keys", "a_keys_sorted", "a_index", "a_index_sorted", "a_records_a",
             "a_records_b", "a_tmp")


def expected_levels(n, block):
    entries = [n]
    while -(-entries[-1] // block) > 1:
        entries.append(2 * -(-entries[-1] // block))
    return entries


@pytest.mark.parametrize("nx,ny", [(1, 1), (1024, 1024), (3, 5), (1, 1024)])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 10 ** 7, 2 ** 31 - 1])
def test_layout_regions(n, nx, ny):
    from topsy_amd import _native
    for has_w, has_v, want_bins in itertools.product((False, True), repeat=3):
        L = _native.histogram_2d_layout(n, nx, ny, has_w, has_v, want_bins)
        block, planes, cells = L["block"], 3 if has_v else 1, nx * ny
        assert block == _native.HIST2D_BLOCK
        entries = expected_levels(n, block)
        assert L["levels"] == len(entries) and L["blocks"] == -(-n // block)
        assert L["records_a"] == (entries[1] if len(entries) > 1 else 0) and L["records_b"] == (entries[2] if len(entries) > 2 else 0)
        for k, m in enumerate(entries[1:]):               # level k writes buffer k & 1: it holds what the next level reads
            assert m <= (L["records_b"] if k & 1 else L["records_a"])
        assert (1 << L["key_bits"]) >= cells + 1 and (L["key_bits"] == 1 or (1 << (L["key_bits"] - 1)) < cells + 1)
        record = lambda m: m * (4 + 4 + 8 * planes)
        need = {"h_x": n * 4, "h_y": n * 4, "h_w": n * 4 if has_w else 0, "h_v": n * 4 if has_v else 0,
                "a_count": cells * 8, "a_sums": planes * cells * 8, "a_edges": (nx + ny + 2) * 8, "a_counters": 16, "a_keys": n * 4,
                "a_keys_sorted": n * 4, "a_index": n * 4, "a_index_sorted": n * 4, "a_records_a": record(L["records_a"]),
                "a_records_b": record(L["records_b"]), "a_tmp": 0}
        for regions, total in ((H_REGIONS, "h_bytes"), (A_REGIONS, "a_bytes")):
            end = 0
            for name in regions:
                assert L[name] % 16 == 0 and L[name] >= end, (name, L)                 # aligned, after the region before
                assert L[name + "_size"] >= need[name], (name, L)                      # large enough for what the kernels index
                end = L[name] + L[name + "_size"]
            assert end <= L[total] and L[total] % 16 == 0, (total, L)
        assert L["bins_bytes"] == (n * 4 if want_bins else 0)
        assert L["h_bytes"] <= 4 * (n * 4 + 256) and L["a_bytes"] <= need["a_count"] + need["a_sums"] + 17 * n + 2 ** 20


def test_layout_refusals_and_constants():
    import re
    from topsy_amd import _native
    for args in ((0, 4, 4), (-1, 4, 4), (2 ** 31, 4, 4), (10, 0, 4), (10, 4, 0), (10, 1025, 4), (10, 4, 1025)):
        with pytest.raises(_native.BackendError):
            _native.histogram_2d_layout(*args)
    text = open(os.path.join(ROOT, "topsy_amd", "csrc", "tsp_hist2d_layout.h")).read()
    const = {k: v for k, v in re.findall(r"constexpr \w+ (\w+) = ([^;]+);", text)}
    assert int(const["BLOCK"]) == _native.HIST2D_BLOCK and int(const["MAX_BINS"]) == _native.HIST2D_MAX_BINS == 1024
    public = open(os.path.join(ROOT, "include", "topsy_splat.h")).read()
    assert f"#define TSP_HIST2D_LAYOUT_VALUES {len(_native.HIST2D_LAYOUT_NAMES)}" in public
    assert f"#define TSP_HIST2D_BLOCK {_native.HIST2D_BLOCK}" in public and "#define TSP_HIST2D_MAX_BINS 1024" in public
    assert _native.load_library().tsp_version() >= 127


def test_layout_header_under_the_sanitizers(tmp_path):
    """tools/hist2d_layout_check.cpp, a program of its own, built with -fsanitize=address,undefined and run: nothing loaded into
    this interpreter is instrumented."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "hist2d_layout_check")
    # the runtimes go into the program itself (clang's default, an option of gcc), so that it runs whatever else the process loads
    version = subprocess.run([cxx, "--version"], capture_output=True, text=True, timeout=60).stdout
    runtime = [] if "clang" in version else ["-static-libasan", "-static-libubsan"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *runtime,
                            "-I", os.path.join(ROOT, "topsy_amd", "csrc"), os.path.join(ROOT, "tools", "hist2d_layout_check.cpp"),
                            "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "record slots hold" in run.stdout, run.stdout + run.stderr
