"""Phase diagrams: weighted 2-D histograms of per-particle quantities (tsp_histogram_2d, include/topsy_splat.h "Weighted 2-D
histograms") -- the mass in each cell of a (rho, T) plane, or any quantity against any other weighted by a third: pynbody's
plot.rho_T / plot.generic.hist2d for arrays.  Everything here is NumPy; the sums come from Context.histogram_2d.

hist_edges builds the bin edges, check_phase_arguments validates what topsy_amd.phase_diagram is given, compute_phase_diagram runs
the call on a context, and PhaseDiagram turns the raw counts and sums into the weight, mean and dispersion per cell.

The bins are half-open: column i holds edges_x[i] <= x < edges_x[i + 1], and a value equal to the last edge is outside (the radial
profile's rule, not numpy.histogram2d's closed last bin); automatic ranges end one float64 ulp above the maximum, so that it is
binned."""
import numpy as np

MAX_BINS = 1024              # tsp_histogram_2d's limit per axis


def _finite_number(name, value):
    if isinstance(value, (bool, str)):
        raise ValueError(f"{name} must be a finite number, not {value!r}")
    try:
        value = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a finite number, not {value!r}") from None
    if not np.isfinite(value):
        raise ValueError(f"{name} must be a finite number, not {value!r}")
    return value


def hist_edges(lo, hi, n_bins, log=False):
    """The n_bins + 1 float64 edges of n_bins (1 to 1024) bins from lo to hi > lo, both end points exact: lo + (hi - lo) * k / n_bins,
    or with log (needs lo > 0) lo * (hi / lo) ** (k / n_bins).  Raises ValueError."""
    if isinstance(n_bins, bool) or not isinstance(n_bins, (int, np.integer)) or not 1 <= n_bins <= MAX_BINS:
        raise ValueError(f"n_bins must be an integer from 1 to {MAX_BINS}, not {n_bins!r}")
    lo, hi = _finite_number("lo", lo), _finite_number("hi", hi)
    if not lo < hi:
        raise ValueError(f"lo = {lo!r} must be below hi = {hi!r}")
    k = np.arange(n_bins + 1, dtype=np.float64) / n_bins
    if log:
        if not lo > 0:
            raise ValueError(f"logarithmic bins need lo > 0, not {lo!r}")
        edges = lo * (hi / lo) ** k
    else:
        edges = lo + (hi - lo) * k
    edges[0], edges[-1] = lo, hi
    if not (np.diff(edges) > 0).all():
        raise ValueError(f"{n_bins} bins between {lo!r} and {hi!r} are not distinct in float64")
    return edges


def check_edges(name, edges):
    """The caller's own edges as float64: 2 to 1025 finite, strictly ascending numbers.  Raises ValueError."""
    try:
        e = np.array(edges, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be an ascending array of numbers, not {edges!r}") from None
    if e.ndim != 1 or not 2 <= len(e) <= MAX_BINS + 1:
        raise ValueError(f"{name} must be 2 to {MAX_BINS + 1} numbers, not shape {e.shape}")
    if not np.isfinite(e).all() or not (np.diff(e) > 0).all():
        raise ValueError(f"{name} must be finite and strictly ascending")
    return e


def auto_range(name, a, log):
    """(lo, hi) of the finite values of a (with log: the finite values > 0): the minimum, and the maximum moved up by one float64 ulp
    of itself, so that the maximum falls into the last bin.  Raises ValueError where no value qualifies."""
    a = np.asarray(a, dtype=np.float64)
    use = np.isfinite(a) & (a > 0) if log else np.isfinite(a)
    if not use.any():
        raise ValueError(f"{name} has no finite{' positive' if log else ''} value to take a range from: pass {name}_range")
    lo, hi = float(a[use].min()), float(a[use].max())
    return lo, float(np.nextafter(hi, np.inf))


def _check_range(name, value):
    try:
        lo, hi = value
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be None or (lo, hi), not {value!r}") from None
    return _finite_number(f"{name}[0]", lo), _finite_number(f"{name}[1]", hi)


def _column(name, a, n):
    try:
        a = np.asarray(a)
        if a.dtype.kind not in "fiu":
            raise TypeError
        a = np.ascontiguousarray(a, dtype=np.float32)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a 1-D array of numbers") from None
    if a.ndim != 1 or (n is not None and len(a) != n):
        raise ValueError(f"{name} must have shape ({'n' if n is None else n},), not {a.shape}")
    return a


def check_phase_arguments(x, y, weights=None, values=None, x_range=None, y_range=None, bins=(256, 256), x_log=False, y_log=False,
                          edges=None):
    """The arguments of topsy_amd.phase_diagram, checked: (x, y, weights, values as float32 (n,) or None; edges_x, edges_y as
    float64).  edges = (edges_x, edges_y) takes the caller's own edges; else bins (an int or a pair (nx, ny)) between x_range /
    y_range, None: the range of the finite (log: and positive) values.  Raises ValueError."""
    x = _column("x", x, None)
    n = len(x)
    if n < 1:
        raise ValueError("x is empty")
    y = _column("y", y, n)
    w = None if weights is None else _column("weights", weights, n)
    v = None if values is None else _column("values", values, n)
    if edges is not None:
        try:
            ex, ey = edges
        except (TypeError, ValueError):
            raise ValueError("edges must be None or the pair (edges_x, edges_y)") from None
        return x, y, w, v, check_edges("edges_x", ex), check_edges("edges_y", ey)
    if isinstance(bins, (int, np.integer)) and not isinstance(bins, bool):
        bins = (bins, bins)
    try:
        nx, ny = bins
    except (TypeError, ValueError):
        raise ValueError(f"bins must be an integer or a pair (nx, ny), not {bins!r}") from None
    out = []
    for name, a, rng, nb, log in (("x", x, x_range, nx, x_log), ("y", y, y_range, ny, y_log)):
        lo, hi = auto_range(name, a, log) if rng is None else _check_range(f"{name}_range", rng)
        out.append(hist_edges(lo, hi, nb, bool(log)))
    return x, y, w, v, out[0], out[1]


class PhaseDiagram:
    """A weighted 2-D histogram built from the raw counts and sums of tsp_histogram_2d by NumPy alone.  Arrays are (ny, nx): row j is
    the y bin, column i the x bin.

    count: the particles per cell; weight: sum w (the count as float64 without weights); with values, mean = sum w v / sum w and
    dispersion = sqrt(max(<v^2> - <v>^2, 0)), NaN where sum w is 0 (None without values).  x_centres / y_centres: the bin centres,
    geometric for a logarithmic axis.  density: weight per cell area in the plotted coordinates -- per dlog10 x for a logarithmic
    axis, per dx for a linear one -- what pynbody's rho_T draws.  info: n_valid (particles with finite x, y, weight and value)
    and n_binned (those in a cell).  bin_index: the cell j * nx + i of every particle, -1 for none (only with return_index)."""

    def __init__(self, edges_x, edges_y, count, sums, info, bin_index=None, x_log=False, y_log=False):
        self.edges_x = np.asarray(edges_x, dtype=np.float64)
        self.edges_y = np.asarray(edges_y, dtype=np.float64)
        self.x_log, self.y_log = bool(x_log), bool(y_log)
        nx, ny = len(self.edges_x) - 1, len(self.edges_y) - 1
        self.count = np.asarray(count, dtype=np.int64).reshape(ny, nx)
        self.sums = np.asarray(sums, dtype=np.float64).reshape(-1, ny, nx)
        if self.sums.shape[0] not in (1, 3):
            raise ValueError(f"sums must hold 1 or 3 planes, not {self.sums.shape[0]}")
        self.info = dict(info)
        self.bin_index = None if bin_index is None else np.asarray(bin_index, dtype=np.int32)
        self.weight = self.sums[0].copy()
        self.x_centres = self._centres(self.edges_x, self.x_log)
        self.y_centres = self._centres(self.edges_y, self.y_log)
        self.mean = self.dispersion = None
        with np.errstate(divide="ignore", invalid="ignore"):
            if self.sums.shape[0] == 3:
                occupied = self.weight != 0
                self.mean = np.where(occupied, self.sums[1] / self.weight, np.nan)
                second = np.where(occupied, self.sums[2] / self.weight, np.nan)
                self.dispersion = np.sqrt(np.maximum(second - self.mean * self.mean, 0.0))
            self.density = self.weight / (self._widths(self.edges_y, self.y_log)[:, None] * self._widths(self.edges_x, self.x_log)[None, :])

    @staticmethod
    def _centres(edges, log):
        return np.sqrt(edges[:-1] * edges[1:]) if log else 0.5 * (edges[:-1] + edges[1:])

    @staticmethod
    def _widths(edges, log):
        return np.diff(np.log10(edges)) if log else np.diff(edges)

    @property
    def shape(self):
        return self.count.shape

    def select(self, x_range=None, y_range=None):
        """A boolean mask over the particles: those binned into a cell that lies wholly inside the rectangle -- a column i with
        x_range[0] <= edges_x[i] and edges_x[i + 1] <= x_range[1], a row likewise; None: every column / row.  Needs the diagram's
        bin_index (return_index=True); ValueError without."""
        if self.bin_index is None:
            raise ValueError("this diagram holds no bin index: ask for it with return_index=True")
        nx = len(self.edges_x) - 1
        keep = []
        for name, edges, rng in (("x_range", self.edges_x, x_range), ("y_range", self.edges_y, y_range)):
            if rng is None:
                keep.append(np.ones(len(edges) - 1, dtype=bool))
            else:
                lo, hi = _check_range(name, rng)
                keep.append((edges[:-1] >= lo) & (edges[1:] <= hi))
        cell = self.bin_index.astype(np.int64)
        inside = cell >= 0
        safe = np.where(inside, cell, 0)
        return inside & keep[0][safe % nx] & keep[1][safe // nx]


def compute_phase_diagram(ctx, x, y, w, v, edges_x, edges_y, x_log=False, y_log=False, return_index=False):
    """The PhaseDiagram of checked arguments (check_phase_arguments) on an existing context."""
    raw = ctx.histogram_2d(x, y, w, v, edges_x=edges_x, edges_y=edges_y, want_bins=bool(return_index))
    info = {"n_valid": raw["n_valid"], "n_binned": raw["n_binned"]}
    return PhaseDiagram(edges_x, edges_y, raw["count"], raw["sums"], info, raw.get("bin_index"), x_log, y_log)
