"""Plain references of the image post-passes (test infrastructure; no GPU, no topsy_amd kernel):
  content_values_ref ..... what tsp_content_sort / tsp_content_values are defined to return (include/topsy_splat.h, "On-device
                           autorange support"): the content in numpy float32, the finite values sorted ascending;
  FakeContentContext ..... the three content calls of topsy_amd._native.Context on top of it, so that the host half of
                           Colormap.autorange_on_device runs without a GPU;
  tile_periodic_f64 ...... tsp_tile_periodic with the tap positions of oracle_np.periodic_tile (float32: they are the definition) but
                           the bilinear values, the weights and the running sum in float64, plus the quantities of its error bound;
  autorange_images ....... the degenerate images the autorange is tried on, shared by the CPU and the GPU tests."""
import numpy as np

f32 = np.float32


# --------------------------------------------------------------------------------------------- order statistics
def content_all(img, kind, scale):
    """Every content value, flattened, non-finite ones included (kind as tsp_content_sort)."""
    img = np.asarray(img, dtype=f32)
    s = f32(scale)
    with np.errstate(all="ignore"):
        if kind == 0:
            v = img[..., 0] * s
        elif kind == 1:
            v = (img[..., 1] * s) / (img[..., 0] * s)
        elif kind == 2:
            v = img[..., :3] * s
        elif kind == 3:
            v = img * s
        else:
            raise ValueError(f"bad content kind {kind}")
    return np.ascontiguousarray(v, dtype=f32).ravel()


def content_values_ref(img, kind, scale):
    """-> (sorted finite float32 values, n_finite, n_nonpositive).  The library's order is by bit pattern, -0.0 before +0.0;
    np.sort compares them equal and may hand back either sign for any of them (its vectorised float32 sort does not keep the
    signs of zeros apart), so the zeros are counted by sign before the sort and written back in the library's order."""
    v = content_all(img, kind, scale)
    fin = v[np.isfinite(v)]
    n_neg_zero = int(((fin == 0) & np.signbit(fin)).sum())
    fin = np.sort(fin)
    zero = fin == 0
    zeros = np.zeros(int(zero.sum()), dtype=f32)
    zeros[:n_neg_zero] = f32(-0.0)
    fin[zero] = zeros
    return fin, int(fin.size), int((fin <= 0).sum())


class FakeBackendError(RuntimeError):
    pass


class FakeContentContext:
    """content_sort / content_values / content_neg_inf of _native.Context over a host image (R, R, C)."""

    def __init__(self, img):
        self.img = np.ascontiguousarray(img, dtype=f32)
        self._sorted = None
        self._neg_inf = 0

    def content_sort(self, kind, scale=1.0):
        if kind == 2 and self.img.shape[-1] != 4:
            raise FakeBackendError("error -1: rgb content needs a 4-channel image")
        self._sorted, n_finite, n_nonpositive = content_values_ref(self.img, kind, scale)
        self._neg_inf = int(np.isneginf(content_all(self.img, kind, scale)).sum())
        return n_finite, n_nonpositive

    def content_values(self, ranks):
        if self._sorted is None:
            raise FakeBackendError("error -4: content_sort has not been called")
        r = np.asarray(ranks, dtype=np.int64)
        if ((r < 0) | (r >= self._sorted.size)).any():
            raise FakeBackendError(f"error -1: rank outside [0, {self._sorted.size})")
        return self._sorted[r].copy()

    def content_neg_inf(self):
        if self._sorted is None:
            raise FakeBackendError("error -4: content_sort has not been called")
        return self._neg_inf


# --------------------------------------------------------------------------------------------- periodic tiling
def tile_axis(R, shift):
    """The taps of one image axis for one instance, float32 as oracle_np.periodic_tile (and the header) define them:
    -> (inside, i0, i1, f) over the R pixel centres; a NaN shift is inside nowhere."""
    centres = np.arange(R, dtype=f32) + f32(0.5)
    with np.errstate(invalid="ignore"):
        s = centres - f32(shift)
        inside = (s >= 0) & (s < f32(R))
        t = s - f32(0.5)
        t0 = np.floor(t)
        f = (t - t0).astype(f32)
        i = np.where(np.isfinite(t0), t0, 0).astype(np.int64)
    return inside, np.clip(i, 0, R - 1), np.clip(i + 1, 0, R - 1), f


def _instances(offsets, weights, R):
    halfR = f32(0.5) * f32(R)
    for (ox, oy), w in zip(np.asarray(offsets, dtype=f32).reshape(-1, 2), np.asarray(weights, dtype=f32).ravel()):
        yield tile_axis(R, ox * halfR), tile_axis(R, -(oy * halfR)), w          # +x clip -> +column, +y clip -> -row


def tile_inside_count(R, offsets):
    """(R, R): how many instances cover each output pixel"""
    count = np.zeros((R, R), dtype=np.int64)
    for (inx, _, _, _), (iny, _, _, _), _ in _instances(offsets, np.ones(len(np.asarray(offsets).reshape(-1, 2))), R):
        count += iny[:, None] & inx[None, :]
    return count


def tile_touch_mask(R, offsets, pixel):
    """(R, R) bool: the output pixels with an instance inside one of whose four taps is source pixel (row, column) = `pixel`"""
    bj, bi = pixel
    touched = np.zeros((R, R), dtype=bool)
    for (inx, i0, i1, _), (iny, j0, j1, _), _ in _instances(offsets, np.ones(len(np.asarray(offsets).reshape(-1, 2))), R):
        touched |= (iny & ((j0 == bj) | (j1 == bj)))[:, None] & (inx & ((i0 == bi) | (i1 == bi)))[None, :]
    return touched


def tile_periodic_f64(img, offsets, weights):
    """-> (sum, A, count): sum = the tiled image in float64 arithmetic on the float32 tap positions of oracle_np.periodic_tile;
    A = the same sum over |src| and |w| (the scale of the rounding error); count (R, R) = instances inside per pixel."""
    img = np.asarray(img, dtype=f32)
    R, _, C = img.shape
    src = img.astype(np.float64)
    mag = np.abs(src)
    total = np.zeros((R, R, C))
    A = np.zeros((R, R, C))
    count = np.zeros((R, R), dtype=np.int64)

    def bilinear(a, i0, i1, fx, j0, j1, fy):
        fx, fy = fx.astype(np.float64), fy.astype(np.float64)
        gx, gy = (1.0 - fx)[None, :, None], (1.0 - fy)[:, None, None]
        fx, fy = fx[None, :, None], fy[:, None, None]
        top = a[j0][:, i0] * gx + a[j0][:, i1] * fx
        bot = a[j1][:, i0] * gx + a[j1][:, i1] * fx
        return top * gy + bot * fy
    for (inx, i0, i1, fx), (iny, j0, j1, fy), w in _instances(offsets, weights, R):
        mask = iny[:, None] & inx[None, :]
        total += np.where(mask[..., None], bilinear(src, i0, i1, fx, j0, j1, fy) * float(w), 0.0)
        A += np.where(mask[..., None], bilinear(mag, i0, i1, fx, j0, j1, fy) * abs(float(w)), 0.0)
        count += mask
    return total, A, count


def tiling_bound(A, count):
    """|float32 result - float64 sum| <= (count + 6) * 2^-24 * A: every instance value passes six float32 roundings on its longest
    path (1 - f, product, sum for the row; product, sum for the column; the weight), each relative 2^-24 of a quantity bounded by
    the pixel's share of A, and every accumulation adds one rounding of a partial sum bounded by A."""
    return (count[..., None] + 6) * 2.0 ** -24 * A


# --------------------------------------------------------------------------------------------- autorange inputs
AUTORANGE_KEYS = ("vmin", "vmax", "log", "ui_range_linear", "ui_range_log", "density_vmin", "density_vmax", "ui_range_density")
AUTORANGE_R = 32


def _k_positive(rs, k):
    """exactly k pixels with finite positive content (both kinds); NaN elsewhere"""
    R = AUTORANGE_R
    img = np.full((R * R, 2), np.nan, dtype=f32)
    where = rs.choice(R * R, k, replace=False)
    img[where, 0] = np.exp(rs.uniform(-3, 3, size=k))
    img[where, 1] = np.exp(rs.uniform(-3, 3, size=k)) * img[where, 0]
    return img.reshape(R, R, 2)


def autorange_images():
    """name -> (R, R, 2) float32, seeded.  The names say which branch of the autorange each is there for."""
    R = AUTORANGE_R
    rs = np.random.RandomState(20240611)
    out = {}

    def positive():
        img = np.empty((R, R, 2), dtype=f32)
        img[..., 0] = np.exp(rs.uniform(-3, 3, size=(R, R)))
        img[..., 1] = np.exp(rs.uniform(-2, 1, size=(R, R))) * img[..., 0]
        return img
    signed = positive()
    signed[..., 1] = rs.normal(size=(R, R)) * signed[..., 0]
    out["signed"] = signed
    out["positive"] = positive()
    img = positive()
    img.reshape(-1, 2)[rs.choice(R * R, 5, replace=False)] = (0.0, -1.0)         # ch1 / ch0 = -inf
    out["neg_inf_content"] = img
    img = positive()
    img.reshape(-1, 2)[rs.choice(R * R, 1, replace=False)] = (0.0, -1.0)
    out["one_neg_inf_content"] = img
    img = positive()
    img.reshape(-1, 2)[rs.choice(R * R, 40, replace=False)] = (0.0, 0.0)         # 0 / 0 = NaN
    out["nan_content"] = img
    img = positive()
    img.reshape(-1, 2)[rs.choice(R * R, 40, replace=False)] = (0.0, 2.5)         # +inf
    out["pos_inf_content"] = img
    out["all_zero"] = np.zeros((R, R, 2), dtype=f32)
    out["all_nan"] = np.full((R, R, 2), np.nan, dtype=f32)
    img = np.empty((R, R, 2), dtype=f32)
    img[..., 0], img[..., 1] = 0.3, 0.75
    out["constant"] = img
    for k in (2, 3, 200, 201):
        out[f"{k}_positive"] = _k_positive(rs, k)
    img = positive()
    img[..., 0] = (rs.randint(1, 5000, size=(R, R)) * 1.4e-45).astype(f32)       # denormal ch0
    img[..., 1] = rs.uniform(0.5, 2.0, size=(R, R)).astype(f32) * img[..., 0]
    out["denormal_ch0"] = img
    img = positive()
    img[..., 0] = rs.uniform(0.5e38, 3.0e38, size=(R, R))                        # scale 3.7 overflows most of it
    img[..., 1] = rs.uniform(0.1, 1.0, size=(R, R)).astype(f32) * img[..., 0]
    out["near_float_max"] = img
    img = positive()
    flat = img.reshape(-1, 2)
    flat[rs.choice(R * R, 30, replace=False)] = (-0.0, -0.0)
    flat[rs.choice(R * R, 30, replace=False), 1] = -0.0                          # weighted content -0.0: not negative
    out["negative_zero"] = img
    return out


def autorange_images_rgb():
    """name -> (R, R, 4) float32: every 2-channel image with two NaN channels beside it, then a plain rgb image whose fragment-count channel holds the largest values (it takes part in the
    percentile: kind 3), and one whose green channel is 0 everywhere."""
    R = AUTORANGE_R
    out = {name: np.concatenate([img, np.full_like(img, np.nan)], axis=-1) for name, img in autorange_images().items()}
    for k in (2, 3, 200, 201):                   # kind 3 takes every channel: one positive value per chosen pixel, k in all
        out[f"{k}_positive"][..., 1] = np.nan
    rs = np.random.RandomState(77)
    img = np.empty((R, R, 4), dtype=f32)
    img[..., :3] = np.exp(rs.uniform(-20, 5, size=(R, R, 3)))
    img[..., 3] = rs.randint(0, 3000, size=(R, R))
    out["rgb_with_count_channel"] = img
    img = img.copy()
    img[..., 1] = 0.0
    out["rgb_zero_green"] = img
    return out


def autorange_parameters_equal(host, dev):
    """The equality of test_device_autorange_equals_host_autorange, with NaN equal to NaN; returns the first differing key."""
    for k in AUTORANGE_KEYS:
        if (k in host) != (k in dev):
            return k
        if k in host and not np.array_equal(np.asarray(host[k], dtype=np.float64), np.asarray(dev[k], dtype=np.float64), equal_nan=True):
            return k
    return None
