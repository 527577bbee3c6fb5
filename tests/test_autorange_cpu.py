"""The host half of the device autorange, without a GPU: Colormap.autorange_on_device over a numpy model of tsp_content_sort
(tests/postpass_ref.py) must set exactly the parameters autorange_vmin_vmax sets from the image itself, on the degenerate images
where the two formulations could part: non-finite content of every class, empty and tiny samples on both sides of the `> 2` and
`> 200` thresholds, denormals, overflow through the mass scale, signed zeros.  tests/test_gpu_postpass.py repeats the same images
on the device."""
import numpy as np
import pytest

import postpass_ref
from topsy_amd.colormap.implementation import Colormap, BivariateColormap, RGBColormap, RGBHDRColormap

MAPS = {
    "density": (Colormap, {"type": "density", "weighted_average": False}, "rgba8unorm"),
    "weighted": (Colormap, {"type": "density", "weighted_average": True}, "rgba8unorm"),
    "bivariate_density": (BivariateColormap, {"type": "bivariate", "weighted_average": False}, "rgba8unorm"),
    "bivariate_weighted": (BivariateColormap, {"type": "bivariate", "weighted_average": True}, "rgba8unorm"),
    "rgb": (RGBColormap, {"type": "rgb", "hdr": False}, "rgba8unorm"),
    "rgb_hdr": (RGBHDRColormap, {"type": "rgb", "hdr": True}, "rgba16float"),
}
IMAGES = postpass_ref.autorange_images()
IMAGES_RGB = postpass_ref.autorange_images_rgb()


class _Texture:
    def __init__(self, context):
        self.context = context


def _run(fn):
    """-> ("ok", parameters) or ("raised", exception type name)"""
    try:
        return "ok", fn()
    except Exception as e:       # noqa: BLE001 -- both formulations must fail together, whatever numpy raises on an empty sample
        return "raised", type(e).__name__


def host_and_device(map_name, img, scale):
    cls, params, fmt = MAPS[map_name]

    def host():
        cm = cls(None, _Texture(None), fmt, dict(params))
        with np.errstate(all="ignore"):
            cm.autorange_vmin_vmax(img * np.float32(scale))
        return cm.get_parameters()

    def device():
        cm = cls(None, _Texture(postpass_ref.FakeContentContext(img)), fmt, dict(params))
        cm.autorange_on_device(scale)
        return cm.get_parameters()
    return _run(host), _run(device)


def _cases():
    for m in MAPS:
        for name in (IMAGES_RGB if m.startswith("rgb") else IMAGES):
            yield m, name


@pytest.mark.parametrize("scale", [1.0, 3.7])
@pytest.mark.parametrize("map_name,image", list(_cases()))
def test_device_formulation_equals_host(map_name, image, scale):
    img = (IMAGES_RGB if map_name.startswith("rgb") else IMAGES)[image]
    (h_state, host), (d_state, dev) = host_and_device(map_name, img, scale)
    assert h_state == d_state, (host, dev)
    if h_state == "ok":
        k = postpass_ref.autorange_parameters_equal(host, dev)
        assert k is None, (k, host[k], dev[k])


def test_neg_inf_content_switches_to_linear():
    """The case the device path used to miss: a single -inf among positive content makes the host rule (vals < 0).any() true."""
    for name in ("neg_inf_content", "one_neg_inf_content"):
        (_, host), (_, dev) = host_and_device("weighted", IMAGES[name], 1.0)
        assert not host["log"] and not dev["log"]
        assert dev["vmin"] > 0      # linear percentiles of the positive ratios, not their logarithms
    (_, host), (_, dev) = host_and_device("weighted", IMAGES["pos_inf_content"], 1.0)
    assert host["log"] and dev["log"]    # +inf is ignored by both


def test_reference_model_itself():
    """content_values_ref on a hand-made image: counts, order, -0.0 before +0.0, every non-finite class dropped."""
    img = np.zeros((2, 2, 2), dtype=np.float32)
    img[..., 0] = [[0.0, -0.0], [2.0, -3.0]]
    img[..., 1] = [[-1.0, 1.0], [np.inf, np.nan]]
    v, nf, nnp = postpass_ref.content_values_ref(img, 0, 1.0)
    assert (nf, nnp) == (4, 3) and np.array_equal(v.view(np.uint32), np.array([-3.0, -0.0, 0.0, 2.0], dtype=np.float32).view(np.uint32))
    v, nf, nnp = postpass_ref.content_values_ref(img, 1, 1.0)       # -inf, -inf (1 / -0), +inf, NaN: nothing finite
    assert (nf, nnp, v.size) == (0, 0, 0)
    ctx = postpass_ref.FakeContentContext(img)
    with pytest.raises(postpass_ref.FakeBackendError):
        ctx.content_values([0])
    assert ctx.content_sort(1) == (0, 0) and ctx.content_neg_inf() == 2
    assert ctx.content_sort(3) == (6, 4) and ctx.content_neg_inf() == 0
    with pytest.raises(postpass_ref.FakeBackendError):
        ctx.content_values([6])
    with pytest.raises(postpass_ref.FakeBackendError):
        ctx.content_sort(2)
