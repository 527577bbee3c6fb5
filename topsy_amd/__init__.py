"""topsy_amd -- MI355X-native SPH particle-splatting backend for topsy's render path.

    import topsy_amd
    vis = topsy_amd.test(1000, render_resolution=200)      # as reference topsy.test(...)
    vis.scale = 200.0
    img = vis.get_sph_presentation_image()                 # (200, 200, 4) uint8

The GPU work goes through libtopsy_splat.so (include/topsy_splat.h).  There is no CPU fallback.
"""
import numpy as np

from . import config
from .drawreason import DrawReason

__version__ = "0.1.0"


def test(nparticle=config.TEST_DATA_NUM_PARTICLES_DEFAULT, **kwargs):
    """Visualizer over the seeded synthetic snapshot (mirror of reference topsy.test, __init__.py:180-187)."""
    from . import visualizer, loader
    kwargs.pop("canvas_class", None)
    return visualizer.Visualizer(data_loader_class=loader.TestDataLoader, data_loader_args=(nparticle,),
                                 data_loader_kwargs={"with_cells": kwargs.pop("with_cells", False),
                                                     "periodic": kwargs.get("periodic_tiling", False)},
                                 **kwargs)


def from_arrays(pos, smooth, mass, quantities=None, rgb=None, with_cells=False, n_smooth=None, periodicity_scale=None,
                **kwargs):
    """Visualizer over caller-supplied numpy arrays (e.g. taken from a pynbody snapshot).

    smooth=None computes the smoothing lengths on the GPU from the n_smooth (default config.SMOOTH_NEIGHBOURS) nearest
    neighbours, in the periodic box of side periodicity_scale if one is given; vis.data_loader.get_smooth() returns them."""
    from . import visualizer, loader
    return visualizer.Visualizer(data_loader_class=loader.ArrayDataLoader,
                                 data_loader_kwargs={"pos": pos, "smooth": smooth, "mass": mass,
                                                     "quantities": quantities, "rgb": rgb, "with_cells": with_cells,
                                                     "n_smooth": n_smooth, "periodicity_scale": periodicity_scale},
                                 **kwargs)


def smoothing_lengths(pos, n_smooth=config.SMOOTH_NEIGHBOURS, periodicity_scale=None, device_id=0):
    """SPH smoothing lengths of an (n, 3) position array on GPU `device_id`: half the distance to the n_smooth-th nearest
    particle, the particle itself included (pynbody's snap['smooth'] convention); NaN where a coordinate is not finite.
    periodicity_scale: side of a periodic box (None: open).  Returns float32 (n,), to be cached as the caller likes."""
    from . import _native, loader
    n_smooth, period = loader.check_smoothing_arguments(n_smooth, periodicity_scale)
    pos = np.asarray(pos, dtype=np.float32)
    if pos.ndim != 2 or pos.shape[1] != 3:
        raise ValueError(f"pos must have shape (n, 3), not {pos.shape}")
    n_finite = int(np.isfinite(pos).all(axis=1).sum())
    if n_finite < n_smooth:
        raise ValueError(f"{n_finite} particles have finite coordinates; n_smooth = {n_smooth} needs at least as many")
    ctx = _native.Context(1, 2, device_id)
    try:
        return ctx.smoothing_lengths(pos[:, 0], pos[:, 1], pos[:, 2], n_smooth, period)
    finally:
        ctx.close()


def SurfaceView(visualizer, **colormap_params):
    """Surface rendering of `visualizer`'s scene (the reference's render_mode "surface"): the front-most sphere of every
    particle above a density cut, smoothed and lit.  render(), get_sph_image() ((R, R, 2) filtered (q, depth)),
    get_sph_presentation_image() ((R, R, 4) uint8), colormap_autorange(), view["depth_scale"] etc., density_cut_percentile."""
    from . import surface
    return surface.SurfaceView(visualizer, **colormap_params)


def __getattr__(name):
    """topsy_amd.VisualizationRecorder (movie recording and export, topsy_amd/recorder), imported on first use."""
    if name == "VisualizationRecorder":
        from .recorder import VisualizationRecorder
        return VisualizationRecorder
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def synthetic_on_device(n_total, first=0, count=None, h_cap=0.0, **kwargs):
    """Visualizer over a device-generated shard of the synthetic snapshot (1e8-1e9 particles)."""
    from . import visualizer, loader
    return visualizer.Visualizer(data_loader_class=loader.DeviceSyntheticLoader,
                                 data_loader_kwargs={"n_total": n_total, "first": first, "count": count,
                                                     "h_cap": h_cap},
                                 **kwargs)
