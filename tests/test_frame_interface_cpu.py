"""VisualizerBase and SurfaceView take their frame interface from one class (topsy_amd/frames.py): the frame methods are the
same function objects on both, so that the two cannot drift apart again (no device)."""
import pytest

from topsy_amd.frames import FrameInterface
from topsy_amd.surface import SurfaceView
from topsy_amd.visualizer import VisualizerBase

SHARED = ["get_presentation_image", "get_presentation_image_yuv420", "_present", "_presentation_layers", "_get_colorbar_label",
          "display_status", "add_frame_listener", "remove_frame_listener", "_frame_produced", "_init_frames"]


@pytest.mark.parametrize("name", SHARED)
def test_frame_methods_are_the_same_functions(name):
    assert getattr(VisualizerBase, name) is getattr(SurfaceView, name) is getattr(FrameInterface, name)
    assert name not in vars(VisualizerBase) and name not in vars(SurfaceView)


def test_switch_defaults_are_shared():
    for name, value in [("show_status", True), ("show_colorbar", True), ("show_scalebar", True), ("crosshairs_visible", False)]:
        assert getattr(VisualizerBase, name) is getattr(SurfaceView, name) is value
        assert name not in vars(VisualizerBase) and name not in vars(SurfaceView)

