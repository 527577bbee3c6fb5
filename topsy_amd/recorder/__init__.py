"""Record camera and colormap changes, replay them at a fixed frame rate and write a movie (topsy's recorder package).

    rec = VisualizationRecorder(vis)
    rec.record()
    ...                      # every frame the visualizer produces samples the view state
    rec.stop()
    rec.save_y4m("fly.y4m", 30, (1920, 1080))       # no library needed; any encoder reads it
    rec.save_mp4("fly.mp4", 30, (1920, 1080))       # through an ffmpeg executable

The timestream files (save_timestream / load_timestream) have the desktop recorder's layout, so a path recorded in topsy on a
subsample replays here on the full snapshot and the reverse.  Two departures from topsy's recorder, both deliberate:
set_vmin_vmax=False really leaves colormap[vmin] and colormap[vmax] alone (topsy's exclusion list names 'vmin' and 'vmax',
which match no recorded property), and a replay gives show_colorbar and show_scalebar back the values they had before (topsy
sets both to True).  Movie frames are composed and converted to 4:2:0 on the GPU (tsp_present_yuv420).
"""
import copy
import fractions
import math
import pickle
import shutil
import subprocess
import tempfile
import time

from .interpolator import (Interpolator, LinearInterpolator, RotationInterpolator, SmoothedLinearInterpolator,
                           SmoothedRotationInterpolator, SmoothedStepInterpolator, StepInterpolator)

__all__ = ["VisualizationRecorder", "Interpolator", "LinearInterpolator", "RotationInterpolator", "StepInterpolator",
           "SmoothedLinearInterpolator", "SmoothedRotationInterpolator", "SmoothedStepInterpolator"]

STATUS_TEXT = "github.com/pynbody/topsy/"


def _get_property(vis, name):
    """vis.colormap[key] for "colormap[key]" (None when the active map has no such parameter), else the attribute."""
    if name.startswith("colormap["):
        return vis.colormap[name[len("colormap["):-1]]
    return getattr(vis, name)


def _set_property(vis, name, value):
    if name.startswith("colormap["):
        vis.colormap[name[len("colormap["):-1]] = value
    else:
        setattr(vis, name, value)


def fps_ratio(fps):
    """The frame rate as the exact ratio a y4m header carries: integers as n:1, the NTSC rates n * 1000/1001 (23.976, 29.97,
    59.94 ...) as (1000 n):1001, anything else as the nearest ratio with a denominator up to 1000000."""
    if isinstance(fps, fractions.Fraction):
        ratio = fps
    else:
        fps = float(fps)
        if not (math.isfinite(fps) and fps > 0):
            raise ValueError(f"fps must be finite and > 0, not {fps}")
        n = round(fps)
        ntsc = round(fps * 1.001)
        if abs(fps - n) < 1e-9:
            ratio = fractions.Fraction(n, 1)
        elif abs(fps - ntsc * 1000 / 1001) < 1e-4:
            return ntsc * 1000, 1001
        else:
            ratio = fractions.Fraction(fps).limit_denominator(1000000)
    if ratio <= 0:
        raise ValueError(f"fps must be > 0, not {fps}")
    return ratio.numerator, ratio.denominator


def y4m_header(width, height, fps):
    num, den = fps_ratio(fps)
    return f"YUV4MPEG2 W{width} H{height} F{num}:{den} Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n".encode("ascii")


class VisualizationRecorder:
    """Records the view state of `vis` at every frame it produces and replays it as a movie.  `clock` gives the time in seconds
    (inject one to script a path: set the camera, mark(), advance the clock)."""

    # NB the order matters: the quantity and the log switch are set before vmin / vmax, so setting them does not autorange
    # over the recorded range
    _record_properties = ["colormap[type]", "quantity_name", "colormap[log]", "colormap[vmin]", "colormap[vmax]",
                          "colormap[gamma]", "colormap[density_vmin]", "colormap[density_vmax]", "rotation_matrix", "scale",
                          "position_offset"]
    _record_interpolation_class_smoothed = [
        StepInterpolator, StepInterpolator, StepInterpolator, SmoothedStepInterpolator, SmoothedStepInterpolator,
        SmoothedStepInterpolator, SmoothedStepInterpolator, SmoothedStepInterpolator, SmoothedRotationInterpolator,
        SmoothedLinearInterpolator, SmoothedLinearInterpolator]
    _record_interpolation_class_unsmoothed = [
        StepInterpolator, StepInterpolator, StepInterpolator, StepInterpolator, StepInterpolator, StepInterpolator,
        StepInterpolator, StepInterpolator, RotationInterpolator, LinearInterpolator, LinearInterpolator]

    def __init__(self, vis, clock=time.monotonic):
        self._visualizer = vis
        self._clock = clock
        self._recording = False
        self._replaying = False
        self._recording_ends_at = None
        self._t0 = None
        if hasattr(vis, "fov"):
            # a perspective target (topsy_amd.PerspectiveView): its field of view is part of the camera path; a visualizer's
            # timestream keeps the desktop recorder's layout
            self._record_properties = self._record_properties + ["fov"]
            self._record_interpolation_class_smoothed = self._record_interpolation_class_smoothed + [SmoothedLinearInterpolator]
            self._record_interpolation_class_unsmoothed = self._record_interpolation_class_unsmoothed + [LinearInterpolator]
        self._reset_timestream()
        vis.add_frame_listener(self._on_frame)

    # -- recording ----------------------------------------------------------------------------------
    def _sample(self):
        return {p: copy.copy(_get_property(self._visualizer, p)) for p in self._record_properties}

    def _reset_timestream(self):
        self._timestream = {p: [(0.0, v)] for p, v in self._sample().items()}

    def _time_elapsed(self):
        return self._clock() - self._t0

    def _append(self):
        t = self._time_elapsed()
        for p, v in self._sample().items():
            self._timestream[p].append((t, v))

    def _on_frame(self, vis):
        if self._recording and not self._replaying:
            self._append()

    def record(self):
        """Start a new recording: every property is seeded with its current value at time 0."""
        self._t0 = self._clock()
        self._reset_timestream()
        self._recording = True

    def mark(self):
        """Sample the view state now, as a frame would, without drawing one."""
        if not self._recording:
            raise RuntimeError("mark() needs a recording: call record() first")
        self._append()

    def stop(self):
        if self._recording:
            self._recording_ends_at = self._time_elapsed()
        self._recording = False

    @property
    def recording(self):
        return self._recording

    def save_timestream(self, fname):
        """Pickle (timestream, recording_ends_at): the layout topsy's recorder reads and writes."""
        with open(fname, "wb") as f:
            pickle.dump((self._timestream, self._recording_ends_at), f)

    def load_timestream(self, fname):
        with open(fname, "rb") as f:
            self._timestream, self._recording_ends_at = pickle.load(f)

    # -- replay ---------------------------------------------------------------------------------------
    def _progress_iterator(self, ntot):
        """The frame indices 0 .. ntot - 1, with a progress display where one is available (overridden by topsy's Qt GUI)."""
        try:
            import tqdm
        except ImportError:
            return range(ntot)
        return tqdm.tqdm(range(ntot), unit="frame")

    def frames(self, fps=30.0, resolution=(1920, 1080), show_colorbar=True, show_scalebar=True, smooth=True,
               set_vmin_vmax=True, set_quantity=True, pixel_format="rgb24"):
        """Replay the recording: int(recording_ends_at * fps) frames, frame i at t = i / fps, each an EXPORT frame of
        `resolution` = (W, H) with the interpolated state set.  Yields (H, W, 3) uint8 RGB ("rgb24") or the planes Y (H, W),
        U, V (H/2, W/2) ("yuv420p", even W and H).  Stops a recording in progress first."""
        width, height = (int(v) for v in resolution)
        if pixel_format not in ("rgb24", "yuv420p"):
            raise ValueError(f"pixel_format must be 'rgb24' or 'yuv420p', not {pixel_format!r}")
        if pixel_format == "yuv420p" and (width % 2 or height % 2):
            raise ValueError(f"yuv420p needs an even width and height, not {width} x {height}")
        if getattr(self._visualizer, "canvas_format", "rgba8unorm") != "rgba8unorm":
            raise ValueError("movie frames are 8-bit: the rgb-hdr canvas cannot be replayed into a movie")
        self.stop()
        if self._recording_ends_at is None:
            raise RuntimeError("nothing to replay: record() and stop() first, or load_timestream()")
        return self._replay(float(fps), (width, height), show_colorbar, show_scalebar, smooth, set_vmin_vmax, set_quantity,
                            pixel_format)

    def _replay(self, fps, resolution, show_colorbar, show_scalebar, smooth, set_vmin_vmax, set_quantity, pixel_format):
        vis = self._visualizer
        exclude = set()
        if not set_vmin_vmax:
            exclude |= {"colormap[vmin]", "colormap[vmax]"}
        if not set_quantity:
            exclude.add("quantity_name")
        classes = self._record_interpolation_class_smoothed if smooth else self._record_interpolation_class_unsmoothed
        # (a timestream recorded without fov -- on a visualizer, or before the perspective view existed -- leaves it alone)
        interpolators = {p: c(self._timestream[p]) for c, p in zip(classes, self._record_properties)
                         if p not in exclude and p in self._timestream}
        layers_before = (vis.show_colorbar, vis.show_scalebar)
        self._replaying = True
        try:
            vis.show_colorbar, vis.show_scalebar = show_colorbar, show_scalebar
            for i in self._progress_iterator(int(self._recording_ends_at * fps)):
                t = i / fps
                for p in self._record_properties:
                    if p in interpolators:
                        value = interpolators[p](t)
                        if value is not Interpolator.no_value:
                            _set_property(vis, p, value)
                vis.display_status(STATUS_TEXT, timeout=1e6)
                if pixel_format == "yuv420p":
                    yield vis.get_presentation_image_yuv420(resolution)
                else:
                    yield vis.get_presentation_image(resolution)[..., :3].copy()
        finally:
            self._replaying = False
            vis.show_colorbar, vis.show_scalebar = layers_before
            vis.display_status("Complete", timeout=1.0)

    # -- movie files ----------------------------------------------------------------------------------
    def _y4m_chunks(self, fps, resolution, **replay_kwargs):
        """frames(pixel_format="yuv420p") as y4m bytes: the header, then b"FRAME\n", Y, U, V per frame.  Called eagerly, so a
        refused replay raises before any file or process is touched."""
        replay_kwargs["pixel_format"] = "yuv420p"
        planes = self.frames(fps, resolution, **replay_kwargs)
        header = y4m_header(int(resolution[0]), int(resolution[1]), fps)

        def chunks():
            yield header
            for y, u, v in planes:
                yield b"FRAME\n"
                yield y.data
                yield u.data
                yield v.data
        return chunks()

    def save_y4m(self, filename, fps, resolution, **replay_kwargs):
        """Write the replay as YUV4MPEG2 (raw 4:2:0, BT.709 limited range), which every encoder reads."""
        chunks = self._y4m_chunks(fps, resolution, **replay_kwargs)
        with open(filename, "wb") as f:
            for c in chunks:
                f.write(c)

    _REPLAY_ARGS = ("show_colorbar", "show_scalebar", "smooth", "set_vmin_vmax", "set_quantity")

    def save_mp4(self, filename, fps, resolution, *args, ffmpeg="ffmpeg", **kwargs):
        """Encode the replay with an ffmpeg executable (`ffmpeg`: its name or path), run as a child process that reads the y4m
        stream on its standard input; tagged BT.709, limited (tv) range.  *args, **kwargs: frames()'s show_colorbar,
        show_scalebar, smooth, set_vmin_vmax and set_quantity."""
        if len(args) > len(self._REPLAY_ARGS):
            raise TypeError(f"save_mp4 takes at most {len(self._REPLAY_ARGS)} replay arguments after resolution")
        kwargs.update(zip(self._REPLAY_ARGS, args))
        exe = shutil.which(ffmpeg)
        if exe is None:
            raise RuntimeError(f"no ffmpeg executable {ffmpeg!r} found: write the movie with save_y4m() and encode it elsewhere")
        chunks = self._y4m_chunks(fps, resolution, **kwargs)
        cmd = [exe, "-y", "-loglevel", "error", "-f", "yuv4mpegpipe", "-i", "-", "-pix_fmt", "yuv420p",
               "-colorspace", "bt709", "-color_primaries", "bt709", "-color_trc", "bt709", "-color_range", "tv", str(filename)]
        with tempfile.TemporaryFile() as err:
            proc = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.DEVNULL, stderr=err)
            try:
                for c in chunks:
                    proc.stdin.write(c)
                proc.stdin.close()
            except BrokenPipeError:
                pass                # ffmpeg stopped reading: its exit status and message say why
            except BaseException:
                proc.kill()
                proc.wait()
                raise
            finally:
                chunks.close()      # ends the replay (restores the layer switches) if ffmpeg stopped early
                try:
                    proc.stdin.close()
                except BrokenPipeError:
                    pass
            rc = proc.wait()
            if rc != 0:
                err.seek(0)
                message = err.read().decode(errors="replace").strip()
                raise RuntimeError(f"ffmpeg exited with status {rc}: {message}")
