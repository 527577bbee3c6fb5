"""Interpolation of a recorded timestream for movie replay (the behaviour of topsy's recorder/interpolator.py).

A timestream is a list of (time, value) pairs in ascending time.  Calling an interpolator with a time returns the value to
set at that time, or Interpolator.no_value when there is nothing to set.  The files the desktop recorder writes hold these
lists, so the semantics (including where an interpolator answers no_value) are kept exactly.
"""
import math

import numpy as np


class Interpolator:
    """Base class: holds the timestream; subclasses define __call__(t)."""

    no_value = object()     # "leave the property as it is"

    def __init__(self, timestream):
        self._timestream = timestream

    def __call__(self, t):
        raise NotImplementedError


class LinearInterpolator(Interpolator):
    """Linear between the two events around t; the first event's value up to its time; no_value after the last event."""

    def __call__(self, t):
        previous = None
        for t_event, value in self._timestream:
            if t_event >= t:
                if previous is None:
                    return value
                t_prev, v_prev = previous
                return v_prev + (value - v_prev) * (t - t_prev) / (t_event - t_prev)
            previous = (t_event, value)
        return self.no_value


class RotationInterpolator(LinearInterpolator):
    """Linear interpolation of the matrix elements, then the nearest orthogonal matrix (U V^T of the SVD)."""

    def __call__(self, t):
        m = super().__call__(t)
        if m is self.no_value:
            return m
        u, _, vh = np.linalg.svd(m)
        return u @ vh


class _Smoothed:
    """Mixin: resample the timestream at `fps` per second with the parent's rule, convolve every component with a Gaussian of
    standard deviation `smoothing` seconds (the series padded at both ends with its first and last sample), and interpolate the
    smoothed series with the parent's rule.  The kernel is sampled at the integers of [-3 sigma, 3 sigma) in units of
    samples and normalised to a sum of 1."""

    def __init__(self, timestream, smoothing=0.25, fps=30):
        super().__init__(timestream)
        self._smoothing = smoothing
        t_end = timestream[-1][0]
        n = max(1, math.floor(t_end * fps))        # a recording shorter than one sample keeps its first value
        samples = np.array([super(_Smoothed, self).__call__(i / fps) for i in range(n)])
        sigma = smoothing * fps
        kernel = np.exp(-np.arange(-3 * sigma, 3 * sigma) ** 2 / (2 * sigma ** 2))
        kernel /= kernel.sum()
        pad = len(kernel) // 2
        padded = np.concatenate([np.repeat(samples[:1], pad, axis=0), samples, np.repeat(samples[-1:], pad, axis=0)])
        flat = padded.reshape(len(padded), -1)
        smoothed = np.stack([np.convolve(flat[:, k], kernel, mode="valid") for k in range(flat.shape[1])], axis=1)
        smoothed = smoothed.reshape((len(smoothed),) + padded.shape[1:])
        self._timestream = [(i / fps, v) for i, v in enumerate(smoothed)]


class SmoothedLinearInterpolator(_Smoothed, LinearInterpolator):
    pass


class SmoothedRotationInterpolator(_Smoothed, RotationInterpolator):
    pass


class StepInterpolator(Interpolator):
    """The value of the last event at or before t, returned only when it differs from the value returned before; no_value
    otherwise.  Times must not decrease from one call to the next (ValueError)."""

    def __init__(self, timestream):
        super().__init__(timestream)
        self._last_value = self.no_value
        self._last_t = None

    def __call__(self, t):
        if self._last_t is not None and t < self._last_t:
            raise ValueError("a StepInterpolator must be called with times that do not decrease")
        self._last_t = t
        current = next((value for t_event, value in reversed(self._timestream) if t_event <= t), self.no_value)
        if current is self.no_value or current == self._last_value:
            return self.no_value
        self._last_value = current
        return current


class SmoothedStepInterpolator(StepInterpolator):
    """A step from one number to another becomes a linear ramp over `smoothing` seconds, starting at the first call that sees
    the new value (that call still returns the old value).  None and steps from or to None are not ramped: a step to None sets
    nothing, a step from None sets the new value at once."""

    def __init__(self, timestream, smoothing=0.25):
        super().__init__(timestream)
        self._smoothing = smoothing
        self._ramp = None       # (t_start, t_end, start value, target value)

    def __call__(self, t):
        if self._ramp is not None:
            t0, t1, v0, v1 = self._ramp
            if t >= t1:
                self._ramp = None
                return v1
            return v0 + (v1 - v0) * (t - t0) / (t1 - t0)
        before = self._last_value
        new = super().__call__(t)
        if new is self.no_value or new is None or new == before:
            return self.no_value
        if before is self.no_value or before is None:
            return new
        self._ramp = (t, t + self._smoothing, before, new)
        return before
