"""Scan guidance (sfm_guidance_* and sfm_min_area_rect of include/sfm_amd.h).

The reference's frame loop ends every RUNNING frame with
CScanGuidance::calculateMask(frame, mapPts, Kopt, P) (CSfM.cpp:80-81,
CScanGuidance.cpp:39-105): the object's centroid and the oriented box around
it, which the caller shows to the person holding the camera.  Here the map
points are read from the device map store, the frame is uploaded once and
one small result comes back; OpenCV's arithmetic is restated
(tests/guidance_ref.py), parity with OpenCV unpinned.  No CPU
fallback: the per-frame work goes through libsfm_amd.so.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from ._ffi import GuidanceOptions, GuidanceResult, check, default_guidance_options, lib, ptr


@dataclass
class GuidanceFrame:
    """One update's result: getCentroid(), getBoundingBox() and the counts."""
    centroid: np.ndarray      # [3] float64; NaN for an empty map
    box_center: np.ndarray    # [2] float32, full-frame pixels
    box_size: np.ndarray      # [2] float32 (width, height)
    box_angle: np.float32     # degrees
    n_points: int
    n_projected: int
    n_hull: int
    n_accepted: int
    area: float               # of the projected points' hull, quarter-size pixels

    @property
    def box(self) -> np.ndarray:
        """cx cy w h angle, float32."""
        return np.array([*self.box_center, *self.box_size, self.box_angle], np.float32)


def min_area_rect(points) -> np.ndarray:
    """cv::minAreaRect of integer points [n][2] (host only) -> float32 cx cy w
    h angle."""
    p = np.ascontiguousarray(points, dtype=np.int32).reshape(-1, 2)
    box = np.zeros(5, np.float32)
    check(lib().sfm_min_area_rect(p.shape[0], ptr(p) if p.size else None, ptr(box)), "sfm_min_area_rect")
    return box


class ScanGuidance:
    """CScanGuidance for frames of width x height.  Options: h_bins, s_bins,
    threshold, alpha, ema (sfm_guidance_options)."""

    def __init__(self, width: int, height: int, device: int = 0, **options):
        o = default_guidance_options()
        for k, v in options.items():
            if k not in ("h_bins", "s_bins", "threshold", "alpha", "ema"):
                raise TypeError(f"unknown guidance option {k!r}")
            setattr(o, k, type(getattr(o, k))(v))
        self.options: GuidanceOptions = o
        self.width, self.height, self.device = int(width), int(height), int(device)
        self.small = (int(self.width * 0.25), int(self.height * 0.25))   # (ws, hs)
        h = ctypes.c_void_p()
        check(lib().sfm_guidance_create(self.device, self.width, self.height, ctypes.byref(o), ctypes.byref(h)),
              "sfm_guidance_create")
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().sfm_guidance_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def update(self, img, R, t, K, map=None, points=None) -> GuidanceFrame:
        """calculateMask(img, points, K, [R|t]); the points are the live points
        of `map` (a DeviceMap, read on the device) or `points` [n][3]."""
        if (map is None) == (points is None):
            raise ValueError("give either map or points")
        im = np.asarray(img)
        if im.dtype != np.uint8 or im.ndim != 3 or im.shape != (self.height, self.width, 3):
            raise ValueError(f"img must be uint8 {(self.height, self.width, 3)}, not {im.dtype} {im.shape}")
        if not (im.strides[2] == 1 and im.strides[1] == 3 and im.strides[0] >= 3 * self.width):
            im = np.ascontiguousarray(im)
        R9 = np.ascontiguousarray(np.asarray(R, np.float64).reshape(9))
        t3 = np.ascontiguousarray(np.asarray(t, np.float64).reshape(3))
        K9 = np.ascontiguousarray(np.asarray(K, np.float64).reshape(9))
        res = GuidanceResult()
        addr = ctypes.c_void_p(im.__array_interface__["data"][0])
        if map is not None:
            check(lib().sfm_guidance_update(self._h, map._h, addr, int(im.strides[0]), ptr(R9), ptr(t3), ptr(K9),
                                            ctypes.byref(res)), "sfm_guidance_update")
        else:
            X = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
            check(lib().sfm_guidance_update_points(self._h, X.shape[0], ptr(X) if X.size else None, addr,
                                                   int(im.strides[0]), ptr(R9), ptr(t3), ptr(K9), ctypes.byref(res)),
                  "sfm_guidance_update_points")
        return GuidanceFrame(np.array(res.centroid, np.float64), np.array(res.box_center, np.float32),
                             np.array(res.box_size, np.float32), np.float32(res.box_angle), int(res.n_points),
                             int(res.n_projected), int(res.n_hull), int(res.n_accepted), float(res.area))

    def planes(self) -> dict:
        """The last update's planes: mask uint8 [hs][ws], bins int16
        [hs][ws][2] (-1 = outside), hist float32 [h_bins][s_bins] (the state
        the back-projection read), bproj float32 [hs][ws], extents int32
        [hs][2] (accepted pixels per row; ws, -1 = empty)."""
        ws, hs = self.small
        out = {"mask": np.zeros((hs, ws), np.uint8), "bins": np.zeros((hs, ws, 2), np.int16),
               "hist": np.zeros((self.options.h_bins, self.options.s_bins), np.float32),
               "bproj": np.zeros((hs, ws), np.float32), "extents": np.zeros((hs, 2), np.int32)}
        check(lib().sfm_guidance_read_planes(self._h, ptr(out["mask"]), ptr(out["bins"]), ptr(out["hist"]),
                                             ptr(out["bproj"]), ptr(out["extents"])), "sfm_guidance_read_planes")
        return out

    def last_time(self) -> np.ndarray:
        """Device time of the last update in ms: upload, kernels, download."""
        ms = np.zeros(3)
        check(lib().sfm_guidance_last_time(self._h, ptr(ms)), "sfm_guidance_last_time")
        return ms


__all__ = ["ScanGuidance", "GuidanceFrame", "min_area_rect"]
