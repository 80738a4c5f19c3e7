"""Camera front end (sfm_camera_*, sfm_undistort_points, sfm_rgb_to_grey,
sfm_frame_detect of include/sfm_amd.h).

The reference is constructed as CSfM(K, imSize, d); every frame passes
CFrame::setFrame (cvtColor(.., CV_RGB2GRAY), /root/reference/CFrame.cpp:
156-164) and CFrame::setKeyPoints (undistortPoints(_pts_dist, _pts, _K, _d,
_Kopt), CFrame.cpp:203-227), and everything downstream works in the
undistorted image of _Kopt = getOptimalNewCameraMatrix(_K, _d, _imSize, 0)
(CFrame.cpp:33).  OpenCV's arithmetic is restated (tests/camera_ref.py),
parity with OpenCV unpinned.  Opt-in: nothing here is applied
unless a Camera is given -- Kopt != K even for d = 0.  No CPU fallback: the
per-frame work goes through libsfm_amd.so; only the forward lens model
(distort, used by synthetic streams; the reference never distorts) is numpy.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._ffi import CameraStruct, check, lib, ptr
from .brisk import DESC_BYTES


class Camera:
    """K (3x3), distortion d (0, 4, 5 or 8 of k1 k2 p1 p2 k3 k4 k5 k6) and
    the image size (width, height); .Kopt is the new camera matrix."""

    def __init__(self, K, d, size):
        K9 = np.ascontiguousarray(np.asarray(K, np.float64).reshape(9))
        dd = np.ascontiguousarray(np.asarray(d if d is not None else [], np.float64).reshape(-1))
        self._c = CameraStruct()
        check(lib().sfm_camera_init(ctypes.byref(self._c), ptr(K9), ptr(dd) if dd.size else None, int(dd.size),
                                    int(size[0]), int(size[1])), "sfm_camera_init")
        self.K = K9.reshape(3, 3).copy()
        self.d = dd.copy()
        self.width, self.height = int(size[0]), int(size[1])
        self.Kopt = np.array(self._c.Kopt9, np.float64).reshape(3, 3)

    def undistort(self, pts, device: int = 0) -> np.ndarray:
        """cv::undistortPoints(pts, K, d, P = Kopt) on the device: [n][2]."""
        p = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 2)
        out = np.zeros_like(p)
        check(lib().sfm_undistort_points(device, ctypes.byref(self._c), p.shape[0], ptr(p), ptr(out)),
              "sfm_undistort_points")
        return out

    def distort(self, pts) -> np.ndarray:
        """Forward lens model (host numpy): pixels of the Kopt image -> pixels
        of K's image; the inverse of undistort up to its five iterations."""
        p = np.asarray(pts, np.float64).reshape(-1, 2)
        k = np.zeros(8)
        k[:self.d.size] = self.d
        k1, k2, p1, p2, k3, k4, k5, k6 = k
        x = (p[:, 0] - self.Kopt[0, 2]) / self.Kopt[0, 0]
        y = (p[:, 1] - self.Kopt[1, 2]) / self.Kopt[1, 1]
        r2 = x * x + y * y
        cd = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
        xd = x * cd + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        yd = y * cd + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        return np.stack([xd * self.K[0, 0] + self.K[0, 2], yd * self.K[1, 1] + self.K[1, 2]], axis=1)


def rgb_to_grey(img, device: int = 0) -> np.ndarray:
    """cvtColor(img, CV_RGB2GRAY) on the device; img uint8 [h][w][3]."""
    c = np.ascontiguousarray(img, dtype=np.uint8)
    if c.ndim != 3 or c.shape[2] != 3:
        raise ValueError("img must be [h][w][3] uint8")
    h, w = c.shape[:2]
    out = np.zeros((h, w), np.uint8)
    check(lib().sfm_rgb_to_grey(device, ptr(c), w, h, 3 * w, ptr(out)), "sfm_rgb_to_grey")
    return out


class FrameFrontEnd:
    """CTracker::setCurrentFrame + detectFeatures + CFrame::setKeyPoints as
    one device call (sfm_frame_detect).  With a KLTTracker the frame becomes
    its current frame; with a FeatureMatcher the detected frame becomes the
    matcher's current frame without leaving the device."""

    def __init__(self, camera: Camera, matcher=None, klt=None, threshold: int = 60, octaves: int = 6):
        self.camera, self.matcher, self.klt = camera, matcher, klt
        self.threshold, self.octaves = int(threshold), int(octaves)
        self._out = None    # the call's output arrays, kept between frames (no per-frame allocation)

    def _buffers(self, cap: int):
        if self._out is None or len(self._out[1]) != cap:
            self._out = (np.zeros((cap, 5), np.float32), np.zeros(cap, np.int32), np.zeros((cap, DESC_BYTES), np.uint8),
                         np.zeros((cap, 2), np.float64))
        return self._out

    def detect(self, img, capacity: int | None = None):
        """img uint8 [h][w] or [h][w][3] -> (keypoints [n][5] float32, layer
        [n], descriptors uint8 [n][64], undistorted positions [n][2])."""
        im = np.ascontiguousarray(img, dtype=np.uint8)
        cam = self.camera
        if im.shape[:2] != (cam.height, cam.width) or im.ndim not in (2, 3) or (im.ndim == 3 and im.shape[2] != 3):
            raise ValueError(f"frame shape {im.shape} does not match the camera's {(cam.height, cam.width)}")
        ch = 1 if im.ndim == 2 else 3
        cap = max(1024, cam.width * cam.height // 64) if capacity is None else int(capacity)
        mt = self.matcher._h if self.matcher is not None else None
        kl = self.klt._h if self.klt is not None else None
        for _ in range(2):  # the call reports the count before it rejects a short buffer
            kps, lay, desc, pts = self._buffers(max(cap, 1))
            n = ctypes.c_int32()
            rc = lib().sfm_frame_detect(mt, kl, ptr(im), ch, ch * cam.width, ctypes.byref(cam._c), self.threshold,
                                        self.octaves, cap, ptr(kps), ptr(lay), ptr(desc), ptr(pts), ctypes.byref(n))
            if rc == 0 or n.value <= cap or capacity is not None or self.klt is not None:
                break  # (a retry would push the frame into the KLT handle twice)
            cap = n.value
        check(rc, "sfm_frame_detect")
        k = n.value
        if self.matcher is not None:
            self.matcher.n = [self.matcher.n[1], k]
        return kps[:k].copy(), lay[:k].copy(), desc[:k].copy(), pts[:k].copy()


__all__ = ["Camera", "rgb_to_grey", "FrameFrontEnd"]
