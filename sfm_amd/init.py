"""Two-view map initialisation: steps 2-5 of CSfM::init
(CSfM.cpp:842-946) -- findHomography, findFundamentalMat(RANSAC), the two
model scores and the choice between them, the decomposition into R, t,
triangulation and the final filter -- on the device through the C ABI
(sfm_two_view_init; init_kernels.hip).  The semantics are the build's
restatement (tests/two_view_ref.py): parity with OpenCV's findFundamentalMat /
findHomography and with GeometryUtils is unpinned.  No CPU fallback.
"""
from __future__ import annotations

import ctypes
from ctypes import c_double, c_int32
from dataclasses import dataclass

import numpy as np

from ._ffi import check, default_two_view_options, lib, ptr

NONE, HOMOGRAPHY, FUNDAMENTAL = 0, 1, 2


@dataclass
class TwoViewResult:
    model: int            # 0 = no initialisation, 1 = homography, 2 = fundamental
    H: np.ndarray         # [3][3] (float32 values)
    F: np.ndarray         # [3][3] (float32 values)
    f_mask: np.ndarray    # uint8 [n]: the RANSAC inliers of F
    scores: np.ndarray    # (s_h, s_f)
    avg_err: float        # errHomo / errFund of the chosen branch
    R: np.ndarray         # [3][3]: second camera x = R X + t (the first is the origin)
    t: np.ndarray         # [3], |t| = 1
    keep: np.ndarray      # uint8 [n]: matches that survive the model's mask and the final filter
    X: np.ndarray         # [n][3] triangulated points, valid where keep
    n_kept: int

    @property
    def ok(self) -> bool:
        return self.model != NONE


def two_view_init(pts0, pts1, K0, K1=None, device: int = 0, **options) -> TwoViewResult:
    """pts0 / pts1 [n][2]: matched pixels of the first keyframe and of the
    current frame; K0 / K1 their intrinsics (K1 = K0 when omitted).  Keyword
    options are the fields of sfm_two_view_options (defaults: the
    reference's constants)."""
    p0 = np.ascontiguousarray(np.asarray(pts0, np.float32).reshape(-1, 2))
    p1 = np.ascontiguousarray(np.asarray(pts1, np.float32).reshape(-1, 2))
    if p0.shape[0] != p1.shape[0]:
        raise ValueError(f"{p0.shape[0]} points in the first view but {p1.shape[0]} in the second")
    k0 = np.ascontiguousarray(np.asarray(K0, np.float64).reshape(9))
    k1 = k0 if K1 is None else np.ascontiguousarray(np.asarray(K1, np.float64).reshape(9))
    o = default_two_view_options()
    for name, value in options.items():
        if name not in dict(o._fields_):
            raise TypeError(f"unknown option {name!r}")
        setattr(o, name, value)
    n = int(p0.shape[0])
    H, F, R, t, scores = np.zeros((3, 3)), np.zeros((3, 3)), np.zeros((3, 3)), np.zeros(3), np.zeros(2)
    f_mask, keep, X = np.zeros(max(1, n), np.uint8), np.zeros(max(1, n), np.uint8), np.zeros((max(1, n), 3))
    model, n_kept, avg = c_int32(0), c_int32(0), c_double(0.0)
    check(lib().sfm_two_view_init(device, n, ptr(p0), ptr(p1), ptr(k0), ptr(k1), ctypes.byref(o),
                                  ctypes.byref(model), ptr(H), ptr(F), ptr(f_mask), ptr(scores), ctypes.byref(avg),
                                  ptr(R), ptr(t), ptr(keep), ptr(X), ctypes.byref(n_kept)), "sfm_two_view_init")
    return TwoViewResult(int(model.value), H, F, f_mask[:n], scores, float(avg.value), R, t, keep[:n], X[:n],
                         int(n_kept.value))
