"""numpy restatement of the camera front end's arithmetic: OpenCV 3.0's
cvtColor(CV_RGB2GRAY, 8-bit), undistortPoints and getOptimalNewCameraMatrix
(alpha = 0, default newImgSize, no centred principal point) as the project
restates them -- OpenCV itself is not available, parity with it is unpinned
(DESIGN.md).  Every expression keeps the operation order of the
specification; the library is compared with this bit for bit.
"""
from __future__ import annotations

import numpy as np

# the iPhone 6s of the reference's only driver (main/main.cpp:47-52)
K_MAIN = np.array([[1072.606693272117800, 0.0, 648.780750477178910],
                   [0.0, 1067.197515608619600, 364.503435962496890],
                   [0.0, 0.0, 1.0]])

LENSES = {
    "L1": (0.039530469484242, -0.149827721353905, -0.000091102042149, 0.001209830654934),
    "L2": (0.12, 0.03, -0.0004, 0.0006),
    "L3": (-0.28, 0.07, 0.0005, -0.0003, 0.0),
    "L4": (-0.21, 0.05, 0.0003, -0.0002, 0.01, 0.02, -0.01, 0.004),
}
SIZES = [(1280, 720), (96, 64)]


def k_for(size):
    """main.cpp's K scaled to an image size (the principal point inside it)."""
    W, H = size
    K = K_MAIN.copy()
    K[0] *= W / 1280.0
    K[1] *= H / 720.0
    return K


def coeffs(d):
    d = np.asarray(d if d is not None else [], np.float64).reshape(-1)
    if d.size not in (0, 4, 5, 8):
        raise ValueError("n_d must be 0, 4, 5 or 8")
    k = np.zeros(8)
    k[:d.size] = d
    return k


def rgb_to_grey(img):
    c = np.asarray(img, np.uint8).astype(np.int64)
    return ((c[..., 0] * 4899 + c[..., 1] * 9617 + c[..., 2] * 1868 + 8192) >> 14).astype(np.uint8)


def undistort_normalised(pts, K, d, iters=5):
    k1, k2, p1, p2, k3, k4, k5, k6 = (np.float64(v) for v in coeffs(d))
    K = np.asarray(K, np.float64).reshape(3, 3)
    p = np.asarray(pts, np.float64).reshape(-1, 2)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    x0 = (p[:, 0] - cx) / fx
    y0 = (p[:, 1] - cy) / fy
    x, y = x0.copy(), y0.copy()
    for _ in range(iters):
        r2 = x * x + y * y
        icd = (1 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x = (x0 - dx) * icd
        y = (y0 - dy) * icd
    return np.stack([x, y], axis=1)


def undistort_points(pts, K, d, P, iters=5):
    """cv::undistortPoints(src, dst, K, d, P)."""
    P = np.asarray(P, np.float64).reshape(3, 3)
    n = undistort_normalised(pts, K, d, iters)
    return np.stack([n[:, 0] * P[0, 0] + P[0, 2], n[:, 1] * P[1, 1] + P[1, 2]], axis=1)


def distort_points(pts, P, d, K):
    """The forward lens model: pixels of P's (undistorted) image -> pixels of
    K's image.  The inverse of undistort_points up to its fixed iterations."""
    k1, k2, p1, p2, k3, k4, k5, k6 = coeffs(d)
    P = np.asarray(P, np.float64).reshape(3, 3)
    K = np.asarray(K, np.float64).reshape(3, 3)
    p = np.asarray(pts, np.float64).reshape(-1, 2)
    x = (p[:, 0] - P[0, 2]) / P[0, 0]
    y = (p[:, 1] - P[1, 2]) / P[1, 1]
    r2 = x * x + y * y
    cd = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
    xd = x * cd + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * cd + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return np.stack([xd * K[0, 0] + K[0, 2], yd * K[1, 1] + K[1, 2]], axis=1)


def optimal_new_camera_matrix(K, d, size):
    """getOptimalNewCameraMatrix(K, d, (W, H), alpha = 0)."""
    W, H = int(size[0]), int(size[1])
    f32 = np.float32
    i = np.arange(9)
    gx = (i.astype(f32) * f32(W) / f32(8)).astype(f32)
    gy = (i.astype(f32) * f32(H) / f32(8)).astype(f32)
    grid = np.stack(np.meshgrid(gx, gy, indexing="xy"), axis=-1).astype(np.float64)  # [j][i]
    n = undistort_normalised(grid.reshape(-1, 2), K, d).astype(f32).reshape(9, 9, 2)
    X0 = n[:, 0, 0].max()
    X1 = n[:, 8, 0].min()
    Y0 = n[0, :, 1].max()
    Y1 = n[8, :, 1].min()
    rw = f32(X1 - X0)
    rh = f32(Y1 - Y0)
    fx = np.float64(W - 1) / np.float64(rw)
    fy = np.float64(H - 1) / np.float64(rh)
    Kopt = np.eye(3)
    Kopt[0, 0] = fx
    Kopt[1, 1] = fy
    Kopt[0, 2] = -fx * np.float64(X0)
    Kopt[1, 2] = -fy * np.float64(Y0)
    return Kopt
