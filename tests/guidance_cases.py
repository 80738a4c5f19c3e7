"""Shared inputs of the scan-guidance tests (tests/test_guidance_ref.py on the
CPU, tests/test_gpu_guidance.py on the device)."""
import numpy as np


def clouds():
    """name -> integer points [n][2] in [0, 512): n = 1, 2, 3 collinear, 65,
    1000, and the degenerate shapes."""
    rng = np.random.default_rng(2017)
    disc = np.rint(rng.normal([40.0, 30.0], [6.0, 4.0], (1000, 2))).astype(np.int64)
    out = {
        "one": np.array([[7, 3]]),
        "two": np.array([[9, 2], [3, 11]]),
        "collinear3": np.array([[2, 1], [6, 3], [4, 2]]),
        "n65": rng.integers(0, 64, (65, 2)),
        "n1000": np.clip(disc, 0, 511),
        "duplicates": np.array([[5, 5]] * 4),
        "horizontal": np.stack([np.arange(3, 40, 3), np.full(13, 8)], 1),
        "vertical": np.stack([np.full(9, 12), np.arange(0, 27, 3)], 1),
        "diagonal": np.stack([np.arange(20), 2 * np.arange(20) + 1], 1),
        "square": np.array([[0, 0], [10, 0], [10, 10], [0, 10], [5, 5], [5, 0], [10, 5]]),
        "rectangle": np.array([[x, y] for x in range(10, 24) for y in range(4, 12)]),
        "triangle": np.array([[0, 0], [17, 3], [5, 29]]),
        "wide": rng.integers(0, 512, (300, 2)) // np.array([1, 8]),
    }
    return {k: np.asarray(v, np.int64).reshape(-1, 2) for k, v in out.items()}


def textured_frame(W, H, seed):
    """A random textured colour frame with a saturated blob in the middle."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (H // 4 + 2, W // 4 + 2, 3), dtype=np.uint8)
    img = np.repeat(np.repeat(base, 4, axis=0), 4, axis=1)[:H, :W].astype(np.int64)
    img = np.clip(img // 2 + rng.integers(0, 64, (H, W, 3)), 0, 255).astype(np.uint8)   # muted, noisy
    y, x = np.mgrid[0:H, 0:W]
    blob = ((x - W * 0.5) / (W * 0.22)) ** 2 + ((y - H * 0.5) / (H * 0.25)) ** 2 <= 1.0
    img[blob] = np.clip(np.array([25, 60, 230]) + rng.integers(-12, 13, (int(blob.sum()), 3)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(img)


def camera_for(W, H):
    K = np.array([[0.9 * W, 0.0, 0.5 * W - 0.3], [0.0, 0.9 * W, 0.5 * H + 0.2], [0.0, 0.0, 1.0]])
    a = 0.05
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    t = np.array([0.01, -0.02, 4.0])
    return R, t, K


def point_set(n, W, H, seed):
    """n map points: most in front of the camera over the blob, plus (n >= 65)
    points behind the camera, points outside the frame, and points that round
    onto the last row / column.  n = 3: collinear."""
    R, t, K = camera_for(W, H)
    rng = np.random.default_rng(seed)
    if n == 0:
        return np.zeros((0, 3))

    def lift(uv, z):
        """3D points that project to the pixels uv at depth z."""
        c = np.column_stack([(uv[:, 0] - K[0, 2]) / K[0, 0] * z, (uv[:, 1] - K[1, 2]) / K[1, 1] * z, z])
        return (c - t) @ R          # R^T (c - t)
    uv = np.column_stack([rng.uniform(0.3 * W, 0.7 * W, n), rng.uniform(0.28 * H, 0.72 * H, n)])
    z = rng.uniform(3.0, 5.0, n)
    if n == 3:                                                # collinear, also after the 0.25 scaling
        a, b, s = W // 16, H // 16, max(1, min(W, H) // 32)
        uv = 4.0 * np.array([[a, b], [a + 2 * s, b + 2 * s], [a + s, b + s]])
        z = np.full(3, 4.0)
    if n >= 65:
        z[:5] = -z[:5]                                        # behind the camera
        uv[5:10] = [[-30.0, 5.0], [W + 20.0, 3.0], [4.0, -9.0], [6.0, H + 11.0], [-0.6, 2.0]]   # outside
        uv[10:14] = [[W - 1.0, 0.4 * H], [0.6 * W, H - 1.0], [W - 1.2, H - 0.8], [W - 0.51, 0.3 * H]]  # last row / column
    return lift(uv, z)


def flat_case():
    """A flat two-colour frame whose box can be derived by hand: 128 x 72, the block
    [16:48, 40:96] (edges at multiples of 4, so no resize tap blends); points
    whose small pixels fill x 12..22, y 5..10.  The accepted set is the block's
    small pixels, x 10..23, y 4..11: centre (66, 30), sides {52, 28}."""
    img = np.empty((72, 128, 3), np.uint8)
    img[:] = (200, 60, 30)
    img[16:48, 40:96] = (20, 40, 220)
    K = np.array([[100.0, 0.0, 64.0], [0.0, 100.0, 36.0], [0.0, 0.0, 1.0]])
    xs, ys = np.meshgrid(np.arange(12, 23), np.arange(5, 11))
    u, v = 4.0 * xs.ravel(), 4.0 * ys.ravel()
    X = np.column_stack([(u - 64.0) / 100.0 * 2.0, (v - 36.0) / 100.0 * 2.0, np.full(u.size, 2.0)])
    return img, X, np.eye(3), np.zeros(3), K
