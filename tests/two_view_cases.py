"""Seeded two-view scenes for the map initialisation tests (1280x720, the
reference's focal length): 3D points seen from the origin and from a second
pose, float32 observations, Gaussian pixel noise and a share of matches
replaced by uniform random points.  The seeds are chosen (on the CPU, by
tests/test_two_view_ref.py's stability conditions) so that no decision of
the pipeline sits on a threshold."""
import numpy as np

from sfm_amd.mapping import F_PIX

W, H = 1280, 720
K = np.array([[F_PIX, 0.0, 640.0], [0.0, F_PIX, 360.0], [0.0, 0.0, 1.0]])


PLANE_N = np.array([0.0, 0.0, 1.0])  # the planar cases: the plane z = 10
PLANE_D = 10.0


def _rot(r):
    th = float(np.linalg.norm(r))
    if th == 0:
        return np.eye(3)
    k = np.asarray(r, float) / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


# name -> (n, seed, kind, noise sigma, outlier share, options of the call)
CASES = {
    # min_good's default (50) exceeds n: lowered so that the smallest RANSAC input still initialises
    "n15": (15, 25, "general", 0.0, 0.0, dict(min_good=10)),
    "n65": (65, 44, "general", 0.3, 0.0, {}),
    "n257_out30": (257, 75, "general", 0.5, 0.3, {}),
    "n600_out60": (600, 248, "general", 0.5, 0.6, {}),
    "planar_exact": (300, 30, "planar", 0.0, 0.0, {}),
    "planar_noisy": (300, 194, "planar", 0.3, 0.0, {}),
    "rotation_only": (300, 4, "rotation", 0.3, 0.0, {}),
}
GENERAL = ["n15", "n65", "n257_out30", "n600_out60"]
PLANAR = ["planar_exact", "planar_noisy"]


def scene(name):
    """-> dict(p0, p1 float32 [n][2], X [n][3], R, t (camera 1: x = R X + t),
    outlier bool [n], opts, plane (n, d) or None)."""
    n, seed, kind, noise, outl, opts = CASES[name]
    rng = np.random.default_rng(1000 + seed)
    uv = np.stack([rng.uniform(60, W - 60, n), rng.uniform(60, H - 60, n)], 1)
    rays = np.concatenate([(uv - K[:2, 2]) / F_PIX, np.ones((n, 1))], 1)
    depth = PLANE_D / (rays @ PLANE_N) if kind == "planar" else rng.uniform(8.0, 14.0, n)
    X = rays * depth[:, None]
    R = _rot(np.array([0.02, -0.03, 0.015]))
    # (planar: a motion towards the plane, so that cheirality resolves the twofold ambiguity of the
    # homography decomposition below the vote's ambiguity ratio)
    t = {"rotation": np.zeros(3), "planar": np.array([-0.6, 0.1, -0.1])}.get(kind, np.array([-0.6, 0.1, 0.15]))
    Xc = X @ R.T + t
    p0 = X[:, :2] / X[:, 2:3] * F_PIX + K[:2, 2]
    p1 = Xc[:, :2] / Xc[:, 2:3] * F_PIX + K[:2, 2]
    if noise > 0:
        p0 = p0 + rng.normal(0, noise, p0.shape)
        p1 = p1 + rng.normal(0, noise, p1.shape)
    outlier = np.zeros(n, bool)
    if outl > 0:
        idx = rng.choice(n, int(round(outl * n)), replace=False)
        outlier[idx] = True
        p1[idx] = np.stack([rng.uniform(0, W, len(idx)), rng.uniform(0, H, len(idx))], 1)
    plane = (PLANE_N, PLANE_D) if kind == "planar" else None
    return dict(p0=p0.astype(np.float32), p1=p1.astype(np.float32), X=X, R=R, t=t, outlier=outlier, opts=dict(opts),
                plane=plane)


_REF = {}


def reference(name, **extra):
    """The CPU restatement's result for a case, computed once and shared."""
    from tests import two_view_ref as T
    key = (name, tuple(sorted(extra.items())))
    if key not in _REF:
        s = scene(name)
        o = dict(s["opts"])
        o.update(extra)
        tr = {}
        _REF[key] = (T.two_view_init(s["p0"], s["p1"], K, K, trace=tr, **o), tr)
    return _REF[key]
