"""Two-keyframe scenes for the map-point filter (tests/test_map_points_ref.py
on the CPU, tests/test_gpu_map_points.py on the device): matched keypoints of
two poses with detector noise and a share of wrong matches, and matches built
so that exactly one rule of the filter rejects them."""
import numpy as np

from oracle import pnp_oracle
from sfm_amd.mapping import F_PIX, _rodrigues
import map_points_ref as ref

K = np.array([[F_PIX, 0.0, 640.0], [0.0, F_PIX, 360.0], [0.0, 0.0, 1.0]])
MAX_ERR = 7.0
SIZES = (1, 63, 65, 300, 1500)          # one lane, either side of a wave, several blocks
# camera 1 moves 2 units TOWARDS the scene (forward) or away from it: a point
# lies farther from the epipole in the nearer camera's image, so a shift across
# the epipolar line there moves the other image's distance by less
POSES = {"forward": ((0.010, 0.020, 0.005), (0.0, 0.0, 0.0), (0.012, 0.030, -0.004), (0.3, 0.05, 2.0)),
         "backward": ((0.010, 0.020, 0.005), (0.0, 0.0, 0.0), (0.012, 0.030, -0.004), (0.3, 0.05, -2.0)),
         "lateral": ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.004, -0.006, 0.010), (0.6, 0.1, 0.25))}


def pose_pair(name):
    """(rot0, t0, rot1, t1) with x_cam = R X + t; the third entry of POSES is
    the camera centre."""
    r0, c0, r1, c1 = (np.array(v, np.float64) for v in POSES[name])
    return r0, -_rodrigues(r0) @ c0, r1, -_rodrigues(r1) @ c1


def _see(rot, t, L):
    Xc = L @ _rodrigues(rot).T + t
    return Xc[:, :2] / Xc[:, 2:3] * F_PIX + K[:2, 2]


def triangulate(uv0, uv1, r0, t0, r1, t1):
    """oracle.pnp_oracle.triangulate_points on the restatement's K [R|t]."""
    P = np.stack([ref.compose_P(K, _rodrigues(r0), t0), ref.compose_P(K, _rodrigues(r1), t1)])
    n = len(uv0)
    return pnp_oracle.triangulate_points(np.zeros(n, np.int32), np.ones(n, np.int32), uv0, uv1, P)


def scene(n, seed, poses="lateral"):
    """n matches: 0.3 px of noise in both views, 30 % of the view-1 points
    displaced by up to +-40 px; X triangulated from what was seen."""
    rng = np.random.default_rng((seed, n))
    r0, t0, r1, t1 = pose_pair(poses)
    L = np.column_stack([rng.uniform(-3.0, 4.0, n), rng.uniform(-2.0, 2.0, n), rng.uniform(8.0, 14.0, n)])
    uv0 = _see(r0, t0, L) + rng.normal(0.0, 0.3, (n, 2))
    uv1 = _see(r1, t1, L) + rng.normal(0.0, 0.3, (n, 2))
    wrong = rng.random(n) < 0.3
    uv1[wrong] += rng.uniform(-40.0, 40.0, (int(wrong.sum()), 2))
    X = triangulate(uv0, uv1, r0, t0, r1, t1)
    return dict(name=f"{poses}-{n}", uv0=uv0, uv1=uv1, X=X, r0=r0, t0=t0, r1=r1, t1=t1)


def _normal_shift(line, delta):
    """The step of length delta across the line (lx, ly, lz)."""
    nrm = np.array([line[0], line[1]])
    return delta * nrm / np.sqrt(nrm @ nrm)


def constructed():
    """Scenes of noise-free matches of which the named rule alone rejects the
    listed ones: [(scene, {rule: indices})].  The rules are the keys of
    map_points_ref.filter_matches(parts=True)."""
    rng = np.random.default_rng(20170)
    out = []
    for poses, depth_rule, dist_rule in (("forward", "z1", "d1"), ("backward", "z0", "d0")):
        r0, t0, r1, t1 = pose_pair(poses)
        R0, R1 = _rodrigues(r0), _rodrigues(r1)
        n = 8
        L = np.column_stack([rng.uniform(-3.0, 4.0, n), rng.uniform(-2.0, 2.0, n), rng.uniform(8.0, 14.0, n)])
        uv0, uv1 = _see(r0, t0, L), _see(r1, t1, L)
        X = L.copy()
        F = ref.fundamental_from_poses(K, R0, t0, K, R1, t1)
        want = {}
        # 0, 1: behind one camera only (the cameras are 2 units apart along
        # their axes: a point 1 unit in front of the rear one)
        for i in (0, 1):
            zc = np.array([0.2 * i, 0.1, 1.0])                      # in the rear camera's frame
            X[i] = R0.T @ (zc - t0) if poses == "forward" else R1.T @ (zc - t1)
        want[depth_rule] = [0, 1]
        # 2, 3: 7.01 px across the epipolar line in the nearer camera's image
        # (over the bound there alone); 4, 5: 6.99 px (kept)
        for i, delta in ((2, 7.01), (3, -7.01), (4, 6.99), (5, -6.99)):
            if dist_rule == "d1":
                uv1[i] += _normal_shift(F @ np.array([uv0[i, 0], uv0[i, 1], 1.0]), delta)
            else:
                uv0[i] += _normal_shift(F.T @ np.array([uv1[i, 0], uv1[i, 1], 1.0]), delta)
        want[dist_rule] = [2, 3]
        # 6: X not finite, yet with +inf depth in both keyframes (R[2][0] < 0
        # in both); 7: untouched
        assert R0[2, 0] < 0 and R1[2, 0] < 0
        X[6, 0] = -np.inf
        want["finite"] = [6]
        out.append((dict(name=f"constructed-{poses}", uv0=uv0, uv1=uv1, X=X, r0=r0, t0=t0, r1=r1, t1=t1), want))
    return out


def all_scenes(seed=3):
    return [scene(n, seed, p) for n in SIZES for p in ("lateral", "forward")] + [s for s, _ in constructed()]
