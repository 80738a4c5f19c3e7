"""Fixed-order fp64 restatement of the map-point creation's host composition
and per-match arithmetic (sfm_amd/csrc/mappoint_kernels.hip): what
sfm_matcher_pair_points, sfm_matcher_refind_points and sfm_filter_matches must
reproduce bit for bit.

The filter is GeometryUtils::calculateFundamentalMatrix + filterMatches as
read from the call site (CSfM.cpp:164-165; sfm_amd.live._filter_matches);
GeometryUtils is absent from the reference tree, so this is the project's
reading (parity with it unpinned).

Association order (every operation is one IEEE fp64 operation, nothing fused;
no `@`, no np.linalg, no hypot):
  * every 3-term sum is (a b + c d) + e f; a fourth term is added last;
  * P = K [R|t]:      P[i][j] = (K[i][0] M[0][j] + K[i][1] M[1][j]) + K[i][2] M[2][j]
  * R = R1 R0^T:      R[i][j] = (R1[i][0] R0[j][0] + R1[i][1] R0[j][1]) + R1[i][2] R0[j][2]
  * t = t1 - R t0:    t[i] = t1[i] - ((R[i][0] t0[0] + R[i][1] t0[1]) + R[i][2] t0[2])
  * E = [t]x R written out: E[0][j] = t1 R[2][j] - t2 R[1][j],
    E[1][j] = t2 R[0][j] - t0 R[2][j], E[2][j] = t0 R[1][j] - t1 R[0][j]
  * K^-1 of the upper-triangular K (fx, s, cx; fy, cy; 1) in closed form:
    [[1/fx, -s/(fx fy), (s cy - cx fy)/(fx fy)], [0, 1/fy, -cy/fy], [0, 0, 1]]
  * F = (K1^-T E) K0^-1, both products in the 3-term order, the first one
    A[i][j] = (K1i[0][i] E[0][j] + K1i[1][i] E[1][j]) + K1i[2][i] E[2][j]
  * lines l1 = F h0, l0 = F^T h1 with h = (u, v, 1): (F.0 u + F.1 v) + F.2
  * d = |(lx u + ly v) + lz| / sqrt(lx lx + ly ly)
  * depth z_i = ((R_i[2][0] x + R_i[2][1] y) + R_i[2][2] z) + t_i[2]
  * project: c_i = ((r_i0 x + r_i1 y) + r_i2 z) + t_i, u = (c0 / c2) fx + cx
"""
import numpy as np


def _f(a, shape):
    return np.asarray(a, np.float64).reshape(shape)


def _dot3(a, b, c, d, e, f):
    return (a * b + c * d) + e * f


def inv_K(K):
    K = _f(K, (3, 3))
    fx, s, cx, fy, cy = K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2]
    one = np.float64(1.0)
    Ki = np.zeros((3, 3))
    Ki[0, 0] = one / fx
    Ki[0, 1] = -s / (fx * fy)
    Ki[0, 2] = (s * cy - cx * fy) / (fx * fy)
    Ki[1, 1] = one / fy
    Ki[1, 2] = -cy / fy
    Ki[2, 2] = one
    return Ki


def compose_P(K, R, t):
    K, R, t = _f(K, (3, 3)), _f(R, (3, 3)), _f(t, 3)
    M = np.zeros((3, 4))
    M[:, :3] = R
    M[:, 3] = t
    P = np.zeros((3, 4))
    for i in range(3):
        for j in range(4):
            P[i, j] = _dot3(K[i, 0], M[0, j], K[i, 1], M[1, j], K[i, 2], M[2, j])
    return P


def fundamental_from_poses(K0, R0, t0, K1, R1, t1):
    R0, R1, t0, t1 = _f(R0, (3, 3)), _f(R1, (3, 3)), _f(t0, 3), _f(t1, 3)
    R = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            R[i, j] = _dot3(R1[i, 0], R0[j, 0], R1[i, 1], R0[j, 1], R1[i, 2], R0[j, 2])
    t = np.zeros(3)
    for i in range(3):
        t[i] = t1[i] - _dot3(R[i, 0], t0[0], R[i, 1], t0[1], R[i, 2], t0[2])
    E = np.zeros((3, 3))
    for j in range(3):
        E[0, j] = t[1] * R[2, j] - t[2] * R[1, j]
        E[1, j] = t[2] * R[0, j] - t[0] * R[2, j]
        E[2, j] = t[0] * R[1, j] - t[1] * R[0, j]
    K0i, K1i = inv_K(K0), inv_K(K1)
    A = np.zeros((3, 3))
    F = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            A[i, j] = _dot3(K1i[0, i], E[0, j], K1i[1, i], E[1, j], K1i[2, i], E[2, j])
    for i in range(3):
        for j in range(3):
            F[i, j] = _dot3(A[i, 0], K0i[0, j], A[i, 1], K0i[1, j], A[i, 2], K0i[2, j])
    return F


def epipolar_distances(F, uv0, uv1):
    """(d0, d1): keypoint 0 to the line of keypoint 1 in image 0, and the
    other way round.  0 / 0 (F = 0) is NaN, as on the device."""
    F = _f(F, (3, 3))
    uv0, uv1 = _f(uv0, (-1, 2)), _f(uv1, (-1, 2))
    u0, v0, u1, v1 = uv0[:, 0], uv0[:, 1], uv1[:, 0], uv1[:, 1]
    l1 = [(F[i, 0] * u0 + F[i, 1] * v0) + F[i, 2] for i in range(3)]
    l0 = [(F[0, j] * u1 + F[1, j] * v1) + F[2, j] for j in range(3)]
    with np.errstate(invalid="ignore", divide="ignore"):
        d1 = np.abs((l1[0] * u1 + l1[1] * v1) + l1[2]) / np.sqrt(l1[0] * l1[0] + l1[1] * l1[1])
        d0 = np.abs((l0[0] * u0 + l0[1] * v0) + l0[2]) / np.sqrt(l0[0] * l0[0] + l0[1] * l0[1])
    return d0, d1


def depth(R, t, X):
    R, t, X = _f(R, (3, 3)), _f(t, 3), _f(X, (-1, 3))
    with np.errstate(invalid="ignore", over="ignore"):
        return _dot3(R[2, 0], X[:, 0], R[2, 1], X[:, 1], R[2, 2], X[:, 2]) + t[2]


def filter_matches(uv0, uv1, X, K0, R0, t0, K1, R1, t1, max_err, parts=False):
    """bool [n]; parts=True: (keep, dict of the five rules' own verdicts and
    the distances)."""
    X = _f(X, (-1, 3))
    F = fundamental_from_poses(K0, R0, t0, K1, R1, t1)
    d0, d1 = epipolar_distances(F, uv0, uv1)
    z0, z1 = depth(R0, t0, X), depth(R1, t1, X)
    fin = np.isfinite(X).all(1)
    with np.errstate(invalid="ignore"):
        rules = {"finite": fin, "z0": z0 > 0, "z1": z1 > 0, "d0": d0 <= max_err, "d1": d1 <= max_err}
    keep = rules["finite"] & rules["z0"] & rules["z1"] & rules["d0"] & rules["d1"]
    if parts:
        return keep, dict(rules, dist0=d0, dist1=d1, depth0=z0, depth1=z1, F=F)
    return keep


def project(K, R, t, X):
    K, R, t, X = _f(K, (3, 3)), _f(R, (3, 3)), _f(t, 3), _f(X, (-1, 3))
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        c = [_dot3(R[i, 0], x, R[i, 1], y, R[i, 2], z) + t[i] for i in range(3)]
        return np.column_stack([(c[0] / c[2]) * K[0, 0] + K[0, 2], (c[1] / c[2]) * K[1, 1] + K[1, 2]])
