"""CPU restatement (numpy + LAPACK) of the two-view map initialisation of
CSfM::init (CSfM.cpp:823-946): findFundamentalMat(FM_RANSAC, 3.84, 0.99),
findHomography(method 0, 5.99), the two model scores (CSfM.cpp:415-469), the
model choice, the decomposition into R, t with a cheirality vote,
triangulation and the final filter.  Test infrastructure only: the product
(sfm_amd/csrc/init_kernels.hip, sfm_two_view_init) computes the same on the
device.

OpenCV 3.0 and GeometryUtils are absent, so this restates the published
OpenCV 3.0 sources (fundam.cpp run7Point / FMEstimatorCallback /
HomographyEstimatorCallback / HomographyRefineCallback, ptsetreg.cpp,
levmarq.cpp) and ORB-SLAM's initialiser for the decompositions, as the build
reads them -- PARITY UNPINNED against OpenCV and GeometryUtils themselves.
cv::RNG, getSubset and RANSACUpdateNumIters come from oracle/pnp_oracle.py.

Everything after the two estimators runs in fp64 on the float32-rounded H
and F (the reference's float arithmetic there sits in GeometryUtils).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

from oracle.pnp_oracle import CvRNG, get_subset, ransac_update_num_iters

DBL_EPS = np.finfo(float).eps
DBL_MIN = np.finfo(float).tiny
FLT_EPS = float(np.finfo(np.float32).eps)

DEFAULTS = dict(f_ransac_threshold=3.84, f_confidence=0.99, f_max_iters=1000, h_score_th=5.99, h_score_gamma=5.99,
                f_score_th=3.84, f_score_gamma=5.99, h_ratio=0.45, max_repr_err=7.0, min_good_fraction=0.9,
                ambiguity_ratio=0.7, min_parallax_deg=1.0, min_good=50)
MIN_POINTS = 15  # below it OpenCV switches to LMedS (not restated): model = 0


# ---- findFundamentalMat(FM_RANSAC) -----------------------------------------
def solve_cubic(a0, a1, a2, a3):
    """cv::solveCubic (3.0) for a0 x^3 + a1 x^2 + a2 x + a3 -> real roots."""
    if a0 == 0:
        if a1 == 0:
            return [] if a2 == 0 else [-a3 / a2]
        d = a2 * a2 - 4 * a1 * a3
        if d < 0:
            return []
        d = math.sqrt(d)
        q1, q2 = (-a2 + d) * 0.5, (a2 + d) * -0.5
        if abs(q1) > abs(q2):
            r = [q1 / a1, a3 / q1]
        else:
            r = [q2 / a1, a3 / q2]
        return r if d > 0 else r[:1]
    a0 = 1.0 / a0
    a1 *= a0
    a2 *= a0
    a3 *= a0
    Q = (a1 * a1 - 3 * a2) * (1.0 / 9)
    R = (2 * a1 * a1 * a1 - 9 * a1 * a2 + 27 * a3) * (1.0 / 54)
    Qc = Q * Q * Q
    d = Qc - R * R
    if d >= 0:
        theta = math.acos(min(1.0, max(-1.0, R / math.sqrt(Qc)))) if Qc > 0 else 0.0
        sq = math.sqrt(Q)
        t0, t1, t2 = -2 * sq, theta * (1.0 / 3), a1 * (1.0 / 3)
        return [t0 * math.cos(t1) - t2, t0 * math.cos(t1 + 2.0 * math.pi / 3) - t2,
                t0 * math.cos(t1 + 4.0 * math.pi / 3) - t2]
    d = math.sqrt(-d)
    e = math.pow(d + abs(R), 1.0 / 3)
    if R > 0:
        e = -e
    return [(e + Q / e) - a1 * (1.0 / 3)]


def _det3(M):
    return (M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
            M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]))


def null_space_7x9(rows):
    """The two right singular vectors cv::SVD(FULL_UV) adds to the seven of a
    7x9 system (JacobiSVDImpl_): cv::RNG(0x12345678) vectors of +-1/9,
    orthogonalised twice against the rows before them, normalised.  They
    depend on the row space alone, not on the basis the SVD found for it."""
    U = [np.asarray(r, np.float64) for r in rows]
    rng = CvRNG(0x12345678)
    eps = DBL_EPS * 10
    for i in range(7, 9):
        sd, ii = 0.0, 0
        while ii < 100 and sd <= DBL_MIN:
            v = np.array([1.0 / 9 if (rng.next() & 256) != 0 else -1.0 / 9 for _ in range(9)])
            for _ in range(2):
                for j in range(i):
                    v = v - float(v @ U[j]) * U[j]
                    asum = float(np.abs(v).sum())
                    v = v * (1.0 / asum if asum > eps * 100 else 0.0)
            sd = math.sqrt(float(v @ v))
            ii += 1
        U.append(v * (1.0 / sd if sd > DBL_MIN else 0.0))
    return U[7].copy(), U[8].copy()


def seven_point(m1, m2, jacobi=False):
    """run7Point on raw pixel coordinates: the null space of the 7x9 system
    (rows m2^T F m1 = 0) by SVD (FULL_UV: null_space_7x9), det(lambda f1 +
    (1 - lambda) f2) = 0, up to three matrices scaled to F33 = 1."""
    A = np.zeros((7, 9))
    for i in range(7):
        x0, y0, x1, y1 = float(m1[i, 0]), float(m1[i, 1]), float(m2[i, 0]), float(m2[i, 1])
        A[i] = [x1 * x0, x1 * y0, x1, y1 * x0, y1 * y0, y1, x0, y0, 1.0]
    if jacobi:
        from oracle.pnp_oracle import cv_svd
        f1, f2 = null_space_7x9(cv_svd(A.T)[1].T)
    else:
        f1, f2 = null_space_7x9(np.linalg.svd(A, full_matrices=False)[2])
    f1 -= f2  # f = lambda (f1 - f2) + f2
    A3, B3 = f1.reshape(3, 3), f2.reshape(3, 3)
    # det(lambda A + B) = det A l^3 + c1 l^2 + c2 l + det B; c2 (c1) = the sum
    # over rows of det B (A) with that row taken from A (B)
    c1 = c2 = 0.0
    for i in range(3):
        M = B3.copy()
        M[i] = A3[i]
        c2 += _det3(M)
        M = A3.copy()
        M[i] = B3[i]
        c1 += _det3(M)
    roots = solve_cubic(_det3(A3), c1, c2, _det3(B3))
    out = []
    for r in roots:
        lam, mu = r, 1.0
        s = f1[8] * r + f2[8]
        F = np.zeros(9)
        if abs(s) > DBL_EPS:
            mu = 1.0 / s
            lam *= mu
            F[8] = 1.0
        F[:8] = f1[:8] * lam + f2[:8] * mu
        out.append(F.reshape(3, 3))
    return out


def _line_terms(F, p0, p1):
    """(d1, n1^2, d0, n0^2): the residual x1^T F x0 against the line F x0 in
    image 1 and against F^T x1 in image 0, with the squared line norms."""
    x0, y0, x1, y1 = p0[:, 0], p0[:, 1], p1[:, 0], p1[:, 1]
    a = F[0, 0] * x0 + F[0, 1] * y0 + F[0, 2]
    b = F[1, 0] * x0 + F[1, 1] * y0 + F[1, 2]
    c = F[2, 0] * x0 + F[2, 1] * y0 + F[2, 2]
    n1 = a * a + b * b
    d1 = x1 * a + y1 * b + c
    a = F[0, 0] * x1 + F[1, 0] * y1 + F[2, 0]
    b = F[0, 1] * x1 + F[1, 1] * y1 + F[2, 1]
    c = F[0, 2] * x1 + F[1, 2] * y1 + F[2, 2]
    n0 = a * a + b * b
    d0 = x0 * a + y0 * b + c
    return d1, n1, d0, n0


def f_errors(F, p0, p1):
    """FMEstimatorCallback::computeError: max of the two squared point-line
    distances, computed in double, stored as float."""
    d1, n1, d0, n0 = _line_terms(F, p0, p1)
    with np.errstate(all="ignore"):
        return np.maximum(d0 * d0 * (1.0 / n0), d1 * d1 * (1.0 / n1)).astype(np.float32)


def epi_distances(F, p0, p1):
    """point-to-epipolar-line distances (not squared): (in image 0, in image 1)"""
    d1, n1, d0, n0 = _line_terms(F, p0, p1)
    with np.errstate(all="ignore"):
        return np.abs(d0) / np.sqrt(n0), np.abs(d1) / np.sqrt(n1)


def find_fundamental_ransac(p0, p1, thr=3.84, confidence=0.99, max_iters=1000, trace=None):
    """-> (F or None, mask uint8 [n]).  `trace`, a dict, receives the float
    errors of every evaluated model and the acceptance chain."""
    n = len(p0)
    thr32 = np.float32(thr * thr)
    rng = CvRNG()
    niters = max(int(max_iters), 1)
    best, best_mask, max_good = None, np.zeros(n, np.uint8), 0
    it = 0
    while it < niters:
        sub = get_subset(rng, n, 7)
        for root, F in enumerate(seven_point(p0[sub], p1[sub])):
            err = f_errors(F, p0, p1)
            mask = err <= thr32
            good = int(mask.sum())
            if trace is not None:
                trace.setdefault("errors", []).append(err)
                trace.setdefault("counts", []).append((good, max(max_good, 6)))
            if good > max(max_good, 6):
                if trace is not None:
                    trace.setdefault("chain", []).append((good, max(max_good, 6)))
                    trace["best"] = (sub, root)
                best, best_mask, max_good = F, mask.astype(np.uint8), good
                niters = ransac_update_num_iters(confidence, (n - good) / n, 7, niters)
        it += 1
    return best, best_mask


# ---- findHomography(method 0) ----------------------------------------------
def homography_dlt(M, m):
    """HomographyEstimatorCallback::runKernel: normalised DLT, M -> m."""
    n = len(M)
    cM, cm = M.sum(0) / n, m.sum(0) / n
    sM, sm = np.abs(M - cM).sum(0), np.abs(m - cm).sum(0)
    if min(sM.min(), sm.min()) < DBL_EPS:
        return None
    sM, sm = n / sM, n / sm
    invHnorm = np.array([[1.0 / sm[0], 0, cm[0]], [0, 1.0 / sm[1], cm[1]], [0, 0, 1]])
    Hnorm2 = np.array([[sM[0], 0, -cM[0] * sM[0]], [0, sM[1], -cM[1] * sM[1]], [0, 0, 1]])
    x, y = (m[:, 0] - cm[0]) * sm[0], (m[:, 1] - cm[1]) * sm[1]
    X, Y = (M[:, 0] - cM[0]) * sM[0], (M[:, 1] - cM[1]) * sM[1]
    one, zero = np.ones(n), np.zeros(n)
    Lx = np.stack([X, Y, one, zero, zero, zero, -x * X, -x * Y, -x], 1)
    Ly = np.stack([zero, zero, zero, X, Y, one, -y * X, -y * Y, -y], 1)
    LtL = Lx.T @ Lx + Ly.T @ Ly
    H0 = np.linalg.eigh(LtL)[1][:, 0].reshape(3, 3)
    H = invHnorm @ H0 @ Hnorm2
    return H * (1.0 / H[2, 2])


def _h_residual(h, M, m, want_j):
    Mx, My = M[:, 0], M[:, 1]
    ww = h[6] * Mx + h[7] * My + 1.0
    ww = np.where(np.abs(ww) > DBL_EPS, 1.0 / np.where(ww == 0, 1.0, ww), 0.0)
    xi = (h[0] * Mx + h[1] * My + h[2]) * ww
    yi = (h[3] * Mx + h[4] * My + h[5]) * ww
    r = np.stack([xi - m[:, 0], yi - m[:, 1]], 1).reshape(-1)
    if not want_j:
        return r, None
    z = np.zeros_like(Mx)
    Jx = np.stack([Mx * ww, My * ww, ww, z, z, z, -Mx * ww * xi, -My * ww * xi], 1)
    Jy = np.stack([z, z, z, Mx * ww, My * ww, ww, -Mx * ww * yi, -My * ww * yi], 1)
    return r, np.stack([Jx, Jy], 1).reshape(-1, 8)


def homography_refine(H, M, m, max_iters=10):
    """cv::LMSolver::run (levmarq.cpp) on HomographyRefineCallback."""
    x = H.reshape(-1)[:8].copy()
    r, J = _h_residual(x, M, m, True)
    S = float(r @ r)
    A, v = J.T @ J, J.T @ r
    D = np.diag(A).copy()
    Rlo, Rhi = 0.25, 0.75
    lam, lc = 1.0, 0.75
    it = 0
    while True:
        Ap = A + np.diag(D * lam)
        d = np.linalg.solve(Ap, v)
        xd = x - d
        rd, _ = _h_residual(xd, M, m, False)
        Sd = float(rd @ rd)
        dS = float(d @ (2 * v - A @ d))
        R = (S - Sd) / (dS if abs(dS) > DBL_EPS else 1.0)
        if R > Rhi:
            lam *= 0.5
            if lam < lc:
                lam = 0.0
        elif R < Rlo:
            t = float(d @ v)
            nu = (Sd - S) / (t if abs(t) > DBL_EPS else 1.0) + 2
            nu = min(max(nu, 2.0), 10.0)
            if lam == 0:
                maxval = max(DBL_EPS, float(np.abs(np.diag(np.linalg.inv(A))).max()))
                lam = lc = 1.0 / maxval
                nu *= 0.5
            lam *= nu
        if Sd < S:
            S, x = Sd, xd
            r, J = _h_residual(x, M, m, True)
            A, v = J.T @ J, J.T @ r
        it += 1
        if not (it < max_iters and np.abs(d).max() >= FLT_EPS and np.abs(r).max() >= FLT_EPS):
            break
    return np.append(x, 1.0).reshape(3, 3)


def find_homography(p0, p1):
    H = homography_dlt(p0, p1)
    if H is None:
        return None
    return homography_refine(H, p0, p1) if len(p0) > 4 else H


def transfer(H, p):
    w = H[2, 0] * p[:, 0] + H[2, 1] * p[:, 1] + H[2, 2]
    with np.errstate(all="ignore"):
        return np.stack([(H[0, 0] * p[:, 0] + H[0, 1] * p[:, 1] + H[0, 2]) / w,
                         (H[1, 0] * p[:, 0] + H[1, 1] * p[:, 1] + H[1, 2]) / w], 1)


def inv3(M):
    c = np.array([[M[1, 1] * M[2, 2] - M[1, 2] * M[2, 1], M[0, 2] * M[2, 1] - M[0, 1] * M[2, 2],
                   M[0, 1] * M[1, 2] - M[0, 2] * M[1, 1]],
                  [M[1, 2] * M[2, 0] - M[1, 0] * M[2, 2], M[0, 0] * M[2, 2] - M[0, 2] * M[2, 0],
                   M[0, 2] * M[1, 0] - M[0, 0] * M[1, 2]],
                  [M[1, 0] * M[2, 1] - M[1, 1] * M[2, 0], M[0, 1] * M[2, 0] - M[0, 0] * M[2, 1],
                   M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]]])
    det = M[0, 0] * c[0, 0] + M[0, 1] * c[1, 0] + M[0, 2] * c[2, 0]
    return c * (1.0 / det)


# ---- decompositions --------------------------------------------------------
def rt_from_essential(E):
    """The four (R, t) of E = U diag(1, 1, 0) V^T, det R = +1, |t| = 1."""
    U, _, Vt = np.linalg.svd(E)
    u1, u2, u3 = U[:, 0], U[:, 1], U[:, 2]
    v1, v2, v3 = Vt[0], Vt[1], Vt[2]
    Ra = np.outer(u2, v1) - np.outer(u1, v2) + np.outer(u3, v3)
    Rb = -np.outer(u2, v1) + np.outer(u1, v2) + np.outer(u3, v3)
    if _det3(Ra) < 0:
        Ra = -Ra
    if _det3(Rb) < 0:
        Rb = -Rb
    t = u3 / math.sqrt(float(u3 @ u3))
    return [(Ra, t), (Ra, -t), (Rb, t), (Rb, -t)]


def rt_from_homography(A):
    """The eight Faugeras candidates of A = K1^-1 H K0 (ORB-SLAM ReconstructH);
    none when two singular values coincide (ratio < 1.00001)."""
    U, w, Vt = np.linalg.svd(A)
    s = _det3(U) * _det3(Vt)
    d1, d2, d3 = (float(x) for x in w)
    if d1 / d2 < 1.00001 or d2 / d3 < 1.00001:
        return []
    aux1 = math.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
    aux3 = math.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
    x1 = [aux1, aux1, -aux1, -aux1]
    x3 = [aux3, -aux3, aux3, -aux3]
    prod = math.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3))
    out = []
    ast = prod / ((d1 + d3) * d2)
    ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
    for i, st in enumerate([ast, -ast, -ast, ast]):
        Rp = np.array([[ct, 0, -st], [0, 1, 0], [st, 0, ct]])
        R = s * (U @ Rp @ Vt)
        t = U @ (np.array([x1[i], 0, -x3[i]]) * (d1 - d3))
        out.append((R, t / math.sqrt(float(t @ t))))
    asp = prod / ((d1 - d3) * d2)
    cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
    for i, sp in enumerate([asp, -asp, -asp, asp]):
        Rp = np.array([[cp, 0, sp], [0, -1, 0], [sp, 0, -cp]])
        R = s * (U @ Rp @ Vt)
        t = U @ (np.array([x1[i], 0, x3[i]]) * (d1 + d3))
        out.append((R, t / math.sqrt(float(t @ t))))
    return out


def triangulate(K0, K1, R, t, p0, p1):
    """sfm_triangulate_points' arithmetic on P0 = K0 [I|0], P1 = K1 [R|t]: the
    4x4 DLT system per point, its smallest right singular vector."""
    Pa = K0 @ np.hstack([np.eye(3), np.zeros((3, 1))])
    Pb = K1 @ np.hstack([R, t.reshape(3, 1)])
    A = np.stack([p0[:, 0:1] * Pa[2] - Pa[0], p0[:, 1:2] * Pa[2] - Pa[1],
                  p1[:, 0:1] * Pb[2] - Pb[0], p1[:, 1:2] * Pb[2] - Pb[1]], 1)
    v = np.linalg.svd(A)[2][:, 3, :]
    with np.errstate(all="ignore"):
        return v[:, :3] / v[:, 3:4]


def vote(K0, K1, R, t, p0, p1, max_err):
    """-> (good [n] bool, cos parallax [n], reprojection errors [n][2], X)"""
    X = triangulate(K0, K1, R, t, p0, p1)
    Xc = X @ R.T + t
    with np.errstate(all="ignore"):
        u0 = X[:, :2] / X[:, 2:3] * [K0[0, 0], K0[1, 1]] + [K0[0, 2], K0[1, 2]]
        u1 = Xc[:, :2] / Xc[:, 2:3] * [K1[0, 0], K1[1, 1]] + [K1[0, 2], K1[1, 2]]
        e = np.stack([np.sqrt(((u0 - p0) ** 2).sum(1)), np.sqrt(((u1 - p1) ** 2).sum(1))], 1)
        C1 = -R.T @ t
        n1 = X - C1
        cosp = (X * n1).sum(1) / (np.sqrt((X * X).sum(1)) * np.sqrt((n1 * n1).sum(1)))
        good = np.isfinite(X).all(1) & (X[:, 2] > 0) & (Xc[:, 2] > 0) & (e[:, 0] <= max_err) & (e[:, 1] <= max_err)
    return good, cosp, e, X


@dataclass
class TwoViewRef:
    model: int = 0
    H: np.ndarray = field(default_factory=lambda: np.zeros((3, 3)))
    F: np.ndarray = field(default_factory=lambda: np.zeros((3, 3)))
    f_mask: np.ndarray = None
    scores: np.ndarray = field(default_factory=lambda: np.zeros(2))
    avg_err: float = 0.0
    R: np.ndarray = field(default_factory=lambda: np.zeros((3, 3)))
    t: np.ndarray = field(default_factory=lambda: np.zeros(3))
    keep: np.ndarray = None
    X: np.ndarray = None
    n_kept: int = 0
    diag: dict = field(default_factory=dict)  # intermediate figures for the stability conditions


def f32_rounding_margin(M):
    """The least distance, in float32 ulps, of an element of the double matrix
    M from the midpoint between two float32 values (where its rounding would
    flip): 0.5 = exactly representable, 0 = on the boundary."""
    M = np.asarray(M, np.float64).reshape(-1)
    M = M[M != 0]
    f = M.astype(np.float32)
    ulp = np.spacing(np.abs(f)).astype(np.float64)
    return float((0.5 - np.abs(M - f.astype(np.float64)) / ulp).min())


def two_view_init(pts0, pts1, K0, K1, trace=None, **opts):
    o = dict(DEFAULTS)
    o.update(opts)
    p0 = np.asarray(pts0, np.float32).reshape(-1, 2).astype(np.float64)
    p1 = np.asarray(pts1, np.float32).reshape(-1, 2).astype(np.float64)
    K0 = np.asarray(K0, np.float64).reshape(3, 3)
    K1 = np.asarray(K1, np.float64).reshape(3, 3)
    n = len(p0)
    res = TwoViewRef(f_mask=np.zeros(n, np.uint8), keep=np.zeros(n, np.uint8), X=np.zeros((n, 3)))
    if n < MIN_POINTS:
        return res
    F64, mask = find_fundamental_ransac(p0, p1, o["f_ransac_threshold"], o["f_confidence"], o["f_max_iters"], trace)
    H64 = find_homography(p0, p1)
    if F64 is None or H64 is None:  # (no model of either kind: no initialisation)
        return res
    F = F64.astype(np.float32).astype(np.float64)
    H = H64.astype(np.float32).astype(np.float64)
    res.F, res.H, res.f_mask = F, H, mask
    res.diag.update(F64=F64, H64=H64)
    # scores (CSfM.cpp:415-469): squared transfer errors for H, distances for F
    fwd, bwd = transfer(H, p0), transfer(inv3(H), p1)
    e01, e10 = ((p1 - fwd) ** 2).sum(1), ((p0 - bwd) ** 2).sum(1)
    th, g = o["h_score_th"], o["h_score_gamma"]
    s_h = float((np.where(e01 < th, g - e01, 0.0) + np.where(e10 < th, g - e10, 0.0)).sum() / n)
    inl = mask == 1
    dist0, dist1 = epi_distances(F, p0, p1)
    th, g = o["f_score_th"], o["f_score_gamma"]
    s_f = float((np.where(dist0 < th, g - dist0, 0.0) + np.where(dist1 < th, g - dist1, 0.0))[inl].sum() / inl.sum())
    res.scores = np.array([s_h, s_f])
    r_h = s_h / (s_h + s_f)
    res.diag["r_h"] = r_h
    if r_h > o["h_ratio"]:
        branch, surv = 1, np.ones(n, bool)
        res.avg_err = float((0.5 * (np.sqrt(e01) + np.sqrt(e10))).sum() / n)
        cands = rt_from_homography(inv3(K1) @ H @ K0)
    else:
        branch, surv = 2, inl
        res.avg_err = float((0.5 * (dist0 + dist1))[inl].sum() / inl.sum())
        cands = rt_from_essential(K1.T @ F @ K0)
    res.diag["branch"] = branch
    if not cands or not res.avg_err < o["max_repr_err"]:
        return res
    # candidate vote over the surviving matches
    votes = [vote(K0, K1, R, t, p0, p1, o["max_repr_err"]) for R, t in cands]
    goods = [int((v[0] & surv).sum()) for v in votes]
    best = int(np.argmax(goods))
    gb = goods[best]
    second = max(g_ for i, g_ in enumerate(goods) if i != best)
    n_surv = int(surv.sum())
    sel = votes[best][0] & surv
    cos_thr = math.cos(math.radians(o["min_parallax_deg"]))
    n_par = int((votes[best][1][sel] <= cos_thr).sum())
    res.diag.update(goods=goods, good_best=gb, second=second, n_surv=n_surv, n_par=n_par,
                    need=max(o["min_good"], o["min_good_fraction"] * n_surv),
                    vote_err=votes[best][2][surv],
                    median_parallax_deg=float(np.degrees(np.arccos(np.clip(np.sort(votes[best][1][sel])[::-1][gb // 2]
                                                                           if gb else 1.0, -1, 1)))))
    if not (gb >= max(o["min_good"], o["min_good_fraction"] * n_surv) and second < o["ambiguity_ratio"] * gb and
            gb > 0 and n_par >= gb - gb // 2):
        return res
    R, t = cands[best]
    X = votes[best][3]
    Xc = X @ R.T + t
    with np.errstate(all="ignore"):
        keep = (surv & np.isfinite(X).all(1) & (X[:, 2] > 0) & (Xc[:, 2] > 0) & (dist0 <= o["max_repr_err"]) &
                (dist1 <= o["max_repr_err"]))
    res.diag["filter_dist"] = np.stack([dist0, dist1], 1)[surv]
    res.model, res.R, res.t = branch, R, t
    res.keep, res.X, res.n_kept = keep.astype(np.uint8), X, int(keep.sum())
    return res
