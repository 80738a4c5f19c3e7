"""Plain NumPy references for the geometry kernels' small dense linear
algebra (sfm_amd/csrc/cv_linalg.h, cv_svd12_lanes), CPU only.

ld_svd          the yardstick everything is measured against: one-sided Jacobi
                from the definition in np.longdouble (x87 extended, unit
                roundoff 2^-64), run until no pair of columns is correlated
                beyond a few longdouble eps, batched over the leading axis
ld_lstsq        truncated least squares on ld_svd with cv::solve(DECOMP_SVD)'s
                rule (w_i <= 2 DBL_EPSILON sum(w) dropped)
ld_triangulate  the DLT point: right singular vector of the smallest singular
                value of the 4x4 system (built in longdouble from the fp64
                inputs), then the division
svd_metrics     the errors of an fp64 SVD against ld_svd (below)
fp64_jacobi     a NumPy model of JacobiSVDImpl_ with switches that plant the
                faults tests/test_linalg_ref.py shows the caps to catch; never
                a yardstick

Metrics (svd_metrics), all dimensionless:
  sv     max |w - sigma| / sigma_1
  recon  |U diag(w) Vt - A|_F / |A|_F
  orthv  max |Vt Vt^T - I|;  orthu  max |U^T U - I| (completed vectors included)
  vecu / vecv   for every returned singular vector the norm of its component
         outside the reference's subspace of its CLUSTER, times gap / sigma_1.
         A cluster is a maximal run of reference singular values whose
         consecutive differences are <= GAP sigma_1 (sign and in-cluster
         rotation are then no errors; for a lone value this is the sine of the
         angle to the reference vector); gap is the cluster's distance to its
         nearest outside neighbour (for the left vectors of a tall matrix the
         left null space is such a neighbour, at 0).  With orthu / orthv at rounding level this
         is the distance between the projectors.  A singular vector's
         condition number is sigma_1 / gap, so the scaled figure has the
         floor eps whatever the spectrum.  Left vectors of (numerically) zero
         singular values are only determined as orthogonal to the range: for
         them the component INSIDE the range counts, scaled the same way.
"""
import numpy as np

LD = np.longdouble
EPS = np.finfo(np.float64).eps
EPS_LD = np.finfo(LD).eps
DBL_MIN = np.finfo(np.float64).tiny
GAP = 1e-6          # cluster threshold, as a fraction of sigma_1
ZERO_LD = 1e-17     # reference singular values below this fraction of sigma_1 count as zero


def ld_svd(A, sweeps=60):
    """A [..., M, N] (M >= N or not) -> sigma [..., N] descending, U [..., M, N]
    (columns; zero where sigma is exactly 0), V [..., N, N] (columns), longdouble."""
    A = np.asarray(A, dtype=LD)
    lead = A.shape[:-2]
    M, N = A.shape[-2:]
    G = A.reshape((-1, M, N)).copy()
    B = G.shape[0]
    V = np.broadcast_to(np.eye(N, dtype=LD), (B, N, N)).copy()
    tol = 2 * EPS_LD
    # columns that have shrunk to the rounding noise of the whole matrix are
    # zero singular values: nothing turns against them any more
    zero2 = (8 * EPS_LD) ** 2 * np.einsum("bkn,bkn->b", G, G)
    for _ in range(sweeps):
        turned = False
        for i in range(N - 1):
            for j in range(i + 1, N):
                gi, gj = G[:, :, i], G[:, :, j]
                a = np.einsum("bk,bk->b", gi, gi)
                b = np.einsum("bk,bk->b", gj, gj)
                p = np.einsum("bk,bk->b", gi, gj)
                act = (np.abs(p) > tol * np.sqrt(a) * np.sqrt(b)) & (a > zero2) & (b > zero2)
                if not act.any():
                    continue
                turned = True
                ps = np.where(act, p, LD(1))
                zeta = (b - a) / (2 * ps)
                t = np.where(zeta >= 0, LD(1), LD(-1)) / (np.abs(zeta) + np.sqrt(1 + zeta * zeta))
                c = 1 / np.sqrt(1 + t * t)
                s = c * t
                c = np.where(act, c, LD(1))[:, None]
                s = np.where(act, s, LD(0))[:, None]
                G[:, :, i], G[:, :, j] = c * gi - s * gj, s * gi + c * gj
                vi, vj = V[:, :, i].copy(), V[:, :, j].copy()
                V[:, :, i], V[:, :, j] = c * vi - s * vj, s * vi + c * vj
        if not turned:
            break
    else:
        raise RuntimeError("ld_svd: no convergence")
    sig = np.sqrt(np.einsum("bkn,bkn->bn", G, G))
    order = np.argsort(-sig, axis=1, kind="stable")
    sig = np.take_along_axis(sig, order, 1)
    G = np.take_along_axis(G, order[:, None, :], 2)
    V = np.take_along_axis(V, order[:, None, :], 2)
    U = np.where(sig[:, None, :] > 0, G / np.where(sig > 0, sig, LD(1))[:, None, :], LD(0))
    return sig.reshape(lead + (N,)), U.reshape(lead + (M, N)), V.reshape(lead + (N, N))


def ld_lstsq(A, b):
    """cv::solve(A, b, DECOMP_SVD) in longdouble: A [..., M, N], b [..., M] -> x
    [..., N], kept [..., N] (which singular values pass w > 2 DBL_EPSILON
    sum(w)), sigma."""
    sig, U, V = ld_svd(A)
    thr = 2 * LD(EPS) * sig.sum(-1, keepdims=True)
    kept = sig > thr
    coef = np.einsum("...mn,...m->...n", U, np.asarray(b, LD)) / np.where(kept, sig, LD(1))
    coef = np.where(kept, coef, LD(0))
    return np.einsum("...kn,...n->...k", V, coef), kept, sig


def tri_system(Pa, Pb, uva, uvb, dtype=LD):
    """The 4x4 DLT systems [n][4][4] of cvTriangulatePoints (tri_point.h)."""
    Pa, Pb = np.asarray(Pa, dtype), np.asarray(Pb, dtype)
    uva, uvb = np.asarray(uva, dtype), np.asarray(uvb, dtype)
    return np.stack([uva[:, 0, None] * Pa[:, 2] - Pa[:, 0], uva[:, 1, None] * Pa[:, 2] - Pa[:, 1],
                     uvb[:, 0, None] * Pb[:, 2] - Pb[:, 0], uvb[:, 1, None] * Pb[:, 2] - Pb[:, 1]], axis=1)


def ld_triangulate(Pa, Pb, uva, uvb):
    """-> X [n][3], h [n] (of the unit right singular vector), cond [n]: the
    relative condition number of X against a rounding-level perturbation of
    the system, (sigma_1 / (sigma_3 - sigma_4)) (1 + |X|) / (|h| |X|): the
    singular vector moves by eps sigma_1 / gap, and X = v[:3] / h turns a
    move d of v into (d[:3] - X d[3]) / h."""
    sig, _, V = ld_svd(tri_system(Pa, Pb, uva, uvb))
    v = V[:, :, 3]
    h = v[:, 3]
    X = v[:, :3] / h[:, None]
    nx = np.sqrt((X * X).sum(1))
    cond = sig[:, 0] / (sig[:, 2] - sig[:, 3]) * (1 + nx) / (np.abs(h) * nx)
    return X, h, cond


def clusters(sig):
    """Runs of one problem's descending singular values with consecutive
    differences <= GAP sigma_1 -> [(lo, hi, gap / sigma_1)], hi exclusive."""
    n = len(sig)
    s1 = sig[0] if sig[0] > 0 else LD(1)
    out, lo = [], 0
    for i in range(1, n + 1):
        if i == n or sig[i - 1] - sig[i] > GAP * s1:
            g = []
            if lo > 0:
                g.append(sig[lo - 1] - sig[lo])
            if i < n:
                g.append(sig[i - 1] - sig[i])
            out.append((lo, i, float(min(g) / s1) if g else 1.0))
            lo = i
    return out


def subspace_errors(sig, R, D, rows=None, left_range=None, null_space=False):
    """R [K, n] reference vectors as columns, D [r, K] device vectors as rows;
    device row q stands at index rows[q] of the descending order.  -> the
    worst gap-scaled component outside the cluster's subspace.  null_space:
    the vectors are left vectors of a tall matrix, whose left null space is a
    neighbour at singular value 0 (Wedin: the gap is then min(gap, sigma))."""
    rows = range(D.shape[0]) if rows is None else rows
    s1 = sig[0] if sig[0] > 0 else LD(1)
    worst = 0.0
    cl = clusters(sig)
    for q, idx in enumerate(rows):
        d = np.asarray(D[q], LD)
        lo, hi, gap = next(c for c in cl if c[0] <= idx < c[1])
        if null_space:
            gap = min(gap, float(sig[hi - 1] / s1))
        if left_range is not None and sig[hi - 1] <= ZERO_LD * s1:
            # a left vector of a zero singular value: anywhere outside the range
            # of the values above the cluster (values of the cluster that are
            # not zero span, with it, the same complement)
            Rn = left_range[:, :lo]
            err = float(np.sqrt(((Rn.T @ d) ** 2).sum())) * gap if lo else 0.0
        else:
            Rc = R[:, lo:hi]
            res = d - Rc @ (Rc.T @ d)
            err = float(np.sqrt((res * res).sum())) * gap
        worst = max(worst, err)
    return worst


def svd_metrics(A, w, Ut, Vt, ref=None):
    """Errors of one fp64 SVD (w [N], Ut [N][M] rows = left vectors, Vt [N][N] or
    None) of A [M][N] against ld_svd (ref = its result for A, if at hand)."""
    sig, U, V = ld_svd(A) if ref is None else ref
    A = np.asarray(A, LD)
    w, Ut = np.asarray(w, LD), np.asarray(Ut, LD)
    N = len(w)
    s1 = sig[0] if sig[0] > 0 else LD(1)
    m = {"sv": float(np.max(np.abs(w - sig)) / s1),
         "orthu": float(np.max(np.abs(Ut @ Ut.T - np.eye(N)))),
         "vecu": subspace_errors(sig, U, Ut, left_range=U, null_space=A.shape[0] > N)}
    if Vt is not None:
        Vt = np.asarray(Vt, LD)
        na = np.sqrt((A * A).sum())
        m["recon"] = float(np.sqrt((((Ut.T * w) @ Vt - A) ** 2).sum()) / (na if na > 0 else 1))
        m["orthv"] = float(np.max(np.abs(Vt @ Vt.T - np.eye(N))))
        m["vecv"] = subspace_errors(sig, V, Vt)
    return m


def svd12_metrics(A, ut, ref=None):
    """cv_svd12_lanes' four rows (ut[q] = left vector of the (11 - q)-th
    value) of the symmetric A [12][12] against ld_svd."""
    sig, U, V = ld_svd(A) if ref is None else ref
    ut = np.asarray(ut, LD)
    return {"orthu": float(np.max(np.abs(ut @ ut.T - np.eye(4)))),
            "vecu": subspace_errors(sig, U, ut, rows=[11, 10, 9, 8], left_range=U)}


def rel_err(x, ref):
    ref = np.asarray(ref, LD)
    d = np.asarray(x, LD) - ref
    n = np.sqrt((ref * ref).sum(-1))
    return np.sqrt((d * d).sum(-1)) / np.where(n > 0, n, LD(1))


# ---- an fp64 model of JacobiSVDImpl_ with planted faults -------------------
def fp64_jacobi(A, fault=None, trace=None):
    """cv::SVD as cv_linalg.h cv_svd computes it (NumPy fp64, not bit-exact; no
    completion of zero singular values) -> w, Ut [N][M], Vt.  trace: a list
    that receives (sweep, i, j, beta) of every rotation made.  fault:
      "skip_rotation"  the pair (0, 1) is never rotated
      "neg_s_row"      entry 0 of the rotated row j takes +s for -s
      "nosort_vt"      the descending sort moves w and U but not Vt"""
    A = np.asarray(A, np.float64)
    M, N = A.shape
    U = A.T.copy()
    Vt = np.eye(N)
    W = (U * U).sum(1)
    for sweep in range(max(M, 30)):
        changed = False
        for i in range(N - 1):
            for j in range(i + 1, N):
                a, b = W[i], W[j]
                p = float(U[i] @ U[j])
                if abs(p) <= 10 * EPS * np.sqrt(a * b):
                    continue
                if fault == "skip_rotation" and (i, j) == (0, 1):
                    continue
                p *= 2
                beta = a - b
                gamma = np.sqrt(p * p + beta * beta)
                if trace is not None:
                    trace.append((sweep, i, j, beta))
                if beta < 0:
                    s = np.sqrt((gamma - beta) * 0.5 / gamma)
                    c = p / (gamma * s * 2)
                else:
                    c = np.sqrt((gamma + beta) / (gamma * 2))
                    s = p / (gamma * c * 2)
                t0, t1 = c * U[i] + s * U[j], -s * U[i] + c * U[j]
                if fault == "neg_s_row":
                    t1[0] = s * U[i][0] + c * U[j][0]
                U[i], U[j] = t0, t1
                W[i], W[j] = t0 @ t0, t1 @ t1
                Vt[i], Vt[j] = c * Vt[i] + s * Vt[j], -s * Vt[i] + c * Vt[j]
                changed = True
        if not changed:
            break
    w = np.sqrt((U * U).sum(1))
    order = np.argsort(-w, kind="stable")
    w, U = w[order], U[order]
    if fault != "nosort_vt":
        Vt = Vt[order]
    U = U / np.where(w > 0, w, 1.0)[:, None]
    return w, U, Vt


def fp64_lstsq(A, b, two_eps=2 * EPS):
    """cv_lstsq on fp64_jacobi; two_eps = 2e-10 plants the misread threshold."""
    w, Ut, Vt = fp64_jacobi(A)
    thr = w.sum() * two_eps
    x = np.zeros(A.shape[1])
    for i in range(len(w)):
        if abs(w[i]) > thr:
            x = x + (Ut[i] @ b / w[i]) * Vt[i]
    return x


def fp64_triangulate(Pa, Pb, uva, uvb, h_row=3):
    """tri_point on fp64_jacobi; h_row != 3 plants h taken from the wrong row."""
    As = tri_system(Pa, Pb, uva, uvb, np.float64)
    X = np.zeros((len(As), 3))
    for i, A in enumerate(As):
        _, _, Vt = fp64_jacobi(A)
        X[i] = Vt[3][:3] / Vt[h_row][3]
    return X
