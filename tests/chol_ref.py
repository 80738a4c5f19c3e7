"""Plain NumPy references for the dense reduced-camera solve (A y = b, A
symmetric positive definite), CPU only.

ref_solve            the yardstick: unblocked Cholesky in np.longdouble (x87
                     extended, 64-bit mantissa, unit roundoff 2^-64) plus three
                     steps of iterative refinement with longdouble residuals
fp64_solve           the textbook fp64 solve (np.linalg.cholesky + two
                     triangular solves): what correct fp64 code achieves
blocked_model_solve  an fp64 model of the formulation the kernels document
                     (chol_kernels.hip): the augmented lower image in 64-wide
                     tiles, an explicit W_j = L_jj^-1, L_ij = P_ij W_j^T, z as
                     row n, y_b = W_b^T (z_b - sum_{k>b} L_kb^T y_k).  Its only
                     purpose: what error the explicit inverse carries by itself
errors               forward and normwise backward error of a solution, in
                     longdouble, on the diagonally equilibrated system

Every solver takes b of shape (n,) or (n, k) (k right-hand sides at once).
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53          # fp64 unit roundoff
NB = 64                 # the kernels' tile width


def _ld_cholesky(A):
    """Lower factor of A (only its upper triangle is read) in longdouble, or
    (None, j) at the first pivot j that is not > 0 (a NaN pivot included)."""
    n = A.shape[0]
    Au = np.triu(np.asarray(A, dtype=LD))
    As = Au + np.triu(Au, 1).T
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        v = As[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0:
            return None, j
        d = np.sqrt(v[0])
        L[j, j] = d
        L[j + 1:, j] = v[1:] / d
    return L, -1


def _ld_lower_solve(L, B):
    X = np.array(B, dtype=LD)
    for i in range(L.shape[0]):
        X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def _ld_upper_solve_t(L, B):
    """Solve L^T X = B."""
    X = np.array(B, dtype=LD)
    for i in range(L.shape[0] - 1, -1, -1):
        X[i] = (X[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


_SPLIT = LD(2.0 ** 32 + 1)   # Veltkamp's constant for a 64-bit mantissa


def _two_prod(a, b):
    """a * b = p + e exactly (Dekker), elementwise in longdouble."""
    p = a * b
    t = _SPLIT * a
    ah = t - (t - a)
    al = a - ah
    t = _SPLIT * b
    bh = t - (t - b)
    bl = b - bh
    return p, al * bl - (((p - ah * bh) - al * bh) - ah * bl)


def _ld_residual(As, y, b):
    """b - As y in longdouble with every product and sum carried error-free
    (Ogita, Rump and Oishi's Dot2): as if formed in twice the precision and
    rounded once.  A plain longdouble residual leaves the refined solution at
    cond(A) 2^-64, which on the graded families (cond 1e6, 1e10) is short of
    a yardstick for fp64 by fewer digits than the tests need."""
    s = np.array(b, dtype=LD)
    c = np.zeros_like(s)
    for j in range(As.shape[0]):
        col = As[:, j] if s.ndim == 1 else As[:, j, None]
        p, e = _two_prod(col, y[j])
        t = s - p
        z = t - s
        c += ((s - (t - z)) + (-p - z)) - e      # TwoSum(s, -p)'s error, and the product's
        s = t
    return s + c


def ref_solve(A, b):
    """(y, -1) with y in longdouble, or (None, j): pivot j was not > 0."""
    L, bad = _ld_cholesky(A)
    if L is None:
        return None, bad
    Au = np.triu(np.asarray(A, dtype=LD))
    As = Au + np.triu(Au, 1).T
    bl = np.asarray(b, dtype=LD)
    y = _ld_upper_solve_t(L, _ld_lower_solve(L, bl))
    for _ in range(3):
        y = y + _ld_upper_solve_t(L, _ld_lower_solve(L, _ld_residual(As, y, bl)))
    return y, -1


def _sym_upper(A):
    Au = np.triu(np.asarray(A, dtype=np.float64))
    return Au + np.triu(Au, 1).T


def _lower_solve(L, B):
    X = np.array(B, dtype=np.float64)
    for i in range(L.shape[0]):
        X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def _upper_solve_t(L, B):
    X = np.array(B, dtype=np.float64)
    for i in range(L.shape[0] - 1, -1, -1):
        X[i] = (X[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


def fp64_solve(A, b):
    L = np.linalg.cholesky(_sym_upper(A))
    return _upper_solve_t(L, _lower_solve(L, np.asarray(b, dtype=np.float64)))


def _lower_inverse(L):
    """W = L^-1 by forward substitution on the identity's columns."""
    return _lower_solve(L, np.eye(L.shape[0]))


def blocked_model_solve(A, b):
    """fp64, the kernels' formulation: left-looking 64-wide tiles over the
    augmented image [A; b^T] (row n carries the right-hand side, so its tiles
    come out as z = L^-1 b), every off-diagonal tile finished with the
    explicit inverse W_j of its column's diagonal factor, then the back
    substitution by block rows, again through W_b."""
    As = _sym_upper(A)
    n = As.shape[0]
    bb = np.asarray(b, dtype=np.float64)
    one = bb.ndim == 1
    B = bb.reshape(n, -1)
    k = B.shape[1]
    nb = (n + NB - 1) // NB
    G = np.vstack([As, B.T])                 # rows n .. n+k-1: the right-hand sides
    L = np.zeros((n + k, n))
    W = []
    for j in range(nb):
        c0, c1 = j * NB, min(j * NB + NB, n)
        P = G[c0:, c0:c1] - L[c0:, :c0] @ L[c0:c1, :c0].T    # P_ij, i >= j
        Ljj = np.linalg.cholesky(P[:c1 - c0])
        Wj = _lower_inverse(Ljj)
        L[c0:c1, c0:c1] = Ljj
        L[c1:, c0:c1] = P[c1 - c0:] @ Wj.T                     # L_ij = P_ij W_j^T (the z rows too)
        W.append(Wj)
    Z = L[n:, :].T                            # (n, k)
    Y = np.zeros((n, k))
    for bi in range(nb - 1, -1, -1):
        c0, c1 = bi * NB, min(bi * NB + NB, n)
        acc = Z[c0:c1].copy()
        for kb in range(nb - 1, bi, -1):      # the chain's order: the last block row first
            k0, k1 = kb * NB, min(kb * NB + NB, n)
            acc -= L[k0:k1, c0:c1].T @ Y[k0:k1]
        Y[c0:c1] = W[bi].T @ acc
    return Y[:, 0] if one else Y


def errors(A, b, y, y_ref):
    """(forward, backward) of y for A y = b (b, y, y_ref of shape (n,)), in
    longdouble on the equilibrated system D = sqrt(diag A), A' = D^-1 A D^-1,
    y' = D y, b' = D^-1 b:
      forward  = max|y' - y'_ref| / max|y'_ref|
      backward = max|b' - A' y'| / (||A'||_inf max|y'| + max|b'|).
    (Unequilibrated, the normwise backward error of a badly scaled system is
    blind: its large rows hide the small ones.)  A zero numerator over a zero
    denominator counts as 0."""
    Au = np.triu(np.asarray(A, dtype=LD))
    As = Au + np.triu(Au, 1).T
    D = np.sqrt(np.diag(As))
    Ae = As / D[:, None] / D[None, :]
    ye = D * np.asarray(y, dtype=LD)
    yr = D * np.asarray(y_ref, dtype=LD)
    be = np.asarray(b, dtype=LD) / D

    def ratio(num, den):
        if num == 0:
            return 0.0
        return float(num / den) if den > 0 else float("inf")

    fwd = ratio(np.max(np.abs(ye - yr)), np.max(np.abs(yr)))
    r = _ld_residual(Ae, ye, be)
    bwd = ratio(np.max(np.abs(r)), np.max(np.sum(np.abs(Ae), axis=1)) * np.max(np.abs(ye)) + np.max(np.abs(be)))
    return fwd, bwd


def caps(A, b, y_ref):
    """The bounds the GPU tests apply to the kernels' y, from correct fp64
    code alone: 8 x the worse of fp64_solve and the blocked model (floors 4u
    forward, u backward).  Returns (cap_fwd, cap_bwd, (ff, fb, mf, mb)).

    The factor 8 is the margin for another accumulation order: chains of
    16x16x4 MFMAs where the models take dot products; at n <= 384 that is at
    most 96 four-term links per entry."""
    return caps_of(A, b, fp64_solve(A, b), blocked_model_solve(A, b), y_ref)


def caps_of(A, b, y_fp64, y_model, y_ref):
    """caps() from solutions already at hand."""
    ff, fb = errors(A, b, y_fp64, y_ref)
    mf, mb = errors(A, b, y_model, y_ref)
    return 8.0 * max(ff, mf, 4 * U), 8.0 * max(fb, mb, U), (ff, fb, mf, mb)
