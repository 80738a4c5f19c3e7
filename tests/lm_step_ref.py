"""One Levenberg-Marquardt step of the bundle adjuster, exactly as the solver
defines it, in plain NumPy (CPU only), written from the definition and
sharing no code with oracle/ba_oracle.cpp or tests/golden/make_lm_branches.py.

lm_step(problem, x0, x, radius, dtype=np.longdouble) is the reference: every
sum, the 3x3 point factors and the reduced camera system are carried in x87
extended precision (64-bit mantissa).  The same code with dtype=np.float64 is
the "fp64 twin": a second correct fp64 solution of the same step, one of the
yardsticks of tests/test_gpu_lm_step.py (beside the oracle and the
split-residual model below).

The step, for the current point x, the radius r and the Jacobi scale taken at
the solve's start point x0 (the solver fixes it at iteration 0):

  J, res      2x9 Jacobians and residuals of the reprojection functor, by
              forward-mode differentiation on arrays (the theta^2 >
              DBL_EPSILON branch of AngleAxisRotatePoint kept)
  active      cameras and points with an observation; STRUCT_ONLY takes the
              cameras, POSE_ONLY the points out of the system (delta 0)
  scale       1 / (1 + ||column of J at x0||)
  Js          J scale;  diag = clip(diag(Js^T Js), min_lm_diagonal,
              max_lm_diagonal);  H = Js^T Js + diag / r
  y           H y = -Js^T res through the Schur complement: V_p (3x3) per
              point, then S = U - W V^-1 W^T of 6 x (active cameras)
  delta       y scale;  x_new = fl64(x + delta)

An assertion refuses a scaled diagonal entry within a factor 2 of a clamp:
without an active clamp H is D_s (J^T J + diag(J^T J) / r) D_s, delta does not
depend on the scale, and the oracle restarted from x (which takes its scale
at x) is a yardstick of the same step.

The reduced system is solved by tests/chol_ref.ref_solve up to DENSE_LD_MAX
rows, above by an fp64 LAPACK factor of the rounded matrix with iterative
refinement on chol_ref's compensated longdouble residuals until the
correction is below 2^-60 of the solution (refined_solve).

A third yardstick, lm_step(..., dtype=np.float64, split_residual=True),
models one property of the device's formulation.  Its passes keep no
per-observation record: the camera-major pass and the point pass each
evaluate the residual again, through the rotation matrix, with different
contraction and a reciprocal in place of two divisions.  Either residual is
right to a few u |uv| (1e-13 px), but g_c = sum F^T r and g_p = sum E^T r' now
come from r != r'.  Along a gauge direction v (J v = 0, the cost does not
change) the exact gradient vanishes because F v_c + E v_p = 0 observation by
observation; with two residuals v^T g = sum (F v_c)^T (r - r') survives, a few
u |uv| |F v_c| where one shared residual leaves u |J| |r|, and the step along v
is that over the damping diag / radius alone.  Near the optimum, where the
step is small and the residuals are not, this is 100 to 1000 times the error
of fp64 code that evaluates each residual once: a property of the
formulation, harmless to the descent (the cost does not see v), and what the
model reproduces on the CPU (tests/test_lm_step_ref.py).

`fault` plants one defect (tests/test_lm_step_ref.py shows that the caps of
the GPU test see each of them):
  ("pair", i, j)          the contribution of the observation pair (i, j) of
                          one point, cameras different, left out of S
  ("backsub_obs", i)      observation i left out of its point's back
                          substitution
  ("stale_point", p, r')  point p's 3x3 factor damped with the radius r'
  ("no_damping", c)       camera c's damping left out of S
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import chol_ref as R

LD = np.longdouble
U64 = 2.0 ** -53
STRUCT_ONLY, POSE_ONLY, STRUCT_AND_POSE = 0, 1, 2
DENSE_LD_MAX = 400          # rows up to which ref_solve's O(n^3) longdouble loop takes under a second
OPTIONS = dict(min_lm_diagonal=1e-6, max_lm_diagonal=1e32, min_relative_decrease=1e-3, max_trust_region_radius=1e16)


def ref_self_error(mode, radius):
    """What the longdouble Schur route may differ from a dense longdouble
    solve of the full normal equations (the blockwise statistic of
    step_error): 2^-64 = 5.4e-20 times the condition of the damped system.
    Where cameras and points are coupled, the gauge directions are held by
    diag / radius alone, so the condition grows like the radius: 1e-19 x
    radius (6e-16 measured at 1e4), at least 1e-18; block diagonal in the
    other modes: 1e-18 (2e-19 measured).  The GPU test refuses a cap of less
    than 1000 times this; tests/test_lm_step_ref.py checks it at three radii."""
    return max(1e-18, 1e-19 * float(radius)) if mode == STRUCT_AND_POSE else 1e-18


# ---- forward-mode differentiation on arrays --------------------------------
class _Jet:
    """n values with their derivatives by the 9 parameters of an observation."""
    __slots__ = ("a", "v")

    def __init__(self, a, v):
        self.a, self.v = a, v

    @staticmethod
    def lift(o, like):
        if isinstance(o, _Jet):
            return o
        a = np.broadcast_to(np.asarray(o, like.a.dtype), like.a.shape)
        return _Jet(a, np.zeros_like(like.v))

    def __add__(self, o):
        o = _Jet.lift(o, self)
        return _Jet(self.a + o.a, self.v + o.v)

    def __sub__(self, o):
        o = _Jet.lift(o, self)
        return _Jet(self.a - o.a, self.v - o.v)

    def __rsub__(self, o):
        return _Jet.lift(o, self) - self

    def __mul__(self, o):
        o = _Jet.lift(o, self)
        return _Jet(self.a * o.a, self.v * o.a[:, None] + o.v * self.a[:, None])

    __radd__, __rmul__ = __add__, __mul__

    def __truediv__(self, o):
        o = _Jet.lift(o, self)
        q = self.a / o.a
        return _Jet(q, (self.v - o.v * q[:, None]) / o.a[:, None])

    def __rtruediv__(self, o):
        return _Jet.lift(o, self) / self


def residuals_jacobians(pb, x, dtype):
    """res (N, 2), jac (N, 2, 9) with columns d rot | d t | d X, in dtype."""
    rot, t, X = (np.asarray(a, dtype) for a in x)
    cam, pt = pb.cam, pb.pt
    n = len(cam)

    def var(a, i):
        v = np.zeros((n, 9), dtype)
        v[:, i] = 1
        return _Jet(np.ascontiguousarray(a), v)

    w = [var(rot[cam, i], i) for i in range(3)]
    tt = [var(t[cam, i], 3 + i) for i in range(3)]
    p = [var(X[pt, i], 6 + i) for i in range(3)]
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    big = th2.a > np.finfo(np.float64).eps
    # the rotation branch (evaluated on theta^2 = 1 where the other branch holds, to stay finite)
    a2 = _Jet(np.where(big, th2.a, dtype(1)), np.where(big[:, None], th2.v, dtype(0)))
    th = np.sqrt(a2.a)
    theta = _Jet(th, a2.v / (2 * th)[:, None])
    cos = _Jet(np.cos(th), -np.sin(th)[:, None] * theta.v)
    sin = _Jet(np.sin(th), np.cos(th)[:, None] * theta.v)
    inv = 1.0 / theta
    ax = [w[i] * inv for i in range(3)]
    axp = [ax[1] * p[2] - ax[2] * p[1], ax[2] * p[0] - ax[0] * p[2], ax[0] * p[1] - ax[1] * p[0]]
    tmp = (ax[0] * p[0] + ax[1] * p[1] + ax[2] * p[2]) * (1.0 - cos)
    rb = [p[i] * cos + axp[i] * sin + ax[i] * tmp for i in range(3)]
    # the small-angle branch
    wxp = [w[1] * p[2] - w[2] * p[1], w[2] * p[0] - w[0] * p[2], w[0] * p[1] - w[1] * p[0]]
    rs = [p[i] + wxp[i] for i in range(3)]
    q = [_Jet(np.where(big, rb[i].a, rs[i].a), np.where(big[:, None], rb[i].v, rs[i].v)) + tt[i] for i in range(3)]
    xp, yp = q[0] / q[2], q[1] / q[2]
    K = np.asarray(pb.K, dtype).reshape(-1, 9)[cam]
    px = xp * K[:, 0] + yp * K[:, 1] + K[:, 2]
    py = yp * K[:, 4] + K[:, 5]
    uv = np.asarray(pb.uv, dtype)
    res = np.stack([px.a - uv[:, 0], py.a - uv[:, 1]], axis=1)
    return res, np.stack([px.v, py.v], axis=1)


def residuals_matrix_form(pb, x, dtype):
    """The residuals alone, by the formulation the device's passes use: the
    rotation matrix R(w) = c I + s [u]x + (1 - c) u u^T (I + [w]x on the
    small-angle branch), p = R X + t, x / z and y / z as products with 1 / z.
    As accurate as the functor evaluated operation by operation (a few
    u |uv|), with other roundings."""
    rot, t, X = (np.asarray(a, dtype) for a in x)
    th2 = (rot * rot).sum(axis=1)
    big = th2 > np.finfo(np.float64).eps
    th = np.sqrt(np.where(big, th2, dtype(1)))
    u = rot / th[:, None]
    s, c = np.sin(th), np.cos(th)

    def skew(a):
        k = np.zeros((len(a), 3, 3), dtype)
        k[:, 0, 1], k[:, 0, 2], k[:, 1, 0] = -a[:, 2], a[:, 1], a[:, 2]
        k[:, 1, 2], k[:, 2, 0], k[:, 2, 1] = -a[:, 0], -a[:, 1], a[:, 0]
        return k

    eye = np.eye(3, dtype=dtype)
    Rb = c[:, None, None] * eye + s[:, None, None] * skew(u) + (1 - c)[:, None, None] * u[:, :, None] * u[:, None, :]
    R = np.where(big[:, None, None], Rb, eye + skew(rot))
    p = np.einsum("nij,nj->ni", R[pb.cam], X[pb.pt]) + t[pb.cam]
    iz = 1 / p[:, 2]
    xp, yp = p[:, 0] * iz, p[:, 1] * iz
    K = np.asarray(pb.K, dtype).reshape(-1, 9)[pb.cam]
    uv = np.asarray(pb.uv, dtype)
    return np.stack([(K[:, 0] * xp + K[:, 1] * yp + K[:, 2]) - uv[:, 0], (K[:, 4] * yp + K[:, 5]) - uv[:, 1]], axis=1)


# ---- small dense pieces ------------------------------------------------------
def _chol3(V):
    """Lower Cholesky factors of the (P, 3, 3) blocks V, elementwise formulas."""
    L = np.zeros_like(V)
    L[:, 0, 0] = np.sqrt(V[:, 0, 0])
    L[:, 1, 0] = V[:, 1, 0] / L[:, 0, 0]
    L[:, 2, 0] = V[:, 2, 0] / L[:, 0, 0]
    L[:, 1, 1] = np.sqrt(V[:, 1, 1] - L[:, 1, 0] ** 2)
    L[:, 2, 1] = (V[:, 2, 1] - L[:, 2, 0] * L[:, 1, 0]) / L[:, 1, 1]
    L[:, 2, 2] = np.sqrt(V[:, 2, 2] - L[:, 2, 0] ** 2 - L[:, 2, 1] ** 2)
    return L


def _solve3(L, B):
    """V^-1 B for V = L L^T; L (n, 3, 3), B (n, 3, k)."""
    y0 = B[:, 0] / L[:, 0, 0, None]
    y1 = (B[:, 1] - L[:, 1, 0, None] * y0) / L[:, 1, 1, None]
    y2 = (B[:, 2] - L[:, 2, 0, None] * y0 - L[:, 2, 1, None] * y1) / L[:, 2, 2, None]
    z2 = y2 / L[:, 2, 2, None]
    z1 = (y1 - L[:, 2, 1, None] * z2) / L[:, 1, 1, None]
    z0 = (y0 - L[:, 1, 0, None] * z1 - L[:, 2, 0, None] * z2) / L[:, 0, 0, None]
    return np.stack([z0, z1, z2], axis=1)


def refined_solve(A, b, tol=2.0 ** -60, max_steps=12):
    """A y = b in longdouble from an fp64 LAPACK Cholesky factor of fl64(A):
    iterative refinement with chol_ref's compensated longdouble residuals of
    the unrounded A, until max|correction| <= tol max|y|.  -> (y, steps)."""
    import scipy.linalg as sl
    A = np.asarray(A, LD)
    b = np.asarray(b, LD)
    cf = sl.cho_factor(np.asarray(A, np.float64), lower=True)
    y = np.asarray(sl.cho_solve(cf, np.asarray(b, np.float64)), LD)
    for k in range(max_steps):
        r = R._ld_residual(A, y, b)
        # the residual is far below fp64's range of b: scale it to keep its leading bits
        s = np.max(np.abs(r))
        if s == 0:
            return y, k
        d = np.asarray(sl.cho_solve(cf, np.asarray(r / s, np.float64)), LD) * s
        y = y + d
        if np.max(np.abs(d)) <= tol * np.max(np.abs(y)):
            return y, k + 1
    raise AssertionError("iterative refinement did not converge")


def dense_solve(A, b, dtype, force=None):
    """The reduced system's solve: longdouble by ref_solve or refined_solve
    (by size, or as `force` = "ref" / "refined" says), fp64 by LAPACK."""
    n = A.shape[0]
    if n == 0:
        return np.zeros(0, dtype)
    if dtype is not LD:
        import scipy.linalg as sl
        return sl.cho_solve(sl.cho_factor(A, lower=True), b)
    how = force or ("ref" if n <= DENSE_LD_MAX else "refined")
    if how == "ref":
        y, bad = R.ref_solve(A, b)
        assert y is not None, f"pivot {bad} of the reduced system is not positive"
        return y
    return refined_solve(A, b)[0]


# ---- the problem --------------------------------------------------------------
def problem(uv, cam_idx, pt_idx, K, mode=STRUCT_AND_POSE, **options):
    o = dict(OPTIONS)
    o.update(options)
    return SimpleNamespace(uv=np.asarray(uv, np.float64), cam=np.asarray(cam_idx, np.int64),
                           pt=np.asarray(pt_idx, np.int64), K=np.asarray(K, np.float64).reshape(-1, 9), mode=mode,
                           opt=SimpleNamespace(**o))


def _scatter(idx, vals, n):
    out = np.zeros((n,) + vals.shape[1:], vals.dtype)
    np.add.at(out, idx, vals)
    return out


def jacobi_scale(pb, x, dtype):
    """(scale_c (C, 6), scale_p (P, 3)) at x; 1 where a block has no observation."""
    C, P = np.shape(x[0])[0], np.shape(x[2])[0]
    _, jac = residuals_jacobians(pb, x, dtype)
    sq = (jac * jac).sum(axis=1)
    one = dtype(1)
    return one / (one + np.sqrt(_scatter(pb.cam, sq[:, :6], C))), one / (one + np.sqrt(_scatter(pb.pt, sq[:, 6:], P)))


def same_point_pairs(pt):
    """All ordered pairs (i, j), i = j included, of observations of one point."""
    order = np.argsort(pt, kind="stable")
    p = pt[order]
    first = np.searchsorted(p, p, side="left")
    cnt = np.searchsorted(p, p, side="right") - first
    i = np.repeat(np.arange(len(p)), cnt)
    j = np.arange(len(i)) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(first, cnt)
    return order[i], order[j]


def _gradient_max(pb, jac, res, act_c, act_p):
    """max |J^T res| over the active parameters (J unscaled) and the
    condition number of that component's sum to roundings of its terms:
    sum |J_ij| (|projection_i| + |uv_i|) / |g_j|.  The residual is itself a
    difference of two numbers of the image's size, so an fp64 residual carries
    u (|projection| + |uv|), not u |res|: near the optimum, and for a single
    component that three yardsticks with the same camera-side residual all hit
    alike, sum |J| |res| would understate what correct fp64 code may lose."""
    C, P = len(act_c), len(act_p)
    g = np.concatenate([(_scatter(pb.cam, np.einsum("nrk,nr->nk", jac[:, :, :6], res), C) * act_c[:, None]).ravel(),
                        (_scatter(pb.pt, np.einsum("nrk,nr->nk", jac[:, :, 6:], res), P) * act_p[:, None]).ravel()])
    k = int(np.argmax(np.abs(g)))
    uv = np.abs(np.asarray(pb.uv, res.dtype))
    size = np.abs(res + np.asarray(pb.uv, res.dtype)) + uv
    a = np.concatenate([_scatter(pb.cam, np.einsum("nrk,nr->nk", np.abs(jac[:, :, :6]), size), C).ravel(),
                        _scatter(pb.pt, np.einsum("nrk,nr->nk", np.abs(jac[:, :, 6:]), size), P).ravel()])
    gm = np.abs(g[k])
    return gm, (float(a[k] / gm) if gm > 0 else 1.0)


def lm_step(pb, x0, x, radius, dtype=LD, decrease_factor=2.0, scale=None, fault=None, force_solver=None,
            dense_full=False, split_residual=False):
    """One LM step from x = (rot, t, X) with the scale of x0 (or `scale` as
    given).  dense_full: solve the full damped normal equations densely
    instead of through the Schur complement (small scenes only).
    split_residual: the model of the record-free passes (see the module's
    text): the point-side sum E^T res takes its residuals from
    residuals_matrix_form, the camera side from the functor."""
    o, mode, cam, pt = pb.opt, pb.mode, pb.cam, pb.pt
    C, P, N = np.shape(x[0])[0], np.shape(x[2])[0], len(pb.cam)
    cams_var, pts_var = mode != STRUCT_ONLY, mode != POSE_ONLY
    act_c = (np.bincount(cam, minlength=C) > 0) & cams_var
    act_p = (np.bincount(pt, minlength=P) > 0) & pts_var
    sc, sp = scale if scale is not None else jacobi_scale(pb, x0, dtype)
    sc, sp = np.asarray(sc, dtype), np.asarray(sp, dtype)
    rad = dtype(radius)

    res, jac = residuals_jacobians(pb, x, dtype)
    cost = (res * res).sum() / 2
    F = jac[:, :, :6] * sc[cam][:, None, :] * act_c[cam][:, None, None]       # (N, 2, 6); zero where constant
    E = jac[:, :, 6:] * sp[pt][:, None, :] * act_p[pt][:, None, None]         # (N, 2, 3)
    grad_max, grad_cond = _gradient_max(pb, jac, res, act_c, act_p)

    dc = _scatter(cam, (F * F).sum(axis=1), C)
    dp = _scatter(pt, (E * E).sum(axis=1), P)
    for d, act in ((dc, act_c), (dp, act_p)):
        live = d[act]
        assert live.size == 0 or (live.min() > 2 * o.min_lm_diagonal and live.max() < o.max_lm_diagonal / 2), \
            "a scaled diagonal entry lies within a factor 2 of a clamp: the step depends on the scale"
    Dc = np.clip(dc, dtype(o.min_lm_diagonal), dtype(o.max_lm_diagonal)) / rad
    Dp = np.clip(dp, dtype(o.min_lm_diagonal), dtype(o.max_lm_diagonal)) / rad
    if fault and fault[0] == "no_damping":
        Dc[fault[1]] = 0
    gc = _scatter(cam, np.einsum("nrk,nr->nk", F, res), C)
    gp = _scatter(pt, np.einsum("nrk,nr->nk", E, residuals_matrix_form(pb, x, dtype) if split_residual else res), P)
    eye3, eye6 = np.eye(3, dtype=dtype), np.eye(6, dtype=dtype)
    U = _scatter(cam, np.einsum("nra,nrb->nab", F, F), C) + Dc[:, :, None] * eye6
    EtE = _scatter(pt, np.einsum("nra,nrb->nab", E, E), P)
    V = EtE + Dp[:, :, None] * eye3
    V[~act_p] = eye3
    ca = np.flatnonzero(act_c)
    slot = np.full(C, -1, np.int64)
    slot[ca] = np.arange(len(ca))
    nc = 6 * len(ca)
    yc, yp = np.zeros((C, 6), dtype), np.zeros((P, 3), dtype)

    if dense_full:
        pa = np.flatnonzero(act_p)
        pslot = np.full(P, -1, np.int64)
        pslot[pa] = np.arange(len(pa))
        n = nc + 3 * len(pa)
        Jd = np.zeros((2 * N, n), dtype)
        rows = np.arange(2 * N).reshape(N, 2)
        for k in range(6):
            ok = act_c[cam]
            Jd[rows[ok], (6 * slot[cam[ok]] + k)[:, None]] = F[ok, :, k]
        for k in range(3):
            ok = act_p[pt]
            Jd[rows[ok], (nc + 3 * pslot[pt[ok]] + k)[:, None]] = E[ok, :, k]
        H = Jd.T @ Jd + np.diag(np.concatenate([Dc[ca].ravel(), Dp[pa].ravel()]))
        y = dense_solve(H, -(Jd.T @ res.ravel()), dtype, force="ref" if dtype is LD else None)
        yc[ca] = y[:nc].reshape(-1, 6)
        yp[pa] = y[nc:].reshape(-1, 3)
    else:
        Lp = _chol3(V)
        if fault and fault[0] == "stale_point":
            p, r_old = fault[1], dtype(fault[2])
            Vs = (EtE[p] + np.diag(np.clip(dp[p], dtype(o.min_lm_diagonal), dtype(o.max_lm_diagonal)) / r_old))[None]
            Lp[p] = _chol3(Vs)[0]
        W = np.einsum("nra,nrb->nab", F, E)                                    # (N, 6, 3): F^T E per observation
        if nc and pts_var:
            T = np.swapaxes(_solve3(Lp[pt], np.swapaxes(W, 1, 2)), 1, 2)       # W V^-1
            i, j = same_point_pairs(pt)
            keep = act_c[cam[i]] & act_c[cam[j]]
            if fault and fault[0] == "pair":
                a, b = fault[1], fault[2]
                assert pt[a] == pt[b] and cam[a] != cam[b]
                keep &= ~(((i == a) & (j == b)) | ((i == b) & (j == a)))
            i, j = i[keep], j[keep]
            S4 = np.zeros((len(ca), 6, len(ca), 6), dtype)
            S4[np.arange(len(ca)), :, np.arange(len(ca)), :] = U[ca]
            np.subtract.at(S4, (slot[cam[i]], slice(None), slot[cam[j]], slice(None)), np.einsum("nab,ncb->nac", T[i], W[j]))
            rhs = -(gc - _scatter(cam, np.einsum("nab,nb->na", T, gp[pt]), C))[ca]
            S = S4.reshape(nc, nc)
            yc[ca] = dense_solve((S + S.T) / 2, rhs.ravel(), dtype, force_solver).reshape(-1, 6)
        elif nc:
            S = np.zeros((len(ca), 6, len(ca), 6), dtype)
            S[np.arange(len(ca)), :, np.arange(len(ca)), :] = U[ca]
            yc[ca] = dense_solve(S.reshape(nc, nc), -gc[ca].ravel(), dtype, force_solver).reshape(-1, 6)
        if pts_var:
            back = np.einsum("nab,na->nb", W, yc[cam])                        # W^T y_c per observation
            if fault and fault[0] == "backsub_obs":
                back[fault[1]] = 0
            yp = _solve3(Lp, (-gp - _scatter(pt, back, P))[:, :, None])[:, :, 0] * act_p[:, None]

    dcam, dpt = yc * sc * act_c[:, None], yp * sp * act_p[:, None]
    out = SimpleNamespace(delta_c=dcam, delta_p=dpt, scale_c=sc, scale_p=sp, act_c=act_c, act_p=act_p, cost=cost,
                          gradient_max_norm=grad_max, gradient_cond=grad_cond, radius_in=float(radius))
    out.step_norm = np.sqrt((dcam * dcam).sum() + (dpt * dpt).sum())
    mr = np.einsum("nrk,nk->nr", F, yc[cam]) + np.einsum("nrk,nk->nr", E, yp[pt])
    terms = mr * (res + mr / 2)
    out.model_cost_change = -terms.sum()
    out.model_cond = float(np.abs(terms).sum() / abs(out.model_cost_change)) if out.model_cost_change != 0 else np.inf
    out.step_is_valid = bool(np.all(np.isfinite(np.asarray(dcam, np.float64))) and np.all(np.isfinite(np.asarray(dpt, np.float64)))
                             and out.model_cost_change >= 0)
    # the candidate: the solver's parameters are fp64, so x_new is x + delta rounded once
    rot, t, X = x
    xc = np.asarray(np.hstack([np.asarray(rot, LD), np.asarray(t, LD)]) + np.asarray(dcam, LD), np.float64)
    xn = (np.ascontiguousarray(xc[:, :3]), np.ascontiguousarray(xc[:, 3:]),
          np.asarray(np.asarray(X, LD) + np.asarray(dpt, LD), np.float64))
    out.x_new = xn
    rn, jn = residuals_jacobians(pb, xn, dtype)
    out.new_cost = (rn * rn).sum() / 2
    out.cost_change = cost - out.new_cost
    out.cost_change_cond = float((cost + out.new_cost) / abs(out.cost_change)) if out.cost_change != 0 else np.inf
    out.relative_decrease = out.cost_change / out.model_cost_change
    out.step_is_successful = bool(out.step_is_valid and out.relative_decrease > o.min_relative_decrease)
    rho = out.relative_decrease
    if out.step_is_successful:
        q = 2 * rho - 1
        den = 1 - q * q * q
        third = dtype(1) / 3
        out.radius = min(dtype(o.max_trust_region_radius), rad / max(third, den))
        # d ln(radius) / d ln(rho), for the radius's floor
        out.radius_cond = float(abs(6 * q * q * rho / den)) if den > third and out.radius < o.max_trust_region_radius else 0.0
        out.new_gradient_max_norm, out.new_gradient_cond = _gradient_max(pb, jn, rn, act_c, act_p)
    else:
        out.radius = rad / dtype(decrease_factor)
        out.radius_cond = 0.0
        out.new_gradient_max_norm, out.new_gradient_cond = grad_max, grad_cond
    return out


# ---- the statistic -----------------------------------------------------------
def block_errors(d_c, d_p, ref):
    """Per parameter block, in scaled units delta / scale: the 2-norm of the
    error against `ref` (an lm_step result) and the block's yardstick norm
    max(|ref block|, RMS block norm of its kind over the active blocks).
    -> ((err_c, den_c), (err_p, den_p)), longdouble arrays over all blocks."""
    out = []
    for d, r, s, act in ((d_c, ref.delta_c, ref.scale_c, ref.act_c), (d_p, ref.delta_p, ref.scale_p, ref.act_p)):
        r = np.asarray(r, LD) / np.asarray(s, LD)
        e = np.asarray(d, LD) / np.asarray(s, LD) - r
        en, rn = np.sqrt((e * e).sum(axis=1)), np.sqrt((r * r).sum(axis=1))
        rms = np.sqrt((rn[act] ** 2).mean()) if act.any() else LD(1)
        out.append((en, np.maximum(rn, rms)))
    return out


def step_error(d_c, d_p, ref):
    """(cameras, points): max over blocks of error / yardstick norm."""
    return tuple(float((e / n).max()) if len(e) else 0.0 for e, n in block_errors(d_c, d_p, ref))


def delta_of(x_new, x):
    """x_new - x in longdouble -> (delta_c (C, 6), delta_p (P, 3))."""
    (r1, t1, X1), (r0, t0, X0) = x_new, x
    ld = lambda a: np.asarray(a, LD)
    return np.hstack([ld(r1) - ld(r0), ld(t1) - ld(t0)]), ld(X1) - ld(X0)


YARD_FLOOR = U64   # no fp64 result is a finer yardstick than one rounding


def delta_ratio(x_new, x, ref, yard_c, yard_p):
    """The device's step against its cap, per kind of block: max over blocks of
    error / (8 x the worse yardstick's statistic x the block's yardstick norm
    + the read-back floor u |x_new| / scale of the block, in the 2-norm)."""
    d_c, d_p = delta_of(x_new, x)
    xn_c = np.hstack([np.abs(x_new[0]), np.abs(x_new[1])])
    out = []
    for (e, n), yard, xa, s in zip(block_errors(d_c, d_p, ref), (yard_c, yard_p), (xn_c, np.abs(x_new[2])),
                                   (ref.scale_c, ref.scale_p)):
        fl = U64 * np.asarray(xa, LD) / np.asarray(s, LD)
        allowed = 8 * max(yard, YARD_FLOOR) * n + np.sqrt((fl * fl).sum(axis=1))
        out.append(float((e / allowed).max()) if len(e) else 0.0)
    return tuple(out)


SCALARS = ("cost", "cost_change", "step_norm", "relative_decrease", "trust_region_radius", "gradient_max_norm")


def scalar_refs(ref):
    """name -> (reference value, condition number of the floor) for trace[k]."""
    rho_cond = ref.cost_change_cond + ref.model_cond
    return {"cost": (ref.new_cost if ref.step_is_successful else ref.cost, 1.0),
            "cost_change": (ref.cost_change, ref.cost_change_cond),
            "step_norm": (ref.step_norm, 1.0),
            "relative_decrease": (ref.relative_decrease, rho_cond),
            "trust_region_radius": (ref.radius, 1.0 + ref.radius_cond * rho_cond),
            "gradient_max_norm": (ref.new_gradient_max_norm, ref.new_gradient_cond)}


def scalar_ratio(value, ref_value, cond, yard_values):
    """|value - ref| / (8 x the worse yardstick's error + 4 u cond |ref|)."""
    rv = LD(ref_value)
    worst = max(abs(LD(y) - rv) for y in yard_values) if yard_values else LD(0)
    cap = 8 * worst + 4 * U64 * cond * abs(rv)
    err = abs(LD(value) - rv)
    return float(err / cap) if cap > 0 else (0.0 if err == 0 else np.inf)
