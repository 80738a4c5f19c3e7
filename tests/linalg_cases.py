"""Seeded cases for the geometry kernels' small linear algebra (the testing
hook sfm_linalg_probe and sfm_triangulate_points), with their longdouble
references, yardstick errors and caps -- all computed on the CPU, from correct
fp64 code alone (tests/linalg_ref.py states the metrics).

Every op x family holds K different problems; a device batch of any size
deals them out with a stride (deal), so adjacent lanes and waves never hold
the same matrix.

Caps.  Two correct fp64 codes are the yardsticks: the oracle's restatement
of OpenCV (oracle.pnp_oracle cv_svd / cv_svbksb / qr_solve /
triangulate_points: the kernels' algorithm) and LAPACK through numpy (another
algorithm).  cap = 8 x the worst yardstick error of the op and family + a
floor of eps x the quantity's condition number: the vector metrics and the
triangulated point are already divided by their condition number
(sigma_1 / gap, and that through the division by h), so their floor is eps;
x of a least-squares solve has the floor eps sigma_1 / sigma_kept_min.

Not tested: whole-matrix scales beyond 1e-60 .. 1e60.  The rotation's
sqrt(a * b) needs a * b inside the fp64 range; past it OpenCV itself
overflows or underflows, and the kernels restate that faithfully.
"""
import functools
import zlib

import numpy as np

import linalg_ref as R
from oracle import pnp_oracle as P

LD = np.longdouble
EPS = R.EPS
K = 6   # problems per op x family

SVD_OPS = {"svd3x3": (3, 3), "svd4x4": (4, 4), "svd9x9": (9, 9), "svd6x3": (6, 3), "svd6x4": (6, 4),
           "svd6x5": (6, 5), "svd_at9x7": (9, 7)}
SVD_FAMILIES = ["gaussian", "graded", "rank1", "rank2", "repeated", "orthogonal", "late_pairs", "beta_signs",
                "scale_small", "scale_large"]
SVD12_FAMILIES = ["epnp_general", "epnp_planar", "epnp_collinear", "tie", "zero", "gaussian", "graded", "dup",
                  "repeated", "orthogonal", "late_pairs", "beta_signs", "scale_small", "scale_large"]
# The path of cv_svd12_lanes each problem takes (fast: every W distinct and
# > DBL_MIN; slow: the sort and the completion): one entry for the whole
# family, or one per problem.  Coplanar points leave three columns of M empty:
# exact zeros, completed from the RNG.  "repeated" has exactly repeated values
# (its entries are dyadic, so the matrix is the same on every machine), and
# whether the sweeps leave an exact tie in W differs by problem.  The
# duplicated row and column of "dup" (a Gram matrix summed in a fixed order)
# end at exactly 0.  tests/test_linalg_ref.py asserts the listed paths.
REPEATED_PATHS = ["fast", "slow", "fast", "slow", "slow", "slow"]
SVD12_PATH = {"epnp_general": "fast", "epnp_planar": "slow", "epnp_collinear": "slow", "tie": "slow", "zero": "slow",
              "gaussian": "fast", "graded": "fast", "dup": "slow", "repeated": REPEATED_PATHS,
              "orthogonal": "fast", "late_pairs": "fast", "beta_signs": "fast", "scale_small": "fast",
              "scale_large": "fast"}
LSTSQ_OPS = {"lstsq6x3": 3, "lstsq6x4": 4, "lstsq6x5": 5}
LSTSQ_FAMILIES = ["well", "dropped", "kept"]
QR_FAMILIES = ["gaussian", "neg_diag", "eta0", "graded"]
WAVE_OPS = ["svd6x4", "svd6x5", "lstsq6x4", "lstsq6x5"]   # ops with a variant 1 beside variant 0
BETA_PATTERN = [1.0, 3.0, 3.0, 1.0]   # column scales: |col 0| < |col 1|, |col 2| > |col 3| (odd problems: reversed)


def families(op):
    if op in SVD_OPS:
        return SVD_FAMILIES
    if op in LSTSQ_OPS:
        return LSTSQ_FAMILIES
    return QR_FAMILIES if op == "qr6x4" else SVD12_FAMILIES


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _orth(rng, m, n):
    q, _ = np.linalg.qr(rng.standard_normal((m, n)))
    return q


def _svd_matrix(family, M, N, k, rng):
    if family in ("gaussian", "scale_small", "scale_large"):
        return rng.standard_normal((M, N)) * {"gaussian": 1.0, "scale_small": 1e-60, "scale_large": 1e60}[family]
    if family == "graded":
        return rng.standard_normal((M, N)) * rng.permutation(np.logspace(-6, 6, N))
    if family in ("rank1", "rank2"):
        A = rng.standard_normal((M, N))
        z = k % N
        if family == "rank2" or k % 2 == 0:
            A[:, z] = 0.0                                # W = 0 exactly: the RNG completion
        if family == "rank2" or k % 2 == 1:
            A[:, (z + 2) % N] = A[:, (z + 1) % N]        # a duplicated column
        return A
    if family == "repeated":
        return (_orth(rng, M, N) * 2.0 ** -(np.arange(N) // 2)) @ _orth(rng, N, N).T
    if family == "orthogonal":                           # no pair turns: the sweeps are empty
        A = np.zeros((M, N))
        A[rng.permutation(M)[:N], np.arange(N)] = rng.permutation(np.arange(1.0, N + 1)) * rng.choice([-1.0, 1.0], N)
        return A
    if family == "late_pairs":                           # only the last pair of a sweep turns
        A = np.zeros((M, N))
        A[np.arange(N - 2), np.arange(N - 2)] = np.arange(3.0, N + 1)
        A[N - 2:, N - 2:] = rng.standard_normal((M - N + 2, 2))
        return A
    if family == "beta_signs":                           # W_0 - W_1 and W_2 - W_3 of opposite signs
        A = rng.standard_normal((M, N))
        return A / np.linalg.norm(A, axis=0) * np.array([BETA_PATTERN[(j + 2 * (k % 2)) % 4] * (1.0 + 0.37 * (j // 4))
                                                         for j in range(N)])
    raise KeyError(family)


def _epnp_mtm(kind, rng):
    """M^T M of EPnP for 5 points (general / coplanar / on one image line)."""
    if kind == "epnp_planar":
        pw = np.c_[rng.uniform(-1, 1, (5, 2)), np.zeros(5)]
    elif kind == "epnp_collinear":                       # on a plane through the camera centre
        pw = np.c_[rng.uniform(-1, 1, 5), np.zeros(5), rng.uniform(-1, 1, 5)]
    else:
        pw = rng.uniform(-1, 1, (5, 3))
    c0 = pw.mean(0)
    _, s, vt = np.linalg.svd(pw - c0)
    cws = np.vstack([c0, c0 + np.sqrt(s[:3, None] ** 2 / 5) * vt[:3]])
    al = (pw - c0) @ np.linalg.pinv((cws[1:] - c0).T).T
    alpha = np.c_[1 - al.sum(1), al]
    th = rng.uniform(-0.2, 0.2, 3)
    Rm = np.array(P.rodrigues_v2m(th)).reshape(3, 3)
    t = np.array([0.1, -0.2, 6.0]) if kind != "epnp_collinear" else np.array([0.1, 0.0, 6.0])
    if kind == "epnp_collinear":
        Rm = np.array(P.rodrigues_v2m([0.0, th[1], 0.0])).reshape(3, 3)   # keeps y = 0 in the camera
    pc = pw @ Rm.T + t
    fu, fv, uc, vc = 800.0, 790.0, 320.0, 240.0
    u, v = fu * pc[:, 0] / pc[:, 2] + uc, fv * pc[:, 1] / pc[:, 2] + vc
    Mm = np.zeros((10, 12))
    for p in range(5):
        for j in range(4):
            Mm[2 * p, 3 * j], Mm[2 * p, 3 * j + 2] = alpha[p, j] * fu, alpha[p, j] * (uc - u[p])
            Mm[2 * p + 1, 3 * j + 1], Mm[2 * p + 1, 3 * j + 2] = alpha[p, j] * fv, alpha[p, j] * (vc - v[p])
    G = Mm.T @ Mm
    return (G + G.T) * 0.5


def _gram(G):
    """G^T G summed row by row in a fixed order (no BLAS: the same bits on
    every machine), exactly symmetric."""
    S = np.zeros((G.shape[1], G.shape[1]))
    for r in G:
        S = S + r[:, None] * r[None, :]
    return S


def _svd12_matrix(family, k, rng):
    if family.startswith("epnp"):
        return _epnp_mtm(family, rng)
    if family in ("gaussian", "scale_small", "scale_large", "zero", "graded", "dup", "beta_signs"):
        G = rng.standard_normal((12, 12))
        if family == "zero":
            G[:, (5 * k) % 12] = 0.0                     # a zero row and column: W = 0 exactly
        if family == "dup":
            G[:, (5 * k + 3) % 12] = G[:, (5 * k) % 12]  # a duplicated row and column: rank 11
        S = _gram(G)
        if family == "graded":                           # D G^T G D: entries graded over 1e-6 .. 1e6
            d = rng.permutation(np.logspace(-3, 3, 12))
            S = S * (d[:, None] * d[None, :])
        if family == "beta_signs":                       # row norms small, large, large, small, ...
            d = np.array([BETA_PATTERN[(j + 2 * (k % 2)) % 4] for j in range(12)])
            S = S * (d[:, None] * d[None, :])
        return S * {"scale_small": 1e-60, "scale_large": 1e60}.get(family, 1.0)
    if family == "repeated":
        # Q diag(2^-(i // 2)) Q with the Householder reflector Q = I - v v^T / 8,
        # |v|^2 = 16: every entry and every partial sum is a short dyadic
        # number, so the product is exact, symmetric and the same everywhere
        v = np.array([1.0] * 8 + [2.0] * 2 + [0.0] * 2)[rng.permutation(12)] * rng.choice([-1.0, 1.0], 12)
        Q = np.eye(12) - np.outer(v, v) / 8
        S = (Q * 2.0 ** -(np.arange(12) // 2)) @ Q
        assert np.array_equal(S, S.T)
        return S
    D = np.diag(rng.permutation(np.arange(1.0, 13.0)))
    if family == "orthogonal":
        return D
    if family == "late_pairs":                           # tests/test_pnp_svd_schedule.py's edge case
        D = np.diag(np.arange(1.0, 13.0))
        D[9, 11] = D[11, 9] = 0.5 + 0.01 * k
        D[10, 11] = D[11, 10] = 0.25
        return D
    if family == "tie":                                  # two rows no rotation touches, equal norms
        D = np.diag(np.arange(1.0, 13.0))
        D[k % 8, k % 8] = D[k % 8 + 1, k % 8 + 1]
        D[9, 11] = D[11, 9] = 0.5
        D[10, 11] = D[11, 10] = 0.25
        return D
    raise KeyError(family)


def _lstsq_problem(family, N, k, rng):
    """A [6][N] | b [6].  dropped / kept: the last column is sigma e_5, exactly
    orthogonal to the others (which leave row 5 empty), so the singular value
    sigma = 1e-3 / 1e3 of the threshold 2 eps sum(w) is met exactly."""
    A = rng.standard_normal((6, N))
    if family != "well":
        A[5, :] = 0.0
        A[:, N - 1] = 0.0
        thr = 2 * EPS * np.linalg.svd(A, compute_uv=False).sum()
        A[5, N - 1] = thr * (1e-3 if family == "dropped" else 1e3)
    return np.r_[A.ravel(), rng.standard_normal(6)]


def _qr_problem(family, k, rng):
    A = rng.standard_normal((6, 4))
    if family == "neg_diag":
        A[0, 0] = -abs(A[0, 0]) - 1.0
        A[1:, 1:] -= 2.0 * np.eye(5, 3)
    elif family == "eta0":
        A[:, k % 4] = 0.0                                # stays zero through the earlier columns' updates
    elif family == "graded":
        A = A * rng.permutation(np.array([1e-6, 1e-2, 1e2, 1e6]))
    return np.r_[A.ravel(), rng.standard_normal(6), np.array([7.25, -3.5, 11.0, 0.125]) + k]


@functools.lru_cache(maxsize=None)
def problems(op, family):
    """[K][doubles in] in sfm_linalg_probe's input layout."""
    out = []
    for k in range(K):
        rng = _rng(op, family, k)
        if op in SVD_OPS:
            out.append(_svd_matrix(family, *SVD_OPS[op], k, rng).ravel())
        elif op == "svd12":
            out.append(_svd12_matrix(family, k, rng).ravel())
        elif op in LSTSQ_OPS:
            out.append(_lstsq_problem(family, LSTSQ_OPS[op], k, rng))
        else:
            out.append(_qr_problem(family, k, rng))
    a = np.array(out)
    a.setflags(write=False)
    return a


def deal(n):
    """Which of the K problems each of n batch slots holds: neighbours differ."""
    return (np.arange(n) * 5 + 1) % K


# ---- the oracle in the probe's output layout (bit identity 2) --------------
def _pack_svd(w, U, Vt=None):
    return np.r_[w, np.asarray(U).T.ravel(), [] if Vt is None else np.asarray(Vt).ravel()]


@functools.lru_cache(maxsize=None)
def oracle_out(op, family):
    out = []
    for row in problems(op, family):
        if op in SVD_OPS:
            M, N = SVD_OPS[op]
            w, U, Vt = P.cv_svd(row.reshape(M, N))
            out.append(_pack_svd(w, U, None if op == "svd_at9x7" else Vt))
        elif op == "svd12":
            _, U, _ = P.cv_svd(row.reshape(12, 12).T, tree=True)
            out.append(U.T[[11, 10, 9, 8]].ravel())
        elif op in LSTSQ_OPS:
            N = LSTSQ_OPS[op]
            w, U, Vt = P.cv_svd(row[:6 * N].reshape(6, N))
            out.append(P.cv_svbksb(w, U, Vt, row[6 * N:]))
        else:
            x = P.qr_solve(row[:24].reshape(6, 4), row[24:30])
            out.append(np.r_[row[30:], 0.0] if x is None else np.r_[x, 1.0])
    a = np.array(out)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def oracle_w12(family):
    """The 12 singular values cv_svd12_lanes ranks (the oracle's, tree order)."""
    return np.array([P.cv_svd(r.reshape(12, 12).T, tree=True)[0] for r in problems("svd12", family)])


def svd12_path(w):
    return "slow" if len(set(w.tolist())) < 12 or np.any(w <= R.DBL_MIN) else "fast"


def numpy_out(op, family):
    """LAPACK's answer in the probe's output layout (a yardstick only)."""
    out = []
    for row in problems(op, family):
        if op in SVD_OPS:
            M, N = SVD_OPS[op]
            U, w, Vt = np.linalg.svd(row.reshape(M, N), full_matrices=False)
            out.append(_pack_svd(w, U, None if op == "svd_at9x7" else Vt))
        elif op == "svd12":
            U, _, _ = np.linalg.svd(row.reshape(12, 12).T)
            out.append(U.T[[11, 10, 9, 8]].ravel())
        elif op in LSTSQ_OPS:
            N = LSTSQ_OPS[op]
            U, w, Vt = np.linalg.svd(row[:6 * N].reshape(6, N), full_matrices=False)
            out.append(P.cv_svbksb(w, U, Vt, row[6 * N:]))     # the same truncation rule on LAPACK's factors
        else:
            A = row[:24].reshape(6, 4)
            if not A.any(0).all():
                out.append(np.r_[row[30:], 0.0])
            else:                                         # LAPACK's Householder QR (no scaling by eta)
                q, r = np.linalg.qr(A)
                out.append(np.r_[np.linalg.solve(r, q.T @ row[24:30]), 1.0])
    return np.array(out)


# ---- references, metrics, caps -----------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(op, family):
    pr = problems(op, family)
    if op in SVD_OPS:
        M, N = SVD_OPS[op]
        return R.ld_svd(pr.reshape(K, M, N))
    if op == "svd12":
        return R.ld_svd(pr.reshape(K, 12, 12).transpose(0, 2, 1))
    if op in LSTSQ_OPS:
        N = LSTSQ_OPS[op]
        return R.ld_lstsq(pr[:, :6 * N].reshape(K, 6, N), pr[:, 6 * N:])
    A = pr[:, :24].reshape(K, 6, 4)
    sig, U, V = R.ld_svd(A)
    ok = A.any(1).all(1)
    coef = np.einsum("kmn,km->kn", U, pr[:, 24:30].astype(LD)) / np.where(sig > 0, sig, LD(1))
    x = np.where(ok[:, None], np.einsum("kin,kn->ki", V, coef), pr[:, 30:].astype(LD))
    return x, ok, sig


def metrics(op, family, out, which=None):
    """Worst error per metric of `out` [n][doubles out] (slot i holds problem
    which[i]; default: the K problems in order) against the reference."""
    which = np.arange(K) if which is None else which
    ref, pr = reference(op, family), problems(op, family)
    worst = {}

    def fold(m):
        for name, v in m.items():
            worst[name] = max(worst.get(name, 0.0), float(v))

    cache = {}
    for i, k in enumerate(which):
        key = (int(k), out[i].tobytes())
        if key in cache:                                  # (a dealt batch repeats K problems)
            continue
        cache[key] = True
        o = out[i]
        if op in SVD_OPS:
            M, N = SVD_OPS[op]
            r = (ref[0][k], ref[1][k], ref[2][k])
            Vt = None if op == "svd_at9x7" else o[N + N * M:].reshape(N, N)
            fold(R.svd_metrics(pr[k].reshape(M, N), o[:N], o[N:N + N * M].reshape(N, M), Vt, r))
        elif op == "svd12":
            fold(R.svd12_metrics(pr[k].reshape(12, 12).T, o.reshape(4, 12), (ref[0][k], ref[1][k], ref[2][k])))
        elif op in LSTSQ_OPS:
            fold({"x": R.rel_err(o, ref[0][k])})
        else:
            x, ok, _ = ref
            fold({"x": R.rel_err(o[:4], x[k]), "flag": abs(o[4] - float(ok[k]))})
            if not ok[k]:
                fold({"untouched": float(np.any(o[:4] != pr[k][30:]))})
    return worst


def floors(op, family):
    """eps x the condition number of each metric's quantity."""
    if op in LSTSQ_OPS:
        _, kept, sig = reference(op, family)
        smin = np.where(kept, sig, np.inf).min(1)
        return {"x": EPS * float((sig[:, 0] / smin).max())}
    if op == "qr6x4":
        # Householder QR is indifferent to the columns' scales: its error
        # follows the condition number of the column-equilibrated matrix
        # (van der Sluis), not that of A
        _, ok, _ = reference(op, family)
        A = problems(op, family)[:, :24].reshape(K, 6, 4)
        c = [float(np.linalg.cond(a / np.linalg.norm(a, axis=0))) for a, o in zip(A, ok) if o]
        return {"x": EPS * max(c, default=1.0), "flag": 0.0, "untouched": 0.0}
    return {m: EPS for m in ("sv", "recon", "orthu", "orthv", "vecu", "vecv")}


@functools.lru_cache(maxsize=None)
def yardsticks(op, family):
    return {"oracle": metrics(op, family, oracle_out(op, family)), "numpy": metrics(op, family, numpy_out(op, family))}


@functools.lru_cache(maxsize=None)
def caps(op, family):
    y = yardsticks(op, family)
    fl = floors(op, family)
    return {m: 8 * max(y["oracle"][m], y["numpy"][m]) + fl[m] for m in y["oracle"]}


# ---- triangulation scenes (sfm_triangulate_points) ----------------------------
TRI_N = 300
TRI_SCENES = ["bd_1e-1", "bd_1e-2", "bd_1e-3", "bd_1e-4", "noise_1e-1", "noise_1e-3", "wide_P", "behind",
              "h_tiny", "same_cam"]


def _look(Rm, C):
    return np.c_[Rm, -Rm @ C]


@functools.lru_cache(maxsize=None)
def tri_scene(name):
    """-> dict(P [2][3][4], cam0, cam1, uv0, uv1 [n][2], X_true, ratio, noise)."""
    rng = _rng("tri", name)
    n = TRI_N
    Kc = np.array([[800.0, 0, 320], [0, 790.0, 240], [0, 0, 1]])
    depth, ratio, noise = 10.0, 0.1, 0.0
    Rm = np.array(P.rodrigues_v2m([0.0, -0.01, 0.002])).reshape(3, 3)
    X = np.c_[rng.uniform(-2, 2, (n, 2)), rng.uniform(8, 12, n)]
    if name.startswith("bd_") or name.startswith("noise_"):
        ratio = float(name.split("_")[1])
        noise = 0.3 if name.startswith("noise_") else 0.0
    C1 = np.array([ratio * depth, 0.0, 0.0])
    if name == "wide_P":
        Kc = np.array([[12000.0, 0, 4000], [0, 11500.0, 3000], [0, 0, 1]])
    if name == "behind":                                 # the second camera stands past the points
        C1 = np.array([1.0, 0.0, 20.0])
    if name == "h_tiny":                                 # |X| = 1e6: h = 1e-6 of the unit singular vector
        X = X / np.linalg.norm(X, axis=1, keepdims=True) * 1e6
        C1 = np.array([1.0, 0.0, 0.0])
    Pm = np.stack([Kc @ _look(np.eye(3), np.zeros(3)), Kc @ _look(Rm, C1)])
    cam0, cam1 = np.zeros(n, np.int32), np.ones(n, np.int32)
    if name == "same_cam":
        cam1 = np.zeros(n, np.int32)
    Xh = np.c_[X, np.ones(n)]
    uv = []
    for c in (cam0, cam1):
        x = np.einsum("nij,nj->ni", Pm[c], Xh)
        uv.append(x[:, :2] / x[:, 2:] + noise * rng.standard_normal((n, 2)))
    return {"P": Pm, "cam0": cam0, "cam1": cam1, "uv0": np.ascontiguousarray(uv[0]),
            "uv1": np.ascontiguousarray(uv[1]), "X": X, "ratio": ratio, "noise": noise, "C1": C1,
            "K": Kc, "R1": Rm, "t1": -Rm @ C1}


@functools.lru_cache(maxsize=None)
def tri_reference(name):
    s = tri_scene(name)
    return R.ld_triangulate(s["P"][s["cam0"]], s["P"][s["cam1"]], s["uv0"], s["uv1"])


@functools.lru_cache(maxsize=None)
def tri_oracle(name):
    s = tri_scene(name)
    return P.triangulate_points(s["cam0"], s["cam1"], s["uv0"], s["uv1"], s["P"])


def tri_numpy(name):
    s = tri_scene(name)
    As = R.tri_system(s["P"][s["cam0"]], s["P"][s["cam1"]], s["uv0"], s["uv1"], np.float64)
    v = np.linalg.svd(As)[2][:, 3]
    return v[:, :3] / v[:, 3:]


def tri_error(name, X):
    """Worst relative error of the points X over their condition number."""
    Xr, _, cond = tri_reference(name)
    return float(np.max(R.rel_err(X, Xr) / cond))


@functools.lru_cache(maxsize=None)
def tri_cap(name):
    y = {"oracle": tri_error(name, tri_oracle(name)), "numpy": tri_error(name, tri_numpy(name))}
    return 8 * max(y.values()) + EPS, y
