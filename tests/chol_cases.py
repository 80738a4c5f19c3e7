"""Deterministic systems for the dense Cholesky tests (tests/chol_ref.py is
the arithmetic): SPD families x sizes x right-hand sides, the layout
contract, and non-SPD matrices paired with the pivot that must fail.

Every random draw comes from default_rng([seed, n]); nothing here imports
the GPU package.
"""
import functools

import numpy as np

from tests import chol_ref as R

NB = 64
FAMILIES = ("well", "graded6", "graded10", "scaled")
# tile structure: ld = 64 ceil((n + 1) / 64), nblk = ld / 64.  1..3: tiny;
# 63/64/65, 127/128/129: the one- and two-tile edges (k_chol_small up to
# nblk = 2, i.e. n <= 127); 191/192: nblk = 3 -> 4 (the first r = 3 helper
# tile); 255/256/257: nblk = 4 -> 5 (the first helper pair); 320/321:
# nblk = 6 (a pair plus a trailing single); 384: nblk = 7.  Every multiple of
# 64 leaves the augmented row alone in the last tile.
SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 255, 256, 257, 320, 321, 384)
RHS = ("random", "A1", "zero", "big")
_SEED = {"well": 11, "graded6": 12, "graded10": 13, "scaled": 14}


def matrix(family, n):
    """The family's SPD matrix (full symmetric, fp64)."""
    rng = np.random.default_rng([_SEED[family], n])
    if family == "well":
        M = rng.standard_normal((n, n))
        return M @ M.T + n * np.eye(n)
    if family in ("graded6", "graded10"):
        k = 6 if family == "graded6" else 10
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        A = (Q * np.logspace(0, -k, n)) @ Q.T
        return 0.5 * (A + A.T)
    if family == "scaled":
        M = rng.standard_normal((n, n))
        D = 10.0 ** rng.uniform(-3, 3, n)
        A = (M @ M.T + n * np.eye(n)) * D[:, None] * D[None, :]
        return 0.5 * (A + A.T)
    raise ValueError(family)


def rhs_block(family, n, A):
    """(n, 4): the four right-hand sides, in RHS order."""
    rng = np.random.default_rng([_SEED[family] + 100, n])
    r0 = rng.standard_normal(n)
    r3 = rng.standard_normal(n) * 1e8
    return np.stack([r0, A @ np.ones(n), np.zeros(n), r3], axis=1)


def spd_ids():
    return [(f, n) for f in FAMILIES for n in SIZES]


@functools.lru_cache(maxsize=None)
def spd_case(family, n):
    """One matrix with its four right-hand sides and everything the tests
    compare against, computed once per process and never modified:
    dict(A, B (n, 4), Y (n, 4) longdouble, caps [(cap_fwd, cap_bwd, four)])."""
    A = matrix(family, n)
    B = rhs_block(family, n, A)
    Y, bad = R.ref_solve(A, B)
    assert Y is not None, (family, n, bad)
    Yf = R.fp64_solve(A, B)
    Ym = R.blocked_model_solve(A, B)
    caps = [R.caps_of(A, B[:, k], Yf[:, k], Ym[:, k], Y[:, k]) for k in range(B.shape[1])]
    for a in (A, B, Y):
        a.setflags(write=False)
    return {"A": A, "B": B, "Y": Y, "caps": caps}


def garbage_lower(A, seed=5):
    """The layout contract: only the row-major upper triangle is read."""
    n = A.shape[0]
    G = A.copy()
    il = np.tril_indices(n, -1)
    rng = np.random.default_rng([seed, n])
    G[il] = rng.standard_normal(len(il[0])) * 1e30
    if len(il[0]):
        G[il[0][0], il[1][0]] = np.nan
    return G


# ---- non-SPD ---------------------------------------------------------------------

NONSPD_SIZES = (100, 192, 320)     # 100: the small path; 192, 320: persistent (n % 64 == 0: no partial tile)
NONSPD_KINDS = ("neg_diag", "zero_pivot", "late_neg", "nan_diag", "nan_off")


def bad_columns(n):
    """Column 0, column n - 1, the first column of tile 1, and a column inside
    the last tile that holds pivots (at n = 100 a partial tile)."""
    last = NB * ((n - 1) // NB) + 17
    return (0, n - 1, NB, last)


def nonspd(kind, n, p):
    """(A, pivot): an identity with one defect aimed at column p, and the
    pivot at which an exact Cholesky stops.  The two-by-two blocks and the
    off-diagonal NaN sit on rows (p - 1, p); at p = 0 they sit on rows (0, 1)
    and stop at pivot 1, except the zero pivot, which is A[0, 0] = 0."""
    A = np.eye(n)
    q = max(p, 1)
    if kind == "neg_diag":
        A[p, p] = -1.0
        return A, p
    if kind == "nan_diag":
        A[p, p] = np.nan
        return A, p
    if kind == "zero_pivot":
        if p == 0:
            A[0, 0] = 0.0
            return A, 0
        A[q - 1, q] = A[q, q - 1] = 1.0            # [[1, 1], [1, 1]]: pivot q is exactly 0
        return A, q
    if kind == "late_neg":
        A[q - 1, q] = A[q, q - 1] = 2.0            # [[1, 2], [2, 1]]: pivot q is 1 - 4
        return A, q
    if kind == "nan_off":
        A[q - 1, q] = A[q, q - 1] = np.nan
        return A, q
    raise ValueError(kind)


def nonspd_ids():
    return [(kind, n, p) for n in NONSPD_SIZES for kind in NONSPD_KINDS for p in bad_columns(n)]
