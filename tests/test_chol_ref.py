"""CPU: the dense Cholesky tests' own yardsticks (tests/chol_ref.py,
tests/chol_cases.py) checked before any kernel is held to them.

- ref_solve against a 50-digit mpmath solve;
- every SPD case: np.linalg.cholesky succeeds, the reference's own backward
  error is far below fp64's unit roundoff, and correct fp64 code (fp64_solve,
  the blocked explicit-inverse model) meets the caps tests/test_gpu_chol.py
  applies to the kernels, with the caps themselves bounded per family so they
  cannot grow vacuous;
- every non-SPD case stops ref_solve at its declared pivot.

SFM_CHOL_REF_RECORD=1 rewrites profiles/chol_reference_errors.txt (each
case's forward / backward error of fp64_solve and of the model) from a full
run of this file.
"""
import os

import numpy as np
import pytest

from tests import chol_cases as C
from tests import chol_ref as R

U = R.U
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fwd_ceiling(A):
    """What a backward-stable fp64 solve may lose: 8 cond_2(A') u on the
    equilibrated A' (cond ~ 5 for well and scaled, up to 1e6 / 1e10 for the
    graded spectra, which equilibration cannot improve; the 8 stands for the
    dimension-dependent constant of the bound, n <= 384)."""
    d = np.sqrt(np.diag(A))
    return 8 * np.linalg.cond(A / d[:, None] / d[None, :]) * U


_rows = {}


@pytest.fixture(scope="module", autouse=True)
def _record():
    yield
    if os.environ.get("SFM_CHOL_REF_RECORD") != "1" or len(_rows) != len(C.spd_ids()) * len(C.RHS):
        return
    with open(os.path.join(ROOT, "profiles", "chol_reference_errors.txt"), "w") as f:
        f.write("# tests/test_chol_ref.py: errors against ref_solve on the equilibrated system, in units of u = 2^-53\n"
                "# family n rhs | fp64_solve forward backward | blocked model forward backward\n")
        for (fam, n, rhs), (ff, fb, mf, mb) in sorted(_rows.items(), key=lambda kv: (C.FAMILIES.index(kv[0][0]),
                                                                                     kv[0][1], C.RHS.index(kv[0][2]))):
            f.write(f"{fam:9s} {n:4d} {rhs:7s} | {ff / U:12.4g} {fb / U:10.4g} | {mf / U:12.4g} {mb / U:10.4g}\n")


@pytest.mark.parametrize("family", C.FAMILIES)
def test_ref_solve_agrees_with_mpmath(family):
    import mpmath as mp
    n = 37
    A = C.matrix(family, n)
    b = C.rhs_block(family, n, A)[:, 0]
    y, bad = R.ref_solve(A, b)
    assert bad == -1
    with mp.workdps(50):
        Am = mp.matrix(n, n)
        for i in range(n):
            for j in range(n):
                Am[i, j] = mp.mpf(float(A[min(i, j), max(i, j)]))
        ym = mp.cholesky_solve(Am, mp.matrix([mp.mpf(float(v)) for v in b]))
        # longdouble -> mpmath exactly: hi + lo parts, each an fp64
        hi = y.astype(np.float64)
        lo = (y - hi.astype(np.longdouble)).astype(np.float64)
        err = max(abs(mp.mpf(float(hi[i])) + mp.mpf(float(lo[i])) - ym[i]) for i in range(n))
        rel = float(err / max(abs(ym[i]) for i in range(n)))
    print(f"{family}: ref_solve vs mpmath {rel:.3e}")
    assert rel <= 1e-17


@pytest.mark.parametrize("family,n", C.spd_ids())
def test_spd_case_yardsticks(family, n):
    c = C.spd_case(family, n)
    A, B, Y = c["A"], c["B"], c["Y"]
    np.linalg.cholesky(A)
    assert np.array_equal(A, A.T)
    ceil = _fwd_ceiling(A)
    for k, rhs in enumerate(C.RHS):
        cap_f, cap_b, (ff, fb, mf, mb) = c["caps"][k]
        _rows[(family, n, rhs)] = (ff, fb, mf, mb)
        _, ref_b = R.errors(A, B[:, k], Y[:, k], Y[:, k])
        print(f"{family} n={n} {rhs}: ref bwd {ref_b / U:.2e} u; fp64 fwd {ff:.2e} bwd {fb / U:.3g} u; "
              f"model fwd {mf:.2e} bwd {mb / U:.3g} u")
        assert ref_b <= 1e-3 * U
        if rhs == "zero":
            assert not np.any(Y[:, k]) and ff == fb == mf == mb == 0.0
            continue
        # correct fp64 code is inside the kernels' caps ...
        assert ff <= cap_f and mf <= cap_f and fb <= cap_b and mb <= cap_b
        # ... and the caps stay where such code puts them
        assert max(ff, mf) <= ceil, (ff, mf, ceil)


@pytest.mark.parametrize("kind,n,p", C.nonspd_ids())
def test_nonspd_case_fails_at_its_pivot(kind, n, p):
    A, pivot = C.nonspd(kind, n, p)
    y, bad = R.ref_solve(A, np.ones(n))
    assert y is None and bad == pivot
    assert pivot in (p, max(p, 1))


def test_garbage_lower_keeps_the_upper_triangle():
    A = C.matrix("well", 65)
    G = C.garbage_lower(A)
    assert np.array_equal(np.triu(G), np.triu(A)) and not np.array_equal(G, A)
    b = np.ones(65)
    assert np.array_equal(R.fp64_solve(G, b), R.fp64_solve(A, b))
    assert np.array_equal(R.blocked_model_solve(G, b), R.blocked_model_solve(A, b))
    assert np.array_equal(R.ref_solve(G, b)[0], R.ref_solve(A, b)[0])
