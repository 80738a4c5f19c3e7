"""GPU: the dense reduced-camera Cholesky (k_chol_fused, k_backsolve,
k_chol_small) against an extended-precision reference.

Every bound comes from tests/chol_ref.py and tests/chol_cases.py (checked on
the CPU by tests/test_chol_ref.py), none from a GPU run: on the equilibrated
system the kernels' y may be 8 x as far from ref_solve's as the worse of
fp64_solve and the blocked explicit-inverse model (floors 4u forward, u
backward).  The 8 is the margin for another accumulation order: chains of
16x16x4 MFMAs where the models take dot products, at n <= 384 at most 96
four-term links per entry.

Two paths: the default (k_chol_small up to two tiles, the persistent pair
above) and the persistent pair at every size (SFM_CHOL_NO_SMALL=1, one child
process for the whole list).  The bitwise checks (epoch reuse, repeated
calls, helper-grid size, skewed walker waves) are what detects an ordering
or hand-off fault without instrumentation.

The panel factor (k_chol_fused<true> + k_panel_update, otherwise reached only
through whole distributed BA solves) goes through the same caps on one rank
(dense_spd_solve_panels).
"""
import functools

import numpy as np
import pytest

from tests import chol_cases as C
from tests import chol_child as K
from tests import chol_ref as R

pytestmark = pytest.mark.gpu

PATHS = ("default", "persistent")
# the skewed walkers' size: the smallest of 639, 1279, 3007 at which at least
# a quarter of the nblk steps took the fast path (9 of 9 at 639, recorded in
# profiles/chol_skew_fast_path.txt)
SKEW_N = 639


@functools.lru_cache(maxsize=None)
def _spd(path):
    return K.run_spd() if path == "default" else K.in_child("spd", SFM_CHOL_NO_SMALL="1")


@functools.lru_cache(maxsize=None)
def _nonspd(path):
    return K.run_nonspd() if path == "default" else K.in_child("nonspd", SFM_CHOL_NO_SMALL="1")


@functools.lru_cache(maxsize=None)
def _default_bits(n):
    return K.run_bits([n])[str(n)]


@functools.lru_cache(maxsize=None)
def _after_ref(n):
    A = C.matrix("well", n)
    b = C.rhs_block("well", n, A)[:, 0]
    y_ref, bad = R.ref_solve(A, b)
    assert bad == -1
    return A, b, y_ref, R.caps(A, b, y_ref)


def _check(A, b, y_ref, cap, hexy, fl, what):
    cap_f, cap_b, _ = cap
    assert fl == 0, what
    y = K.unhex(hexy)
    if not np.any(b):
        assert not np.any(y), what
        return
    fwd, bwd = R.errors(A, b, y, y_ref)
    print(f"{what}: forward {fwd:.3e} (cap {cap_f:.3e}), backward {bwd / R.U:.3g} u (cap {cap_b / R.U:.3g} u)")
    assert fwd <= cap_f, what
    assert bwd <= cap_b, what


@pytest.mark.parametrize("family,n", C.spd_ids())
@pytest.mark.parametrize("path", PATHS)
def test_spd_solve_within_reference_caps(path, family, n):
    c = C.spd_case(family, n)
    got = _spd(path)
    for k, rhs in enumerate(C.RHS):
        hexy, fl = got[f"{family}-{n}-{rhs}"]
        _check(c["A"], c["B"][:, k], c["Y"][:, k], c["caps"][k], hexy, fl, f"{path} {family} n={n} {rhs}")


@pytest.mark.parametrize("n", [65, 192])
@pytest.mark.parametrize("path", PATHS)
def test_only_the_upper_triangle_is_read(path, n):
    got = _spd(path)
    assert got[f"garbage-{n}"] == got[f"scaled-{n}-random"]


@pytest.mark.parametrize("n", [128, 256, 320])
def test_epoch_reuse_same_bits(n):
    """reps = 3 runs epochs 1..3 on the same flags, tickets and W image."""
    A, b = K.well(n)
    assert K._solve(A, b, reps=3) == _default_bits(n)


@pytest.mark.parametrize("n", [128, 256, 320, 600])
def test_repeated_calls_same_bits(n):
    A, b = K.well(n)
    first = _default_bits(n)
    assert first[1] == 0
    for _ in range(5):
        assert K._solve(A, b) == first


@pytest.mark.parametrize("helpers", [1, 2, 7])
def test_helper_grid_size_same_bits(helpers):
    """One helper makes the walker's polls miss on every step (the !early
    path); the default grid is one workgroup per CU.  One and two helpers are
    also fewer than a column has tiles that await W_j: every wait must be for
    a ticket taken earlier, or the grid stalls until the bounded waits give
    up (fail bit 4 -- what this test found at n = 192 with one helper while
    the walker awaited P(j+1,j+1) ahead of publishing W_j)."""
    sizes = [192, 320, 600]
    got = K.in_child("bits", sizes, SFM_CHOL_HELPERS=str(helpers))
    for n in sizes:
        assert got[str(n)] == _default_bits(n), n


@pytest.mark.parametrize("kind,n,p", C.nonspd_ids())
@pytest.mark.parametrize("path", PATHS)
def test_nonspd_reports_bit_one_only(path, kind, n, p):
    """chol_fail == 1: the pivot bit, and neither timeout bit (2, 4)."""
    assert _nonspd(path)[f"{kind}-{n}-{p}"] == 1


@pytest.mark.parametrize("kind,n,p", C.nonspd_ids())
@pytest.mark.parametrize("path", PATHS)
def test_spd_solve_after_a_failed_one(path, kind, n, p):
    """The solve right after each failed one, in the same process (on the
    persistent path a factor that stopped at a late column or on a NaN)."""
    A, b, y_ref, cap = _after_ref(n)
    hexy, fl = _nonspd(path)[f"after-{kind}-{n}-{p}"]
    _check(A, b, y_ref, cap, hexy, fl, f"{path} after {kind} n={n} p={p}")


@pytest.mark.parametrize("skew", [1, 2])
def test_skewed_walker_same_bits(skew):
    """SFM_CHOL_TEST_SKEW: waves 1-3 (1) or wave 0 (2) of the walker held back
    ~7 us between the POTRF and the Tn hand-off on every step.  The factor
    does not depend on which side arrives first: y bitwise the unskewed one
    and inside the reference caps; and the run did take the path in question
    (prefetch stored without a flag wait after it) on at least nblk / 4 steps.
    Without the barrier between the Tn writes and the TRSM, skew 1 changes
    y's bits at this size (shown once on a scratch build, same profile file);
    skew 2 guards the opposite arrival order."""
    n = SKEW_N
    nblk = (n + 1 + 63) // 64
    hexy, fl, fast, steps = K.in_child("skew", [n], SFM_CHOL_TEST_SKEW=str(skew))[str(n)]
    print(f"skew {skew}: n={n}, nblk={nblk}: {fast} of {steps} steps on the fast path")
    assert steps == nblk - 1
    assert 4 * fast >= nblk
    assert [hexy, fl] == _default_bits(n)
    A, b = K.well(n)
    y_ref, _ = R.ref_solve(A, b)
    _check(A, b, y_ref, R.caps(A, b, y_ref), hexy, fl, f"skew {skew} n={n}")


# ---- the panel factor (k_chol_fused<true>, k_panel_update) on one rank ----------
# (n, panel_tiles): nblk = 3, 4, 6, 7 with one-, two- and three-tile panels;
# (257, 2): nblk = 5, the last panel narrower; (192, 8): one panel holds all
PANEL_SHAPES = [(n, pt) for n in (128, 192, 320, 384) for pt in (1, 2, 3)] + [(257, 2), (192, 8)]


@pytest.mark.parametrize("family", C.FAMILIES)
@pytest.mark.parametrize("n,pt", PANEL_SHAPES)
def test_panel_factor_within_reference_caps(n, pt, family):
    from sfm_amd.ba import dense_spd_solve_panels
    c = C.spd_case(family, n)
    for k, rhs in enumerate(C.RHS):
        y, fl = dense_spd_solve_panels(c["A"], c["B"][:, k], pt)
        _check(c["A"], c["B"][:, k], c["Y"][:, k], c["caps"][k], y.tobytes().hex(), fl,
               f"panels of {pt}: {family} n={n} {rhs}")


@pytest.mark.parametrize("kind", C.NONSPD_KINDS)
@pytest.mark.parametrize("n,pt,p", [(192, 1, 64 + 17), (320, 2, 128), (320, 2, 255)])
def test_panel_factor_reports_a_bad_pivot_in_the_second_panel(n, pt, p, kind):
    from sfm_amd.ba import dense_spd_solve_panels
    A, pivot = C.nonspd(kind, n, p)
    assert pt * 64 <= pivot < 2 * pt * 64
    _, fl = dense_spd_solve_panels(A, np.ones(n), pt)
    assert fl == 1
