"""GPU: the device two-view initialisation (sfm_two_view_init,
init_kernels.hip) against the CPU restatement (tests/two_view_ref.py) on the
seeded scenes of tests/two_view_cases.py: the same model, F mask, keep mask
and count (integer parity), H and F within 1e-6 of their largest element,
scores and the average error within 1e-6 relative, R and t within 1e-6, the
kept points within 1e-6 relative -- the tolerance tests/test_gpu_pnp.py uses
between the device's Jacobi SVDs and LAPACK.  The cases' stability
conditions (no decision on a threshold) are asserted on the CPU by
tests/test_two_view_ref.py."""
import numpy as np
import pytest

import sfm_amd
from tests.two_view_cases import CASES, K, reference, scene

pytestmark = pytest.mark.gpu


def run(name, **extra):
    s = scene(name)
    o = dict(s["opts"])
    o.update(extra)
    return sfm_amd.two_view_init(s["p0"], s["p1"], K, K, **o)


def compare(g, r):
    print("model", g.model, r.model, "kept", g.n_kept, r.n_kept, "mask", int(g.f_mask.sum()), int(r.f_mask.sum()))
    dH = np.abs(g.H - r.H).max() / max(np.abs(r.H).max(), 1e-300)
    dF = np.abs(g.F - r.F).max() / max(np.abs(r.F).max(), 1e-300)
    dS = np.abs(g.scores - r.scores) / np.maximum(np.abs(r.scores), 1e-300)
    dE = abs(g.avg_err - r.avg_err) / max(abs(r.avg_err), 1e-300)
    print("dH", dH, "dF", dF, "dScores", dS, "dErr", dE)
    assert g.model == r.model
    assert np.array_equal(g.f_mask, r.f_mask)
    assert np.array_equal(g.keep, r.keep) and g.n_kept == r.n_kept
    assert dH <= 1e-6 and dF <= 1e-6
    assert np.all(dS <= 1e-6) and dE <= 1e-6
    if r.model:
        k = r.keep == 1
        dR, dt = np.abs(g.R - r.R).max(), np.abs(g.t - r.t).max()
        dX = (np.abs(g.X[k] - r.X[k]).max(1) / np.abs(r.X[k]).max(1)).max()
        print("dR", dR, "dt", dt, "dX", dX)
        assert dR <= 1e-6 and dt <= 1e-6
        assert dX <= 1e-6
    else:
        assert not g.R.any() and not g.t.any() and not g.X.any() and g.n_kept == 0


@pytest.mark.parametrize("name", list(CASES))
def test_two_view_matches_reference(name):
    compare(run(name), reference(name)[0])


def test_two_view_expected_models():
    """the branches the cases are built for"""
    got = {name: run(name).model for name in CASES}
    assert got == {"n15": 2, "n65": 2, "n257_out30": 2, "n600_out60": 2, "planar_exact": 1, "planar_noisy": 1,
                   "rotation_only": 0}


@pytest.mark.parametrize("name", ["n257_out30", "planar_noisy"])
def test_two_view_is_bitwise_reproducible(name):
    a, b = run(name), run(name)
    assert a.model == b.model and a.n_kept == b.n_kept and a.avg_err == b.avg_err
    for f in ("H", "F", "f_mask", "scores", "R", "t", "keep", "X"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f


def test_two_view_too_few_points():
    p = np.random.default_rng(0).uniform(0, 700, (14, 2)).astype(np.float32)
    r = sfm_amd.two_view_init(p, p + 3, K)
    assert r.model == 0 and r.n_kept == 0 and not r.keep.any() and not r.f_mask.any() and not r.F.any()


def test_two_view_rejects_non_finite_input():
    s = scene("n65")
    p1 = s["p1"].copy()
    p1[7, 1] = np.nan
    with pytest.raises(sfm_amd.SfmError) as e:
        sfm_amd.two_view_init(s["p0"], p1, K)
    assert e.value.code == -22
    Kb = K.copy()
    Kb[0, 0] = np.inf
    with pytest.raises(sfm_amd.SfmError) as e:
        sfm_amd.two_view_init(s["p0"], s["p1"], Kb)
    assert e.value.code == -22


def test_two_view_null_optional_outputs():
    """every output pointer but `model` may be NULL"""
    import ctypes
    from sfm_amd._ffi import check, lib, ptr
    s = scene("n65")
    p0, p1, k = np.ascontiguousarray(s["p0"]), np.ascontiguousarray(s["p1"]), np.ascontiguousarray(K.reshape(9))
    model = ctypes.c_int32(-1)
    check(lib().sfm_two_view_init(0, len(p0), ptr(p0), ptr(p1), ptr(k), ptr(k), None, ctypes.byref(model), None, None,
                                  None, None, None, None, None, None, None, None), "sfm_two_view_init")
    assert model.value == reference("n65")[0].model
    assert lib().sfm_two_view_init(0, len(p0), ptr(p0), ptr(p1), ptr(k), ptr(k), None, None, None, None, None, None,
                                   None, None, None, None, None, None) == -22


@pytest.mark.parametrize("name,extra", [("n257_out30", dict(f_ransac_threshold=2.5)), ("n65", dict(f_max_iters=1)), ("n600_out60", dict(f_max_iters=5)),
                                        ("n65", dict(h_ratio=0.05))])
def test_two_view_options_follow_reference(name, extra):
    """a tighter threshold keeps fewer inliers, one iteration finds no model
    that initialises, a low h_ratio sends a general scene down the homography
    branch (which then fails): each as the reference does"""
    compare(run(name, **extra), reference(name, **extra)[0])
