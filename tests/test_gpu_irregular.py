"""The kernels chosen by camera count on the visibility a tracker produces
(tests/irregular_cases.py): points of degree 0 to C - 2, two cameras without
observations (the last block row of S among them), 40 doubled (camera, point)
keys, shuffled caller order -- where every other test of these paths has ten
views per point, in generator order, and no camera twice.

* 128+ cameras (irr_136, irr_136_big, rej_130_irr): k_schur_pairs_rot_pw with
  empty, one-pair and 130-pair lists and same-camera pairs in its diagonal
  blocks, which k_cam_sum_diag (folded evaluation) or k_schur_diag_sum (the
  prep redone after a rejected step) write first; k_backsub_pm with points of
  no, one and 135 observations.
* 65-127 cameras (irr_100_hub, irr_100, rej_100_irr): the folded point pass,
  k_schur_pts and the three-pass back substitution, on the sorted setup (a
  hub's degree above kSmallSetupMaxPtObs) and on the small one.

tests/test_irregular_oracle.py shows on the CPU that every scene is inside
set_problem's bounds and that the oracle's trajectory is decisive.  The
tolerances are the project's (tests/test_gpu_rotated_form.py,
tests/test_gpu_parity.py, tests/test_gpu_scale.py) and, for the rejecting
scenes, the step-prep tests' (floors 1e-9 / 1e-6, or 20 x the oracle's recorded
disagreement with the dense numpy loop, tests/golden/irregular.json).
"""
import functools
import json
import os

import numpy as np
import pytest

import irregular_cases as IC
import step_prep_helpers as H
import sfm_amd
from sfm_amd import ba as B
from oracle import ffi as O
from test_gpu_rotated_form import _assert_parity

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIX = json.load(open(os.path.join(G, "irregular.json")))


@functools.lru_cache(maxsize=None)
def _scene(name):
    return IC.build(name)


@functools.lru_cache(maxsize=None)
def _oracle(name, mode=B.STRUCT_AND_POSE):
    # one oracle solve per scene and mode, shared (left unchanged)
    s = _scene(name)
    r, t, X = s.copy_params()
    sm, tr = O.solve(s.uv, s.cam_idx, s.pt_idx, s.K, r, t, X, mode=mode)
    return sm, tr, r, t, X


def _solve_device(name, mode=B.STRUCT_AND_POSE):
    s = _scene(name)
    r, t, X = s.copy_params()
    sm, tr = sfm_amd.solve(s.uv, s.cam_idx, s.pt_idx, s.K, r, t, X, mode=mode)
    return sm, tr, r, t, X


def _assert_trace_parity(name, o, g):
    """test_gpu_parity.test_full_solve_parity's per-iteration checks, and the
    validity of every step."""
    tr_o, tr_g = o[1], g[1]
    assert IC.seq_of(tr_o) == FIX[name]["sequence"]  # the live oracle is the fixture's
    assert len(tr_g) == len(tr_o)
    worst_c = max(abs(a["cost"] - b["cost"]) / b["cost"] for a, b in zip(tr_g, tr_o))
    worst_r = max(abs(a["trust_region_radius"] - b["trust_region_radius"]) / b["trust_region_radius"]
                  for a, b in zip(tr_g, tr_o))
    par = max(H.rel(a, b) for a, b in zip(g[2:], o[2:]))
    print(f"{name}: {IC.seq_of(tr_g)} cost {worst_c:.2e} (1e-9) radius {worst_r:.2e} (1e-6) params {par:.2e} (1e-6)")
    assert [t["step_is_valid"] for t in tr_g] == [t["step_is_valid"] for t in tr_o]
    for a, b in zip(tr_g, tr_o):
        assert abs(a["cost"] - b["cost"]) <= 1e-9 * b["cost"]
        assert abs(a["trust_region_radius"] - b["trust_region_radius"]) <= 1e-6 * b["trust_region_radius"]


def _assert_unused_untouched(name, rot, t, X):
    s = _scene(name)
    e = list(IC.empty_cameras(name))
    assert rot[e].tobytes() == s.rot[e].tobytes() and t[e].tobytes() == s.t[e].tobytes()
    un = np.flatnonzero(np.bincount(s.pt_idx, minlength=s.n_pts) == 0)
    assert len(un) == FIX[name]["counts"]["unobserved_points"]
    assert X[un].tobytes() == s.X[un].tobytes()


@pytest.mark.parametrize("name", IC.PLAIN)
def test_full_solve_matches_oracle(name):
    o, g = _oracle(name), _solve_device(name)
    _assert_trace_parity(name, o, g)
    _assert_parity(o, g)
    _assert_unused_untouched(name, *g[2:])


@pytest.mark.parametrize("name", ["irr_136", "irr_100_hub"])
def test_evaluate_keeps_the_callers_order(name):
    # residuals and Jacobians per observation, in the shuffled order with its
    # duplicates (test_gpu_scale.test_device_layout_keeps_caller_order_of_duplicates' bounds)
    s = _scene(name)
    with sfm_amd.BundleAdjuster() as ba:
        ba.set_problem(s.uv, s.cam_idx, s.pt_idx, s.K, s.rot, s.t, s.X)
        cost, res, jac = ba.evaluate()
    r_o, j_o = O.residuals_jacobians(s.uv, s.cam_idx, s.pt_idx, s.K, s.rot, s.t, s.X)
    assert res.shape == r_o.shape and jac.shape == j_o.shape
    scale = np.maximum(np.abs(j_o).max(axis=(1, 2), keepdims=True), 1e-300)
    print(f"{name}: residuals {np.max(np.abs(res - r_o)):.2e} (1e-9) jacobians {np.max(np.abs(jac - j_o) / scale):.2e} "
          f"(1e-10)")
    assert np.max(np.abs(res - r_o)) < 1e-9
    assert np.max(np.abs(jac - j_o) / scale) < 1e-10
    assert abs(cost - 0.5 * np.sum(r_o ** 2)) <= 1e-9 * cost


@pytest.mark.parametrize("sub", [16, 32, 64])
def test_other_lanes_per_block_match_oracle(sub, monkeypatch):
    # k_schur_pairs_rot_pw<16 / 32 / 64>: most lists (a mean of 9 pairs) shorter
    # than the lanes of a block, empty ones, the diagonal ones
    monkeypatch.setenv("SFM_SCHUR_PTS_SUB", str(sub))
    o, g = _oracle("irr_136"), _solve_device("irr_136")
    _assert_trace_parity("irr_136", o, g)
    _assert_parity(o, g)
    _assert_unused_untouched("irr_136", *g[2:])


@pytest.mark.parametrize("mode", [B.POSE_ONLY, B.STRUCT_ONLY])
def test_other_modes_match_oracle(mode):
    s = _scene("irr_136")
    o, g = _oracle("irr_136", mode), _solve_device("irr_136", mode)
    _assert_parity(o, g)
    for a, b in zip(g[1], o[1]):
        assert abs(a["cost"] - b["cost"]) <= 1e-9 * b["cost"]
    _assert_unused_untouched("irr_136", *g[2:])
    # the constant side is bitwise unchanged, the other one moved
    if mode == B.STRUCT_ONLY:
        assert g[2].tobytes() == s.rot.tobytes() and g[3].tobytes() == s.t.tobytes()
        assert not np.array_equal(g[4], s.X)
    else:
        assert g[4].tobytes() == s.X.tobytes()
        assert not np.array_equal(g[3], s.t)


@pytest.mark.parametrize("name", ["irr_136", "irr_100_hub"])
def test_two_solves_of_one_handle_are_bitwise_equal(name):
    s = _scene(name)
    with sfm_amd.BundleAdjuster() as ba:
        ba.set_problem(s.uv, s.cam_idx, s.pt_idx, s.K, s.rot, s.t, s.X)
        sm1, tr1 = ba.solve()
        p1 = ba.parameters()
        ba.reset()
        sm2, tr2 = ba.solve()
        p2 = ba.parameters()
    assert tr1 == tr2 and sm1.final_cost == sm2.final_cost and sm1.num_iterations == sm2.num_iterations
    for a, b in zip(p1, p2):
        assert a.tobytes() == b.tobytes()
    _assert_parity(_oracle(name), (sm1, tr1) + tuple(p1))


@functools.lru_cache(maxsize=None)
def _branch_oracle(name):
    return H.solve_oracle(FIX[name], _scene(name))


@pytest.mark.parametrize("name", IC.REJECTING)
def test_rejected_steps_redo_the_prep(name, monkeypatch):
    """Five rejected steps in a row, then accepted ones: the stand-alone prep
    kernels rewrite the diagonal blocks that hold same-camera pairs (130
    cameras: before k_schur_pairs_rot_pw adds to them) for five stale radii."""
    c = FIX[name]
    oracle = _branch_oracle(name)
    dev, host = H.solve_device_and_host(c, oracle[0], monkeypatch)
    seq = H.seq_of(dev[1])
    assert "RA" in seq and seq.index("R") > 0, seq
    H.assert_loops_equal(dev, host)
    H.assert_branch_parity(name, c, oracle, dev)
    H.assert_branch_parity(name, c, oracle, host)
    _assert_unused_untouched(name, *dev[2])


@pytest.mark.parametrize("name", ["irr_100", "rej_100_irr"])
def test_small_setup_path_is_bitwise_the_sorted_path(name, monkeypatch):
    # as test_gpu_scale's at 12-40 cameras: here the small setup feeds the
    # folded evaluation (more than 64 cameras), with rejected steps in rej_100_irr
    s = _scene(name)
    out = []
    for flag in ("0", "1"):
        monkeypatch.setenv("SFM_SMALL_SETUP", flag)
        with sfm_amd.BundleAdjuster() as ba:
            ba.set_problem(s.uv, s.cam_idx, s.pt_idx, s.K, s.rot, s.t, s.X)
            ev = ba.evaluate()
            sm, tr = ba.solve()
            out.append((ev, sm.final_cost, tr, ba.parameters()))
    (ev0, c0, tr0, p0), (ev1, c1, tr1, p1) = out
    assert ev0[0] == ev1[0] and np.array_equal(ev0[1], ev1[1]) and np.array_equal(ev0[2], ev1[2]), name
    assert c0 == c1 and tr0 == tr1, name
    for a, b in zip(p0, p1):
        assert np.array_equal(a, b), name
    assert H.seq_of(tr1) == FIX[name]["sequence"]
