"""The LM step's preparation folded into the evaluation (unsharded
STRUCT_AND_POSE solves with more than 64 cameras): the point factor inside
the point pass, k_obs_prep_rc and the diagonal blocks behind it, the camera
step inside the one-pass back substitution (128 to 512 cameras).

* After an unsuccessful or invalid step the radius changes with no
  evaluation in between: the stand-alone prep kernels redo the preparation
  (the only route on which they run after a fold).  Scenes of
  tests/step_prep_cases.py; the device loop and the host loop must agree
  bitwise, and both with the oracle within the branch tests' tolerances
  (tests/test_gpu_lm_branches.py), scaled by tests/golden/step_prep.json.
* Camera counts 65 / 128 / 129 / 513 times point counts 1 / 255 / 257 / 1025
  against the oracle as tests/test_gpu_rotated_form.py does, each solved
  twice on one handle (bitwise equal).
* POSE_ONLY, STRUCT_ONLY and a 20-camera problem keep their sequence.
"""
import functools
import json
import os

import numpy as np
import pytest

import step_prep_cases as SP
import step_prep_helpers as H  # the rejecting scenes' helpers, shared with tests/test_gpu_irregular.py
import sfm_amd
from sfm_amd import ba as B
from sfm_amd import scene
from oracle import ffi as O

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIX = json.load(open(os.path.join(G, "step_prep.json")))

seq_of, _rel = H.seq_of, H.rel


@functools.lru_cache(maxsize=None)
def _branch_oracle(name):
    build, _, _ = SP.cases()[name]
    return H.solve_oracle(FIX[name], build())


def _solve_device_and_host(name, monkeypatch):
    return H.solve_device_and_host(FIX[name], _branch_oracle(name)[0], monkeypatch)


_assert_loops_equal = H.assert_loops_equal


def _assert_branch_parity(name, got):
    H.assert_branch_parity(name, FIX[name], _branch_oracle(name), got)


def test_rejected_steps_redo_the_prep(monkeypatch):
    """Three rejected steps, then accepted ones, at 130 cameras: the radius
    the evaluation prepared for is stale three times over."""
    dev, host = _solve_device_and_host("reject_130", monkeypatch)
    seq = seq_of(dev[1])
    assert "RA" in seq and seq.index("R") > 0, seq  # an unsuccessful step after a fold, a successful one after it
    _assert_loops_equal(dev, host)
    _assert_branch_parity("reject_130", dev)
    _assert_branch_parity("reject_130", host)


def test_invalid_steps_redo_the_prep(monkeypatch):
    """A zero pivot of the reduced camera matrix at every radius (130
    cameras): five invalid steps, each with its prep redone for the smaller
    radius, then FAILURE with the parameters untouched."""
    dev, host = _solve_device_and_host("invalid_130", monkeypatch)
    assert seq_of(dev[1]) == "IIIII", seq_of(dev[1])
    _assert_loops_equal(dev, host)
    _assert_branch_parity("invalid_130", dev)
    s = _branch_oracle("invalid_130")[0]
    for a, b in zip(dev[2], s.copy_params()):
        assert np.array_equal(a, b)


def _oracle_grid(cams, pts):
    s = SP.grid_scene(cams, pts)
    if cams == 513:  # recorded (tests/golden/make_step_prep.py): 12 s each on a CPU
        z = np.load(os.path.join(G, "step_prep_513.npz"))
        k = f"p{pts}__"
        return s, dict(term=int(z[k + "summary"][0]), iters=int(z[k + "summary"][1]), cost=float(z[k + "final_cost"][0]),
                       succ=[int(v) for v in z[k + "successful"]], sol=(z[k + "rot"], z[k + "t"], z[k + "X"]))
    r, t, X = s.copy_params()
    sm, tr = O.solve(s.uv, s.cam_idx, s.pt_idx, s.K, r, t, X)
    return s, dict(term=sm["termination_type"], iters=sm["num_iterations"], cost=sm["final_cost"],
                   succ=[it["step_is_successful"] for it in tr], sol=(r, t, X))


@pytest.mark.parametrize("pts", SP.GRID_POINTS)
@pytest.mark.parametrize("cams", SP.GRID_CAMS)
def test_camera_and_point_count_edges(cams, pts):
    s, o = _oracle_grid(cams, pts)
    with sfm_amd.BundleAdjuster() as ba:
        ba.set_problem(s.uv, s.cam_idx, s.pt_idx, s.K, s.rot, s.t, s.X)
        sm1, tr1 = ba.solve()
        p1 = ba.parameters()
        ba.reset()
        sm2, tr2 = ba.solve()
        p2 = ba.parameters()
    # the cost carries the residuals' absolute rounding (a pixel coordinate
    # of ~2e3 rounds to ~4e-13; a few operations: 4e-12 px per residual),
    # which is all there is of the one-point scenes' costs (1e-19)
    n, delta = 2 * s.n_obs, 4e-12
    tol_cost = 1e-9 * o["cost"] + np.sqrt(2.0 * n * o["cost"]) * delta + n * delta * delta
    par = max(_rel(a, b) for a, b in zip(p1, o["sol"]))
    print(f"{cams} x {pts}: {seq_of(tr1)} cost diff {abs(sm1.final_cost - o['cost']):.2e} (tol {tol_cost:.2e}) "
          f"params {par:.2e}")
    # the assertions of test_gpu_rotated_form._assert_parity
    assert sm1.termination_type == o["term"]
    assert sm1.num_iterations == o["iters"]
    assert [t["step_is_successful"] for t in tr1] == o["succ"]
    assert abs(sm1.final_cost - o["cost"]) <= tol_cost
    assert par < 1e-6
    # two solves of one handle
    assert tr1 == tr2 and sm1.final_cost == sm2.final_cost
    for a, b in zip(p1, p2):
        assert a.tobytes() == b.tobytes()


def _assert_parity(s, mode):
    r_o, t_o, X_o = s.copy_params()
    sm_o, tr_o = O.solve(s.uv, s.cam_idx, s.pt_idx, s.K, r_o, t_o, X_o, mode=mode)
    r_g, t_g, X_g = s.copy_params()
    sm_g, tr_g = sfm_amd.solve(s.uv, s.cam_idx, s.pt_idx, s.K, r_g, t_g, X_g, mode=mode)
    assert sm_g.termination_type == sm_o["termination_type"]
    assert sm_g.num_iterations == sm_o["num_iterations"]
    assert [t["step_is_successful"] for t in tr_g] == [t["step_is_successful"] for t in tr_o]
    assert abs(sm_g.final_cost - sm_o["final_cost"]) <= 1e-9 * max(sm_o["final_cost"], 1e-300)
    assert _rel(X_g, X_o) < 1e-6 and _rel(t_g, t_o) < 1e-6 and _rel(r_g, r_o) < 1e-6


@pytest.mark.parametrize("mode", [B.STRUCT_ONLY, B.POSE_ONLY])
def test_other_modes_at_129_cameras(mode):
    _assert_parity(scene.generate(129, 1025, views=10, seed=11), mode)


def test_small_system_keeps_its_sequence():
    # 20 cameras: the camera sums ride in the point pass, one-workgroup factor
    _assert_parity(scene.generate(20, 1025, views=10, seed=11), B.STRUCT_AND_POSE)
