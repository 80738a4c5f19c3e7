"""The two kernels of large reduced systems against the oracle, and the small
path's bits against fixtures recorded before they existed:

* k_schur_pairs_rot_pw, the off-diagonal Schur pass with the rotation columns
  taken from the rotated point (j_k x (R X)), and
* k_backsub_pm, the one-pass point-major back substitution (at most 512
  cameras, STRUCT_AND_POSE).

Both run where C (C + 1) / 2 > 8192 (the solver's camera-block count, with
the diagonal and the empty blocks), i.e. from 128 cameras on whatever the
visibility; 127 cameras are the last on the small path.  The full-solve cases
use scene.generate(136, 3000, views=10, seed=11): 30k observations, about 15
pairs per block, 8 lanes per block (kSub = 8).  A camera in the first-order
branch of ceres::AngleAxisRotatePoint (theta^2 <= DBL_EPSILON) takes e_k x X
instead of j_k x (R X), so the rotations (0, 0, 0), (1e-9, 0, 0) and
(1e-7, 0, 0) straddle that switch.
"""

import functools
import importlib.util
import os

import numpy as np
import pytest

import sfm_amd
from sfm_amd import ba as B
from sfm_amd import scene
from oracle import ffi as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _rel(a, b, floor=1e-3):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor)))


def _assert_parity(o, g):
    # the assertions of test_gpu_scale._assert_parity
    sm_o, tr_o, r_o, t_o, X_o = o
    sm_g, tr_g, r_g, t_g, X_g = g
    assert sm_g.termination_type == sm_o["termination_type"]
    assert sm_g.num_iterations == sm_o["num_iterations"]
    assert [t["step_is_successful"] for t in tr_g] == [t["step_is_successful"] for t in tr_o]
    assert abs(sm_g.final_cost - sm_o["final_cost"]) <= 1e-9 * max(sm_o["final_cost"], 1e-300)
    assert _rel(X_g, X_o) < 1e-6
    assert _rel(t_g, t_o) < 1e-6
    assert _rel(r_g, r_o) < 1e-6


def _solve_oracle(s, mode=B.STRUCT_AND_POSE):
    r_o, t_o, X_o = s.copy_params()
    sm_o, tr_o = O.solve(s.uv, s.cam_idx, s.pt_idx, s.K, r_o, t_o, X_o, mode=mode)
    return sm_o, tr_o, r_o, t_o, X_o


def _solve_both(s, mode=B.STRUCT_AND_POSE, oracle=None):
    sm_o, tr_o, r_o, t_o, X_o = oracle if oracle is not None else _solve_oracle(s, mode)
    r_g, t_g, X_g = s.copy_params()
    sm_g, tr_g = sfm_amd.solve(s.uv, s.cam_idx, s.pt_idx, s.K, r_g, t_g, X_g, mode=mode)
    return (sm_o, tr_o, r_o, t_o, X_o), (sm_g, tr_g, r_g, t_g, X_g)


@functools.lru_cache(maxsize=None)
def _scene(cams, views):
    return scene.generate(cams, 3000, views=views, seed=11)


@functools.lru_cache(maxsize=None)
def _oracle_136():
    # one oracle solve shared by the cases on the 136-camera scene (left unchanged)
    return _solve_oracle(_scene(136, 10))


def _all_blocks_non_empty(s):
    seen = np.zeros((s.n_cams, s.n_cams), bool)
    order = np.argsort(s.pt_idx, kind="stable")
    ci = s.cam_idx[order].reshape(s.n_pts, -1)  # every point has `views` observations
    for a in range(ci.shape[1]):
        for b in range(ci.shape[1]):
            seen[ci[:, a], ci[:, b]] = True
    return bool(seen.all())


@pytest.mark.parametrize("views", [10, 12])
def test_full_solve_matches_oracle(views):
    s = _scene(136, views)
    assert _all_blocks_non_empty(s)
    o, g = _solve_both(s, oracle=_oracle_136() if views == 10 else None)
    assert o[0]["termination_type"] == 0 and o[0]["num_iterations"] == 3  # CONVERGENCE, as measured on the oracle
    _assert_parity(o, g)


def test_two_solves_of_one_handle_are_bitwise_equal():
    s = _scene(136, 10)
    with sfm_amd.BundleAdjuster() as ba:
        ba.set_problem(s.uv, s.cam_idx, s.pt_idx, s.K, s.rot, s.t, s.X)
        sm1, tr1 = ba.solve()
        p1 = ba.parameters()
        ba.reset()
        sm2, tr2 = ba.solve()
        p2 = ba.parameters()
    assert sm1.final_cost == sm2.final_cost and sm1.num_iterations == sm2.num_iterations
    assert [t["cost"] for t in tr1] == [t["cost"] for t in tr2]
    for a, b in zip(p1, p2):
        assert np.array_equal(a, b)


def _small_angle_scene():
    """Cameras 1 and 2 become twins of camera 0 (true rotation exactly 0):
    its intrinsics, its true pose, their observations re-projected through it
    with the scene's pixel noise; the initial rotations are then (0, 0, 0),
    (1e-9, 0, 0) and (1e-7, 0, 0): theta^2 below, below and above DBL_EPSILON.
    The oracle converges on it in 3 iterations, like the unchanged scene."""
    s = scene.generate(136, 3000, views=10, seed=11)
    assert not s.rot_true[0].any() and not s.rot[0].any()
    rng = np.random.default_rng(5)
    K = s.K[0].reshape(3, 3)
    for c, w in ((1, 1e-9), (2, 1e-7)):
        m = s.cam_idx == c
        pc = s.X_true[s.pt_idx[m]] + s.t_true[0]
        assert np.all(pc[:, 2] > 0.1)
        x, y = pc[:, 0] / pc[:, 2], pc[:, 1] / pc[:, 2]
        s.uv[m, 0] = K[0, 0] * x + K[0, 1] * y + K[0, 2]
        s.uv[m, 1] = K[1, 1] * y + K[1, 2]
        s.uv[m] += rng.normal(0, 0.5, (int(m.sum()), 2))
        s.K[c] = s.K[0]
        s.rot[c] = (w, 0.0, 0.0)
        s.t[c] = s.t[0]
    return s


def test_small_angle_cameras_match_oracle():
    s = _small_angle_scene()
    o, g = _solve_both(s)
    assert o[0]["termination_type"] == 0  # the oracle itself converges on this input
    _assert_parity(o, g)


@pytest.mark.parametrize("mode", [B.STRUCT_ONLY, B.POSE_ONLY])
def test_other_modes_keep_working_at_136_cameras(mode):
    o, g = _solve_both(_scene(136, 10), mode)
    _assert_parity(o, g)


@pytest.mark.parametrize("cams", [127, 128, 129])
def test_gate_boundary(cams):
    # the gate is C (C + 1) / 2 > 8192: 127 cameras (8128 blocks) take
    # k_schur_pts and the three-pass back substitution -- that they do is
    # shown by test_127_cameras_are_bitwise_the_recorded_solve,
    # whose fixture the commit before these kernels recorded --, 128 (8256)
    # and 129 cameras take k_schur_pairs_rot_pw and k_backsub_pm
    assert (cams * (cams + 1) // 2 > 8192) == (cams >= 128)
    s = _scene(cams, 10)
    o, g = _solve_both(s)
    _assert_parity(o, g)


@pytest.mark.parametrize("sub", [16, 32, 64])
def test_other_lanes_per_block_match_oracle(sub, monkeypatch):
    # k_schur_pairs_rot_pw<16 / 32 / 64>: the camera staging's lane mapping and
    # ballot masks depend on the lanes per block (set_problem reads the override)
    monkeypatch.setenv("SFM_SCHUR_PTS_SUB", str(sub))
    o, g = _solve_both(_scene(136, 10), oracle=_oracle_136())
    _assert_parity(o, g)


def test_dense_scene_picks_16_lanes_per_block():
    # 26 views per point: 325 pairs per point, ~105 per block, which
    # set_problem's rule (a tenth of the mean, 8..64) turns into 16 lanes
    s = _scene(136, 26)
    assert 80 < s.n_pts * 26 * 25 / 2 / (136 * 137 / 2) < 160
    o, g = _solve_both(s)
    _assert_parity(o, g)


def _make_small_path():
    spec = importlib.util.spec_from_file_location("make_small_path", os.path.join(GOLDEN, "make_small_path.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _assert_bitwise_fixture(name):
    mod = _make_small_path()
    got = mod.solve_small_path(*mod.FIXTURES[name])
    want = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert sorted(want.files) == sorted(got)
    for k in want.files:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), k


def test_small_path_is_bitwise_the_recorded_solve():
    _assert_bitwise_fixture("small_path_60x3000")


def test_127_cameras_are_bitwise_the_recorded_solve():
    # the old side of the gate: 127 cameras (8128 camera blocks) still run the
    # kernels of the commit before, which recorded this fixture
    _assert_bitwise_fixture("small_path_127x3000")
