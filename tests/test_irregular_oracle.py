"""CPU: the irregular scenes of tests/irregular_cases.py against the committed
fixture tests/golden/irregular.json (made by tests/golden/make_irregular.py)
and against what they claim to be: points of every degree from 0 to nearly C,
two cameras without observations (the last one among them), doubled (camera,
point) keys, inside every bound of set_problem they approach, on the regime of
ba_host_layout.h they are named for, with a trajectory no correct fp64
implementation can leave.  None of these numbers comes from the device.
"""
import functools
import json
import os

import numpy as np
import pytest

import irregular_cases as IC
from oracle import ffi as O

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIX = json.load(open(os.path.join(G, "irregular.json")))
NAMES = sorted(IC.SCENES)
TERMINATION = ["CONVERGENCE", "NO_CONVERGENCE", "FAILURE"]


@functools.lru_cache(maxsize=None)
def _solved(name):
    s = IC.build(name)
    r, t, X = s.copy_params()
    sm, tr = O.solve(s.uv, s.cam_idx, s.pt_idx, s.K, r, t, X, mode=2, options=O.default_options(**FIX[name]["options"]))
    return s, IC.structure(s, IC.SCENES[name][3]), sm, tr, (r, t, X)


def test_fixture_names_the_scenes():
    assert sorted(FIX) == NAMES
    assert set(IC.PLAIN) | set(IC.REJECTING) == set(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_matches(name):
    s, st, sm, tr, _ = _solved(name)
    c = FIX[name]
    assert IC.seq_of(tr) == c["sequence"] == IC.seq_of(c["trace"])
    assert TERMINATION[sm["termination_type"]] == c["termination"] == "CONVERGENCE"
    assert st == c["counts"]
    assert sm["num_iterations"] == c["summary"]["num_iterations"]


def test_recorded_trajectories():
    seqs = {n: FIX[n]["sequence"] for n in NAMES}
    assert all(seqs[n] == "AAR" for n in IC.PLAIN), seqs
    assert seqs["rej_130_irr"] == "AAARRRRRAAAAAAR" and seqs["rej_100_irr"] == "AARRRRRAAAAAAAR"


@pytest.mark.parametrize("name", NAMES)
def test_scene_is_what_it_claims_to_be(name):
    s, st, _, _, _ = _solved(name)
    C, P, _, hubs = IC.SCENES[name]
    cdeg = np.bincount(s.cam_idx, minlength=C)
    deg = np.bincount(s.pt_idx, minlength=P)
    e = IC.empty_cameras(name)
    assert e == (7, C - 1) and cdeg[7] == 0 and cdeg[C - 1] == 0
    assert st["single_view_points"] >= (30 if P == 400 else 100)
    if C in (136, 100):
        assert st["unobserved_points"] >= 1 and st["min_degree"] == 0
    assert st["duplicate_keys"] >= 30
    if hubs:
        # (irr_136_big: the 40 draws out of 76497 observations miss the hubs' 536)
        assert st["duplicates_on_hubs"] >= (0 if name == "irr_136_big" else 1)
        assert st["max_degree"] >= C - 4 and all(deg[h] >= C - 4 for h in hubs)
    else:
        assert st["max_degree"] <= 64
    # pair lists: empty ones (a camera without observations empties its whole
    # block row and column: 2 C - 1 blocks for two of them), and blocks of a
    # single pair.  Every hub adds one pair to every block of two live
    # cameras, so the single pairs are counted among the other points
    # (structure()); irr_136_big alone, with 14000 points over the same 9316
    # blocks (28 pairs per block), has fewer than 100 of them.
    assert st["empty_blocks"] >= max(100, 2 * C - 1)
    if name != "irr_136_big":
        assert st["one_pair_blocks"] >= 100
    assert st["diagonal_pairs"] == 2 * st["duplicate_keys"] and st["keys_seen_more_than_twice"] == 0
    # shuffled caller order: neither point- nor camera-major
    assert np.any(np.diff(s.pt_idx) < 0) and np.any(np.diff(s.cam_idx) < 0)
    assert s.uv.dtype == np.float64 and s.cam_idx.dtype == np.int32 and s.pt_idx.dtype == np.int32
    assert np.all(np.isfinite(s.uv))


@pytest.mark.parametrize("name", NAMES)
def test_regime_predicates(name):
    """Restated from ba_plan.h (plan_problem, plan_solve): which kernels a scene runs."""
    _, st, _, _, _ = _solved(name)
    C = st["n_cams"]
    assert st["n_blk"] == C * (C + 1) // 2
    large = st["n_blk"] > IC.K_SCHUR_XCD_MIN_BLOCKS  # k_schur_pairs_rot_pw, and k_backsub_pm while C <= kCamPMMax
    assert large == (name in ("irr_136", "irr_136_big", "rej_130_irr")) == (C >= 128)
    assert 64 < C <= IC.K_CAM_PM_MAX  # the evaluation prepares the step; every camera record fits the LDS
    assert (st["n_obs"] <= IC.K_HOST_CHECK_MAX_OBS) == (name != "irr_136_big")
    assert IC.host_counts(st) == (name != "irr_136_big")
    assert IC.small_setup_sizes_fit(st, C) == (name in ("irr_100", "rej_100_irr"))
    if name == "irr_100_hub":  # the hub's degree alone takes it off the small path
        assert IC.small_setup_sizes_fit(dict(st, max_degree=IC.K_SMALL_SETUP_MAX_PT_OBS), C)
        assert st["max_degree"] > IC.K_SMALL_SETUP_MAX_PT_OBS
    # lanes per block from the mean pair count (schur_shape): 8 for all of them
    assert st["pairs_est"] / st["n_blk"] / 10.0 <= 8
    if name == "irr_136":
        assert (st["n_obs"], st["pairs_est"]) == (16837, 84293)
    if name == "irr_136_big":
        assert st["n_obs"] == 76497


@pytest.mark.parametrize("name", NAMES)
def test_pair_bound(name):
    """The small path sizes the pair buffer 2 * pairs_est, without a count:
    k_pair_count's rule emits every unordered pair of a point's observations
    at most twice (twice exactly when both are of one camera)."""
    _, st, _, _, _ = _solved(name)
    assert st["pairs_est"] < st["n_pairs"] <= 2 * st["pairs_est"]
    assert st["n_pairs"] == st["pairs_est"] + st["diagonal_pairs"] // 2
    assert st["n_pairs"] < 2 ** 31 - 1  # the 32-bit pair offsets


@pytest.mark.parametrize("name", NAMES)
def test_trajectory_is_decisive(name):
    _, _, sm, tr, _ = _solved(name)
    o = FIX[name]["options"]
    for it in tr[1:-1]:
        assert it["step_is_valid"]
        assert abs(it["relative_decrease"] - o["min_relative_decrease"]) >= 0.01, it
    last, before = tr[-1], tr[-2]
    assert abs(last["cost_change"]) / last["cost"] <= o["function_tolerance"] / 3
    assert abs(before["cost_change"]) / before["cost"] >= 3 * o["function_tolerance"]
    assert o["min_relative_decrease"] == 1e-3 and o["function_tolerance"] == 1e-6
    if name in IC.REJECTING:
        seq = IC.seq_of(tr)
        assert "RA" in seq and seq.index("R") > 0 and "A" in seq[:seq.index("R")], seq
        for k in ("numpy_cost_rel_diff", "numpy_radius_rel_diff"):
            assert len(FIX[name][k]) == len(tr)
        assert FIX[name]["numpy_termination"] == "CONVERGENCE"


@pytest.mark.parametrize("name", NAMES)
def test_unused_blocks_are_untouched(name):
    s, st, _, _, (r, t, X) = _solved(name)
    e = list(IC.empty_cameras(name))
    assert r[e].tobytes() == s.rot[e].tobytes() and t[e].tobytes() == s.t[e].tobytes()
    un = np.flatnonzero(np.bincount(s.pt_idx, minlength=s.n_pts) == 0)
    assert len(un) == st["unobserved_points"]
    assert X[un].tobytes() == s.X[un].tobytes()
    seen = np.setdiff1d(np.arange(s.n_pts), un)
    assert not np.array_equal(X[seen], s.X[seen]) and not np.array_equal(t[0], s.t[0])
