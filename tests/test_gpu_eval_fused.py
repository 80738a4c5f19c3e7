"""The evaluation's two camera-major passes as one (k_jac_obs_prep: the scaled
k_jacobian<false> and k_obs_prep_rc over one walk of the chunk table, behind
the point pass), and the cameras' staged records written by k_cam_sum_diag in
place of k_cam_stage_rot.  Unsharded STRUCT_AND_POSE solves with more than 64
cameras take it; SFM_EVAL_SPLIT=1 forces the separate kernels.

Every case solves with and without the switch and asserts equal trace
records, summaries and parameter bytes: the fused pass changes no operation
and no summation order.

* 65 / 130 / 513 cameras times 1 / 255 / 257 / 1025 points, both LM loops.
* Chunk edges: cameras with 1, 63, 64, 65 and 129 observations (the last
  chunk's padding, a full chunk, a run of three).
* The carry of a camera's per-lane sums across chunks: one workgroup per XCD
  (SFM_JAC_WG_PER_XCD=1), so a wave walks many chunks.
* A rejected step: the stand-alone k_obs_prep_rc and the Schur pass run after
  a fused evaluation, with the cameras' records left from it.
* POSE_ONLY, STRUCT_ONLY and sfm_ba_evaluate do not take the path.
"""
import json
import os

import numpy as np
import pytest

import irregular_cases as IR
import step_prep_cases as SP
import step_prep_helpers as H
import sfm_amd
from sfm_amd import ba as B
from sfm_amd import scene

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIX = json.load(open(os.path.join(G, "step_prep.json")))

_COUNTS = ("termination_type", "num_iterations", "num_successful_steps", "num_unsuccessful_steps",
           "num_invalid_steps", "num_residual_evaluations", "num_jacobian_evaluations", "num_linear_solves")


def _solve(s, monkeypatch, split, host=False, mode=B.STRUCT_AND_POSE, options=None, env=None):
    """One resident solve of scene s -> (summary, trace, (rot, t, X))."""
    for k, v in dict(SFM_EVAL_SPLIT="1" if split else None, SFM_HOST_LM="1" if host else None, **(env or {})).items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    with sfm_amd.BundleAdjuster() as ba:
        ba.set_problem(s.uv, s.cam_idx, s.pt_idx, s.K, s.rot, s.t, s.X)
        sm, tr = ba.solve(options, mode=mode) if options is not None else ba.solve(mode=mode)
        return sm, tr, ba.parameters()


def _assert_same(a, b):
    (sa, ta, pa), (sb, tb, pb) = a, b
    assert ta == tb, (H.seq_of(ta), H.seq_of(tb))
    for f in _COUNTS:
        assert getattr(sa, f) == getattr(sb, f), f
    assert sa.initial_cost == sb.initial_cost and sa.final_cost == sb.final_cost
    for x, y in zip(pa, pb):
        assert x.tobytes() == y.tobytes()


def _fused_equals_split(s, monkeypatch, **kw):
    """Both LM loops, each fused against split; -> the device loop's fused result."""
    out = None
    for host in (False, True):
        fused = _solve(s, monkeypatch, False, host, **kw)
        _assert_same(fused, _solve(s, monkeypatch, True, host, **kw))
        assert len(fused[1]) > 1  # at least one step after the initial evaluation
        if out is None:
            out = fused
        else:
            _assert_same(out, fused)  # (the two loops agree, as everywhere)
    return out


@pytest.mark.parametrize("pts", (1, 255, 257, 1025))
@pytest.mark.parametrize("cams", (65, 130, 513))
def test_camera_and_point_counts(cams, pts, monkeypatch):
    _fused_equals_split(SP.grid_scene(cams, pts), monkeypatch)


EDGE_COUNTS = {10: 1, 11: 63, 12: 64, 13: 65, 14: 129}


def _chunk_edge_scene():
    """irregular_cases' construction at 136 cameras / 6000 points, then
    cameras 10..14 cut down to 1, 63, 64, 65 and 129 observations."""
    s = IR.irregular(scene.generate(136, 6000, views=10, seed=11), seed=5, hubs=IR.HUBS, empty=(7, 135), dups=40,
                     shuffle=True, maxdeg=10)
    keep = np.ones(len(s.cam_idx), bool)
    for c, n in EDGE_COUNTS.items():
        idx = np.flatnonzero(s.cam_idx == c)
        assert len(idx) >= n, (c, len(idx))
        keep[idx[n:]] = False
    s.uv, s.cam_idx, s.pt_idx = s.uv[keep].copy(), s.cam_idx[keep].copy(), s.pt_idx[keep].copy()
    return s


def test_chunk_edges(monkeypatch):
    s = _chunk_edge_scene()
    cnt = np.bincount(s.cam_idx, minlength=136)
    assert {c: int(cnt[c]) for c in EDGE_COUNTS} == EDGE_COUNTS
    assert cnt[7] == 0 and cnt[135] == 0
    _fused_equals_split(s, monkeypatch)


@pytest.mark.parametrize("pts", (3000, 20000))
def test_sums_carried_across_chunks(pts, monkeypatch):
    """One workgroup per XCD: 32 waves walk the whole chunk table, each one
    contiguous run of a point slice's chunks (camera-major within the slice).
    3000 points: about 520 chunks, 16 per wave and at most 4 per camera, so
    every run crosses cameras.  20000 points: every camera has at least 2
    chunks in each of the 8 point slices however they divide (count / 8 / 64
    >= 2), so runs also hold consecutive chunks of one camera, whose per-lane
    sums are carried."""
    s = scene.generate(130, pts, views=10, seed=11)
    cnt = np.bincount(s.cam_idx, minlength=130)
    chunks = int(np.sum((cnt + 63) // 64))
    jac_blocks = 8 * max(1, min((chunks // 8 + 3) // 4, 1))  # camera_runs' formula with SFM_JAC_WG_PER_XCD=1
    waves = 4 * jac_blocks
    assert waves == 32
    per_cam = (cnt + 63) // 64
    assert chunks / waves >= 2 * per_cam.max() and per_cam.min() >= 3, (chunks, per_cam.min(), per_cam.max())
    if pts == 20000:
        assert (cnt // (8 * 64)).min() >= 2, cnt.min()
    _fused_equals_split(s, monkeypatch, env={"SFM_JAC_WG_PER_XCD": "1"})
    # and the same results as the default grid's one chunk per wave
    _assert_same(_solve(s, monkeypatch, False, env={"SFM_JAC_WG_PER_XCD": "1"}), _solve(s, monkeypatch, False))


def test_rejected_step_after_a_fused_evaluation(monkeypatch):
    build, over, mode = SP.cases()["reject_130"]
    c = FIX["reject_130"]
    got = _fused_equals_split(build(), monkeypatch, mode=c["mode"], options=sfm_amd.make_options(**c["options"]))
    assert H.seq_of(got[1]) == H.seq_of(c["trace"]), H.seq_of(got[1])
    assert "R" in H.seq_of(got[1])


@pytest.mark.parametrize("mode", [B.POSE_ONLY, B.STRUCT_ONLY])
def test_other_modes_unchanged(mode, monkeypatch):
    s = scene.generate(130, 1025, views=10, seed=11)
    _fused_equals_split(s, monkeypatch, mode=mode)


def test_evaluate_unchanged(monkeypatch):
    s = scene.generate(130, 1025, views=10, seed=11)
    out = []
    for split in (False, True):
        if split:
            monkeypatch.setenv("SFM_EVAL_SPLIT", "1")
        else:
            monkeypatch.delenv("SFM_EVAL_SPLIT", raising=False)
        with sfm_amd.BundleAdjuster() as ba:
            ba.set_problem(s.uv, s.cam_idx, s.pt_idx, s.K, s.rot, s.t, s.X)
            out.append(ba.evaluate())
    (c0, r0, j0), (c1, r1, j1) = out
    assert c0 == c1 and r0.tobytes() == r1.tobytes() and j0.tobytes() == j1.tobytes()
