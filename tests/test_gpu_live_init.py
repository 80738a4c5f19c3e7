"""GPU: the live loop started by the two-view initialisation
(LiveSfM(init="estimate"): sfm_two_view_init on the matcher's matches,
CSfM.cpp:823-946) instead of the stream's known pose.

* KeypointStream, 60 frames, init_gap 12: by the stream's geometry (2 px per
  frame at depth 8-14) the matches of frames 0 and 12 move 22 px (median; 36
  at most, inside the 40-px match window) with a true parallax of ~1.3
  degrees, and the CPU restatement (tests/two_view_ref.py) initialises there
  on the fundamental branch; the map then grows as in tests/test_gpu_live.py:
  no frame lost, every keyframe BA equal to the oracle's, map points and
  keyframe centres equal to the stream's truth after a Sim(3) alignment at
  that file's bounds (the gauge floats there too; only the scale differs: the
  first baseline is the unit).
* BriskVideoStream (a textured plane), 40 frames: the attempts before the
  median parallax reaches 1 degree return model 0 and the first keyframe
  stays; the homography branch then starts the map (frame 9), and the
  adjusted map reproduces the video's image motion at test_live_path_on_
  device_brisk_detections' bounds (median < 1 px, p90 < 3 px) for keyframes 9
  and 19.  At keyframe 29 the bound is the scene's: with the CPU
  restatement's R, t, X, keep in place of the device's (same matches, rest of
  the loop unchanged) the figures are median 1.0851 px, p90 3.5609 px
  (device: 1.0971, 3.6477; keyframes 9 and 19: 0.351 / 1.199 and 0.515 /
  1.738 with the restatement) -- the unit-baseline start at frame 9 leaves
  keyframes 10 frames apart from there, and the plane's pose drifts over the
  last one.  That keyframe is asserted at twice the restatement's figures.
* every attempt's device result equals the CPU restatement on the same
  matches (model, kept matches).
* a default LiveSfM() run is bitwise what the parent commit computed
  (tests/golden/live_known_30.json, recorded from the parent build)."""
import json
import os

import numpy as np
import pytest

from oracle import ffi as O
from sfm_amd.live import BriskVideoStream, KeypointStream, LiveSfM, _project
from sfm_amd.mapping import _rodrigues
from tests import two_view_ref as T

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "live_known_30.json")
GAP = 12
# image-motion bounds (median, p90, px) per keyframe where the scene, not the code, misses (1, 3):
# twice the CPU restatement's figures (see above)
BRISK_BOUNDS = {29: (2 * 1.0851, 2 * 3.5609)}


def _rel(a, b, floor=1e-3):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(np.abs(np.asarray(b)), floor)))


def _umeyama(A, B):
    """s, R, t minimising |s R A + t - B| (rows are points)."""
    ma, mb = A.mean(0), B.mean(0)
    a, b = A - ma, B - mb
    U, S, Vt = np.linalg.svd(b.T @ a / len(A))
    D = np.eye(3)
    D[2, 2] = np.sign(np.linalg.det(U @ Vt))
    R = U @ D @ Vt
    s = np.trace(np.diag(S) @ D) / (a ** 2).sum(1).mean()
    return s, R, mb - s * R @ ma


def _attempts_follow_reference(s):
    for e in s.init_log:
        r = T.two_view_init(e["pts0"], e["pts1"], s.K, s.K)
        print("attempt at frame", e["frame"], e["matches"], "matches: model", e["model"], "kept", e["n_kept"],
              "reference", r.model, r.n_kept, "median parallax", r.diag.get("median_parallax_deg"))
        assert (e["model"], e["n_kept"]) == (r.model, r.n_kept)


@pytest.fixture(scope="module")
def run60():
    s = LiveSfM(KeypointStream(), init="estimate", init_gap=GAP)
    s.run(60)
    yield s
    s.close()


def test_estimated_start_tracks_every_frame(run60):
    s = run60
    assert [e["frame"] for e in s.init_log] == [GAP] and s.init_log[0]["model"] == 2   # the fundamental branch
    assert [f.no for f in s.kfs][:2] == [0, GAP]
    assert s.lost == 0 and s.stats["tracked"] == 60 - GAP - 1
    assert len(s.kfs) >= 3 and len(s.ba_log) == len(s.kfs) - 1
    assert abs(np.linalg.norm(s.init_log[0]["scores"])) > 0
    _attempts_follow_reference(s)


def test_estimated_start_every_keyframe_ba_matches_oracle(run60):
    for rec in run60.ba_log:
        r, t, X = rec["rot"].copy(), rec["t"].copy(), rec["X"].copy()
        sm_o, tr_o = O.solve(rec["uv"], rec["cam_idx"], rec["pt_idx"], rec["K"], r, t, X)
        sm_g, tr_g = rec["summary"], rec["trace"]
        assert sm_g.termination_type == sm_o["termination_type"]
        assert sm_g.num_iterations == sm_o["num_iterations"]
        assert [x["step_is_successful"] for x in tr_g] == [x["step_is_successful"] for x in tr_o]
        assert abs(sm_g.final_cost - sm_o["final_cost"]) <= 1e-9 * max(sm_o["final_cost"], 1e-300)
        assert _rel(rec["X_out"], X) < 1e-6
        assert _rel(rec["t_out"], t) < 1e-6
        assert _rel(rec["rot_out"], r, floor=1e-2) < 1e-6


def test_estimated_start_geometry_matches_ground_truth(run60):
    s = run60
    st = s.stream
    votes = {}
    for kf in s.kfs:
        lid = st.frame(kf.no)[2]
        for j in np.flatnonzero(kf.pt3d >= 0):
            votes.setdefault(int(kf.pt3d[j]), []).append(int(lid[j]))
    ids = np.array([k for k, v in votes.items() if len(set(v)) == 1 and v[0] >= 0])
    assert len(ids) >= 0.97 * len(votes)
    lm = np.array([votes[k][0] for k in ids])
    X = s.map.getPointsAtIdx(ids)
    sc, R, t = _umeyama(X, st.L[lm])
    d = np.linalg.norm((sc * X @ R.T + t) - st.L[lm], axis=1)
    C = np.array([-_rodrigues(f.rot).T @ f.t for f in s.kfs])
    Cg = np.array([-_rodrigues(st.pose(f.no)[0]).T @ st.pose(f.no)[1] for f in s.kfs])
    err = np.linalg.norm((sc * C @ R.T + t) - Cg, axis=1)
    print("point error median / p90", np.median(d), np.percentile(d, 90), "centre error max", err.max(), "scale", sc)
    assert np.median(d) < 0.1
    assert err.max() < 0.06
    dm = np.linalg.norm(np.diff(sc * C @ R.T, axis=0), axis=1)
    dg = np.linalg.norm(np.diff(Cg, axis=0), axis=1)
    print("step lengths", dm, dg)
    assert np.max(np.abs(dm - dg) / dg) < 0.05


def test_estimated_start_on_brisk_video_takes_the_homography_branch():
    s = LiveSfM(BriskVideoStream(), init="estimate", init_gap=5)
    try:
        s.run(40)
        st = s.stream
        _attempts_follow_reference(s)
        models = [e["model"] for e in s.init_log]
        assert models[-1] == 1 and not any(models[:-1])      # retried on model 0, then the homography branch
        assert len(models) > 1                                # (the parallax rule held the first attempts back)
        assert [f.no for f in s.kfs][:2] == [0, s.init_log[-1]["frame"]]
        assert s.lost == 0 and len(s.kfs) >= 3
        kf0 = s.kfs[0]
        have = np.flatnonzero(kf0.pt3d >= 0)
        X = s.map.getPointsAtIdx(kf0.pt3d[have].astype(np.int32))
        for f in s.kfs[1:]:
            uv, z = _project(s.K, f.rot, f.t, X)
            truth = st.video.map_points(kf0.no, f.no, kf0.pts[have])
            inside = (z > 0) & (truth[:, 0] > 0) & (truth[:, 0] < st.video.w) & (truth[:, 1] > 0) & \
                (truth[:, 1] < st.video.h)
            e = np.linalg.norm(uv[inside] - truth[inside], axis=1)
            print(f"keyframe {f.no}: {inside.sum()} points of keyframe 0, image motion error median "
                  f"{np.median(e):.3f} px, p90 {np.percentile(e, 90):.3f} px")
            med_max, p90_max = BRISK_BOUNDS.get(int(f.no), (1.0, 3.0))
            assert np.median(e) < med_max and np.percentile(e, 90) < p90_max
    finally:
        s.close()


def test_default_run_is_bitwise_the_parent_commits():
    with open(GOLDEN) as f:
        g = json.load(f)
    s = LiveSfM(KeypointStream())
    try:
        s.run(30)
        assert s.init == "known"
        assert [int(f.no) for f in s.kfs] == g["keyframes"]
        assert [[float(x).hex() for x in f.rot] for f in s.kfs] == g["rot"]
        assert [[float(x).hex() for x in f.t] for f in s.kfs] == g["t"]
        assert [int(x) for x in s.map.size()] == g["map_size"]
        assert [float(x).hex() for x in s.prev.rot] == g["prev_rot"]
        assert [float(x).hex() for x in s.prev.t] == g["prev_t"]
        assert {k: int(v) for k, v in s.stats.items()} == g["stats"]
    finally:
        s.close()


def test_incremental_mapper_estimated_start():
    """the same switch in sfm_amd.mapping's pipeline (KLT tracks of a textured
    plane): attempts until the two-view initialisation accepts, then the map
    and the keyframe BA as with the known pose"""
    from sfm_amd.mapping import IncrementalMapper
    from sfm_amd.video import SyntheticVideo
    v = SyntheticVideo()
    m = IncrementalMapper(v, kf_every=10, init="estimate")
    try:
        for k in range(41):
            m.process_frame(v.frame(k))
        print("attempts", m.init_log, "keyframes", m.kf_frames)
        assert m.init_log and m.init_log[-1]["model"] == 1 and not any(e["model"] for e in m.init_log[:-1])
        assert m.kf_frames[:2] == [0, m.init_log[-1]["frame"]] and len(m.kf_frames) >= 3
        assert m.X.shape[0] > 100 and len(m.ba_log) == len(m.kf_frames) - 1
        for rec in m.ba_log:
            assert rec["summary"].final_cost < rec["summary"].initial_cost
        assert m.pnp_frames >= 41 - m.kf_frames[1] - 5
    finally:
        m.close()
