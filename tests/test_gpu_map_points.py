"""GPU: map-point creation on the device (sfm_matcher_pair_points,
sfm_matcher_refind_points, sfm_filter_matches, sfm_map_add_keyframe_rows;
CSfM::mapping, CSfM.cpp:118-227) against the calls it fuses and the
fixed-order restatement tests/map_points_ref.py, bit for bit, and the live
loop with device_mapping=True against the oracle and the ground truth."""
import ctypes

import numpy as np
import pytest

import map_points_cases as C
import map_points_ref as ref
from map_points_composed import composed
from oracle import ffi as O
from sfm_amd._ffi import SfmError, lib, ptr
from sfm_amd.cmap import DeviceMap
from sfm_amd.live import MAX_REPR_ERR, KeypointStream, LiveSfM
from sfm_amd.mapping import _rodrigues, filter_matches, triangulate_points
from sfm_amd.matcher import FeatureMatcher
from test_gpu_live import _rel, _umeyama

pytestmark = pytest.mark.gpu


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


class _Pair:
    """KeypointStream(n_landmarks=N) frames 0 and 5 with the stream's poses,
    stored as keyframes 0 and 1; a seeded 30 % of the frame-5 positions are
    displaced by up to +-25 px (inside the 40 px match window, mostly outside
    the 7 px filter)."""

    def __init__(self, n_landmarks, desc_bytes=64):
        st = KeypointStream(n_landmarks=n_landmarks, desc_bytes=desc_bytes)
        self.K = st.K
        self.p0, self.d0, self.l0 = st.frame(0)
        self.p1, self.d1, self.l1 = st.frame(5)
        rng = np.random.default_rng(n_landmarks)
        moved = rng.random(len(self.p1)) < 0.3
        self.p1 = self.p1.copy()
        self.p1[moved] += rng.uniform(-25.0, 25.0, (int(moved.sum()), 2))
        (r0, self.t0), (r1, self.t1) = st.pose(0), st.pose(5)
        self.R0, self.R1 = _rodrigues(r0), _rodrigues(r1)
        self.m = FeatureMatcher(desc_bytes)
        self.m.store_keyframe(0, self.p0, self.d0)
        self.m.store_keyframe(1, self.p1, self.d1)

    def fused(self, idx0, idx1, R1=None, t1=None, **kw):
        return self.m.pair_points(0, idx0, 1, idx1, self.K, self.R0, self.t0, self.K,
                                  self.R1 if R1 is None else R1, self.t1 if t1 is None else t1, MAX_REPR_ERR, **kw)

    def composed(self, idx0, idx1):
        return composed(self.m, 0, self.p0, idx0, 1, self.p1, idx1, self.K, self.R0, self.t0, self.R1, self.t1,
                        MAX_REPR_ERR)


@pytest.fixture(scope="module")
def pairs():
    made = {}

    def get(n):
        if n not in made:
            made[n] = _Pair(n)
        return made[n]
    yield get
    for p in made.values():
        p.m.close()


def _check_fused(p, idx0, idx1, label):
    m0, m1, X, n_matched = p.fused(idx0, idx1)
    pi, ci, Xa, keep = p.composed(idx0, idx1)
    print(f"{label}: rows {len(idx0)} x {len(idx1)}, matched {n_matched}, kept {len(m0)}")
    assert n_matched == len(pi)
    assert np.array_equal(m0, pi[keep]) and np.array_equal(m1, ci[keep])
    assert _bits(X, Xa[keep])
    return n_matched, len(m0)


@pytest.mark.parametrize("n_landmarks", [100, 1200, 8000, 24000])
def test_pair_points_equals_match_triangulate_filter(pairs, n_landmarks):
    """Whole frames: the match counts cross one wave (64), one block (256)
    and one compaction step (1024 flags)."""
    p = pairs(n_landmarks)
    nm, nk = _check_fused(p, np.arange(len(p.p0)), np.arange(len(p.p1)), f"N = {n_landmarks}")
    lo, hi = {100: (1, 63), 1200: (65, 255), 8000: (257, 1023), 24000: (1025, 10 ** 6)}[n_landmarks]
    assert lo <= nm <= hi, (nm, lo, hi)
    assert 0 < nk < nm or nm < 4


def test_pair_points_with_no_and_one_match(pairs):
    p = pairs(1200)
    both = np.intersect1d(p.l0[p.l0 >= 0], p.l1[p.l1 >= 0])
    pi, ci = p.m.match_keyframes(0, np.arange(len(p.p0)), 1, np.arange(len(p.p1)))
    q, t = int(pi[0]), int(ci[0])
    far = np.flatnonzero(np.linalg.norm(p.p1 - p.p0[q], axis=1) > 100.0)[:2]
    assert len(both) and len(far) == 2
    assert _check_fused(p, [q], far, "no match")[0] == 0
    assert _check_fused(p, [q], [int(far[0]), t], "one match")[0] == 1
    # n0 == 0 or n1 < 2: no matches, as the existing overloads
    assert p.fused([], [t, int(far[0])])[3] == 0 and p.fused([q], [t])[3] == 0
    # a reversed subset order is the matcher's order still
    _check_fused(p, np.arange(len(p.p0))[::-1].copy(), np.arange(len(p.p1))[::-1].copy(), "reversed")


def test_pair_points_degenerate_poses_keep_nothing(pairs):
    """Both keyframes at the first one's pose (R = I, t = 0): F = 0, the
    distances are NaN, nothing is kept, the match count is what it was."""
    p = pairs(8000)
    assert np.array_equal(p.R0, np.eye(3)) and not p.t0.any()
    i0, i1 = np.arange(len(p.p0)), np.arange(len(p.p1))
    m0, m1, X, nm = p.fused(i0, i1, R1=p.R0, t1=p.t0)
    assert len(m0) == len(m1) == len(X) == 0
    assert nm == len(p.m.match_keyframes(0, i0, 1, i1)[0]) > 50


def test_last_time_covers_a_pair_points_call(pairs):
    """On a handle whose only device call was pair_points."""
    p = pairs(1200)
    m = FeatureMatcher(64)
    try:
        m.store_keyframe(0, p.p0, p.d0)
        m.store_keyframe(1, p.p1, p.d1)
        assert m.last_time_ms() == (0.0, 0.0)
        m0 = m.pair_points(0, np.arange(len(p.p0)), 1, np.arange(len(p.p1)), p.K, p.R0, p.t0, p.K, p.R1, p.t1,
                           MAX_REPR_ERR)[0]
        knn_ms, total_ms = m.last_time_ms()
    finally:
        m.close()
    print(f"pair_points device time: 2-NN {knn_ms:.4f} ms, whole call {total_ms:.4f} ms")
    assert len(m0) > 0
    assert np.isfinite(knn_ms) and np.isfinite(total_ms) and 0 < knn_ms <= total_ms


def test_filter_matches_equals_the_restatement():
    for s in C.all_scenes():
        R0, R1 = _rodrigues(s["r0"]), _rodrigues(s["r1"])
        keep, F = filter_matches(s["uv0"], s["uv1"], s["X"], C.K, R0, s["t0"], C.K, R1, s["t1"], C.MAX_ERR,
                                 return_F=True)
        want = ref.filter_matches(s["uv0"], s["uv1"], s["X"], C.K, R0, s["t0"], C.K, R1, s["t1"], C.MAX_ERR)
        print(f"{s['name']}: kept {int(keep.sum())} of {len(keep)}")
        assert np.array_equal(keep, want), (s["name"], np.flatnonzero(keep != want)[:10])
        assert _bits(F, ref.fundamental_from_poses(C.K, R0, s["t0"], C.K, R1, s["t1"])), s["name"]
    for s, want in C.constructed():      # each rule's own rejections, by index
        keep = filter_matches(s["uv0"], s["uv1"], s["X"], C.K, _rodrigues(s["r0"]), s["t0"], C.K,
                              _rodrigues(s["r1"]), s["t1"], C.MAX_ERR)
        assert np.flatnonzero(~keep).tolist() == sorted(i for v in want.values() for i in v)
    # a skewed K goes through the closed-form inverse
    Ks = np.array([[1000.0, 2.5, 640.0], [0.0, 990.0, 360.0], [0.0, 0.0, 1.0]])
    s = C.scene(65, 3)
    R0, R1 = _rodrigues(s["r0"]), _rodrigues(s["r1"])
    _, F = filter_matches(s["uv0"], s["uv1"], s["X"], Ks, R0, s["t0"], C.K, R1, s["t1"], C.MAX_ERR, return_F=True)
    assert _bits(F, ref.fundamental_from_poses(Ks, R0, s["t0"], C.K, R1, s["t1"]))


def test_refind_points_equals_match_keyframes_on_projections(pairs):
    p = pairs(8000)
    m0, m1, X, _ = p.fused(np.arange(len(p.p0)), np.arange(len(p.p1)))
    assert len(m0) > 100
    X = X.copy()
    X[3] = p.R1.T @ (np.array([0.1, 0.1, -5.0]) - p.t1)        # behind keyframe 1
    X[4, 2] = np.nan
    un = np.setdiff1d(np.arange(len(p.p1)), m1[::2]).astype(np.int32)   # half of the partners stay
    for rows in (m0, m0[::-1].copy()):
        Xr = X if rows is m0 else X[::-1].copy()
        uv = ref.project(p.K, p.R1, p.t1, Xr)
        a0, a1 = p.m.refind_points(0, rows, Xr, p.K, p.R1, p.t1, 1, un, 0.8, 0.0, MAX_REPR_ERR)
        b0, b1 = p.m.match_keyframes(0, rows, 1, un, uv, 0.8, 0.0, MAX_REPR_ERR)
        print(f"re-find: {len(rows)} points against {len(un)} rows: {len(a0)} found")
        assert np.array_equal(a0, b0) and np.array_equal(a1, b1)
        assert 20 < len(a0) < len(rows)
        bad = np.flatnonzero(np.isin(rows, m0[[3, 4]]))
        assert not np.isin(bad, a0).any()


@pytest.mark.parametrize("desc_bytes", [64, 8])
def test_add_keyframe_rows_equals_point_matches_plus_descriptors(desc_bytes):
    rng = np.random.default_rng(desc_bytes)
    n_rows = 2000
    desc = rng.integers(0, 256, (n_rows, desc_bytes), dtype=np.uint8)
    pts = rng.uniform(0, 1000, (n_rows, 2))
    mt = FeatureMatcher(desc_bytes)
    mt.store_keyframe(2, pts, desc)
    a, b = DeviceMap(desc_bytes), DeviceMap(desc_bytes)
    try:
        P = 1600
        X = rng.normal(size=(P, 3))
        for mp in (a, b):
            idx = mp.addNewPoints(X, np.arange(P).reshape(1, -1), [7])
            mp.addDescriptors(idx, desc[:P])
        frame = 10
        for n in (1, 65, 1500):
            for with_obs in (True, False):
                p3 = rng.permutation(P)[:n].astype(np.int32)
                rows = rng.integers(0, n_rows, n).astype(np.int32)   # repeats allowed
                if with_obs:
                    a.addPointMatches(p3, rows, frame)
                a.addDescriptors(p3, desc[rows])
                b.addKeyframeRows(mt, 2, frame, p3, rows, with_observations=with_obs)
                _same_map(a, b, [7, frame])
                frame += 1
        # after a removal slots and live points differ
        gone = np.sort(rng.permutation(P)[:200]).astype(np.int32)
        for mp in (a, b):
            mp.removePoints(gone)
        live = np.setdiff1d(np.arange(P), gone).astype(np.int32)
        p3, rows = live[rng.permutation(len(live))[:700]], rng.integers(0, n_rows, 700).astype(np.int32)
        a.addPointMatches(p3, rows, frame)
        a.addDescriptors(p3, desc[rows])
        b.addKeyframeRows(mt, 2, frame, p3, rows)
        _same_map(a, b, [7, frame], live)
        with pytest.raises(SfmError, match="removed"):
            b.addKeyframeRows(mt, 2, frame + 1, gone[:3], rows[:3])
        _same_map(a, b, [7, frame], live)
    finally:
        a.close()
        b.close()
        mt.close()


def _same_map(a, b, frames, live=None):
    assert a.size() == b.size()
    P = a.size()[0]
    for f in frames:
        for x, y in zip(a.getPointsInFrame(f), b.getPointsInFrame(f)):
            assert np.array_equal(x, y)
    ids = np.arange(P, dtype=np.int32)
    assert np.array_equal(a.pointState(ids), b.pointState(ids))
    ids = ids if live is None else live
    ra, ba = a.getRepresentativeDescriptors(ids, return_best=True)
    rb, bb = b.getRepresentativeDescriptors(ids, return_best=True)
    assert np.array_equal(ra, rb) and np.array_equal(ba, bb)


def test_errors_leave_the_handles_usable(pairs):
    p = pairs(1200)
    i0, i1 = np.arange(len(p.p0), dtype=np.int32), np.arange(len(p.p1), dtype=np.int32)
    good = p.fused(i0, i1)
    nk = len(good[0])
    assert nk > 1

    def refused(fn, *a, **k):
        with pytest.raises(SfmError) as e:
            fn(*a, **k)
        assert e.value.code == -22 and len(str(e.value).split(": ", 1)[1]) > 3, str(e.value)
        return e.value

    K, R0, t0, R1, t1 = p.K, p.R0, p.t0, p.R1, p.t1
    refused(p.m.pair_points, 9, i0, 1, i1, K, R0, t0, K, R1, t1)                    # unstored slot
    refused(p.m.pair_points, 0, [len(p.p0)], 1, i1, K, R0, t0, K, R1, t1)           # row out of range
    refused(p.m.pair_points, 0, i0, 1, [0, -1], K, R0, t0, K, R1, t1)
    refused(p.m.pair_points, 0, i0, 1, i1, K, R0 * np.nan, t0, K, R1, t1)           # non-finite matrix
    refused(p.m.pair_points, 0, i0, 1, i1, K, R0, t0, K, R1, t1, max_err=np.inf)
    e = refused(p.m.pair_points, 0, i0, 1, i1, K, R0, t0, K, R1, t1, capacity=nk - 1)
    assert e.n_kept == nk                                                           # still reported
    # NULL outputs, straight at the C ABI
    m9 = [np.ascontiguousarray(m, np.float64).reshape(9) for m in (K, R0, K, R1)]
    o = np.zeros(len(i0), np.int32)
    X = np.zeros((len(i0), 3))
    c = ctypes.c_int32(0)
    for outs in ((None, ptr(o), ptr(X), ctypes.byref(c), ctypes.byref(c)),
                 (ptr(o), ptr(o), None, ctypes.byref(c), ctypes.byref(c)),
                 (ptr(o), ptr(o), ptr(X), None, ctypes.byref(c))):
        rc = lib().sfm_matcher_pair_points(p.m._h, 0, ptr(i0), len(i0), 1, ptr(i1), len(i1), 0.8, 1.5, 40.0,
                                           ptr(m9[0]), ptr(m9[1]), ptr(t0), ptr(m9[2]), ptr(m9[3]), ptr(t1), 7.0,
                                           len(i0), *outs)
        assert rc == -22 and lib().sfm_last_error()
    rc = lib().sfm_matcher_refind_points(p.m._h, 0, ptr(i0), 1, ptr(X), ptr(m9[0]), ptr(m9[1]), ptr(t0), 1, ptr(i1),
                                         len(i1), 0.8, 0.0, 7.0, None, ptr(o), ctypes.byref(c))
    assert rc == -22
    for outs in ((None, ptr(o)), (ptr(o), None)):
        rc = lib().sfm_matcher_match_keyframes(p.m._h, 0, ptr(i0), len(i0), None, 1, ptr(i1), len(i1), 0.8, 1.5, 40.0,
                                               *outs, ctypes.byref(c))
        assert rc == -22 and lib().sfm_last_error()
    Xq = good[2][:2]
    refused(p.m.refind_points, 0, [5, 5], Xq, K, R1, t1, 1, i1)                     # repeated q_idx
    refused(p.m.refind_points, 9, [5, 6], Xq, K, R1, t1, 1, i1)
    refused(p.m.refind_points, 0, [5, 6], Xq, K, R1, t1, 1, [len(p.p1)])
    # the map's checks: widths differ, slot, row, removed point
    mp, mp8 = DeviceMap(64), DeviceMap(8)
    try:
        for x in (mp, mp8):
            x.addNewPoints(np.zeros((4, 3)), np.arange(4).reshape(1, -1), [0])
        refused(mp8.addKeyframeRows, p.m, 0, 1, [0, 1], [0, 1])
        refused(mp.addKeyframeRows, p.m, 9, 1, [0, 1], [0, 1])
        refused(mp.addKeyframeRows, p.m, 0, 1, [0, 1], [0, len(p.p0)])
        refused(mp.addKeyframeRows, p.m, 0, 1, [0, 4], [0, 1])
        assert mp.size() == (4, 4, 0)
        mp.addKeyframeRows(p.m, 0, 1, [0, 1], [0, 1])                               # one good call
        assert mp.size() == (4, 6, 2)
        assert np.array_equal(mp.getRepresentativeDescriptors([0, 1]), p.d0[:2])
    finally:
        mp.close()
        mp8.close()
    again = p.fused(i0, i1)                                                         # and the matcher's
    assert all(np.array_equal(x, y) for x, y in zip(good[:3], again[:3])) and good[3] == again[3]
    a0, _ = p.m.refind_points(0, i0[good[0]], good[2], K, R1, t1, 1, i1, 0.8, 0.0, 7.0)
    assert len(a0) > 0


# ---- the live loop -------------------------------------------------------------

@pytest.fixture(scope="module")
def run60():
    s = LiveSfM(KeypointStream(), device_mapping=True)
    s.run(60)
    yield s
    s.close()


def test_loop_loses_no_frame_and_replays_through_the_composed_calls(run60):
    s = run60
    d = LiveSfM(KeypointStream())
    try:
        d.run(60)
        print("device_mapping keyframes", [f.no for f in s.kfs], s.stats)
        print("default        keyframes", [f.no for f in d.kfs], d.stats)
    finally:
        d.close()
    assert s.lost == 0 and s.stats["tracked"] == 60 - 5 - 1
    assert len(s.kfs) >= 5 and len(s.map_log) >= 6 and s.stats["new_points"] > 500
    kept = 0
    for e in s.map_log:
        pi, ci = s.matcher.match_keyframes(e["slot0"], e["idx0"], e["slot1"], e["idx1"])
        kf0 = next(f for f in s.kfs if f.slot == e["slot0"])
        kf1 = next(f for f in s.kfs if f.slot == e["slot1"])
        uv0, uv1 = kf0.pts[e["idx0"][pi]], kf1.pts[e["idx1"][ci]]
        P = np.stack([ref.compose_P(e["K"], e["R0"], e["t0"]), ref.compose_P(e["K"], e["R1"], e["t1"])])
        X = triangulate_points(np.zeros(len(pi), np.int32), np.ones(len(pi), np.int32), uv0, uv1, P)
        keep = ref.filter_matches(uv0, uv1, X, e["K"], e["R0"], e["t0"], e["K"], e["R1"], e["t1"], MAX_REPR_ERR)
        assert e["n_matched"] == len(pi)
        assert np.array_equal(e["m0"], pi[keep]) and np.array_equal(e["m1"], ci[keep])
        assert _bits(e["X"], X[keep])
        kept += len(e["m0"])
    assert kept == s.stats["new_points"] - len(s.ba_log[0]["X"])   # all but the initial pair's


def test_loop_every_keyframe_ba_matches_oracle(run60):
    assert len(run60.ba_log) == len(run60.kfs) - 1
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


def _associations_hold(s):
    for kf in s.kfs:
        p3, p2 = s.map.getPointsInFrame(kf.no)
        assert len(p3) == len(p2) == kf.n_matched()
        assert (kf.pt3d[p2] == p3).all()


def test_loop_map_store_and_ground_truth(run60):
    s, st = run60, run60.stream
    _associations_hold(s)
    cov = s.map.getPointsInFrames([f.no for f in s.kfs])
    assert cov.tolist() == list(range(s.map.size()[0]))
    # every observation carries its keyframe's descriptor row
    n_pts, n_obs, n_rows = s.map.size()
    assert n_rows == n_obs
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
    Cc = np.array([-_rodrigues(f.rot).T @ f.t for f in s.kfs])
    Cg = np.array([-_rodrigues(st.pose(f.no)[0]).T @ st.pose(f.no)[1] for f in s.kfs])
    err = np.linalg.norm((sc * Cc @ R.T + t) - Cg, axis=1)
    print("device_mapping: point error median", np.median(d), "centre error max", err.max())
    assert np.median(d) < 0.1
    assert err.max() < 0.06


def test_loop_composes_with_culling():
    s = LiveSfM(KeypointStream(), device_mapping=True, cull=True)
    try:
        s.run(60)
        print("device_mapping + cull keyframes", [f.no for f in s.kfs], s.stats)
        assert s.lost == 0 and s.stats["tracked"] == 60 - 5 - 1
        assert len(s.map_log) >= 6 and s.stats["culled_points"] > 0
        _associations_hold(s)
        assert s.map.getNPoints() == s.map.size()[0] - s.stats["culled_points"]
    finally:
        s.close()
