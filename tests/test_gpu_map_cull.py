"""GPU: map-point and keyframe culling in the device map store
(sfm_map_remove_points_threshold / _remove_points / _remove_frame /
_cull_keyframes and the counters, map_store.hip) against the restatement
tests/cmap_cull_ref.py: the pinned hand-checked case through the ABI, seeded
histories compared query by query after every round, one larger map (keyframe
lists above one workgroup's width), the error cases with the store proved
unchanged, and a map that never culls."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cmap_cull_ref import CMapCullRef  # noqa: E402
from oracle.cmap_oracle import CMapOracle  # noqa: E402
import cull_cases  # noqa: E402
from cull_cases import Mirror  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("desc_bytes", [64, 16])
def test_pinned_case_through_the_abi(desc_bytes):
    m = Mirror(desc_bytes)
    try:
        cull_cases.pinned_case(m, desc_bytes)
    finally:
        m.close()


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_random_histories_match_the_restatement(seed):
    # the conditions come from the restatement alone (also a CPU test)
    c = cull_cases.random_history(CMapCullRef(), seed, rounds=8, rate=0.5)
    assert c["size"] and c["score"] and c["rule2"] and c["kf"] and c["doubled"] and c["unlisted"], c
    m = Mirror()
    try:
        assert cull_cases.random_history(m, seed, rounds=8, rate=0.5) == c
    finally:
        m.close()


def test_rate_0_9_and_short_descriptors():
    c = cull_cases.random_history(CMapCullRef(16), 1, rounds=8, rate=0.9, desc_bytes=16)
    assert c["kf"] and c["size"] and c["score"] and c["rule2"], c
    m = Mirror(16)
    try:
        assert cull_cases.random_history(m, 1, rounds=8, rate=0.9, desc_bytes=16) == c
    finally:
        m.close()


def test_larger_map():
    """Keyframe lists above 1024 points (k_walk_keyframes strides its one
    workgroup over them) and several workgroups of observations."""
    kw = dict(rounds=5, rate=0.5, n0=1500, n_new=300, check_every_round=False)
    c = cull_cases.random_history(CMapCullRef(), 0, **kw)
    assert c["size"] > 1000 and c["score"] and c["rule2"] > 100 and c["kf"] >= 2, c
    m = Mirror()
    try:
        assert cull_cases.random_history(m, 0, **kw) == c
        assert m.dev.size()[1] > 1024
    finally:
        m.close()


def test_score_edges_on_the_device():
    m = Mirror()
    try:
        # kfAlive 1, 3 observations each: views / time = 5 / 20 kept, 4 / 17 culled, 3 / 0 kept (+inf)
        a = m.addNewPoints(np.zeros((2, 3)), [[0, 1]] * 3, [0, 1, 2])
        m.updatePointViews([0, 0, 1])
        m.incrementMapAge(17, 0)
        b = m.addNewPoints(np.zeros((1, 3)), [[2]] * 3, [0, 1, 2])
        m.incrementMapAge(0, 1)
        m.check_all()
        # p0 5 / 17, p1 4 / 17, p2 3 / 0
        cull, status = m.removePointsThreshold()
        assert list(cull) == [1] and list(status) == [0, -1, 0] and list(a) == [0, 1] and list(b) == [2]
        m.incrementMapAge(3, 0)  # p0 5 / 20: not below 0.25f
        assert list(m.removePointsThreshold()[0]) == []
        m.incrementMapAge(1, 0)  # p0 5 / 21
        assert list(m.removePointsThreshold()[0]) == [0]
        m.check_all()
    finally:
        m.close()


def test_errors_leave_the_store_unchanged():
    """Mirror re-queries everything after each refused call."""
    m = Mirror()
    try:
        m.addNewPoints(np.zeros((3, 3)), [[0, 1, 2], [3, 4, 5]], [0, 5])
        for _ in range(2):
            m.addDescriptors([0, 1, 2], np.arange(3 * 64, dtype=np.uint8).reshape(3, 64))
        m.addPointMatches([1], [9], 3)  # out of order: p1's list is [0, 5, 3]
        m.addDescriptors([1], np.zeros((1, 64), np.uint8))
        m.addPointMatches([2], [9], 7)  # no descriptor row for p2's third observation
        for f, pts in [(9, [0]), (4, [0]), (3, [0, 1]), (7, [2]), (0, [0, 0]), (0, [1, 0, 0]), (0, [3]),
                       (0, [-1])]:
            with pytest.raises(ValueError):
                m.removeFrame(f, pts)
        for bad in ([1, 0], [0, 0], [5]):
            with pytest.raises(ValueError):
                m.removePoints(bad)
        # a keyframe cull that fails keeps the earlier keyframes' removals and names (frame, point)
        import sfm_amd
        kfs = [(0, [0, 1, 2]), (4, [0]), (5, [0, 1, 2])]
        with pytest.raises(ValueError):
            m.ref.cullKeyFrames(kfs, 0, 0.0)
        with pytest.raises(sfm_amd.SfmError, match=r"removeFrame\(4\): point 0 ") as e:
            m.dev.cullKeyFrames(kfs, 0, 0.0)
        assert e.value.code == cull_cases.SFM_EINVAL and e.value.culled.tolist() == [1, 0, 0]
        m.check_all()
        m.removePoints([0])
        m.check_all()
        for call in (lambda: m.removeFrame(5, [0]), lambda: m.updatePointViews([0]), lambda: m.removePoints([0]),
                     lambda: m.addPointMatches([0], [1], 9), lambda: m.arePointsSeenByAtLeast([0], 1, 0.5),
                     lambda: m.addDescriptors([0], np.zeros((1, 64), np.uint8))):
            with pytest.raises(ValueError):
                call()
        with pytest.raises(sfm_amd.SfmError):
            m.dev.getRepresentativeDescriptors([0])
        # too small a capacity removes nothing
        import ctypes
        from sfm_amd._ffi import lib, ptr
        m.incrementMapAge(0, 4)
        out, n = np.zeros(1, np.int32), ctypes.c_int32()
        rc = lib().sfm_map_remove_points_threshold(m.dev._h, 3, 0.25, 1, ptr(out), ctypes.byref(n), None)
        assert rc == cull_cases.SFM_EINVAL and n.value == 2
        m.check_all()
        assert list(m.removePointsThreshold()[0]) == [1, 2]
        m.check_all()
    finally:
        m.close()


def test_a_map_that_never_culls_answers_as_before():
    """The existing queries against the plain CMap restatement (oracle/), the
    history shaped as tests/test_gpu_map.py's; the new counters alongside."""
    import sfm_amd
    rng = np.random.default_rng(5)
    dm, om = sfm_amd.DeviceMap(), CMapOracle()
    try:
        frames = []
        for k in range(6):
            f = 10 * k + 3
            frames.append(f)
            n_pts = len(om.pts3D)
            if k:
                X = rng.normal(size=(200, 3))
                i2 = rng.integers(0, 2000, size=(2, 200)).astype(np.int32)
                a = dm.addNewPoints(X, i2, [frames[-2], f])
                assert a.tolist() == om.addNewPoints(X, i2, [frames[-2], f])
                for _ in range(2):
                    d = rng.integers(0, 256, size=(200, 64), dtype=np.uint8)
                    dm.addDescriptors(a, d)
                    om.addDescriptors(a, d)
            if n_pts:
                idx = rng.choice(n_pts, size=min(n_pts, 150), replace=False).astype(np.int32)
                idx = np.concatenate([idx, idx[:3]])
                i2 = rng.integers(0, 2000, size=len(idx)).astype(np.int32)
                dm.addPointMatches(idx, i2, f)
                om.addPointMatches(idx, i2, f)
                d = rng.integers(0, 256, size=(len(idx), 64), dtype=np.uint8)
                dm.addDescriptors(idx, d)
                om.addDescriptors(idx, d)
        assert dm.size()[:2] == (len(om.pts3D), len(om.mm)) and dm.getNPoints() == len(om.pts3D)
        for (d3, d2), f in zip(dm.getPointsInFrameMulti(frames), frames):
            r3, r2 = om.getPointsInFrame(f)
            assert d3.tolist() == r3 and d2.tolist() == r2
            e3, e2 = dm.getPointsInFrame(f)
            assert e3.tolist() == r3 and e2.tolist() == r2
        assert dm.getPointsInFrames(frames[1:3]).tolist() == om.getPointsInFrames(frames[1:3])
        q = np.arange(len(om.pts3D), dtype=np.int32)
        dd, db = dm.getRepresentativeDescriptors(q, return_best=True)
        rb, rd = om.getRepresentativeDescriptors(q)
        assert np.array_equal(db, rb) and np.array_equal(dd, rd)
        st = dm.pointState(q)
        assert np.array_equal(st[:, 3], [len(x) for x in om.frameNo]) and np.array_equal(st[:, 2], st[:, 3])
        assert not st[:, :2].any() and st[:, 4].all()
    finally:
        dm.close()
