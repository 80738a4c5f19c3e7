"""CPU: the culling restatement (tests/cmap_cull_ref.py) on the pinned
hand-checked case, the score edges, the error cases and the
ceil(ratio n) threshold of CMap::arePointsSeenByAtLeast."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cmap_cull_ref import CMapCullRef, lower_bound  # noqa: E402
import cull_cases  # noqa: E402


def test_pinned_case():
    cull_cases.pinned_case(CMapCullRef())


def _point(views, time, kf=1, n_obs=3):
    m = CMapCullRef()
    m.addNewPoints(np.zeros((1, 3)), [[0]] * n_obs, list(range(n_obs)))
    m.updatePointViews([0] * (views - n_obs))
    m.incrementMapAge(time, kf)
    return m


@pytest.mark.parametrize("views,time,culled", [(5, 20, False), (4, 17, True), (3, 0, False)])
def test_score_edges(views, time, culled):
    """float32 views / time against 0.25f as written: 5 / 20 is not below,
    4 / 17 is, 3 / 0 is +inf."""
    m = _point(views, time)
    cull, status = m.removePointsThreshold()
    assert cull == ([0] if culled else []) and status.tolist() == [-1 if culled else 0]


def test_rules_by_age():
    assert _point(10, 10, kf=0, n_obs=1).removePointsThreshold()[0] == []   # too young for either rule
    assert _point(10, 10, kf=3, n_obs=2).removePointsThreshold()[0] == [0]  # rule 1, size
    assert _point(10, 10, kf=4, n_obs=2).removePointsThreshold()[0] == [0]  # rule 2
    assert _point(1, 100, kf=4, n_obs=3).removePointsThreshold()[0] == []   # old: the score no longer counts


def test_lower_bound_is_the_bisection_not_a_search():
    assert [lower_bound([0, 5, 15], v) for v in (0, 5, 6, 15, 16)] == [0, 1, 2, 2, 3]
    assert lower_bound([25, 5, 15], 5) == 0  # unsorted: where the halving lands


def _two_frame_map():
    m = CMapCullRef()
    m.addNewPoints(np.zeros((3, 3)), [[0, 1, 2], [3, 4, 5]], [0, 5])
    for _ in range(2):
        m.addDescriptors([0, 1, 2], np.zeros((3, 64), np.uint8))
    return m


def _snapshot(m):
    return ([list(f) for f in m.frameNo], [list(i) for i in m.pts2DIdx], [len(d) for d in m.descriptor], list(m.mm),
            list(m.pif), list(m.ptsViews), list(m.live))


def test_error_cases_leave_the_map_unchanged():
    m = _two_frame_map()
    m.addPointMatches([1], [9], 3)  # out of order: p1's list is [0, 5, 3]
    m.addDescriptors([1], np.zeros((1, 64), np.uint8))
    m.addPointMatches([2], [9], 7)  # no descriptor row for p2's third observation
    s = _snapshot(m)
    for f, pts in [(9, [0]),            # absent frame, past the end
                   (4, [0]),            # absent frame, lands on 5
                   (3, [0, 1]),         # the bisection on [0, 5, 3] ends past the end
                   (7, [2]),            # too few descriptor rows
                   (0, [0, 0]),         # listed twice, held once
                   (0, [1, 0, 0]),      # the same after a point that succeeds, which must be restored
                   (0, [3]), (0, [-1])]:  # out of range
        with pytest.raises(ValueError):
            m.removeFrame(f, pts)
        assert _snapshot(m) == s, (f, pts)
    for bad in ([1, 0], [0, 0], [5]):
        with pytest.raises(ValueError):
            m.removePoints(bad)
        assert _snapshot(m) == s
    m.removePoints([0])
    s = _snapshot(m)
    for call in (lambda: m.removeFrame(0, [0]), lambda: m.updatePointViews([0]), lambda: m.removePoints([0]),
                 lambda: m.addPointMatches([0], [1], 9), lambda: m.arePointsSeenByAtLeast([0], 1, 0.5),
                 lambda: m.addDescriptors([0], np.zeros((1, 64), np.uint8)),
                 lambda: m.getRepresentativeDescriptors([0])):
        with pytest.raises(ValueError):
            call()
        assert _snapshot(m) == s
    assert m.getPointsAtIdx([0]).shape == (1, 3)
    # a keyframe cull that fails keeps the earlier keyframes' removals
    m = _two_frame_map()
    m.addPointMatches([0, 1, 2], [6, 7, 8], 9)
    m.addDescriptors([0, 1, 2], np.zeros((3, 64), np.uint8))
    with pytest.raises(ValueError):
        m.cullKeyFrames([(0, [0, 1, 2]), (4, [0]), (9, [0, 1, 2])], 1, 0.0)
    assert m.frameNo == [[5, 9]] * 3 and m.equal_range(0) == []


def test_ceil_threshold_sweep():
    """count > ceil(ratio n), the product in double: n points of which c have
    more than nFrames observations, for every n up to 400."""
    m = CMapCullRef()
    m.addNewPoints(np.zeros((400, 3)), [[0] * 400] * 4, [0, 1, 2, 3])   # 4 observations
    m.addNewPoints(np.zeros((400, 3)), [[0] * 400] * 3, [0, 1, 2])      # 3
    for n in range(0, 401):
        for ratio in (0.9, 0.5, 0.75, 0.25, 0.0, 1.0):
            thr = int(math.ceil(ratio * n))
            for c in {0, max(thr - 1, 0), min(thr, n), min(thr + 1, n), n}:
                pts = list(range(c)) + list(range(400, 400 + n - c))
                assert m.arePointsSeenByAtLeast(pts, 3, ratio) == (c > thr), (n, ratio, c)
    # (for these ratios the double product's ceiling is the exact one up to n = 400)
    for num, den in ((9, 10), (3, 4), (1, 2), (1, 4)):
        for n in range(401):
            assert int(math.ceil(num / den * n)) == -((-num * n) // den), (num, den, n)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_generator_fires_every_rule(seed):
    c = cull_cases.random_history(CMapCullRef(), seed, rounds=8, rate=0.5)
    assert c["size"] and c["score"] and c["rule2"] and c["kf"] and c["doubled"] and c["unlisted"], c
