"""GPU: the map store's three row tables (observations, points, descriptor
rows; RowTable in sfm_amd/csrc/owner.h) taken to exactly their capacity and
one row past it, twice: the documented growth rule is at least the need, at
least double, a floor of 1024 rows, so the capacities are 1024 and 2048 rows.
After every step Mirror.check_all() re-queries everything against the
restatement (tests/cmap_cull_ref.py); a removePoints of a third of the points
and one cullKeyFrames follow straight after the last growth."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cull_cases import Mirror, _rows  # noqa: E402

pytestmark = pytest.mark.gpu

FLOOR = 1024
# rows after each step: at the first capacity, one past it (the table doubles), at the second, one past it
STEPS = [FLOOR, FLOOR + 1, 2 * FLOOR, 2 * FLOOR + 1]


def _remove_a_third_then_cull(m, rng, n_pts, desc_bytes):
    """Straight after a growth: every third point removed (one compaction of
    all three tables), then a keyframe cull that removes two frames of the
    points 0, 3, 6, ..., which first get four more observations each."""
    group = list(range(0, min(n_pts, 120), 3))
    m.removePoints(list(range(2, n_pts, 3)))
    m.check_all()
    for f in (1, 2, 3, 4):
        m.addPointMatches(group, rng.integers(0, 2000, size=len(group)), f)
        m.addDescriptors(group, _rows(rng, len(group), desc_bytes))
    culled = m.cullKeyFrames([(1, group), (2, group), (4, group)], 3, 0.9)
    assert list(culled) == [1, 1, 0]  # 5 then 4 observations each > 3; the newest keyframe is never tried
    m.check_all()
    assert m.getNPoints() == n_pts - len(range(2, n_pts, 3))


def test_points_and_observations_across_their_capacity():
    """One frame per point, so the point table and the observation table reach
    each capacity in the same call."""
    rng = np.random.default_rng(5)
    m = Mirror(64)
    try:
        n = 0
        for rows in STEPS:
            k = rows - n
            idx = m.addNewPoints(rng.normal(size=(k, 3)), rng.integers(0, 2000, size=(1, k)), [0])
            assert list(idx) == list(range(n, rows))
            n = rows
            assert m.dev.size() == (n, n, 0)
            m.check_all()
        # a descriptor row for frame 0's observation of the points the cull lists
        group = list(range(0, 120, 3))
        m.addDescriptors(group, _rows(rng, len(group), 64))
        _remove_a_third_then_cull(m, rng, n, 64)
    finally:
        m.close()


@pytest.mark.parametrize("desc_bytes", [64, 8])
def test_descriptor_rows_across_their_capacity(desc_bytes):
    rng = np.random.default_rng(desc_bytes)
    n_pts = 64
    m = Mirror(desc_bytes)
    try:
        m.addNewPoints(rng.normal(size=(n_pts, 3)), rng.integers(0, 2000, size=(1, n_pts)), [0])
        n = 0
        for rows in STEPS:
            pts = [(n + i) % n_pts for i in range(rows - n)]  # (every point has a row after the first step)
            m.addDescriptors(pts, _rows(rng, len(pts), desc_bytes))
            n = rows
            assert m.dev.size() == (n_pts, n_pts, n)
            m.check_all()
        _remove_a_third_then_cull(m, rng, n_pts, desc_bytes)
    finally:
        m.close()
