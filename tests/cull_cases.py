"""Shared culling cases (TEST INFRASTRUCTURE): the pinned hand-checked case
and the seeded history generator, written against the member names the
restatement (tests/cmap_cull_ref.py) and sfm_amd.DeviceMap have in common,
plus Mirror, which drives both at once and compares every output."""
import numpy as np
import pytest

from cmap_cull_ref import CMapCullRef

SFM_EINVAL = -22  # include/sfm_amd.h


def _rows(rng, n, desc_bytes):
    return rng.integers(0, 256, size=(n, desc_bytes), dtype=np.uint8)


def _state(m, pts):
    """[(timeAlive, kfAlive, views, observations)]"""
    return [tuple(int(v) for v in r[:4]) for r in np.asarray(m.pointState(pts))]


def _lists(m, p):
    """a point's (frames, 2D indices) in the restatement; under Mirror the
    device is held to them through pointState and the frame queries"""
    r = m.ref if isinstance(m, Mirror) else m
    return list(r.frameNo[p]), list(r.pts2DIdx[p])


def pinned_case(m, desc_bytes=64):
    """The issue's pinned case, step by step; every expectation is written
    out by hand from CMap.cpp:384-574 / CSfM.cpp:708-752."""
    rng = np.random.default_rng(11)
    chk = getattr(m, "check_all", lambda: None)

    def add_matches(pts, i2, f):
        m.addPointMatches(pts, i2, f)
        m.addDescriptors(pts, _rows(rng, len(pts), desc_bytes))

    # 1. setup
    a = m.addNewPoints(rng.normal(size=(6, 3)), [[10, 11, 12, 13, 14, 15], [20, 21, 22, 23, 24, 25]], [0, 5])
    assert list(a) == [0, 1, 2, 3, 4, 5]
    m.addDescriptors(a, _rows(rng, 6, desc_bytes))
    m.addDescriptors(a, _rows(rng, 6, desc_bytes))
    m.incrementMapAge(0, 2)
    m.updatePointViews([0] * 10 + [2] + [3] * 2 + [4] * 10 + [5] * 10)
    m.incrementMapAge(10, 0)
    add_matches([0, 2, 3, 4, 4, 5], [30, 32, 33, 34, 35, 36], 15)
    b = m.addNewPoints(rng.normal(size=(2, 3)), [[16, 17]], [0])
    assert list(b) == [6, 7]
    m.addDescriptors(b, _rows(rng, 2, desc_bytes))
    add_matches([6], [26], 5)
    add_matches([6, 7], [37, 38], 15)
    assert _state(m, range(8)) == [(10, 2, 13, 3), (10, 2, 2, 2), (10, 2, 4, 3), (10, 2, 5, 3), (10, 2, 14, 4),
                                   (10, 2, 13, 3), (0, 0, 3, 3), (0, 0, 2, 2)]
    assert m.getNPoints() == 8
    chk()

    # 2. first point cull: p1 (kfAlive 2, 2 observations)
    cull, status = m.removePointsThreshold()
    assert list(cull) == [1] and list(status) == [0, -1, 0, 0, 0, 0, 0, 0]
    assert m.getNPoints() == 7 and int(m.pointState([1])[0][4]) == 0
    chk()

    # 3. first keyframe cull: nothing at rate 0.9
    kfs = [(0, [0, 3, 4, 5, 6, 7]), (5, [0, 3, 4, 5, 6]), (15, [0, 3, 4, 4, 5, 6, 7])]
    assert list(m.cullKeyFrames(kfs, 3, 0.9)) == [0, 0, 0]
    chk()
    m.incrementMapAge(0, 1)

    # 4. next keyframe
    m.incrementMapAge(10, 0)
    m.updatePointViews([0, 3, 4, 5, 6] * 10)
    add_matches([0, 3, 4, 5, 6], [40, 43, 44, 45, 46], 25)
    chk()

    # 5. second point cull: p2 by score (4 / 20, 3 observations), p7 by size
    assert _state(m, [2, 7]) == [(20, 3, 4, 3), (10, 1, 2, 2)]
    cull, status = m.removePointsThreshold()
    assert list(cull) == [2, 7] and list(status) == [0, 0, -1, 0, 0, 0, 0, -1]
    chk()

    # 6. second keyframe cull (p6 left out of keyframe 0's list)
    kfs = [(0, [0, 3, 4, 5]), (5, [0, 3, 4, 5, 6]), (15, [0, 3, 4, 4, 5, 6]), (25, [0, 3, 4, 5, 6])]
    assert not m.arePointsSeenByAtLeast(kfs[0][1], 3, 0.9) and m.arePointsSeenByAtLeast(kfs[0][1], 3, 0.5)
    assert list(m.cullKeyFrames(kfs, 3, 0.9)) == [0, 0, 0, 0]
    chk()
    assert list(m.cullKeyFrames(kfs, 3, 0.5)) == [1, 0, 0, 0]
    chk()
    assert _state(m, [0, 4, 6]) == [(20, 3, 23, 3), (20, 3, 24, 4), (10, 1, 14, 4)]
    assert _lists(m, 0) == ([5, 15, 25], [20, 30, 40])
    assert _lists(m, 4) == ([5, 15, 15, 25], [24, 34, 35, 44])
    assert _lists(m, 6) == ([0, 5, 15, 25], [16, 26, 37, 46])
    p3, p2 = m.getPointsInFrame(0)
    assert list(p3) == [] and list(p2) == []
    assert list(m.getPointsInFrames([0])) == []
    p3, p2 = m.getPointsInFrame(15)
    assert list(p3) == [0, 3, 4, 4, 5, 6] and list(p2) == [30, 33, 34, 35, 34, 35, 36, 37]
    # (every 2D index p6 still has, frame by frame: its frame-0 one is out of the multimap's reach)
    assert [list(m.getPointsInFrame(f)[1]) for f in (5, 25)] == [[20, 23, 24, 25, 26], [40, 43, 44, 45, 46]]

    # 7. third keyframe cull
    m.incrementMapAge(0, 1)
    assert list(m.cullKeyFrames(kfs[1:], 2, 0.0)) == [1, 1, 0]
    chk()
    assert _state(m, [0, 3, 4, 5, 6]) == [(20, 4, 21, 1), (20, 4, 13, 1), (20, 4, 21, 1), (20, 4, 21, 1),
                                          (10, 2, 12, 2)]
    assert _lists(m, 6) == ([0, 25], [16, 46])
    for p in (0, 3, 4, 5):
        assert _lists(m, p)[0] == [25]
    p3, p2 = m.getPointsInFrame(25)
    assert list(p3) == [0, 3, 4, 5, 6] and list(p2) == [40, 43, 44, 45, 46]

    # 8. third point cull: p6 by rule 1, the rest by rule 2
    cull, status = m.removePointsThreshold()
    assert list(cull) == [0, 3, 4, 5, 6] and list(status) == [-1, 0, 0, -1, -1, -1, -1, 0]
    assert m.getNPoints() == 0
    for f in (0, 5, 15, 25):
        assert list(m.getPointsInFrame(f)[0]) == []
    assert [int(r[3]) for r in m.pointState(range(8))] == [0] * 8
    chk()

    # 9. error case
    with pytest.raises(ValueError):
        m.removeFrame(15, [0])
    chk()


class Mirror:
    """A DeviceMap and the restatement driven together: every mutation goes
    to both, every output is compared, and check_all() compares every query.
    The restatement's ValueError must be the device's SFM_EINVAL, with the
    store unchanged."""

    def __init__(self, desc_bytes=64):
        import sfm_amd
        self.dev = sfm_amd.DeviceMap(desc_bytes)
        self.ref = CMapCullRef(desc_bytes)
        self.frames = set()

    def close(self):
        self.dev.close()

    def _both(self, name, *args, same=None):
        import sfm_amd
        try:
            r = getattr(self.ref, name)(*args)
        except ValueError:
            with pytest.raises(sfm_amd.SfmError) as e:
                getattr(self.dev, name)(*args)
            assert e.value.code == SFM_EINVAL, e.value
            self.check_all()
            raise
        d = getattr(self.dev, name)(*args)
        if same is not None:
            same(d, r)
        return d

    @staticmethod
    def _eq(d, r):
        assert np.array_equal(np.asarray(d), np.asarray(r)), (d, r)

    def addNewPoints(self, X, i2, fr):
        self.frames.update(int(f) for f in fr)
        return self._both("addNewPoints", X, i2, fr, same=self._eq)

    def addPointMatches(self, pts, i2, f):
        self.frames.add(int(f))
        return self._both("addPointMatches", pts, i2, f)

    def addDescriptors(self, pts, d):
        return self._both("addDescriptors", pts, d)

    def updatePointViews(self, pts):
        return self._both("updatePointViews", pts)

    def incrementMapAge(self, t, k):
        return self._both("incrementMapAge", t, k)

    def getNPoints(self):
        return self._both("getNPoints", same=self._eq)

    def pointState(self, pts):
        return self._both("pointState", list(pts), same=self._eq)

    def getPointsInFrame(self, f):
        return self._both("getPointsInFrame", f, same=lambda d, r: (self._eq(d[0], r[0]), self._eq(d[1], r[1])))

    def getPointsInFrames(self, fr):
        return self._both("getPointsInFrames", fr, same=self._eq)

    def arePointsSeenByAtLeast(self, pts, n, ratio):
        return self._both("arePointsSeenByAtLeast", pts, n, ratio, same=self._eq)

    def removePointsThreshold(self, *a):
        return self._both("removePointsThreshold", *a,
                          same=lambda d, r: (self._eq(d[0], r[0]), self._eq(d[1], r[1])))

    def removePoints(self, pts):
        return self._both("removePoints", pts, same=self._eq)

    def removeFrame(self, f, pts):
        return self._both("removeFrame", f, pts)

    def cullKeyFrames(self, kfs, n=3, ratio=0.9):
        return self._both("cullKeyFrames", kfs, n, ratio, same=self._eq)

    # the rest of DeviceMap as the live loop uses it (queries go to the device)
    def __getattr__(self, name):
        return getattr(self.dev, name)

    def setPointsAtIdx(self, idx, X):
        self.dev.setPointsAtIdx(idx, X)
        for p, x in zip(np.asarray(idx).reshape(-1), np.asarray(X, np.float64).reshape(-1, 3)):
            self.ref.pts3D[int(p)] = x.copy()

    def check_state(self):
        """sizes, the live count and every point's counters"""
        dev, ref = self.dev, self.ref
        P = len(ref.pts3D)
        n_obs = sum(len(f) for f in ref.frameNo)
        n_rows = sum(len(d) for d in ref.descriptor)
        assert dev.size() == (P, n_obs, n_rows), (dev.size(), (P, n_obs, n_rows))
        assert dev.getNPoints() == ref.getNPoints()
        if P:
            self._eq(dev.pointState(range(P)), ref.pointState(range(P)))

    def check_all(self):
        dev, ref = self.dev, self.ref
        P = len(ref.pts3D)
        self.check_state()
        frames = sorted(self.frames) + [max(self.frames, default=0) + 7]
        for f in frames:
            d3, d2 = dev.getPointsInFrame(f)
            r3, r2 = ref.getPointsInFrame(f)
            assert d3.tolist() == r3 and d2.tolist() == r2, f
        for (d3, d2), f in zip(dev.getPointsInFrameMulti(frames[::-1]), frames[::-1]):
            r3, r2 = ref.getPointsInFrame(f)
            assert d3.tolist() == r3 and d2.tolist() == r2, f
        assert dev.getPointsInFrames(frames).tolist() == ref.getPointsInFrames(frames)
        assert dev.getPointsInFrames(frames[:2]).tolist() == ref.getPointsInFrames(frames[:2])
        q = [p for p in ref.live if ref.descriptor[p]]
        if q:
            dd, db = dev.getRepresentativeDescriptors(q, return_best=True)
            rb, rd = ref.getRepresentativeDescriptors(q)
            assert np.array_equal(db, rb) and np.array_equal(dd, rd)
        if P:
            assert np.array_equal(dev.getPointsAtIdx(range(P)), ref.getPointsAtIdx(range(P)))


def random_history(m, seed, rounds, rate, n0=40, n_new=15, desc_bytes=64, check_every_round=True):
    """The issue's generator.  Frame numbers only ever increase, so the
    restatement never raises.  Returns the counts, taken from the
    restatement's state (m.ref, or m itself): culls by rule, keyframes culled,
    doubled and unlisted points."""
    ref = m.ref if isinstance(m, Mirror) else m
    rng = np.random.default_rng(seed)
    counts = dict.fromkeys(("size", "score", "rule2", "kf", "doubled", "unlisted"), 0)
    chk = getattr(m, "check_all", lambda: None)

    def rows(n):
        return _rows(rng, n, desc_bytes)

    kfs = {0: [], 5: []}  # frameNo -> the keyframe's own matched-point list
    a = list(m.addNewPoints(rng.normal(size=(n0, 3)), rng.integers(0, 2000, size=(2, n0)), [0, 5]))
    m.addDescriptors(a, rows(n0))
    m.addDescriptors(a, rows(n0))
    kfs[0] += a
    kfs[5] += a
    m.incrementMapAge(0, 2)
    q = {p: rng.uniform() for p in a}  # per-point visibility
    f = 5
    for _ in range(rounds):
        live = list(ref.live)
        # 10 tracked frames
        views = [p for _ in range(10) for p in live if rng.uniform() < q[p]]
        if views:
            m.updatePointViews(views)
        m.incrementMapAge(10, 0)
        f += 10
        # the new keyframe: each live point with probability q, 5% of them twice
        seen = [p for p in live if rng.uniform() < q[p]]
        twice = [p for p in seen if rng.uniform() < 0.05]
        counts["doubled"] += len(twice)
        lst = sorted(seen + twice)
        kfs[f] = list(lst)
        if lst:
            m.addPointMatches(lst, rng.integers(0, 2000, size=len(lst)), f)
            m.addDescriptors(lst, rows(len(lst)))
        # new points from a random earlier keyframe g0, re-found in the
        # keyframes between with probability 0.5 (a quarter of those left out
        # of that keyframe's own list), then matched in the new keyframe: each
        # point's frames ascend, as in the pinned case's p6 / p7
        older = [g for g in sorted(kfs) if g < f]
        g0 = older[int(rng.integers(0, len(older)))]
        new = list(m.addNewPoints(rng.normal(size=(n_new, 3)), rng.integers(0, 2000, size=(1, n_new)), [g0]))
        m.addDescriptors(new, rows(n_new))
        kfs[g0] += new
        for p in new:
            q[p] = rng.uniform()
        for g in older:
            if g <= g0:
                continue
            found = [p for p in new if rng.uniform() < 0.5]
            if not found:
                continue
            m.addPointMatches(found, rng.integers(0, 2000, size=len(found)), g)
            m.addDescriptors(found, rows(len(found)))
            listed = [p for p in found if rng.uniform() >= 0.25]
            counts["unlisted"] += len(found) - len(listed)
            kfs[g] += listed
        m.addPointMatches(new, rng.integers(0, 2000, size=n_new), f)
        m.addDescriptors(new, rows(n_new))
        kfs[f] += new
        chk()
        # the point cull
        before = {p: (ref.timeAlive[p], ref.kfAlive[p], ref.ptsViews[p], len(ref.frameNo[p])) for p in ref.live}
        cull, _ = m.removePointsThreshold()
        for p in map(int, cull):
            t, kf, v, n = before[p]
            counts["rule2" if kf > 3 else "size" if n < 3 else "score"] += 1
        gone = set(map(int, cull))
        for g in kfs:
            kfs[g] = [p for p in kfs[g] if p not in gone]
        if check_every_round:
            chk()
        # the keyframe cull
        order = sorted(kfs)
        culled = m.cullKeyFrames([(g, kfs[g]) for g in order], 3, rate)
        for g, c in zip(order, culled):
            if c:
                del kfs[g]
                counts["kf"] += 1
        m.incrementMapAge(0, 1)
        chk()
    return counts
