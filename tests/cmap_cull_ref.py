"""CPU restatement of CMap's culling members (TEST INFRASTRUCTURE ONLY: the
checker of the sfm_map_* culling calls, never imported by the product).

Extends oracle.cmap_oracle.CMapOracle, in its style, with the reference's
remaining containers made explicit:

* live: _pts3DIdx, the indices of the points still in the map, ascending
  (CMap.cpp:409-412 keeps it sorted by set_difference);
* timeAlive / kfAlive / ptsViews: _timeAlive, _kfAlive, _ptsViews per point;
* pif: _pointInFrameIdx, the (point, frame) multimap as a list in emplace
  order (one entry per observation, next to every _frameViewsPointIdx
  emplace).

Members:

* addNewPoints (CMap.cpp:36-78): views = the number of frames, ages 0, the
  point joins _pts3DIdx; addPointMatches (CMap.cpp:118-132): views++;
* updatePointViews (CMap.cpp:569-574): views++ per entry, repeats count;
* incrementMapAge (CMap.cpp:561-567): the live points only;
* removePointsThreshold (CMap.cpp:384-404), removePoints (CMap.cpp:406-474),
  removeFrame (CMap.cpp:483-541), arePointsSeenByAtLeast (CMap.cpp:544-558);
* cullKeyFrames: the greedy loop of CSfM::cullKeyFrames (CSfM.cpp:708-752).

Two deliberate departures from the reference:

1. removeFrame erases `_frameNo[p].erase(lower_bound(...))` unchecked: when
   the bisection ends past the list, on an entry of another frame, or on a
   position the point has no descriptor row for, the reference erases a wrong
   entry or runs off the end.  Here these cases raise ValueError and leave
   the map as it was.
2. removePoints leaves a removed point's stale _frameNo / _pts2DIdx /
   _descriptor behind (only the lookup multimaps forget it).  Here they are
   dropped, and a removed point is refused by every member but
   getPointsAtIdx.
"""
from __future__ import annotations

import math

import numpy as np

from oracle.cmap_oracle import CMapOracle


def lower_bound(v, val) -> int:
    """std::lower_bound's bisection as written (first/count halving), on the
    list as it stands: _frameNo[p] is not guaranteed sorted (SURVEY.md
    App. B), so the result is whatever the bisection lands on."""
    first, count = 0, len(v)
    while count > 0:
        step = count // 2
        if v[first + step] < val:
            first += step + 1
            count -= step + 1
        else:
            count = step
    return first


class CMapCullRef(CMapOracle):
    def __init__(self, desc_bytes: int = 64):
        super().__init__(desc_bytes)
        self.live: list[int] = []
        self.timeAlive: list[int] = []
        self.kfAlive: list[int] = []
        self.ptsViews: list[int] = []
        self.pif: list[tuple[int, int]] = []  # _pointInFrameIdx, emplace order

    # ---- bookkeeping next to the base class's appends
    def _need_live(self, pts):
        for p in pts:
            if not (0 <= int(p) < len(self.pts3D)) or not self._is_live(int(p)):
                raise ValueError(f"point {int(p)} is not in the map")

    def _is_live(self, p: int) -> bool:
        i = lower_bound(self.live, p)
        return i < len(self.live) and self.live[i] == p

    def addNewPoints(self, pts3D, pts2DIdx, frameNo):
        out = super().addNewPoints(pts3D, pts2DIdx, frameNo)
        for p in out:
            self.live.append(p)  # (new indices exceed every old one)
            self.timeAlive.append(0)
            self.kfAlive.append(0)
            self.ptsViews.append(len(frameNo))
            for f in frameNo:
                self.pif.append((p, int(f)))
        return out

    def addPointMatches(self, pts3DIdx, pts2DIdx, frameNo):
        self._need_live(pts3DIdx)
        super().addPointMatches(pts3DIdx, pts2DIdx, frameNo)
        for p in pts3DIdx:
            self.ptsViews[int(p)] += 1
            self.pif.append((int(p), int(frameNo)))

    def addDescriptors(self, pts3DIdx, descriptors):
        self._need_live(pts3DIdx)
        super().addDescriptors(pts3DIdx, descriptors)

    def getRepresentativeDescriptors(self, pts3DIdx):
        self._need_live(pts3DIdx)
        return super().getRepresentativeDescriptors(pts3DIdx)

    def updatePointViews(self, pts3DIdx):
        self._need_live(pts3DIdx)
        for p in pts3DIdx:
            self.ptsViews[int(p)] += 1

    def incrementMapAge(self, tIncrement: int, kfIncrement: int):
        for p in self.live:
            self.timeAlive[p] += int(tIncrement)
            self.kfAlive[p] += int(kfIncrement)

    def getNPoints(self) -> int:
        return len(self.live)

    def pointState(self, pts3DIdx):
        """[n][5]: timeAlive, kfAlive, views, observations, live."""
        return np.array([[self.timeAlive[p], self.kfAlive[p], self.ptsViews[p], len(self.frameNo[p]),
                          int(self._is_live(p))] for p in map(int, pts3DIdx)], np.int32).reshape(-1, 5)

    # ---- culling
    def removePointsThreshold(self, kfThreshold: int = 3, trackThreshold=np.float32(0.25)):
        """(culled indices ascending, status [n_pts]: -1 culled, 0 otherwise)."""
        thr = np.float32(trackThreshold)
        cull = []
        for p in self.live:
            n_obs = len(self.frameNo[p])
            kf = self.kfAlive[p]
            if 1 <= kf <= kfThreshold:
                with np.errstate(divide="ignore", invalid="ignore"):
                    # (float)_ptsViews / _timeAlive: the int divisor converts to
                    # float; 0 gives +inf (0 / 0 NaN), neither below the threshold
                    score = np.float32(self.ptsViews[p]) / np.float32(self.timeAlive[p])
                if n_obs < kfThreshold or score < thr:
                    cull.append(p)
            if n_obs < kfThreshold and kf > kfThreshold:
                cull.append(p)
        status = np.zeros(len(self.pts3D), np.int32)
        if cull:
            cull.sort()
            status = self.removePoints(cull)
        return cull, status

    def removePoints(self, ptsCullIdx):
        idx = [int(p) for p in ptsCullIdx]
        if any(b <= a for a, b in zip(idx, idx[1:])):
            raise ValueError("removePoints: the list must be ascending and distinct")
        self._need_live(idx)
        gone = set(idx)
        self.live = [p for p in self.live if p not in gone]
        self.mm = [(f, p) for (f, p) in self.mm if p not in gone]
        self.pif = [(p, f) for (p, f) in self.pif if p not in gone]
        for p in idx:  # departure 2: the stale lists go too
            self.frameNo[p] = []
            self.pts2DIdx[p] = []
            self.descriptor[p] = []
        status = np.zeros(len(self.pts3D), np.int32)
        status[idx] = -1
        return status

    def removeFrame(self, frameNo: int, framePtsIdx):
        frameNo = int(frameNo)
        pts = [int(p) for p in framePtsIdx]
        self._need_live(pts)
        # on copies of the touched lists: nothing changes when an entry raises
        fr, i2, de, dv = {}, {}, {}, {}
        for p in pts:
            if p not in fr:
                fr[p], i2[p], de[p], dv[p] = list(self.frameNo[p]), list(self.pts2DIdx[p]), list(self.descriptor[p]), 0
            pos = lower_bound(fr[p], frameNo)
            if pos >= len(fr[p]) or fr[p][pos] != frameNo or len(de[p]) <= pos:
                raise ValueError(f"removeFrame: frame {frameNo} is not where the bisection ends for point {p}")
            del fr[p][pos], i2[p][pos], de[p][pos]
            dv[p] += 1
        for p in fr:
            self.frameNo[p], self.pts2DIdx[p], self.descriptor[p] = fr[p], i2[p], de[p]
            for _ in range(dv[p]):
                self.pif.remove((p, frameNo))
            self.ptsViews[p] -= dv[p]
        self.mm = [(f, p) for (f, p) in self.mm if f != frameNo]

    def arePointsSeenByAtLeast(self, pts3DIdx, nFramesThreshold: int, ratioPtsThreshold: float) -> bool:
        self._need_live(pts3DIdx)
        ptsThreshold = int(math.ceil(float(ratioPtsThreshold) * len(pts3DIdx)))
        count = sum(1 for p in pts3DIdx if len(self.frameNo[int(p)]) > nFramesThreshold)
        return count > ptsThreshold

    def cullKeyFrames(self, kfs, nFrames: int = 3, ratio: float = 0.9):
        """kfs: [(frameNo, the keyframe's matched points)], oldest first.
        Returns the culled flag per keyframe; the last is never tried."""
        culled = [0] * len(kfs)
        for k in range(len(kfs) - 1):
            f, pts = kfs[k]
            if self.arePointsSeenByAtLeast(pts, nFrames, ratio):
                self.removeFrame(f, pts)
                culled[k] = 1
        return culled
