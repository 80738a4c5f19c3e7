"""GPU: the live loop with culling (LiveSfM(cull=True): CSfM::cullMapPoints
and CSfM::cullKeyFrames between the pair loop and the BA, CSfM.cpp:232-252)
on 80 frames of synthetic detector output, every map mutation mirrored into
the restatement tests/cmap_cull_ref.py (cull_cases.Mirror compares every
output of every mirrored call, the cull calls' included)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import ffi as O  # noqa: E402
from cull_cases import Mirror  # noqa: E402
from sfm_amd.live import KeypointStream, LiveSfM  # noqa: E402

pytestmark = pytest.mark.gpu

# thresholdRate of CSfM::cullKeyFrames: the reference's 0.9 does cull in these
# 80 frames (the rule was the largest of {0.9, 0.75, 0.5, 0.25} that does).
# Observed on an MI355X: 0.9 culls keyframe 25 (at frame 65) and 581 of 2212
# points, keyframes left [0, 5, 15, 35, 45, 55, 65, 75]; 0.75 culls 3
# keyframes / 835 points; 0.5 and 0.25 cull 6 / 1319.  Every BA converges.
RATE = 0.9


def _rel(a, b, floor=1e-3):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(np.abs(np.asarray(b)), floor)))


class _Mirrored(LiveSfM):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.map.close()
        self.map = Mirror(self.stream.desc_bytes)
        self.mappings = 0

    def _mapping(self):
        super()._mapping()
        self.mappings += 1
        self.map.check_state()
        for kf in self.kfs:
            # Mirror: the device's answer is the restatement's; and both are the keyframe's own
            p3, p2 = self.map.getPointsInFrame(kf.no)
            assert len(p3) == len(p2) == kf.n_matched(), kf.no
            assert (kf.pt3d[p2] == p3).all(), kf.no
        live = np.zeros(len(self.map.ref.pts3D), bool)
        live[self.map.ref.live] = True
        for f in self.kfs + [self.prev, self._cur]:
            assert live[f.pt3d[f.pt3d >= 0]].all(), f.no


@pytest.fixture(scope="module")
def run80():
    s = _Mirrored(KeypointStream(), cull=True, cull_kf_rate=RATE)
    s.run(80)
    yield s
    s.close()


def test_culling_fires_and_tracking_survives(run80):
    s = run80
    ref = s.map.ref
    print(f"live cull, rate {RATE}: {s.stats}, keyframes {[f.no for f in s.kfs]}, "
          f"{len(ref.pts3D)} points created, {len(ref.live)} live")
    # from the restatement, not the device
    assert len(ref.pts3D) - len(ref.live) >= 1
    kept = {f.no for f in s.kfs}
    culled_kfs = [e["keyframes"] for e in s.cull_log if e["keyframes"]]
    assert culled_kfs and all(not ref.equal_range(f) for fs in culled_kfs for f in fs)
    assert all(ref.equal_range(f) for f in kept)
    assert s.stats["culled_points"] == len(ref.pts3D) - len(ref.live)
    assert s.stats["culled_keyframes"] == sum(len(fs) for fs in culled_kfs)
    assert s.lost == 0 and s.prev.no == 79 and s.stats["tracked"] == 80 - 5 - 1
    assert s.mappings >= 5 and len(s.ba_log) == s.mappings + 1


def test_every_ba_after_culling_matches_the_oracle(run80):
    for rec in run80.ba_log:
        r, t, X = rec["rot"].copy(), rec["t"].copy(), rec["X"].copy()
        sm_o, tr_o = O.solve(rec["uv"], rec["cam_idx"], rec["pt_idx"], rec["K"], r, t, X)
        sm_g, tr_g = rec["summary"], rec["trace"]
        assert sm_g.termination_type == sm_o["termination_type"]
        assert sm_g.num_iterations == sm_o["num_iterations"]
        assert [x["step_is_successful"] for x in tr_g] == [x["step_is_successful"] for x in tr_o]
        # (a NO_CONVERGENCE end would fall under DESIGN.md §3's capped allowances; none occurs in this run)
        assert sm_o["termination_type"] == 0
        assert abs(sm_g.final_cost - sm_o["final_cost"]) <= 1e-9 * max(sm_o["final_cost"], 1e-300)
        assert _rel(rec["X_out"], X) < 1e-6
        assert _rel(rec["t_out"], t) < 1e-6
        assert _rel(rec["rot_out"], r, floor=1e-2) < 1e-6
