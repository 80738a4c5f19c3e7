"""CPU: the fixed-order restatement of the map-point filter
(tests/map_points_ref.py, what the device kernels are pinned to) against the
live loop's numpy form (sfm_amd.live._filter_matches, BLAS products, hypot),
with the triangulation of oracle.pnp_oracle.triangulate_points.

* flags: equal on every scene whose smallest |d - 7| exceeds 1e-6 px (the
  scenes are seeded so that every one does, asserted);
* distances: 1e-9 relative (floor 1e-3 px).  The two forms differ by the
  rounding of a handful of fp64 products, an absolute error of some 1e-13 px
  whatever the distance: measured on these scenes at most 2.6e-10 relative
  (4.4e-10 on the noise-free constructed matches, whose distances sit at the
  floor), the smallest margin to the bound 4.5e-3 px;
* every rule of the filter rejects matches that all the other rules accept."""
import numpy as np
import pytest

import map_points_cases as C
import map_points_ref as ref
from sfm_amd.live import _R, _filter_matches
from sfm_amd.mapping import _rodrigues


class _Pose:
    def __init__(self, rot, t):
        self.rot, self.t = rot, t


def _blas_distances(s):
    """The distances as sfm_amd.live._filter_matches forms them."""
    R0, R1 = _R(s["r0"]), _R(s["r1"])
    R = R1 @ R0.T
    tt = s["t1"] - R @ s["t0"]
    tx = np.array([[0, -tt[2], tt[1]], [tt[2], 0, -tt[0]], [-tt[1], tt[0], 0]])
    Ki = np.linalg.inv(C.K)
    F = Ki.T @ tx @ R @ Ki
    h0 = np.column_stack([s["uv0"], np.ones(len(s["uv0"]))])
    h1 = np.column_stack([s["uv1"], np.ones(len(s["uv1"]))])
    l1, l0 = h0 @ F.T, h1 @ F
    d1 = np.abs((l1 * h1).sum(1)) / np.hypot(l1[:, 0], l1[:, 1])
    d0 = np.abs((l0 * h0).sum(1)) / np.hypot(l0[:, 0], l0[:, 1])
    return d0, d1


def _ref_flags(s, parts=False):
    return ref.filter_matches(s["uv0"], s["uv1"], s["X"], C.K, _rodrigues(s["r0"]), s["t0"], C.K,
                              _rodrigues(s["r1"]), s["t1"], C.MAX_ERR, parts=parts)


@pytest.fixture(scope="module")
def scenes():
    return C.all_scenes()


def test_restatement_equals_the_live_filter(scenes):
    worst, margin_min = 0.0, np.inf
    for s in scenes:
        keep, p = _ref_flags(s, parts=True)
        live = _filter_matches(C.K, _Pose(s["r0"], s["t0"]), _Pose(s["r1"], s["t1"]), s["uv0"], s["uv1"], s["X"],
                               C.MAX_ERR)
        b0, b1 = _blas_distances(s)
        rel = max(float(np.max(np.abs(p["dist0"] - b0) / np.maximum(b0, 1e-3))),
                  float(np.max(np.abs(p["dist1"] - b1) / np.maximum(b1, 1e-3))))
        margin = float(min(np.min(np.abs(p["dist0"] - C.MAX_ERR)), np.min(np.abs(p["dist1"] - C.MAX_ERR))))
        worst, margin_min = max(worst, rel), min(margin_min, margin)
        print(f"{s['name']}: kept {int(keep.sum())} of {len(keep)}, distance rel diff {rel:.2e}, "
              f"margin to the bound {margin:.2e} px")
        assert rel <= 1e-9, s["name"]
        assert margin > 1e-6, f"{s['name']}: a distance within 1e-6 px of the bound (reseed the scene)"
        assert np.array_equal(keep, live), s["name"]
        if len(keep) >= 63:
            assert 0 < keep.sum() < len(keep), s["name"]      # the filter has work to do
    print(f"worst distance rel diff {worst:.2e}, smallest margin {margin_min:.2e} px")


def test_every_rule_rejects_matches_the_others_accept():
    names = ("finite", "z0", "z1", "d0", "d1")
    seen = {k: 0 for k in names}
    for s, want in C.constructed():
        keep, p = _ref_flags(s, parts=True)
        listed = sorted(i for v in want.values() for i in v)
        for rule, idx in want.items():
            for i in idx:
                verdicts = {k: bool(p[k][i]) for k in names}
                assert verdicts == {k: k != rule for k in names}, (s["name"], rule, i, verdicts)
                seen[rule] += 1
        # what was not built to fail is kept (the +-6.99 px shifts among them)
        assert np.flatnonzero(~keep).tolist() == listed, s["name"]
        live = _filter_matches(C.K, _Pose(s["r0"], s["t0"]), _Pose(s["r1"], s["t1"]), s["uv0"], s["uv1"], s["X"],
                               C.MAX_ERR)
        assert np.array_equal(keep, live), s["name"]
    assert seen == {"finite": 2, "z0": 2, "z1": 2, "d0": 2, "d1": 2}


def test_degenerate_pair_keeps_nothing():
    """Two equal poses: R = I, t = 0 exactly, F = 0, every distance NaN."""
    s = C.scene(65, 3)
    I3, z3 = np.eye(3), np.zeros(3)
    keep, p = ref.filter_matches(s["uv0"], s["uv1"], s["X"], C.K, I3, z3, C.K, I3, z3, C.MAX_ERR, parts=True)
    assert not p["F"].any() and np.isnan(p["dist0"]).all() and np.isnan(p["dist1"]).all()
    assert not keep.any()


def test_host_composition_of_the_library_equals_the_restatement():
    """sfm_filter_matches composes F on the host before it touches a device:
    with no matches it needs none, and F9 must be the restatement's, bitwise."""
    from sfm_amd._ffi import SfmError
    from sfm_amd.mapping import filter_matches
    Ks = np.array([[1000.0, 2.5, 640.0], [0.0, 990.0, 360.0], [0.0, 0.0, 1.0]])
    none = np.zeros((0, 2))
    for name in C.POSES:
        r0, t0, r1, t1 = C.pose_pair(name)
        R0, R1 = _rodrigues(r0), _rodrigues(r1)
        for K0, K1 in ((C.K, C.K), (Ks, C.K), (C.K, Ks)):
            keep, F = filter_matches(none, none, np.zeros((0, 3)), K0, R0, t0, K1, R1, t1, C.MAX_ERR, return_F=True)
            want = ref.fundamental_from_poses(K0, R0, t0, K1, R1, t1)
            assert len(keep) == 0 and np.array_equal(F.view(np.uint64), want.view(np.uint64)), name
    r0, t0, r1, t1 = C.pose_pair("lateral")
    bad_K = C.K.copy()
    bad_K[1, 0] = 1e-3                                # not upper triangular: the closed-form inverse does not hold
    for K0, R0, tt in ((bad_K, _rodrigues(r0), t0), (C.K, np.full((3, 3), np.nan), t0), (C.K, _rodrigues(r0), np.full(3, np.inf))):
        with pytest.raises(SfmError) as e:
            filter_matches(none, none, np.zeros((0, 3)), K0, R0, tt, C.K, _rodrigues(r1), t1, C.MAX_ERR)
        assert e.value.code == -22


def test_compose_and_project_agree_with_blas():
    s = C.scene(300, 3)
    R1 = _rodrigues(s["r1"])
    P = ref.compose_P(C.K, R1, s["t1"])
    Pb = C.K @ np.hstack([R1, s["t1"].reshape(3, 1)])
    assert np.max(np.abs(P - Pb) / np.maximum(np.abs(Pb), 1e-3)) < 1e-14
    uv = ref.project(C.K, R1, s["t1"], s["X"])
    Xc = s["X"] @ R1.T + s["t1"]
    uvb = Xc[:, :2] / Xc[:, 2:3] * np.array([C.K[0, 0], C.K[1, 1]]) + C.K[:2, 2]
    assert np.max(np.abs(uv - uvb)) < 1e-8     # px; the triangulated wrong matches reach ~1e5 px
    Ki = ref.inv_K(np.array([[1000.0, 2.5, 640.0], [0.0, 990.0, 360.0], [0.0, 0.0, 1.0]]))
    assert np.max(np.abs(Ki - np.linalg.inv(np.array([[1000.0, 2.5, 640.0], [0.0, 990.0, 360.0], [0.0, 0.0, 1.0]])))) \
        < 1e-15
