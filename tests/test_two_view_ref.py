"""CPU: the restatement of the two-view initialisation (tests/two_view_ref.py)
pinned to geometry, so that the GPU test against it (test_gpu_two_view.py) is
not circular, and the stability conditions of the seeded cases
(tests/two_view_cases.py): no decision of the pipeline sits on a threshold,
so an implementation that agrees to rounding takes the same decisions.

The geometric errors the restatement reaches are recorded in
tests/golden/two_view_ref.json (figures() below wrote them) and asserted at
twice those: the float32 observations alone limit the accuracy to about
1e-5 rad, and RANSAC returns a minimal-sample model without a refit.

Conventions: camera 1 sees x = R X + t, so a plane n.X = d induces
H = K (R + t n^T / d) K^-1 (the sign of t follows the convention)."""
import json
import math
import os

import numpy as np
import pytest

from tests import two_view_ref as T
from tests.two_view_cases import CASES, GENERAL, K, PLANAR, reference, scene

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "two_view_ref.json")
# the option variants test_gpu_two_view.py runs: the same conditions hold for them
VARIANTS = [("n257_out30", dict(f_ransac_threshold=2.5)), ("n65", dict(f_max_iters=1)), ("n600_out60", dict(f_max_iters=5)),
            ("n65", dict(h_ratio=0.05))]
EXPECTED = {"n15": 2, "n65": 2, "n257_out30": 2, "n600_out60": 2, "planar_exact": 1, "planar_noisy": 1,
            "rotation_only": 0}


def _angle(a, b):
    c = float(a @ b) / (np.linalg.norm(a) * np.linalg.norm(b))
    return math.acos(min(1.0, max(-1.0, c)))


def figures(name):
    """the geometric errors of the restatement on a case"""
    s, (r, _) = scene(name), reference(name)
    out = {}
    p0, p1 = s["p0"].astype(np.float64), s["p1"].astype(np.float64)
    if r.model:
        out["rot_rad"] = math.acos(min(1.0, max(-1.0, (np.trace(r.R.T @ s["R"]) - 1) / 2)))
        out["t_dir_rad"] = _angle(r.t, s["t"])
        k = (r.keep == 1) & ~s["outlier"]
        Xs = r.X[k] * np.linalg.norm(s["t"])  # up to the baseline's scale
        out["X_rel"] = float((np.linalg.norm(Xs - s["X"][k], axis=1) / np.linalg.norm(s["X"][k], axis=1)).max())
    if name in GENERAL:
        d0, d1 = T.epi_distances(r.F, p0, p1)
        inl = r.f_mask == 1
        out["epi_px"] = float(max(d0[inl].max(), d1[inl].max()))
    if s["plane"] is not None:
        n, d = s["plane"]
        Ht = K @ (s["R"] + np.outer(s["t"], n) / d) @ np.linalg.inv(K)
        Ht = Ht / Ht[2, 2]
        out["H_rel"] = float(np.abs(r.H - Ht).max() / np.abs(Ht).max())
    if s["outlier"].any():
        m, good = r.f_mask == 1, ~s["outlier"]
        out["mask_false_inliers"] = float((m & ~good).sum() / max(1, m.sum()))  # 1 - precision
        out["mask_missed_inliers"] = float((~m & good).sum() / good.sum())      # 1 - recall
    return out


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CASES))
def test_reference_reaches_its_recorded_accuracy(name):
    fig, gold = figures(name), golden()[name]
    print(name, fig)
    assert set(fig) == set(gold)
    for key, v in fig.items():
        assert v <= 2 * gold[key] + 1e-12, (key, v, gold[key])


def test_reference_chooses_the_expected_models():
    assert {name: reference(name)[0].model for name in CASES} == EXPECTED


def test_noise_free_general_case_recovers_the_motion():
    """x1^T F x0 = 0 on the inliers, R and the direction of t are the truth
    (to what float32 observations and a 7-point model of pixels allow)"""
    fig = figures("n15")
    assert fig["epi_px"] < 1e-3 and fig["rot_rad"] < 1e-4 and fig["t_dir_rad"] < 1e-3 and fig["X_rel"] < 1e-2
    assert reference("n15")[0].f_mask.all()


def test_noise_free_planar_case_recovers_the_homography():
    r = reference("planar_exact")[0]
    fig = figures("planar_exact")
    assert r.model == 1 and fig["H_rel"] < 1e-6
    assert fig["rot_rad"] < 1e-5 and fig["t_dir_rad"] < 1e-4 and fig["X_rel"] < 1e-4


@pytest.mark.parametrize("name", ["n257_out30", "n600_out60"])
def test_mask_separates_the_planted_outliers(name):
    fig = figures(name)
    assert fig["mask_false_inliers"] < 0.1 and fig["mask_missed_inliers"] < 0.15


def _conditions(name, extra):
    s = scene(name)
    o = dict(T.DEFAULTS)
    o.update(s["opts"])
    o.update(extra)
    r, tr = reference(name, **extra)
    d = r.diag
    if len(s["p0"]) < T.MIN_POINTS:
        return
    # no point error of any evaluated model within a relative 1e-9 of the RANSAC threshold
    thr = float(np.float32(o["f_ransac_threshold"] ** 2))
    errs = np.concatenate(tr["errors"]).astype(np.float64)
    errs = errs[np.isfinite(errs)]
    assert np.abs(errs - thr).min() / thr > 1e-9
    # no tie between a model's count and the count it had to beat (accepted or not, so that the
    # order of a subset's roots cannot matter)
    assert not [c for c in tr["counts"] if c[0] == c[1] and c[0] > 6]
    if "r_h" not in d:
        return
    assert abs(d["r_h"] - o["h_ratio"]) > 0.02
    # the float32 rounding of H and F is itself a threshold: no element of the double H within
    # 0.05 float32 ulp (3e-9 relative) of a rounding boundary, none of F within 0.15 ulp (1e-8) --
    # the small elements of F (1e-7 of F33) come out of a cancellation in the 7-point solve on raw
    # pixels (condition ~1e6), where two correct fp64 implementations agree to ~1e-9..1e-8 only
    assert T.f32_rounding_margin(d["F64"]) > 0.15 and T.f32_rounding_margin(d["H64"]) > 0.05
    if "vote_err" in d:
        ve = d["vote_err"][np.isfinite(d["vote_err"])]
        assert np.abs(ve - o["max_repr_err"]).min() / o["max_repr_err"] > 1e-9
        # the winner clears (or misses) its thresholds by at least one point
        gb, second = d["good_best"], d["second"]
        assert abs(gb - d["need"]) >= 1 and abs(second - o["ambiguity_ratio"] * gb) >= 0.7
        assert abs(d["n_par"] - (gb - gb // 2) + 0.5) >= 1
    if "filter_dist" in d:
        fd = d["filter_dist"][np.isfinite(d["filter_dist"])]
        assert np.abs(fd - o["max_repr_err"]).min() / o["max_repr_err"] > 1e-9


@pytest.mark.parametrize("name,extra", [(n, {}) for n in CASES] + VARIANTS)
def test_case_is_stable(name, extra):
    _conditions(name, extra)


def test_too_few_points_give_no_model():
    p = np.random.default_rng(0).uniform(0, 700, (14, 2)).astype(np.float32)
    r = T.two_view_init(p, p + 3, K, K)
    assert r.model == 0 and r.n_kept == 0


def test_rotation_only_fails_by_parallax():
    d = reference("rotation_only")[0].diag
    assert reference("rotation_only")[0].model == 0
    if "good_best" in d:  # the vote was reached: its winner has (almost) no parallax
        assert d["median_parallax_deg"] < 0.2
