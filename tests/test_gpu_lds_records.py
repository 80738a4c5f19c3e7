"""The camera records that the BA passes keep in LDS changed layout, not
value: k_schur_pairs_rot_pw's blocks lie 528 B apart (512 B put the four
blocks of a 16-byte read's lane group on the same banks), and k_backsub_pm's
record has 38 doubles, 16-B aligned and read by 16-byte loads.
(k_point_eval_lds keeps its 17-double record: an aligned 18-double one
measured slower, profiles/lds_records_ab.txt; its cases stay as controls.)
No arithmetic changed, so every solve must equal, bit for bit, what
tests/golden/make_lds_records_parent.py recorded on the commit before
(tests/golden/lds_records_parent.json): trace, summary and parameters after
at most two LM iterations.

Cases (the maker's CASES): 65, 128, 129 and 512 cameras -- the first
k_point_eval_lds<512, 2>, the first k_schur_pairs_rot_pw / k_backsub_pm sizes
and k_backsub_pm's last --, 128 cameras at 8, 16, 32 and 64 lanes per block,
60 cameras (k_point_eval_lds<64>), 129 cameras on the sorted layouts (the
wave-major streams) and under the host-driven loop, and 513 cameras (the
global-memory point pass and the three-pass back substitution, untouched) as
a control.  The scenes are irregular: see the maker.
"""
import importlib.util
import json
import os

import numpy as np
import pytest

import irregular_cases as IC

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _maker():
    spec = importlib.util.spec_from_file_location("make_lds_records_parent",
                                                  os.path.join(GOLDEN, "make_lds_records_parent.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


M = _maker()
with open(M.FIXTURE) as _f:
    FIX = json.load(_f)


def test_fixture_covers_the_cases():
    assert sorted(FIX) == sorted(M.CASES)
    for case, want in FIX.items():
        assert 1 <= len(want["trace"]) <= 1 + M.MAX_ITERATIONS, case
        assert want["summary"][1] <= M.MAX_ITERATIONS, case


@pytest.mark.parametrize("case", ["c60", "c65", "c128", "c129", "c512", "c513"])
def test_scenes_are_irregular(case):
    s = M.scene(case)
    C, P, _ = M.CASES[case]
    assert (s.n_cams, s.n_pts) == (C, P)
    assert np.bincount(s.cam_idx, minlength=C).min() > 0  # every camera is observed
    assert not s.rot[0].any()  # identity: the first-order flag is taken
    deg = np.bincount(s.pt_idx, minlength=P)
    assert deg.min() >= 1 and deg.max() >= 10
    _, blocks = IC.pair_count_rule(s.cam_idx, s.pt_idx, P)
    sizes = np.array(list(blocks.values()))
    assert np.any(sizes % 8 != 0) and np.any(sizes % 64 != 0)  # pair lists that fill no whole round of lanes
    assert len(blocks) < C * (C + 1) // 2  # empty slots
    if C >= 128:
        assert C * (C + 1) // 2 > IC.K_SCHUR_XCD_MIN_BLOCKS  # the rotated-point pair pass
    assert (C <= IC.K_CAM_PM_MAX) == (case != "c513")


@pytest.mark.parametrize("case", list(M.CASES))
def test_bitwise_the_parent_solve(case):
    got = M.record(case)
    want = FIX[case]
    assert got["trace"] == want["trace"]
    assert got["summary"] == want["summary"]
    assert got["params"] == want["params"]
