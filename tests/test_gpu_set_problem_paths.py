"""Every route through sfm_ba_set_problem (ba_problem.hip) gives the results
recorded before it was split into a host plan and staged passes, bit for bit.

The route a problem takes -- host counts or device validation, small or
sorted layouts, in-line or deferred uv, parameters staged early, staged late
or on the side stream from one of its three enqueue points -- changes its
speed, never its results, so a wrong predicate passes every path-against-path
test.  tests/golden/set_problem_paths.json (make_set_problem_paths.py, which
also defines the scenes: the smallest that reach each route) pins the digests
of evaluate()'s outputs, the solve's trace and the solved parameters per
scene.  Which route a size takes is checked on the CPU (tests/asan, the plan's
literal rows); here the three routes no other test solves against the oracle
get that parity check too.
"""
import importlib.util
import json
import os

import numpy as np
import pytest

import sfm_amd
from tests.test_gpu_scale import _assert_parity, _solve_both

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load_maker():
    spec = importlib.util.spec_from_file_location("make_set_problem_paths",
                                                  os.path.join(GOLDEN, "make_set_problem_paths.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MAKER = _load_maker()
with open(os.path.join(GOLDEN, "set_problem_paths.json")) as _f:
    FIXTURE = json.load(_f)
ORACLE_PARITY = ("sorted_130", "above_stage_44k", "side_params_66k")


@pytest.mark.parametrize("name", list(MAKER.SCENES))
def test_route_gives_the_recorded_bits(name):
    s = MAKER.make_scene(name)
    got, want = MAKER.record(s), FIXTURE[name]
    assert got["n_obs"] == want["n_obs"]
    assert got["evaluate"] == want["evaluate"], name
    assert got["trace"] == want["trace"], name
    assert got["final_cost"] == want["final_cost"], name
    assert got["params"] == want["params"], name
    if name in ORACLE_PARITY:
        _assert_parity(*_solve_both(s))


def test_device_validation_in_line_reports_the_first_bad_observation():
    """44 000 observations: above the stage, below the deferred uv, so
    k_validate sees the indices and uv in one launch.  A bad camera index at
    100 comes before a non-finite uv at 30000; the handle then takes the
    clean scene and solves."""
    s = MAKER.make_scene("above_stage_44k")
    uv, cam = s.uv.copy(), s.cam_idx.copy()
    uv[30000] = np.nan
    cam[100] = s.n_cams
    with sfm_amd.BundleAdjuster() as ba:
        with pytest.raises(sfm_amd.SfmError) as ei:
            ba.set_problem(uv, cam, s.pt_idx, s.K, s.rot, s.t, s.X)
        assert "cam_idx out of range at 100" in str(ei.value)
        ba.set_problem(s.uv, s.cam_idx, s.pt_idx, s.K, s.rot, s.t, s.X)
        sm, _ = ba.solve()
        assert sm.num_iterations > 0
