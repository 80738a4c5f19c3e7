"""GPU: the LM loop's drivers leave bit for bit what the commit before the
shared trust-region state machine (sfm_amd/csrc/ba_lm.h) left: trace records,
summary (without the times) and parameters, on every branch scene and the two
rejecting irregular scenes, under the default device loop, SFM_LM_UNFUSED=1 and
SFM_HOST_LM=1, and on a two-rank solve through the host all-reduce hook
(tests/lm_loop_cases.py; recorded by tests/golden/make_lm_loop_parent.py into
tests/golden/lm_loop_parent.json)."""
import pytest

import lm_loop_cases as LC

pytestmark = pytest.mark.gpu

FIX = LC.load_fixture()


def test_fixture_is_complete():
    keys = {f"{n}/{e}" for n in LC.scene_names() for e in LC.ENVS} | {LC.TWO_RANKS}
    assert set(FIX) == keys
    assert all(v["reproduces"] for v in FIX.values())  # (both recordings of every entry agreed)


@pytest.mark.parametrize("env", sorted(LC.ENVS))
@pytest.mark.parametrize("name", LC.scene_names())
def test_solve_equals_parent_commit(name, env):
    want = FIX[f"{name}/{env}"]
    got = LC.record(name, env)
    assert got["summary"] == want["record"]["summary"]
    assert got["trace"] == want["record"]["trace"]
    assert got["params_sha256"] == want["record"]["params_sha256"]


@pytest.mark.timeout(240)
def test_two_rank_host_comm_solve_equals_parent_commit():
    want = FIX[LC.TWO_RANKS]
    assert want["reproduces"]
    assert LC.record_two_ranks() == want["record"]
