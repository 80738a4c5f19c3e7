"""k_schur_pairs_rot_pw, the off-diagonal Schur pass of 128 cameras and more:
a wave walks several groups of slots, reading set_problem's slot records and
k_cam_stage_rot's camera records, with the next group's start-up in flight
behind the current group's work.

Every scene is solved at three grids through the test knob SFM_SCHUR_WGS
(read by set_problem): 8 workgroups -- one per list, so every wave walks
dozens of groups: the pipeline's prologue, steady state and drain, empty slots
in the middle and at the end of a list --, 16, and unset (on these scenes most
waves then get one group or none).  Trace and parameters must equal, bit for
bit, the digests tests/golden/make_schur_persistent.py recorded on the commit
before the kernel existed (tests/golden/schur_persistent.json).

Scenes: 128 and 129 cameras (the first that run the kernel); the irregular
scenes of tests/irregular_cases.py (empty blocks, one-pair blocks, hubs,
doubled keys, cameras without observations; irr_100_hub stays on the pass of
small systems); rej_130_irr, whose rejected steps make the device LM loop skip
launches of the pass (gated off) between live ones; 8, 16, 32 and 64 lanes
per block; cameras in the first-order branch of the rotation.
"""
import importlib.util
import json
import os

import pytest

import sfm_amd
from test_gpu_rotated_form import _assert_parity, _solve_oracle

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _maker():
    spec = importlib.util.spec_from_file_location("make_schur_persistent",
                                                  os.path.join(GOLDEN, "make_schur_persistent.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


M = _maker()
with open(M.FIXTURE) as _f:
    FIX = json.load(_f)

WGS = [8, 16, None]
_scenes = {}


def _scene(name):
    if name not in _scenes:
        _scenes[name] = M.SCENES[name][0]()
    return _scenes[name]


def _set_wgs(monkeypatch, wgs):
    if wgs is None:
        monkeypatch.delenv("SFM_SCHUR_WGS", raising=False)
    else:
        monkeypatch.setenv("SFM_SCHUR_WGS", str(wgs))


def test_fixture_covers_the_scenes():
    assert sorted(FIX) == sorted(M.SCENES)
    # rej_130_irr rejects steps (the gated-off launches), the others accept every step
    assert any(it[2] == 0 for it in FIX["rej_130_irr"]["trace"][1:])


@pytest.mark.parametrize("wgs", WGS)
@pytest.mark.parametrize("name", list(M.SCENES))
def test_bitwise_the_recorded_solve_at_every_grid(name, wgs, monkeypatch):
    _set_wgs(monkeypatch, wgs)
    got, _ = M.record(name, _scene(name))
    want = FIX[name]
    assert got["trace"] == want["trace"]
    assert got["final_cost"] == want["final_cost"]
    assert got["params"] == want["params"]


@pytest.mark.parametrize("name,wgs", [("gen_129", 8), ("irr_136", 16)])
def test_matches_oracle(name, wgs, monkeypatch):
    _set_wgs(monkeypatch, wgs)
    s = _scene(name)
    _, g = M.record(name, s)
    _assert_parity(_solve_oracle(s), g)


@pytest.mark.parametrize("name", ["irr_136", "rej_130_irr"])
def test_two_host_loop_solves_of_one_handle(name, monkeypatch):
    # consecutive launches on one handle, by the host-driven loop (bitwise the device loop's)
    _set_wgs(monkeypatch, 8)
    monkeypatch.setenv("SFM_HOST_LM", "1")
    s = _scene(name)
    kw = M.solve_kwargs(name)
    with sfm_amd.BundleAdjuster() as ba:
        ba.set_problem(s.uv, s.cam_idx, s.pt_idx, s.K, s.rot, s.t, s.X)
        out = []
        for _ in range(2):
            sm, tr = ba.solve(**kw)
            out.append(M.digest(sm, tr, ba.parameters()))
            ba.reset()
    assert out[0] == out[1] == FIX[name]


def test_device_loop_twice_with_rejected_steps(monkeypatch):
    # gated-off launches between live ones, then the same again on the same handle
    _set_wgs(monkeypatch, 8)
    monkeypatch.delenv("SFM_HOST_LM", raising=False)
    s = _scene("rej_130_irr")
    kw = M.solve_kwargs("rej_130_irr")
    with sfm_amd.BundleAdjuster() as ba:
        ba.set_problem(s.uv, s.cam_idx, s.pt_idx, s.K, s.rot, s.t, s.X)
        out = []
        for _ in range(2):
            sm, tr = ba.solve(**kw)
            out.append(M.digest(sm, tr, ba.parameters()))
            ba.reset()
    assert out[0] == out[1] == FIX["rej_130_irr"]
