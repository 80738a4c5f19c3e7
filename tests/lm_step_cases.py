"""Scenes for the single-step tests of the bundle adjuster
(tests/test_gpu_lm_step.py against tests/lm_step_ref.py): one on each side of
every boundary of the solve plan (sfm_amd/csrc/ba_plan.h, DESIGN.md "Which
kernel runs when"), at the smallest sizes that reach the variant.

plan() restates plan_problem / plan_solve for one unsharded rank in Python
(as tests/irregular_cases.py restates the setup's bounds);
tests/test_lm_step_ref.py asserts on the CPU that every scene lies on the
side its row of CASES claims, and that the steps chosen from a rejecting
scene's sequence are of the kinds they are chosen for.
"""
from __future__ import annotations

import functools
import json
import os

import numpy as np

from sfm_amd import scene

import irregular_cases as IC
import lm_cases as L

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STRUCT_ONLY, POSE_ONLY, BOTH = 0, 1, 2

# restated from ba_plan.h / chol_kernels.hip (launch_cholesky: up to two 64-wide tiles)
K_ACCEPT_FOLD_MAX_CAMS = 256
K_ACCEPT_FOLD_MAX_X = 3 * 8192
K_CHOL_SMALL_MAX_N = 128


def _irr(C, P):
    return IC.irregular(scene.generate(C, P, views=10, seed=11), seed=5, hubs=IC.HUBS, empty=(7, C - 1), dups=40,
                        shuffle=True, maxdeg=10)


# scene name -> builder
SCENES = {
    "c21": lambda: scene.generate(21, 300, views=4, seed=L.SEED + 21),
    "c22": lambda: scene.generate(22, 300, views=4, seed=L.SEED + 22),
    "wg6": lambda: scene.generate(6, 480, views=6, seed=L.SEED + 6),
    "c64": lambda: scene.generate(64, 500, views=4, seed=L.SEED + 64),
    "c65": lambda: scene.generate(65, 500, views=4, seed=L.SEED + 65),
    "c127": lambda: scene.generate(127, 700, views=4, seed=L.SEED + 127),
    "c128": lambda: scene.generate(128, 700, views=4, seed=L.SEED + 128),
    "c256": lambda: scene.generate(256, 1100, views=4, seed=L.SEED + 256),
    "c257": lambda: scene.generate(257, 1100, views=4, seed=L.SEED + 257),
    "c512": lambda: scene.generate(512, 2100, views=4, seed=L.SEED + 512),
    "c513": lambda: scene.generate(513, 2100, views=4, seed=L.SEED + 513),
    "irr_100": lambda: _irr(100, 900),
    "irr_130": lambda: _irr(130, 600),
    "rej_100_irr": lambda: IC.build("rej_100_irr"),
    "rej_130_irr": lambda: IC.build("rej_130_irr"),
    "reject_a": lambda: L.reject_scene("reject_a"),
}
REJECTING = ("rej_100_irr", "rej_130_irr", "reject_a")


@functools.lru_cache(maxsize=None)
def build(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def recorded_sequence(name):
    """The oracle's recorded accept / reject sequence of a rejecting scene."""
    if name == "reject_a":
        tr = json.load(open(os.path.join(G, "lm_branches.json")))[name]["trace"]
        return IC.seq_of(tr)
    return json.load(open(os.path.join(G, "irregular.json")))[name]["sequence"]


def steps_of(name):
    """Steps 1 and 2; on a rejecting scene also the first rejected step, the
    step after it and the first accepted step that follows a rejected one."""
    if name not in REJECTING:
        return (1, 2)
    seq = recorded_sequence(name)
    r = seq.index("R") + 1
    a = seq.index("RA") + 2
    return tuple(sorted({1, 2, r, r + 1, a}))


# case name -> (scene, mode, environment, what the plan must say)
def _case(scene_name, mode=BOTH, env=None, **expect):
    return (scene_name, mode, dict(env or {}), expect)


CASES = {
    # k_chol_small against the persistent factor
    "c21": _case("c21", chol_small=True, point_pass="Lds64", cam_sums="InPointPass", pair_pass="Pts"),
    "c22": _case("c22", chol_small=False, point_pass="Lds64", cam_sums="InPointPass", pair_pass="Pts"),
    # a workgroup per block, with the diagonal blocks
    "wg6": _case("wg6", pair_pass="WgBlocks", pts_sub=64, prep_folded=False),
    # Lds64 and the camera sums in the point pass end at 64 cameras
    "c64": _case("c64", point_pass="Lds64", cam_sums="InPointPass", prep_folded=False),
    "c65": _case("c65", point_pass="Lds512x2", cam_sums="SumDiag", prep_folded=True, cam_pass="JacObsPrep",
                 small_setup=True),
    # the rotated persistent pair pass and the one-pass back substitution begin at 128
    "c127": _case("c127", pair_pass="Pts", backsub="ThreePass", large=False, prep_folded=True),
    "c128": _case("c128", pair_pass="RotPersistent", backsub="OnePass", large=True, stage_cams=True),
    # the deciding workgroup makes the step current up to 256 cameras
    "c256": _case("c256", lm="DeviceFusedAcceptFold"),
    "c257": _case("c257", lm="DeviceFused"),
    # k_backsub_pm and the LDS point pass end at 512
    "c512": _case("c512", point_pass="Lds512x2", backsub="OnePass", large=True),
    "c513": _case("c513", point_pass="Rc", backsub="ThreePass", large=True, pair_pass="RotPersistent"),
    # irregular visibility
    "irr_100": _case("irr_100", pair_pass="Pts", prep_folded=True, small_setup=False),
    "irr_130": _case("irr_130", pair_pass="RotPersistent", backsub="OnePass"),
    # rejecting scenes
    "rej_100_irr": _case("rej_100_irr", pair_pass="Pts", prep_folded=True),
    "rej_130_irr": _case("rej_130_irr", pair_pass="RotPersistent", prep_folded=True),
    "reject_a": _case("reject_a", cam_sums="InPointPass", chol_small=True),
    # the other modes at <= 64, 65..127 and >= 128 cameras
    "c22_struct": _case("c22", STRUCT_ONLY, cam_sums="None", prep_folded=False),
    "c22_pose": _case("c22", POSE_ONLY, cam_sums="SumFinalize", prep_folded=False),
    "irr_100_struct": _case("irr_100", STRUCT_ONLY, cam_sums="None", prep_folded=False),
    "irr_100_pose": _case("irr_100", POSE_ONLY, cam_sums="SumFinalize", prep_folded=False, backsub="ThreePass"),
    "irr_130_struct": _case("irr_130", STRUCT_ONLY, cam_sums="None", backsub="ThreePass"),
    "irr_130_pose": _case("irr_130", POSE_ONLY, cam_sums="SumFinalize", backsub="ThreePass"),
    # knobs
    "c127_pack": _case("c127", env={"SFM_FORCE_PACK": "1"}, pack_allreduce=True),
    "c65_sorted": _case("c65", env={"SFM_SMALL_SETUP": "0"}, small_setup=False, wave_major=True),
}
# lanes per block of the pair pass
for _s, _pp in (("irr_100", "Pts"), ("irr_130", "RotPersistent")):
    for _sub in (8, 16, 32, 64):
        CASES[f"{_s}_sub{_sub}"] = _case(_s, env={"SFM_SCHUR_PTS_SUB": str(_sub)}, pts_sub=_sub, pair_pass=_pp)


def case_steps():
    """(case, step) of every test: the further steps on the rejecting scenes' own rows only."""
    return [(c, k) for c in CASES for k in (steps_of(c) if c in REJECTING else (1, 2))]


def schur_shape(n_pairs, n_blk, pts_sub_forced, wg_forced):
    """hostlayout::schur_shape (ba_host_layout.h)."""
    avg = n_pairs / n_blk if n_blk else 0.0
    sub = 8
    if pts_sub_forced:
        sub = pts_sub_forced
    else:
        while sub < 64 and sub < avg / 10.0:
            sub *= 2
    wg = sub == 64 and n_blk <= 4 * 256 and avg >= 256.0
    if wg_forced >= 0:
        wg = wg_forced == 1 and sub == 64
    return sub, wg


def plan(s, mode, env):
    """plan_problem and plan_solve of one unsharded rank without a host
    collective, from the scene's index arrays and the SFM_* switches in env."""
    C, P, N = s.n_cams, s.n_pts, s.n_obs
    deg = np.bincount(s.pt_idx, minlength=P).astype(np.int64)
    cdeg = np.bincount(s.cam_idx, minlength=C)
    st = dict(n_obs=N, n_pts=P, camera_chunks=int(np.sum((cdeg + 63) // 64)), max_degree=int(deg.max()))
    assert IC.host_counts(st)            # the host counted: its pair estimate is the plan's
    n_pairs = int(np.sum(deg * (deg - 1) // 2))
    n_blk = C * (C + 1) // 2
    v = env.get("SFM_SCHUR_PTS_SUB")
    forced = 0 if v is None else (int(v) if int(v) in (8, 32, 64) else 16)
    v = env.get("SFM_SCHUR_WG")
    wg_forced = -1 if v is None else (1 if v[0] == "1" else 0)
    p = {}
    p["small_setup"] = env.get("SFM_SMALL_SETUP", "1")[0] != "0" and IC.small_setup_sizes_fit(st, C)
    p["wave_major"] = N > 0 and P > 0 and not p["small_setup"] and env.get("SFM_PM_WAVE_MAJOR", "1")[0] != "0"
    p["pts_sub"], wg = schur_shape(n_pairs, n_blk, forced, wg_forced)
    p["large"] = n_blk > IC.K_SCHUR_XCD_MIN_BLOCKS
    xcd_order = p["large"] and not p["small_setup"]
    pm_backsub = p["large"] and C <= IC.K_CAM_PM_MAX
    both = mode == BOTH
    cams_var, pts_var = mode != STRUCT_ONLY, mode != POSE_ONLY
    fuse = env.get("SFM_HOST_LM", "0")[0] != "1" and env.get("SFM_LM_UNFUSED", "0")[0] != "1"
    fold = fuse and 0 < C <= K_ACCEPT_FOLD_MAX_CAMS and 3 * P <= K_ACCEPT_FOLD_MAX_X \
        and env.get("SFM_NO_ACCEPT_FOLD", "0")[0] != "1"
    p["lm"] = "Host" if env.get("SFM_HOST_LM", "0")[0] == "1" else \
        "DeviceFusedAcceptFold" if fold else "DeviceFused" if fuse else "Device"
    p["prep_folded"] = both and P > 0 and C > 64 and N > 0 and not wg
    split = env.get("SFM_EVAL_SPLIT", "0")[0] == "1"
    p["cam_pass"] = "JacObsPrep" if p["prep_folded"] and not split else "Jacobian"
    in_pp = cams_var and pts_var and P > 0 and 0 < C <= 64
    p["cam_sums"] = "InPointPass" if in_pp else "SumDiag" if p["prep_folded"] else "None" if not cams_var else "SumFinalize"
    g1 = env.get("SFM_PE_GROUPS1", "0")[0] == "1"
    p["point_pass"] = "Lds64" if C <= 64 else "Lds512x2" if C <= 512 and not g1 else "Lds512" if C <= 512 else "Rc"
    p["pair_pass"] = "WgBlocks" if wg else "RotPersistent" if p["large"] else "Pts"
    cam_records = C > 0 and p["large"] and xcd_order and not wg
    p["stage_cams"] = p["cam_pass"] == "JacObsPrep" and cam_records
    p["pack_allreduce"] = env.get("SFM_FORCE_PACK", "0")[0] == "1"
    p["backsub"] = "OnePass" if pm_backsub and cams_var and pts_var and P > 0 and N > 0 else "ThreePass"
    p["chol_small"] = 6 * C <= K_CHOL_SMALL_MAX_N
    p["n_pairs"], p["n_blk"] = n_pairs, n_blk
    return p


ZERO_TOL = dict(function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)


def oracle_step(s, mode, x, radius, threads=1):
    """The oracle restarted at x = (rot, t, X) with the given radius, for one
    iteration (it takes its Jacobi scale at x) -> (trace, x_new)."""
    from oracle import ffi as O
    r, t, X = (np.array(a, np.float64) for a in x)
    o = O.default_options(max_num_iterations=1, initial_trust_region_radius=float(radius), **ZERO_TOL)
    _, tr = O.solve(s.uv, s.cam_idx, s.pt_idx, s.K, r, t, X, mode=mode, options=o, threads=threads)
    return tr, (r, t, X)
