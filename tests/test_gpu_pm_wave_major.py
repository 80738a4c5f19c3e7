"""The wave-major copy of the point-major observation stream (DevProblem::uv_wm
/ cam_wm / woff, made by set_problem; read by k_point_eval_* and k_backsub_pm)
against the point-major arrays it copies (SFM_PM_WAVE_MAJOR=0): bitwise the
same solve, on both LM loops.

Scenes: 130 cameras (the smallest count on the k_schur_pairs_rot_pw / k_backsub_pm
path), 1 / 63 / 65 / 257 / 1025 points -- one lane, one wave short of full, a
second wave of one lane, a second 256-point block, a second workgroup of
k_backsub_pm<4> -- with 2..12 views per point: 2 + ((p + 189) // 23) % 11, so a
wave of 64 points holds three or four different counts and pads to its
largest, and point 64 (a wave of its own in p65) has two.  A wave of one
point pads 64-fold, so p1 is on the point-major side of the cap by the rule
itself.
`hub_257` gives point 100 a view from every camera that sees it in front: its
wave alone pads past the cap and set_problem keeps the point-major arrays.
`edge_257` raises point 100 from 3 views to 6, the most the cap admits (one
more slot would not fit; checked below from the index arrays).  `rej_257`
starts far from the solution (tests/irregular_cases.py's rejecting noise): five
rejected steps in a row and accepted ones after them, so the stand-alone prep
kernels run.  Every scene is
shuffled and has duplicated (camera, point) keys, as tests/irregular_cases.py's.

Oracle tolerances: tests/test_gpu_rotated_form.py's _assert_parity (1e-9 final
cost, 1e-6 parameters), and the oracle's accept / reject sequence.  Measured:
cost within 1.3e-10, parameters within 2.7e-9 on every scene.
"""
import functools

import numpy as np
import pytest

import irregular_cases as IC
import step_prep_helpers as H
import sfm_amd
from sfm_amd import scene
from oracle import ffi as O

C = 130
VIEWS = 12


def degree_rule(p):
    return 2 + ((p + 189) // 23) % 11


def _build(P, target=None, noise=None, seed=IC.SEED + 31, dups=5):
    """scene.generate(130, P, views=12) with point p keeping the first
    degree_rule(p) of its observations; target = (point, views): that point
    gets views from further cameras (IC.irregular's hub rule) up to `views`
    (None: every camera that sees it in front); `dups` doubled keys; shuffled."""
    s = scene.generate(C, P, views=VIEWS, seed=seed, **(noise or {}))
    rng = np.random.default_rng(5)
    uv, cam, pt = s.uv, s.cam_idx, s.pt_idx
    first = np.searchsorted(pt, pt, side="left")
    keep = np.arange(len(pt)) - first < degree_rule(pt)
    uv, cam, pt = uv[keep], cam[keep], pt[keep]
    if target is not None:
        h, views = target
        cs = np.setdiff1d(np.arange(C), cam[pt == h])
        pc = IC._rotate(s.rot_true[cs], s.X_true[h]) + s.t_true[cs]
        x, y = pc[:, 0] / pc[:, 2], pc[:, 1] / pc[:, 2]
        K = s.K[cs]
        p = np.stack([K[:, 0] * x + K[:, 1] * y + K[:, 2], K[:, 4] * y + K[:, 5]], axis=1)
        p = p + rng.normal(0, 0.5, p.shape)
        ok = np.flatnonzero((pc[:, 2] > 0.5) & (np.abs(p[:, 0]) < 4000) & (np.abs(p[:, 1]) < 4000))
        if views is not None:
            ok = ok[:views - int(np.sum(pt == h))]
        uv = np.vstack([uv, p[ok]])
        cam = np.concatenate([cam, cs[ok].astype(cam.dtype)])
        pt = np.concatenate([pt, np.full(len(ok), h, pt.dtype)])
    dups = min(dups, len(pt) // 8)
    d = rng.choice(len(pt), dups, replace=False)
    uv = np.vstack([uv, uv[d] + rng.normal(0, 0.3, (dups, 2))])
    cam, pt = np.concatenate([cam, cam[d]]), np.concatenate([pt, pt[d]])
    perm = rng.permutation(len(pt))
    s.uv = np.ascontiguousarray(uv[perm], dtype=np.float64)
    s.cam_idx = np.ascontiguousarray(cam[perm], dtype=np.int32)
    s.pt_idx = np.ascontiguousarray(pt[perm], dtype=np.int32)
    return s


def cap(s):
    """(slots, fits, one more slot fits): set_problem's rule, restated from
    hostlayout::wave_major_slots / wave_major_fits (ba_host_layout.h)."""
    deg = np.bincount(s.pt_idx, minlength=s.n_pts)
    n_w = (s.n_pts + 63) // 64
    slots = int(sum(deg[64 * w:64 * w + 64].max() for w in range(n_w)))
    fits = lambda k: 64 * k <= 1.5 * len(s.pt_idx) + 64 * n_w
    return slots, fits(slots), fits(slots + 1)


EDGE_VIEWS = 6  # point 100 of edge_257: the most views the cap admits
_REJ = dict(pt_sigma=1.0, rot_sigma=0.3, t_sigma=2.0)
# name -> (points, target, noise, wave-major expected)
SCENES = {
    "p1": (1, None, None, False),
    "p63": (63, None, None, True),
    "p65": (65, None, None, True),
    "p257": (257, None, None, True),
    "p1025": (1025, None, None, True),
    "hub_257": (257, (100, None), None, False),
    "edge_257": (257, (100, EDGE_VIEWS), None, True),
    "rej_257": (257, None, _REJ, True),
}


@functools.lru_cache(maxsize=None)
def _scene(name):
    P, target, noise, _ = SCENES[name]
    return _build(P, target, noise, seed=IC.SEED + (227 if noise else 31))


@pytest.mark.parametrize("name", list(SCENES))
def test_scenes_are_on_their_side_of_the_cap(name):
    s = _scene(name)
    deg = np.bincount(s.pt_idx, minlength=s.n_pts)
    slots, fits, more_fits = cap(s)
    print(f"{name}: N {len(s.pt_idx)} degrees {deg.min()}..{deg.max()} slots {slots} padded {64 * slots} "
          f"cap {1.5 * len(s.pt_idx) + 64 * ((s.n_pts + 63) // 64):.0f}")
    assert s.n_cams == C and C * (C + 1) // 2 > IC.K_SCHUR_XCD_MIN_BLOCKS and C <= IC.K_CAM_PM_MAX
    assert fits == SCENES[name][3]
    # cameras per point (a doubled key adds a view, not a camera)
    keys = np.unique(s.pt_idx.astype(np.int64) * C + s.cam_idx)
    cams = np.bincount(keys // C, minlength=s.n_pts)
    rest = np.delete(cams, 100) if SCENES[name][1] else cams
    assert 2 <= rest.min() and rest.max() <= VIEWS and len(s.pt_idx) == len(keys) + min(5, len(keys) // 8)
    if name == "hub_257":
        assert cams[100] > 100
    if name == "edge_257":
        assert cams[100] == EDGE_VIEWS and not more_fits


def _solve(s, host, wave_major, monkeypatch):
    if host:
        monkeypatch.setenv("SFM_HOST_LM", "1")
    else:
        monkeypatch.delenv("SFM_HOST_LM", raising=False)
    if wave_major:
        monkeypatch.delenv("SFM_PM_WAVE_MAJOR", raising=False)
    else:
        monkeypatch.setenv("SFM_PM_WAVE_MAJOR", "0")
    r, t, X = s.copy_params()
    sm, tr = sfm_amd.solve(s.uv, s.cam_idx, s.pt_idx, s.K, r, t, X)
    return sm, tr, (r, t, X)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    s = _scene(name)
    r, t, X = s.copy_params()
    sm, tr = O.solve(s.uv, s.cam_idx, s.pt_idx, s.K, r, t, X)
    return sm, tr, (r, t, X)


@pytest.mark.gpu
@pytest.mark.parametrize("host", [False, True], ids=["device_lm", "host_lm"])
@pytest.mark.parametrize("name", list(SCENES))
def test_wave_major_solve_is_bitwise_the_point_major_solve(name, host, monkeypatch):
    s = _scene(name)
    wm = _solve(s, host, True, monkeypatch)
    pm = _solve(s, host, False, monkeypatch)
    H.assert_loops_equal(wm, pm)  # trace, summary counts, final cost, parameters: bitwise
    assert wm[0].initial_cost == pm[0].initial_cost
    sm_o, tr_o, sol_o = _oracle(name)
    seq = H.seq_of(wm[1])
    par = max(H.rel(a, b) for a, b in zip(wm[2], sol_o))
    worst_c = max(abs(a["cost"] - b["cost"]) / b["cost"] for a, b in zip(wm[1], tr_o))
    print(f"{name}: {seq} cost {worst_c:.2e} (1e-9) params {par:.2e} (1e-6)")
    assert seq == H.seq_of(tr_o)
    if name == "rej_257":
        assert "RA" in seq, seq
    assert wm[0].termination_type == sm_o["termination_type"]
    assert wm[0].num_iterations == sm_o["num_iterations"]
    assert abs(wm[0].final_cost - sm_o["final_cost"]) <= 1e-9 * max(sm_o["final_cost"], 1e-300)
    assert par < 1e-6
