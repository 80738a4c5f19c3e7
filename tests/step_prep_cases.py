"""Seeded scenes for tests/test_gpu_step_prep.py: LM trajectories with
rejected and invalid steps at camera counts where the evaluation also
prepares the coming step (more than 64 cameras; from 128 on the one-pass
back substitution takes the camera step too).  Built like the branch scenes
of tests/lm_cases.py, found by scanning seeds with the oracle.

Shared with tests/golden/make_step_prep.py, which records the oracle's
trajectories and its disagreement with the dense numpy restatement of the
loop (tests/golden/step_prep.json), the scale of the test's tolerances.
"""
from __future__ import annotations

import numpy as np

from sfm_amd import scene

import lm_cases as L


def reject_scene():
    """130 cameras / 400 points / 10 views; the oracle's trajectory is
    A R R R A A A A A A A R (function tolerance)."""
    return scene.generate(130, 400, views=10, seed=L.SEED + 211, pt_sigma=1.0, rot_sigma=0.3, t_sigma=2.0)


def on_axis_scene(n_axis: int = 5):
    """lm_cases.on_axis_scene at 130 cameras: camera 0 (rot = 0, t = (0, 0, 8))
    keeps only observations of points exactly on its optical axis, so its
    rot_z and t_z columns are exactly zero; with min_lm_diagonal = 0 the
    reduced camera matrix has a zero pivot at every radius: invalid steps
    until max_num_consecutive_invalid_steps -> FAILURE."""
    s = scene.generate(130, 400, views=10, seed=L.SEED + 300, pt_sigma=0.05, rot_sigma=0.01, t_sigma=0.05)
    s.rot[0] = 0.0
    s.t[0] = [0.0, 0.0, 8.0]
    cam0 = np.flatnonzero(s.cam_idx == 0)
    keep_pts = np.unique(s.pt_idx[cam0])[:n_axis]
    drop = cam0[~np.isin(s.pt_idx[cam0], keep_pts)]
    keep = np.ones(s.n_obs, bool)
    keep[drop] = False
    s.uv, s.cam_idx, s.pt_idx = s.uv[keep].copy(), s.cam_idx[keep].copy(), s.pt_idx[keep].copy()
    zs = np.linspace(-0.8, 0.8, len(keep_pts))
    for p, z in zip(keep_pts, zs):
        s.X[p] = [0.0, 0.0, z]
    return s


# The camera / point count grid: 65 cameras are the first whose sums do not
# ride in the point pass, 128 / 129 the first with the one-pass back
# substitution, 513 beyond its and the point pass's LDS camera copies; 1, 255,
# 257 and 1025 points are the edges of the 256-thread blocks and of the
# 512- and 1024-thread workgroups that stand for two and four of them.
GRID_CAMS = (65, 128, 129, 513)
GRID_POINTS = (1, 255, 257, 1025)


def grid_scene(cams: int, pts: int):
    return scene.generate(cams, pts, views=10, seed=11)


def cases():
    """name -> (scene builder, options overrides, mode)"""
    return {
        "reject_130": (reject_scene, {}, 2),
        "invalid_130": (on_axis_scene, {"min_lm_diagonal": 0.0}, 2),
    }
