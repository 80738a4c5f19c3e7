#!/usr/bin/env python3
"""Records the small-path fixtures of tests/test_gpu_rotated_form.py: GPU
solves of problems with at most 127 cameras (C (C + 1) / 2 <= 8192 camera
blocks: plain Schur block order, k_schur_pts, three-pass back substitution).

  small_path_60x3000.npz    scene.generate(60, 3000, views=6, seed=11)
  small_path_127x3000.npz   scene.generate(127, 3000, views=10, seed=11): the
                            last camera count on the small path (128 cameras
                            are 8256 blocks and take the large path)

They were recorded on the commit BEFORE the rotated-point Schur pass and the
one-pass point-major back substitution of large systems went in; the tests
assert byte equality with them, i.e. that work on the large path leaves the
small path's bits alone.  Re-record only for a change that is meant to move
them.

Run on a GPU machine from the repository root:
  python tests/golden/make_small_path.py [OUT_DIR]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

TRACE_FIELDS = ("iteration", "step_is_valid", "step_is_successful", "cost", "cost_change", "gradient_max_norm",
                "step_norm", "relative_decrease", "trust_region_radius")
# fixture name -> (cameras, views)
FIXTURES = {"small_path_60x3000": (60, 6), "small_path_127x3000": (127, 10)}


def solve_small_path(cams=60, views=6):
    import sfm_amd
    from sfm_amd import scene
    s = scene.generate(cams, 3000, views=views, seed=11)
    rot, t, X = s.copy_params()
    sm, tr = sfm_amd.solve(s.uv, s.cam_idx, s.pt_idx, s.K, rot, t, X)
    trace = np.array([[it[k] for k in TRACE_FIELDS] for it in tr], dtype=np.float64).reshape(-1, len(TRACE_FIELDS))
    return {"rot": rot, "t": t, "X": X, "final_cost": np.array([sm.final_cost], dtype=np.float64), "trace": trace}


if __name__ == "__main__":
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden")
    for name, (cams, views) in FIXTURES.items():
        out = os.path.join(out_dir, name + ".npz")
        np.savez(out, **solve_small_path(cams, views))
        print("wrote", out)
