#!/usr/bin/env python3
"""Generates tests/golden/step_prep.json: the oracle's trajectories on the
scenes of tests/step_prep_cases.py, each cross-checked against the dense
numpy restatement of the trust-region loop (make_lm_branches.np_lm), with the
per-iteration disagreement of the two that scales the GPU test's tolerances
(as tests/golden/lm_branches.json does for the branch scenes), and
tests/golden/step_prep_513.npz: the oracle's solves of the 513-camera scenes
of the camera / point count grid.

Run from the repository root:  python tests/golden/make_step_prep.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from make_lm_branches import np_lm, opts_dict, run_oracle, seq_of  # noqa: E402


def main():
    import lm_cases as L
    import step_prep_cases as SP
    from oracle import ffi as O

    out = {}
    for name, (build, spec, mode) in SP.cases().items():
        s = build()
        od = opts_dict(O, **spec)
        sm, tr, (r, t, X) = run_oracle(O, s, mode, od)
        ntr, nterm, nx = np_lm(s.uv, s.cam_idx, s.pt_idx, s.K, s.rot.copy(), s.t.copy(), s.X.copy(), mode, od)
        term = ["CONVERGENCE", "NO_CONVERGENCE", "FAILURE"][sm["termination_type"]]
        assert seq_of(tr) == seq_of(ntr), (name, seq_of(tr), seq_of(ntr))
        assert term == nterm, (name, term, nterm)
        C_, P_ = s.rot.shape[0], s.X.shape[0]
        nxc = nx[:6 * C_].reshape(C_, 6)
        res_fn = lambda *a: O.residuals_jacobians(*a, jacobian=False)[0]
        gi_res, gi_al = L.gauge_invariant_diff(res_fn, s, (r, t, X), (nxc[:, :3], nxc[:, 3:], nx[6 * C_:].reshape(P_, 3)))
        xf = np.concatenate([np.hstack([r, t]).ravel(), X.ravel()])
        out[name] = dict(
            mode=mode, options=od, summary=sm, trace=tr, numpy_termination=nterm,
            numpy_cost_rel_diff=[abs(a["cost"] - b["cost"]) / b["cost"] for a, b in zip(tr, ntr)],
            numpy_radius_rel_diff=[abs(a["trust_region_radius"] - b["trust_region_radius"]) / b["trust_region_radius"]
                                   for a, b in zip(tr, ntr)],
            numpy_param_max_rel=float(np.max(np.abs(xf - nx) / np.maximum(np.abs(nx), 1e-3))),
            numpy_residual_max_abs=gi_res, numpy_aligned_max_rel=gi_al,
            n_obs=int(s.n_obs), n_cams=int(C_), n_pts=int(P_))
        print(f"{name:12s} {term:12s} {seq_of(tr):16s} cost {max(out[name]['numpy_cost_rel_diff']):.1e} "
              f"radius {max(out[name]['numpy_radius_rel_diff']):.1e} params {out[name]['numpy_param_max_rel']:.1e} "
              f"res {gi_res:.1e} aligned {gi_al:.1e}")
    with open(os.path.join(HERE, "step_prep.json"), "w") as f:
        json.dump(out, f, indent=0)
    # the oracle's solves of the 513-camera grid scenes (12 s each on a CPU:
    # recorded, where the smaller grid scenes are solved live by the test)
    arrays = {}
    for pts in SP.GRID_POINTS:
        s = SP.grid_scene(513, pts)
        r, t, X = s.copy_params()
        sm, tr = O.solve(s.uv, s.cam_idx, s.pt_idx, s.K, r, t, X, mode=2)
        k = f"p{pts}__"
        arrays[k + "rot"], arrays[k + "t"], arrays[k + "X"] = r, t, X
        arrays[k + "summary"] = np.array([sm["termination_type"], sm["num_iterations"]], np.int64)
        arrays[k + "final_cost"] = np.array([sm["final_cost"]])
        arrays[k + "successful"] = np.array([it["step_is_successful"] for it in tr], np.int64)
        print(f"513 x {pts}: {seq_of(tr)} final cost {sm['final_cost']:.6e}")
    np.savez_compressed(os.path.join(HERE, "step_prep_513.npz"), **arrays)


if __name__ == "__main__":
    main()
